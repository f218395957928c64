"""View coverage on the GPU (fiesta_hip_view_coverage[_dev], include/fiesta_hip.h; kernels: fiesta_amd/csrc/view_kernels.hpp).

The expected result is always fiesta_amd.view_coverage_model (the header's definition in numpy over the plain-Python walk;
tests/test_view_rule.py checks it against a literal restatement over ray_query_model) fed from what the map itself reports through
calls that existed before: download_field / download_hash and GetDistance -- never from the call under test.  Every output is an
integer: all comparisons are exact.  One scene -- a hall with a wall, an unobserved block and an unobserved curtain -- exists as a
dense map with a ragged origin and as a hash-block map at negative coordinates.
"""
import math

import numpy as np
import pytest

from scenarios import P_DEFAULT

pytestmark = pytest.mark.gpu
RES = 0.1
SHAPE = (48, 40, 24)
ORIGIN = {"dense": (-1.03, 0.27, -0.51), "hash": (0.03, -0.02, 0.01)}
SHIFT = {"dense": (0, 0, 0), "hash": (-41, -23, -37)}     # negative coordinates, nothing aligned with the 16 x 16 x 32 tiles
FREE, OCC, UNK, OUT = 0, 1, 2, 4
PER_VIEW, PER_ENTRY, PER_GROUP = ("view_class", "n_in_view", "n_visible"), ("cover_count", "first_view"), ("best_view", "best_count")
TOTALS = ("n_usable", "n_pairs", "pairs_in_view", "pairs_visible")
SENSOR = dict(min_range=0.3, max_range=1.6, tan_h=math.tan(math.radians(40.0)), tan_v=math.tan(math.radians(30.0)), min_clearance=0.15,
              min_visible=3)
ERR_INVALID = 1

# observed-free boxes: a hall around an unobserved block (x 30 .. 37, y 14 .. 25) with an unobserved curtain (x = 41, y 8 .. 31) beyond it
FREE_BOXES = (((2, 2, 2), (29, 37, 21)), ((30, 2, 2), (37, 13, 21)), ((30, 26, 2), (37, 37, 21)), ((38, 2, 2), (40, 37, 21)),
              ((42, 2, 2), (45, 37, 21)), ((41, 2, 2), (41, 7, 21)), ((41, 32, 2), (41, 37, 21)))
WALL = ((24, 10, 2), (24, 29, 17))                        # occupied, between the open hall and the block's -x face


def scene_arrays():
    """the scene as boolean arrays over SHAPE (what the maps must report)"""
    obs, occ = np.zeros(SHAPE, bool), np.zeros(SHAPE, bool)
    for lo, hi in FREE_BOXES:
        obs[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = True
    lo, hi = WALL
    occ[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = True
    return obs, occ


def scene_targets(frontier):
    """targets and groups out of the scene's frontier voxels (scene coordinates, sorted): every second voxel around the block and the
    curtain, grouped by the face they lie on; members permuted, one member out of range on either side, one group empty.
    Returns vox (n, 3), offsets, members"""
    f = frontier[(frontier[:, 0] >= 26) & (frontier[:, 2] >= 6) & (frontier[:, 2] <= 15)]
    x, y = f[:, 0], f[:, 1]
    inner = (y >= 12) & (y <= 27)
    faces = [(x == 29) & inner, (x == 38) & inner, (y == 13) & (x >= 30) & (x <= 37), (y == 26) & (x >= 30) & (x <= 37), (x == 42) & inner]
    rng = np.random.RandomState(3)
    vox, offsets, members = [], [0], []
    for k, sel in enumerate(faces):
        part = f[sel][::2]
        if k == 4:
            part = np.concatenate([part, [[33, 20, 10]]])          # inside the unobserved block: nobody sees it past unknown voxels
        idx = len(np.concatenate(vox)) if vox else 0
        vox.append(part)
        mem = idx + rng.permutation(len(part))
        if k == 1:
            mem = np.concatenate([mem[:7], [-1, 10 ** 6], mem[7:]])
        members.append(mem)
        offsets.append(offsets[-1] + len(mem))
        if k == 2:
            offsets.append(offsets[-1])                   # an empty group
    return np.concatenate(vox).astype(np.int32), np.array(offsets, np.int64), np.concatenate(members).astype(np.int64)


def scene_views(origin, shift, vox, offsets, members):
    """a ring of 3 radii x 8 angles around every group's mean member centre, then views that are unusable for every reason"""
    from fiesta_amd import view_ring
    ring = view_ring([0.6, 1.2, 2.0], 8, [0.05])
    org = np.asarray(origin, np.float64)
    pos, dirs, group = [], [], []
    for g in range(len(offsets) - 1):
        mem = members[offsets[g]:offsets[g + 1]]
        mem = mem[(mem >= 0) & (mem < len(vox))]
        c = (vox[mem].mean(0) + 0.5) * RES + org if len(mem) else org + (np.asarray(shift) + 10.5) * RES
        pos.append(c + ring[:, :3]), dirs.append(ring[:, 3:]), group.append(np.full(len(ring), g))
    s = np.asarray(shift)
    special = [((24, 20, 10), 0), ((33, 20, 10), 0), ((23, 20, 10), 0), ((60, 20, 10), 1), ((10, 20, 10), 9), ((10, 20, 10), -1),
               ((20, 20, 10), 0)]                          # in the wall, in the block, next to the wall, far outside, bad groups, a good one
    pos.append(org + (np.array([v for v, _ in special]) + s + 0.5) * RES), dirs.append(np.tile([1.0, 0.0], (len(special), 1)))
    group.append(np.array([g for _, g in special]))
    pos = np.concatenate(pos)
    pos[5] = np.nan                                       # a NaN position among the ring views
    return pos, np.concatenate(dirs), np.concatenate(group).astype(np.int32)


class Scene:
    """a map of either kind, what it reports of itself, the targets and views; every expectation computed once, left unchanged"""

    def __init__(self, kind):
        import fiesta_amd
        from fiesta_amd import frontier_model
        self.kind, self.origin, self.shift = kind, ORIGIN[kind], np.asarray(SHIFT[kind], np.int32)
        if kind == "dense":
            self.m = fiesta_amd.ESDFMap(self.origin, RES, tuple((s - 0.5) * RES for s in SHAPE))
            assert self.m.grid_size == SHAPE
        else:
            self.m = fiesta_amd.ESDFMap(self.origin, RES, reserve_size=100000, mode="hash")
        fill(self.m, self.shift)
        self.load_model_arrays()
        obs, occ = scene_arrays()
        frontier, _ = frontier_model(obs, occ)
        self.vox, self.offsets, self.members = scene_targets(frontier)
        self.vox = np.ascontiguousarray(self.vox + self.shift)
        self.pos, self.dir, self.group = scene_views(self.origin, self.shift, self.vox, self.offsets, self.members)
        self.cache, self.memo = {}, {}

    def load_model_arrays(self):
        m = self.m
        if self.kind == "dense":
            f = m.download_field(("d2", "occ"))
            self.obs, self.occ = (f["d2"] >= 0).reshape(SHAPE), f["occ"].reshape(SHAPE) != 0
            self.ov, self.bounded, self.pos_range = np.zeros(3, np.int64), True, m.pos_range
            obs, occ = scene_arrays()
            assert np.array_equal(self.obs, obs) and np.array_equal(self.occ, occ)
        else:
            h = m.download_hash()
            self.ov = h["vox"].min(0).astype(np.int64) - 1
            shape = tuple(int(v) for v in (h["vox"].max(0) - self.ov + 2))
            i = tuple((h["vox"] - self.ov).T)
            self.obs, self.occ = np.zeros(shape, bool), np.zeros(shape, bool)
            self.obs[i], self.occ[i] = h["d2"] >= 0, h["occ"] != 0
            self.bounded, self.pos_range = False, None
        all_vox = (np.argwhere(np.ones(self.obs.shape, bool)) + self.ov).astype(np.int32)
        self.dist = m.GetDistance(all_vox).reshape(self.obs.shape)

    def model(self, vox=None, **kw):
        from fiesta_amd import view_coverage_model
        args = dict(SENSOR, block_mask=3)
        args.update(kw)
        return view_coverage_model(self.obs, self.occ, self.origin, RES, self.vox if vox is None else vox, dist=self.dist, origin_vox=self.ov,
                                   bounded=self.bounded, pos_range=self.pos_range, walk_cache=self.cache, **args)

    def main(self, block_mask=3, **kw):
        """the main case: every view against its group"""
        key = (block_mask, tuple(sorted(kw.items())))
        if key not in self.memo:
            self.memo[key] = self.model(pos=self.pos, dir=self.dir, group=self.group, offsets=self.offsets, members=self.members,
                                        block_mask=block_mask, **kw)
        return self.memo[key]

    def call(self, vox=None, **kw):
        args = dict(SENSOR, block_mask=3)
        args.update(kw)
        return self.m.ViewCoverage(self.vox if vox is None else vox, **args)


def fill(m, shift):
    s = np.asarray(shift, np.int32)
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    for lo, hi in FREE_BOXES:
        m.SetOccupancyBox(s + lo, s + hi, 0)
    m.UpdateOccupancy(True)
    m.UpdateESDF()
    lo, hi = WALL
    wall = np.array([(lo[0], y, z) for y in range(lo[1], hi[1] + 1) for z in range(lo[2], hi[2] + 1)], np.int32) + s
    for _ in range(3):                                    # (an obstacle needs three hits to count as occupied)
        m.SetOccupancy(wall, 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()


@pytest.fixture(scope="module")
def scenes(hip_lib):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = Scene(kind)
        return made[kind]
    yield get
    for s in made.values():
        s.m.close()


@pytest.fixture(params=["dense", "hash"])
def scene(request, scenes):
    return scenes(request.param)


def assert_same(got, want, what=""):
    for k in TOTALS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in PER_VIEW + PER_ENTRY + PER_GROUP:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, f"{what}: {k} differs in {len(bad)} places, first {bad[:5].tolist()}: got {g[bad[:5]].tolist()} want {w[bad[:5]].tolist()}"


def test_the_scene_is_not_vacuous(scene):
    """asserted on the MODEL: every way a pair can end holds at least 5 % of the pairs, every reason makes a view unusable"""
    s = scene
    m3, m1 = s.main(3, want_pairs=True), s.main(1, want_pairs=True)
    p3, p1 = m3["pairs"], m1["pairs"]
    n = len(p3)
    assert n == m3["n_pairs"] > 3000 and np.array_equal(p3[:, :4], p1[:, :4])
    listed = p3[:, 1] >= 0
    share = {"range": (listed & (p3[:, 2] == 0)).sum() / n, "field of view": ((p3[:, 2] == 1) & (p3[:, 3] == 0)).sum() / n,
             "occupied": ((p1[:, 3] == 1) & (p1[:, 4] == 0)).sum() / n, "unknown only": ((p1[:, 4] == 1) & (p3[:, 4] == 0)).sum() / n,
             "visible": (p3[:, 4] == 1).sum() / n}
    print(s.kind, {k: round(float(v), 3) for k, v in share.items()}, "pairs", n, "views", len(s.pos), "targets", len(s.vox))
    assert all(v >= 0.05 for v in share.values()), share
    assert (~listed).sum() > 0
    # unusable views: not FREE (occupied, unknown, outside), clearance, group out of range, NaN
    cls, usable = m3["view_class"], m3["n_visible"] >= 0
    no_clear = s.main(3, min_clearance=0.0)["n_visible"] >= 0
    assert {FREE, OCC, UNK} <= set(cls[~usable].tolist()) and (s.kind == "hash" or OUT in cls[~usable])
    assert (no_clear & ~usable).sum() >= 1                                       # usable but for the clearance
    ok_pos = (cls == FREE) & np.isfinite(s.pos).all(1)
    assert (ok_pos & ~no_clear).sum() == 2 and not usable[5] and cls[5] == 0     # the two bad groups; the NaN
    assert (m3["best_view"] >= 0).sum() >= 3 and (m3["best_view"] == -1).sum() >= 1 and m3["n_usable"] > 40
    assert (m3["cover_count"] > 1).any() and (m3["cover_count"] == 0).any()


@pytest.mark.parametrize("block_mask", (0, 1, 3, 7))
def test_every_output_equals_the_model(scene, block_mask):
    s = scene
    got = s.call(pos=s.pos, dir=s.dir, group=s.group, offsets=s.offsets, members=s.members, block_mask=block_mask)
    assert_same(got, s.main(block_mask), f"{s.kind} block_mask {block_mask}")


def test_omni_clearance_and_min_visible(scene):
    s = scene
    kw = dict(pos=s.pos, group=s.group, offsets=s.offsets, members=s.members)
    assert_same(s.call(omni=True, **kw), s.model(omni=True, **kw), "omni, no dir")
    assert_same(s.call(omni=True, dir=s.dir, **kw), s.model(omni=True, **kw), "omni ignores dir")
    for extra in (dict(min_clearance=0.0), dict(min_clearance=0.45), dict(min_visible=1), dict(min_visible=60), dict(tan_h=math.inf, tan_v=0.0),
                  dict(min_range=0.0, max_range=math.inf)):
        assert_same(s.call(dir=s.dir, **kw, **extra), s.model(dir=s.dir, **kw, **extra), str(extra))
    assert s.model(dir=s.dir, min_visible=60, **kw)["best_view"].max() == -1 < s.model(dir=s.dir, min_visible=1, **kw)["best_view"].max()


@pytest.mark.parametrize("size", (0, 1, 63, 64, 65, 255, 257, 1025))
def test_group_sizes_across_wave_tile_and_batch_boundaries(scene, size):
    """one group of `size` members (1025: one above the 1024 pairs of an LDS batch), seen by three views; members repeat the
    scene's targets, so the larger groups list a target more than once"""
    s = scene
    members = (np.arange(size, dtype=np.int64) * 7) % len(s.vox)
    views = [10, 34, 105]                                                       # three usable ring views of different groups
    kw = dict(pos=s.pos[views], dir=s.dir[views], offsets=[0, size], members=members)
    want = s.model(**kw)
    assert_same(s.call(**kw), want, f"group of {size}")
    assert want["n_pairs"] == size * want["n_usable"] and want["n_usable"] >= 2
    if size >= 63:
        assert want["pairs_visible"] > 0


@pytest.mark.parametrize("n_views", (1, 2, 65, 257))
def test_view_counts(scene, n_views):
    s = scene
    idx = (np.arange(n_views) * 5) % len(s.pos)
    kw = dict(pos=s.pos[idx], dir=s.dir[idx], group=s.group[idx], offsets=s.offsets, members=s.members)
    assert_same(s.call(**kw), s.model(**kw), f"{n_views} views")


def test_one_view_past_a_trip_of_the_pair_scan(scene):
    """4097 views: k_view_scan takes kViewScanBlock * kViewScanItems = 4096 pair counts per trip, so the last view's first pair is
    the carry alone, and the total is the carry plus that view's count.  Six groups of 0 .. 3 targets that lie close together (the
    model stays cheap); the views repeat the scene's, the last two are usable ones of groups that have members"""
    s = scene
    n_views = 4097
    sizes = np.array([3, 1, 2, 0, 3, 1])
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    near = np.argsort(np.abs(s.vox - s.vox[40]).sum(1), kind="stable")[:6]
    members = near[np.arange(offsets[-1]) % 6]
    idx = (np.arange(n_views) * 5) % len(s.pos)
    usable = np.flatnonzero((s.main(3)["n_visible"] >= 0) & (sizes[np.clip(s.group, 0, 5)] > 0))
    idx[-2:] = usable[[3, len(usable) // 2]]
    kw = dict(pos=s.pos[idx], dir=s.dir[idx], group=s.group[idx], offsets=offsets, members=members, min_visible=1)
    want = s.model(**kw)
    assert (want["n_visible"][-2:] >= 0).all() and (want["n_visible"] < 0).any() and want["pairs_visible"] > 0
    assert want["n_pairs"] == sizes[s.group[idx][want["n_visible"] >= 0]].sum() > 0
    assert_same(s.call(**kw), want, "4097 views")


def test_many_tiny_groups_share_a_wave(scene):
    """groups of 0 .. 3 members: one wave of the pair kernel serves dozens of views"""
    s = scene
    rng = np.random.RandomState(12)
    sizes = rng.randint(0, 4, 300)
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    near = np.argsort(np.abs(s.vox - s.vox[40]).sum(1))[:60]                     # targets close together, so that views see several groups
    members = near[rng.randint(0, len(near), offsets[-1])]
    idx = rng.randint(0, 48, 300)                                                # views of the first two rings
    kw = dict(pos=s.pos[idx], dir=s.dir[idx], group=np.arange(300, dtype=np.int32), offsets=offsets, members=members, min_visible=1)
    want = s.model(**kw)
    assert_same(s.call(**kw), want, "tiny groups")
    assert want["pairs_visible"] > 20 and (want["best_view"] >= 0).sum() > 10
    # the direct form: no members, offsets cut vox itself; no offsets either: one group of everything
    cut = np.array([0, 10, 10, 200, len(s.vox)])
    kw = dict(pos=s.pos[:48], dir=s.dir[:48], group=(np.arange(48) % 4).astype(np.int32), offsets=cut)
    assert_same(s.call(**kw), s.model(**kw), "offsets without members")
    kw = dict(pos=s.pos[:48], dir=s.dir[:48])
    assert_same(s.call(**kw), s.model(**kw), "neither offsets nor members")
    kw = dict(pos=s.pos[:48], dir=s.dir[:48], members=s.members[:100])
    assert_same(s.call(**kw), s.model(**kw), "members without offsets")


def test_work_groups_that_take_several_batches_carry_their_queue(scene):
    """More pairs than the 2048 work-groups x 1024 pairs of one batch each: a work-group culls three batches, so its queue is
    drained in the middle (a batch of a well-placed view leaves several hundred survivors), pairs are appended behind what a drain
    left over, and the rest goes after the last batch.  24 views that see something, one group whose member list repeats 37 nearby
    targets 7100 times (interleaved, so a wave holds distinct targets); every output against the model, which walks a target once
    per view"""
    s = scene
    good = np.flatnonzero(s.main(3)["n_visible"][:48] > 0)
    views = good[np.arange(24) % len(good)]
    near = np.argsort(np.abs(s.vox - s.vox[40]).sum(1), kind="stable")[:37]
    members = near[(np.arange(37 * 7100) * 5) % 37]
    kw = dict(pos=s.pos[views], dir=s.dir[views], members=members)
    want = s.model(**kw)
    assert want["n_pairs"] > 2 * 2048 * 1024 and want["n_usable"] == 24
    # a drain in mid-course needs 256 survivors out of at most 3072 pairs, left-overs need fewer than all of them
    assert 0.25 < want["pairs_in_view"] / want["n_pairs"] < 0.75 and 0 < want["pairs_visible"] < want["pairs_in_view"]
    assert want["n_in_view"].max() > 0.5 * len(members) and (want["n_in_view"] < 0.1 * len(members)).any()
    assert_same(s.call(**kw), want, "several batches per work-group")
    assert (want["cover_count"] > 7100).any() and (want["first_view"][near] > 0).any() and want["best_count"][0] > 100000


def test_permuted_views_map_through_the_permutation(scene):
    s = scene
    perm = np.random.RandomState(8).permutation(len(s.pos))
    got = s.call(pos=s.pos[perm], dir=s.dir[perm], group=s.group[perm], offsets=s.offsets, members=s.members)
    base = s.main(3)
    for k in PER_VIEW:
        assert np.array_equal(got[k], base[k][perm]), k
    assert np.array_equal(got["cover_count"], base["cover_count"]) and np.array_equal(got["best_count"], base["best_count"])
    for k in TOTALS:
        assert got[k] == base[k]
    # first_view / best_view name the lowest NEW index among the same candidates: the model on the permuted views says which
    assert_same(got, s.model(pos=s.pos[perm], dir=s.dir[perm], group=s.group[perm], offsets=s.offsets, members=s.members), "permuted")
    seen = base["first_view"] >= 0
    assert np.array_equal(got["first_view"] >= 0, seen)
    has = base["best_view"] >= 0
    assert np.array_equal(base["n_visible"][perm][got["best_view"][has]], base["best_count"][has])


def test_a_target_in_the_views_own_voxel_and_bad_inputs(scene):
    s = scene
    org = np.asarray(s.origin)
    here = s.shift + np.array([10, 10, 10], np.int32)
    vox = np.array([here, here + [3, 0, 0], here + [0, 0, 1]], np.int32)
    pos = org + (here + np.array([[0.2, 0.5, 0.5], [0.9, 0.5, 0.5]])) * RES       # behind / ahead of the voxel's centre
    kw = dict(pos=pos, dir=[(1.0, 0.0), (1.0, 0.0)], min_range=0.0, min_clearance=0.0, min_visible=1, tan_v=1.0)
    want = s.model(vox=vox, **kw)
    assert_same(s.call(vox=vox, **kw), want, "own voxel")
    assert want["n_visible"].tolist() == [2, 1] and want["cover_count"].tolist() == [1, 2, 0]
    # bad members, bad groups and a NaN position leave the others alone: the main case without them
    keep = np.ones(len(s.pos), bool)
    keep[[5, len(s.pos) - 3, len(s.pos) - 2]] = False
    good = (s.members >= 0) & (s.members < len(s.vox))
    offsets = np.concatenate([[0], np.cumsum(good)])[s.offsets]
    kw = dict(pos=s.pos[keep], dir=s.dir[keep], group=s.group[keep], offsets=offsets, members=s.members[good])
    clean, base = s.call(**kw), s.main(3)
    for k in ("n_in_view", "n_visible"):
        assert np.array_equal(clean[k], base[k][keep]), k
    assert np.array_equal(clean["cover_count"], base["cover_count"]) and np.array_equal(clean["best_count"], base["best_count"])
    assert clean["n_pairs"] == base["n_pairs"] - 2 * (base["n_visible"][24:48] >= 0).sum() and clean["pairs_visible"] == base["pairs_visible"]


def test_ring_form_equals_the_explicit_form(scene):
    from fiesta_amd import view_ring
    s = scene
    ring = view_ring([0.6, 1.2], 6, [0.0, 0.3])
    G = len(s.offsets) - 1
    org = np.asarray(s.origin)
    cen = org + (s.shift + np.array([[27, 20, 10], [40, 20, 11], [33, 10, 9], [33, 30, 12], [44, 20, 10], [43, 15, 10]]) + 0.37) * RES
    assert len(cen) == G
    kw = dict(offsets=s.offsets, members=s.members)
    got = s.call(centroid=cen, ring=ring, **kw)
    pos = (cen[:, None, :] + ring[None, :, :3]).reshape(-1, 3)
    explicit = s.call(pos=pos, dir=np.tile(ring[:, 3:], (G, 1)), group=np.repeat(np.arange(G), len(ring)).astype(np.int32), **kw)
    assert_same(got, explicit, "ring against explicit")
    assert_same(got, s.model(centroid=cen, ring=ring, **kw), "ring against the model")
    assert got["pairs_visible"] > 100 and len(got["n_visible"]) == G * len(ring)
    empty = s.call(centroid=cen, ring=np.zeros((0, 5)), **kw)
    assert len(empty["n_visible"]) == 0 and empty["best_view"].tolist() == [-1] * G and empty["n_pairs"] == 0


def test_identities_for_no_views_and_no_targets(scene):
    s = scene
    none = s.call(pos=np.zeros((0, 3)), dir=np.zeros((0, 2)), offsets=s.offsets, members=s.members)
    assert none["cover_count"].tolist() == [0] * len(s.vox) and (none["first_view"] == -1).all() and (none["best_view"] == -1).all()
    assert (none["best_count"] == 0).all() and [none[k] for k in TOTALS] == [0, 0, 0, 0]
    got = s.call(vox=np.zeros((0, 3), np.int32), pos=s.pos[:30], dir=s.dir[:30])
    want = s.model(vox=np.zeros((0, 3), np.int32), pos=s.pos[:30], dir=s.dir[:30])
    assert_same(got, want, "no targets")
    assert got["n_pairs"] == 0 and got["n_usable"] > 10 and got["best_view"].tolist() == [-1]


def device_call(s, n_groups_dev=None, ring=None, centroid=None, **kw):
    """the device variant through torch tensors; returns what ViewCoverage returns"""
    import torch
    from fiesta_amd._lib import ViewResult
    from fiesta_amd.esdf_map import VIEW_FIELDS, VIEW_INFO_KEYS
    dev = torch.device("cuda", 0)

    def up(a, dtype):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)
    vox, off, mem = up(s.vox, np.int32), up(s.offsets, np.int64), up(s.members, np.int64)
    G = len(s.offsets) - 1
    if ring is None:
        pos, dirs, grp = up(s.pos, np.float64), up(s.dir, np.float64), up(s.group, np.int32)
        V = len(s.pos)
        form = dict(pos_dev_ptr=pos.data_ptr(), dir_dev_ptr=dirs.data_ptr(), group_dev_ptr=grp.data_ptr(), n_views=V)
    else:
        cen, rg = up(centroid, np.float64), up(ring, np.float64)
        V = G * len(ring)
        form = dict(centroid_dev_ptr=cen.data_ptr(), ring_dev_ptr=rg.data_ptr(), n_ring=len(ring))
    sizes = {"views": V, "entries": len(s.vox), "groups": G}
    out = {name: torch.full((sizes[size] + 3,), 123, dtype=getattr(torch, np.dtype(dtype).name), device=dev) for name, dtype, size in VIEW_FIELDS}
    info = torch.zeros(4, dtype=torch.int64, device=dev)
    gdev = None if n_groups_dev is None else torch.tensor([n_groups_dev], dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    args = dict(SENSOR, block_mask=3)
    args.update(kw)
    s.m.ViewCoverageDevice(vox.data_ptr(), len(s.vox), info.data_ptr(), offsets_dev_ptr=off.data_ptr(), members_dev_ptr=mem.data_ptr(), n_groups=G,
                           n_groups_dev_ptr=0 if gdev is None else gdev.data_ptr(), n_members=len(s.members),
                           out={name: out[name].data_ptr() for name, _ in ViewResult._fields_}, **form, **args)
    s.m.synchronize()
    res = {}
    for name, _, size in VIEW_FIELDS:
        a = out[name].cpu().numpy()
        assert (a[sizes[size]:] == 123).all(), (name, "written past its end")
        res[name] = a[:sizes[size]]
    res.update(zip(VIEW_INFO_KEYS, info.cpu().numpy().tolist()))
    return res


def test_device_variant_and_the_device_group_count(scene):
    s = scene
    assert_same(device_call(s), s.main(3), "device variant")
    G = len(s.offsets) - 1
    for count in (G + 5, 2, 0, -3):
        want = s.model(pos=s.pos, dir=s.dir, group=s.group, offsets=s.offsets, members=s.members, n_groups_effective=count)
        assert_same(device_call(s, n_groups_dev=count), want, f"n_groups_dev {count}")
    assert want["n_usable"] == 0 and len(want["best_view"]) == G
    two = s.model(pos=s.pos, dir=s.dir, group=s.group, offsets=s.offsets, members=s.members, n_groups_effective=2)
    assert 0 < two["n_usable"] < s.main(3)["n_usable"] and (two["best_view"][2:] == -1).all()


def test_visibility_agrees_with_the_ray_query_on_the_same_segments(scene):
    """independent of the model: RayQueryDevice on a sample of (view, target) segments"""
    import torch
    s = scene
    rng = np.random.RandomState(4)
    usable = np.flatnonzero(s.main(3)["n_visible"] >= 0)
    views = usable[rng.randint(0, len(usable), 400)]
    ents = rng.randint(0, len(s.vox), 400)
    org = np.asarray(s.origin)
    start, end = s.pos[views], (s.vox[ents].astype(np.float64) + 0.5) * RES + org
    dev = torch.device("cuda", 0)
    ds, de = torch.from_numpy(start).to(dev), torch.from_numpy(end).to(dev)
    hit, hv = torch.empty(400, dtype=torch.int32, device=dev), torch.empty((400, 3), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    s.m.RayQueryDevice(ds.data_ptr(), de.data_ptr(), 400, stop_mask=3, out={"hit_index": hit.data_ptr(), "hit_vox": hv.data_ptr()})
    s.m.synchronize()
    clear = (hit.cpu().numpy() == -1) | (hv.cpu().numpy() == s.vox[ents]).all(1)
    # one call per pair keeps the answer per pair: a single view, a single target, no cull
    seen = np.array([s.call(vox=s.vox[e:e + 1], pos=s.pos[v:v + 1], omni=True, min_range=0.0, max_range=math.inf, tan_v=math.inf,
                            min_clearance=0.0)["n_visible"][0] for v, e in zip(views[:60], ents[:60])])
    assert np.array_equal(seen == 1, clear[:60]) and 5 < clear[:60].sum() < 55
    # and all 400 in one call: every view its own group of one target
    got = s.call(pos=s.pos[views], group=np.arange(400, dtype=np.int32), offsets=np.arange(401), members=ents, omni=True, min_range=0.0,
                 max_range=math.inf, tan_v=math.inf, min_clearance=0.0)
    q = end - start
    flat = np.hypot(q[:, 0], q[:, 1]) > 0                                         # (straight up or down is in no OMNI cone)
    assert np.array_equal(got["n_visible"][flat] == 1, clear[flat]) and flat.sum() > 390


def test_errors_leave_the_map_usable(scene):
    import fiesta_amd
    s = scene
    kw = dict(pos=s.pos, dir=s.dir, group=s.group, offsets=s.offsets, members=s.members)
    for bad in (dict(block_mask=8), dict(min_visible=0), dict(max_range=0.1), dict(tan_h=-1.0), dict(dir=None), dict(centroid=np.zeros((6, 3)), ring=np.zeros((1, 5)))):
        with pytest.raises(fiesta_amd.FiestaHipError) as e:
            s.call(**dict(kw, **bad))
        assert e.value.code == ERR_INVALID
    assert_same(s.call(**kw), s.main(3), "after the errors")


def test_device_chain_equals_the_host_staged_route(scene):
    from fiesta_amd import view_ring
    s = scene
    ring = view_ring([0.5, 1.0], 8, [0.0])
    sensor = {k: v for k, v in SENSOR.items() if k != "min_clearance"}
    sensor.update(block_mask=3, view_clearance=SENSOR["min_clearance"])
    lo, hi = s.shift + np.array([26, 6, 6], np.int32), s.shift + np.array([44, 33, 15], np.int32)
    for attempt in range(2):                                                     # (the second call reuses the buffers)
        got = s.m.FrontierViews(lo, hi, min_clearance=0.0, connectivity=26, min_size=10, ring=ring, **sensor)
    fv, mask = s.m.GetFrontierVoxels(lo, hi)
    assert len(fv) == len(got["vox"]) > 500 and got["n_clusters"] >= 2
    # the host-staged route on the chain's own list (the frontier call's order is unspecified): clusters, then coverage, call by call
    cl = s.m.ClusterVoxels(got["vox"], mask=got["mask"], connectivity=26, min_size=10)
    for k in ("label", "size", "root", "offsets"):
        assert np.array_equal(cl[k], got[k]), k
    assert np.array_equal(cl["centroid"].view(np.int64), got["centroid"].view(np.int64))
    kw = dict(SENSOR, block_mask=3)
    host = s.m.ViewCoverage(got["vox"], centroid=got["centroid"], ring=ring, offsets=got["offsets"], members=got["members"], **kw)
    for k in PER_VIEW + PER_ENTRY + PER_GROUP + TOTALS:
        assert np.array_equal(got[k], host[k]), k
    want = s.model(vox=got["vox"], centroid=got["centroid"], ring=ring, offsets=got["offsets"], members=got["members"])
    assert_same(host, want, "chain against the model")
    has = got["best_view"] >= 0
    assert has.sum() >= 2 and np.isnan(got["best_pos"][~has]).all()
    assert np.array_equal(got["best_pos"][has], got["view_pos"][got["best_view"][has]]) and got["pairs_visible"] > 100


def test_shard_answers_for_its_own_array(hip_lib):
    import fiesta_amd
    from fiesta_amd import view_coverage_model
    gg = (32, 16, 16)
    m = fiesta_amd.ESDFMap((0, 0, 0), RES, (15.5 * RES,) * 3, shard_lo=(16, 0, 0), global_grid=gg)
    m.SetParameters(*P_DEFAULT)
    m.SetOriginalRange()
    m.SetOccupancyBox((16, 3, 3), (28, 12, 12), 0)
    m.UpdateOccupancy(True)
    for _ in range(3):
        m.SetOccupancy(np.array([[22, y, z] for y in range(5, 10) for z in range(5, 10)], np.int32), 1, want_ret=False)
        m.UpdateOccupancy(True)
    m.UpdateESDF()
    info = m.shard_info()
    lo, dims = np.array(info["local_origin"]), tuple(int(v) for v in info["local_dims"])
    f = m.download_field(("d2", "occ"))
    obs, occ = (f["d2"] >= 0).reshape(dims), f["occ"].reshape(dims) != 0
    rng = np.random.RandomState(6)
    vox = np.stack([rng.randint(10, 31, 80), rng.randint(2, 14, 80), rng.randint(2, 14, 80)], 1).astype(np.int32)
    pos = np.stack([rng.uniform(0.5, 3.1, 40), rng.uniform(0.3, 1.3, 40), rng.uniform(0.3, 1.3, 40)], 1)
    kw = dict(pos=pos, omni=True, tan_v=1.0, max_range=1.5, block_mask=5)
    want = view_coverage_model(obs, occ, (0, 0, 0), RES, vox, origin_vox=lo, pos_range=m.pos_range, **kw)
    got = m.ViewCoverage(vox, **kw)
    assert_same(got, want, "shard")
    assert OUT in want["view_class"] and want["n_usable"] > 5 and 0 < want["pairs_visible"] < want["pairs_in_view"]
    m.close()
