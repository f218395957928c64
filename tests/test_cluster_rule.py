"""The rule of fiesta_hip_cluster_voxels on the CPU: fiesta_amd.cluster_model (the definition the device call has to reproduce bit for
bit) against a literal flood-fill loop and against scipy.ndimage.label, the numbering / min_size / key rules, the whole-call errors
(they need no device), and the resource usage of the built kernels."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 2 ** 20 - 1
I32_MAX = 2 ** 31 - 1


def literal_clusters(vox, connectivity):
    """the definition once more, as literally as it can be said: a set of distinct valid voxels, repeated passes that merge the
    label sets of adjacent voxels until nothing changes.  Returns {frozenset of voxels}"""
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    cells = {tuple(int(c) for c in v) for v in vox if all(abs(int(c)) < LIMIT for c in v)}
    lab = {c: i for i, c in enumerate(sorted(cells))}
    changed = True
    while changed:
        changed = False
        for a in cells:
            for b in cells:
                d = [abs(p - q) for p, q in zip(a, b)]
                if max(d) == 1 and sum(d) <= most and lab[a] != lab[b]:
                    lab[a] = lab[b] = min(lab[a], lab[b])
                    changed = True
    groups = {}
    for c, l in lab.items():
        groups.setdefault(l, set()).add(c)
    return {frozenset(g) for g in groups.values()}


def model_partition(vox, out):
    """{frozenset of voxels} of the model's kept clusters, through members / offsets"""
    got = set()
    for k in range(out["n_clusters"]):
        seg = out["members"][out["offsets"][k]:out["offsets"][k + 1]]
        got.add(frozenset(tuple(int(c) for c in vox[i]) for i in seg))
    return got


def random_list(rng, n, span, shift):
    vox = rng.integers(-span, span + 1, (n, 3)) + shift
    vox = np.concatenate([vox, vox[rng.integers(0, n, n // 4)]])                     # duplicates
    bad = np.array([[LIMIT, 0, 0], [0, -LIMIT, 0], [1, 2, -2 ** 31], [2 ** 31 - 1, 0, 0]])
    vox = np.concatenate([vox, bad])
    return vox[rng.permutation(len(vox))]


@pytest.mark.parametrize("connectivity", (6, 18, 26))
def test_model_against_a_literal_flood_fill(connectivity):
    from fiesta_amd import cluster_model
    rng = np.random.default_rng(5 + connectivity)
    for trial in range(6):
        vox = random_list(rng, 60, 3, np.array([0, -2, 5]) * (trial % 2))
        out = cluster_model(vox, connectivity=connectivity)
        want = literal_clusters(vox, connectivity)
        assert model_partition(vox, out) == want
        assert out["n_invalid"] == 4 and out["n_clusters"] == len(want) and out["n_dropped_clusters"] == 0
        assert sorted(out["size"].tolist()) == sorted(len(g) for g in want)
        valid = (np.abs(vox) < LIMIT).all(axis=1)
        assert (out["label"][~valid] == -1).all() and (out["label"][valid] >= 0).all()
        assert out["n_duplicates"] == int(valid.sum()) - sum(len(g) for g in want) > 0
        assert out["n_members"] == len(out["members"]) == len(set(out["members"].tolist())) == sum(len(g) for g in want)
        # a duplicate carries its voxel's label; roots are the lowest entry of their cluster and number the clusters
        for k in range(out["n_clusters"]):
            idx = np.flatnonzero(out["label"] == k)
            assert idx[0] == out["root"][k]
            seg = out["members"][out["offsets"][k]:out["offsets"][k + 1]]
            assert {tuple(v) for v in vox[idx].tolist()} == {tuple(v) for v in vox[seg].tolist()} and len(seg) == out["size"][k]
        assert (np.diff(out["root"]) > 0).all()


@pytest.mark.parametrize("connectivity,rank", ((6, 1), (18, 2), (26, 3)))
def test_model_against_scipy_label(connectivity, rank):
    from scipy import ndimage
    from fiesta_amd import cluster_model
    rng = np.random.default_rng(40 + connectivity)
    structure = ndimage.generate_binary_structure(3, rank)
    for fill in (0.15, 0.3, 0.5):
        grid = rng.random((9, 8, 7)) < fill
        vox = np.argwhere(grid)
        vox = vox[rng.permutation(len(vox))] - np.array([4, 4, 3])                  # negative coordinates too
        lab, count = ndimage.label(grid, structure=structure)
        out = cluster_model(vox, connectivity=connectivity)
        assert out["n_clusters"] == count
        theirs = lab[tuple((vox + np.array([4, 4, 3])).T)]
        pairs = set(zip(out["label"].tolist(), theirs.tolist()))
        assert len(pairs) == count                                                  # the same partition
        sizes = np.bincount(lab.ravel())[1:]
        for mine, other in pairs:
            assert out["size"][mine] == sizes[other - 1]
        assert out["largest"] == sizes.max()


def test_numbering_min_size_and_statistics():
    from fiesta_amd import cluster_model
    # entry 0: a lone voxel; entries 1, 3: a pair; entries 2, 4, 5, 6: a bar of three with a duplicate (entry 5 repeats entry 2)
    vox = np.array([[10, 0, 0], [0, 0, 0], [-5, 1, 1], [0, 1, 0], [-4, 1, 1], [-5, 1, 1], [-3, 1, 1]])
    mask = np.array([1, 2, 4, 8, 16, 32, 1], np.uint8)
    out = cluster_model(vox, mask=mask, connectivity=6, resolution=0.5, origin=(1.0, -2.0, 0.25))
    assert out["root"].tolist() == [0, 1, 2] and out["size"].tolist() == [1, 2, 3]
    assert out["label"].tolist() == [0, 1, 2, 1, 2, 2, 2]
    assert out["mask_or"].tolist() == [1, 2 | 8, 4 | 16 | 1]                         # the duplicate's 32 counts for nothing
    assert out["box_lo"].tolist() == [[10, 0, 0], [0, 0, 0], [-5, 1, 1]] and out["box_hi"].tolist() == [[10, 0, 0], [0, 1, 0], [-3, 1, 1]]
    assert out["centroid"][2].tolist() == [(-12.0 / 3.0 + 0.5) * 0.5 + 1.0, (3.0 / 3.0 + 0.5) * 0.5 - 2.0, (3.0 / 3.0 + 0.5) * 0.5 + 0.25]
    assert out["offsets"].tolist() == [0, 1, 3, 6] and sorted(out["members"][3:].tolist()) == [2, 4, 6]
    assert (out["n_duplicates"], out["n_invalid"], out["n_dropped_clusters"], out["largest"]) == (1, 0, 0, 3)
    assert (out["key_min"] == I32_MAX).all() and (out["key_argmin"] == -1).all()
    two = cluster_model(vox, mask=mask, connectivity=6, min_size=2)
    assert two["root"].tolist() == [1, 2] and two["label"].tolist() == [-1, 0, 1, 0, 1, 1, 1] and two["n_dropped_clusters"] == 1
    assert two["n_members"] == 5 and two["offsets"].tolist() == [0, 2, 5]
    none = cluster_model(vox, min_size=4)
    assert none["n_clusters"] == 0 and (none["label"] == -1).all() and none["largest"] == 0 and none["n_dropped_clusters"] == 3
    assert none["offsets"].tolist() == [0] and len(none["members"]) == 0
    # (-2, 2, 1) touches the bar across an edge and (-1, 1, 0), which is 6-adjacent to the pair, across a corner
    bridged = np.concatenate([vox, [[-2, 2, 1]], [[-1, 1, 0]], [[-1, 0, 0]]])
    assert cluster_model(bridged, connectivity=6)["n_clusters"] == 4
    assert cluster_model(bridged, connectivity=18)["n_clusters"] == 3
    assert cluster_model(bridged, connectivity=26)["n_clusters"] == 2
    empty = cluster_model(np.zeros((0, 3), np.int32))
    assert empty["n_clusters"] == 0 and empty["offsets"].tolist() == [0]


def test_key_rules():
    from fiesta_amd import cluster_model
    vox = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [2, 0, 0], [9, 9, 9], [20, 0, 0], [21, 0, 0]])
    #                entry 4 repeats entry 2 with a lower key: it counts for nothing
    key = np.array([-1, 7, 5, 5, 1, -3, I32_MAX, I32_MAX], np.int32)
    out = cluster_model(vox, key=key, connectivity=6)
    assert out["root"].tolist() == [0, 5, 6]
    assert out["key_min"].tolist() == [5, I32_MAX, I32_MAX]          # negative keys ignored; INT32_MAX takes part
    assert out["key_argmin"].tolist() == [2, -1, 6]                  # ties: the lowest entry index; none: -1
    with pytest.raises(ValueError):
        cluster_model(vox, connectivity=8)
    with pytest.raises(ValueError):
        cluster_model(vox, min_size=0)


def test_whole_call_errors_need_no_device():
    """every whole-call error is found before the map handle is touched"""
    import __graft_entry__ as g
    g.build_hip()
    import fiesta_amd
    from fiesta_amd._lib import ClusterInfo, ClusterResult
    lib = fiesta_amd.load()
    vox = np.zeros((4, 3), np.int32)
    info, res = ClusterInfo(), ClusterResult()
    info.n_clusters = 77
    p = vox.ctypes.data
    for name, extra in (("fiesta_hip_cluster_voxels", ()), ("fiesta_hip_cluster_voxels_dev", (None,))):
        fn = getattr(lib, name)

        def call(v, n, conn, min_size, ccap, mcap, inf):
            return fn(None, v, None, None, n, *extra, conn, min_size, ccap, mcap, C.byref(res), inf)
        cases = [(p, -1, 26, 1, 0, 0, C.byref(info), "entry count"), (p, 2 ** 24 + 1, 26, 1, 0, 0, C.byref(info), "entry count"),
                 (p, 4, 8, 1, 0, 0, C.byref(info), "connectivity"), (p, 4, 0, 1, 0, 0, C.byref(info), "connectivity"),
                 (p, 4, 26, 0, 0, 0, C.byref(info), "min_size"), (p, 4, 26, 1, -1, 0, C.byref(info), "capacity"),
                 (p, 4, 26, 1, 0, -1, C.byref(info), "capacity"), (None, 4, 26, 1, 0, 0, C.byref(info), "vox is null"),
                 (p, 4, 26, 1, 0, 0, None, "info is null")]
        for v, n, conn, min_size, ccap, mcap, inf, word in cases:
            st = call(v, n, conn, min_size, ccap, mcap, inf)
            assert st == 1, (word, st)                                       # FIESTA_HIP_ERR_INVALID
            assert word in lib.fiesta_hip_last_error().decode(), (word, lib.fiesta_hip_last_error())
    assert info.n_clusters == 77


def test_cluster_kernels_use_no_scratch():
    import sys
    import __graft_entry__ as g
    so = g.build_hip()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources
    res = {k: v for k, v in check_kernel_resources.kernel_resources(so).items() if "k_cluster_" in k}
    # (planner.hip holds the only copy of each; the link pass has one instance per connectivity)
    for kernel, copies in (("k_cluster_init", 1), ("k_cluster_insert", 1), ("k_cluster_seed", 1), ("k_cluster_link", 3), ("k_cluster_flatten", 1),
                           ("k_cluster_number", 1), ("k_cluster_reduce", 1), ("k_cluster_finish", 1)):
        assert sum(kernel in k for k in res) == copies, (kernel, sorted(res))
    for k, v in res.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
