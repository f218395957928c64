"""The definition of fiesta_hip_get_skeleton_voxels (include/fiesta_hip.h) in numpy: the ridge of the distance field between
obstacles, from what a map's dumps report (download_field / download_hash: d2, coc, occ) and GetDistance.  Slow and obvious on
purpose: the device call (fiesta_amd/csrc/skeleton_kernels.hpp) has to reproduce every row of this function exactly."""
from __future__ import annotations

import numpy as np

INT32_MAX = 2 ** 31 - 1
# the mask's bit order: -x, +x, -y, +y, -z, +z (the frontier call's)
SKELETON_NEIGHBOURS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))


def skeleton_model(d2, coc, occ, min_sep2, dist=None, lo=None, hi=None, min_clearance=0.0, origin_vox=(0, 0, 0)):
    """d2 (nx, ny, nz) integers as the dumps report them (-1: never observed, INT32_MAX: observed, no obstacle), coc (nx, ny, nz, 3)
    the closest obstacles in MAP voxel coordinates (read only where a site is defined), occ (nx, ny, nz) occupancy; element (0, 0, 0)
    of the arrays is map voxel `origin_vox`.  site(v) is defined iff 0 <= d2 < INT32_MAX.  For a 6-neighbour n of v inside the array
    with a = site(v), b = site(n) both defined: sep2 = |a - b|^2, g(x) = |x - b|^2 - |x - a|^2, and
        ridge(v, n)  iff  sep2 >= min_sep2 and g(v) >= 0 and g(n) <= 0 and g(v) <= -g(n).
    skeleton(v) iff v is observed and not occupied, site(v) is defined, some neighbour gives a ridge, v lies inside the inclusive
    map-voxel box [lo, hi] (None: everything) and -- only if min_clearance > 0 -- dist >= min_clearance (`dist`: the f64 array of
    GetDistance(Vector3i)).  A neighbour outside the array gives no ridge (a hash-block map is scattered into an array padded by one
    voxel whose absent voxels have d2 = -1).  Returns a dict of rows sorted by (x, y, z): vox (n, 3) int32 in map voxel coordinates,
    mask (n,) uint8, d2 (n,) int32, sep2 (n,) int32: the largest sep2 over the set bits of the mask."""
    d2 = np.asarray(d2, dtype=np.int64)
    if d2.ndim != 3:
        raise ValueError("d2 must be a 3-D array indexed [x, y, z]")
    nx, ny, nz = d2.shape
    coc = np.asarray(coc, dtype=np.int64).reshape(nx, ny, nz, 3)
    occ = np.asarray(occ).reshape(nx, ny, nz).astype(bool)
    if int(min_sep2) != min_sep2 or min_sep2 < 1:
        raise ValueError("min_sep2 must be an integer >= 1")
    if np.isnan(min_clearance):
        raise ValueError("min_clearance is NaN")
    if (lo is None) != (hi is None):
        raise ValueError("lo and hi must both be given or both be None")
    if min_clearance > 0 and dist is None:
        raise ValueError("min_clearance > 0 needs dist")
    org = np.asarray(origin_vox, dtype=np.int64).reshape(3)
    site = (d2 >= 0) & (d2 < INT32_MAX)
    free = (d2 >= 0) & ~occ
    pos = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=-1).astype(np.int64) + org
    a = np.where(site[..., None], coc, 0)          # (undefined sites never enter a result: every use is masked by `site`)

    def sq(u):
        return (u * u).sum(axis=-1)

    mask = np.zeros((nx, ny, nz), np.uint8)
    best = np.zeros((nx, ny, nz), np.int64)
    for bit, (dx, dy, dz) in enumerate(SKELETON_NEIGHBOURS):
        # v: the voxels that have this neighbour inside the array; n: the neighbour
        sv = tuple(slice(max(0, -d), m - max(0, d)) for d, m in ((dx, nx), (dy, ny), (dz, nz)))
        sn = tuple(slice(max(0, d), m - max(0, -d)) for d, m in ((dx, nx), (dy, ny), (dz, nz)))
        av, bn, pv, pn = a[sv], a[sn], pos[sv], pos[sn]
        sep2 = sq(av - bn)
        gv = sq(pv - bn) - sq(pv - av)
        gn = sq(pn - bn) - sq(pn - av)
        ridge = site[sv] & site[sn] & (sep2 >= min_sep2) & (gv >= 0) & (gn <= 0) & (gv <= -gn)
        mask[sv] |= ridge.astype(np.uint8) << bit
        best[sv] = np.maximum(best[sv], np.where(ridge, sep2, 0))
    keep = free & site & (mask != 0)
    if lo is not None:
        blo = np.asarray(lo, dtype=np.int64).reshape(3)
        bhi = np.asarray(hi, dtype=np.int64).reshape(3)
        keep &= ((pos >= blo) & (pos <= bhi)).all(axis=-1)
    if min_clearance > 0:
        keep &= np.asarray(dist, dtype=np.float64).reshape(nx, ny, nz) >= min_clearance
    idx = np.argwhere(keep)                        # (row-major: sorted by x, then y, then z)
    return {"vox": (idx + org).astype(np.int32).reshape(-1, 3), "mask": mask[keep].astype(np.uint8),
            "d2": d2[keep].astype(np.int32), "sep2": best[keep].astype(np.int32)}
