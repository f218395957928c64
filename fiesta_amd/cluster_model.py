"""The definition of fiesta_hip_cluster_voxels (include/fiesta_hip.h) in plain Python / numpy: a dict of voxel -> first entry index
and a breadth-first search.  Slow and obvious on purpose: the device call (fiesta_amd/csrc/cluster_kernels.hpp) has to reproduce
every output of this function bit for bit (member segments as sets)."""
from __future__ import annotations

from collections import deque

import numpy as np

CLUSTER_COORD_LIMIT = 2 ** 20 - 1   # an entry with |c| >= this on any axis is INVALID
CLUSTER_MAX_ENTRIES = 2 ** 24
INT32_MAX = 2 ** 31 - 1


def cluster_stencil(connectivity):
    """the neighbour offsets of connectivity 6 / 18 / 26: at most 1 per axis, at most 1 / 2 / 3 axes changed"""
    if connectivity not in (6, 18, 26):
        raise ValueError("connectivity must be 6, 18 or 26")
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    return [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
            if 0 < (dx != 0) + (dy != 0) + (dz != 0) <= most]


def cluster_model(vox, mask=None, key=None, connectivity=26, min_size=1, resolution=1.0, origin=(0.0, 0.0, 0.0)):
    """vox: (n, 3) integers; mask: (n,) uint8 or None; key: (n,) int32 or None.  Returns a dict: label (n,) int32; per kept cluster
    size, root, box_lo, box_hi, centroid, mask_or, key_min, key_argmin; offsets (K + 1,) and members (sorted inside each segment);
    and the counters of fiesta_hip_cluster_info"""
    v = np.asarray(vox, dtype=np.int64).reshape(-1, 3)
    n = len(v)
    if n > CLUSTER_MAX_ENTRIES:
        raise ValueError("more than 2^24 entries")
    if min_size < 1:
        raise ValueError("min_size must be >= 1")
    stencil = cluster_stencil(connectivity)
    mask = None if mask is None else np.asarray(mask, dtype=np.uint8).reshape(n)
    key = None if key is None else np.asarray(key, dtype=np.int64).reshape(n)
    valid = (np.abs(v) < CLUSTER_COORD_LIMIT).all(axis=1)
    first = {}                                   # voxel -> its representative
    rep_of = np.full(n, -1, np.int64)
    for i in range(n):
        if valid[i]:
            rep_of[i] = first.setdefault((int(v[i, 0]), int(v[i, 1]), int(v[i, 2])), i)
    # components of the representatives, each found from its lowest entry index: its root
    comp = np.full(n, -1, np.int64)              # per representative: its component's root
    comps = []
    for i in range(n):
        if rep_of[i] != i or comp[i] >= 0:
            continue
        comp[i] = i
        todo, cells = deque([i]), [i]
        while todo:
            a = todo.popleft()
            x, y, z = (int(c) for c in v[a])
            for dx, dy, dz in stencil:
                b = first.get((x + dx, y + dy, z + dz))
                if b is not None and comp[b] < 0:
                    comp[b] = i
                    todo.append(b)
                    cells.append(b)
        comps.append((i, sorted(cells)))
    kept = [(root, cells) for root, cells in comps if len(cells) >= min_size]     # (already in increasing root order)
    K = len(kept)
    ident = {root: k for k, (root, _) in enumerate(kept)}
    label = np.full(n, -1, np.int32)
    for i in range(n):
        if valid[i]:
            label[i] = ident.get(int(comp[rep_of[i]]), -1)
    res = float(resolution)
    org = [float(c) for c in origin]
    out = {"label": label, "size": np.zeros(K, np.int32), "root": np.zeros(K, np.int64), "box_lo": np.zeros((K, 3), np.int32),
           "box_hi": np.zeros((K, 3), np.int32), "centroid": np.zeros((K, 3), np.float64), "mask_or": np.zeros(K, np.uint8),
           "key_min": np.full(K, INT32_MAX, np.int32), "key_argmin": np.full(K, -1, np.int64), "offsets": np.zeros(K + 1, np.int64)}
    members = []
    for k, (root, cells) in enumerate(kept):
        c = v[cells]
        size = len(cells)
        out["size"][k], out["root"][k] = size, root
        out["box_lo"][k], out["box_hi"][k] = c.min(axis=0), c.max(axis=0)
        for a in range(3):
            s = int(c[:, a].sum())               # exact
            out["centroid"][k, a] = (float(s) / float(size) + 0.5) * res + org[a]
        if mask is not None:
            out["mask_or"][k] = np.bitwise_or.reduce(mask[cells])
        if key is not None:
            best = None
            for i in cells:                      # (increasing index: the first to attain the minimum stays)
                if key[i] >= 0 and (best is None or key[i] < key[best]):
                    best = i
            if best is not None:
                out["key_min"][k], out["key_argmin"][k] = key[best], best
        members.extend(cells)
        out["offsets"][k + 1] = len(members)
    out["members"] = np.asarray(members, np.int64).reshape(-1)
    out["n_clusters"] = K
    out["n_members"] = len(members)
    out["n_invalid"] = int((~valid).sum())
    out["n_duplicates"] = int((valid & (rep_of != np.arange(n))).sum())
    out["n_dropped_clusters"] = len(comps) - K
    out["largest"] = max((len(cells) for _, cells in kept), default=0)
    return out
