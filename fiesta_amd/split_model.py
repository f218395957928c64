"""The definition of fiesta_hip_split_clusters (include/fiesta_hip.h) in plain Python: a literal recursion that bisects every
oversize part of a cluster at the middle of its box's longest axis.  Slow and obvious on purpose: the device call
(fiesta_amd/csrc/split_kernels.hpp) has to reproduce every output of this function bit for bit (member segments as sets)."""
from __future__ import annotations

import numpy as np

from .cluster_model import CLUSTER_COORD_LIMIT, CLUSTER_MAX_ENTRIES, INT32_MAX

SPLIT_OK, SPLIT_INVALID = 0, 1
SPLIT_MAX_DEPTH = 63
SPLIT_INFO_KEYS = ("n_parts", "n_members", "n_split_clusters", "n_oversize", "largest", "deepest", "status")


def split_oversize(size, extent, max_size, max_extent):
    """the rule's test: 0 switches a criterion off"""
    return (max_size > 0 and size > max_size) or (max_extent > 0 and max(extent) > max_extent)


def split_data_error(vox, offsets, members, n_clusters=None):
    """the first data error of the inputs as a string, None if there is none.  n_clusters: the effective cluster count (the device
    variant's min(n_clusters, *n_clusters_dev)); the effective member count is offsets[n_clusters]"""
    v = np.asarray(vox, dtype=np.int64).reshape(-1, 3)
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    mem = np.asarray(members, dtype=np.int64).reshape(-1)
    K = len(off) - 1 if n_clusters is None else int(n_clusters)
    if K <= 0:
        return None
    if off[0] < 0:
        return "offsets[0] is negative"
    if off[K] > len(mem):
        return "offsets[n_clusters] is above n_members"
    if (np.diff(off[:K + 1]) < 0).any():
        return "offsets decrease"
    used = mem[off[0]:off[K]]
    if ((used < 0) | (used >= len(v))).any():
        return "a member index lies outside the entry list"
    if (np.abs(v[used]) >= CLUSTER_COORD_LIMIT).any():
        return "a member's voxel breaks the coordinate limit"
    return None


def split_model(vox, offsets, members, mask=None, key=None, max_size=0, max_extent=0, max_depth=SPLIT_MAX_DEPTH, resolution=1.0,
                origin=(0.0, 0.0, 0.0), n_clusters=None, device=False):
    """vox: (n, 3) integers; offsets (K + 1,) and members: the cluster call's CSR pair; mask: (n,) uint8 or None; key: (n,) int32 or
    None.  Returns a dict: per part parent, depth, size, root, box_lo, box_hi, centroid, mask_or, key_min, key_argmin; offsets
    (P + 1,) and members (the input's positions, sorted inside each part's segment; positions below offsets[0] keep the input's
    value); label (n,) int32; and the counters of fiesta_hip_split_info (its `depth` is the key `deepest` here).  A data error
    raises ValueError, or with device=True returns what the device variant leaves: status INVALID, no part, label all -1"""
    v = np.asarray(vox, dtype=np.int64).reshape(-1, 3)
    n = len(v)
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    mem = np.asarray(members, dtype=np.int64).reshape(-1)
    K = max(len(off) - 1, 0) if n_clusters is None else int(n_clusters)
    if n > CLUSTER_MAX_ENTRIES or len(mem) > CLUSTER_MAX_ENTRIES or K > CLUSTER_MAX_ENTRIES or K < 0 or K > max(len(off) - 1, 0):
        raise ValueError("a count outside 0 .. 2^24")
    if max_size < 0 or max_extent < 0 or not 0 <= max_depth <= SPLIT_MAX_DEPTH:
        raise ValueError("max_size and max_extent must be >= 0, max_depth in 0 .. 63")
    mask = None if mask is None else np.asarray(mask, dtype=np.uint8).reshape(n)
    key = None if key is None else np.asarray(key, dtype=np.int64).reshape(n)
    err = split_data_error(v, off, mem, K)
    if err is not None:
        if not device:
            raise ValueError(err)
        out = _outputs(0, n)
        out["members"] = np.zeros(0, np.int64)
        out.update(dict.fromkeys(SPLIT_INFO_KEYS, 0), status=SPLIT_INVALID)
        return out

    parts = []                                   # (parent, depth, member list), in the order of the rule

    def split(parent, depth, part):
        c = v[part]
        lo, hi = c.min(axis=0), c.max(axis=0)
        extent = [int(hi[a] - lo[a] + 1) for a in range(3)]
        # (members of one voxel -- a member listed twice, entries that name the same voxel -- cannot be told apart: never cut)
        if depth >= max_depth or max(extent) < 2 or not split_oversize(len(part), extent, max_size, max_extent):
            parts.append((parent, depth, sorted(part)))
            return
        a = extent.index(max(extent))            # the largest extent, the lowest axis among equals
        mid = int(lo[a]) + ((int(hi[a]) - int(lo[a])) >> 1)
        split(parent, depth + 1, [i for i in part if v[i, a] <= mid])
        split(parent, depth + 1, [i for i in part if v[i, a] > mid])

    for k in range(K):
        seg = [int(i) for i in mem[off[k]:off[k + 1]]]
        if seg:
            split(k, 0, seg)

    P = len(parts)
    res, org = float(resolution), [float(c) for c in origin]
    out = _outputs(P, n)
    m0 = int(off[0]) if K else 0
    out["offsets"][0] = m0
    listed = [int(i) for i in mem[:m0]]
    n_oversize = 0
    for p, (parent, depth, cells) in enumerate(parts):
        c = v[cells]
        size = len(cells)
        out["parent"][p], out["depth"][p], out["size"][p], out["root"][p] = parent, depth, size, min(cells)
        out["box_lo"][p], out["box_hi"][p] = c.min(axis=0), c.max(axis=0)
        n_oversize += bool(split_oversize(size, (out["box_hi"][p].astype(np.int64) - out["box_lo"][p] + 1).tolist(), max_size, max_extent))
        for a in range(3):
            s = int(c[:, a].sum())               # exact
            out["centroid"][p, a] = (float(s) / float(size) + 0.5) * res + org[a]
        if mask is not None:
            out["mask_or"][p] = np.bitwise_or.reduce(mask[cells])
        if key is not None:
            best = None
            for i in cells:                      # (increasing index: the first to attain the minimum stays)
                if key[i] >= 0 and (best is None or key[i] < key[best]):
                    best = i
            if best is not None:
                out["key_min"][p], out["key_argmin"][p] = key[best], best
        listed.extend(cells)
        out["offsets"][p + 1] = len(listed)
        out["label"][cells] = p                  # (parts in increasing order: the largest index stays)
    out["members"] = np.asarray(listed, np.int64).reshape(-1)
    out["n_parts"], out["n_members"] = P, len(listed) if K else 0
    out["n_split_clusters"] = len({parent for parent, depth, _ in parts if depth > 0})
    out["n_oversize"] = n_oversize
    out["largest"] = max((len(cells) for _, _, cells in parts), default=0)
    out["deepest"] = max((depth for _, depth, _ in parts), default=0)
    out["status"] = SPLIT_OK
    return out


def _outputs(P, n):
    return {"parent": np.zeros(P, np.int32), "depth": np.zeros(P, np.uint8), "size": np.zeros(P, np.int32), "root": np.zeros(P, np.int64),
            "box_lo": np.zeros((P, 3), np.int32), "box_hi": np.zeros((P, 3), np.int32), "centroid": np.zeros((P, 3), np.float64),
            "mask_or": np.zeros(P, np.uint8), "key_min": np.full(P, INT32_MAX, np.int32), "key_argmin": np.full(P, -1, np.int64),
            "offsets": np.zeros(P + 1, np.int64), "label": np.full(n, -1, np.int32)}
