"""CPU side of the batched path clearance (fiesta_hip_path_clearance, include/fiesta_hip.h): the sample rule.

fiesta_amd.path_samples (numpy) is the model the GPU tests reduce over, so it must be the header's formula bit for bit: it is checked
against a plain Python loop over that formula, on the special cases the header names, and against the C++ facade's
fiesta::ESDFMap::PathSample compiled with the host compiler alone.  Also: the ctypes mirror of fiesta_hip_path_result and the version.
"""
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rule_loop(waypoints, offsets, step):
    """The header's rule, one Python float at a time (IEEE f64, no contraction): per path its samples, or None if invalid."""
    out = []
    for p in range(len(offsets) - 1):
        w = [tuple(float(c) for c in waypoints[i]) for i in range(offsets[p], offsets[p + 1])]
        if not all(math.isfinite(c) for v in w for c in v):
            out.append(None)
            continue
        samples, bad = [], False
        for a, b in zip(w[:-1], w[1:]):
            d = (b[0] - a[0], b[1] - a[1], b[2] - a[2])
            L = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            q = L / step
            if not q <= 2.0 ** 24:
                bad = True
                break
            S = max(1, int(math.ceil(q)))
            samples += [tuple(a[c] + d[c] * (float(k) / float(S)) for c in range(3)) for k in range(S)]
        if bad:
            out.append(None)
            continue
        if w:
            samples.append(w[-1])
        out.append(samples)
    return out


def check_against_loop(w, off, step):
    import fiesta_amd
    pos, n = fiesta_amd.path_samples(w, off, step)
    want = rule_loop(w, off, step)
    assert len(n) == len(want)
    at = 0
    for p, s in enumerate(want):
        if s is None:
            assert n[p] == -1, p
            continue
        assert n[p] == len(s), (p, n[p], len(s))
        got = pos[at:at + len(s)]
        assert np.array_equal(got.view(np.int64), np.array(s, np.float64).reshape(-1, 3).view(np.int64)), p
        at += len(s)
    assert at == len(pos)
    return pos, n


def test_path_samples_equals_the_header_formula_on_random_paths():
    rng = np.random.RandomState(3)
    lens = rng.randint(0, 12, 300)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    w = rng.randn(off[-1], 3) * rng.choice([0.05, 0.7, 5.0], (off[-1], 1))
    dup = np.nonzero(rng.rand(len(w)) < 0.1)[0]
    dup = dup[dup > 0]
    w[dup] = w[dup - 1]                                                    # zero-length segments
    for step in (0.05, 0.2 * 0.37, 1.0, 3.7):
        check_against_loop(w, off, step)


def test_path_samples_special_cases():
    import fiesta_amd
    step = 0.1
    W = np.array([[1.0, 2.0, 3.0],                                          # 0: one waypoint
                  [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.3, 0.0, 0.0],       # 1: a zero-length segment (one sample), then 0.3 / 0.1
                  [0.0, 0.0, 0.0], [0.4, 0.0, 0.0],                        # 2: 0.4 / 0.1 = 4 in f64
                  [5.0, 5.0, 5.0], [5.01, 5.0, 5.0],                       # 3: step > L: one sample per segment
                  [0.0, 0.0, 0.0], [2.0 ** 24 * 0.1 * 1.5, 0.0, 0.0],      # 4: L / step > 2^24: invalid
                  [0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [1.0, 1.0, 1.0],    # 5: NaN waypoint: invalid
                  [0.0, np.inf, 0.0],                                      # 6: inf waypoint: invalid
                  [-0.0, -0.0, -0.0]])                                     # 8: one waypoint, negative zeros kept
    off = np.array([0, 1, 4, 6, 8, 10, 13, 14, 14, 15])                     # (7: empty)
    pos, n = check_against_loop(W, off, step)
    assert list(n) == [1, 1 + math.ceil(0.3 / 0.1) + 1, 5, 2, -1, -1, -1, 0, 1], n
    assert np.array_equal(pos[0], W[0])
    assert np.signbit(pos[-1]).all()                                        # the final sample is the waypoint itself
    # an exact multiple: 0.5 / 0.125 = 4 samples + the end, at 0, 1/4, 1/2, 3/4, 1
    p2, n2 = fiesta_amd.path_samples([[0, 0, 0], [0.5, 0, 0]], [0, 2], 0.125)
    assert n2[0] == 5 and np.array_equal(p2[:, 0], [0, 0.125, 0.25, 0.375, 0.5])
    # one ulp above the 2^24 limit is invalid (the limit itself is valid: tests/test_gpu_path_queries.py, 2^24 + 1 samples)
    _, n3 = fiesta_amd.path_samples([[0, 0, 0], [np.nextafter(2.0 ** 24, np.inf), 0, 0], [0, 0, 0], [1, 0, 0]], [0, 2, 4], 1.0)
    assert list(n3) == [-1, 2]
    with pytest.raises(ValueError):
        fiesta_amd.path_samples(W, [0, 3, 2, 15], step)
    with pytest.raises(ValueError):
        fiesta_amd.path_samples(W, off, 0.0)


def test_facade_path_sample_equals_path_samples(tmp_path):
    """fiesta::ESDFMap::PathSample, compiled with g++ only (no HIP), prints the samples of >= 10^4 random segments as hex doubles:
    the same bits as path_samples"""
    import fiesta_amd
    src = tmp_path / "path_sample.cpp"
    src.write_text(r'''
#include <cstdio>
#include <vector>
#include "fiesta/ESDFMap.h"
int main(int argc, char **argv) {
  FILE *f = std::fopen(argv[1], "rb");
  long long n = 0;
  double step = 0;
  if (std::fread(&n, 8, 1, f) != 1 || std::fread(&step, 8, 1, f) != 1) return 1;
  std::vector<double> w(6 * n);
  if (std::fread(w.data(), 8, w.size(), f) != w.size()) return 1;
  for (long long s = 0; s < n; ++s) {
    std::vector<Eigen::Vector3d> path{Eigen::Vector3d(w[6 * s], w[6 * s + 1], w[6 * s + 2]),
                                      Eigen::Vector3d(w[6 * s + 3], w[6 * s + 4], w[6 * s + 5])};
    for (long long k = 0;; ++k) {
      const Eigen::Vector3d p = fiesta::ESDFMap::PathSample(path, step, k);
      if (p(0) != p(0)) break;
      std::printf("%lld %a %a %a\n", s, p(0), p(1), p(2));
    }
  }
  return 0;
}
''')
    exe = str(tmp_path / "path_sample")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-o", exe], check=True)
    rng = np.random.RandomState(5)
    n, step = 12000, 0.0731
    a = rng.rand(n, 3) * 20 - 10
    b = a + rng.randn(n, 3) * rng.choice([0.0, 0.01, 0.1, 0.4], (n, 1))
    w = np.stack([a, b], 1).reshape(-1, 3)
    blob = tmp_path / "segments.bin"
    blob.write_bytes(np.int64(n).tobytes() + np.float64(step).tobytes() + w.tobytes())
    out = subprocess.run([exe, str(blob)], capture_output=True, text=True, check=True).stdout.split("\n")
    rows = [ln.split() for ln in out if ln]
    got = np.array([[float.fromhex(v) for v in r[1:]] for r in rows])
    pos, ns = fiesta_amd.path_samples(w, np.arange(0, 2 * n + 1, 2), step)
    assert np.all(ns > 0) and len(got) == len(pos) == ns.sum()
    assert np.array_equal(got.view(np.int64), pos.view(np.int64))


def test_path_result_struct_matches_header():
    from fiesta_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    body = re.search(r"typedef struct fiesta_hip_path_result \{(.*?)\} fiesta_hip_path_result;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    names = [d.split(None, 1)[1].lstrip("*").strip() for d in decls]
    assert names == [f[0] for f in _lib.PathResult._fields_]
    assert all(d.split(None, 1)[1].startswith("*") for d in decls)       # seven pointers
    import fiesta_amd.esdf_map as em
    assert [f[0] for f in em.PATH_FIELDS] == names
    types = [d.split(None, 1)[0] for d in decls]
    assert ["int64_t" if f[1] == np.int64 else "double" for f in em.PATH_FIELDS] == types


def test_version_announces_path_clearance():
    import __graft_entry__ as g
    g.build_hip()
    import fiesta_amd
    lib = fiesta_amd.load()
    assert lib.fiesta_hip_version() == 101
    assert hasattr(lib, "fiesta_hip_path_clearance") and hasattr(lib, "fiesta_hip_path_clearance_dev")
