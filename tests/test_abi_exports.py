"""CPU-side checks of the drop-in boundary: libfiesta_hip.so loads without a GPU, exports every symbol
include/fiesta_hip.h declares (and nothing is declared that the Python mirror does not bind), reports zero
devices instead of crashing, and FAILS LOUDLY -- no CPU fallback -- when asked to create a map without one.
"""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    import fiesta_amd
    return fiesta_amd.load()


def test_every_declared_symbol_is_exported_and_bound(lib):
    from fiesta_amd import _lib
    declared = _lib.declared_symbols()
    assert len(declared) >= 30
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in include/fiesta_hip.h but not exported"
    assert sorted(lib._fiesta_signatures) == declared, "python binding and header disagree"
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (fiesta_hip_[a-z0-9_]+)", nm))
    assert exported == set(declared), exported ^ set(declared)


def test_struct_layouts_match_header():
    from fiesta_amd import _lib
    text = open(_lib.HEADER_PATH).read()

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            for nm_ in decl.split(None, 1)[1].split(","):
                out.append(re.sub(r"\[.*?\]", "", nm_).strip())
        return out
    assert fields("fiesta_hip_config") == [f[0] for f in _lib.Config._fields_]
    assert fields("fiesta_hip_stats") == [f[0] for f in _lib.Stats._fields_]
    assert fields("fiesta_hip_raycast_params") == [f[0] for f in _lib.RaycastParams._fields_]


def test_no_gpu_means_loud_failure_not_fallback(lib):
    import torch
    import fiesta_amd
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible; the no-device behaviour is checked on the CPU container")
    assert fiesta_amd.device_count() == 0
    with pytest.raises(fiesta_amd.FiestaHipError):
        fiesta_amd.ESDFMap((0, 0, 0), 0.1, (1.0, 1.0, 1.0))
    assert b"no HIP device" in lib.fiesta_hip_last_error() or lib.fiesta_hip_last_error()


def test_product_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under fiesta_amd/ or include/ may reference it."""
    bad = []
    for base in ("fiesta_amd", "include"):
        for dp, _, fs in os.walk(os.path.join(ROOT, base)):
            for f in fs:
                if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                    src = open(os.path.join(dp, f), errors="replace").read()
                    if re.search(r"(from|import)\s+oracle|oracle_api\.h|pyoracle|libfiesta_port|libfiesta_ref", src):
                        bad.append(os.path.join(dp, f))
    assert not bad, bad


def test_hand_scheduled_kernels_do_not_spill():
    """k_nn_fill_full, k_ft_x and k_ft_plane wait for LDS-DMA fetches with COUNTED s_waitcnt vmcnt(n) around inline asm: a scratch
    spill (an extra VMEM operation the count does not know) would make them consume stale records silently.  The
    code objects inside the built library are inspected: no scratch, no spilled registers."""
    import sys
    from fiesta_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import check_kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build_hip()
    guarded = check_kernel_resources.check(_lib.LIB_PATH)
    assert any("k_nn_fill_full" in k for k in guarded) and any("k_ft_x" in k for k in guarded)


def test_planner_kernels_are_compiled_once():
    """All sixteen planner calls are compiled in planner.hip alone: each of their kernels sits in exactly one code object of the
    library, all in the same one.  The library holds four: those of dense_map.hip, hash_map.hip, planner.hip and raycast.hip (the
    other sources define no kernel).  Held more than once are only k_level_next, k_zero_words and k_zero_words2, of the headers
    that the store units share.  Kernel names only are read."""
    import sys
    from fiesta_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build_hip()
    copies = check_kernel_resources.kernel_copies(_lib.LIB_PATH)
    families = ("k_reach_path_", "k_leg_path_", "k_cluster_", "k_split_", "k_tour_", "k_corridor_bounds", "k_bounds_fill",
                "k_reach_", "k_rmx_", "k_view_", "k_path_", "k_cost_", "k_refine", "k_timing", "k_frontier_", "k_ray_query",
                "k_free_boxes", "k_corridor_")
    mine = {k: v for k, v in copies.items() if any(f in k for f in families)}
    for f in families:
        assert any(f in k for k in mine), (f, sorted(mine))
    assert all(len(v) == 1 for v in mine.values()), {k: v for k, v in mine.items() if len(v) != 1}
    assert len({v[0] for v in mine.values()}) == 1, mine
    assert len(check_kernel_resources.code_objects(_lib.LIB_PATH)) == 4
    shared = sorted(k for k, v in copies.items() if len(v) > 1)
    assert len(shared) <= 3, shared
    # (mangled names: the length-prefixed identifier, then E)
    assert all(any(name in k for name in ("12k_level_nextE", "12k_zero_wordsE", "13k_zero_words2E")) for k in shared), shared


def test_path_note_names_follow_the_header():
    """fiesta_hip_stats.path_notes: the names the Python statistics give the bits (`why`) are the header's FIESTA_HIP_NOTE_* in
    bit order, and the struct mirrors end in the same field."""
    import re
    from fiesta_amd._lib import Stats
    text = open(os.path.join(ROOT, "include", "fiesta_hip.h")).read()
    notes = re.findall(r"#define FIESTA_HIP_NOTE_(\w+) (0x[0-9a-fA-F]+)", text)
    assert len(notes) == len(Stats.NOTES) >= 10
    for bit, (name, value) in enumerate(notes):
        assert int(value, 16) == 1 << bit, (name, value)
        assert Stats.NOTES[bit] == name.lower(), (bit, name, Stats.NOTES[bit])
    assert Stats._fields_[-1][0] == "path_notes"
    assert re.search(r"int64_t path_notes;[^}]*\} fiesta_hip_stats;", text, re.S)
