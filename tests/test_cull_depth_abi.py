"""CPU checks of the consistency filter's side of the boundary (ABI v22): the declarations, the version, the binding's lists, the
symbols and kernels of the two built libraries, the two structs as the C compiler sees them against the ctypes mirrors, the header /
facade still plain C99 / C++11, the default parameters, and the code-object metadata of the new kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cull_depth_reference as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PRODUCT = ["ellc_keyframe_cull_depth", "ellc_cull_default_params"]
PARAM_FIELDS = ["agree_k2", "sigma_i2", "photo_k", "min_support", "min_judged", "min_in_front", "min_photo"]
STATS_FIELDS = ["n_kept", "n_retained", "n_unseen", "n_culled_free_space", "n_culled_unsupported", "n_culled_photo", "sum_agree", "sum_in_front",
                "sum_behind", "sum_photo", "sum_photo_bad"]
STATUS = ("NOT_TAKING_PART", "KEPT", "CULLED_FREE_SPACE", "CULLED_UNSUPPORTED", "CULLED_PHOTO", "UNSEEN")


@pytest.fixture(scope="module")
def api():
    import __graft_entry__ as g
    g.build()
    from egomotion_with_local_loop_closures_amd import api
    return api


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_symbols_are_declared_bound_built_and_versioned(api):
    from egomotion_with_local_loop_closures_amd import _lib
    header = open(os.path.join(ROOT, "include", "ellc_abi.h")).read()
    diag_header = open(os.path.join(ROOT, "include", "ellc_abi_diag.h")).read()
    for name in PRODUCT:
        assert name in _lib.ABI_SYMBOLS and name not in _lib.DIAG_SYMBOLS
        assert re.search(r"\b%s\s*\(" % name, header)
        assert hasattr(_lib.lib(), name) and hasattr(_lib.diag_lib(), name)
    assert "ellc_profile_cull_depth" in _lib.DIAG_SYMBOLS and "ellc_profile_cull_depth" not in _lib.ABI_SYMBOLS
    assert re.search(r"ellc_status\s+ellc_profile_cull_depth\s*\(", diag_header) and "ellc_profile_cull_depth" not in header
    assert int(re.search(r"#define ELLC_ABI_VERSION (\d+)", header).group(1)) >= 22
    assert _lib.lib().ellc_abi_version() >= 22 and _lib.diag_lib().ellc_abi_version() == _lib.lib().ellc_abi_version()
    for k, name in enumerate(STATUS):
        assert re.search(r"ELLC_CULL_%s = %d\b" % (name, k), header), name
        assert _lib.CULL_STATUS[k] == name
    assert (Q.NOT_TAKING_PART, Q.KEPT, Q.CULLED_FREE_SPACE, Q.CULLED_UNSUPPORTED, Q.CULLED_PHOTO, Q.UNSEEN) == tuple(range(6))
    assert list(_lib.CULL_STATS_FIELDS) == STATS_FIELDS
    for name in ("cull_depth", "profile_cull_depth"):
        assert callable(getattr(api.Context, name))
    assert callable(api.cull_default_params)
    ship, diag = exported(_lib.SO_PATH), exported(_lib.DIAG_SO_PATH)
    assert set(PRODUCT) <= ship and set(PRODUCT) <= diag
    assert "ellc_profile_cull_depth" in diag and "ellc_profile_cull_depth" not in ship
    for path in (_lib.SO_PATH, _lib.DIAG_SO_PATH):
        so = open(path, "rb").read()
        for kernel in (b"cull_pixels", b"cull_finish"):
            assert kernel in so, (path, kernel)


def test_default_params(api):
    p = api.cull_default_params()
    assert (p.agree_k2, p.sigma_i2, p.photo_k, p.min_support, p.min_judged, p.min_in_front, p.min_photo) == (1.0, 16.0, 3.0, 1, 2, 1, 2)
    q = api.cull_default_params(photo_k=0.0, min_judged=3)
    assert (q.photo_k, q.min_judged, q.agree_k2, q.min_photo) == (0.0, 3, 1.0, 2)
    assert Q.DEFAULT_PARAMS == dict(agree_k2=1.0, sigma_i2=16.0, photo_k=3.0, min_support=1, min_judged=2, min_in_front=1, min_photo=2)
    header = open(os.path.join(ROOT, "include", "ellc_abi.h")).read()
    section = header[header.index("removed (v22)"):header.index("ellc_cull_status;")]
    assert "{1, 16, 3, 1, 2, 1, 2}" in section and "DESIGN CHOICES" in section   # the defaults are called what they are
    assert "K at the identity agrees with itself" in section


def test_struct_layouts_match_header(tmp_path, api):
    from egomotion_with_local_loop_closures_amd import _lib
    assert [f[0] for f in _lib.EllcCullParams._fields_] == PARAM_FIELDS and [f[0] for f in _lib.EllcCullStats._fields_] == STATS_FIELDS
    lines = ['#include "ellc_abi.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {",
             '  printf("params %zu\\n", sizeof(ellc_cull_params));', '  printf("stats %zu\\n", sizeof(ellc_cull_stats));']
    for st, fields in (("ellc_cull_params", PARAM_FIELDS), ("ellc_cull_stats", STATS_FIELDS)):
        for f in fields:
            lines.append('  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (st, f, st, f, st, f))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    seen = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert seen["params"] == [28] and ctypes.sizeof(_lib.EllcCullParams) == 28
    assert seen["stats"] == [64] and ctypes.sizeof(_lib.EllcCullStats) == 64
    for st, cls, fields in (("ellc_cull_params", _lib.EllcCullParams, PARAM_FIELDS), ("ellc_cull_stats", _lib.EllcCullStats, STATS_FIELDS)):
        for f in fields:
            d = getattr(cls, f)
            assert seen["%s.%s" % (st, f)] == [d.offset, d.size], (st, f)
            assert d.offset % d.size == 0, (st, f)   # every field naturally aligned
    assert seen["ellc_cull_stats.n_culled_photo"] == [20, 4] and seen["ellc_cull_stats.sum_agree"] == [24, 8]
    assert seen["ellc_cull_stats.sum_photo_bad"] == [56, 8]


def test_header_is_c99_and_the_facade_cxx11(tmp_path):
    c = tmp_path / "abi.c"
    c.write_text('#include "ellc_abi.h"\nint main(void) { ellc_cull_params p; ellc_cull_stats st; ellc_map_filter f = {0.0f, 0, 1.0f, 1}; int s = 0; '
                 'float T[12] = {0}; float l[2] = {1, 0}; ellc_cull_default_params(&p); st.n_kept = 0; '
                 'ellc_cull_status q = ELLC_CULL_CULLED_PHOTO; (void)q; '
                 'return (int)ellc_keyframe_cull_depth(0, 0, 0, 1, 1, &s, T, l, &f, &p, -1, 0, 0, 0, 0, 0, &st); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(c)])
    cc = tmp_path / "facade.cpp"
    cc.write_text('#include "ellc_facade.hpp"\n'
                  'long long use(ellc::globalOptimize& g) { g.refineMatchSim3 = true; g.cullMatchDepth = true; g.cull_matches_file.open("cull.txt"); '
                  'return g.lastCullStats.n_culled_free_space + g.lastCullStats.sum_agree + g.lastCullViews; }\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(cc)])


def test_kernels_have_no_scratch_and_no_spills(tmp_path, api):
    """The gfx950 code object of the shipping library holds cull_pixels and cull_finish with a private segment of 0 and no spilled
    registers (the code object's own metadata, read with the toolchain that built it, as tests/test_refine_depth_abi.py reads it)."""
    from egomotion_with_local_loop_closures_amd import _lib
    llvm = "/opt/rocm/llvm/bin"
    fat, co = tmp_path / "fat.bin", tmp_path / "gfx950.co"
    subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=%s" % fat, _lib.SO_PATH, str(tmp_path / "copy.so")], check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=%s" % fat,
                    "--output=%s" % co, "--unbundle"], check=True)
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for block in re.split(r"\n  - (?=\.)", notes):   # one block per entry of amdhsa.kernels
        name = re.search(r"^\s*\.name:\s+(\S+)\s*$", block, flags=re.M)
        if name and ".private_segment_fixed_size" in block:
            kernels[name.group(1)] = {k: int(v) for k, v in re.findall(
                r"^\s*\.(private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\d+)\s*$", block, flags=re.M)}
    for kernel in ("cull_pixels", "cull_finish"):
        found = [v for k, v in kernels.items() if kernel in k]
        assert len(found) == 1, (kernel, sorted(kernels)[:5])
        print(kernel, found[0])
        assert found[0]["private_segment_fixed_size"] == 0 and found[0]["vgpr_spill_count"] == 0 and found[0]["sgpr_spill_count"] == 0, (kernel, found[0])
    # no LDS beyond the stats tail: the four wave records (five 64-bit sums, eight 32-bit words each)
    assert [v for k, v in kernels.items() if "cull_pixels" in k][0]["group_segment_fixed_size"] == 4 * 72
    assert [v for k, v in kernels.items() if "cull_finish" in k][0]["group_segment_fixed_size"] == 0
