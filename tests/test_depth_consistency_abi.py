"""CPU checks of ellc_keyframe_depth_consistency's side of the boundary (ABI v14): the declaration, the version, the binding's lists,
the symbols of the two built libraries, the record as the C compiler sees it against the ctypes mirror, and the header / facade still
plain C99 / C++11."""
import ctypes
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["sum_chi2", "sum_w_ss", "sum_w_st", "sum_abs_di", "sum_di2", "n_kept", "n_in_view", "n_overlap", "n_agree", "n_in_front", "n_behind",
          "n_weighted"]


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_symbol_is_declared_bound_built_and_versioned():
    import __graft_entry__ as g
    g.build()
    from egomotion_with_local_loop_closures_amd import _lib, api
    assert "ellc_keyframe_depth_consistency" in _lib.ABI_SYMBOLS and "ellc_keyframe_depth_consistency" not in _lib.DIAG_SYMBOLS
    assert "ellc_profile_depth_consistency" in _lib.DIAG_SYMBOLS and "ellc_profile_depth_consistency" not in _lib.ABI_SYMBOLS
    header = open(os.path.join(ROOT, "include", "ellc_abi.h")).read()
    assert re.search(r"ellc_status\s+ellc_keyframe_depth_consistency\s*\(", header)
    assert int(re.search(r"#define ELLC_ABI_VERSION (\d+)", header).group(1)) >= 14
    diag_header = open(os.path.join(ROOT, "include", "ellc_abi_diag.h")).read()
    assert re.search(r"ellc_status\s+ellc_profile_depth_consistency\s*\(", diag_header) and "ellc_profile_depth_consistency" not in header
    assert _lib.lib().ellc_abi_version() >= 14
    assert hasattr(_lib.lib(), "ellc_keyframe_depth_consistency") and hasattr(_lib.diag_lib(), "ellc_keyframe_depth_consistency")
    assert callable(api.Context.depth_consistency) and callable(api.Context.profile_depth_consistency)
    ship, diag = exported(_lib.SO_PATH), exported(_lib.DIAG_SO_PATH)
    assert "ellc_keyframe_depth_consistency" in ship and "ellc_keyframe_depth_consistency" in diag
    assert "ellc_profile_depth_consistency" in diag and "ellc_profile_depth_consistency" not in ship
    so = open(_lib.SO_PATH, "rb").read()
    for kernel in (b"consist_pass", b"consist_finish"):
        assert kernel in so, kernel


def test_record_layout_matches_header(tmp_path):
    from egomotion_with_local_loop_closures_amd import _lib
    cls = _lib.EllcDepthConsistency
    assert [f[0] for f in cls._fields_] == FIELDS
    lines = ['#include "ellc_abi.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {",
             '  printf("size %zu\\n", sizeof(ellc_depth_consistency));']
    for f in FIELDS:
        lines.append('  printf("%s %%zu %%zu\\n", offsetof(ellc_depth_consistency, %s), sizeof(((ellc_depth_consistency*)0)->%s));' % (f, f, f))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    seen = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert seen["size"] == [72] and ctypes.sizeof(cls) == 72
    dt = np.dtype(cls)
    assert dt.itemsize == 72 and list(dt.names) == FIELDS
    for f in FIELDS:
        d = getattr(cls, f)
        assert seen[f] == [d.offset, d.size], f
        assert d.offset % d.size == 0, f   # every field naturally aligned
        assert dt.fields[f][1] == d.offset and dt.fields[f][0].itemsize == d.size, f


def test_header_is_c99_and_the_facade_cxx11(tmp_path):
    c = tmp_path / "abi.c"
    c.write_text('#include "ellc_abi.h"\nint main(void) { ellc_map_filter f; ellc_depth_consistency r; int s = 0; float T[12] = {0}; f.stride = 1; '
                 'r.n_kept = 0; (void)r; return (int)ellc_keyframe_depth_consistency(0, 1, &s, &s, T, 0, &f, 1.0f, &r); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(c)])
    cc = tmp_path / "facade.cpp"
    cc.write_text('#include "ellc_facade.hpp"\n'
                  'double use(ellc::globalOptimize& g) { g.collectMatchGeometry = true; g.match_geometry_file.open("geometry.txt"); '
                  'double s = 0; for (size_t i = 0; i < g.lastMatchGeometry.size(); i++) s += g.lastMatchGeometry[i].scale * g.lastMatchGeometry[i].rec.n_agree; '
                  'return s; }\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(cc)])
