"""CPU checks of the depth sweep's side of the boundary (ABI v21): the declarations, the version, the binding's lists, the symbols and
kernels of the two built libraries, the two structs as the C compiler sees them against the ctypes mirrors, the header / facade still
plain C99 / C++11, the default parameters, and the code-object metadata of the new kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import sweep_depth_reference as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PRODUCT = ["ellc_keyframe_sweep_depth", "ellc_sweep_default_params"]
PARAM_FIELDS = ["sigma_i2", "huber_k", "d_min", "d_max", "min_grad2", "max_cost", "distinct_ratio", "var_scale", "n_samples", "min_views"]
STATS_FIELDS = ["n_ok", "n_swept", "n_created", "n_no_valid_sample", "n_at_range_end", "n_cost_too_high", "n_not_distinct", "n_flat", "sum_views",
                "sum_cost", "reserved"]
STATUS = ("NOT_SWEPT", "CREATED", "NO_VALID_SAMPLE", "AT_RANGE_END", "COST_TOO_HIGH", "NOT_DISTINCT", "FLAT")


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
    assert "ellc_profile_sweep_depth" in _lib.DIAG_SYMBOLS and "ellc_profile_sweep_depth" not in _lib.ABI_SYMBOLS
    assert re.search(r"ellc_status\s+ellc_profile_sweep_depth\s*\(", diag_header) and "ellc_profile_sweep_depth" not in header
    assert int(re.search(r"#define ELLC_ABI_VERSION (\d+)", header).group(1)) >= 21
    assert _lib.lib().ellc_abi_version() >= 21
    assert re.search(r"#define ELLC_SWEEP_MAX_SAMPLES 64\b", header)
    for k, name in enumerate(STATUS):
        assert re.search(r"ELLC_SWEEP_%s = %d\b" % (name, k), header), name
        assert _lib.SWEEP_STATUS[k] == name
    assert list(_lib.SWEEP_STATS_FIELDS) == STATS_FIELDS[:-1]
    for name in ("sweep_depth", "profile_sweep_depth"):
        assert callable(getattr(api.Context, name))
    assert callable(api.sweep_params)
    ship, diag = exported(_lib.SO_PATH), exported(_lib.DIAG_SO_PATH)
    assert set(PRODUCT) <= ship and set(PRODUCT) <= diag
    assert "ellc_profile_sweep_depth" in diag and "ellc_profile_sweep_depth" not in ship
    so = open(_lib.SO_PATH, "rb").read()
    for kernel in (b"sweep_pixels", b"sweep_finish"):
        assert kernel in so, kernel


def test_default_params(api):
    p = api.sweep_params()
    assert (p.sigma_i2, p.huber_k, p.d_min, p.d_max, p.min_grad2, p.max_cost, p.distinct_ratio, p.var_scale, p.n_samples, p.min_views) == (
        16.0, F(1.345), 0.125, 4.0, 100.0, 0.0, F(0.7), 1.0, 64, 2)
    q = api.sweep_params(n_samples=16, d_max=2.0)
    assert (q.n_samples, q.d_max, q.d_min, q.min_views) == (16, 2.0, 0.125, 2)
    assert W.DEFAULT_PARAMS == dict(sigma_i2=16.0, huber_k=1.345, d_min=0.125, d_max=4.0, min_grad2=100.0, max_cost=0.0, distinct_ratio=0.7,
                                    var_scale=1.0, n_samples=64, min_views=2)
    header = open(os.path.join(ROOT, "include", "ellc_abi.h")).read()
    assert "DESIGN CHOICES" in header   # the defaults are called what they are


def test_struct_layouts_match_header(tmp_path, api):
    from egomotion_with_local_loop_closures_amd import _lib
    assert [f[0] for f in _lib.EllcSweepParams._fields_] == PARAM_FIELDS and [f[0] for f in _lib.EllcSweepStats._fields_] == STATS_FIELDS
    lines = ['#include "ellc_abi.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {",
             '  printf("params %zu\\n", sizeof(ellc_sweep_params));', '  printf("stats %zu\\n", sizeof(ellc_sweep_stats));']
    for st, fields in (("ellc_sweep_params", PARAM_FIELDS), ("ellc_sweep_stats", STATS_FIELDS)):
        for f in fields:
            lines.append('  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (st, f, st, f, st, f))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    seen = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert seen["params"] == [40] and ctypes.sizeof(_lib.EllcSweepParams) == 40
    assert seen["stats"] == [64] and ctypes.sizeof(_lib.EllcSweepStats) == 64
    for st, cls, fields in (("ellc_sweep_params", _lib.EllcSweepParams, PARAM_FIELDS), ("ellc_sweep_stats", _lib.EllcSweepStats, STATS_FIELDS)):
        for f in fields:
            d = getattr(cls, f)
            assert seen["%s.%s" % (st, f)] == [d.offset, d.size], (st, f)
            element = 4 if f == "reserved" else d.size
            assert d.offset % element == 0, (st, f)   # every field naturally aligned
    assert seen["ellc_sweep_stats.sum_views"] == [32, 8] and seen["ellc_sweep_stats.sum_cost"] == [40, 8]
    assert seen["ellc_sweep_stats.reserved"] == [48, 16]


def test_header_is_c99_and_the_facade_cxx11(tmp_path):
    c = tmp_path / "abi.c"
    c.write_text('#include "ellc_abi.h"\nint main(void) { ellc_sweep_params p; ellc_sweep_stats st; int s = 0; float T[12] = {0}; '
                 'float l[2] = {1, 0}; ellc_sweep_default_params(&p); st.n_ok = 0; '
                 'ellc_sweep_status q = ELLC_SWEEP_CREATED; (void)q; '
                 'return (int)ellc_keyframe_sweep_depth(0, 0, 0, 1, 1, &s, T, l, &p, -1, 0, 0, 0, 0, &st); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(c)])
    cc = tmp_path / "facade.cpp"
    cc.write_text('#include "ellc_facade.hpp"\n'
                  'double use(ellc::globalOptimize& g) { g.refineMatchSim3 = true; g.sweepMatchDepth = true; g.sweep_matches_file.open("sweep.txt"); '
                  'return g.lastSweepStats.n_created + g.lastSweepStats.sum_cost + g.lastSweepViews; }\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(cc)])


def test_kernels_have_no_scratch_and_no_spills(tmp_path, api):
    """The gfx950 code object of the shipping library holds sweep_pixels and sweep_finish with a private segment of 0 and no spilled
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
    for kernel in ("sweep_pixels", "sweep_finish"):
        found = [v for k, v in kernels.items() if kernel in k]
        assert len(found) == 1, (kernel, sorted(kernels)[:5])
        print(kernel, found[0])
        assert found[0]["private_segment_fixed_size"] == 0 and found[0]["vgpr_spill_count"] == 0 and found[0]["sgpr_spill_count"] == 0, (kernel, found[0])
    # the samples' costs are carried in registers while they go by: the pixel kernel's only LDS is the four wave records of the stats tail
    assert [v for k, v in kernels.items() if "sweep_pixels" in k][0]["group_segment_fixed_size"] == 4 * 56   # (a record: one double, one 64-bit integer, ten 32-bit words)
