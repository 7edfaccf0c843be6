"""CPU checks of the depth refinement's side of the boundary (ABI v20): the declarations, the version, the binding's lists, the symbols
and kernels of the two built libraries, the two structs as the C compiler sees them against the ctypes mirrors, the header / facade
still plain C99 / C++11, the default parameters, ellc_sim3_invert on the library itself, and the code-object metadata of the new
kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import refine_depth_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PRODUCT = ["ellc_keyframe_refine_depth", "ellc_refine_default_params", "ellc_sim3_invert"]
PARAM_FIELDS = ["sigma_i2", "huber_k", "prior_weight", "max_step_rel", "n_iter", "min_views"]
STATS_FIELDS = ["n_kept", "n_taking_part", "n_refined", "n_too_few_views", "n_no_information", "n_bad_step", "n_views_changed", "n_cost_rose",
                "sum_views", "sum_cost_before", "sum_cost_after", "reserved"]


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
    assert "ellc_profile_refine_depth" in _lib.DIAG_SYMBOLS and "ellc_profile_refine_depth" not in _lib.ABI_SYMBOLS
    assert re.search(r"ellc_status\s+ellc_profile_refine_depth\s*\(", diag_header) and "ellc_profile_refine_depth" not in header
    assert int(re.search(r"#define ELLC_ABI_VERSION (\d+)", header).group(1)) >= 20
    assert _lib.lib().ellc_abi_version() >= 20
    assert re.search(r"#define ELLC_REFINE_MAX_VIEWS 64\b", header)
    for k, name in enumerate(("NOT_TAKING_PART", "REFINED", "TOO_FEW_VIEWS", "NO_INFORMATION", "BAD_STEP", "VIEWS_CHANGED", "COST_ROSE")):
        assert re.search(r"ELLC_REFINE_%s = %d\b" % (name, k), header), name
        assert _lib.REFINE_STATUS[k] == name
    for name in ("refine_depth", "profile_refine_depth"):
        assert callable(getattr(api.Context, name))
    assert callable(api.refine_default_params) and callable(api.sim3_invert)
    ship, diag = exported(_lib.SO_PATH), exported(_lib.DIAG_SO_PATH)
    assert set(PRODUCT) <= ship and set(PRODUCT) <= diag
    assert "ellc_profile_refine_depth" in diag and "ellc_profile_refine_depth" not in ship
    so = open(_lib.SO_PATH, "rb").read()
    for kernel in (b"refine_pixels", b"refine_finish"):
        assert kernel in so, kernel


def test_default_params(api):
    p = api.refine_default_params()
    assert (p.sigma_i2, p.huber_k, p.prior_weight, p.max_step_rel, p.n_iter, p.min_views) == (16.0, F(1.345), 1.0, 0.5, 3, 2)
    q = api.refine_default_params(n_iter=5, prior_weight=0.0)
    assert (q.n_iter, q.prior_weight, q.min_views) == (5, 0.0, 2)
    assert {k: v for k, v in R.DEFAULT_PARAMS.items()} == dict(sigma_i2=16.0, huber_k=1.345, prior_weight=1.0, max_step_rel=0.5, n_iter=3, min_views=2)


def test_struct_layouts_match_header(tmp_path, api):
    from egomotion_with_local_loop_closures_amd import _lib
    assert [f[0] for f in _lib.EllcRefineParams._fields_] == PARAM_FIELDS and [f[0] for f in _lib.EllcRefineStats._fields_] == STATS_FIELDS
    lines = ['#include "ellc_abi.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {",
             '  printf("params %zu\\n", sizeof(ellc_refine_params));', '  printf("stats %zu\\n", sizeof(ellc_refine_stats));']
    for st, fields in (("ellc_refine_params", PARAM_FIELDS), ("ellc_refine_stats", STATS_FIELDS)):
        for f in fields:
            lines.append('  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (st, f, st, f, st, f))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    seen = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert seen["params"] == [24] and ctypes.sizeof(_lib.EllcRefineParams) == 24
    assert seen["stats"] == [64] and ctypes.sizeof(_lib.EllcRefineStats) == 64
    for st, cls, fields in (("ellc_refine_params", _lib.EllcRefineParams, PARAM_FIELDS), ("ellc_refine_stats", _lib.EllcRefineStats, STATS_FIELDS)):
        for f in fields:
            d = getattr(cls, f)
            assert seen["%s.%s" % (st, f)] == [d.offset, d.size], (st, f)
            element = 4 if f == "reserved" else d.size
            assert d.offset % element == 0, (st, f)   # every field naturally aligned
    assert seen["ellc_refine_stats.sum_views"] == [32, 8] and seen["ellc_refine_stats.sum_cost_after"] == [48, 8]
    assert seen["ellc_refine_stats.reserved"] == [56, 8]


def test_header_is_c99_and_the_facade_cxx11(tmp_path):
    c = tmp_path / "abi.c"
    c.write_text('#include "ellc_abi.h"\nint main(void) { ellc_map_filter f; ellc_refine_params p; ellc_refine_stats st; int s = 0; float T[12] = {0}; '
                 'float l[2] = {1, 0}; f.stride = 1; ellc_refine_default_params(&p); st.n_kept = 0; ellc_sim3_invert(T, l, T, l); '
                 'ellc_refine_status q = ELLC_REFINE_REFINED; (void)q; '
                 'return (int)ellc_keyframe_refine_depth(0, 0, 0, 1, 1, &s, T, l, &f, &p, -1, 0, 0, 0, 0, &st); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(c)])
    cc = tmp_path / "facade.cpp"
    cc.write_text('#include "ellc_facade.hpp"\n'
                  'double use(ellc::globalOptimize& g) { g.refineMatchSim3 = true; g.refineMatchDepth = true; g.refine_matches_file.open("refine.txt"); '
                  'return g.lastRefineStats.n_refined + g.lastRefineStats.sum_cost_after + g.lastRefineViews; }\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(cc)])


def test_sim3_invert_on_the_library(api):
    """ellc_sim3_invert within 2 f32 ulp of max |T'| of numpy.linalg.inv in double (the reference rule's own bound,
    tests/test_refine_depth_reference.py), the light's two values bit for bit (one division in double, one rounding); NULL lights; in place."""
    rng = np.random.default_rng(20)
    from egomotion_with_local_loop_closures_amd import synth, _lib
    for k in range(20):
        T = synth.se3_exp(rng.uniform(-0.5, 0.5, 6))[:3].copy()
        T[:, :3] *= rng.uniform(0.3, 3.0)
        T[:, 3] *= rng.uniform(0.1, 10.0)
        T32 = T.astype(F).reshape(12)
        light = np.array([rng.uniform(0.3, 3.0), rng.uniform(-40, 40)], F)
        got, gl = api.sim3_invert(T32, light)
        want = np.linalg.inv(np.vstack([T32.reshape(3, 4).astype(np.float64), [0, 0, 0, 1]]))[:3].reshape(12)
        bound = 2 * float(np.spacing(F(np.abs(want).max())))
        assert np.abs(got.astype(np.float64) - want).max() <= bound, (k, got, want)
        ref_T, ref_l = R.sim3_invert(T32, light)
        assert np.abs(got.astype(np.float64) - ref_T.astype(np.float64)).max() <= bound
        assert gl.tobytes() == ref_l.tobytes()
        # NULL light in: (1, 0) out; NULL light out: accepted; outputs may be the inputs
        To = np.zeros(12, F); lo = np.full(2, 7, F)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        _lib.lib().ellc_sim3_invert(p(T32), None, p(To), p(lo))
        assert To.tobytes() == got.tobytes() and lo.tolist() == [1.0, 0.0]
        _lib.lib().ellc_sim3_invert(p(T32), p(light), p(To), None)
        inplace_T, inplace_l = T32.copy(), light.copy()
        _lib.lib().ellc_sim3_invert(p(inplace_T), p(inplace_l), p(inplace_T), p(inplace_l))
        assert inplace_T.tobytes() == got.tobytes() and inplace_l.tobytes() == gl.tobytes()
    ident = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)
    got, gl = api.sim3_invert(ident)
    assert np.array_equal(got, ident) and gl.tolist() == [1.0, 0.0]


def test_kernels_have_no_scratch_and_no_spills(tmp_path, api):
    """The gfx950 code object of the shipping library holds refine_pixels and refine_finish with a private segment of 0 and no spilled
    registers (the code object's own metadata, read with the toolchain that built it, as tests/test_sim3_abi.py reads it)."""
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
    for kernel in ("refine_pixels", "refine_finish"):
        found = [v for k, v in kernels.items() if kernel in k]
        assert len(found) == 1, (kernel, sorted(kernels)[:5])
        print(kernel, found[0])
        assert found[0]["private_segment_fixed_size"] == 0 and found[0]["vgpr_spill_count"] == 0 and found[0]["sgpr_spill_count"] == 0, (kernel, found[0])
    # the pixel kernel's only LDS is the four wave records of the stats tail (a record indexed at run time would move to LDS: 16 KB more)
    assert [v for k, v in kernels.items() if "refine_pixels" in k][0]["group_segment_fixed_size"] == 4 * 64
