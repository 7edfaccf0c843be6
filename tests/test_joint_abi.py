"""CPU checks of the joint refinement's side of the boundary (ABI v23): the declarations, the version, the binding's lists, the symbols
and kernels of the two built libraries, the structs as the C compiler sees them against the ctypes mirrors, the header still plain
C99, the default parameters, ellc_joint_solve on the library itself, and the code-object metadata of the new kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import joint_reference as J
import refine_depth_reference as R
from map_points_reference import level_intrinsics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PRODUCT = ["ellc_keyframe_joint_step", "ellc_joint_solve", "ellc_keyframe_joint_apply", "ellc_keyframe_joint_refine", "ellc_joint_default_params"]
DIAG = ["ellc_profile_joint_step", "ellc_profile_joint_apply"]
KERNELS = ["joint_pixels", "joint_count_finish", "joint_pairs", "joint_pair_finish", "joint_apply_pixels"]
PARAM_FIELDS = ["sigma_i2", "huber_k", "prior_weight", "max_step_rel", "min_views"]
NORMAL_FIELDS = ["A", "a", "S", "s", "chi2_photo", "chi2_prior", "n_terms", "n_kept", "n_taking_part", "n_used", "n_too_few_views", "n_no_information", "B",
                 "n_view_terms"]
APPLY_FIELDS = ["n_kept", "n_taking_part", "n_stepped", "n_too_few_views", "n_no_information", "n_bad_step", "reserved"]


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
    for name in DIAG:
        assert name in _lib.DIAG_SYMBOLS and name not in _lib.ABI_SYMBOLS
        assert re.search(r"ellc_status\s+%s\s*\(" % name, diag_header) and name not in header
    assert int(re.search(r"#define ELLC_ABI_VERSION (\d+)", header).group(1)) >= 23
    assert _lib.lib().ellc_abi_version() >= 23
    assert re.search(r"#define ELLC_JOINT_MAX_VIEWS 8\b", header) and _lib.JOINT_MAX_VIEWS == 8 == J.MAX_VIEWS
    for k, name in enumerate(("NOT_TAKING_PART", "STEPPED", "TOO_FEW_VIEWS", "NO_INFORMATION", "BAD_STEP")):
        assert re.search(r"ELLC_JOINT_%s = %d\b" % (name, k), header), name
        assert _lib.JOINT_STATUS[k] == name and getattr(J, name) == k
    for name in ("joint_step", "joint_apply", "joint_refine", "profile_joint_step", "profile_joint_apply"):
        assert callable(getattr(api.Context, name))
    assert callable(api.joint_default_params) and callable(api.joint_solve)
    ship, diag = exported(_lib.SO_PATH), exported(_lib.DIAG_SO_PATH)
    assert set(PRODUCT) <= ship and set(PRODUCT) <= diag
    assert set(DIAG) <= diag and not set(DIAG) & ship
    so = open(_lib.SO_PATH, "rb").read()
    for kernel in KERNELS:
        assert kernel.encode() in so, kernel


def test_default_params(api):
    p = api.joint_default_params()
    r = api.refine_default_params()
    assert (p.sigma_i2, p.huber_k, p.prior_weight, p.max_step_rel, p.min_views) == (r.sigma_i2, r.huber_k, r.prior_weight, r.max_step_rel, r.min_views)
    assert (p.sigma_i2, p.huber_k, p.prior_weight, p.max_step_rel, p.min_views) == (16.0, F(1.345), 1.0, 0.5, 2)
    q = api.joint_default_params(min_views=1, prior_weight=0.0)
    assert (q.min_views, q.prior_weight, q.max_step_rel) == (1, 0.0, 0.5)
    assert J.DEFAULT_PARAMS == dict(sigma_i2=16.0, huber_k=1.345, prior_weight=1.0, max_step_rel=0.5, min_views=2)


def test_struct_layouts_match_header(tmp_path, api):
    from egomotion_with_local_loop_closures_amd import _lib
    structs = (("ellc_joint_params", _lib.EllcJointParams, PARAM_FIELDS, 20), ("ellc_joint_normal", _lib.EllcJointNormal, NORMAL_FIELDS, 11600),
               ("ellc_joint_apply_stats", _lib.EllcJointApplyStats, APPLY_FIELDS, 32))
    lines = ['#include "ellc_abi.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {"]
    for st, cls, fields, size in structs:
        assert [f[0] for f in cls._fields_] == fields
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        for f in fields:
            lines.append('  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (st, f, st, f, st, f))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    seen = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    for st, cls, fields, size in structs:
        assert seen[st] == [size] and ctypes.sizeof(cls) == size, st
        for f in fields:
            d = getattr(cls, f)
            assert seen["%s.%s" % (st, f)] == [d.offset, d.size], (st, f)
    for f, off in (("a", 1344), ("S", 1728), ("s", 11136), ("chi2_photo", 11520), ("n_terms", 11536), ("n_kept", 11544), ("B", 11564), ("n_view_terms", 11568)):
        assert seen["ellc_joint_normal." + f][0] == off, f
    assert api.JOINT_NORMAL_DTYPE.itemsize == 11600


def test_header_is_c99_and_the_facade_cxx11(tmp_path):
    c = tmp_path / "abi.c"
    c.write_text('#include "ellc_abi.h"\nint main(void) { ellc_map_filter f; ellc_joint_params p; static ellc_joint_normal r; ellc_joint_apply_stats st; '
                 'int s = 0, it = 0; float T[12] = {0}; double xi[6] = {0}; f.stride = 1; ellc_joint_default_params(&p); st.n_kept = 0; '
                 'ellc_joint_status q = ELLC_JOINT_STEPPED; (void)q; (void)ellc_joint_solve(&r, 0.0, xi); '
                 '(void)ellc_keyframe_joint_step(0, 0, 0, 1, 1, &s, T, 0, &f, &p, 0, &r); '
                 '(void)ellc_keyframe_joint_apply(0, 0, 0, 1, 1, &s, T, 0, &f, &p, 0, xi, -1, T, 0, 0, 0, 0, 0, &st); '
                 'return (int)ellc_keyframe_joint_refine(0, 0, 0, 1, 1, &s, T, 0, &f, &p, 0, 6, 0.0f, 0.0, -1, T, &r, &it, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(c)])
    cc = tmp_path / "facade.cpp"
    cc.write_text('#include "ellc_facade.hpp"\n'
                  'double use(ellc::globalOptimize& g) { g.refineMatchSim3 = true; g.refineMatchJoint = true; g.joint_matches_file.open("joint.txt"); '
                  'return g.lastJointRecord.n_used + g.lastJointRecord.chi2_prior + g.lastJointViews + g.lastJointIters; }\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(cc)])


def record_of(api, M, g, rng=None):
    """An ellc_joint_normal whose reduced system is (M, g): H = blockdiag(A) - S, b = a - s, the diagonal blocks split at random between
    A and S where rng is given, everything in S otherwise."""
    n = g.size
    rec = np.zeros(1, api.JOINT_NORMAL_DTYPE)
    rec["B"] = n // 6
    for i in range(n):
        for j in range(i, n):
            part = 0.0
            if i // 6 == j // 6 and rng is not None:
                part = rng.uniform(-1, 2) * M[i, j]
                rec["A"][0][i // 6][J.tri(6, i % 6, j % 6)] = part
            rec["S"][0][J.tri(n, i, j)] = part - M[i, j]
        part = rng.uniform(-1, 2) * g[i] if rng is not None else 0.0
        rec["a"][0][i // 6][i % 6] = part
        rec["s"][0][i] = part - g[i]
    return rec[0]


def test_joint_solve_against_numpy(api):
    """Random symmetric positive definite systems of 6, 18 and 48 unknowns and the recorded systems of the reference on a small world (1, 3
    and 8 views): the library's L D L^T in double against numpy.linalg.solve. Cholesky-type factorisations are backward stable: the
    solution moves by at most about n^2 2^-53 cond |xi|; 64 n cond 2^-53 |xi| is asserted (n <= 48)."""
    rng = np.random.default_rng(23)
    worst = 0.0

    def check(rec, lam, what):
        nonlocal worst
        xi, refused = api.joint_solve(rec, lam)
        want, ref_refused = J.solve(rec, lam)
        assert not refused and not ref_refused, what
        H, _ = J.reduced_system(rec)
        H[np.diag_indices(H.shape[0])] *= 1.0 + lam
        bound = 64 * H.shape[0] * np.linalg.cond(H) * 2.0 ** -53 * np.abs(want).max()
        dist = np.abs(xi - want).max()
        assert xi.shape == want.shape and dist <= bound, (what, dist, bound)
        worst = max(worst, dist / bound)

    for n in (6, 18, 48):
        for trial in range(4):
            Q = rng.normal(size=(n, n + 3))
            M = Q @ Q.T + 0.1 * np.eye(n)
            g = rng.normal(size=n)
            check(record_of(api, M, g, rng if trial % 2 else None), (0.0, 0.5)[trial // 2], "random %d" % n)
    from map_points_reference import make_scene
    scenes = [make_scene(23, 17, s) for s in (11, 12, 13)]
    kf = (scenes[0]["depth0"], scenes[0]["var0"], scenes[0]["kf_image"])
    intr = level_intrinsics(*scenes[0]["intrinsics"], 0)
    for B in (1, 3, 8):
        Ts = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F), (B, 1))
        for b in range(B):
            Ts[b][3] = 0.01 * (b + 1); Ts[b][7] = -0.008 * (b % 3); Ts[b][11] = 0.02 * (b % 2)
        ref = J.step(kf, [scenes[(b + 1) % 3]["kf_image"] for b in range(B)], intr, Ts, None, R.FILTERS[0], dict(min_views=1))
        rec = np.zeros(1, api.JOINT_NORMAL_DTYPE)
        for name in J.SUMS + ("chi2_photo", "chi2_prior", "B"):
            rec[name][0] = ref[name]
        check(rec[0], 1e-3, "recorded %d" % (6 * B))
    print("largest distance / bound %.3g" % worst)


def test_a_singular_record_is_refused_and_nothing_is_written(api):
    from egomotion_with_local_loop_closures_amd import _lib
    rng = np.random.default_rng(24)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    Q = rng.normal(size=(18, 18))
    good = Q @ Q.T + np.eye(18)
    cases = []
    low = rng.normal(size=(18, 5))
    cases.append(("rank 5", low @ low.T, 0.0, 3))
    cases.append(("zero", np.zeros((18, 18)), 0.0, 3))
    neg = good.copy(); neg[7, 7] = -1.0
    cases.append(("negative pivot", neg, 0.0, 3))
    nan = good.copy(); nan[2, 3] = nan[3, 2] = np.nan
    cases.append(("nan", nan, 0.0, 3))
    inf = good.copy(); inf[0, 0] = np.inf
    cases.append(("inf", inf, 0.0, 3))
    cases.append(("negative lambda", good, -0.5, 3))
    cases.append(("nan lambda", good, np.nan, 3))
    cases.append(("B = 0", good, 0.0, 0))
    cases.append(("B = 9", good, 0.0, 9))
    for what, M, lam, B in cases:
        rec = np.ascontiguousarray(np.asarray(record_of(api, M, rng.normal(size=18))).reshape(1))
        rec["B"] = B
        xi = np.full(72, 7.25)
        assert _lib.lib().ellc_joint_solve(p(rec), ctypes.c_double(lam), p(xi)) != 0, what
        assert (xi == 7.25).all(), what
        assert J.solve(rec[0], lam)[1] if 1 <= B <= 8 and lam >= 0 else True, what
    rec = np.ascontiguousarray(np.asarray(record_of(api, good, rng.normal(size=18))).reshape(1))
    xi = np.full(72, 7.25)
    assert _lib.lib().ellc_joint_solve(p(rec), ctypes.c_double(0.0), p(xi)) == 0 and (xi[18:] == 7.25).all() and not (xi[:18] == 7.25).any()
    assert _lib.lib().ellc_joint_solve(None, ctypes.c_double(0.0), p(xi)) != 0 and _lib.lib().ellc_joint_solve(p(rec), ctypes.c_double(0.0), None) != 0


def test_kernels_have_no_scratch_and_no_spills(tmp_path, api):
    """The gfx950 code object of the shipping library holds the five kernels with a private segment of 0 and no spilled registers (the
    code object's own metadata, as tests/test_refine_depth_abi.py reads it)."""
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
    for kernel in KERNELS:
        found = [v for k, v in kernels.items() if kernel in k]
        assert len(found) == 1, (kernel, sorted(kernels)[:5])
        print(kernel, found[0])
        assert found[0]["private_segment_fixed_size"] == 0 and found[0]["vgpr_spill_count"] == 0 and found[0]["sgpr_spill_count"] == 0, (kernel, found[0])
