"""CPU checks of the Sim(3) refinement's side of the boundary (ABI v15): the declarations, the version, the binding's lists, the symbols
and kernels of the two built libraries, the record as the C compiler sees it against the ctypes mirror, the header / facade still plain
C99 / C++11, and the two host helpers - ellc_sim3_apply against scipy's expm, ellc_sim3_solve against numpy's solve."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.linalg import expm

import sim3_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["H", "b", "chi2_photo", "chi2_depth", "n_kept", "n_in_view", "n_photo", "n_photo_huber", "n_depth", "n_depth_gated"]
PRODUCT = ["ellc_keyframe_sim3_step", "ellc_keyframe_sim3_align", "ellc_sim3_default_params", "ellc_sim3_solve", "ellc_sim3_apply"]


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
    assert "ellc_profile_sim3_step" in _lib.DIAG_SYMBOLS and "ellc_profile_sim3_step" not in _lib.ABI_SYMBOLS
    assert re.search(r"ellc_status\s+ellc_profile_sim3_step\s*\(", diag_header) and "ellc_profile_sim3_step" not in header
    assert int(re.search(r"#define ELLC_ABI_VERSION (\d+)", header).group(1)) >= 15
    assert _lib.lib().ellc_abi_version() >= 15
    for name in ("sim3_step", "sim3_align", "profile_sim3_step"):
        assert callable(getattr(api.Context, name))
    assert callable(api.sim3_solve) and callable(api.sim3_apply)
    ship, diag = exported(_lib.SO_PATH), exported(_lib.DIAG_SO_PATH)
    assert set(PRODUCT) <= ship and set(PRODUCT) <= diag
    assert "ellc_profile_sim3_step" in diag and "ellc_profile_sim3_step" not in ship
    so = open(_lib.SO_PATH, "rb").read()
    for kernel in (b"sim3_pass", b"sim3_finish"):
        assert kernel in so, kernel
    p = api.sim3_params()
    assert (p.sigma_i2, p.huber_k, p.gate_k2, p.depth_weight) == (16.0, np.float32(1.345), 9.0, 1.0)
    assert api.sim3_params(gate_k2=4.0).gate_k2 == 4.0


def test_record_layout_matches_header(tmp_path, api):
    from egomotion_with_local_loop_closures_amd import _lib
    cls = _lib.EllcSim3Normal
    assert [f[0] for f in cls._fields_] == FIELDS
    lines = ['#include "ellc_abi.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {",
             '  printf("size %zu\\n", sizeof(ellc_sim3_normal));', '  printf("params %zu\\n", sizeof(ellc_sim3_params));']
    for f in FIELDS:
        lines.append('  printf("%s %%zu %%zu\\n", offsetof(ellc_sim3_normal, %s), sizeof(((ellc_sim3_normal*)0)->%s));' % (f, f, f))
    for f in ("sigma_i2", "huber_k", "gate_k2", "depth_weight"):
        lines.append('  printf("%s %%zu %%zu\\n", offsetof(ellc_sim3_params, %s), sizeof(((ellc_sim3_params*)0)->%s));' % (f, f, f))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    seen = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert seen["size"] == [320] and ctypes.sizeof(cls) == 320
    dt = np.dtype(cls)
    assert dt.itemsize == 320 and list(dt.names) == FIELDS and api.SIM3_NORMAL_DTYPE == dt
    for f in FIELDS:
        d = getattr(cls, f)
        assert seen[f] == [d.offset, d.size], f
        element = 8 if f in ("H", "b") else d.size
        assert d.offset % element == 0, f   # every field naturally aligned
        assert dt.fields[f][1] == d.offset and dt.fields[f][0].itemsize == d.size, f
    assert seen["H"] == [0, 224] and seen["b"] == [224, 56] and seen["n_depth_gated"] == [316, 4]
    assert seen["params"] == [16] and ctypes.sizeof(_lib.EllcSim3Params) == 16
    for f in ("sigma_i2", "huber_k", "gate_k2", "depth_weight"):
        d = getattr(_lib.EllcSim3Params, f)
        assert seen[f] == [d.offset, d.size], f


def test_header_is_c99_and_the_facade_cxx11(tmp_path):
    c = tmp_path / "abi.c"
    c.write_text('#include "ellc_abi.h"\nint main(void) { ellc_map_filter f; ellc_sim3_params p; ellc_sim3_normal r; int s = 0, it = 0; float T[12] = {0}; '
                 'double xi[7]; f.stride = 1; ellc_sim3_default_params(&p); r.n_kept = 0; (void)ellc_sim3_solve(&r, xi); ellc_sim3_apply(xi, T, T); '
                 '(void)ellc_keyframe_sim3_align(0, 1, &s, &s, T, 0, 0, &f, &p, 10, 1e-4f, T, &r, &it, 0, 0, 0); '
                 'return (int)ellc_keyframe_sim3_step(0, 1, &s, &s, T, 0, &f, &p, &r); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(c)])
    cc = tmp_path / "facade.cpp"
    cc.write_text('#include "ellc_facade.hpp"\n'
                  'double use(ellc::globalOptimize& g) { g.refineMatchSim3 = true; g.match_sim3_file.open("sim3.txt"); '
                  'double s = 0; for (size_t i = 0; i < g.lastMatchSim3.size(); i++) s += g.lastMatchSim3[i].scale * g.lastMatchSim3[i].rec.n_photo '
                  '+ g.lastMatchSim3[i].T[3] + g.lastMatchSim3[i].iters; return s; }\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(cc)])


def test_apply_against_scipy_expm(api):
    """Every entry within 2^-23 max |T| of float64 expm(xi^) T for twenty seeded xi with |xi|_inf <= 0.3; xi = 0 returns T's bits."""
    rng = np.random.default_rng(15)
    T = S.scene_transforms(1.0)[1].copy()
    T[:9:4] *= np.float32(1.3); T[1:10:4] *= np.float32(1.3); T[2:11:4] *= np.float32(1.3)   # a similarity: the 3x3 block scaled
    for k in range(20):
        xi = rng.uniform(-0.3, 0.3, 7)
        got = api.sim3_apply(xi, T)
        want = (expm(S.generator(xi)) @ np.vstack([T.reshape(3, 4).astype(np.float64), [0, 0, 0, 1]]))[:3].reshape(12)
        err = np.abs(got.astype(np.float64) - want).max()
        assert err <= 2.0 ** -23 * np.abs(want).max(), (k, err)
        T = got   # the next one starts where this one ended
    assert api.sim3_apply(np.zeros(7), T).tobytes() == T.tobytes()
    assert api.sim3_apply(np.zeros(7), S.scene_transforms(2.0)[2]).tobytes() == S.scene_transforms(2.0)[2].tobytes()


def record(api, A, b):
    r = np.zeros(1, api.SIM3_NORMAL_DTYPE)
    r["H"][0] = A[np.triu_indices(7)]
    r["b"][0] = b
    return r


def test_solve_against_numpy(api):
    """Seeded symmetric positive definite systems with condition numbers up to 1e6: relative 1e-9 against numpy.linalg.solve."""
    rng = np.random.default_rng(16)
    for k in range(20):
        Q, _ = np.linalg.qr(rng.normal(size=(7, 7)))
        ev = 10.0 ** rng.uniform(0, 6, 7); ev[0] = 1.0; ev[1] = 10.0 ** (6 * k / 19.0)
        A = (Q * ev) @ Q.T
        A = 0.5 * (A + A.T)
        assert np.linalg.cond(A) <= 1e6 * (1 + 1e-9)
        b = rng.normal(size=7) * ev.max()
        xi, singular = api.sim3_solve(record(api, A, b))
        want = np.linalg.solve(A, -b)
        assert not singular and np.abs(xi - want).max() <= 1e-9 * np.abs(want).max(), (k, xi, want)
        ref, ref_singular = S.solve(A[np.triu_indices(7)], b)
        assert not ref_singular and np.abs(ref - want).max() <= 1e-9 * np.abs(want).max()


def test_solve_reports_the_singular_case(api):
    rng = np.random.default_rng(17)
    A = rng.normal(size=(7, 7)); A = A @ A.T + np.eye(7)
    b = rng.normal(size=7)
    assert not api.sim3_solve(record(api, A, b))[1]
    for z in (6, 2, 0):   # a zero row (and column: H is symmetric)
        Z = A.copy(); Z[z, :] = 0; Z[:, z] = 0
        xi, singular = api.sim3_solve(record(api, Z, b))
        assert singular and not xi.any(), z
        assert S.solve(Z[np.triu_indices(7)], b)[1]
    xi, singular = api.sim3_solve(record(api, np.zeros((7, 7)), b))
    assert singular and not xi.any()
    N = A.copy(); N[3, 3] = np.nan
    assert api.sim3_solve(record(api, N, b))[1]


def test_kernels_have_no_scratch_and_no_spills(tmp_path, api):
    """sim3_pass carries 34 double accumulators per thread: the gfx950 code object of the shipping library must hold both kernels with a
    private segment of 0 and no spilled registers (the code object's own metadata, read with the toolchain that built it)."""
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
            kernels[name.group(1)] = {k: int(v) for k, v in re.findall(r"^\s*\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\d+)\s*$",
                                                                         block, flags=re.M)}
    for kernel in ("sim3_pass", "sim3_finish"):
        found = [v for k, v in kernels.items() if kernel in k]
        assert len(found) == 1, (kernel, sorted(kernels)[:5])
        print(kernel, found[0])
        assert found[0]["private_segment_fixed_size"] == 0 and found[0]["vgpr_spill_count"] == 0 and found[0]["sgpr_spill_count"] == 0, (kernel, found[0])
