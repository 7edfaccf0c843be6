"""CPU checks of the affine-brightness side of the boundary (ABI v19): the declarations, the version, the binding's lists, the symbols
and kernels of the two built libraries, the two structs as the C compiler sees them against the ctypes mirrors, the header still
plain C99, the new kernels' scratch and spills in the shipping code object, and ellc_light_solve - against numpy's least squares
and refusal by refusal."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import light_reference as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["sum_w", "sum_w_s", "sum_w_t", "sum_w_ss", "sum_w_st", "sum_w_tt", "chi2_photo", "n_kept", "n_in_view", "n_photo", "n_photo_huber"]
PARAM_FIELDS = ["gain_min", "gain_max", "min_pixels"]
PRODUCT = ["ellc_keyframe_light_step", "ellc_keyframe_sim3_step_lit", "ellc_keyframe_sim3_align_lit", "ellc_light_default_params", "ellc_light_solve"]
DIAG = ["ellc_profile_light_step", "ellc_profile_sim3_step_lit"]
KERNELS = ("light_pass", "light_finish")   # (ellc_keyframe_sim3_step_lit runs sim3_pass / sim3_finish: tests/test_sim3_abi.py holds those)


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
    assert int(re.search(r"#define ELLC_ABI_VERSION (\d+)", header).group(1)) >= 19
    assert _lib.lib().ellc_abi_version() >= 19
    for name in ("light_step", "sim3_step_lit", "sim3_align_lit", "profile_light_step", "profile_sim3_step_lit"):
        assert callable(getattr(api.Context, name))
    assert callable(api.light_solve) and callable(api.light_params)
    ship, diag = exported(_lib.SO_PATH), exported(_lib.DIAG_SO_PATH)
    assert set(PRODUCT) <= ship and set(PRODUCT) <= diag
    assert set(DIAG) <= diag and not set(DIAG) & ship
    so = open(_lib.SO_PATH, "rb").read()
    for kernel in KERNELS:
        assert kernel.encode() in so, kernel
    p = api.light_params()
    assert (p.gain_min, p.gain_max, p.min_pixels) == (0.25, 4.0, 16)
    assert api.light_params(min_pixels=1 << 30).min_pixels == 1 << 30


def test_layouts_match_the_header(tmp_path, api):
    from egomotion_with_local_loop_closures_amd import _lib
    cls, prm = _lib.EllcLightNormal, _lib.EllcLightParams
    assert [f[0] for f in cls._fields_] == FIELDS and [f[0] for f in prm._fields_] == PARAM_FIELDS
    lines = ['#include "ellc_abi.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {",
             '  printf("size %zu\\n", sizeof(ellc_light_normal));', '  printf("params %zu\\n", sizeof(ellc_light_params));']
    for f in FIELDS:
        lines.append('  printf("%s %%zu %%zu\\n", offsetof(ellc_light_normal, %s), sizeof(((ellc_light_normal*)0)->%s));' % (f, f, f))
    for f in PARAM_FIELDS:
        lines.append('  printf("%s %%zu %%zu\\n", offsetof(ellc_light_params, %s), sizeof(((ellc_light_params*)0)->%s));' % (f, f, f))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    seen = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert seen["size"] == [72] and ctypes.sizeof(cls) == 72
    assert seen["params"] == [12] and ctypes.sizeof(prm) == 12
    dt = np.dtype(cls)
    assert dt.itemsize == 72 and list(dt.names) == FIELDS and api.LIGHT_NORMAL_DTYPE == dt
    for f in FIELDS:
        d = getattr(cls, f)
        assert seen[f] == [d.offset, d.size], f
        assert d.offset % d.size == 0, f   # every field naturally aligned
        assert dt.fields[f][1] == d.offset and dt.fields[f][0].itemsize == d.size, f
    assert seen["chi2_photo"] == [48, 8] and seen["n_photo_huber"] == [68, 4]
    for f in PARAM_FIELDS:
        d = getattr(prm, f)
        assert seen[f] == [d.offset, d.size], f


def test_header_is_c99_and_the_facade_cxx11(tmp_path):
    c = tmp_path / "abi.c"
    c.write_text('#include "ellc_abi.h"\nint main(void) { ellc_map_filter f; ellc_sim3_params p; ellc_light_params lp; ellc_sim3_normal r; ellc_light_normal lr; '
                 'int s = 0, it = 0; float T[12] = {0}, l[2] = {1, 0}; f.stride = 1; ellc_sim3_default_params(&p); ellc_light_default_params(&lp); '
                 'lr.n_photo = 0; (void)ellc_light_solve(&lr, &lp, 0, l); '
                 '(void)ellc_keyframe_sim3_align_lit(0, 1, &s, &s, T, l, 0, 0, &f, &p, &lp, 10, 1e-4f, T, l, &r, &lr, &it, 0, 0, 0, 0, 0); '
                 '(void)ellc_keyframe_light_step(0, 1, &s, &s, T, l, 0, &f, &p, &lr); '
                 'return (int)ellc_keyframe_sim3_step_lit(0, 1, &s, &s, T, 0, 0, &f, &p, &r); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(c)])
    cc = tmp_path / "facade.cpp"
    cc.write_text('#include "ellc_facade.hpp"\n'
                  'double use(ellc::globalOptimize& g) { g.refineMatchSim3 = true; g.matchAffineLight = true; double s = 0; '
                  'for (size_t i = 0; i < g.lastMatchSim3.size(); i++) s += g.lastMatchSim3[i].gain + g.lastMatchSim3[i].offset; return s; }\n'
                  'int main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(cc)])


def test_kernels_have_no_scratch_and_no_spills(tmp_path, api):
    """The metadata check of tests/test_sim3_abi.py on the two light kernels: each exactly once in the gfx950 code object of the
    shipping library, with a private segment of 0 and no spilled registers."""
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
    for kernel in KERNELS:
        found = [v for k, v in kernels.items() if kernel in k]
        assert len(found) == 1, (kernel, sorted(kernels)[:5])
        print(kernel, found[0])
        assert found[0]["private_segment_fixed_size"] == 0 and found[0]["vgpr_spill_count"] == 0 and found[0]["sgpr_spill_count"] == 0, (kernel, found[0])


def record(api, Is, Iw, w, n_photo=None):
    """The light record of pixels (Is, Iw) with weights w, the sums in double."""
    r = np.zeros(1, api.LIGHT_NORMAL_DTYPE)
    r["sum_w"] = w.sum(); r["sum_w_s"] = (w * Is).sum(); r["sum_w_t"] = (w * Iw).sum()
    r["sum_w_ss"] = (w * Is * Is).sum(); r["sum_w_st"] = (w * Is * Iw).sum(); r["sum_w_tt"] = (w * Iw * Iw).sum()
    r["n_photo"] = Is.size if n_photo is None else n_photo
    return r


def test_solve_against_numpy_lstsq(api):
    """Twenty seeded weighted systems (grey values 0..255, gains 0.3..3.5, offsets -100..100, noise, weights 1/16 down to 1/160):
    gain within 1e-9 relative and offset within 1e-9 * 255 of numpy.linalg.lstsq on sqrt(w) [Is 1] x = sqrt(w) Iw; the result is those
    doubles rounded to f32 once, and tests/light_reference.solve agrees bit for bit."""
    rng = np.random.default_rng(19)
    for k in range(20):
        n = int(rng.integers(16, 3000))
        Is = rng.integers(0, 256, n).astype(np.float64)
        g, o = rng.uniform(0.3, 3.5), rng.uniform(-100, 100)
        Iw = g * Is + o + rng.normal(0, 3.0, n)
        w = rng.uniform(0.1, 1.0, n) / 16.0
        rec = record(api, Is, Iw, w)
        got, refused = api.light_solve(rec)
        sq = np.sqrt(w)
        want = np.linalg.lstsq(np.stack([Is, np.ones(n)], 1) * sq[:, None], Iw * sq, rcond=None)[0]
        assert not refused, k
        # (the comparison is made on the doubles behind the f32 result: an f32 ulp of a gain is 6e-8 relative)
        sw, ss, st, sss, sst = (float(rec[f][0]) for f in ("sum_w", "sum_w_s", "sum_w_t", "sum_w_ss", "sum_w_st"))
        gain = (sw * sst - ss * st) / (sw * sss - ss * ss)
        offset = (st - gain * ss) / sw
        assert abs(gain - want[0]) <= 1e-9 * abs(want[0]) and abs(offset - want[1]) <= 1e-9 * 255, (k, gain, offset, want)
        assert got.tobytes() == np.array([gain, offset], np.float32).tobytes(), (k, got, gain, offset)
        ref, ref_refused = LR.solve(rec[0])
        assert not ref_refused and np.array(ref, np.float32).tobytes() == got.tobytes()


def test_every_refusal_of_the_solve(api):
    rng = np.random.default_rng(20)
    Is = rng.integers(0, 256, 200).astype(np.float64)
    Iw = 0.5 * Is + 30
    w = np.full(200, 1 / 16.0)
    good = record(api, Is, Iw, w)
    light_in = np.array([0.9, 3.0], np.float32)

    def refused(rec, params=None, lin=light_in):
        got, r = api.light_solve(rec, lin, params)
        want = np.array([1, 0], np.float32) if lin is None else lin
        assert r and got.tobytes() == want.tobytes(), (got, r)
        assert LR.solve(rec[0], want, params)[1]

    got, r = api.light_solve(good, light_in)
    assert not r and abs(got[0] - 0.5) < 1e-6 and abs(got[1] - 30) < 1e-4
    got, r = api.light_solve(good, None, dict(min_pixels=200))
    assert not r and abs(got[0] - 0.5) < 1e-6
    refused(good, dict(min_pixels=201)); refused(good, dict(min_pixels=1 << 30)); refused(good, dict(min_pixels=201), lin=None)   # too few pixels
    refused(record(api, np.full(200, 77.0), Iw, w))                                        # a constant source: det = 0
    refused(record(api, np.zeros(200), Iw, w)); refused(record(api, Is, Iw, np.zeros(200)))   # ... an all-black one; no weight at all
    for f in ("sum_w", "sum_w_s", "sum_w_t", "sum_w_ss", "sum_w_st"):                       # NaN fails every test
        bad = good.copy(); bad[f] = np.nan
        refused(bad)
    refused(good, dict(gain_min=0.6)); refused(record(api, Is, 3.0 * Is, w), dict(gain_max=2.5))   # gain outside the range
    refused(record(api, Is, 5.0 * Is, w)); refused(record(api, Is, 0.2 * Is, w))                  # ... outside the default range
    assert not api.light_solve(record(api, Is, 4.0 * Is, w))[1] and not api.light_solve(record(api, Is, 0.25 * Is, w))[1]   # its edges are inside
    refused(record(api, Is, Is + 256.0, w)); refused(record(api, Is, Is - 256.0, w))              # |offset| > 255
    assert not api.light_solve(record(api, Is, Is + 255.0, w))[1]
