"""CPU checks of the v24 side of the boundary (affine brightness in the absorb, the trial propagation and the restart): the declarations,
the version, the binding's lists and the 96-byte record against the C compiler's layout, the header as C99 and C++11, the resource usage
of the touched kernels, and ellc_trial_light_solve against ellc_light_solve on the equivalent ellc_light_normal."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ellc_depth_absorb_keyframes_lit", "ellc_depth_restart_from_keyframes_lit", "ellc_keyframe_trial_propagate_lit")
SOLVE = "ellc_trial_light_solve"
KERNELS = ("absorb_mark", "trial_pass", "trial_finish", "trial_lit_pass", "trial_lit_finish")
FIELDS = ("sum_r2", "sum_abs_r", "n_kept", "n_in_view", "n_interior", "n_low_grad", "n_candidates", "n_targets", "reserved",
          "sum_s", "sum_t", "sum_ss", "sum_st", "sum_tt", "n_fit", "reserved2")
OFFSETS = (0, 8, 16, 20, 24, 28, 32, 36, 40, 48, 56, 64, 72, 80, 88, 92)


def test_symbols_are_declared_bound_built_and_versioned():
    import __graft_entry__ as g
    g.build()
    from egomotion_with_local_loop_closures_amd import _lib, api
    header = open(os.path.join(ROOT, "include", "ellc_abi.h")).read()
    for name in NEW + (SOLVE,):
        assert name in _lib.ABI_SYMBOLS and name not in _lib.DIAG_SYMBOLS
        assert re.search(r"(ellc_status|int)\s+%s\s*\(" % name, header), name
        assert hasattr(_lib.lib(), name) and hasattr(_lib.diag_lib(), name)
    assert re.search(r"}\s*ellc_trial_propagation_lit;", header)
    assert int(re.search(r"#define ELLC_ABI_VERSION (\d+)", header).group(1)) >= 24
    assert _lib.lib().ellc_abi_version() >= 24 and _lib.diag_lib().ellc_abi_version() == _lib.lib().ellc_abi_version()
    assert callable(api.Context.trial_propagate_lit) and callable(api.trial_light_solve)
    import inspect
    assert "lights" in inspect.signature(api.Context.depth_absorb).parameters and "lights" in inspect.signature(api.Context.depth_restart).parameters
    so = open(_lib.SO_PATH, "rb").read()
    for kernel in KERNELS:
        assert kernel.encode() in so, kernel


def test_record_matches_the_compilers_layout(tmp_path):
    from egomotion_with_local_loop_closures_amd import _lib, api
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ellc_abi.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(ellc_trial_propagation_lit));']
    lines += ['  printf("%s %%zu\\n", offsetof(ellc_trial_propagation_lit, %s));' % (f, f) for f in FIELDS]
    lines += ['  printf("narrow_%s %%zu\\n", offsetof(ellc_trial_propagation, %s));' % (f, f) for f in FIELDS[:9]]
    lines += ['  return 0;', '}']
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_lib.EllcTrialPropagationLit) == api.TRIAL_LIT_DTYPE.itemsize == 96
    assert tuple(n for n, _ in _lib.EllcTrialPropagationLit._fields_) == FIELDS
    for f, off in zip(FIELDS, OFFSETS):
        assert int(got[f]) == getattr(_lib.EllcTrialPropagationLit, f).offset == api.TRIAL_LIT_DTYPE.fields[f][1] == off, f
        assert off % getattr(_lib.EllcTrialPropagationLit, f).size == 0 or f == "reserved", f   # naturally aligned
    for f in FIELDS[:9]:   # the first 48 bytes are an ellc_trial_propagation
        assert got["narrow_" + f] == got[f], f


def test_touched_kernels_have_no_scratch_and_no_spills(tmp_path):
    """A private segment of 0 and no spilled register, from the code object's own metadata, for absorb_mark (the gate takes the light)
    and both instances of the trial pass and its finish."""
    import __graft_entry__ as g
    g.build()
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
            kernels[name.group(1)] = {k: int(v) for k, v in re.findall(r"^\s*\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count|sgpr_count):\s+(\d+)\s*$",
                                                                         block, flags=re.M)}
    for kernel in KERNELS:
        found = [v for k, v in kernels.items() if kernel in k]
        assert len(found) == 1, (kernel, [k for k in kernels if "trial" in k or "absorb" in k])
        print(kernel, found[0])
        assert found[0]["private_segment_fixed_size"] == 0 and found[0]["vgpr_spill_count"] == 0 and found[0]["sgpr_spill_count"] == 0, (kernel, found[0])


PROGRAM = ('#include "ellc_abi.h"\nint main(void) { ellc_map_filter f; ellc_absorb_params p; ellc_absorb_stats s; ellc_light_params lp; '
           'ellc_trial_propagation_lit r; int k = 0; float T[12] = {0}; float light[2] = {1.0f, 0.0f}; float factor = 0.0f; f.stride = 1; r.reserved2 = 0; '
           's.reserved = 0; ellc_absorb_default_params(&p); ellc_light_default_params(&lp); '
           'return (int)ellc_keyframe_trial_propagate_lit(0, 1, &k, 0, &k, T, light, &f, 1, &r) + '
           '(int)ellc_depth_absorb_keyframes_lit(0, 1, &k, T, light, &f, &p, &s) + '
           '(int)ellc_depth_restart_from_keyframes_lit(0, 1, 1, &k, T, light, &f, &p, &factor, &s) + '
           'ellc_trial_light_solve(&r, &lp, light, light) + r.reserved2 + s.reserved; }\n')


def test_header_is_c99_and_cxx11(tmp_path):
    c = tmp_path / "abi.c"
    c.write_text(PROGRAM)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(c)])
    cc = tmp_path / "abi.cpp"
    cc.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(cc)])


def test_trial_light_solve_is_light_solve_of_the_equivalent_normal():
    """Same bits, same return, accepted and refused: host only, no device."""
    from egomotion_with_local_loop_closures_amd import api
    rng = np.random.default_rng(5)

    def record(n, gain, offset, spread=60.0):
        Is = rng.uniform(128 - spread, 128 + spread, n).astype(np.float32).astype(np.float64)
        Iw = (gain * Is + offset + rng.normal(0, 2, n)).astype(np.float32).astype(np.float64)
        rec = np.zeros(1, api.TRIAL_LIT_DTYPE)
        rec["n_kept"] = n + 7; rec["n_in_view"] = n + 3; rec["n_interior"] = n; rec["n_fit"] = n
        rec["sum_s"] = Is.sum(); rec["sum_t"] = Iw.sum(); rec["sum_ss"] = (Is * Is).sum(); rec["sum_st"] = (Is * Iw).sum(); rec["sum_tt"] = (Iw * Iw).sum()
        rec["sum_r2"] = 12345.0   # (not read by the solve)
        return rec

    cases = [(record(500, 1.6, -20), None, None, False), (record(500, 0.7, 15), (1.2, 3.0), None, False),
             (record(10, 1.1, 2), (1.2, 3.0), None, True),                       # fewer than min_pixels
             (record(500, 5.0, 0), None, None, True),                            # gain above gain_max
             (record(500, 5.0, 0), None, dict(gain_max=8.0), False),
             (record(500, 1.0, 0, spread=0.0), (0.9, 1.0), None, True),          # no spread in Is: det fails
             (record(500, 1.0, 300), None, None, True),                          # |offset| > 255
             (np.zeros(1, api.TRIAL_LIT_DTYPE), (1.5, -2.0), None, True)]        # an empty record
    for rec, light_in, params, refused in cases:
        normal = np.zeros(1, api.LIGHT_NORMAL_DTYPE)
        normal["sum_w"] = float(rec["n_fit"][0])
        for a, b in (("sum_w_s", "sum_s"), ("sum_w_t", "sum_t"), ("sum_w_ss", "sum_ss"), ("sum_w_st", "sum_st"), ("sum_w_tt", "sum_tt")):
            normal[a] = rec[b]
        normal["n_photo"] = rec["n_fit"]
        want, want_refused = api.light_solve(normal[0], light_in, params)
        got, got_refused = api.trial_light_solve(rec[0], light_in, params)
        assert got.tobytes() == want.tobytes() and got_refused == want_refused == refused, (got, want, got_refused, refused)
        if refused:
            assert got.tobytes() == np.asarray(light_in if light_in is not None else (1, 0), np.float32).tobytes()
