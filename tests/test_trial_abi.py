"""CPU checks of ellc_keyframe_trial_propagate's and ellc_depth_restart_from_keyframes' side of the boundary (ABI v18): the declarations,
the version, the binding's lists and structure against the C compiler's layout, the symbols and kernels of the two built libraries, and
the resource usage of the new kernels and of the two kernels of the absorb that share code with them."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ellc_keyframe_trial_propagate", "ellc_depth_restart_from_keyframes")
HOOK = "ellc_profile_trial_propagate"
KERNELS = ("trial_pass", "trial_finish", "absorb_wipe", "absorb_mark", "absorb_fold")
FIELDS = ("sum_r2", "sum_abs_r", "n_kept", "n_in_view", "n_interior", "n_low_grad", "n_candidates", "n_targets", "reserved")
OFFSETS = (0, 8, 16, 20, 24, 28, 32, 36, 40)


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_symbols_are_declared_bound_built_and_versioned():
    import __graft_entry__ as g
    g.build()
    from egomotion_with_local_loop_closures_amd import _lib, api
    for name in NEW:
        assert name in _lib.ABI_SYMBOLS and name not in _lib.DIAG_SYMBOLS
    assert HOOK in _lib.DIAG_SYMBOLS and HOOK not in _lib.ABI_SYMBOLS
    header = open(os.path.join(ROOT, "include", "ellc_abi.h")).read()
    for name in NEW:
        assert re.search(r"ellc_status\s+%s\s*\(" % name, header), name
    assert re.search(r"}\s*ellc_trial_propagation;", header)
    assert int(re.search(r"#define ELLC_ABI_VERSION (\d+)", header).group(1)) >= 18
    diag_header = open(os.path.join(ROOT, "include", "ellc_abi_diag.h")).read()
    assert re.search(r"ellc_status\s+%s\s*\(" % HOOK, diag_header) and HOOK not in header
    assert _lib.lib().ellc_abi_version() >= 18 and _lib.diag_lib().ellc_abi_version() == _lib.lib().ellc_abi_version()
    for name in NEW:
        assert hasattr(_lib.lib(), name) and hasattr(_lib.diag_lib(), name)
    assert hasattr(_lib.diag_lib(), HOOK) and not hasattr(_lib.lib(), HOOK)
    assert callable(api.Context.trial_propagate) and callable(api.Context.depth_restart) and callable(api.Context.profile_trial_propagate)
    ship, diag = exported(_lib.SO_PATH), exported(_lib.DIAG_SO_PATH)
    for name in NEW:
        assert name in ship and name in diag
    assert HOOK in diag and HOOK not in ship
    # the absorb's entry point and kernels are still there beside the new ones
    assert "ellc_depth_absorb_keyframes" in ship
    so = open(_lib.SO_PATH, "rb").read()
    for kernel in (b"trial_pass", b"trial_finish", b"absorb_wipe", b"absorb_mark", b"absorb_scatter", b"absorb_fold", b"absorb_finish"):
        assert kernel in so, kernel


def test_structure_matches_the_compilers_layout(tmp_path):
    import numpy as np
    from egomotion_with_local_loop_closures_amd import _lib
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ellc_abi.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(ellc_trial_propagation));']
    lines += ['  printf("%s %%zu\\n", offsetof(ellc_trial_propagation, %s));' % (f, f) for f in FIELDS]
    lines += ['  return 0;', '}']
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_lib.EllcTrialPropagation) == np.dtype(_lib.EllcTrialPropagation).itemsize == 48
    assert tuple(n for n, _ in _lib.EllcTrialPropagation._fields_) == FIELDS
    for f, off in zip(FIELDS, OFFSETS):
        assert int(got[f]) == getattr(_lib.EllcTrialPropagation, f).offset == off, f
    assert _lib.EllcTrialPropagation.reserved.size == 8   # reserved[2]


def test_new_kernels_have_no_scratch_and_no_spills(tmp_path):
    """As every kernel of the library: a private segment of 0 and no spilled register (the code object's own metadata, read with the
    toolchain that built it), for the new kernels and for absorb_mark / absorb_fold, whose gate the trial pass shares."""
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
        assert len(found) == 1, (kernel, sorted(kernels)[:5])
        print(kernel, found[0])
        assert found[0]["private_segment_fixed_size"] == 0 and found[0]["vgpr_spill_count"] == 0 and found[0]["sgpr_spill_count"] == 0, (kernel, found[0])


def test_header_is_c99(tmp_path):
    c = tmp_path / "abi.c"
    c.write_text('#include "ellc_abi.h"\n#include "ellc_abi_diag.h"\nint main(void) { ellc_map_filter f; ellc_absorb_params p; ellc_absorb_stats s; '
                 'ellc_trial_propagation r; int k = 0; float T[12] = {0}; float factor = 0.0f, ms = 0.0f; f.stride = 1; r.reserved[1] = 0; s.reserved = 0; '
                 'ellc_absorb_default_params(&p); return (int)ellc_keyframe_trial_propagate(0, 1, &k, 0, &k, T, &f, 1, &r) + '
                 '(int)ellc_profile_trial_propagate(0, 1, &k, 1, &k, T, &f, 1, &r, 0, &ms) + '
                 '(int)ellc_depth_restart_from_keyframes(0, 1, 1, &k, T, &f, &p, &factor, &s) + r.reserved[1] + s.reserved; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(c)])
