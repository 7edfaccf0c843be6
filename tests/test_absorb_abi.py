"""CPU checks of ellc_depth_absorb_keyframes' side of the boundary (ABI v17): the declarations, the version, the binding's lists and
structures against the C compiler's layout, the default parameters, the symbols and kernels of the two built libraries, and the new
kernels' resource usage."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("absorb_mark", "absorb_scatter", "absorb_fold", "absorb_finish")
PARAM_FIELDS = ("agree_k2", "max_fold", "photo_gate", "src_validity", "finalise")


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_symbol_is_declared_bound_built_and_versioned():
    import __graft_entry__ as g
    g.build()
    from egomotion_with_local_loop_closures_amd import _lib, api
    for name in ("ellc_depth_absorb_keyframes", "ellc_absorb_default_params"):
        assert name in _lib.ABI_SYMBOLS and name not in _lib.DIAG_SYMBOLS
    assert "ellc_profile_depth_absorb" in _lib.DIAG_SYMBOLS and "ellc_profile_depth_absorb" not in _lib.ABI_SYMBOLS
    header = open(os.path.join(ROOT, "include", "ellc_abi.h")).read()
    assert re.search(r"ellc_status\s+ellc_depth_absorb_keyframes\s*\(", header) and re.search(r"void\s+ellc_absorb_default_params\s*\(", header)
    assert re.search(r"}\s*ellc_absorb_params;", header) and re.search(r"}\s*ellc_absorb_stats;", header)
    assert int(re.search(r"#define ELLC_ABI_VERSION (\d+)", header).group(1)) >= 17
    diag_header = open(os.path.join(ROOT, "include", "ellc_abi_diag.h")).read()
    assert re.search(r"ellc_status\s+ellc_profile_depth_absorb\s*\(", diag_header) and "ellc_profile_depth_absorb" not in header
    assert _lib.lib().ellc_abi_version() >= 17
    assert hasattr(_lib.lib(), "ellc_depth_absorb_keyframes") and hasattr(_lib.diag_lib(), "ellc_depth_absorb_keyframes")
    assert callable(api.Context.depth_absorb) and callable(api.Context.profile_depth_absorb) and callable(api.absorb_params)
    ship, diag = exported(_lib.SO_PATH), exported(_lib.DIAG_SO_PATH)
    for name in ("ellc_depth_absorb_keyframes", "ellc_absorb_default_params"):
        assert name in ship and name in diag
    assert "ellc_profile_depth_absorb" in diag and "ellc_profile_depth_absorb" not in ship
    # the fusion's entry point and kernels are still there beside the new ones
    assert "ellc_keyframe_fuse_depth" in ship
    so = open(_lib.SO_PATH, "rb").read()
    for kernel in (b"absorb_mark", b"absorb_scatter", b"absorb_fold", b"absorb_finish", b"fuse_agree", b"fuse_offsets", b"fuse_scatter", b"fuse_merge"):
        assert kernel in so, kernel


def test_structures_match_the_compilers_layout(tmp_path):
    from egomotion_with_local_loop_closures_amd import _lib
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ellc_abi.h"', 'int main(void) {',
             '  printf("params %zu\\n", sizeof(ellc_absorb_params)); printf("stats %zu\\n", sizeof(ellc_absorb_stats));']
    lines += ['  printf("params.%s %%zu\\n", offsetof(ellc_absorb_params, %s));' % (f, f) for f in PARAM_FIELDS]
    lines += ['  printf("stats.%s %%zu\\n", offsetof(ellc_absorb_stats, %s));' % (f, f) for f in _lib.ABSORB_STATS_FIELDS]
    lines += ['  return 0;', '}']
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["params"]) == C.sizeof(_lib.EllcAbsorbParams) == 20 and int(got["stats"]) == C.sizeof(_lib.EllcAbsorbStats) == 64
    assert tuple(n for n, _ in _lib.EllcAbsorbParams._fields_) == PARAM_FIELDS
    for f in PARAM_FIELDS:
        assert int(got["params." + f]) == getattr(_lib.EllcAbsorbParams, f).offset, f
    for k, f in enumerate(_lib.ABSORB_STATS_FIELDS):
        assert int(got["stats." + f]) == getattr(_lib.EllcAbsorbStats, f).offset == 4 * k, f
    assert len(_lib.ABSORB_STATS_FIELDS) == 16 and _lib.ABSORB_STATS_FIELDS[-1] == "reserved"


def test_default_parameters():
    import __graft_entry__ as g
    g.build()
    from egomotion_with_local_loop_closures_amd import _lib, api
    p = _lib.EllcAbsorbParams(-1.0, -1, -1, -1, -1)
    _lib.lib().ellc_absorb_default_params(C.byref(p))
    assert (p.agree_k2, p.max_fold, p.photo_gate, p.src_validity, p.finalise) == (1.0, 64, 1, 20, 1)
    _lib.lib().ellc_absorb_default_params(None)   # a NULL is ignored
    q = api.absorb_params(max_fold=2, finalise=0)
    assert (q.agree_k2, q.max_fold, q.photo_gate, q.src_validity, q.finalise) == (1.0, 2, 1, 20, 0)
    header = open(os.path.join(ROOT, "include", "ellc_abi.h")).read()
    assert int(re.search(r"#define ELLC_FUSE_MAX_MERGE (\d+)", header).group(1)) == p.max_fold


def test_new_kernels_have_no_scratch_and_no_spills(tmp_path):
    """As every kernel of the library: a private segment of 0 and no spilled register (the code object's own metadata, read with the
    toolchain that built it)."""
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
    for kernel in KERNELS + ("sim3_pass", "fuse_merge"):   # (the two whose source this change touched or shares code with)
        found = [v for k, v in kernels.items() if kernel in k]
        assert len(found) == 1, (kernel, sorted(kernels)[:5])
        print(kernel, found[0])
        assert found[0]["private_segment_fixed_size"] == 0 and found[0]["vgpr_spill_count"] == 0 and found[0]["sgpr_spill_count"] == 0, (kernel, found[0])


def test_header_is_c99(tmp_path):
    c = tmp_path / "abi.c"
    c.write_text('#include "ellc_abi.h"\nint main(void) { ellc_map_filter f; ellc_absorb_params p; ellc_absorb_stats s; int k = 0; float T[12] = {0}; '
                 'f.stride = 1; ellc_absorb_default_params(&p); s.reserved = 0; return (int)ellc_depth_absorb_keyframes(0, 1, &k, T, &f, &p, &s) + s.reserved; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(c)])
