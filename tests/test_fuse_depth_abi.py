"""CPU checks of ellc_keyframe_fuse_depth's side of the boundary (ABI v16): the declaration, the version, the binding's lists, the
symbols and kernels of the two built libraries, the new kernels' resource usage, and the header / facade still plain C99 / C++11."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("fuse_agree", "fuse_tile_sums", "fuse_offsets", "fuse_scatter", "fuse_merge", "fuse_finish")


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_symbol_is_declared_bound_built_and_versioned():
    import __graft_entry__ as g
    g.build()
    from egomotion_with_local_loop_closures_amd import _lib, api
    assert "ellc_keyframe_fuse_depth" in _lib.ABI_SYMBOLS and "ellc_keyframe_fuse_depth" not in _lib.DIAG_SYMBOLS
    assert "ellc_profile_fuse_depth" in _lib.DIAG_SYMBOLS and "ellc_profile_fuse_depth" not in _lib.ABI_SYMBOLS
    header = open(os.path.join(ROOT, "include", "ellc_abi.h")).read()
    assert re.search(r"ellc_status\s+ellc_keyframe_fuse_depth\s*\(", header)
    assert re.search(r"#define ELLC_FUSE_MAX_MERGE 64\b", header)
    assert int(re.search(r"#define ELLC_ABI_VERSION (\d+)", header).group(1)) >= 16
    diag_header = open(os.path.join(ROOT, "include", "ellc_abi_diag.h")).read()
    assert re.search(r"ellc_status\s+ellc_profile_fuse_depth\s*\(", diag_header) and "ellc_profile_fuse_depth" not in header
    assert _lib.lib().ellc_abi_version() >= 16
    assert hasattr(_lib.lib(), "ellc_keyframe_fuse_depth") and hasattr(_lib.diag_lib(), "ellc_keyframe_fuse_depth")
    assert callable(api.Context.fuse_depth) and callable(api.Context.profile_fuse_depth)
    ship, diag = exported(_lib.SO_PATH), exported(_lib.DIAG_SO_PATH)
    assert "ellc_keyframe_fuse_depth" in ship and "ellc_keyframe_fuse_depth" in diag
    assert "ellc_profile_fuse_depth" in diag and "ellc_profile_fuse_depth" not in ship
    # the render's entry point and kernels are still there beside the new ones
    assert "ellc_keyframe_render_depth" in ship
    so = open(_lib.SO_PATH, "rb").read()
    for kernel in (b"fuse_offsets", b"fuse_scatter", b"fuse_merge", b"render_min", b"render_resolve", b"render_finish", b"render_agree"):
        assert kernel in so, kernel


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
            kernels[name.group(1)] = {k: int(v) for k, v in re.findall(r"^\s*\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\d+)\s*$",
                                                                         block, flags=re.M)}
    for kernel in KERNELS:
        found = [v for k, v in kernels.items() if kernel in k]
        assert len(found) == 1, (kernel, sorted(kernels)[:5])
        print(kernel, found[0])
        assert found[0]["private_segment_fixed_size"] == 0 and found[0]["vgpr_spill_count"] == 0 and found[0]["sgpr_spill_count"] == 0, (kernel, found[0])


def test_header_is_c99_and_the_facade_cxx11(tmp_path):
    c = tmp_path / "abi.c"
    c.write_text('#include "ellc_abi.h"\nint main(void) { ellc_map_filter f; int s = 0; float T[12] = {0}; f.stride = 1; '
                 'return (int)ellc_keyframe_fuse_depth(0, 1, &s, T, 0, &f, 1.0f, ELLC_FUSE_MAX_MERGE, -1, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(c)])
    cc = tmp_path / "facade.cpp"
    cc.write_text('#include "ellc_facade.hpp"\n'
                  'void use(ellc::globalOptimize& g, const ellc_map_filter& f, const float* pose, ellc::frame* into) { ellc::FusedView v; '
                  'g.fuseLocalMap(pose, 0, f, 1.0f, ELLC_FUSE_MAX_MERGE, into, v); ellc::write_pfm("depth.pfm", v.depth, v.cols, v.rows); '
                  'ellc::RenderedView& r = v; (void)r; (void)v.merged.size(); (void)v.n_fused; (void)v.max_merge; }\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(cc)])
