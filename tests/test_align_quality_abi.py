"""CPU checks of ellc_align_quality_at's side of the boundary (ABI v11): the record's layout as the C compiler sees the header
against the ctypes mirror, the symbol in the binding's list, and the header still plain C99."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quality_record_layout_matches_header(tmp_path):
    """sizeof / offsetof of ellc_align_quality (the method of test_struct_layouts_match_header)."""
    from egomotion_with_local_loop_closures_amd import _lib
    fields = [f[0] for f in _lib.EllcAlignQuality._fields_]
    assert fields == ["n_depth", "n_used", "sum_r2", "sum_abs_r", "sum_w", "sum_wr2", "H", "b", "Hinv"]
    lines = ['#include "ellc_abi.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {",
             '  printf("ellc_align_quality %zu\\n", sizeof(ellc_align_quality));']
    for f in fields:
        lines.append('  printf("%s %%zu %%zu\\n", offsetof(ellc_align_quality, %s), sizeof(((ellc_align_quality*)0)->%s));' % (f, f, f))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    seen = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert seen["ellc_align_quality"] == [ctypes.sizeof(_lib.EllcAlignQuality)]
    for f in fields:
        d = getattr(_lib.EllcAlignQuality, f)
        assert seen[f] == [d.offset, d.size], f
    # the counts are 32-bit integers, the four sums doubles, the matrices f32
    assert _lib.EllcAlignQuality.n_used.size == 4 and _lib.EllcAlignQuality.sum_wr2.size == 8 and _lib.EllcAlignQuality.Hinv.size == 36 * 4


def test_symbol_is_declared_bound_and_versioned():
    import re
    from egomotion_with_local_loop_closures_amd import _lib, api
    assert "ellc_align_quality_at" in _lib.ABI_SYMBOLS and "ellc_align_quality_at" not in _lib.DIAG_SYMBOLS
    header = open(os.path.join(ROOT, "include", "ellc_abi.h")).read()
    assert re.search(r"ellc_status\s+ellc_align_quality_at\s*\(", header)
    assert int(re.search(r"#define ELLC_ABI_VERSION (\d+)", header).group(1)) >= 11
    assert callable(api.Context.align_quality)


def test_header_with_the_record_is_c99(tmp_path):
    c = tmp_path / "abi.c"
    c.write_text('#include "ellc_abi.h"\nint main(void) { ellc_align_quality q; q.n_used = 0; (void)q; return ELLC_OK; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(c)])
    cc = tmp_path / "facade.cpp"
    cc.write_text('#include "ellc_facade.hpp"\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(cc)])
