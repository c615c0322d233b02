"""The scalar source's entry points at the C boundary, without a device (the pattern of test_abi_scalar.py): exported
with C linkage, declared in include/iblb.h and bound in cuda_iblb_11_amd/_lib.py, refused on a NULL context with
their outputs untouched, the ctypes mirror of iblb_scalar_source equal to the header's struct, and the ABI version
unchanged (no existing struct changed layout)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from cuda_iblb_11_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["iblb_set_scalar_source", "iblb_scalar_source_info", "iblb_get_scalar_source"]


def test_the_entry_points_are_exported_unmangled():
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    names = L.header_functions()
    for n in NEW:
        assert n in exported, f"{n} not exported unmangled"
        assert n in names and n in L._SIGS, n
    assert sorted(L._SIGS) == names
    assert L.load().iblb_abi_version() == 6
    hdr = open(os.path.join(REPO, "include", "iblb.h")).read()
    assert int(re.search(r"#define IBLB_ABI_VERSION (\d+)", hdr).group(1)) == 6


def test_a_null_context_is_refused():
    lib = L.load()
    src = L.ScalarSource(None, 0.0, (C.c_void_p * 2)(None, None), (C.c_void_p * 2)(None, None))
    buf = (C.c_double * 20)(*([-7.0] * 20))
    k, m = C.c_double(-3.0), C.c_uint(77)
    assert lib.iblb_set_scalar_source(None, C.byref(src)) == L.IBLB_ERR_ARG
    assert lib.iblb_set_scalar_source(None, None) == L.IBLB_ERR_ARG
    assert lib.iblb_scalar_source_info(None, C.byref(k), C.byref(m)) == L.IBLB_ERR_ARG
    assert lib.iblb_get_scalar_source(None, buf) == L.IBLB_ERR_ARG
    assert list(buf) == [-7.0] * 20 and (k.value, m.value) == (-3.0, 77)


def test_the_source_struct_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "iblb.h"', 'int main(void) {',
             '    printf("size %zu\\n", sizeof(iblb_scalar_source));']
    for fname, _ in L.ScalarSource._fields_:
        lines.append(f'    printf("{fname} %zu\\n", offsetof(iblb_scalar_source, {fname}));')
    lines += ['    return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out if ln.strip()}
    assert got.pop("size") == C.sizeof(L.ScalarSource)
    assert list(got) == [f for f, _ in L.ScalarSource._fields_] == ["source", "decay", "wall_flux", "wall_value"]
    for fname, _ in L.ScalarSource._fields_:
        assert got[fname] == getattr(L.ScalarSource, fname).offset, fname


def test_the_present_bits_are_those_of_the_header():
    assert (L.SCALAR_SOURCE_SET, L.SCALAR_SOURCE_FIELD) == (1, 2)
    assert L.SCALAR_SOURCE_WALL_FLUX == (4, 8) and L.SCALAR_SOURCE_WALL_VALUE == (16, 32)
