"""The scalar ends' entry points at the C boundary, without a device (the pattern of test_abi_scalar_uptake.py): exported
with C linkage, declared in include/iblb.h and bound in cuda_iblb_11_amd/_lib.py, refused on a NULL context with their
outputs untouched, the ctypes mirror of iblb_scalar_ends equal to the header's struct, the kinds and present bits those
of the header, and the ABI version unchanged (no existing struct changed layout)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from cuda_iblb_11_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["iblb_set_scalar_ends", "iblb_get_scalar_ends", "iblb_reset_scalar_ends", "iblb_scalar_ends_info"]


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


def test_the_kinds_and_present_bits_are_those_of_the_header():
    hdr = open(os.path.join(REPO, "include", "iblb.h")).read()
    kinds = dict(re.findall(r"#define (IBLB_SCALAR_END_[A-Z]+)\s+(\d+)", hdr))
    assert kinds == {"IBLB_SCALAR_END_NOFLUX": "0", "IBLB_SCALAR_END_VALUE": "1", "IBLB_SCALAR_END_OUTFLOW": "2"}
    assert (L.SCALAR_END_NOFLUX, L.SCALAR_END_VALUE, L.SCALAR_END_OUTFLOW) == (0, 1, 2)
    assert L.SCALAR_END_KINDS == {"noflux": 0, "value": 1, "outflow": 2}
    assert L.SCALAR_ENDS_SET == 1 and L.SCALAR_ENDS_PROFILE == (2, 4)


def test_a_null_context_is_refused():
    lib = L.load()
    ends = L.ScalarEnds((C.c_int * 2)(1, 2), (C.c_double * 2)(0.5, 0.0), (C.c_void_p * 2)(None, None))
    bufs = [(C.c_double * 20)(*([-7.0] * 20)) for _ in range(4)]
    kind, value = (C.c_int * 2)(-3, -4), (C.c_double * 2)(-7.0, -8.0)
    m, n = C.c_uint(77), C.c_longlong(-5)
    assert lib.iblb_set_scalar_ends(None, C.byref(ends)) == L.IBLB_ERR_ARG
    assert lib.iblb_set_scalar_ends(None, None) == L.IBLB_ERR_ARG
    assert lib.iblb_get_scalar_ends(None, *bufs, C.byref(n)) == L.IBLB_ERR_ARG
    assert lib.iblb_reset_scalar_ends(None) == L.IBLB_ERR_ARG
    assert lib.iblb_scalar_ends_info(None, kind, value, C.byref(m), C.byref(n)) == L.IBLB_ERR_ARG
    assert all(list(b) == [-7.0] * 20 for b in bufs) and (m.value, n.value) == (77, -5)
    assert list(kind) == [-3, -4] and list(value) == [-7.0, -8.0]


def test_the_ends_struct_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "iblb.h"', 'int main(void) {',
             '    printf("size %zu\\n", sizeof(iblb_scalar_ends));']
    for fname, _ in L.ScalarEnds._fields_:
        lines.append(f'    printf("{fname} %zu\\n", offsetof(iblb_scalar_ends, {fname}));')
    lines += ['    return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out if ln.strip()}
    assert got.pop("size") == C.sizeof(L.ScalarEnds)
    assert list(got) == [f for f, _ in L.ScalarEnds._fields_] == ["kind", "value", "profile"]
    for fname, _ in L.ScalarEnds._fields_:
        assert got[fname] == getattr(L.ScalarEnds, fname).offset, fname
