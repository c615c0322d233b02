"""The scalar's fields and iblb_get_scalar_wall_flux at the C boundary, without a device: the entry point exported
with C linkage, declared in include/iblb.h and bound in cuda_iblb_11_amd/_lib.py, refused on a NULL context with its
outputs untouched; READ_FIELDS and SCALAR_FIELDS equal to the header's values, from a C program compiled with gcc
(the method of test_fields_ref.py); _lib.FIELDS still the fluid's seven."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from cuda_iblb_11_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_wall_flux_is_exported_unmangled():
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    n = "iblb_get_scalar_wall_flux"
    assert n in exported and n in L.header_functions() and n in L._SIGS
    assert sorted(L._SIGS) == L.header_functions()
    assert L.load().iblb_abi_version() == 6


def test_a_null_context_is_refused():
    buf = (C.c_double * 8)(*([-7.0] * 8))
    assert L.load().iblb_get_scalar_wall_flux(None, buf, buf) == L.IBLB_ERR_ARG
    assert list(buf) == [-7.0] * 8


def test_the_field_tables_match_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include "iblb.h"', 'int main(void) {']
    for name in L.READ_FIELDS:
        lines.append(f'    printf("{name} %d\\n", IBLB_FIELD_{name.upper()});')
    lines += ['    return 0;', '}']
    src = tmp_path / "bits.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "bits"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out if ln.strip()}
    assert got == L.READ_FIELDS and list(got) == list(L.READ_FIELDS)
    assert L.SCALAR_FIELDS == {"c": 4096, "cux": 8192, "cuy": 16384}
    assert L.READ_FIELDS == {**L.FIELDS, **L.SCALAR_FIELDS}
    assert list(L.READ_FIELDS.values()) == sorted(L.READ_FIELDS.values())
    # iblb_reduce_fields takes them after its own four quantities; 2048 is no bit anywhere
    assert list(L.QUANTITIES)[-3:] == list(L.SCALAR_FIELDS) and 2048 not in L.QUANTITIES.values()
    assert len(L.QUANTITIES) == 14


def test_the_fluid_fields_are_still_the_seven():
    assert L.FIELDS == {"rho": 1, "ux": 2, "uy": 4, "vort": 8, "sxx": 16, "sxy": 32, "syy": 64}
    assert list(L.FIELDS) == ["rho", "ux", "uy", "vort", "sxx", "sxy", "syy"]
