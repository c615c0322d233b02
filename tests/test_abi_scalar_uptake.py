"""The scalar uptake's entry points at the C boundary, without a device (the pattern of test_abi_scalar_source.py):
exported with C linkage, declared in include/iblb.h and bound in cuda_iblb_11_amd/_lib.py, refused on a NULL context
with their outputs untouched, the ctypes mirror of iblb_scalar_uptake equal to the header's struct, and the ABI version
unchanged (no existing struct changed layout)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from cuda_iblb_11_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["iblb_set_scalar_uptake", "iblb_get_scalar_uptake", "iblb_reset_scalar_uptake", "iblb_scalar_uptake_info"]


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
    # the wall kinds stay the two of iblb_set_scalar: a reactive wall is a no-flux wall with a rate
    assert sorted(set(re.findall(r"#define (IBLB_SCALAR_WALL_[A-Z]+)", hdr))) == ["IBLB_SCALAR_WALL_NOFLUX",
                                                                                   "IBLB_SCALAR_WALL_VALUE"]


def test_a_null_context_is_refused():
    lib = L.load()
    up = L.ScalarUptake((C.c_void_p * 2)(None, None))
    bufs = [(C.c_double * 20)(*([-7.0] * 20)) for _ in range(4)]
    m, n = C.c_uint(77), C.c_longlong(-5)
    assert lib.iblb_set_scalar_uptake(None, C.byref(up)) == L.IBLB_ERR_ARG
    assert lib.iblb_set_scalar_uptake(None, None) == L.IBLB_ERR_ARG
    assert lib.iblb_get_scalar_uptake(None, *bufs, C.byref(n)) == L.IBLB_ERR_ARG
    assert lib.iblb_reset_scalar_uptake(None) == L.IBLB_ERR_ARG
    assert lib.iblb_scalar_uptake_info(None, C.byref(m), C.byref(n)) == L.IBLB_ERR_ARG
    assert all(list(b) == [-7.0] * 20 for b in bufs) and (m.value, n.value) == (77, -5)


def test_the_uptake_struct_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "iblb.h"', 'int main(void) {',
             '    printf("size %zu\\n", sizeof(iblb_scalar_uptake));']
    for fname, _ in L.ScalarUptake._fields_:
        lines.append(f'    printf("{fname} %zu\\n", offsetof(iblb_scalar_uptake, {fname}));')
    lines += ['    return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out if ln.strip()}
    assert got.pop("size") == C.sizeof(L.ScalarUptake)
    assert list(got) == [f for f, _ in L.ScalarUptake._fields_] == ["rate"]
    for fname, _ in L.ScalarUptake._fields_:
        assert got[fname] == getattr(L.ScalarUptake, fname).offset, fname


def test_the_present_bits_are_those_of_the_header():
    assert L.SCALAR_UPTAKE_SET == 1 and L.SCALAR_UPTAKE_RATE == (2, 4)
