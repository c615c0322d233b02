"""The scalar gauges' entry points at the C boundary, without a device (the pattern of test_abi_scalar_ends.py): exported
with C linkage, declared in include/iblb.h and bound in cuda_iblb_11_amd/_lib.py, refused on a NULL context with their
outputs untouched, the ctypes mirror of iblb_scalar_gauges equal to the header's struct, and the ABI version unchanged
(no existing struct changed layout)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from cuda_iblb_11_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["iblb_set_scalar_gauges", "iblb_get_scalar_gauges", "iblb_reset_scalar_gauges", "iblb_scalar_gauges_info"]


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
    st, lv = (C.c_int * 2)(0, 3), (C.c_int * 1)(2)
    ga = L.ScalarGauges(2, C.addressof(st), 1, C.addressof(lv))
    bufs = [(C.c_double * 20)(*([-7.0] * 20)) for _ in range(4)]
    ns, nl, n = C.c_int(-3), C.c_int(-4), C.c_longlong(-5)
    pos = [(C.c_int * 4)(-9, -9, -9, -9) for _ in range(2)]
    assert lib.iblb_set_scalar_gauges(None, C.byref(ga)) == L.IBLB_ERR_ARG
    assert lib.iblb_set_scalar_gauges(None, None) == L.IBLB_ERR_ARG
    assert lib.iblb_get_scalar_gauges(None, *bufs, C.byref(n)) == L.IBLB_ERR_ARG
    assert lib.iblb_reset_scalar_gauges(None) == L.IBLB_ERR_ARG
    assert lib.iblb_scalar_gauges_info(None, C.byref(ns), pos[0], C.byref(nl), pos[1], C.byref(n)) == L.IBLB_ERR_ARG
    assert all(list(b) == [-7.0] * 20 for b in bufs) and (ns.value, nl.value, n.value) == (-3, -4, -5)
    assert all(list(p) == [-9] * 4 for p in pos)
    assert list(st) == [0, 3] and list(lv) == [2]


def test_the_gauges_struct_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "iblb.h"', 'int main(void) {',
             '    printf("size %zu\\n", sizeof(iblb_scalar_gauges));']
    for fname, _ in L.ScalarGauges._fields_:
        lines.append(f'    printf("{fname} %zu\\n", offsetof(iblb_scalar_gauges, {fname}));')
    lines += ['    return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out if ln.strip()}
    assert got.pop("size") == C.sizeof(L.ScalarGauges)
    assert list(got) == [f for f, _ in L.ScalarGauges._fields_] == ["n_stations", "station", "n_levels", "level"]
    for fname, _ in L.ScalarGauges._fields_:
        assert got[fname] == getattr(L.ScalarGauges, fname).offset, fname
