"""The passive scalar's entry points at the C boundary, without a device: exported with C linkage, declared in
include/iblb.h and bound in cuda_iblb_11_amd/_lib.py, refused on a NULL context with their outputs untouched, the
ctypes mirror of iblb_scalar equal to the header's struct (size and every offset, from a C program compiled with
gcc: the method of test_abi.py), and the ABI version unchanged (no existing struct changed layout)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from cuda_iblb_11_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["iblb_set_scalar", "iblb_get_scalar", "iblb_get_scalar_populations", "iblb_scalar_info"]


def test_the_entry_points_are_exported_unmangled():
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    names = L.header_functions()
    for n in NEW:
        assert n in exported, f"{n} not exported unmangled"
        assert n in names and n in L._SIGS, n
    assert sorted(L._SIGS) == names
    assert L.load().iblb_abi_version() == 6


def test_a_null_context_is_refused():
    lib = L.load()
    cfg = L.Scalar(0.8, 1, (C.c_int * 2)(0, 0), (C.c_double * 2)(0.0, 0.0))
    buf = (C.c_double * 20)(*([-7.0] * 20))
    w = L.Window(0, 0, 2, 2, 1, 1)
    n = C.c_longlong(-3)
    assert lib.iblb_set_scalar(None, C.byref(cfg), buf, None) == L.IBLB_ERR_ARG
    assert lib.iblb_set_scalar(None, None, None, None) == L.IBLB_ERR_ARG
    assert lib.iblb_get_scalar(None, C.byref(w), buf) == L.IBLB_ERR_ARG
    assert lib.iblb_get_scalar(None, None, buf) == L.IBLB_ERR_ARG
    assert lib.iblb_get_scalar_populations(None, buf) == L.IBLB_ERR_ARG
    info = L.Scalar(-3.0, -3, (C.c_int * 2)(-3, -3), (C.c_double * 2)(-3.0, -3.0))
    assert lib.iblb_scalar_info(None, C.byref(info), C.byref(n)) == L.IBLB_ERR_ARG
    assert list(buf) == [-7.0] * 20 and n.value == -3
    assert (info.tau, info.stride, list(info.wall_kind), list(info.wall_value)) == (-3.0, -3, [-3, -3], [-3.0, -3.0])


def test_the_scalar_struct_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "iblb.h"', 'int main(void) {',
             '    printf("size %zu\\n", sizeof(iblb_scalar));']
    for fname, _ in L.Scalar._fields_:
        lines.append(f'    printf("{fname} %zu\\n", offsetof(iblb_scalar, {fname}));')
    lines += ['    return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out if ln.strip()}
    assert got.pop("size") == C.sizeof(L.Scalar)
    assert list(got) == [f for f, _ in L.Scalar._fields_] == ["tau", "stride", "wall_kind", "wall_value"]
    for fname, _ in L.Scalar._fields_:
        assert got[fname] == getattr(L.Scalar, fname).offset, fname


def test_the_wall_kinds_match_the_header():
    hdr = open(os.path.join(REPO, "include", "iblb.h")).read()
    kinds = {n: int(v) for n, v in re.findall(r"#define IBLB_SCALAR_WALL_([A-Z]+)\s+(\d+)", hdr)}
    assert kinds == {"NOFLUX": L.SCALAR_WALL_NOFLUX, "VALUE": L.SCALAR_WALL_VALUE} == {"NOFLUX": 0, "VALUE": 1}
    assert int(re.search(r"#define IBLB_ABI_VERSION (\d+)", hdr).group(1)) == 6
