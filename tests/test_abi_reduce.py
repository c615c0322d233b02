"""The ctypes mirror of iblb_field_stats (cuda_iblb_11_amd/_lib.py FieldStats) against the C header:
size and every field's offset, from a C program compiled with gcc against include/iblb.h (the method
of test_abi.py's test_struct_layouts_match_the_header; no device needed), and the IBLB_QTY_* bits."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from cuda_iblb_11_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_field_stats_layout_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "iblb.h"', 'int main(void) {',
             '    printf("size %zu\\n", sizeof(iblb_field_stats));']
    for fname, _ in L.FieldStats._fields_:
        lines.append(f'    printf("{fname} %zu\\n", offsetof(iblb_field_stats, {fname}));')
    lines += ['    return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out if ln.strip()}
    assert got.pop("size") == C.sizeof(L.FieldStats)
    assert list(got) == [f for f, _ in L.FieldStats._fields_]
    for fname, _ in L.FieldStats._fields_:
        assert got[fname] == getattr(L.FieldStats, fname).offset, fname


def test_quantity_bits_match_the_header():
    hdr = open(os.path.join(REPO, "include", "iblb.h")).read()
    bits = {n.lower(): int(v) for n, v in re.findall(r"#define IBLB_(?:FIELD|QTY)_([A-Z]+)\s+(\d+)", hdr)}
    assert bits == L.QUANTITIES and list(L.QUANTITIES.values()) == sorted(L.QUANTITIES.values())
    assert {n: b for n, b in L.QUANTITIES.items() if b < 128} == L.FIELDS  # Lattice.fields accepts what it did
    assert int(re.search(r"#define IBLB_ABI_VERSION (\d+)", hdr).group(1)) == 6
