"""The tracer model's entry points at the C boundary, without a device (the pattern of test_abi_scalar_uptake.py):
exported with C linkage, declared in include/iblb.h and bound in cuda_iblb_11_amd/_lib.py, refused on a NULL context
with their outputs untouched, the constants and the ctypes mirror of iblb_tracer_model equal to the header's, and the
ABI version unchanged (only new functions and one new struct)."""
import ctypes as C
import os
import re
import subprocess

from cuda_iblb_11_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["iblb_set_tracer_model", "iblb_tracer_model_info", "iblb_get_tracer_fates", "iblb_get_tracer_deposits"]


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


def test_the_constants_are_those_of_the_header():
    hdr = open(os.path.join(REPO, "include", "iblb.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define (IBLB_TRACER_[A-Z_]+)\s+(\d+)", hdr)}
    assert got == {"IBLB_TRACER_WALL_CLAMP": 0, "IBLB_TRACER_WALL_REFLECT": 1, "IBLB_TRACER_WALL_ABSORB": 2,
                   "IBLB_TRACER_ALIVE": 0, "IBLB_TRACER_AT_BOTTOM": 1, "IBLB_TRACER_AT_TOP": 2}
    assert L.TRACER_WALLS == {"clamp": 0, "reflect": 1, "absorb": 2}
    assert (L.TRACER_ALIVE, L.TRACER_AT_BOTTOM, L.TRACER_AT_TOP) == (0, 1, 2)


def test_a_null_context_is_refused():
    lib = L.load()
    m = L.TracerModel(0.5, (C.c_double * 2)(0.25, -0.25), (C.c_int * 2)(2, 1), 9)
    st = (C.c_int * 4)(*([-7] * 4))
    it = (C.c_longlong * 4)(*([-7] * 4))
    present, counts = C.c_int(77), (C.c_longlong * 3)(-5, -5, -5)
    assert lib.iblb_set_tracer_model(None, C.byref(m), None, None) == L.IBLB_ERR_ARG
    assert lib.iblb_set_tracer_model(None, None, None, None) == L.IBLB_ERR_ARG
    assert lib.iblb_tracer_model_info(None, C.byref(m), C.byref(present), counts) == L.IBLB_ERR_ARG
    assert lib.iblb_get_tracer_fates(None, st, it) == L.IBLB_ERR_ARG
    assert lib.iblb_get_tracer_deposits(None, it, it) == L.IBLB_ERR_ARG
    assert list(st) == [-7] * 4 and list(it) == [-7] * 4 and present.value == 77 and list(counts) == [-5] * 3
    assert (m.diffusivity, list(m.drift), list(m.wall), m.seed) == (0.5, [0.25, -0.25], [2, 1], 9)


def test_the_model_struct_matches_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "iblb.h"', 'int main(void) {',
             '    printf("size %zu\\n", sizeof(iblb_tracer_model));']
    for fname, _ in L.TracerModel._fields_:
        lines.append(f'    printf("{fname} %zu\\n", offsetof(iblb_tracer_model, {fname}));')
    lines += ['    return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out if ln.strip()}
    assert got.pop("size") == C.sizeof(L.TracerModel) == 40
    assert list(got) == [f for f, _ in L.TracerModel._fields_] == ["diffusivity", "drift", "wall", "seed"]
    for fname, _ in L.TracerModel._fields_:
        assert got[fname] == getattr(L.TracerModel, fname).offset, fname
