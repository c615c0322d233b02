"""iblb_save_checkpoint_ex and iblb_checkpoint_info at the C boundary, without a device (the pattern of
test_abi_scalar_gauges.py): exported with C linkage, declared in include/iblb.h and bound in cuda_iblb_11_amd/_lib.py,
the IBLB_CKPT_* constants of the header equal to Python's, the ABI version unchanged, and iblb_checkpoint_info driven
on files this test writes from the documented format (tests/ckpt_format_ref.py): a fluid part for a 4 x 3 lattice
with zeros for populations, with and without hand-made sections."""
import ctypes as C
import os
import re
import subprocess

import pytest

import ckpt_format_ref as ref
import cuda_iblb_11_amd as P
from cuda_iblb_11_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["iblb_save_checkpoint_ex", "iblb_checkpoint_info"]
FLUID = ref.fluid_part(4, 3, t=17)
END = ref.section(ref.END)


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


def test_the_constants_match_the_header():
    hdr = open(os.path.join(REPO, "include", "iblb.h")).read()
    got = {n: int(v) for n, v in re.findall(r"#define IBLB_CKPT_([A-Z]+)\s+(\d+)", hdr)}
    assert got == {"SCALAR": L.CKPT_SCALAR, "TRACERS": L.CKPT_TRACERS, "AVERAGE": L.CKPT_AVERAGE, "OBSERVERS": L.OBSERVERS}
    assert got == {"SCALAR": 1, "TRACERS": 2, "AVERAGE": 4, "OBSERVERS": 7}
    assert L.OBSERVERS == L.CKPT_SCALAR | L.CKPT_TRACERS | L.CKPT_AVERAGE
    assert (P.CKPT_SCALAR, P.CKPT_TRACERS, P.CKPT_AVERAGE, P.OBSERVERS) == (1, 2, 4, 7)
    assert ref.BITS == (L.CKPT_SCALAR, L.CKPT_TRACERS, L.CKPT_AVERAGE)


def test_a_null_context_or_path_is_refused(tmp_path):
    lib = L.load()
    step, obs = C.c_longlong(-3), C.c_uint(99)
    assert lib.iblb_save_checkpoint_ex(None, os.fsencode(tmp_path / "x.ck"), L.OBSERVERS) == L.IBLB_ERR_ARG
    assert not os.listdir(tmp_path)
    assert lib.iblb_checkpoint_info(None, C.byref(step), C.byref(obs)) == L.IBLB_ERR_ARG
    assert lib.iblb_checkpoint_info(os.fsencode(tmp_path / "missing.ck"), C.byref(step), C.byref(obs)) == L.IBLB_ERR_ARG
    assert (step.value, obs.value) == (-3, 99)
    with pytest.raises(P.IblbError) as e:
        P.checkpoint_info(tmp_path / "missing.ck")
    assert e.value.code == L.IBLB_ERR_ARG


GOOD = {
    "fluid only": (FLUID, 0),
    "end alone": (FLUID + END, 0),
    "scalar": (FLUID + ref.section(ref.SCALAR, bytes(24)) + END, 1),
    "tracers": (FLUID + ref.section(ref.TRACERS, bytes(5)) + END, 2),
    "average": (FLUID + ref.section(ref.AVERAGE) + END, 4),
    "scalar and average": (FLUID + ref.section(ref.SCALAR, bytes(3)) + ref.section(ref.AVERAGE, bytes(9)) + END, 5),
    "all": (FLUID + b"".join(ref.section(k, bytes(8 * k)) for k in (ref.SCALAR, ref.TRACERS, ref.AVERAGE)) + END, 7),
    "f32 with points": (ref.fluid_part(4, 3, prec=1, t=17, ns=6) + ref.section(ref.TRACERS, b"ab") + END, 2),
}
BAD = {
    "empty": b"",
    "not a checkpoint": b"IBLBCK02" + FLUID[8:],
    "another version": FLUID[:8] + (2).to_bytes(8, "little") + FLUID[16:],
    "cut in the header": FLUID[:60],
    "cut in the populations": FLUID[:-8],
    "no end section": FLUID + ref.section(ref.SCALAR, bytes(24)),
    "unknown tag": FLUID + ref.section(ref.SCALAR, bytes(4), tag=b"IBLBFOO1") + END,
    "out of order": FLUID + ref.section(ref.AVERAGE) + ref.section(ref.SCALAR) + END,
    "duplicated": FLUID + ref.section(ref.TRACERS) + ref.section(ref.TRACERS) + END,
    "length past the end": FLUID + ref.section(ref.SCALAR, bytes(24), length=41) + END,
    "negative length": FLUID + ref.section(ref.SCALAR, bytes(24), length=-24) + END,
    "cut in a section header": FLUID + ref.section(ref.SCALAR, bytes(24)) + END[:9],
    "bytes after the end": FLUID + ref.section(ref.SCALAR, bytes(24)) + END + b"x",
    "end section with a payload": FLUID + ref.section(ref.END, b"payload!"),
}


@pytest.mark.parametrize("name", list(GOOD))
def test_info_of_a_well_formed_file(tmp_path, name):
    data, bits = GOOD[name]
    assert ref.scan(data, len(data) if name == "fluid only" else data.index(b"IBLB", 8))[0] == ref.OK
    path = tmp_path / "good.ck"
    path.write_bytes(data)
    assert P.checkpoint_info(path) == {"step": 17, "observers": bits}
    lib = L.load()  # either pointer may be NULL
    step, obs = C.c_longlong(-1), C.c_uint(99)
    assert lib.iblb_checkpoint_info(os.fsencode(path), C.byref(step), None) == L.IBLB_OK and step.value == 17
    assert lib.iblb_checkpoint_info(os.fsencode(path), None, C.byref(obs)) == L.IBLB_OK and obs.value == bits
    assert lib.iblb_checkpoint_info(os.fsencode(path), None, None) == L.IBLB_OK


@pytest.mark.parametrize("name", list(BAD))
def test_info_refuses_a_malformed_file(tmp_path, name):
    path = tmp_path / "bad.ck"
    path.write_bytes(BAD[name])
    lib = L.load()
    step, obs = C.c_longlong(-3), C.c_uint(99)
    assert lib.iblb_checkpoint_info(os.fsencode(path), C.byref(step), C.byref(obs)) == L.IBLB_ERR_ARG
    assert (step.value, obs.value) == (-3, 99)
    with pytest.raises(P.IblbError) as e:
        P.checkpoint_info(path)
    assert e.value.code == L.IBLB_ERR_ARG and str(e.value) != "IBLB_ERR_ARG: "
