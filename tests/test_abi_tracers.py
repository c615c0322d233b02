"""The point sampler's and the tracers' entry points at the C boundary, without a device: exported with C
linkage, declared in include/iblb.h and bound in cuda_iblb_11_amd/_lib.py, refused on a NULL context, and
the ABI version unchanged (no struct crossing the ABI changed layout)."""
import ctypes as C
import subprocess

from cuda_iblb_11_amd import _lib as L

NEW = ["iblb_sample_points", "iblb_set_tracers", "iblb_get_tracers", "iblb_tracer_count"]


def test_the_entry_points_are_exported_unmangled():
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    names = L.header_functions()
    for n in NEW:
        assert n in exported, f"{n} not exported unmangled"
        assert n in names and n in L._SIGS, n
    assert L.load().iblb_abi_version() == 6


def test_a_null_context_is_refused():
    lib = L.load()
    x = (C.c_double * 2)(0.5, 1.5)
    out = (C.c_double * 2)(-7.0, -7.0)
    n, stride, updates = C.c_longlong(-3), C.c_int(-3), C.c_longlong(-3)
    assert lib.iblb_sample_points(None, 2, x, x, 1, out) == L.IBLB_ERR_ARG
    assert lib.iblb_set_tracers(None, 2, x, x, 1) == L.IBLB_ERR_ARG
    assert lib.iblb_get_tracers(None, out, out, None) == L.IBLB_ERR_ARG
    assert lib.iblb_tracer_count(None, C.byref(n), C.byref(stride), C.byref(updates)) == L.IBLB_ERR_ARG
    assert list(out) == [-7.0, -7.0] and (n.value, stride.value, updates.value) == (-3, -3, -3)
