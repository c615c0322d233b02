"""The history recorder's entry points at the C boundary, without a device: exported with C linkage, declared in
include/iblb.h and bound in cuda_iblb_11_amd/_lib.py, refused on a NULL context, and the ABI version unchanged
(no struct crossing the ABI changed layout)."""
import ctypes as C
import os
import re
import subprocess

from cuda_iblb_11_amd import _lib as L

NEW = ["iblb_set_history", "iblb_get_history", "iblb_get_history_stats", "iblb_get_history_points",
       "iblb_reset_history", "iblb_history_info"]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "iblb.h")


def test_the_entry_points_are_exported_unmangled():
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    names = L.header_functions()
    for n in NEW:
        assert n in exported, f"{n} not exported unmangled"
        assert n in names and n in L._SIGS, n
    assert L.load().iblb_abi_version() == 6


def test_the_header_declares_them():
    text = open(HEADER).read()
    for n in NEW:
        assert re.search(r"^int " + n + r"\(iblb_ctx\* ctx[,)]", text, re.M), n
    assert re.search(r"^#define IBLB_HIST_TRACERS 1\b", text, re.M) and L.HIST_TRACERS == 1
    assert re.search(r"^#define IBLB_ABI_VERSION 6\b", text, re.M)
    # the contract says what no checkpoint holds
    assert "No checkpoint holds a history" in text


def test_a_null_context_is_refused():
    lib = L.load()
    x = (C.c_double * 2)(0.5, 1.5)
    out = (C.c_double * 2)(-7.0, -7.0)
    it = (C.c_longlong * 2)(-7, -7)
    n, fields, stride = C.c_longlong(-3), C.c_uint(3), C.c_int(-3)
    cap, flags, rec = C.c_longlong(-3), C.c_uint(3), C.c_longlong(-3)
    assert lib.iblb_set_history(None, 2, x, x, 2, 1, 4, 0) == L.IBLB_ERR_ARG
    assert lib.iblb_get_history(None, 0, 1, out, it) == L.IBLB_ERR_ARG
    assert lib.iblb_get_history_stats(None, it, it, out, out, out, out, it, it) == L.IBLB_ERR_ARG
    assert lib.iblb_get_history_points(None, out, out) == L.IBLB_ERR_ARG
    assert lib.iblb_reset_history(None) == L.IBLB_ERR_ARG
    assert lib.iblb_history_info(None, C.byref(n), C.byref(fields), C.byref(stride), C.byref(cap), C.byref(flags),
                                 C.byref(rec)) == L.IBLB_ERR_ARG
    assert list(out) == [-7.0, -7.0] and list(it) == [-7, -7]
    assert (n.value, fields.value, stride.value, cap.value, flags.value, rec.value) == (-3, 3, -3, -3, 3, -3)
