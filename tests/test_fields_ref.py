"""The definitions of iblb_get_fields' fields, pinned on the CPU: the numpy reference
(tests/fields_ref.py) on the oracle's force-driven half-channel (bounce-back bottom row, mirror top
row, periodic in x), plus what the C ABI answers without a device and the ctypes Window layout.

Half-channel: a uniform body force g along x drives a steady flow u_x(y) between the no-slip wall
(half a cell below row 0) and the symmetry line (half a cell above row ny-1).  The momentum balance
gives the shear stress line sxy(y) = g_eff (ny - 1/2 - y), and the stress must equal the viscosity
times the velocity gradient the vorticity measures: sxy = nu (-vort), nu = C_S^2 (tau - 1/2).
g_eff = g (1 + (1/tau2 - 1/tau)/2): the reference relaxes its forcing term's odd part with tau2
(TRT), which the oracle reproduces.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import fields_ref as R
from cuda_iblb_11_amd import _lib as L
from oracle import oracle as O

G = 1e-6
NX = 8
# (tau, tau2, ny, steps)
CASES = [(1.0, 0.6, 16, 4608), (0.8, 0.8, 24, 17280)]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"tau{c[0]}-tau2{c[1]}-ny{c[2]}")
def channel(request):
    tau, tau2, ny, steps = request.param
    sim = O.Simulation(NX, ny, tau, tau2, body_force=(G, 0.0))
    sim.step(steps)
    return tau, tau2, ny, R.fields_ref(sim.rho, sim.u, sim.f, tau, NX, ny)


def test_stress_matches_velocity_gradient(channel):
    """Rows 1 .. ny-2 (central differences): sxy = nu (-vort) within 1e-3 g."""
    tau, _, ny, fld = channel
    nu = O.C_S ** 2 * (tau - 0.5)
    dev = np.max(np.abs(fld["sxy"][1:ny - 1] - nu * (-fld["vort"][1:ny - 1])))
    print(f"max |sxy - nu (-vort)| = {dev / G:.3g} g")
    assert dev <= 1e-3 * G


def test_steady_stress_line(channel):
    """Every row: sxy = g_eff (ny - 1/2 - y) within 0.5 % of g_eff ny."""
    tau, tau2, ny, fld = channel
    g_eff = G * (1.0 + (1.0 / tau2 - 1.0 / tau) / 2.0)
    line = g_eff * (ny - 0.5 - np.arange(ny))[:, None]
    dev = np.max(np.abs(fld["sxy"] - line))
    print(f"max |sxy - g_eff (ny - 1/2 - y)| = {100 * dev / (g_eff * ny):.3g} % of g_eff ny")
    assert dev <= 5e-3 * g_eff * ny


def test_reference_window_sampling():
    a = np.arange(7 * 5, dtype=float).reshape(7, 5)
    w = R.sample(a, (1, 2, 2, 3, 3, 2))  # x = 1, 4; y = 2, 4, 6
    assert np.array_equal(w, a[[2, 4, 6]][:, [1, 4]])
    assert R.sample(a, None) is a


def test_fields_without_a_context_are_argument_errors():
    lib = L.load()
    w = L.Window(0, 0, 1, 1, 1, 1)
    out = (C.c_double * 8)()
    assert lib.iblb_get_fields(None, C.byref(w), 1, out) == L.IBLB_ERR_ARG
    assert lib.iblb_get_fields(None, None, 0, None) == L.IBLB_ERR_ARG
    i0, n = C.c_int(0), C.c_int(0)
    assert lib.iblb_window_local(None, C.byref(w), C.byref(i0), C.byref(n)) == L.IBLB_ERR_ARG
    assert lib.iblb_window_local(None, None, None, None) == L.IBLB_ERR_ARG


def test_window_layout_matches_the_header(tmp_path):
    """ctypes Window against struct iblb_window: size and every field's offset from a C program
    compiled with gcc against include/iblb.h, and the IBLB_FIELD_* bits against FIELDS."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "iblb.h"', 'int main(void) {',
             '    printf("size %zu\\n", sizeof(iblb_window));']
    for fname, _ in L.Window._fields_:
        lines.append(f'    printf("{fname} %zu\\n", offsetof(iblb_window, {fname}));')
    for name in L.FIELDS:
        lines.append(f'    printf("bit_{name} %d\\n", IBLB_FIELD_{name.upper()});')
    lines += ['    return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(repo, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out if ln.strip()}
    assert got["size"] == C.sizeof(L.Window)
    for fname, _ in L.Window._fields_:
        assert got[fname] == getattr(L.Window, fname).offset, fname
    for name, bit in L.FIELDS.items():
        assert got["bit_" + name] == bit, name
    assert [f for f, _ in L.Window._fields_] == ["x0", "y0", "nx", "ny", "sx", "sy"]
