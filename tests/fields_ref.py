"""TEST INFRASTRUCTURE: numpy reference of iblb_get_fields (include/iblb.h).

`fields_ref(rho, u, f, tau, nx, ny, window)` computes every field of the reader from the arrays
iblb_get_macro and iblb_get_populations return (reference layouts, j = y*nx + x), on a lattice that
is periodic in x over its nx columns:

  rho, ux, uy   the given values
  vort          d(uy)/dx - d(ux)/dy: central differences at lattice spacing 1, periodic in x, the
                one-sided first difference at y = 0 and y = ny-1 (numpy.gradient's default edge rule)
  sxx sxy syy   -(1 - 1/(2 tau)) * PiNeq_ab,  PiNeq_ab = sum_i c_ia c_ib (f_i - feq_i(rho, u)), feq the
                oracle's equilibrium (LatticeBoltzmann.cu:45-49, C_S = 0.57735); the O(u F) term of
                Guo forcing is left out

and samples them on the window (x0, y0, nx, ny, sx, sy) (None: the whole lattice): a dict of arrays
of shape (window ny, window nx).
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

NAMES = ("rho", "ux", "uy", "vort", "sxx", "sxy", "syy")


def fields_full(rho, u, f, tau, nx, ny) -> dict:
    """Every field on the whole lattice, arrays of shape (ny, nx)."""
    rho = np.asarray(rho, dtype=np.float64).reshape(ny, nx)
    u = np.asarray(u, dtype=np.float64).reshape(2, ny, nx)
    f = np.asarray(f, dtype=np.float64).reshape(ny, nx, 9)
    ux, uy = u[0], u[1]
    duy_dx = (np.roll(uy, -1, axis=1) - np.roll(uy, 1, axis=1)) / 2.0
    dux_dy = np.gradient(ux, axis=0)
    fneq = f - O.feq(rho.ravel(), u.ravel(), nx, ny).reshape(ny, nx, 9)
    c = O.C_L.astype(np.float64)
    k = -(1.0 - 1.0 / (2.0 * tau))
    pi = lambda a, b: np.tensordot(fneq, c[:, a] * c[:, b], axes=([2], [0]))
    return {"rho": rho, "ux": ux, "uy": uy, "vort": duy_dx - dux_dy,
            "sxx": k * pi(0, 0), "sxy": k * pi(0, 1), "syy": k * pi(1, 1)}


def sample(a: np.ndarray, window) -> np.ndarray:
    if window is None:
        return a
    x0, y0, wnx, wny, sx, sy = window
    return a[y0:y0 + (wny - 1) * sy + 1:sy, x0:x0 + (wnx - 1) * sx + 1:sx]


def fields_ref(rho, u, f, tau, nx, ny, window=None) -> dict:
    return {n: np.ascontiguousarray(sample(a, window)) for n, a in fields_full(rho, u, f, tau, nx, ny).items()}
