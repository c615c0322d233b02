"""numpy restatement of the scalar's fields (include/iblb.h IBLB_FIELD_C, _CUX, _CUY) and of
iblb_get_scalar_wall_flux, on arrays shaped like Lattice.scalar_populations output (populations (5, ny, nx)) and
Lattice.fields output (fields (ny, nx)).

Every arithmetic step is one numpy operation (numpy's elementwise kernels round once per operation and do not
contract a multiply and an add), in the order the header states: the results are meant to be compared with `==`.
"""
import numpy as np

import scalar_ref as S


def scalar_fields(g, ux, uy):
    """{"c": (((g0+g1)+g2)+g3)+g4, "cux": c*ux, "cuy": c*uy}, in ascending bit order."""
    g, ux, uy = (np.asarray(v, dtype=np.float64) for v in (g, ux, uy))
    with np.errstate(invalid="ignore", over="ignore"):
        c = S.concentration(g)
        return {"c": c, "cux": c * ux, "cuy": c * uy}


def wall_flux(g, walls):
    """(bottom, top), [nx] each: what entered every column through the wall below row 0 / above row ny - 1 during
    the substep that left the populations g.  A value wall: 2.0*g3(x, 0) - (2.0*w1)*value, 2.0*g4(x, ny-1) -
    (2.0*w1)*value; a no-flux wall: 0.0 exactly.  walls as scalar_ref.substep takes them."""
    g = np.asarray(g, dtype=np.float64)
    (k0, v0), (k1, v1) = walls
    nx = g.shape[2]
    with np.errstate(invalid="ignore", over="ignore"):
        bottom = 2.0 * g[3][0] - (2.0 * S.W1) * float(v0) if k0 == S.VALUE else np.zeros(nx)
        top = 2.0 * g[4][-1] - (2.0 * S.W1) * float(v1) if k1 == S.VALUE else np.zeros(nx)
    return bottom, top
