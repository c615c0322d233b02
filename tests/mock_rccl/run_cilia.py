#!/usr/bin/env python3
"""TEST INFRASTRUCTURE: the on-device cilia (iblb_set_cilia) on the slabs of an RCCL group, as the driver
bin/IBLB runs them on every rank (iblb_attach_rccl, iblb_set_cilia, bulk iblb_step), with N ranks as threads
on one GPU through the mock-RCCL build (tests/mock_rccl/libiblb_mockrccl.so; cf. run_group.py).  Prints one
JSON line; exit status 0 = every check holds.

usage: run_cilia.py NRANKS CONFIG(WIDE|REF) PRECISION(f64|f32) CALLS(comma list) [SAVE_AFTER_CALL]

Every rank attaches, sets the cilia, sets its part of the state and steps the calls (configurations, state and
the oracle twin: tests/cilia_cases.py).  Checked:
  * the assembled fields against the lone slab of the same build stepped through the same calls (1e-12 f64 /
    1e-5 f32, flux 1e-12: run_group.py's tolerances);
  * the assembled fields against the oracle twin (1e-9 / 1e-4, each of rho - 1, u_x, u_y by its own maximum,
    as run_group.py's mode 3);
  * lagrangian() of every rank after every call against the twin's points, u_s, epsilon, bit for bit;
  * lagrangian_force() of every rank against the lone slab's (1e-5); gather_macro against the assembled slabs;
  * with SAVE_AFTER_CALL = k: every rank saves a checkpoint after the k-th call (counted from 1); a second set
    of fresh ranks (no iblb_set_cilia: the configuration comes from the file) attaches, loads and steps the
    remaining calls, and must equal the first run to 1e-12 (absolute, fields; relative, flux).
The line reports band_cycles and deep_launches per rank (of the first run).
"""
import json
import os
import shutil
import sys
import tempfile
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import cilia_cases as CC  # noqa: E402
from cuda_iblb_11_amd import _lib as L  # noqa: E402
from cuda_iblb_11_amd import workloads as W  # noqa: E402
from cuda_iblb_11_amd.lattice import Lattice, plan_slabs, rccl_unique_id, split_state  # noqa: E402


def main():
    n, cfg, prec = int(sys.argv[1]), CC.CONFIGS[sys.argv[2]], sys.argv[3]
    calls = [int(v) for v in sys.argv[4].split(",")]
    save = int(sys.argv[5]) if len(sys.argv) > 5 else None
    if save is not None and not 1 <= save < len(calls):
        raise SystemExit("SAVE_AFTER_CALL must leave at least one call to finish")
    nx, ny = cfg.nx, cfg.ny
    lib = L.load_from(os.path.join(HERE, "libiblb_mockrccl.so"))
    rho, u = cfg.state()
    kw = dict(precision=prec, body_force=CC.BODY, max_points=cfg.max_points, lib=lib)

    # the lone slab of the same build through the same calls
    single = Lattice(nx, ny, W.TAU, W.TAU2, **kw)
    single.set_cilia(*cfg.cilia)
    single.set_state(rho, u)
    for k in calls:
        single.step(k)
    r1, u1 = single.macro()
    q1, f1 = single.flux, single.lagrangian_force()
    single.close()

    # the oracle twin, one iteration at a time
    from oracle import oracle as O
    O.load()
    snaps = CC.run_twin(O, cfg, CC.steps(*calls))[1]
    ro, uo = snaps[-1]["rho"], snaps[-1]["u"]

    uid, uid2 = rccl_unique_id(lib), rccl_unique_id(lib)
    out, gathered, restarted = [None] * n, [None] * n, [None] * n
    points_ok = [True] * n
    errors = []
    tmp = tempfile.mkdtemp(prefix="iblb_cilia_ck_")
    ck = lambda r: os.path.join(tmp, f"ck.rank{r}")

    def guarded(fn):
        def run(r):
            try:
                fn(r)
            except Exception as e:  # a failed rank would leave the others waiting: report and exit hard
                errors.append(f"rank {r}: {e!r}")
                print(json.dumps({"ok": False, "errors": errors}), flush=True)
                os._exit(2)
        return run

    def same_points(lat, snap):
        s, us, eps = lat.lagrangian()
        return bool(np.array_equal(s, snap["s"]) and np.array_equal(us, snap["u_s"]) and np.array_equal(eps, snap["eps"]))

    @guarded
    def worker(r):
        xb, xc = plan_slabs(nx, n)[r]
        lat = Lattice(nx, ny, W.TAU, W.TAU2, x_begin=xb, x_count=xc, **kw)
        lat.attach_rccl(uid, n, r)
        lat.set_cilia(*cfg.cilia)
        lat.set_state(split_state(rho, 1, nx, ny, xb, xc), split_state(u, 2, nx, ny, xb, xc))
        for i, k in enumerate(calls):
            lat.step(k)
            points_ok[r] = points_ok[r] and same_points(lat, snaps[i])
            if save is not None and i + 1 == save:
                lat.save_checkpoint(ck(r))
        tm = lat.timing()
        rs, us = lat.macro()
        out[r] = (xb, xc, rs, us, lat.flux, lat.lagrangian_force(), tm["band_cycles"], tm["deep_launches"])  # collective
        gathered[r] = lat.gather_macro(0)  # collective output gather to rank 0
        lat.close()

    @guarded
    def resume(r):  # fresh contexts: attach, restore the checkpoint (cilia configuration included), finish
        xb, xc = plan_slabs(nx, n)[r]
        lat = Lattice(nx, ny, W.TAU, W.TAU2, x_begin=xb, x_count=xc, **kw)
        lat.attach_rccl(uid2, n, r)
        lat.load_checkpoint(ck(r))
        ok = lat.steps == sum(calls[:save]) and same_points(lat, snaps[save - 1])
        for i in range(save, len(calls)):
            lat.step(calls[i])
            ok = ok and same_points(lat, snaps[i])
        rs, us = lat.macro()
        restarted[r] = (rs, us, lat.flux, lat.steps, ok, lat.timing()["band_cycles"])
        lat.close()

    for fn in (worker, resume) if save is not None else (worker,):
        th = [threading.Thread(target=fn, args=(r,)) for r in range(n)]
        for t in th:
            t.start()
        for t in th:
            t.join()

    shutil.rmtree(tmp, ignore_errors=True)
    R = np.empty((ny, nx))
    U = np.empty((2, ny, nx))
    for xb, xc, rs, us, *_ in out:
        R[:, xb:xb + xc] = rs.reshape(ny, xc)
        U[:, :, xb:xb + xc] = us.reshape(2, ny, xc)
    R, U = R.ravel(), U.reshape(2, -1).ravel()
    N = nx * ny
    d_rho = float(np.max(np.abs(R - r1)) / np.max(np.abs(r1)))
    d_u = float(np.max(np.abs(U - u1)) / np.max(np.abs(u1)))
    fluxes = [o[4] for o in out]
    d_q = float(max(abs(q - q1) for q in fluxes) / max(abs(q1), 1e-300))
    tol = 1e-12 if prec == "f64" else 1e-5
    ok = d_rho <= tol and d_u <= tol and d_q <= 1e-12
    d_oracle = {"rho-1": float(np.max(np.abs((R - 1) - (ro - 1))) / np.max(np.abs(ro - 1))),
                "ux": float(np.max(np.abs(U[:N] - uo[:N])) / np.max(np.abs(uo[:N]))),
                "uy": float(np.max(np.abs(U[N:] - uo[N:])) / np.max(np.abs(uo[N:])))}
    ok = ok and max(d_oracle.values()) <= (1e-9 if prec == "f64" else 1e-4)
    ok = ok and all(points_ok)
    d_fs = max(float(np.max(np.abs(o[5] - f1)) / np.max(np.abs(f1))) for o in out)
    ok = ok and d_fs <= 1e-5
    g_ok = bool(np.array_equal(gathered[0][0], R) and np.array_equal(gathered[0][1], U)
                and all(g == (None, None) for g in gathered[1:]))
    ok = ok and g_ok
    d_re, rs_ok, re_cycles = None, None, None
    if save is not None:
        rs_ok = all(restarted[r][3] == sum(calls) and restarted[r][4] for r in range(n))
        d_re = 0.0
        for r in range(n):
            a, b = out[r], restarted[r]
            d_re = max(d_re, float(np.max(np.abs(a[2] - b[0]))), float(np.max(np.abs(a[3] - b[1]))))
            rs_ok = rs_ok and abs(a[4] - b[2]) <= 1e-12 * max(abs(a[4]), 1e-300)
        rs_ok = bool(rs_ok and d_re <= 1e-12)
        re_cycles = [b[5] for b in restarted]
        ok = ok and rs_ok
    print(json.dumps({"ok": bool(ok), "n": n, "config": cfg.name, "precision": prec, "calls": calls, "d_rho": d_rho,
                      "d_u": d_u, "d_flux": d_q, "d_oracle": d_oracle, "points_ok": points_ok, "d_F_s": d_fs,
                      "gather_ok": g_ok, "restart_ok": rs_ok, "d_restart": d_re, "band_cycles": [o[6] for o in out],
                      "deep_launches": [o[7] for o in out], "restart_band_cycles": re_cycles}), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
