"""numpy restatement of the sampling rule of iblb_set_average (include/iblb.h) on dicts shaped like
Lattice.fields output ({name: (ny, nx) array}), and of the plan iblb_step cuts its calls into when
tracers, averaging or both are set.

The sums are built sequentially, one numpy operation per arithmetic step (numpy's elementwise kernels
do not contract a multiply and an add), in sample order, starting from +0.0 as the device's zeroed
accumulators do: the results are meant to be compared with `==`.
"""
import numpy as np


def accumulate(samples, nbins=1, squares=False, uxuy=False):
    """samples: a list of {name: (ny, nx) array} in sample order (sample m goes to bin m % nbins).
    Returns one dict per bin, shaped like Lattice.average: {"samples": n, "sum": {name: array},
    "sum_sq": {name: array} or None, "sum_uxuy": array or None}.  A bin without a sample holds zeros."""
    if nbins < 1:
        raise ValueError("nbins must be >= 1")
    if not samples:
        raise ValueError("at least one sample is needed for the shapes")
    names = list(samples[0])
    shape = np.asarray(samples[0][names[0]]).shape
    if uxuy and not ("ux" in names and "uy" in names):
        raise ValueError("uxuy needs ux and uy")
    bins = [{"samples": 0,
             "sum": {n: np.zeros(shape) for n in names},
             "sum_sq": {n: np.zeros(shape) for n in names} if squares else None,
             "sum_uxuy": np.zeros(shape) if uxuy else None} for _ in range(nbins)]
    with np.errstate(invalid="ignore", over="ignore"):
        for m, s in enumerate(samples):
            b = bins[m % nbins]
            for n in names:
                v = np.asarray(s[n], dtype=np.float64)
                b["sum"][n] = b["sum"][n] + v
                if squares:
                    b["sum_sq"][n] = b["sum_sq"][n] + v * v
            if uxuy:
                b["sum_uxuy"] = b["sum_uxuy"] + np.asarray(s["ux"], dtype=np.float64) * np.asarray(s["uy"], dtype=np.float64)
            b["samples"] += 1
    return bins


def pieces(calls, t, tracers=None, average=None):
    """The pieces iblb_step cuts `calls` (a list of step counts) into from the state at iteration t.
    tracers / average: None, or (t0, stride) of that event set (events after t0 + stride, t0 + 2 stride,
    ...; t0 <= t).  Returns [(iterations, tracer update?, average sample?)]: the call is cut at the union
    of both event sets, and with neither set a call is one piece."""
    def first_after(ev):
        if ev is None:
            return None
        t0, stride = ev
        if stride < 1 or t0 > t:
            raise ValueError("need stride >= 1 and t0 <= t")
        nxt = t0 + stride
        while nxt <= t:
            nxt += stride
        return nxt

    nt, na = first_after(tracers), first_after(average)
    out = []
    for n in calls:
        while n > 0:
            ahead = [e - t for e in (nt, na) if e is not None]
            p = min([n] + ahead)
            t, n = t + p, n - p
            ut, ua = nt is not None and t == nt, na is not None and t == na
            out.append((p, ut, ua))
            if ut:
                nt += tracers[1]
            if ua:
                na += average[1]
    return out
