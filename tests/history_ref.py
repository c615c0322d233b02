"""numpy restatement of the history recorder (include/iblb.h iblb_set_history): the ring's slot arithmetic with
the records a reader may ask for, and the running statistics.

A record is an (np, n) array: plane k at probe p.  The statistics follow the header's rule with one numpy
operation per arithmetic step, so that each step is rounded once, as on the device: the results are meant to be
compared with `==`.  A record built from fields uses tracer_ref.sample, the restatement of iblb_sample_points.
"""
import numpy as np

import tracer_ref as T

STAT_KEYS = ("count", "nonfinite", "sum", "sum_sq", "min", "max", "min_rec", "max_rec")


def slot(m, capacity):
    """The ring slot of record number m."""
    return m % capacity


def window(recorded, capacity):
    """(oldest, recorded): the record numbers the ring still holds are oldest .. recorded - 1."""
    return max(0, recorded - capacity), recorded


def readable(first, count, recorded, capacity):
    """Whether iblb_get_history accepts records [first, first + count)."""
    return count >= 0 and first >= window(recorded, capacity)[0] and first + count <= recorded


def runs(first, count, capacity):
    """The contiguous runs of slots [(slot0, length)] that hold records [first, first + count): at most two."""
    if count == 0:
        return []
    s0 = slot(first, capacity)
    n1 = min(count, capacity - s0)
    return [(s0, n1)] + ([(0, count - n1)] if count > n1 else [])


def record_of(fields, names, x, y):
    """The (len(names), n) record of the named (ny, nx) fields sampled at the points (x, y)."""
    return np.stack([T.sample(fields[m], x, y) for m in names])


class History:
    """A ring of `capacity` records of shape (planes, n) with the iteration of each slot, and the statistics."""

    def __init__(self, planes, n, capacity):
        self.capacity = capacity
        self.ring = np.zeros((capacity, planes, n))
        self.iteration = np.zeros(capacity, dtype=np.int64)
        self.shape = (planes, n)
        self.reset()

    def reset(self):
        self.recorded = 0
        s = self.shape
        self.stats = {
            "count": np.zeros(s, dtype=np.int64), "nonfinite": np.zeros(s, dtype=np.int64),
            "sum": np.zeros(s), "sum_sq": np.zeros(s), "min": np.full(s, np.inf), "max": np.full(s, -np.inf),
            "min_rec": np.full(s, -1, dtype=np.int64), "max_rec": np.full(s, -1, dtype=np.int64),
        }

    def append(self, record, iteration):
        v = np.asarray(record, dtype=np.float64).reshape(self.shape)
        m, st = self.recorded, self.stats
        k = slot(m, self.capacity)
        self.ring[k] = v
        self.iteration[k] = iteration
        ok = np.isfinite(v)
        st["nonfinite"] = st["nonfinite"] + (~ok)
        st["count"] = st["count"] + ok
        with np.errstate(invalid="ignore", over="ignore"):
            s1 = st["sum"] + v
            sq = v * v
            s2 = st["sum_sq"] + sq
            st["sum"] = np.where(ok, s1, st["sum"])
            st["sum_sq"] = np.where(ok, s2, st["sum_sq"])
            lo = ok & (v < st["min"])
            hi = ok & (v > st["max"])
        st["min"] = np.where(lo, v, st["min"])
        st["min_rec"] = np.where(lo, m, st["min_rec"])
        st["max"] = np.where(hi, v, st["max"])
        st["max_rec"] = np.where(hi, m, st["max_rec"])
        self.recorded = m + 1

    def get(self, first=None, count=None):
        """(records (count, planes, n), iterations (count,)) of [first, first + count); by default all the ring
        holds.  ValueError where iblb_get_history returns IBLB_ERR_ARG."""
        oldest, rec = window(self.recorded, self.capacity)
        first = oldest if first is None else first
        count = rec - first if count is None else count
        if not readable(first, count, self.recorded, self.capacity):
            raise ValueError((first, count, self.recorded, self.capacity))
        idx = np.concatenate([np.arange(s, s + n) for s, n in runs(first, count, self.capacity)] or
                             [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        return self.ring[idx].copy(), self.iteration[idx].copy()
