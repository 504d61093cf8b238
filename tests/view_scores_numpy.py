"""The definition of the view scores, in numpy: what csrc/render.hip's score kernel reproduces bit for bit.
Original to this project.  ``scores`` is a twin of render_numpy.image's loop: for every visible record in the draw order and
every pixel of its rectangle where the image's ``add`` is true, wgt = alpha * T -- the float32 product the colour sum uses --
gives  peak[row] = max(peak[row], wgt)  and  total[row] += uint64(wgt * 2**24)  (scaling a float32 by a power of two is exact
and wgt lies in [~3.9e-7, 0.99], so this is an exact truncation to an integer below 2**24).  A pixel's finishing splat adds
nothing; rows that are invisible or never blended keep 0.  Over views: the maximum of the peaks, the sum of the totals.

``total_keys`` is the ranking key 0xffffffff - fbits(total), fbits the bit pattern of total as a float32 rounded toward zero,
from the integer formula; ``keep_peak`` and ``keep_budget`` are the two selections.
"""
import numpy as np

import render_numpy as rn

F32 = np.float32
UNIT = F32(2.0 ** 24)


def scores(rec, plan):
    """-> (peak float32[n], total uint64[n]) of the records `rec` (render_numpy.records) under plan.camera's image size"""
    w, h = plan.camera.width, plan.camera.height
    n = len(rec)
    peak, total = np.zeros(n, F32), np.zeros(n, np.uint64)
    PX, PY = np.meshgrid(np.arange(w, dtype=F32), np.arange(h, dtype=F32))
    T = np.ones((h, w), F32)
    done = np.zeros((h, w), bool)
    with np.errstate(all="ignore"):
        for i in rn.draw_order(rec):
            s = rec[i]
            sl = (slice(int(s["y0"]), int(s["y1"]) + 1), slice(int(s["x0"]), int(s["x1"]) + 1))
            dx, dy = s["u"] - PX[sl], s["v"] - PY[sl]
            power = F32(-0.5) * (s["a"] * (dx * dx) + s["c"] * (dy * dy)) - (s["b"] * dx) * dy
            act = ~done[sl] & (power <= 0)
            alpha = np.minimum(rn.ALPHA_MAX, s["opac"] * rn.lib.np_exp_host(power))
            act &= ~(alpha < rn.ALPHA_MIN)
            Tn = T[sl] * (F32(1) - alpha)
            stop = act & (Tn < rn.T_MIN)
            add = act & ~stop
            done[sl] |= stop
            wgt = alpha * T[sl]
            assert wgt.dtype == F32
            if add.any():
                peak[i] = max(peak[i], wgt[add].max())
                total[i] += (wgt[add] * UNIT).astype(np.uint64).sum(dtype=np.uint64)
            T[sl] = np.where(add, Tn, T[sl])
    return peak, total


def table_scores(table, plans):
    """the accumulated scores of `table` over the plans (any plan render_numpy.records takes: the colour plays no part)"""
    return accumulate([scores(rn.records(table, plan), plan) for plan in plans], len(table))


def accumulate(per_view, n=None):
    """[(peak, total)] per view -> (the maximum of the peaks, the sum of the totals)"""
    n = len(per_view[0][0]) if per_view else int(n)
    peak, total = np.zeros(n, F32), np.zeros(n, np.uint64)
    for p, t in per_view:
        peak = np.maximum(peak, p)
        total = total + t
    return peak, total


def fbits(total: int) -> int:
    """the bit pattern of the integer `total` converted to float32 rounding toward zero, in integers"""
    total = int(total)
    if total == 0:
        return 0
    e = total.bit_length() - 1
    m = total >> (e - 23) if e >= 23 else total << (23 - e)
    return ((e + 127) << 23) | (m & 0x7fffff)


def total_keys(total) -> np.ndarray:
    """-> uint32 keys, smallest = most visible; 0 -> 0xffffffff"""
    return np.array([0xffffffff - fbits(t) for t in np.asarray(total, np.uint64).tolist()], np.uint32).reshape(np.shape(total))


def keep_peak(peak, w) -> np.ndarray:
    """the filter: bool per row, peak >= float32(w)"""
    return np.asarray(peak, F32) >= F32(w)


def keep_budget(total, rows, max_count) -> np.ndarray:
    """the budget among the ascending row numbers `rows`: the max_count smallest keys, equal keys to the lower row -> the kept
    row numbers, ascending"""
    rows = np.asarray(rows, np.int64)
    keys = total_keys(np.asarray(total, np.uint64)[rows])
    order = np.argsort(keys, kind="stable")[:max_count]
    return np.sort(rows[order])


def select(table, plans, min_contribution=None, max_count=None):
    """one scoring pass and both selections, as DataProcessor._view_pass applies them -> (kept rows ascending, peak, total)"""
    peak, total = table_scores(table, plans)
    rows = np.arange(len(table))
    if min_contribution is not None:
        rows = rows[keep_peak(peak, min_contribution)]
    if max_count is not None and max_count < len(rows):
        rows = keep_budget(total, rows, max_count)
    return rows, peak, total
