"""Shared by test_evaluator.py and test_hip_evaluator.py: the yardstick of the statistic means — `math.fsum` of the entering values divided by
their count — the bound a mean must keep to it, and rows that carry what the definition names (NaNs, an all-NaN row, infinities).

The bound is derived, not measured (include/hns.h, hns_eval_means): an fp64 sum of n <= 2^20 values in any order is off by at most
(n - 1) 2^-53 sum|x|, the division adds 2^-53 |exact|, together at most 2^-33 mean|x|; the one rounding to fp32 adds 2^-24 |exact|."""
import math

import numpy as np


def exact_mean(row, mask=None):
    """(fsum of the values of `row` that enter / their count, mean |x| of them, their count); (nan, 0.0, 0) when none enters.  A row with
    an infinity gives what IEEE addition gives: that infinity, or NaN when both signs are there."""
    row = np.asarray(row, np.float32).reshape(-1)
    keep = ~np.isnan(row) if mask is None else (~np.isnan(row) & (np.asarray(mask).reshape(-1) != 0))
    vals = [float(v) for v in row[keep]]
    if not vals:
        return float("nan"), 0.0, 0
    if any(math.isinf(v) for v in vals):
        signs = {v > 0 for v in vals if math.isinf(v)}
        return (float("nan") if len(signs) == 2 else (math.inf if True in signs else -math.inf)), math.inf, len(vals)
    return math.fsum(vals) / len(vals), math.fsum(abs(v) for v in vals) / len(vals), len(vals)


def check_mean(got, row, mask=None, what=""):
    """`got` (the fp32 mean under test) against exact_mean within 2^-24 |exact| + 2^-33 mean|x|; returns the count that must have entered."""
    exact, mean_abs, n = exact_mean(row, mask)
    got = float(got)
    if math.isnan(exact) or math.isinf(exact):
        assert (math.isnan(got) and math.isnan(exact)) or got == exact, (what, got, exact)
        return n
    err, bound = abs(got - exact), 2.0 ** -24 * abs(exact) + 2.0 ** -33 * mean_abs
    assert err <= bound, f"{what}: mean {got!r} is {err:.3e} from the exact {exact!r}, bound {bound:.3e}"
    return n


def make_rows(count, n, seed):
    """[count, n] fp32: magnitudes over six decades and both signs; every third row a fifth NaNs, row 1 (when there) all NaN, the last row of
    a table of more than two rows one +inf (when n > 1: it must still leave a value beside it)."""
    g = np.random.default_rng(seed)
    rows = (g.standard_normal((count, n)) * 10.0 ** g.uniform(-3, 3, (count, 1)) + g.uniform(-5, 5, (count, 1))).astype(np.float32)
    for i in range(0, count, 3):
        rows[i, g.random(n) < 0.2] = np.nan
    if count > 1:
        rows[1] = np.nan
    if count > 2 and n > 1:
        rows[-1, g.integers(n)] = np.inf
    return rows


def make_mask(kind, n, seed):
    """None (every env), "partial" (about two thirds of the envs, any non-zero byte counts) or "zero" (no env)."""
    if kind is None:
        return None
    if kind == "zero":
        return np.zeros(n, np.uint8)
    g = np.random.default_rng(seed + 1)
    m = (g.random(n) < 0.67).astype(np.uint8)
    m[m != 0] = g.integers(1, 256, int((m != 0).sum()), dtype=np.uint8)
    return m
