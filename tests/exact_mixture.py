"""The mixture contract of include/spkd.h, section 9 (restated in tests/reseg_gmm_numpy.py's docstring),
at 50 digits -- TEST INFRASTRUCTURE ONLY.

What tests/reseg_gmm_numpy.py and tests/link_clr_numpy.py compute in float64, in the device's own
raw-moment form B / G - mean^2, is computed here so that it shares neither the precision nor the
formulation:

  inputs    converted exactly: a float32 frame and a float64 model value are integers over 2^300 (asserted);
  sums      of frames, squares and quadratic forms are sums of integers, exact; a responsibility enters
            a sum as an integer over 2^400 (it is known to 50 digits, no better);
  variance  centred: sum g (x - mean)^2 / G around the 50-digit mean (the initial model's and the
            floor's, whose weights are 0 or 1, exactly (n S2 - S1^2) / n^2);
  the rest  exp, ln, quotients and the log-likelihoods in mpmath at mp.dps = 50.

One rule of float64 is part of the contract: exp(l_k - m) is 0 once it underflows.  exp flushes
around -745; the reference flushes at FLUSH = -750, and tests/mixture_cases.py keeps every l_k - m of
its cases out of -800 .. -700 so that no case depends on where in that band an exp gives up.

Every function also returns what the cases' conditions are checked on (`info`): every l_k - m of every
frame ('gaps'), every G_k ('G') and whether it is a sum of exact zeros and ones ('unit'), every
unfloored variance over its floor ('ratio').
"""
import math

import numpy as np
from mpmath import mp, mpf

DPS = 50
DIM = 39
COMP = 80
MEAN, IVAR, NORM = 1, 1 + DIM, COMP - 1
MIN_PER_COMP = DIM + 1
S = 300                     # frames and model values: integers over 2^S
SG = 400                    # responsibilities: integers over 2^SG
ONE, ONE_G = 1 << S, 1 << SG
FLUSH = -750


def _fix(v):
    """The float v as an integer over 2^S, exactly."""
    n, d = float(v).as_integer_ratio()
    assert d <= ONE, 'a value below 2^-%d of its unit' % S
    return n * (ONE // d)


def _mp(i, scale):
    """The integer i over 2^scale as an mpf (rounded once)."""
    return mp.ldexp(mpf(i), -scale)


def _int_g(g):
    """The mpf g in [0, 1] as an integer over 2^SG, rounded down."""
    sign, man, exp, _ = g._mpf_
    assert not sign
    sh = exp + SG
    return man << sh if sh >= 0 else man >> -sh


def frames_int(x):
    """x [N, 39] float32 -> (rows of integers over 2^S, every frame finite)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1, DIM)
    if not np.isfinite(x).all():
        return None, False
    return [[_fix(v) for v in row] for row in x.astype(np.float64).tolist()], True


def _floor(X, var_floor):
    n = len(X)
    out, good = [], n > 0
    for d in range(DIM):
        s1 = sum(r[d] for r in X)
        s2 = sum(r[d] * r[d] for r in X)
        v = _mp(n * s2 - s1 * s1, 2 * S) / (n * n) if n else mpf('nan')
        good = good and v > 0
        out.append(v)
    return [mpf(var_floor) * v for v in out], bool(good), out


def variance_floor(x, var_floor):
    """(floor [39], ok, V [39]): var_floor times the ML variance of all the frames."""
    with mp.workdps(DPS):
        X, fin = frames_int(x)
        if not fin:
            return None, False, None
        return _floor(X, var_floor)


def _component(G, n, mean, var, floor, old):
    """A model row of the weight G / n and, when G >= 2, the mean and the floored variance; `old`: the row
    that stays otherwise (None: mean 0, variance 1).  Returns (row, unfloored variance over floor or None)."""
    row = [mp.log(G / n) if G > 0 else mpf('-inf')]
    if G >= 2:
        ratio = [v / f for v, f in zip(var, floor)]
        var = [f if v < f else v for v, f in zip(var, floor)]
        row += mean + [1 / v for v in var]
        row.append(-(DIM * mp.log(2 * mp.pi) + sum(mp.log(v) for v in var)) / 2)
        return row, ratio
    if old is None:
        return row + [mpf(0)] * DIM + [mpf(1)] * DIM + [-DIM * mp.log(2 * mp.pi) / 2], None
    return row + [mpf(float(v)) for v in old[MEAN:]], None


def init_model(x, k_comp, var_floor):
    """(model [K][80] of mpf, ok, info): the segmental start."""
    with mp.workdps(DPS):
        X, fin = frames_int(x)
        if not fin:
            return None, False, None
        n = len(X)
        floor, good, _ = _floor(X, var_floor)
        model, info = [], {'G': [], 'unit': [], 'ratio': [], 'gaps': []}
        for k in range(k_comp):
            rows = X[k * n // k_comp:(k + 1) * n // k_comp]
            c = len(rows)
            mean = var = None
            if c >= 2:
                s1 = [sum(r[d] for r in rows) for d in range(DIM)]
                s2 = [sum(r[d] * r[d] for r in rows) for d in range(DIM)]
                mean = [_mp(a, S) / c for a in s1]
                var = [_mp(c * b - a * a, 2 * S) / (c * c) for a, b in zip(s1, s2)]
            row, ratio = _component(mpf(c), n, mean, var, floor, None)
            model.append(row)
            info['G'].append(mpf(c))
            info['unit'].append(True)
            info['ratio'].append(ratio)
        return model, bool(good and n >= MIN_PER_COMP * k_comp), info


def _model_int(model):
    """model [K, 80] float64 -> per live component (k, ln w + log_norm as mpf, means, 1 / var as integers)."""
    model = np.asarray(model, dtype=np.float64).reshape(-1, COMP)
    out = []
    for k, c in enumerate(model.tolist()):
        if c[0] != -math.inf:
            out.append((k, mpf(c[0]) + mpf(c[NORM]), [_fix(v) for v in c[MEAN:IVAR]], [_fix(v) for v in c[IVAR:NORM]]))
    return len(model), out


def _frame(row, live, gaps):
    """One frame under the live components: (m + ln sum exp(l - m), [(k, exp(l_k - m))], the sum)."""
    if not live:
        return mpf('-inf'), [], mpf(0)
    ls = []
    for k, c, mean, ivar in live:
        q = 0
        for xv, mv, iv in zip(row, mean, ivar):
            d = xv - mv
            q += d * d * iv
        ls.append(c - _mp(q, 3 * S) / 2)
    m = max(ls)
    es, total = [], mpf(0)
    for (k, _, _, _), l in zip(live, ls):
        t = l - m
        gaps.append(float(t))
        e = mp.exp(t) if t > FLUSH else mpf(0)
        es.append((k, e))
        total += e
    return m + mp.log(total), es, total


def _e_step(X, model):
    """(K, per frame [(k, g as an integer over 2^SG)], L, gaps)."""
    k_comp, live = _model_int(model)
    gaps, resp, total = [], [], mpf(0)
    for row in X:
        ll, es, s = _frame(row, live, gaps)
        total += ll
        resp.append([(k, _int_g(e / s)) for k, e in es if e != 0])
    return k_comp, resp, total, gaps


def _sums(X, resp, k_comp):
    """G_k (integers over 2^SG), A_k (over 2^(S + SG)) and whether every g_k is exactly 0 or 1."""
    G = [0] * k_comp
    A = [[0] * DIM for _ in range(k_comp)]
    unit = [True] * k_comp
    for row, gs in zip(X, resp):
        for k, g in gs:
            G[k] += g
            unit[k] = unit[k] and g == ONE_G
            a = A[k]
            for d in range(DIM):
                a[d] += g * row[d]
    return G, A, unit


def em_step(x, model, var_floor):
    """One EM step from `model` ([K, 80] float64) -> (model [K][80] of mpf, L of the model that entered,
    G [K], ok, info)."""
    with mp.workdps(DPS):
        X, fin = frames_int(x)
        if not fin:
            return None, None, None, False, None
        n = len(X)
        old = np.asarray(model, dtype=np.float64).reshape(-1, COMP).tolist()
        floor, good, _ = _floor(X, var_floor)
        k_comp, resp, total, gaps = _e_step(X, old)
        G, A, unit = _sums(X, resp, k_comp)
        means = [[(mpf(a) / g) if g else None for a in A[k]] for k, g in enumerate(G)]       # over 2^S
        cent = [[_int_m(v) if v is not None else 0 for v in means[k]] for k in range(k_comp)]
        C = [[0] * DIM for _ in range(k_comp)]
        for row, gs in zip(X, resp):
            for k, g in gs:
                c, mk = C[k], cent[k]
                for d in range(DIM):
                    dv = row[d] - mk[d]
                    c[d] += g * dv * dv
        out, info = [], {'G': [], 'unit': unit, 'ratio': [], 'gaps': gaps}
        for k in range(k_comp):
            Gk = _mp(G[k], SG)
            mean = var = None
            if Gk >= 2:
                # sum g (x - c)^2 / G - (mean - c)^2 is the centred variance for any centre c; c is the mean
                # rounded to 2^-S, so the correction is below 2^-2S
                mean = [mp.ldexp(v, -S) for v in means[k]]
                var = [_mp(C[k][d], 2 * S + SG) / Gk - (mean[d] - _mp(cent[k][d], S)) ** 2 for d in range(DIM)]
            row, ratio = _component(Gk, n, mean, var, floor, old[k])
            out.append(row)
            info['G'].append(Gk)
            info['ratio'].append(ratio)
        return out, total, info['G'], bool(good and n >= MIN_PER_COMP * k_comp), info


def _int_m(v):
    """The mpf v (already in units of 2^-S) rounded down to an integer."""
    return int(mp.floor(v))


def scores(x, models):
    """x [T, 39] float32, models [[K, 80] float64] -> ([T][len(models)] of mpf, info): m + ln sum exp(l - m)."""
    with mp.workdps(DPS):
        X, fin = frames_int(x)
        assert fin
        lives = [_model_int(m)[1] for m in models]
        gaps = []
        return [[_frame(row, live, gaps)[0] for live in lives] for row in X], {'gaps': gaps}


def ubm_record(x, ubm):
    """(n_c [C], f_c [C][39], info) of the frames x under the UBM [C, 80] float64."""
    with mp.workdps(DPS):
        X, fin = frames_int(x)
        assert fin
        k_comp, resp, _, gaps = _e_step(X, ubm)
        G, A, unit = _sums(X, resp, k_comp)
        n = [_mp(g, SG) for g in G]
        return n, [[_mp(a, S + SG) for a in A[k]] for k in range(k_comp)], {'G': n, 'unit': unit, 'gaps': gaps, 'ratio': []}


def to_float(model):
    """A model of mpf as [K, 80] float64, each value rounded once."""
    return np.array([[float(v) for v in row] for row in model], dtype=np.float64).reshape(-1, COMP)
