"""The linking and gallery contract of include/spkd.h, sections 10 and 11, in exact arithmetic -- TEST
INFRASTRUCTURE ONLY.

What tests/link_clr_numpy.py and tests/gallery_numpy.py compute in float64, in the device's own form
(0.5 (m^2 - mu^2) / var and (m - mu) / var formed apart, then one dot product), is computed here so that
it shares neither the precision nor the formulation:

  inputs    converted exactly: a float64 record, model value or relevance is an integer over 2^S (asserted);
  MAP       m = (f + r mu) / (n + r) is a rational; with g = f - n mu (an integer over 2^2S)
            m - mu = g / (n + r)  exactly, so that
  H(a|b)    = (1 / N_a) sum_c [sum_d (g^b_cd (2 g^a_cd (n^b_c + r) - n^a_c g^b_cd)) / var_cd] / (2 (n^b_c + r)^2):
            per component one sum of integers over one integer, a rational; N_a = sum_c n^a_c exactly;
  CLR       H(a|b) + H(b|a), a fractions.Fraction; None when N_a or N_b is 0 (the device's 0 / 0: not finite);
  merge     record[a] += record[b] is the ONE rule of float64 that is part of the contract: each element
            is the exact sum rounded once to nearest-even (what an IEEE addition gives; asserted against
            the rounded rational in tests/test_clr_exact.py).

The decisions -- the chain of section 10 with its tie and stop rules, the assignment of section 11 --
are taken on those rationals.  Both also return their margins on the exact values: the least lead of a
chosen pair over the best pair of a lower value it competed with, the least distance of a compared
value from the threshold, and how many choices were exact ties.
"""
from fractions import Fraction

import numpy as np

DIM = 39
COMP = 80            # SPKD_GMM_COMP
BW_COMP = 40         # SPKD_BW_COMP
MEAN, IVAR = 1, 1 + DIM
S = 400              # every input: an integer over 2^S
ONE = 1 << S


def _fix(v):
    """The float v as an integer over 2^S, exactly."""
    n, d = float(v).as_integer_ratio()
    assert d <= ONE, 'a value below 2^-%d of its unit' % S
    return n * (ONE // d)


class Model(object):
    """The UBM's means and inverse variances and the relevance as integers over 2^S."""

    def __init__(self, ubm, r):
        ubm = np.asarray(ubm, dtype=np.float64).reshape(-1, COMP)
        assert np.isfinite(ubm[:, MEAN:IVAR + DIM]).all() and np.isfinite(r) and r > 0
        self.K = len(ubm)
        self.mu = [[_fix(v) for v in row[MEAN:IVAR]] for row in ubm.tolist()]
        self.iv = [[_fix(v) for v in row[IVAR:IVAR + DIM]] for row in ubm.tolist()]
        self.r = _fix(r)


class Record(object):
    """A record [C, 40] float64: n_c (over 2^S), g_cd = f_cd - n_c mu_cd (over 2^2S), N (over 2^S)."""

    def __init__(self, rec, model):
        rec = np.asarray(rec, dtype=np.float64).reshape(model.K, BW_COMP)
        assert np.isfinite(rec).all()
        rows = rec.tolist()
        self.n = [_fix(row[0]) for row in rows]
        self.f = [[_fix(v) for v in row[1:]] for row in rows]
        self.g = [[(fv << S) - n * mv for fv, mv in zip(f, mu)] for n, f, mu in zip(self.n, self.f, model.mu)]
        self.N = sum(self.n)


def map_means(rec, ubm, r):
    """m_cd = (f_cd + r mu_cd) / (n_c + r) as [C][39] Fractions."""
    m = Model(ubm, r)
    a = Record(rec, m)
    return [[Fraction((fv << S) + m.r * mv, (n + m.r) << S) for fv, mv in zip(f, mu)] for n, f, mu in zip(a.n, a.f, m.mu)]


def total(rec):
    """N = sum_c n_c, exactly."""
    return sum(Fraction(float(v)) for v in np.asarray(rec, dtype=np.float64).reshape(-1, BW_COMP)[:, 0])


def _half(a, b, m):
    """H(a|b) of two Records, a Fraction; None when N_a = 0."""
    if a.N == 0:
        return None
    h = Fraction(0)
    for c in range(m.K):
        den = b.n[c] + m.r                                      # over 2^S, > 0
        na = a.n[c]
        num = 0                                                 # over 2^6S
        for iv, gb, ga in zip(m.iv[c], b.g[c], a.g[c]):
            num += iv * gb * (2 * ga * den - na * gb)
        h += Fraction(num, (2 * den * den) << (4 * S))
    return h / Fraction(a.N, ONE)


def half(a, b, ubm, r):
    m = Model(ubm, r)
    return _half(Record(a, m), Record(b, m), m)


def _clr(a, b, m):
    x, y = _half(a, b, m), _half(b, a, m)
    return None if x is None or y is None else x + y


def clr(a, b, ubm, r):
    m = Model(ubm, r)
    return _clr(Record(a, m), Record(b, m), m)


def merged(a, b):
    """record a + record b as the contract has it: the exact sum of each element rounded once."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a + b


def merged_rational(a, b):
    """The same through rationals: float(Fraction) rounds once to nearest-even."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = [float(Fraction(x) + Fraction(y)) for x, y in zip(a.ravel().tolist(), b.ravel().tolist())]
    return np.array(out, dtype=np.float64).reshape(a.shape)


def matrix(records, ok, ubm, r):
    """{(a, b): CLR} over the ok pairs a < b, and whether every one is finite."""
    m = Model(ubm, r)
    recs = [Record(x, m) if k else None for x, k in zip(records, ok)]
    out, fin = {}, True
    for a in range(len(recs)):
        for b in range(a + 1, len(recs)):
            if ok[a] and ok[b]:
                out[(a, b)] = _clr(recs[a], recs[b], m)
                fin = fin and out[(a, b)] is not None
    return out, fin


class Margins(object):
    def __init__(self):
        self.to_th, self.to_next, self.ties = None, None, 0

    def threshold(self, d, th):
        gap = abs(d - th)
        self.to_th = gap if self.to_th is None or gap < self.to_th else self.to_th

    def rivals(self, d, others):
        """others: the values the chosen d competed with (all <= d)."""
        lower = [v for v in others if v < d]
        if len(lower) < len(others):
            self.ties += 1
        if lower:
            lead = d - max(lower)
            self.to_next = lead if self.to_next is None or lead < self.to_next else self.to_next

    def floats(self):
        f = lambda v: float('inf') if v is None else float(v)
        return {'to_threshold': f(self.to_th), 'to_next': f(self.to_next), 'ties': self.ties}


def chain(records, ok, ubm, r, threshold, max_spk=0):
    """spkd_clr_link on exact values -> (merges [(a, b, d as a Fraction)], stat_max, stat_min, finite,
    margins): the positions are those of the shrinking list (speakers.pop(b))."""
    m = Model(ubm, r)
    raw = [np.array(x, dtype=np.float64) for x in records]
    good = [bool(k) for k in ok]
    recs = [Record(x, m) if k else None for x, k in zip(raw, good)]
    th = Fraction(float(threshold))
    mar = Margins()
    val = {}
    for a in range(len(recs)):
        for b in range(a + 1, len(recs)):
            if good[a] and good[b]:
                val[(a, b)] = _clr(recs[a], recs[b], m)
    if any(v is None for v in val.values()):
        fin = [v for v in val.values() if v is not None]
        return [], (max(fin) if fin else None), (min(fin) if fin else None), False, mar
    smax, smin = (max(val.values()), min(val.values())) if val else (None, None)
    merges = []
    while val:
        d = max(val.values())
        a, b = min(p for p, v in val.items() if v == d)                 # the first in row-major order
        forced = max_spk > 0 and len(recs) > max_spk
        if not forced:
            mar.threshold(d, th)
        if not (d > th or forced):
            break
        mar.rivals(d, [v for p, v in val.items() if p != (a, b)])
        merges.append((a, b, d))
        raw[a] = merged(raw[a], raw.pop(b))
        good.pop(b)
        recs.pop(b)
        recs[a] = Record(raw[a], m)
        shift = lambda x: x - (x > b)
        val = {(shift(p), shift(q)): v for (p, q), v in val.items() if b not in (p, q) and a not in (p, q)}
        for x in range(len(recs)):
            if x != a and good[x]:
                v = _clr(recs[min(a, x)], recs[max(a, x)], m)
                if v is None:
                    return merges, smax, smin, False, mar
                val[(min(a, x), max(a, x))] = v
    return merges, smax, smin, True, mar


def labels_from_merges(n, merges):
    groups = [[i] for i in range(n)]
    for a, b, _ in merges:
        groups[a].extend(groups.pop(b))
    out = [0] * n
    for k, g in enumerate(groups):
        for i in g:
            out[i] = k + 1
    return out


def scores(probes, probe_ok, gallery, gallery_ok, ubm, r):
    """([S][G] of Fractions, None where a side is not ok, 'nan' where the value is not finite; finite)."""
    m = Model(ubm, r)
    ps = [Record(x, m) if k else None for x, k in zip(probes, probe_ok)]
    gs = [Record(x, m) if k else None for x, k in zip(gallery, gallery_ok)]
    out, fin = [], True
    for p in ps:
        row = []
        for g in gs:
            v = None
            if p is not None and g is not None:
                v = _clr(p, g, m)
                if v is None:
                    v, fin = 'nan', False
            row.append(v)
        out.append(row)
    return out, fin


def assign(mat, probe_ok, gallery_ok, group_off, threshold, exclusive=True):
    """spkd_clr_identify's decisions on the exact matrix -> (ident, score, second, margins); score and
    second are Fractions or None (the device's NaN)."""
    n_s = len(mat)
    cols = [g for g in range(len(gallery_ok)) if gallery_ok[g]]
    th = Fraction(float(threshold))
    ident = [-1] * n_s
    mar = Margins()

    def best(s, free):
        """(value, column): the highest of row s over free (ascending), the lowest column on a tie."""
        j = max(free, key=lambda c: (mat[s][c], -c))
        return mat[s][j], j

    for lo, hi in zip(group_off[:-1], group_off[1:]):
        rows = [s for s in range(int(lo), int(hi)) if probe_ok[s]]
        if not cols:
            continue
        if not exclusive:
            for s in rows:
                v, j = best(s, cols)
                mar.threshold(v, th)
                mar.rivals(v, [mat[s][c] for c in cols if c != j])
                if v > th:
                    ident[s] = j
            continue
        free = list(cols)
        while rows and free:
            v, s, j = max((mat[s][c], -s, -c) for s in rows for c in free)
            s, j = -s, -j
            mar.threshold(v, th)
            if not v > th:
                break
            mar.rivals(v, [mat[x][c] for x in rows for c in free if (x == s) != (c == j)])
            ident[s] = j
            rows.remove(s)
            free.remove(j)
    score, second = [None] * n_s, [None] * n_s
    for s in range(n_s):
        if not probe_ok[s] or not cols:
            continue
        j = ident[s] if ident[s] >= 0 else best(s, cols)[1]
        score[s] = mat[s][j]
        rest = [c for c in cols if c != j]
        if rest:
            second[s] = best(s, rest)[0]
    return ident, score, second, mar
