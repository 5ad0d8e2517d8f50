"""Vectorised float64 restatement of the CLR matrix, the chain and the gallery's assignment for sizes
the loops of tests/link_clr_numpy.py and tests/gallery_numpy.py cannot reach -- TEST INFRASTRUCTURE ONLY.

The values are link_clr_numpy.clr's in the derived form of spkd_clr.hpp's header: per record
T[c][0] = -sum_d 1/2 (m^2 - mu^2) / var, T[c][1 + d] = (m - mu) / var, N = sum_c n_c (component order),
H(a|b) = (R_a . T_b) / N_a, so the matrix is (R T^t) / N plus its transpose: one matrix product.  The
product is numpy.einsum's, which adds the terms of every dot product in one order wherever the pair
sits, so identical records give identical bits (a BLAS tiles the matrix and need not: planted ties would
come out in an order of its own); the order is not the device's, and the values agree with the loops' to
1e-12, not to the bit.  The chain keeps every cluster in its slot, recomputes only row and column a after a merge
(two matrix-vector products) and states positions in the shrinking list by counting the live slots
below; the assignment works on whole rows.

Every decision function also returns its margins, in the sense of gallery_numpy.margins: dict(
to_threshold: the least distance of a compared value from the threshold, to_next: the least lead of a
chosen pair over the best pair of a LOWER value it competed with, ties: how many choices had a rival of
exactly the same value).  A case is sound when its margins dwarf the error of float64 (1e-14 here).
"""
import numpy as np

import link_clr_numpy as L
import reseg_gmm_numpy as G


def derive(rec, ubm, r):
    """(T [n, C, 40], N [n]) of records [n, C, 40]."""
    rec = np.asarray(rec, dtype=np.float64)
    ubm = np.asarray(ubm, dtype=np.float64).reshape(-1, G.COMP)
    mu, iv = ubm[:, G.MEAN:G.IVAR], ubm[:, G.IVAR:G.NORM]
    with np.errstate(all='ignore'):
        m = (rec[:, :, 1:] + r * mu) / (rec[:, :, :1] + r)
        T = np.empty_like(rec)
        T[:, :, 1:] = (m - mu) * iv
        T[:, :, 0] = -(0.5 * (m * m - mu * mu) * iv).sum(axis=2)
    N = np.zeros(len(rec))
    for c in range(rec.shape[1]):
        N = N + rec[:, c, 0]
    return T, N


def _flat(x):
    return x.reshape(len(x), x.shape[1] * x.shape[2])


def _dots(A, B):
    """[len(A), len(B)]: every dot product, each summed in the same order."""
    return np.einsum('ie,je->ij', _flat(A), _flat(B))


def cross(Ra, Ta, Na, Rb, Tb, Nb):
    """[len(a), len(b)]: CLR of every record of a with every record of b."""
    with np.errstate(all='ignore'):
        return _dots(Ra, Tb) / Na[:, None] + (_dots(Rb, Ta) / Nb[:, None]).T


def square(R, T, N):
    """[n, n]: CLR of every two of the records; one product."""
    with np.errstate(all='ignore'):
        h = _dots(R, T) / N[:, None]
        return h + h.T


def _margins():
    return {'to_threshold': np.inf, 'to_next': np.inf, 'ties': 0}


def _rival(mar, v, other):
    """other: the highest value the chosen v competed with (-inf: none)."""
    if other == v:
        mar['ties'] += 1
    elif other > -np.inf:
        mar['to_next'] = min(mar['to_next'], float(v - other))


def clr_link(records, ok, ubm, r, threshold, max_spk=0):
    """link_clr_numpy.clr_link -> (merges [(a, b, d)], stat_max, stat_min, finite, margins)."""
    R = np.array(records, dtype=np.float64)
    n = len(R)
    good = np.asarray(ok) != 0
    mar = _margins()
    nan = float('nan')
    if n == 0:
        return [], nan, nan, True, mar
    T, N = derive(R, ubm, r)
    pair = good[:, None] & good[None, :] & np.triu(np.ones((n, n), dtype=bool), 1)
    mat = np.where(pair, square(R, T, N), -np.inf)
    vals = mat[pair]
    fin = bool(np.isfinite(vals).all())
    seen = vals[np.isfinite(vals)]
    smax, smin = (float(seen.max()), float(seen.min())) if len(seen) else (nan, nan)
    merges = []
    if not fin:
        return merges, smax, smin, False, mar
    alive = np.ones(n, dtype=bool)
    live = n
    while True:
        flat = int(np.argmax(mat))                                     # (the first in row-major order)
        a, b = flat // n, flat % n
        d = float(mat[a, b])
        if d == -np.inf:
            break
        forced = max_spk > 0 and live > max_spk
        if not forced:
            mar['to_threshold'] = min(mar['to_threshold'], abs(d - threshold))
        if not (d > threshold or forced):
            break
        mat[a, b] = -np.inf
        _rival(mar, d, float(mat.max()))
        merges.append((int(alive[:a].sum()), int(alive[:b].sum()), d))
        live -= 1
        R[a] = R[a] + R[b]
        alive[b] = False
        mat[b, :] = -np.inf
        mat[:, b] = -np.inf
        Ta, Na = derive(R[a:a + 1], ubm, r)
        T[a], N[a] = Ta[0], Na[0]
        x = np.nonzero(alive & good)[0]
        x = x[x != a]
        v = cross(R[a:a + 1], T[a:a + 1], N[a:a + 1], R[x], T[x], N[x])[0]
        if not np.isfinite(v).all():
            return merges, smax, smin, False, mar
        lo = x < a
        mat[x[lo], a] = v[lo]
        mat[a, x[~lo]] = v[~lo]
    return merges, smax, smin, True, mar


def scores(probes, probe_ok, gallery, gallery_ok, ubm, r):
    """gallery_numpy.scores -> (mat [S, G], finite)."""
    P, Q = np.asarray(probes, dtype=np.float64), np.asarray(gallery, dtype=np.float64)
    pok, gok = np.asarray(probe_ok) != 0, np.asarray(gallery_ok) != 0
    Tp, Np = derive(P, ubm, r)
    Tg, Ng = derive(Q, ubm, r)
    both = pok[:, None] & gok[None, :]
    mat = np.where(both, cross(P, Tp, Np, Q, Tg, Ng), np.nan)
    return mat, bool(np.isfinite(mat[both]).all())


def _top2(rows):
    """Per row of rows [m, G] (-inf: a column that is not there): (the highest value, its lowest column,
    the highest over the other columns)."""
    j = np.argmax(rows, axis=1)
    at = np.arange(len(rows))
    v = rows[at, j]
    rest = rows.copy()
    rest[at, j] = -np.inf
    return v, j, rest.max(axis=1) if rows.shape[1] else np.full(len(rows), -np.inf)


def assign(mat, probe_ok, gallery_ok, group_off, threshold, exclusive=True):
    """gallery_numpy.assign -> (ident, score, second, margins)."""
    S, Gn = mat.shape
    pok, gok = np.asarray(probe_ok) != 0, np.asarray(gallery_ok) != 0
    ident = np.full(S, -1, dtype=np.int32)
    score, second = np.full(S, np.nan), np.full(S, np.nan)
    mar = _margins()
    if not gok.any():
        return ident, score, second, mar
    base = np.where(pok[:, None] & gok[None, :], mat, -np.inf)         # (a row that is not ok: all -inf)
    v1, j1, v2 = _top2(base)
    for lo, hi in zip(group_off[:-1], group_off[1:]):
        lo, hi = int(lo), int(hi)
        rows = np.arange(lo, hi)[pok[lo:hi]]
        if not len(rows):
            continue
        if not exclusive:
            mar['to_threshold'] = min(mar['to_threshold'], float(np.abs(v1[rows] - threshold).min()))
            lead = v1[rows] - v2[rows]
            mar['ties'] += int((lead == 0.0).sum())
            if (lead > 0.0).any():
                mar['to_next'] = min(mar['to_next'], float(lead[lead > 0.0].min()))
            hit = rows[v1[rows] > threshold]
            ident[hit] = j1[hit]
            continue
        sub = base[rows].copy()                                        # a taken row or column: -inf
        while True:
            flat = int(np.argmax(sub))                                 # (the first in row-major order)
            i, j = flat // Gn, flat % Gn
            v = float(sub[i, j])
            if v == -np.inf:
                break
            mar['to_threshold'] = min(mar['to_threshold'], abs(v - threshold))
            if not v > threshold:
                break
            sub[i, j] = -np.inf
            _rival(mar, v, float(max(sub[i].max(), sub[:, j].max())))
            ident[rows[i]] = j
            sub[i, :] = -np.inf
            sub[:, j] = -np.inf
    # score and second: of a known probe the assigned pair's and the row's best other column
    known = np.nonzero(ident >= 0)[0]
    unknown = np.nonzero(pok & (ident < 0))[0]
    score[unknown] = v1[unknown]
    second[unknown] = np.where(v2[unknown] > -np.inf, v2[unknown], np.nan)
    first = ident[known] == j1[known]
    score[known] = base[known, ident[known]]
    other = np.where(first, v2[known], v1[known])
    second[known] = np.where(other > -np.inf, other, np.nan)
    return ident, score, second, mar


def identify(probes, probe_ok, group_off, gallery, gallery_ok, ubm, r, threshold, exclusive=True):
    """gallery_numpy.identify -> (ident, score, second, mat, finite, margins)."""
    mat, fin = scores(probes, probe_ok, gallery, gallery_ok, ubm, r)
    if not fin:
        S = len(mat)
        return np.full(S, -1, dtype=np.int32), np.full(S, np.nan), np.full(S, np.nan), mat, False, _margins()
    ident, score, second, mar = assign(mat, probe_ok, gallery_ok, group_off, threshold, exclusive)
    return ident, score, second, mat, True, mar
