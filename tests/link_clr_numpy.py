"""CPU restatement (numpy, float64) of linking by UBM-MAP cross-likelihood ratio -- TEST INFRASTRUCTURE ONLY.

PARITY: no reference counterpart.  The reference links nothing across files; what spkd_ubm_stats and
spkd_clr_link compute (include/spkd.h, section 10) and what pipeline.link_batch does with LINK_CLR is
stated here.  Training and posteriors are reseg_gmm_numpy's.

  UBM       [C, 80] doubles, spkd_gmm_train's model of ONE speaker that owns the ranges of all speakers.
  record    [C, 40] doubles per speaker: n_c = sum g_c(x), f_c = sum g_c(x) x over its frames, g_c the
            responsibility of reseg_gmm_numpy.em_step.  The frames are numbered in range order, cut into
            tiles of 64 and chunks of 16 tiles; a chunk is one chain in ordinal order, the chunks are
            added in chunk order.
  merge     record a + record b, in that order.
  MAP       m_c = (f_c + r mu_c) / (n_c + r).
  H(a|b)    (1 / N_a) sum_c sum_d [(m^b_cd - mu_cd) f^a_cd - 1/2 n^a_c ((m^b_cd)^2 - mu_cd^2)] / var_cd,
            N_a = sum_c n^a_c in component order.
  CLR       H(a|b) + H(b|a); higher is more alike.
  chain     over the ok clusters the pair a < b of the highest CLR, the first in row-major order on a
            tie; merged when d > threshold or (max_spk > 0 and more than max_spk clusters are in the
            list, the not-ok ones included); record[a] += record[b], speakers.pop(b).
"""
import numpy as np

import reseg_gmm_numpy as G

DIM = G.DIM
BW_COMP = 40        # SPKD_BW_COMP
MAX_N = 4096        # SPKD_CLR_MAX_N
CHUNK = G.TILE * G.CHUNK_TILES


def frames_of(feats, ranges):
    """The frames of the ranges [(begin, end)] in range order, [N, 39] float32."""
    feats = np.asarray(feats, dtype=np.float32).reshape(-1, DIM)
    return np.concatenate([feats[b:e] for b, e in ranges] + [np.zeros((0, DIM), dtype=np.float32)])


def posteriors(x, ubm):
    """g [N, C] of the frames under the UBM: em_step's responsibilities (0 for a component whose ln w is -inf)."""
    x = G._f64(x)
    ubm = np.asarray(ubm, dtype=np.float64).reshape(-1, G.COMP)
    live = ubm[:, 0] != -np.inf
    with np.errstate(all='ignore'):
        _, e, s = G._logsumexp(G.component_loglik(x, ubm), live)
        return e / s[:, None]


def ubm_stats(x, ubm):
    """(record [C, 40], ok) of one speaker's frames x [N, 39]: a chunk of 1 024 ordinals is one chain in
    ordinal order (np.add.reduce along the first axis adds row after row), the chunks are added in
    chunk order."""
    x = G._f64(x)
    ubm = np.asarray(ubm, dtype=np.float64).reshape(-1, G.COMP)
    rec = np.zeros((len(ubm), BW_COMP))
    if len(x) == 0:
        return rec, False
    g = posteriors(x, ubm)
    ones = np.concatenate([np.ones((len(x), 1)), x], axis=1)
    with np.errstate(all='ignore'):
        for c0 in range(0, len(x), CHUNK):
            part = np.add.reduce(g[c0:c0 + CHUNK, :, None] * ones[c0:c0 + CHUNK, None, :], axis=0)
            rec = rec + part
    return rec, bool(np.isfinite(rec).all())


def train_ubm(feats, speakers, link):
    """The UBM of a linking problem: one speaker that owns the ranges of all speakers in speaker order,
    cut by ubm_ranges.  speakers: per speaker its [(begin, end)].  Returns (model [C, 80], ok)."""
    cut = ubm_ranges(speakers, link['ubm_max_frames'])
    x = frames_of(feats, [r for rs in cut for r in rs])
    model, ok, _ = G.train(x, link['components'], link['iterations'], link['var_floor'])
    return model, ok


def ubm_ranges(speakers, cap):
    """What each speaker gives to UBM training: all its ranges when the speakers hold at most `cap`
    frames, else its first floor(cap N_s / N_total) frames in ordinal order."""
    n = [sum(e - b for b, e in rs) for rs in speakers]
    total = sum(n)
    if total <= cap:
        return [list(rs) for rs in speakers]
    out = []
    for rs, ns in zip(speakers, n):
        left = cap * ns // total
        cut = []
        for b, e in rs:
            take = min(e - b, left)
            cut.append((b, b + take))
            left -= take
        out.append(cut)
    return out


def map_means(rec, ubm, r):
    ubm = np.asarray(ubm, dtype=np.float64).reshape(-1, G.COMP)
    return (rec[:, 1:] + r * ubm[:, G.MEAN:G.IVAR]) / (rec[:, :1] + r)


def total(rec):
    n = 0.0
    for c in range(len(rec)):
        n += rec[c, 0]
    return n


def half(a, b, ubm, r):
    """H(a|b): a's frames under b's adapted means against the UBM, per frame, at the UBM alignment."""
    ubm = np.asarray(ubm, dtype=np.float64).reshape(-1, G.COMP)
    mu, iv = ubm[:, G.MEAN:G.IVAR], ubm[:, G.IVAR:G.NORM]
    m = map_means(b, ubm, r)
    with np.errstate(all='ignore'):
        return float((((m - mu) * a[:, 1:] - 0.5 * a[:, :1] * (m * m - mu * mu)) * iv).sum() / total(a))


def clr(a, b, ubm, r):
    return half(a, b, ubm, r) + half(b, a, ubm, r)


def clr_link(records, ok, ubm, r, threshold, max_spk=0):
    """The chain on records [n, C, 40].  Returns (merges [(a, b, d)], stat_max, stat_min, finite):
    finite False when a CLR among ok speakers was not finite (the log so far is returned)."""
    recs = [np.array(x, dtype=np.float64) for x in records]
    good = [bool(k) for k in ok]
    n = len(recs)
    mat = np.full((n, n), -np.inf)
    merges = []

    def fill(a, b):
        mat[a, b] = clr(recs[a], recs[b], ubm, r)
        return np.isfinite(mat[a, b])

    fin = True
    for a in range(n):
        for b in range(a + 1, n):
            if good[a] and good[b]:
                fin = fill(a, b) and fin
    vals = mat[np.isfinite(mat)]
    smax, smin = (float(vals.max()), float(vals.min())) if len(vals) else (float('nan'), float('nan'))
    if not fin:
        return merges, smax, smin, False
    while True:
        if not np.isfinite(mat).any():
            break
        flat = int(np.argmax(mat))                       # (the first in row-major order)
        a, b = flat // len(recs), flat % len(recs)
        d = float(mat[a, b])
        if not (d > threshold or (max_spk > 0 and len(recs) > max_spk)):
            break
        merges.append((a, b, d))
        recs[a] = recs[a] + recs.pop(b)
        good.pop(b)
        mat = np.delete(np.delete(mat, b, axis=0), b, axis=1)
        for x in range(len(recs)):
            if x != a and good[x]:
                lo, hi = min(a, x), max(a, x)
                if not fill(lo, hi):
                    return merges, smax, smin, False
    return merges, smax, smin, True


def labels_from_merges(n, merges):
    """spkd_labels_from_merges: the final 1-based cluster of each of the n initial speakers."""
    groups = [[i] for i in range(n)]
    for a, b, _ in merges:
        groups[a].extend(groups.pop(b))
    out = np.zeros(n, dtype=np.int32)
    for k, g in enumerate(groups):
        out[g] = k + 1
    return out


def link(feats, speakers, link):
    """pipeline.link_batch(link=LINK_CLR) on speakers given as range lists: (global 1-based label per
    speaker, merges, stat_max, stat_min, records, ok, ubm)."""
    n = len(speakers)
    ubm, ubm_ok = train_ubm(feats, speakers, link)
    if not ubm_ok:
        return np.arange(1, n + 1, dtype=np.int32), [], float('nan'), float('nan'), None, None, ubm
    got = [ubm_stats(frames_of(feats, rs), ubm) for rs in speakers]
    recs, ok = [g[0] for g in got], [g[1] for g in got]
    merges, smax, smin, fin = clr_link(recs, ok, ubm, link['relevance'], link['threshold'], link['max_spk'])
    if not fin:
        raise ValueError('array must not contain infs or NaNs')
    return labels_from_merges(n, merges), merges, smax, smin, np.array(recs), np.array(ok), ubm
