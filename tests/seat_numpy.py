"""CPU restatement of the seat stages (include/spkd.h (6b4)) -- TEST INFRASTRUCTURE ONLY.

PARITY: no reference counterpart.  What the two calls compute is stated here, in the order csrc/spkd_seat.hpp states it:

  g         of one channel (n, sx, sxx) of a record: dn = float(n); mean = float(sx) / dn; v = float(sxx) / dn - mean *
            mean; var = v if v > floor_f else floor_f; g = dn * log(var).  numpy float64, one rounding per operation;
            floor_f = (floor_s * rate_in)^2.
  delta     over the channels c < C, c != ref with n_A >= m and n_B >= m, ascending, from d = 0: t = g(A + B) - g(A);
            t = t - g(B); t = 0.5 * t; t = t / w; p = float(n_A + n_B) / w; p = log(p); p = lambdac * p; d = d + (t - p),
            with w = float(H * rate_out) / float(hop * rate_in).  None when no channel counts.  Beside it S, the sum the
            device tolerance scales with: sum over counted c of (|g(A+B)| + |g(A)| + |g(B)|) / (2 w) + |lambdac log(n / w)|.
  cuts      per range the candidates t in (b, e) with step(t) != step(t - 1), t - b >= min_piece, e - t >= min_piece;
            the value of a candidate is delta(moments of [b, t), moments of [t, e)), the moments summed frame by frame
            in integers; the highest defined delta, the lowest frame among equals; a cut iff that delta > threshold.
  split     the chain over the placed records of a problem: the pair a < b with the lowest defined delta, the first in
            row-major order on a tie; merged iff not (delta > threshold); record[a] += record[b], pop(b).

cut_loop and split_labels restate what seats.seat_cut_batch and seats.seat_split_batch do with those calls, on frames.
perturb: None, or a function d -> d' every delta goes through before any decision reads it (the tie test).

A file is tdoa_numpy's dict(delay int [T, C], reliable bool [T, C], ref, H, rate_in, frame0); the clock (hop, window, rate_out)."""
import math

import numpy as np

MAX_CH = 8


def file_w(f, clock):
    hop, window, rate_out = clock
    return np.float64(int(f['H']) * int(rate_out)) / np.float64(int(hop) * int(f['rate_in']))


def floor_f(f, floor_s):
    fr = np.float64(floor_s) * np.float64(int(f['rate_in']))
    return fr * fr


def g(n, sx, sxx, fl):
    dn = np.float64(n)
    mean = np.float64(sx) / dn
    v = np.float64(sxx) / dn - mean * mean
    var = v if v > fl else fl
    return dn * np.float64(math.log(var))


def delta(A, B, f, clock, m, floor_s, lambdac, perturb=None):
    """A, B: records [8][3] of Python integers -> (delta or None, S)."""
    C = np.asarray(f['delay']).shape[1]
    w, fl = file_w(f, clock), floor_f(f, floor_s)
    d, S, any_ = np.float64(0.0), 0.0, False
    for c in range(min(C, MAX_CH)):
        if C < 2 or c == f['ref']:
            continue
        na, nb = int(A[c][0]), int(B[c][0])
        if na >= m and nb >= m:
            gs = g(na + nb, int(A[c][1]) + int(B[c][1]), int(A[c][2]) + int(B[c][2]), fl)
            ga, gb = g(na, int(A[c][1]), int(A[c][2]), fl), g(nb, int(B[c][1]), int(B[c][2]), fl)
            t = gs - ga
            t = t - gb
            t = np.float64(0.5) * t
            t = t / w
            p = np.float64(na + nb) / w
            p = np.float64(math.log(p))
            p = np.float64(lambdac) * p
            d = d + (t - p)
            S += (abs(gs) + abs(ga) + abs(gb)) / (2.0 * w) + abs(p)
            any_ = True
    if not any_:
        return None, 0.0
    return (float(d) if perturb is None else float(perturb(float(d)))), float(S)


def steps(f, clock, b, e):
    """The step of every file-local frame of [b, e): the forward rule, vectorised in int64."""
    hop, window, rate_out = clock
    T = len(f['delay'])
    t = np.arange(int(b), int(e), dtype=np.int64)
    return np.minimum(T - 1, ((t * hop + window // 2) * int(f['rate_in'])) // (rate_out * int(f['H'])))


def prefix_moments(f, clock, b, e):
    """Per channel the exact sums over the frames [b, b + i) for i = 0 .. e - b: int64 [e - b + 1, 8, 3] (a range of
    fewer than 2^31 frames at |x| <= 4096 stays inside int64)."""
    k = steps(f, clock, b, e)
    delay, rel = np.asarray(f['delay'], dtype=np.int64), np.asarray(f['reliable'], dtype=bool)
    out = np.zeros((len(k) + 1, MAX_CH, 3), dtype=np.int64)
    for c in range(delay.shape[1]):
        if c == f['ref']:
            continue
        r, x = rel[k, c].astype(np.int64), delay[k, c]
        out[1:, c, 0], out[1:, c, 1], out[1:, c, 2] = np.cumsum(r), np.cumsum(r * x), np.cumsum(r * x * x)
    return k, out


def cuts(files, clock, ranges, min_piece, m, floor_s, lambdac, threshold, perturb=None):
    """ranges = [(begin, end, file)] in the batch's numbering -> [(cut frame or -1, best delta or None, its S)]."""
    out = []
    for b0, e0, fi in ranges:
        f = files[fi]
        T, C = np.asarray(f['delay']).shape
        b, e = int(b0) - int(f['frame0']), int(e0) - int(f['frame0'])
        best = (-1, None, 0.0)
        if C > 1 and T > 0 and e > b:
            k, pre = prefix_moments(f, clock, b, e)
            tot = pre[-1]
            for i in np.nonzero(k[1:] != k[:-1])[0] + 1:
                if i < min_piece or (e - b) - i < min_piece:
                    continue
                d, S = delta(pre[i].tolist(), (tot - pre[i]).tolist(), f, clock, m, floor_s, lambdac, perturb)
                if d is not None and (best[1] is None or d > best[1]):
                    best = (b + int(i) + int(f['frame0']), d, S)
        out.append((best[0] if best[1] is not None and best[1] > threshold else -1, best[1], best[2]))
    return out


def placed(rec, f, m):
    C = np.asarray(f['delay']).shape[1]
    return C > 1 and any(int(rec[c][0]) >= m for c in range(C) if c != f['ref'])


def split(records, f, clock, m, floor_s, lambdac, threshold, perturb=None):
    """records: [n][8][3] integers of one problem -> (merges [(a, b, delta, S)] in list positions, placed flags)."""
    recs = [[[int(v) for v in ch] for ch in r] for r in records]
    ok = [placed(r, f, m) for r in recs]
    flags = list(ok)
    mat = {}

    def pair(i, j):
        mat[(i, j)] = delta(recs[i], recs[j], f, clock, m, floor_s, lambdac, perturb) if ok[i] and ok[j] else (None, 0.0)

    ids = list(range(len(recs)))                          # the clusters' keys in `mat`, in list order
    for x in range(len(recs)):
        for y in range(x + 1, len(recs)):
            pair(x, y)
    merges = []
    while True:
        best = None
        for x in range(len(ids)):
            for y in range(x + 1, len(ids)):
                d, S = mat[(ids[x], ids[y])]
                if d is not None and (best is None or d < best[2]):
                    best = (x, y, d, S)
        if best is None or best[2] > threshold:
            break
        a, b = best[0], best[1]
        merges.append(best)
        ia, ib = ids[a], ids[b]
        recs[ia] = [[u + v for u, v in zip(ca, cb)] for ca, cb in zip(recs[ia], recs[ib])]
        ids.pop(b)
        for x, ix in enumerate(ids):
            if ix != ia:
                pair(min(ix, ia), max(ix, ia))
    return merges, flags


def replay(n, merges):
    """The clusters of a merge log, as lists of members, in list order."""
    clusters = [[i] for i in range(n)]
    for mg in merges:
        a, b = mg[0], mg[1]
        clusters[a] = clusters[a] + clusters[b]
        clusters.pop(b)
    return clusters


def range_record(f, clock, b, e):
    """The record of the file-local frames [b, e) as Python integers."""
    if e <= b or np.asarray(f['delay']).shape[1] < 2 or len(f['delay']) < 1:
        return [[0, 0, 0] for _ in range(MAX_CH)]
    return prefix_moments(f, clock, b, e)[1][-1].tolist()


def cut_loop(f, clock, segments, min_piece, m, floor_s, lambdac, threshold, max_passes, perturb=None):
    """seat_cut_batch on one file's frame ranges [(b, e)] -> (the pieces, the cut frames, the calls made)."""
    work = [(b, e, True) for b, e in segments]
    found, passes = [], 0
    while passes < max_passes:
        new = [i for i, s in enumerate(work) if s[2]]
        if not new:
            break
        got = cuts([f], clock, [(work[i][0], work[i][1], 0) for i in new], min_piece, m, floor_s, lambdac, threshold, perturb)
        passes += 1
        work = [(b, e, False) for b, e, _ in work]
        for i, (t, _, _) in sorted(zip(new, got), reverse=True):
            if t >= 0:
                b, e, _ = work[i]
                work[i:i + 1] = [(b, t, True), (t, e, True)]
                found.append(t)
        if all(t < 0 for t, _, _ in got):
            break
    return [(b, e) for b, e, _ in work], sorted(found), passes


def split_labels(f, clock, segments, m, floor_s, lambdac, threshold, perturb=None):
    """seat_split_batch on one problem: the segments [(b, e)] of one acoustic cluster -> (per segment its seat from 0,
    ordered by first segment; the merge log; the placed flags)."""
    recs = [range_record(f, clock, b, e) for b, e in segments]
    merges, flags = split(recs, f, clock, m, floor_s, lambdac, threshold, perturb)
    clusters = [c for c in replay(len(recs), merges) if any(flags[i] for i in c)]
    if len(clusters) < 2:
        return [0] * len(recs), merges, flags
    seat = [-1] * len(recs)
    held = []
    for s, c in enumerate(clusters):
        for i in c:
            seat[i] = s
        held.append(sum(segments[i][1] - segments[i][0] for i in c if flags[i]))
    most = held.index(max(held))
    return [s if flags[i] else most for i, s in enumerate(seat)], merges, flags
