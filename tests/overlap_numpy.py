"""CPU restatement of the overlap stage (include/spkd.h (6b5)) -- TEST INFRASTRUCTURE ONLY.

PARITY: no reference counterpart.  What the stage computes is stated here:

  second    entry i: NONE if float32(val[i, 0]) < float32(min_peak).  Else the slots k = 0 .. n_best - 1 in order; the
            first with a finite value and |lag[i, k] - delay[i]| > guard is the runner-up: its lag if float32(value) >=
            float32(min_second), else NONE; NONE when no slot qualifies.
  near      lag x is near a model (mean, var, inv2var, ln) iff ((x - mean) * (x - mean)) * inv2var <= gate in numpy
            float64, one rounding per operation.
  raw pair  per step: over the channels that are live, not the reference, and hold both a tracked delay p and a
            runner-up q, channel c agrees with j < k iff (p near j and q near k) or (q near j and p near k).  The pair
            with the most agreeing channels, the lexicographically smallest among equals, if that count >=
            min(min_channels, live channels) and >= 1; else (-1, -1).  No live channel, fewer than two speakers, one
            channel: (-1, -1).
  runs      a step keeps its raw pair iff it lies in a run of >= min_steps consecutive steps with that pair.

A file is tdoa_numpy's dict(delay, reliable, ref, H, rate_in, frame0) with `second` int [T, C] (NONE: none) beside it.
The scenes of the CPU tests are built here from beamform_numpy's helpers."""
import numpy as np

import beamform_numpy as B
import tdoa_numpy as TD

NONE = TD.NONE


def second(delay, lag, val, n_best, min_peak, min_second, guard):
    """delay int [n], lag int [n, 4], val float32 [n, 4] -> int32 [n]."""
    delay, lag, val = np.asarray(delay).reshape(-1), np.asarray(lag).reshape(-1, 4), np.asarray(val, dtype=np.float32).reshape(-1, 4)
    out = np.full(len(delay), NONE, dtype=np.int64)
    for i in range(len(delay)):
        if not val[i, 0] >= np.float32(min_peak):
            continue
        for k in range(n_best):
            if np.isfinite(val[i, k]) and abs(int(lag[i, k]) - int(delay[i])) > guard:
                if val[i, k] >= np.float32(min_second):
                    out[i] = int(lag[i, k])
                break
    return out.astype(np.int32)


def near(x, model, gate):
    d = np.float64(int(x)) - np.float64(model[0])
    t = d * d
    t = t * np.float64(model[2])
    return bool(t <= np.float64(gate))


def raw_pairs(f, models, live, gate, min_channels):
    """f: a file with `second`; models float64 [n_spk, 8, 4] of the file's speakers; live: the file's mask.
    -> [(j, k)] per step."""
    delay, reliable, sec = np.asarray(f['delay']), np.asarray(f['reliable']), np.asarray(f['second'])
    T, C = delay.shape
    n_spk = len(models)
    chans = [c for c in range(C) if C > 1 and (int(live) >> c) & 1 and c != f['ref']]
    need = min(int(min_channels), len(chans))
    out = []
    for t in range(T):
        if n_spk < 2 or need < 1:
            out.append((-1, -1))
            continue
        P, Q = {}, {}
        for c in chans:
            if reliable[t, c] and int(sec[t, c]) != NONE:
                P[c] = [near(delay[t, c], models[j][c], gate) for j in range(n_spk)]
                Q[c] = [near(sec[t, c], models[j][c], gate) for j in range(n_spk)]
        best, pair = 0, (-1, -1)
        for j in range(n_spk):
            for k in range(j + 1, n_spk):
                n = sum(1 for c in P if (P[c][j] and Q[c][k]) or (Q[c][j] and P[c][k]))
                if n > best:
                    best, pair = n, (j, k)
        out.append(pair if best >= need else (-1, -1))
    return out


def run_filter(raw, min_steps):
    T = len(raw)
    out = []
    for t in range(T):
        if raw[t][0] < 0:
            out.append((-1, -1))
            continue
        a = t
        while a > 0 and raw[a - 1] == raw[t]:
            a -= 1
        b = t
        while b + 1 < T and raw[b + 1] == raw[t]:
            b += 1
        out.append(raw[t] if b - a + 1 >= min_steps else (-1, -1))
    return out


def overlap(files, models, live, spk_off, gate, min_channels, min_steps):
    """-> per file int32 [T, 2]."""
    out = []
    for fi, f in enumerate(files):
        m = models[int(spk_off[fi]):int(spk_off[fi + 1])]
        got = run_filter(raw_pairs(f, m, live[fi], gate, min_channels), min_steps)
        out.append(np.array(got, dtype=np.int32).reshape(-1, 2))
    return out


def detected(steps):
    return [t for t, (j, k) in enumerate(np.asarray(steps).reshape(-1, 2).tolist()) if j >= 0]


# ------------------------------------------------------------------ scenes
SEAT_1, SEAT_2 = (0, 37, -160, 5), (0, -70, 60, -120)         # scene S3's talker and its intruder
N, LO, HI = 48000, 16000, 32000                               # two talkers: 1 alone to LO, both to HI, 2 alone after
FULL, PART = (4, 5, 6), (3, 4, 5, 6, 7)                       # the steps wholly inside the overlap; those that touch it


def two_talkers(db_down=0.0, seed=301):
    """Two white sources at scene S3's two seats, the second db_down below the first, independent noise 10 dB below the
    first: the first talks over [0, HI), the second over [LO, N) -> int16 [N, 4]."""
    rng = np.random.default_rng(seed)
    s1, s2 = B._source(rng, N), B._source(rng, N, amp=3000.0 * 10.0 ** (-db_down / 20.0))
    x = (3000.0 / np.sqrt(10.0)) * rng.standard_normal((N, 4))
    for c in range(4):
        x[:HI, c] += B._delayed(s1, N, SEAT_1[c])[:HI]
        x[LO:, c] += B._delayed(s2, N, SEAT_2[c])[LO:]
    return B._quantise(x)


def analysed(x, ref=0, n_best=B.N_BEST, min_peak=B.MIN_PEAK, min_second=0.1, guard=3):
    """The beamformer's restatement on one file, then the runner-up rule -> a file with `second`, and (lag, val)."""
    r = B.beamform(x, B.GEOM_16K, ref)
    T, C = r['delay'].shape
    sec = second(r['delay'].ravel(), r['lag'].reshape(-1, 4), r['val'].reshape(-1, 4), n_best, min_peak, min_second, guard).reshape(T, C)
    f = dict(delay=r['delay'], reliable=r['reliable'], ref=r['ref'], H=B.GEOM_16K[0], rate_in=16000, frame0=0, second=sec)
    return f, r['lag'], r['val']


def seat_models(seats, floor_s=1.0 / 16000.0, rate_in=16000):
    """One model per seat at the variance floor, as tdoa_numpy.models writes a model: float64 [n, 8, 4]."""
    fr = np.float64(floor_s) * np.float64(rate_in)
    var = fr * fr
    out = np.zeros((len(seats), TD.MAX_CH, 4))
    out[:, :, 1] = var
    for j, seat in enumerate(seats):
        for c, d in enumerate(seat):
            out[j, c] = (np.float64(d), var, np.float64(1.0) / (np.float64(2.0) * var), -0.5 * np.log(TD.TWO_PI * var))
    return out
