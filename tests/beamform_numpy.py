"""The three beamforming stages of include/spkd.h (6b2), restated in numpy (float64 transforms, the
correlation rounded to float32 where the header says), and the synthetic scenes the tests use.

A file is int16 [n, C]; a geometry is (H, W, D) = (hop, window, max_lag) in samples."""
import numpy as np

NFFT, NBEST = 8192, 4
GEOM_16K = (4000, 8000, 160)
# pipeline.BEAMFORM's tracking options, stated again: the fixtures are judged against these
N_BEST, MIN_PEAK, JUMP_PENALTY, JUMP_CAP = 4, 0.1, 0.02, 25
NEG = -np.inf


def steps(n, C, geom):
    H, W, _ = geom
    if C == 1:
        return 0
    return 1 if n <= W else (n - W) // H + 1


def pick_ref(x, ref=-1):
    """The reference channel: as requested, or the largest exact sum of squares (lowest index on a tie)."""
    if ref >= 0:
        return int(ref)
    e = [sum(int(v) * int(v) for v in x[:, c].tolist()) for c in range(x.shape[1])]     # Python integers: exact
    return int(max(range(len(e)), key=lambda c: (e[c], -c)))


def window(x, t, geom):
    """float64 [NFFT, C]: step t's frames, zero beyond the file and beyond the window."""
    H, W, _ = geom
    out = np.zeros((NFFT, x.shape[1]))
    part = x[t * H:t * H + W]
    out[:len(part)] = part
    return out


def curve(x, ref, geom, dtype=np.float32):
    """v[t, c, d + D]; the reference channel's row is 1 at lag 0 by definition."""
    D = geom[2]
    T, C = steps(len(x), x.shape[1], geom), x.shape[1]
    out = np.zeros((T, C, 2 * D + 1), dtype=dtype)
    lags = np.arange(-D, D + 1) % NFFT
    for t in range(T):
        w = window(x, t, geom)
        A = np.fft.fft(w[:, ref])
        for c in range(C):
            if c == ref:
                out[t, c, D] = 1.0
                continue
            P = np.fft.fft(w[:, c]) * np.conj(A)
            mag = np.abs(P)
            G = np.where(mag > 0, P / np.where(mag > 0, mag, 1.0), 0.0)
            out[t, c] = np.fft.ifft(G).real[lags].astype(dtype)
    return out


def select(v, D):
    """The candidates of one curve v[2 D + 1]: (lag int32 [4], value float32 [4])."""
    v = np.asarray(v)
    up = np.concatenate([[True], v[1:] > v[:-1]])
    down = np.concatenate([v[:-1] >= v[1:], [True]])
    idx = np.nonzero(up & down)[0]
    order = idx[np.lexsort((idx, -v[idx].astype(np.float64)))][:NBEST]
    lag = np.full(NBEST, order[0] - D, dtype=np.int32)
    val = np.full(NBEST, NEG, dtype=np.float32)
    lag[:len(order)] = order - D
    val[:len(order)] = v[order]
    return lag, val


def candidates(curves, ref, D):
    """(lag int32 [T, C, 4], val float32 [T, C, 4]) of curves [T, C, 2 D + 1]."""
    T, C = curves.shape[:2]
    lag = np.zeros((T, C, NBEST), dtype=np.int32)
    val = np.full((T, C, NBEST), NEG, dtype=np.float32)
    for t in range(T):
        for c in range(C):
            if c == ref:
                val[t, c, 0] = 1.0
            else:
                lag[t, c], val[t, c] = select(curves[t, c], D)
    return lag, val


def _filled(lag, val, n_best, min_peak):
    """One channel's steps as the Viterbi sees them: (lags [T, 4] int, values [T, 4] float, reliable [T])."""
    T = len(lag)
    reliable = np.array([np.float32(val[t, 0]) >= np.float32(min_peak) for t in range(T)], dtype=bool)
    good = np.nonzero(reliable)[0]
    L, V = [], []
    for t in range(T):
        if reliable[t]:
            src = t
        elif len(good) == 0:
            src = None
        else:
            earlier = good[good < t]
            src = int(earlier[-1]) if len(earlier) else int(good[0])
        if src is None:
            L.append([0] * NBEST)
            V.append([0.0] + [NEG] * (NBEST - 1))
            continue
        x = [float(val[src, k]) if k < n_best else NEG for k in range(NBEST)]
        L.append([int(v) for v in lag[src]])
        V.append(x if reliable[t] else [NEG if v == NEG else 0.0 for v in x])
    return L, V, reliable


def _cost(a, b, penalty, cap):
    return penalty * float(min(abs(a - b), cap))


def track_channel(lag, val, n_best=N_BEST, min_peak=MIN_PEAK, penalty=JUMP_PENALTY, cap=JUMP_CAP, margin=False):
    """One channel: lag [T, 4], val [T, 4] -> (delay int32 [T], reliable bool [T]); with margin, also the
    score of the winning path minus the best score of a path through a slot with another lag."""
    T = len(lag)
    if T == 0:
        return (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=bool)) + ((np.inf,) if margin else ())
    L, V, reliable = _filled(lag, val, n_best, min_peak)
    S = [list(V[0])]
    back = [[0] * NBEST]
    for t in range(1, T):
        row, bp = [], []
        for k in range(NBEST):
            best, arg = None, 0
            for j in range(NBEST):
                s = S[-1][j] - _cost(L[t][k], L[t - 1][j], penalty, cap)      # a multiply, then a subtract
                if best is None or s > best:
                    best, arg = s, j
            row.append(best + V[t][k])
            bp.append(arg)
        S.append(row)
        back.append(bp)
    k = max(range(NBEST), key=lambda j: (S[-1][j], -j))
    top = S[-1][k]
    delay = np.zeros(T, dtype=np.int32)
    for t in range(T - 1, -1, -1):
        delay[t] = L[t][k]
        k = back[t][k]
    if not margin:
        return delay, reliable
    # the best continuation behind every (t, k), for the score of the best path through it
    B = [[0.0] * NBEST for _ in range(T)]
    for t in range(T - 2, -1, -1):
        for j in range(NBEST):
            B[t][j] = max(B[t + 1][k] + V[t + 1][k] - _cost(L[t + 1][k], L[t][j], penalty, cap) for k in range(NBEST))
    other = [S[t][k] + B[t][k] for t in range(T) for k in range(NBEST) if L[t][k] != delay[t] and S[t][k] > NEG]
    return delay, reliable, top - max(other + [NEG])


def track(lag, val, **kw):
    """lag, val [T, C, 4] -> (delay int32 [T, C], reliable bool [T, C])."""
    T, C = lag.shape[:2]
    delay = np.zeros((T, C), dtype=np.int32)
    reliable = np.zeros((T, C), dtype=bool)
    for c in range(C):
        delay[:, c], reliable[:, c] = track_channel(lag[:, c], val[:, c], **kw)
    return delay, reliable


def delay_sum(x, geom, delay):
    """int16 [n, C] and delay [T, C] -> int16 [n]."""
    H, W, _ = geom
    n, C = x.shape
    if C == 1:
        return x[:, 0].copy()
    T = len(delay)
    s = np.arange(n, dtype=np.int64)
    a0 = W // 2
    inner = (s >= a0) & (s < (T - 1) * H + a0)
    t0 = np.where(inner, (s - a0) // H, np.where(s < a0, 0, T - 1))
    t1 = np.where(inner, t0 + 1, t0)
    j = np.where(inner, (s - a0) % H, 0)
    num = np.zeros(n, dtype=np.int64)
    xl = x.astype(np.int64)
    for c in range(C):
        for t, wgt in ((t0, H - j), (t1, j)):
            i = s + delay[t, c].astype(np.int64)
            ok = (i >= 0) & (i < n)
            num += wgt * np.where(ok, xl[np.clip(i, 0, max(n - 1, 0)), c], 0)
    y = np.rint(num.astype(np.float64) / np.float64(C * H))
    return np.clip(y, -32768, 32767).astype(np.int16)


def beamform(x, geom, ref=-1, **kw):
    """The whole chain on one file -> dict(ref, curve, lag, val, delay, reliable, out)."""
    if x.shape[1] == 1:
        e = np.zeros((0, 1), dtype=np.int32)
        return dict(ref=0, curve=np.zeros((0, 1, 2 * geom[2] + 1), dtype=np.float32), lag=np.zeros((0, 1, NBEST), dtype=np.int32),
                    val=np.zeros((0, 1, NBEST), dtype=np.float32), delay=e, reliable=e.astype(bool), out=x[:, 0].copy())
    r = pick_ref(x, ref)
    cv = curve(x, r, geom)
    lag, val = candidates(cv, r, geom[2])
    delay, reliable = track(lag, val, **kw)
    return dict(ref=r, curve=cv, lag=lag, val=val, delay=delay, reliable=reliable, out=delay_sum(x, geom, delay))


# ------------------------------------------------------------------ scenes
PAD = 4096          # source samples in front of frame 0, so that every delay finds some


def _source(rng, n, coloured=False, amp=3000.0):
    s = rng.standard_normal(n + 2 * PAD)
    if coloured:                                  # lightly: one zero at 0.5, rescaled to the same power
        s = (s + 0.5 * np.concatenate([[0.0], s[:-1]])) / np.sqrt(1.25)
    return amp * s


def _delayed(s, n, d):
    """x[i] = s[i - d] for i in [0, n)."""
    return s[PAD - d:PAD - d + n]


def _quantise(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def scene(name):
    """-> dict(x int16 [n, C], geom, truth: [(first frame, last frame, delays)], clean: float64 [n] or None).
    `truth` lists the stretches of one delay setting."""
    rng = np.random.default_rng({'S1': 101, 'S1c': 102, 'S2': 103, 'S3': 104, 'S4': 105, 'S5': 106}[name])
    noise = 3000.0 / np.sqrt(10.0)                # independent noise 10 dB down
    if name in ('S1', 'S1c', 'S3'):
        n, d = 48000, (0, 37, -160, 5)
        s = _source(rng, n, coloured=name == 'S1c')
        x = np.stack([_delayed(s, n, k) for k in d], axis=1) + noise * rng.standard_normal((n, 4))
        if name == 'S3':                          # an intruder during one window only, at other delays
            s2 = _source(rng, n)
            for c, (k, amp) in enumerate(zip((0, -70, 60, -120), (3300.0, 3500.0, 3800.0, 4000.0))):
                x[20000:28000, c] += (amp / 3000.0) * _delayed(s2, n, k)[20000:28000]
        return dict(x=_quantise(x), geom=GEOM_16K, truth=[(0, n, d)], clean=_delayed(s, n, 0))
    if name == 'S2':
        n, cut, d0, d1 = 48000, 22400, (0, 37, -160, 5), (0, -12, 90, 5)
        s = _source(rng, n)
        x = np.stack([np.concatenate([_delayed(s, n, a)[:cut], _delayed(s, n, b)[cut:]]) for a, b in zip(d0, d1)], axis=1)
        x = x + noise * rng.standard_normal((n, 4))
        return dict(x=_quantise(x), geom=GEOM_16K, truth=[(0, cut, d0), (cut, n, d1)], clean=None)
    if name == 'S4':                              # half a second of source, 1 s of digital silence, 1 s of noise, source
        n, d = 48000, (0, 37)
        s = _source(rng, n)
        x = np.stack([_delayed(s, n, k) for k in d], axis=1) + noise * rng.standard_normal((n, 2))
        x[8000:24000] = 0.0
        x[24000:40000] = 3.0 * rng.standard_normal((16000, 2))
        return dict(x=_quantise(x), geom=GEOM_16K, truth=[(0, n, d)], clean=None)
    if name == 'S5':
        n, d = 5000, (0, 9, 0)
        s = _source(rng, n)
        x = np.stack([_delayed(s, n, k) for k in d], axis=1) + noise * rng.standard_normal((n, 3))
        x[:, 2] = 0.0
        return dict(x=_quantise(x), geom=GEOM_16K, truth=[(0, n, d)], clean=None)
    raise KeyError(name)


SCENES = ('S1', 'S1c', 'S2', 'S3', 'S4', 'S5')


def snr_db(y, clean):
    """Signal-to-noise ratio of y against the clean source, at the gain that fits it best."""
    y, clean = np.asarray(y, dtype=np.float64), np.asarray(clean, dtype=np.float64)
    g = np.dot(y, clean) / np.dot(clean, clean)
    return 10.0 * np.log10(np.dot(g * clean, g * clean) / np.dot(y - g * clean, y - g * clean))
