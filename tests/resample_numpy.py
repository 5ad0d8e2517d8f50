"""numpy restatement of spkd_resample_batch (include/spkd.h, section 6b): the filter table and the
meaning of a conversion, for one file.  It builds its own table -- nothing of the package is imported
here -- and evaluates every output in float64 with the taps in ascending order, one multiply and one
add per tap, which is what the kernel's fused multiply-add gives too: a float32 tap (24 bits) times
a channel sum of at most 8 int16 (19 bits) is exact in float64.

PARITY UNPINNED: ffmpeg, whose `-ar 16000 -ac 1` this stage stands in for, is not available; the
filter is a documented choice -- 16 zero crossings to either side, Kaiser beta 9, half-amplitude
point at 0.92 of the lower Nyquist frequency."""
import math

import numpy as np

ZERO_CROSSINGS, BETA, CUTOFF = 16, 9.0, 0.92


def ratio(rate_in, rate_out):
    """(L, M, half): L = rate_out / g, M = rate_in / g, half = ceil(16 / min(1, L / M)); 0 for L == M."""
    g = math.gcd(int(rate_in), int(rate_out))
    L, M = int(rate_out) // g, int(rate_in) // g
    if L == M:
        return L, M, 0
    return L, M, (ZERO_CROSSINGS * M + L - 1) // L if M > L else ZERO_CROSSINGS


def taps(rate_in, rate_out):
    """float32 [L][2 half]: row p, column k + half - 1 holds h[p][k], k in [-half + 1, half]."""
    L, M, half = ratio(rate_in, rate_out)
    if half == 0:
        return np.zeros((L, 0), dtype=np.float32)
    fc = CUTOFF * min(1.0, L / M)
    rows = []
    for p in range(L):
        t = np.arange(-half + 1, half + 1, dtype=np.float64) - p / L
        w = np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - (t / half) ** 2))) / np.i0(BETA)
        w[np.abs(t) > half] = 0.0
        h = fc * np.sinc(fc * t) * w
        rows.append(h / math.fsum(h))
    return np.array(rows).astype(np.float32)


def n_out(n_in, rate_in, rate_out):
    L, M, _ = ratio(rate_in, rate_out)
    return -((-int(n_in) * L) // M)


def convert(samples, rate_in, rate_out, table=None):
    """samples int16 [n] or [n, channels] -> (y int16 [n_out], pre float64 [n_out]): pre is the value
    that is rounded, acc / channels.  table: another float32 table of the conversion's shape."""
    a = np.asarray(samples)
    a = (a.reshape(-1, 1) if a.ndim == 1 else a).astype(np.int64)
    C = a.shape[1]
    s = a.sum(axis=1)                                   # exact channel sums
    L, M, half = ratio(rate_in, rate_out)
    if half == 0:
        pre = s.astype(np.float64) / C
    else:
        h = (taps(rate_in, rate_out) if table is None else np.asarray(table, dtype=np.float32)).astype(np.float64)
        n = np.arange(n_out(len(s), rate_in, rate_out), dtype=np.int64)
        i, p = (n * M) // L, (n * M) % L
        # zero padding of the file: frame j is padded[j + half - 1]
        padded = np.concatenate([np.zeros(half - 1), s.astype(np.float64), np.zeros(half + 1)])
        acc = np.zeros(len(n), dtype=np.float64)
        for col in range(2 * half):                     # k = col - half + 1, ascending
            acc = acc + h[p, col] * padded[i + col]
        pre = acc / C
    y = np.clip(np.rint(pre), -32768, 32767).astype(np.int16)
    return y, pre


def near_tie(pre, margin=1e-6):
    """The samples whose value before rounding lies within `margin` of a half-integer."""
    return np.abs(pre - np.floor(pre) - 0.5) <= margin
