"""CPU restatement of the delay stream (include/spkd.h (6b3)) -- TEST INFRASTRUCTURE ONLY.

PARITY: no reference counterpart.  What the stage computes is stated here:

  step      feature frame t of a file (file-local) belongs to step min(T - 1, ((t hop + window // 2) rate_in)
            // (rate_out H)), in Python integers (step); step_brute finds the same step by walking the
            steps' first samples.
  pack      entry = delay where float32(first candidate's value) >= float32(min_peak), NONE elsewhere.
  moments   per (set, channel) (n, sum x, sum x^2) over the frames of the set's ranges whose step is
            reliable on the channel, frame by frame, in Python integers; the reference channel and
            channels >= C stay 0.
  models    ok_c = n >= min_frames; mean = float(sx) / float(n); var = max(float(sxx) / float(n) - mean *
            mean, (floor_s rate_in)^2); 1 / (2 var); -1/2 log(2 pi var): numpy float64, one rounding per
            operation, in this order.  Not ok_c: (0, floor, 0, 0).  live: the channels that are ok_c for
            every speaker of the file whose acoustic model is ok.
  score     score + weight * sum_{c live, reliable at step(frame)} [ln_c - (x - mean_c)^2 inv_c], ascending
            c: exactly in mpmath from the model's stored doubles (score_exact, rounded once to float32),
            and in float64 in the kernel's operation order (score_f64).

A file of the stream is a dict(delay int [T, C], reliable bool [T, C], ref, H, rate_in, frame0); the clock is
(hop, window, rate_out)."""
import math

import numpy as np

NONE = -(1 << 31)
MAX_CH = 8
TWO_PI = 6.283185307179586


def step(t, clock, f):
    hop, window, rate_out = clock
    T = len(f['delay'])
    return min(T - 1, ((int(t) * hop + window // 2) * int(f['rate_in'])) // (rate_out * int(f['H'])))


def step_brute(t, clock, f):
    """The last step whose first sample, s H at rate_in, is at or before the centre of frame t's window, by
    walking the steps: compares s H / rate_in <= (t hop + window // 2) / rate_out as integers."""
    hop, window, rate_out = clock
    T, H, rate_in = len(f['delay']), int(f['H']), int(f['rate_in'])
    centre = int(t) * hop + window // 2
    s = 0
    while s + 1 < T and (s + 1) * H * rate_out <= centre * rate_in:
        s += 1
    return s


def pack(delay, val0, min_peak):
    ok = np.asarray(val0, dtype=np.float32) >= np.float32(min_peak)
    return np.where(ok, np.asarray(delay, dtype=np.int64), NONE).astype(np.int32), ok


def moments(files, clock, ranges, n_sets):
    """ranges = [(begin, end, file, set)] in the batch's frame numbering -> Python integers [n_sets][8][3]."""
    out = [[[0, 0, 0] for _ in range(MAX_CH)] for _ in range(n_sets)]
    for b, e, fi, s in ranges:
        f = files[fi]
        T, C = np.asarray(f['delay']).shape
        if C < 2 or T < 1:
            continue
        for t in range(int(b), int(e)):
            k = step(t - int(f['frame0']), clock, f)
            for c in range(C):
                if c != f['ref'] and f['reliable'][k][c]:
                    x = int(f['delay'][k][c])
                    m = out[s][c]
                    m[0] += 1
                    m[1] += x
                    m[2] += x * x
    return out


def models(stats, spk_file, ok, files, min_frames, floor_s):
    """-> (float64 [n_spk, 8, 4]: mean, var, 1 / (2 var), -1/2 log(2 pi var); live masks per file)."""
    n_spk = len(stats)
    out = np.zeros((n_spk, MAX_CH, 4))
    dead = [0] * len(files)
    for s in range(n_spk):
        f = files[spk_file[s]]
        C = np.asarray(f['delay']).shape[1]
        fr = np.float64(floor_s) * np.float64(int(f['rate_in']))
        floor_f = fr * fr
        for c in range(MAX_CH):
            out[s, c] = (0.0, floor_f, 0.0, 0.0)
            if C < 2 or c >= C or c == f['ref']:
                continue
            n, sx, sxx = stats[s][c]
            if n >= min_frames:
                dn = np.float64(n)
                mean = np.float64(sx) / dn
                v = np.float64(sxx) / dn - mean * mean
                var = v if v > floor_f else floor_f
                out[s, c] = (mean, var, np.float64(1.0) / (np.float64(2.0) * var), -0.5 * math.log(TWO_PI * var))
            elif ok[s]:
                dead[spk_file[s]] |= 1 << c
    live = []
    for fi, f in enumerate(files):
        C = np.asarray(f['delay']).shape[1]
        live.append((((1 << C) - 1) & ~(1 << int(f['ref'])) & ~dead[fi]) if C > 1 else 0)
    return out, live


def _terms(f, clock, live, frame, mods):
    """[(x, model row)] of the channels that enter the sum at this frame, ascending."""
    T, C = np.asarray(f['delay']).shape
    k = step(frame - int(f['frame0']), clock, f)
    return [(int(f['delay'][k][c]), mods[c]) for c in range(C) if (live >> c) & 1 and f['reliable'][k][c]]


def score_f64(val, f, clock, live, frame, mods, weight):
    """One entry as the kernel computes it: float64, one rounding per operation."""
    val = np.float32(val)
    if not np.isfinite(val):
        return val
    ll = np.float64(0.0)
    for x, m in _terms(f, clock, live, frame, mods):
        d = np.float64(x) - m[0]
        t = d * d
        t = t * m[2]
        ll = ll + (m[3] - t)
    return np.float32(np.float64(val) + np.float64(weight) * ll)


def round_f32(v):
    """An mpmath value rounded once to float32 (to nearest; an exact tie, which these values never are, would go
    to the candidate found first)."""
    from mpmath import mpf
    c = np.float32(float(v))
    best = c
    for cand in (np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))):
        if np.isfinite(cand) and abs(mpf(float(cand)) - v) < abs(mpf(float(best)) - v):
            best = cand
    return best


def score_exact(val, f, clock, live, frame, mods, weight):
    """The same entry from the model's stored doubles in 50-digit arithmetic, rounded once to float32."""
    from mpmath import mp, mpf
    mp.dps = 50
    val = np.float32(val)
    if not np.isfinite(val):
        return val
    ll = mpf(0)
    for x, m in _terms(f, clock, live, frame, mods):
        d = mpf(x) - mpf(float(m[0]))
        ll += mpf(float(m[3])) - d * d * mpf(float(m[2]))
    return round_f32(mpf(float(val)) + mpf(float(weight)) * ll)


def ulps(a, b):
    """The distance of two finite float32 in units in the last place (through the ordered integer view)."""
    def key(x):
        i = int(np.float32(x).view(np.int32))
        return i if i >= 0 else -(i & 0x7fffffff)
    return abs(key(a) - key(b))
