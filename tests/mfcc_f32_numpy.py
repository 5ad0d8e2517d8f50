"""The front-end's chain in the kernels' own arithmetic (numpy float32) -- TEST INFRASTRUCTURE ONLY.

The same chain as oracle/mfcc_numpy.py (the float64 restatement, which alone defines what the
kernels should produce), evaluated the way k_mfcc_static / k_mfcc_post evaluate it:

  window   (x[n] - float32(pre_emph) x[n-1]) * hamming[n] formed in float64, rounded to float32
  DFT      per (frame, bin k) ONE serial chain over n = 0 .. WIN-1 of re = fmaf(y, cos, re),
           im = fmaf(-y, sin, im); the twiddle of phase (k n) mod 512 is cos / sin in float64,
           rounded.  fmaf is the exact product added in float64 and rounded once more (a float32
           product is exact in float64; the second rounding differs from a fused one in about one
           case in 2^29).  Vectorised over frames and bins: a WIN-step loop over [T, 257] arrays.
  power    thread k holds mag[k]^2 (thread 0 also bin 256), a 64-lane butterfly sum per wave, the
           four wave sums added in order; log of it, floor 1e-10
  mel/DCT  serial fmaf chains over the 257 bins / the 21 bands, float32 log
  post     the mean in float64 over the frames that exist, the result rounded; both delta stages in
           float32, divided by the norm

It serves two ends.  (a) It measures how far float32 arithmetic of this shape lies from the
float64 restatement on an input: tests/test_mfcc_reference.py builds every bound from that
difference.  (b) `fault=` plants ONE semantic fault (FAULTS), `variant=` one change of precision
that is no fault (VARIANTS): the tests show that their comparator rejects the first and accepts
the second.
"""
import numpy as np

f32, f64 = np.float32, np.float64
N_FFT, N_BINS, N_MEL = 512, 257, 21
POST_TILE = 128                        # frames per workgroup of k_mfcc_post (the two tile faults need it)
FLOOR = f32(1e-10)

FAULTS = {
    'power_without_bin_256': 'bin 256 left out of the power sum',
    'power_without_bin_0': 'bin 0 left out of the power sum',
    'twiddle_slot_160': 'phase 160 (a multiple of 32) reads the twiddle of phase 159',
    'bin_255_step': 'bin 255 advances its phase by 254 a sample',
    'hamming_over_win': 'the Hamming denominator is WIN, not WIN - 1',
    'centre_late': 'every frame is centred one sample late',
    'zero_outside': 'samples outside the file are 0, not the border sample',
    'zero_predecessor': 'the predecessor of sample 0 is 0, not sample 0',
    'mean_short_right': 'the mean window ends one frame early',
    'mean_full_divisor': 'the mean divides by left + right + 1 where the window is clipped',
    'delta_clamp_tile': 'delta indices clamp to the 128-frame tile, not to the file',
    'halo_row_missing': 'the last halo row behind a tile is missing from its first delta stage',
    'cms_swapped': 'cms_left and cms_right swapped',
}
VARIANTS = {
    'twiddle_f32': 'the twiddle angle and its cos / sin evaluated in float32',
    'mean_f32': 'the mean summed in float32',
}
DFT_FAULTS = ('twiddle_slot_160', 'bin_255_step', 'hamming_over_win', 'centre_late', 'zero_outside', 'zero_predecessor')
POWER_FAULTS = ('power_without_bin_256', 'power_without_bin_0')
POST_FAULTS = ('mean_short_right', 'mean_full_divisor', 'delta_clamp_tile', 'halo_row_missing', 'cms_swapped')
assert sorted(DFT_FAULTS + POWER_FAULTS + POST_FAULTS) == sorted(FAULTS)


def _fma(a, b, c):
    """fmaf(a, b, c) of float32 arrays."""
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def windowed(pcm, cfg, fault=None):
    """int16 samples -> the pre-emphasised, windowed frames, float32 [T, WIN]."""
    x = np.asarray(pcm, dtype=f64)
    W = cfg.window_width
    T = len(x) // cfg.hop
    if T == 0:
        return np.zeros((0, W), dtype=f32)
    idx = np.arange(T)[:, None] * cfg.hop - W // 2 + np.arange(W)[None, :] + (1 if fault == 'centre_late' else 0)
    take = lambda i: x[np.clip(i, 0, len(x) - 1)]
    cur, prev = take(idx), take(idx - 1)
    if fault == 'zero_outside':
        cur = np.where((idx >= 0) & (idx < len(x)), cur, 0.0)
        prev = np.where((idx - 1 >= 0) & (idx - 1 < len(x)), prev, 0.0)
    if fault == 'zero_predecessor':
        prev = np.where(idx == 0, 0.0, prev)
    ham = 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(W) / (W if fault == 'hamming_over_win' else W - 1))
    return ((cur - float(f32(cfg.pre_emph)) * prev) * ham[None, :]).astype(f32)


def twiddles(variant=None):
    """(cos, sin) of 2 pi p / 512, p = 0 .. 511, float32."""
    if variant == 'twiddle_f32':
        a = f32(2.0 * np.pi) * np.arange(N_FFT, dtype=f32) / f32(N_FFT)
        return np.cos(a), np.sin(a)
    a = 2.0 * np.pi * np.arange(N_FFT) / N_FFT
    return np.cos(a).astype(f32), np.sin(a).astype(f32)


def magnitudes(pcm, cfg, fault=None, variant=None, bins=None):
    """The magnitude spectrum, float32 [T, 257]: per (frame, bin) the serial fmaf chain.  bins: an
    index array restricts the work to those bins (the others come back 0)."""
    y = windowed(pcm, cfg, fault)
    T, W = y.shape
    k = np.arange(N_BINS) if bins is None else np.asarray(bins)
    step = np.where(k == 255, 254, k) if fault == 'bin_255_step' else k
    cos, sin = twiddles(variant)
    re = np.zeros((T, len(k)), dtype=f32)
    im = np.zeros((T, len(k)), dtype=f32)
    for n in range(W):
        ph = (step * n) % N_FFT
        if fault == 'twiddle_slot_160':
            ph = np.where(ph == 160, 159, ph)
        v = y[:, n:n + 1]
        re = _fma(v, cos[ph][None, :], re)
        im = _fma(-v, sin[ph][None, :], im)
    mag = np.zeros((T, N_BINS), dtype=f32)
    mag[:, k] = np.sqrt(re * re + im * im)
    return mag


def statics(mag, melfb, dct, fault=None):
    """float32 magnitudes [T, 257] and the two float32 tables -> the static rows, float32 [T, 13]."""
    mag = np.asarray(mag, dtype=f32)
    melfb = np.asarray(melfb, dtype=f32)
    dct = np.asarray(dct, dtype=f32)
    T = mag.shape[0]
    acc = np.zeros((T, melfb.shape[0]), dtype=f32)
    for b in range(N_BINS):
        acc = _fma(melfb[None, :, b], mag[:, b:b + 1], acc)
    lmel = np.log(np.maximum(acc, FLOOR))
    cep = np.zeros((T, dct.shape[0]), dtype=f32)
    for m in range(melfb.shape[0]):
        cep = _fma(dct[None, :, m], lmel[:, m:m + 1], cep)
    sq = mag * mag
    lanes = sq[:, :256].copy()
    if fault == 'power_without_bin_0':
        lanes[:, 0] = 0
    if fault != 'power_without_bin_256':
        lanes[:, 0] = _fma(mag[:, 256], mag[:, 256], lanes[:, 0])
    lanes = lanes.reshape(T, 4, 64)
    lane = np.arange(64)
    for s in (1, 2, 4, 8, 16, 32):
        lanes = lanes + lanes[:, :, lane ^ s]
    p = np.zeros(T, dtype=f32)
    for w in range(4):
        p = p + lanes[:, w, 0]
    return np.concatenate([cep, np.log(np.maximum(p, FLOOR))[:, None]], axis=1)


def _delta(x, width, norm, lo, hi):
    """One delta stage in float32; frame t clamps its neighbours to [lo[t], hi[t]]."""
    t = np.arange(x.shape[0])
    v = np.zeros_like(x)
    for k in range(1, width + 1):
        v = v + f32(k) * (x[np.minimum(t + k, hi)] - x[np.maximum(t - k, lo)])
    return v / f32(norm)


def post(stat, cfg, fault=None, variant=None):
    """float32 static rows [T, 13] -> the stage-space features, float32 [T, 39]: mean-subtracted
    statics, deltas, delta-deltas (what the kernel writes under mean 0, scale 1, transform I)."""
    stat = np.asarray(stat, dtype=f32)
    T = stat.shape[0]
    if T == 0:
        return np.zeros((0, 3 * stat.shape[1]), dtype=f32)
    left, right = (cfg.cms_right, cfg.cms_left) if fault == 'cms_swapped' else (cfg.cms_left, cfg.cms_right)
    t = np.arange(T)
    lo = np.maximum(t - left, 0)
    hi = np.minimum(t + right + 1, T)
    if fault == 'mean_short_right':
        hi = np.maximum(np.minimum(t + right, T), lo + 1)
    div = np.full(T, left + right + 1) if fault == 'mean_full_divisor' else hi - lo
    if variant == 'mean_f32':                        # a serial float32 sum per frame, as the kernel's loop would be
        s = np.zeros(stat.shape, dtype=f32)
        for q in range(-left, right + 1):
            inside = ((t + q >= lo) & (t + q < hi))[:, None]
            s = np.where(inside, s + stat[np.clip(t + q, 0, T - 1)], s)
        mean = (s / div[:, None].astype(f32)).astype(f64)
    else:                                            # float64 (a running sum, the kernel a serial one: both far below a float32 ulp)
        c = np.concatenate([np.zeros((1, stat.shape[1])), np.cumsum(stat, axis=0, dtype=f64)])
        mean = (c[hi] - c[lo]) / div[:, None]
    cms = (stat.astype(f64) - mean).astype(f32)
    if fault == 'delta_clamp_tile':
        first = t // POST_TILE * POST_TILE
        last = np.minimum(first + POST_TILE, T) - 1
    else:
        first, last = np.zeros(T, dtype=np.int64), np.full(T, T - 1)
    w1, w2 = cfg.delta_width
    n1, n2 = cfg.delta_norm
    d1 = _delta(cms, w1, n1, first, last)
    d2 = _delta(d1, w2, n2, first, last)
    if fault == 'halo_row_missing':
        # the tile [t0, t0 + 128) forms d1 of its halo frames t0 + 128, t0 + 129 from the cms rows up to
        # t0 + 131; without the last of them the term k = 2 of d1[t0 + 129] has no partner and drops out,
        # and with it d2 of the tile's last frame moves
        for e in range(POST_TILE - 1, T, POST_TILE):
            if e + 4 > T - 1 or w1 < 2 or w2 < 2:
                continue
            bad = (f32(1) * (cms[e + 3] - cms[e + 1])) / f32(n1)
            d2[e] = (f32(1) * (d1[e + 1] - d1[e - 1]) + f32(2) * (bad - d1[e - 2])) / f32(n2)
    return np.concatenate([cms, d1, d2], axis=1)


def stage_features(pcm, cfg, melfb, dct, fault=None, variant=None):
    """The whole chain in stage space, float32 [T, 39]."""
    assert fault is None or fault in FAULTS, fault
    assert variant is None or variant in VARIANTS, variant
    mag = magnitudes(pcm, cfg, fault if fault in DFT_FAULTS else None, variant)
    stat = statics(mag, melfb, dct, fault if fault in POWER_FAULTS else None)
    return post(stat, cfg, fault if fault in POST_FAULTS else None, variant)
