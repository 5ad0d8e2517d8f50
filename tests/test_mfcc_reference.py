"""The front-end's kernels (k_mfcc_static, k_mfcc_post through spkd_mfcc_batch) against the float64
restatement oracle/mfcc_numpy.py at every border, parameter and bin -- with ONE comparator, whose
bound comes from the reference side alone and which the same inputs show to reject planted faults.

The comparator (tests/mfcc_compare.py: `ratios`, `column_bound`) works in STAGE SPACE: mean 0,
scale 1, transform I, so the 39 columns are the mean-subtracted statics, the deltas and the
delta-deltas themselves (the device then writes its stage values unchanged: a product with 1 and a
sum with zeros are exact).  The bound is per column, MARGIN times the largest distance over the
frames of an input (the files of one call) between tests/mfcc_f32_numpy.py without a fault and
the restatement, with a floor of FLOOR_ULPS float32 ulps.  Nothing the device computes enters it,
and neither do frontend.py's table builders: the device is given their tables, the reference side
builds its own from the restatement.  MARGIN covers what the emulation does not model: the
device's logf / sqrtf / cos and contraction of a * a + b * b.

CPU tests: on every input the GPU tests use, the comparator accepts the fault-free float32
restatement and rejects each of the 13 planted faults on at least one input (the test prints
which, and by how much: hundreds to millions of times the bound).  Of the two changes of precision that are
no faults, twiddles formed in float32 stay inside the bound on the dense inputs; a mean summed in
float32 does not over 151 frames (the two tests say where and why).  The every-bin input is also
shown to have no (frame, bin) of near-zero magnitude.

GPU tests: the device through the same comparator on the border grid (both window widths, stage
space and the real scale / transform), the parameter grid, every one of the 257 bins through
selector tables, and the signals the older tests lack (piecewise constant, piecewise +-A, full
scale, digital silence).

MARGIN started at 4.  On an MI355X the device then lay at 0.72 of the bound on the border batch and
the parameter grid (statics; deltas 0.57, delta-deltas 0.55), at 0.21 under the real scale and
transform, at 0.45 - 0.66 on the constant / +-A / full-scale files (0.99 for +-A, 256-sample window),
and at 1.024 in ONE column of the 1 584 of the every-bin calls (a delta-delta over 24 frames); the
device differs from the emulation by its logf, one or two ulps of values near 10 - 30.  It needs 4.1.
Kept: 6 -- the next even step, not a measured need -- where every planted fault is still rejected at
hundreds of times the bound (the CPU test prints each).  Device error / bound at 6:
  border batch, stage space        statics 0.48, deltas 0.38, delta-deltas 0.37 (256: 0.41, 0.34, 0.34)
  border batch, scale + transform  0.14 (256: 0.13)
  parameter grid                   statics 0.48, deltas 0.40, delta-deltas 0.37
  every bin                        statics 0.39, deltas 0.63, delta-deltas 0.68 (256: 0.50, 0.57, 0.65)
  constant / +-A / full scale      0.30 / 0.33 / 0.39 (256: 0.30 / 0.66 / 0.44)
"""
import functools
import os
import re

import numpy as np
import pytest

import mfcc_f32_numpy as e32
from conftest import pkg
from helpers import ROOT
from mfcc_compare import MARGIN, accepted, blocks, column_bound, full_chain, ratios
from test_frontend import GOLD, _cfg_text, _signal

HOP, RATE = 128, 16000

DEFAULT = (75, 75, 2, 2, 1.0, 10.0)                 # cms_left, cms_right, delta widths, delta norms
BORDER_T = [1, 2, 3, 4, 5, 7, 8, 9, 75, 76, 77, 127, 128, 129, 131, 132, 133, 151, 152, 256, 257, 260]
SHORT = [130, 205, 300, 399]                        # samples: files shorter than one 400-sample window (1, 1, 2, 3 frames)
GRID_T = [1, 3, 5, 77, 129, 133, 260]               # the parameter grid's files, of the border batch
MEAN_WINDOWS = [(75, 75), (0, 0), (0, 40), (40, 0), (3, 200), (136, 136)]
DELTA_WIDTHS = [(1, 1), (1, 2), (2, 1), (2, 2)]
DELTA_NORMS = [(1.0, 10.0), (2.5, 0.5)]
BIN_CALLS = [[(12 * i + j) % e32.N_BINS for j in range(12)] for i in range(22)]     # 22 x 12 covers 0 .. 256
assert sorted(set(k for call in BIN_CALLS for k in call)) == list(range(257))


# ------------------------------------------------------------------ inputs
class Cfg:
    """What both restatements read of a feature configuration."""
    sample_rate, frame_rate, hop, n_cep, dim, pre_emph = RATE, RATE // HOP, HOP, 12, 39, 0.97

    def __init__(self, window, params=DEFAULT):
        self.window_width = window
        self.cms_left, self.cms_right = params[0], params[1]
        self.delta_width, self.delta_norm = [params[2], params[3]], [params[4], params[5]]


@functools.lru_cache(maxsize=None)
def border_files():
    """name -> int16 samples.  The border batch: T frames and a remainder that is no multiple of the
    hop, the files shorter than a window, empty files first, in the middle and last; full-scale noise
    and +-3 noise in turn (the level is what a leak across a border carries)."""
    rng = np.random.default_rng(20261019)
    lengths = [('empty0', 0)] + [('s%d' % n, n) for n in SHORT]
    for i, T in enumerate(BORDER_T):
        lengths.append(('T%d' % T, T * HOP + 1 + (37 * i + 11) % (HOP - 1)))
        if i == len(BORDER_T) // 2:
            lengths.append(('empty1', 0))
    lengths.append(('empty2', 0))
    assert all(n < 400 for n in SHORT) and all(n % HOP for _, n in lengths if n)
    return {name: (rng.integers(-32768, 32768, n) if i % 2 else rng.integers(-3, 4, n)).astype(np.int16)
            for i, (name, n) in enumerate(lengths)}


def _levels(rng, n_frames, values):
    """A level per sample: stretches of 1 .. 6 frames, each at one of `values` -- some windows see
    several levels, some lie inside one stretch, and the mean over a window does not cancel them."""
    out = []
    while len(out) < n_frames:
        out += [rng.choice(values)] * int(rng.integers(1, 7))
    return np.repeat(np.array(out[:n_frames], dtype=np.int64), HOP)


@functools.lru_cache(maxsize=None)
def special_files():
    rng = np.random.default_rng(20261020)
    T = 40
    const = _levels(rng, T, [900, 4000, 12000, 30000, -7000])
    sign = np.where(np.arange(T * HOP) % 2 == 0, 1, -1)
    nyquist = _levels(rng, T, [500, 3000, 9000, 16000]) * sign
    full = np.where(rng.random(T * HOP + 77) < 0.5, 32767, -32768)
    full[:HOP] = -32768
    full[-HOP:] = 32767
    return {'constant': np.concatenate([const, const[-1:].repeat(19)]).astype(np.int16),
            'nyquist': np.concatenate([nyquist, np.zeros(5, dtype=np.int64)]).astype(np.int16),
            'full_scale': full.astype(np.int16),
            'silence': np.zeros(T * HOP + 100, dtype=np.int16),
            'every_bin': _every_bin_signal()}


def _every_bin_signal():
    """24 frames whose every window holds one dominant impulse (so that no bin of it is near zero:
    three impulses of a window weigh 1, 0.35 and 0.35 at the most) over dense noise of a hundredth
    of its height (so that every sample, and with it every twiddle, moves every bin).  That is the
    signal AFTER pre-emphasis; the samples are its running sum x[n] = y[n] + 0.97 x[n-1]."""
    rng = np.random.default_rng(23)
    n = 24 * HOP + 57
    y = 120.0 * rng.standard_normal(n)
    y[5::HOP] += 12000.0 * rng.uniform(0.85, 1.15, len(y[5::HOP]))
    y[:5] = 0.0
    x, acc = np.zeros(n), 0.0
    for i in range(n):
        acc = y[i] + 0.97 * acc
        x[i] = acc
    assert np.abs(x).max() < 32767
    return np.round(x).astype(np.int16)


def pcm_of(name):
    return special_files()[name] if name in special_files() else border_files()[name]


def selector_tables(bins):
    """A filterbank with one weight per row and a DCT that selects rows: column c of the statics is
    log |X[bins[c]]|."""
    melfb = np.zeros((e32.N_MEL, e32.N_BINS), dtype=np.float32)
    dct = np.zeros((12, e32.N_MEL), dtype=np.float32)
    for c, k in enumerate(bins):
        melfb[c, k] = 1.0
        dct[c, c] = 1.0
    return melfb, dct


def tables(call):
    """The reference side's tables.  call None: the restatement's own mel filterbank and DCT, rounded to
    float32 as a device table is (frontend.py's builders are the device's side: `device`); else the
    selector tables of BIN_CALLS[call]."""
    if call is None:
        from oracle import mfcc_numpy as m
        return m.mel_filterbank(RATE).astype(np.float32), m.dct_matrix(12).astype(np.float32)
    return selector_tables(BIN_CALLS[call])


def device_tables(call):
    """What the device is given: the front-end's own tables, or the selector tables."""
    if call is None:
        fe = pkg('frontend')
        return fe.mel_filterbank(RATE), fe.dct_matrix(12)
    return selector_tables(BIN_CALLS[call])


class Input:
    """One device call: files, window width, parameters, tables."""

    def __init__(self, name, files, window, params=DEFAULT, call=None):
        self.name, self.files, self.window, self.params, self.call = name, tuple(files), window, tuple(params), call
        self.cfg = Cfg(window, params)


def border_inputs():
    return [Input('border-%d' % w, border_files(), w) for w in (400, 256)]


def grid_inputs(mean_windows=MEAN_WINDOWS):
    files = ['empty0'] + ['T%d' % T for T in GRID_T] + ['s300']
    return [Input('grid-%d,%d-%d,%d-%g,%g' % (lr + dw + dn), files, 400, lr + dw + dn)
            for lr in mean_windows for dw in DELTA_WIDTHS for dn in DELTA_NORMS]


def bin_inputs(window):
    return [Input('bins-%d-%d' % (window, i), ['every_bin'], window, call=i) for i in range(len(BIN_CALLS))]


def special_inputs():
    return [Input('%s-%d' % (s, w), [s], w) for s in ('constant', 'nyquist', 'full_scale', 'silence') for w in (400, 256)]


def all_inputs():
    """Every input of the GPU tests; the small ones first."""
    return special_inputs() + bin_inputs(400) + bin_inputs(256) + grid_inputs() + border_inputs()


# ------------------------------------------------------------------ the two restatements, computed once
@functools.lru_cache(maxsize=None)
def _mag32(name, window, fault, variant):
    if fault == 'bin_255_step':                      # one bin moves: the others are the fault-free ones
        mag = _mag32(name, window, None, variant).copy()
        mag[:, 255] = e32.magnitudes(pcm_of(name), Cfg(window), fault, variant, bins=[255])[:, 255]
        return mag
    return e32.magnitudes(pcm_of(name), Cfg(window), fault, variant)


def stage32(inp, fault=None, variant=None):
    """The float32 restatement of an input, float32 [sum T, 39] (files in order)."""
    melfb, dct = tables(inp.call)
    out = []
    for name in inp.files:
        mag = _mag32(name, inp.window, fault if fault in e32.DFT_FAULTS else None,
                     variant if variant == 'twiddle_f32' else None)
        stat = e32.statics(mag, melfb, dct, fault if fault in e32.POWER_FAULTS else None)
        out.append(e32.post(stat, inp.cfg, fault if fault in e32.POST_FAULTS else None, variant))
    return np.concatenate(out)


def stage64(inp):
    """The float64 restatement of an input, float64 [sum T, 39]."""
    from oracle import mfcc_numpy as m
    melfb, dct = (None, None) if inp.call is None else tables(inp.call)       # None: its own float64 tables
    return np.concatenate([m.stage_features(pcm_of(name), inp.cfg, melfb, dct) for name in inp.files])


_REF = {}


def reference(inp):
    """(f64 [sum T, 39], bound [39]) of an input: computed once, shared, read-only."""
    key = (inp.files, inp.window, inp.params, inp.call)
    if key not in _REF:
        want = stage64(inp)
        bound = column_bound(stage32(inp), want)
        want.setflags(write=False)
        bound.setflags(write=False)
        _REF[key] = (want, bound)
    return _REF[key]


# ------------------------------------------------------------------ CPU: the comparator on the restatements
def test_inputs_hold_the_borders_levels_and_signals_they_claim():
    files = border_files()
    names = list(files)
    assert [len(files['T%d' % T]) // HOP for T in BORDER_T] == BORDER_T
    assert [len(files['s%d' % n]) // HOP for n in SHORT] == [1, 1, 2, 3]
    assert len(files[names[0]]) == len(files[names[-1]]) == len(files['empty1']) == 0
    assert 0 < names.index('empty1') < len(names) - 1
    loud = [int(np.abs(files[n].astype(np.int64)).max()) for n in names if len(files[n])]
    assert min(loud) <= 3 and max(loud) > 32000
    sp = special_files()
    assert sp['full_scale'].max() == 32767 and sp['full_scale'].min() == -32768 and not sp['silence'].any()
    assert len(set(np.abs(sp['nyquist'][:40 * HOP].astype(np.int64)))) > 2
    assert np.all(sp['nyquist'][:40 * HOP:2] > 0) and np.all(sp['nyquist'][1:40 * HOP:2] < 0)
    assert len(sp['every_bin']) // HOP == 24
    assert len(grid_inputs()) == 48 and len(bin_inputs(400)) == 22


def test_default_tables_leave_the_restatement_as_it_was():
    """static_features / features with the two tables left out are the former code bit for bit."""
    from oracle import mfcc_numpy as m
    cfg = pkg('feaconfig').FeatureConfig(_cfg_text(GOLD))
    pcm = _signal(0.9, seed=5)
    s = m.static_features(pcm, cfg)
    x = np.asarray(pcm, dtype=np.float64)
    idx = np.arange(len(x) // 128)[:, None] * 128 - 200 + np.arange(400)[None, :]
    y = (x[np.clip(idx, 0, len(x) - 1)] - cfg.pre_emph * x[np.clip(idx - 1, 0, len(x) - 1)]) * np.hamming(400)[None, :]
    mag = np.abs(np.fft.rfft(y, n=512, axis=1))
    cep = np.log(np.maximum(mag @ m.mel_filterbank(16000).T, 1e-10)) @ m.dct_matrix(12).T
    power = np.log(np.maximum((mag ** 2).sum(axis=1), 1e-10))
    assert np.array_equal(s, np.concatenate([cep, power[:, None]], axis=1))
    assert np.array_equal(s, m.static_features(pcm, cfg, m.mel_filterbank(16000), m.dct_matrix(12)))
    # the former post stage, restated line for line
    T = s.shape[0]
    c = np.concatenate([np.zeros((1, s.shape[1])), np.cumsum(s, axis=0)])
    lo = np.maximum(np.arange(T) - cfg.cms_left, 0)
    hi = np.minimum(np.arange(T) + cfg.cms_right + 1, T)
    cms = s - (c[hi] - c[lo]) / (hi - lo)[:, None]

    def delta(x, width, norm):
        out, t = np.zeros_like(x), np.arange(T)
        for k in range(1, width + 1):
            out += k * (x[np.minimum(t + k, T - 1)] - x[np.maximum(t - k, 0)])
        return out / norm

    d1 = delta(cms, cfg.delta_width[0], cfg.delta_norm[0])
    d2 = delta(d1, cfg.delta_width[1], cfg.delta_norm[1])
    stage = np.concatenate([cms, d1, d2], axis=1)
    assert np.array_equal(m.stage_features(pcm, cfg), stage)
    z = (stage - cfg.mean[None, :]) * cfg.scale[None, :]
    assert np.array_equal(m.features(pcm, cfg), (z @ cfg.transform.astype(np.float64).T).astype(np.float32))
    assert m.features(pcm[:100], cfg).shape == (0, 39) and m.features(pcm[:100], cfg).dtype == np.float32


def test_the_front_end_builds_the_restatement_s_tables():
    """frontend.py's table builders, whose tables extract / extract_batch give the device, against the
    restatement's: the same numbers, rounded to float32 -- at the rate and the cepstrum count in use.
    (The device tests hold them apart as well: `device_tables` against `tables`.)"""
    from oracle import mfcc_numpy as m
    fe = pkg('frontend')
    cfg = pkg('feaconfig').FeatureConfig(_cfg_text(GOLD))
    assert (cfg.sample_rate, cfg.n_cep) == (RATE, 12)
    melfb, dct = fe.mel_filterbank(cfg.sample_rate), fe.dct_matrix(cfg.n_cep)
    assert melfb.dtype == dct.dtype == np.float32
    assert np.array_equal(melfb, m.mel_filterbank(cfg.sample_rate).astype(np.float32))
    assert np.array_equal(dct, m.dct_matrix(cfg.n_cep).astype(np.float32))
    assert (fe.N_FFT, fe.N_MEL) == (m.N_FFT, m.N_MEL) == (512, e32.N_MEL)


def test_the_comparator_accepts_the_float32_restatement_on_every_input():
    for inp in all_inputs():
        want, bound = reference(inp)
        assert accepted(ratios(stage32(inp), want, bound)), inp.name
        assert np.all(bound > 0) or inp.name.startswith('silence')
    # (0, 0): every frame is its own mean
    for inp in grid_inputs([(0, 0)]):
        assert not stage32(inp)[:, :13].any()
        assert np.abs(reference(inp)[0][:, :13]).max() < 1e-10        # the restatement's difference of two running sums


def test_the_every_bin_input_has_no_near_zero_magnitude():
    """log |X[k]| is as well determined as |X[k]| is large against sum |y[n]|, the size of the terms
    that cancel in it: a serial float32 chain of WIN fmaf and rounded twiddles leaves at most
    (WIN + 2) u sum|y| of error in X, u = 2^-24, so (WIN + 2) u sum|y| / |X| in the logarithm and twice
    that after the mean is taken off.  The input keeps sum|y| / |X| below 128 at EVERY (frame, bin);
    and in every element of all 44 calls the float32 restatement lies inside the bound, which in turn
    lies inside MARGIN times that figure -- no element is skipped, no bin has a bound to hide in."""
    for window in (400, 256):
        y = e32.windowed(pcm_of('every_bin'), Cfg(window)).astype(np.float64)
        mag = np.abs(np.fft.rfft(y, n=512, axis=1))
        cond = np.abs(y).sum(axis=1)[:, None] / mag
        print('window %d: sum|y| / |X| at most %.1f (frame %d, bin %d)' % (
            (window, cond.max()) + np.unravel_index(cond.argmax(), cond.shape)))
        assert mag.shape == (24, 257) and cond.max() < 128
        worst = 0.0
        for inp in bin_inputs(window):
            want, bound = reference(inp)
            diff = np.abs(stage32(inp).astype(np.float64) - want)
            assert np.all(diff <= bound[None, :]), inp.name                    # every element, not a summary
            worst = max(worst, float(bound[:12].max()))
        print('window %d: largest bound of a bin column %.3g' % (window, worst))
        assert worst < MARGIN * 2 * (window + 2) * 2.0 ** -24 * 128


@pytest.mark.parametrize('fault', sorted(e32.FAULTS))
def test_the_comparator_rejects_each_planted_fault(fault):
    """On the GPU tests' own inputs, through the GPU tests' own comparator and bound."""
    inputs = all_inputs()
    if fault in ('twiddle_slot_160', 'bin_255_step'):
        # the two DFT faults must (also) fall to the every-bin calls, and there in a column that holds
        # a bin (the power column 12 and its deltas see every bin in every call)
        own = np.array([c % 13 != 12 for c in range(39)])
        for window in (400, 256):
            calls = bin_inputs(window)
            r = [ratios(stage32(inp, fault), *reference(inp)) for inp in calls]
            hit = [inp.name for inp, ri in zip(calls, r) if ri[own].max() > 1.0]
            print('%s: every-bin calls of window %d that reject it in the column of a bin: %d of 22, at up to %.3g times the bound' % (
                fault, window, len(hit), max(ri[own].max() for ri in r)))
            assert hit, window
            if fault == 'bin_255_step':
                call = [i for i, b in enumerate(BIN_CALLS) if 255 in b][0]
                assert r[call][BIN_CALLS[call].index(255)] > 1.0 and len(hit) == 1
    for inp in inputs:
        want, bound = reference(inp)
        r = ratios(stage32(inp, fault), want, bound)
        if not accepted(r):
            print('%s (%s): rejected by %s, column %d at %.3g times its bound' % (
                fault, e32.FAULTS[fault], inp.name, int(r.argmax()), float(r.max())))
            return
    raise AssertionError('%s: no input rejects it -- the inputs are too kind' % fault)


def _variant_ratios(variant, inputs):
    out = {}
    for inp in inputs:
        r = ratios(stage32(inp, variant=variant), *reference(inp))
        key = inp.name if not inp.name.startswith(('grid', 'bins')) else inp.name.split('-')[0]
        out[key] = max(out.get(key, 0.0), float(r.max()))
    return out


def test_float32_twiddles_alone_stay_inside_the_bound():
    """Twiddles whose angle, cos and sin are formed in float32 are a change of precision, no fault:
    on the border batch, the parameter grid and the every-bin calls -- dense spectra, where a
    twiddle's error meets 400 independent samples -- the comparator need not catch it and does not
    (0.94 of the bound at MARGIN 4, 0.63 at 6).
    On the line spectra it is told apart (asserted for the constant file, measured for the rest) (at MARGIN 6: constant 6.6 times
    the bound, +-A 1.2), because 250 of their 257 bins hold leakage that cancels to a thousandth of
    its terms and the twiddles' last bits decide it; and so it is in the power column of the
    constant-modulus full-scale file, 256-sample window (2.8), where rounding noise averages out
    over the bins and a twiddle's error, the same in every frame, does not."""
    dense = _variant_ratios('twiddle_f32', border_inputs() + grid_inputs() + bin_inputs(400) + bin_inputs(256))
    print('twiddle_f32, asserted:', {k: round(v, 2) for k, v in dense.items()})
    lines = _variant_ratios('twiddle_f32', special_inputs())
    print('twiddle_f32, line spectra and constant modulus:', {k: round(v, 2) for k, v in lines.items()})
    assert max(dense.values()) <= 1.0, dense
    assert lines['constant-400'] > 1.0 and lines['constant-256'] > 1.0          # told apart where the docstring says so


def test_a_float32_mean_is_inside_the_bound_for_short_windows_only():
    """A mean summed in float32 was expected to lie below the bound like
    the twiddles.  As the kernel would do it -- one serial float32 sum per frame -- it does where
    the window holds few frames (the every-bin calls, 24 frames: asserted).  Over the 151 frames of
    the border batch it does not: the running sum of values near 30 reaches 4 000, each of its 150
    roundings is up to 1.2e-4, and the mean comes out 1e-5 off where the chain's own noise in that
    column is 1e-6 -- 2.5 times the bound at MARGIN 6 (3.7 at 4; numpy's pairwise sum: 1.1 and 1.6).
    And on silence it turns the exact 0 into 6e-7.  So the comparator tells a float32 mean from the
    kernel's float64 one, which is what the float64 sum is there for; that much is asserted too."""
    short = _variant_ratios('mean_f32', bin_inputs(400) + bin_inputs(256))
    long = _variant_ratios('mean_f32', border_inputs())
    print('mean_f32, 24 frames:', {k: round(v, 2) for k, v in short.items()}, '151-frame windows:',
          {k: round(v, 2) for k, v in long.items()})
    assert max(short.values()) <= 1.0, short
    assert min(long.values()) > 1.0, long
    for inp in special_inputs():
        if inp.files == ('silence',):
            assert stage32(inp, variant='mean_f32').any() and not stage32(inp).any()
            assert not accepted(ratios(stage32(inp, variant='mean_f32'), *reference(inp)))


def test_header_kernels_and_binding_state_one_mean_window_limit():
    hipabi = pkg('hipabi')
    code = open(os.path.join(ROOT, 'include', 'spkd.h')).read()
    kern = open(os.path.join(ROOT, 'speaker-diarization_amd', 'csrc', 'spkd_mfcc.hpp')).read()
    head = {n: int(re.search(r'#define SPKD_MFCC_%s (\d+)' % n, code).group(1))
            for n in ('POST_TILE', 'POST_HALO', 'POST_LDS', 'CMS_MAX')}
    assert head['POST_TILE'] == hipabi.MFCC_POST_TILE == int(re.search(r'constexpr int MP_FR = (\d+);', kern).group(1))
    assert head['POST_HALO'] == hipabi.MFCC_POST_HALO == int(re.search(r'constexpr int MP_HALO = (\d+);', kern).group(1))
    assert head['POST_LDS'] == hipabi.MFCC_POST_LDS == 60 * 1024 and 'MP_LDS_MAX = 60 * 1024' in kern
    assert head['CMS_MAX'] == hipabi.MFCC_CMS_MAX == cms_limit()
    assert e32.POST_TILE == hipabi.MFCC_POST_TILE


def post_lds_bytes(cms):
    """k_mfcc_post's LDS for a mean window of left + right = cms, from the exported tile constants
    (the formula of mp_lds_floats and of include/spkd.h §6)."""
    hipabi = pkg('hipabi')
    span = hipabi.MFCC_POST_TILE + 2 * hipabi.MFCC_POST_HALO
    return 4 * (13 * (3 * span + cms) + 39 * hipabi.MFCC_POST_TILE + 39 * 39)


def cms_limit():
    """The widest mean window the formula admits."""
    hipabi = pkg('hipabi')
    cms = 0
    while post_lds_bytes(cms + 1) <= hipabi.MFCC_POST_LDS:
        cms += 1
    return cms


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def ctx():
    c = pkg('hipabi').Context(0)
    yield c
    c.close()


IDENTITY = (np.zeros(39, dtype=np.float32), np.ones(39, dtype=np.float32), np.eye(39, dtype=np.float32))


def mfcc_params(inp):
    hipabi = pkg('hipabi')
    p = inp.params
    return hipabi.MfccParams(RATE, RATE // HOP, inp.window, 512, e32.N_MEL, 12, p[0], p[1], (hipabi.C.c_int32 * 2)(p[2], p[3]),
                             0.97, (hipabi.C.c_float * 2)(p[4], p[5]))


def device(ctx, inp, norm=IDENTITY):
    """One spkd_mfcc_batch call with MfccParams given directly -> float32 [sum T, 39]."""
    fe = pkg('frontend')
    pcms = [pcm_of(name) for name in inp.files]
    d_pcm, sample_off = fe.upload_batch(ctx, pcms)
    total = sum(len(p) // HOP for p in pcms)
    out = np.full((total + 1, 39), np.nan, dtype=np.float32)
    d_out = ctx.dev_scratch('test_mfcc_reference_out', out.nbytes)
    ctx.h2d(d_out, out)
    frame_off = ctx.mfcc_batch(d_pcm, sample_off, mfcc_params(inp), *device_tables(inp.call), *norm, d_out)
    ctx.d2h(out, d_out)
    assert list(np.diff(frame_off)) == [len(p) // HOP for p in pcms] and np.all(np.isnan(out[total]))
    return out[:total]


def check(ctx, inp):
    """The device on an input through the comparator; prints the ratio of each column block."""
    want, bound = reference(inp)
    r = ratios(device(ctx, inp), want, bound)
    print('%-28s device error / bound: statics %.3f, deltas %.3f, delta-deltas %.3f' % ((inp.name,) + blocks(r)))
    assert accepted(r), (inp.name, int(r.argmax()), float(r.max()))
    return r


@pytest.mark.gpu
@pytest.mark.parametrize('window', [400, 256])
def test_device_border_grid_in_stage_space(ctx, window):
    inp = [i for i in border_inputs() if i.window == window][0]
    want, bound = reference(inp)
    got = device(ctx, inp)
    r = ratios(got, want, bound)
    print('%s: device error / bound: statics %.3f, deltas %.3f, delta-deltas %.3f' % ((inp.name,) + blocks(r)))
    # per file too, so that a failure names the length
    at = np.concatenate([[0], np.cumsum([len(pcm_of(n)) // HOP for n in inp.files])])
    for i, name in enumerate(inp.files):
        if at[i + 1] > at[i]:
            rf = ratios(got[at[i]:at[i + 1]], want[at[i]:at[i + 1]], bound)
            assert accepted(rf), (name, int(rf.argmax()), float(rf.max()))
    assert accepted(r)
    one = got[at[inp.files.index('T1')]]
    assert not one[13:].any()                           # a single frame: both delta stages are exactly 0


@pytest.mark.gpu
@pytest.mark.parametrize('window', [400, 256])
def test_device_border_grid_under_the_real_scale_and_transform(ctx, window):
    cfg = pkg('feaconfig').FeatureConfig(_cfg_text(GOLD))
    inp = [i for i in border_inputs() if i.window == window][0]
    assert inp.params == (cfg.cms_left, cfg.cms_right) + tuple(cfg.delta_width) + tuple(cfg.delta_norm)
    want, bound = full_chain(*reference(inp), cfg.mean, cfg.scale, cfg.transform)
    r = ratios(device(ctx, inp, (cfg.mean, cfg.scale, cfg.transform)), want, bound)
    print('%s, real scale and transform: device error / bound at most %.3f (column %d)' % (inp.name, r.max(), r.argmax()))
    assert accepted(r)


@pytest.mark.gpu
@pytest.mark.parametrize('mean_window', MEAN_WINDOWS, ids=lambda lr: '%d-%d' % lr)
def test_device_parameter_grid(ctx, mean_window):
    worst = np.zeros(39)
    for inp in grid_inputs([mean_window]):
        got = device(ctx, inp)
        want, bound = reference(inp)
        r = ratios(got, want, bound)
        worst = np.maximum(worst, r)
        assert accepted(r), (inp.name, int(r.argmax()), float(r.max()))
        if mean_window == (0, 0):
            assert not got[:, :13].any()                # every frame is its own mean: exact zeros
    print('mean window %r, 8 delta settings: device error / bound: statics %.3f, deltas %.3f, delta-deltas %.3f' % (
        (mean_window,) + blocks(worst)))


@pytest.mark.gpu
@pytest.mark.parametrize('window', [400, 256])
def test_device_every_bin(ctx, window):
    """log |X[k]| of each of the 257 bins in a column of its own, 12 bins a call."""
    worst, seen = np.zeros(39), set()
    for inp in bin_inputs(window):
        want, bound = reference(inp)
        got = device(ctx, inp)
        r = ratios(got, want, bound)
        inside = bool(np.all(np.abs(got.astype(np.float64) - want) <= bound[None, :]))         # every element
        assert inside, (inp.name, BIN_CALLS[inp.call], int(r.argmax()), float(r.max()))
        assert accepted(r), (inp.name, BIN_CALLS[inp.call], int(r.argmax()), float(r.max()))
        worst = np.maximum(worst, r)
        seen.update(BIN_CALLS[inp.call])
    assert seen == set(range(257))
    print('every bin, window %d: device error / bound: statics %.3f, deltas %.3f, delta-deltas %.3f' % (
        (window,) + blocks(worst)))


@pytest.mark.gpu
@pytest.mark.parametrize('signal', ['constant', 'nyquist', 'full_scale'])
def test_device_signals_the_other_tests_lack(ctx, signal):
    for inp in special_inputs():
        if inp.files == (signal,):
            check(ctx, inp)


@pytest.mark.gpu
def test_device_digital_silence_is_exact(ctx):
    """Silence ends at both 1e-10 floors: every static row is the same float, the float64 mean over
    identical values is that value, so the stage-space output is exactly 0; under a general mean,
    scale and transform every frame is the same 39 floats."""
    cfg = pkg('feaconfig').FeatureConfig(_cfg_text(GOLD))
    rng = np.random.default_rng(7)
    mean = rng.standard_normal(39).astype(np.float32)
    for inp in special_inputs():
        if inp.files != ('silence',):
            continue
        got = device(ctx, inp)
        assert got.shape == (40, 39) and not got.any()
        check(ctx, inp)
        got = device(ctx, inp, (mean, cfg.scale, cfg.transform))
        assert np.all(got.view(np.uint32) == got[0].view(np.uint32)[None, :]) and got.any()
        want, _ = full_chain(np.zeros((1, 39)), np.zeros(39), mean, cfg.scale, cfg.transform)
        assert np.allclose(got[0], want[0], rtol=1e-5, atol=1e-5)


@pytest.mark.gpu
def test_device_mean_window_limit_both_edges(ctx):
    """left + right = the limit of the LDS formula runs and matches the restatement; one more is
    SPKD_EINVAL with the LDS message.  Both numbers come from the exported tile constants."""
    hipabi = pkg('hipabi')
    limit = cms_limit()
    assert post_lds_bytes(limit) <= hipabi.MFCC_POST_LDS < post_lds_bytes(limit + 1)
    files = ['T%d' % T for T in (3, 129, 260)]
    for left in (limit // 2, 0, limit):
        check(ctx, Input('limit-%d,%d' % (left, limit - left), files, 400, (left, limit - left) + DEFAULT[2:]))
    for left in (limit // 2, 0, limit + 1):
        with pytest.raises(hipabi.SpkdError, match='too wide for the LDS tile') as err:
            device(ctx, Input('over', files, 400, (left, limit + 1 - left) + DEFAULT[2:]))
        assert err.value.status == hipabi.SPKD_EINVAL
    check(ctx, Input('after-refusal', files, 400))        # the context is usable afterwards
