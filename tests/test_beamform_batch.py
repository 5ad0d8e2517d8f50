"""Delay-and-sum beamforming of a batch on the device (spkd_bf_gcc, spkd_bf_track, spkd_bf_sum,
frontend.beamform_geometry / beamform_batch / resample_batch(beamform=...),
pipeline.diarize_audio_batch(beamform=...), ./to16k.py --beamform) against the numpy restatement of
tests/beamform_numpy.py, which also holds the scenes S1 .. S5 and the coloured variant of S1.

What is compared how:
  the correlation   all elements of d_curve against the float64 restatement, within CURVE_BOUND: 16
                    times the largest difference measured on the MI355X over these very scenes
                    (profiles/beamform_accuracy.json, written by tools/beamform_accuracy.py); the factor
                    covers the error of a float32 transform moving with the data on so few scenes.  The
                    bound may not exceed 1e-4, 1/500 of the smallest decision gap the fixture guard
                    guarantees (0.05): a larger error means the transform's arithmetic is to be mended.
  the candidates    exactly, against the selection rule applied in numpy to the device's own curve;
  the delays        exactly, against the restatement's Viterbi run on the device's candidates, and on
                    hand-made tables for the ties and rules no audio can aim at;
  the sum           exactly (its numerator is an integer).
Every decision the scenes' tests rest on has a margin the guard test asserts on the CPU, so a scene that
disagrees on the GPU is not a near-tie.

All audio is 3 s or shorter, except one 19.5 s two-channel file: 77 steps, more than a wave has lanes."""
import ctypes as C
import functools
import json
import os
import re
import subprocess
import sys
import types
import wave

import numpy as np
import pytest

import beamform_numpy as B
from conftest import pkg
from helpers import ROOT
from test_generate_exp import _synthetic_mixtures, load_model, write_model
from test_mfcc_batch import _cfg, _talk

GUARD, GUARD_BYTE = 64, 0x5a
G16 = B.GEOM_16K
TRACK = dict(n_best=B.N_BEST, min_peak=B.MIN_PEAK, penalty=B.JUMP_PENALTY, cap=B.JUMP_CAP)
MAX_CURVE_BOUND = 1e-4
NEG = -np.inf


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@functools.lru_cache(maxsize=None)
def _scene(name):
    """A scene and its restatement with reference channel 0, computed once."""
    sc = B.scene(name)
    return sc, B.beamform(sc['x'], sc['geom'], ref=0)


@functools.lru_cache(maxsize=None)
def _long_file():
    """19.5 s, two channels: a voice and itself 37 samples later, each over a little noise of its own."""
    s = _talk(19.5, 114).astype(np.float64)
    rng = np.random.default_rng(5)
    x = np.stack([s, np.concatenate([np.zeros(37), s[:-37]])], axis=1) + 20.0 * rng.standard_normal((len(s), 2))
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _opts(**kw):
    return dict(pkg('pipeline').BEAMFORM, **kw)


# ------------------------------------------------------------------ not GPU
def test_entry_points_struct_defines_and_timers_are_declared_exported_and_mirrored():
    hipabi = pkg('hipabi')
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'spkd.h')).read(), flags=re.S)
    lib = hipabi.load_library()
    for name in ('spkd_bf_gcc', 'spkd_bf_track', 'spkd_bf_sum'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in hipabi.EXPORTS and hasattr(lib, name), name
        assert hasattr(hipabi.Context, name[len('spkd_'):]), name
    assert re.search(r'\{\s*int32_t hop, window, max_lag;\s*\}\s*spkd_bf_geom\s*;', code) and C.sizeof(hipabi.BfGeom) == 12
    for name, value in (('NFFT', 8192), ('NBEST', 4), ('MAX_HOP', 1 << 20)):
        assert int(re.search(r'#define SPKD_BF_%s (\d+)' % name, code).group(1)) == value == getattr(hipabi, 'BF_' + name)
    assert int(re.search(r'#define SPKD_ABI_VERSION (\d+)', code).group(1)) == 2
    names = [n for n, _ in sorted(hipabi.TIMERS.items(), key=lambda kv: kv[1])]
    enum = re.search(r'enum \{\s*SPKD_T_CALL = 0,(.*?)SPKD_N_TIMERS', code, flags=re.S).group(1)
    assert ['call'] + [n.strip()[len('SPKD_T_'):].lower() for n in enum.split(',') if n.strip()] == names
    at = names.index('resample')
    assert names[at - 3:at] == ['bf_gcc', 'bf_track', 'bf_sum'] and names[at + 1:at + 3] == ['frame_energy', 'energy_seeds']
    assert B.NFFT == hipabi.BF_NFFT and B.NBEST == hipabi.BF_NBEST
    bf = pkg('pipeline').BEAMFORM
    assert (bf['n_best'], bf['min_peak'], bf['jump_penalty'], bf['jump_cap']) == (B.N_BEST, B.MIN_PEAK, B.JUMP_PENALTY, B.JUMP_CAP)
    assert bf == dict(step_s=0.25, window_s=0.5, max_delay_s=0.01, n_best=4, min_peak=0.1, jump_penalty=0.02, jump_cap=25, ref=-1)


def _refusals():
    """(name, a word of its error text, call(lib, ctx handle) -> status) of every refusal of the three calls."""
    hipabi = pkg('hipabi')
    Geom = hipabi.BfGeom
    good_off = np.array([0, 600, 1000], dtype=np.int64)
    good_geoms = [Geom(100, 200, 10), Geom(50, 60, 0)]
    dev = C.c_void_p(256)                         # never dereferenced: the refusal comes first
    keep = []
    i64 = lambda *v: np.array(v, dtype=np.int64)

    def files(off, n, channels, geom, geoms, n_geom):
        ch = None if channels is None else np.array(channels, dtype=np.int32)
        gi = None if geom is None else np.array(geom, dtype=np.int32)
        table = None if geoms is None else (Geom * max(len(geoms), 1))(*geoms)
        keep.extend([ch, gi, table])
        nc = (0 if geoms is None else len(geoms)) if n_geom is None else n_geom
        p = lambda a: None if a is None else _ptr(a)
        return n, p(off), p(ch), p(gi), nc, table

    def gcc(off=good_off, n=2, channels=(2, 1), geom=(0, 1), geoms=good_geoms, n_geom=None, ref=(0, -1), d_in=dev, d_ref=dev,
            d_lag=dev, d_val=dev, d_curve=None, step_off=True, curve_off=True):
        n, off, ch, gi, nc, table = files(off, n, channels, geom, geoms, n_geom)
        rf = None if ref is None else np.array(ref, dtype=np.int32)
        so, co = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64)
        keep.extend([rf, so, co])
        return lambda lib, h: lib.spkd_bf_gcc(h, d_in, n, off, ch, gi, nc, table, None if rf is None else _ptr(rf), d_ref, d_lag,
                                              d_val, d_curve, _ptr(so) if step_off else None, _ptr(co) if curve_off else None)

    def total(off=good_off, n=2, channels=(2, 1), geom=(0, 1), geoms=good_geoms, n_geom=None, d_in=dev, d_delay=dev, d_out=dev,
              out_off=True):
        n, off, ch, gi, nc, table = files(off, n, channels, geom, geoms, n_geom)
        oo = np.zeros(3, dtype=np.int64)
        keep.append(oo)
        return lambda lib, h: lib.spkd_bf_sum(h, d_in, n, off, ch, gi, nc, table, d_delay, d_out, _ptr(oo) if out_off else None)

    def track(step_off=i64(0, 3, 5), n=2, channels=(2, 3), d_lag=dev, d_val=dev, n_best=4, min_peak=0.1, penalty=0.02, cap=25,
              d_delay=dev):
        ch = None if channels is None else np.array(channels, dtype=np.int32)
        keep.extend([ch, step_off])
        return lambda lib, h: lib.spkd_bf_track(h, n, None if step_off is None else _ptr(step_off), None if ch is None else _ptr(ch),
                                                d_lag, d_val, n_best, min_peak, penalty, cap, d_delay)

    out = []
    for call, tag in ((gcc, 'gcc'), (total, 'sum')):
        out += [(tag + ': negative file count', 'negative', call(n=-1)),
                (tag + ': negative geometry count', 'negative', call(n_geom=-1)),
                (tag + ': null in_off', 'null host', call(off=None)),
                (tag + ': null channels', 'null host', call(channels=None)),
                (tag + ': null geometry index', 'null host', call(geom=None)),
                (tag + ': null geometries', 'null host', call(geoms=None, n_geom=2)),
                (tag + ': in_off not from 0', 'start at 0', call(off=i64(2, 600, 1000))),
                (tag + ': decreasing in_off', 'non-decreasing', call(off=i64(0, 600, 400))),
                (tag + ': span no multiple of the channels', 'multiple', call(off=i64(0, 601, 1000))),
                (tag + ': no channel', 'channel count', call(channels=(0, 1))),
                (tag + ': nine channels', 'channel count', call(off=i64(0, 900, 1000), channels=(9, 1))),
                (tag + ': geometry index -1', 'index', call(geom=(-1, 1))),
                (tag + ': geometry index behind the last', 'index', call(geom=(0, 2))),
                (tag + ': hop 0', 'hop', call(geoms=[Geom(0, 200, 10), Geom(50, 60, 0)])),
                (tag + ': hop above 2^20', 'hop', call(geoms=[Geom((1 << 20) + 1, 200, 10), Geom(50, 60, 0)])),
                (tag + ': window 0', 'window', call(geoms=[Geom(100, 0, 10), Geom(50, 60, 0)])),
                (tag + ': negative max_lag', 'max_lag', call(geoms=[Geom(100, 200, -1), Geom(50, 60, 0)])),
                (tag + ': window + max_lag above the transform', '8192', call(geoms=[Geom(100, 8000, 193), Geom(50, 60, 0)])),
                (tag + ': null input with a sample', 'null device', call(d_in=None))]
    out += [('gcc: null ref', 'null host', gcc(ref=None)),
            ('gcc: null step_off', 'null host', gcc(step_off=False)),
            ('gcc: a curve without curve_off', 'null host', gcc(d_curve=dev, curve_off=False)),
            ('gcc: reference channel -2', 'reference channel', gcc(ref=(-2, 0))),
            ('gcc: reference channel behind the last', 'reference channel', gcc(ref=(2, 0))),
            ('gcc: null d_ref', 'null device', gcc(d_ref=None)),
            ('gcc: null d_lag', 'null device', gcc(d_lag=None)),
            ('gcc: null d_val', 'null device', gcc(d_val=None)),
            ('sum: null out_off', 'null host', total(out_off=False)),
            ('sum: null delays with a step', 'null device', total(d_delay=None)),
            ('sum: null output with a sample', 'null device', total(d_out=None)),
            ('track: negative file count', 'negative', track(n=-1)),
            ('track: null step_off', 'null host', track(step_off=None)),
            ('track: null channels', 'null host', track(channels=None)),
            ('track: step_off not from 0', 'start at 0', track(step_off=i64(1, 3, 5))),
            ('track: decreasing step_off', 'non-decreasing', track(step_off=i64(0, 3, 2))),
            ('track: nine channels', 'channel count', track(channels=(2, 9))),
            ('track: n_best 0', 'n_best', track(n_best=0)),
            ('track: n_best 5', 'n_best', track(n_best=5)),
            ('track: min_peak not a number', 'min_peak', track(min_peak=float('nan'))),
            ('track: negative jump_penalty', 'jump_penalty', track(penalty=-0.5)),
            ('track: infinite jump_penalty', 'jump_penalty', track(penalty=float('inf'))),
            ('track: negative jump_cap', 'jump_cap', track(cap=-1)),
            ('track: null candidates with a step', 'null device', track(d_lag=None)),
            ('track: null delays with a step', 'null device', track(d_delay=None))]
    return out


def test_argument_refusals_come_before_any_device_work():
    """No context, no device: every refusal is SPKD_EINVAL (a null context is itself refused first, so this
    shows only that no case touches a device on its way out; the GPU test tells the refusals apart)."""
    hipabi = pkg('hipabi')
    lib = hipabi.load_library()
    for name, _, call in _refusals():
        assert call(lib, None) == hipabi.SPKD_EINVAL, name


def test_geometry_per_rate_and_host_errors_before_the_context_is_touched():
    fe, pipeline = pkg('frontend'), pkg('pipeline')
    want = {8000: (2000, 4000, 80), 11025: (2756, 5512, 111), 16000: (4000, 8000, 160), 44100: (11025, 7751, 441),
            48000: (12000, 7712, 480), 96000: (24000, 7232, 960)}
    for rate, geom in want.items():
        assert fe.beamform_geometry(rate, pipeline.BEAMFORM) == geom, rate
        assert geom[1] + geom[2] <= 8192
    with pytest.raises(ValueError, match='largest delay'):
        fe.beamform_geometry(16000, _opts(max_delay_s=0.2570))            # D = 4112 > 4096
    assert fe.beamform_geometry(16000, _opts(max_delay_s=0.256))[2] == 4096
    with pytest.raises(ValueError, match='window'):
        fe.beamform_geometry(16000, _opts(window_s=0.0))
    with pytest.raises(ValueError, match='step'):
        fe.beamform_geometry(16000, _opts(step_s=0.0))
    ok = np.zeros((100, 2), dtype=np.int16)
    for call in (lambda a, o: fe.beamform_batch(None, a, o), lambda a, o: fe.resample_batch(None, a, 16000, beamform=o)):
        with pytest.raises(ValueError, match='int16 samples'):
            call([(ok, 48000), (np.zeros((2, 5, 2), dtype=np.int16), 48000)], pipeline.BEAMFORM)
        with pytest.raises(ValueError, match='channels'):
            call([(np.zeros((10, 9), dtype=np.int16), 48000)], pipeline.BEAMFORM)
        with pytest.raises(ValueError, match='sample rate'):
            call([(ok, 0)], pipeline.BEAMFORM)
        with pytest.raises(ValueError, match='keys of BEAMFORM'):
            call([(ok, 16000)], dict(step_s=0.25))
        with pytest.raises(ValueError, match='n_best'):
            call([(ok, 16000)], _opts(n_best=5))
        with pytest.raises(ValueError, match='reference channel'):
            call([(ok, 16000)], _opts(ref=2))
        with pytest.raises(ValueError, match='one per file'):
            call([(ok, 16000)], _opts(ref=[0, 0]))
        with pytest.raises(ValueError, match='negative'):
            call([(ok, 16000)], _opts(jump_penalty=-1.0))
    model = types.SimpleNamespace(cfg=types.SimpleNamespace(sample_rate=16000, hop=_cfg(400).hop))
    with pytest.raises(ValueError, match='keys of BEAMFORM'):
        pipeline.diarize_audio_batch(None, model, _cfg(400), [(ok, 48000)], beamform={})


@pytest.mark.parametrize('name', B.SCENES)
def test_the_restatement_recovers_the_true_delays(name):
    sc, r = _scene(name)
    H, W, D = sc['geom']
    x = sc['x']
    T = len(r['delay'])
    assert T == B.steps(len(x), x.shape[1], sc['geom']) and r['ref'] == 0
    inside = 0
    for t in range(T):
        for lo, hi, d in sc['truth']:
            if lo <= t * H and (t * H + W <= hi or T == 1):
                assert r['delay'][t].tolist() == list(d), (name, t)
                inside += 1
    if name in ('S1', 'S1c'):
        assert inside == T == 11 and r['reliable'].all()
        best, second = r['val'][:, 1:, 0], r['val'][:, 1:, 1]
        assert best.min() >= 0.7 and second.max() <= 0.03
    if name == 'S2':
        assert r['delay'][:, 1].tolist() == [37] * 5 + [-12] * 6 and r['delay'][:, 2].tolist() == [-160] * 5 + [90] * 6
    if name == 'S3':                              # the arg-max goes to the intruder, the Viterbi does not
        flipped = [(t, c) for t in range(T) for c in (1, 2, 3) if r['lag'][t, c, 0] != r['delay'][t, c]]
        assert flipped and all(t in (4, 5, 6) for t, _ in flipped), flipped
        assert all(r['delay'][t].tolist() == [0, 37, -160, 5] for t in range(T))
    if name == 'S4':
        assert r['reliable'][:, 1].tolist() == [True, True] + [False] * 7 + [True, True]
        assert r['delay'][:, 1].tolist() == [37] * 11
        assert r['val'][2:5, 1, 0].tolist() == [0.0] * 3 and r['lag'][2:5, 1, 0].tolist() == [-D] * 3
        assert 0.0 < r['val'][5:9, 1, 0].max() < 0.06
    if name == 'S5':
        assert T == 1 and r['reliable'].tolist() == [[True, True, False]] and r['delay'].tolist() == [[0, 9, 0]]
        assert r['lag'][0, 2].tolist() == [-D] * 4 and r['val'][0, 2].tolist() == [0.0, NEG, NEG, NEG]


def test_aligning_beats_one_microphone_and_the_plain_average():
    """S1: four equal channels and a white source: the derived gain over one channel is 10 log10 4 = 6.0 dB."""
    sc, r = _scene('S1')
    x, clean = sc['x'], sc['clean']
    one, mean, aligned = B.snr_db(x[:, 0], clean), B.snr_db(x.astype(np.float64).mean(axis=1), clean), B.snr_db(r['out'], clean)
    print('SNR: one channel %.2f dB, plain average %.2f dB, aligned %.2f dB' % (one, mean, aligned))
    assert aligned >= one + 5.0 and aligned >= mean + 15.0 and mean < one


def _guard(lag, val):
    """The margins of one scene's decisions, in float64 -> (smallest slot gap, smallest path gap, nearest to min_peak)."""
    T, Cn = lag.shape[:2]
    slot, path, near = np.inf, np.inf, np.inf
    for c in range(Cn):
        v0, v1 = val[:, c, 0].astype(np.float64), val[:, c, 1].astype(np.float64)
        if np.all(v0 == 1.0) and np.all(v1 == NEG):
            continue                              # the reference channel
        _, reliable, margin = B.track_channel(lag[:, c], val[:, c], margin=True, **TRACK)
        slot = min(slot, np.min((v0 - v1)[reliable], initial=np.inf))
        path = min(path, margin)
        near = min(near, np.abs(v0 - B.MIN_PEAK).min())
    return slot, path, near


@pytest.mark.parametrize('name', B.SCENES + ('long',))
def test_fixture_guard_every_decision_has_a_margin(name):
    """Slot 0 against slot 1 at reliable steps and the winning path against the runner-up: >= 0.05; no slot-0
    value within 0.01 of min_peak.  A scene that fails this is a bad fixture, mended here."""
    r = B.beamform(_long_file(), G16, ref=0) if name == 'long' else _scene(name)[1]
    slot, path, near = _guard(r['lag'], r['val'])
    print('%s: slot gap %.3f, path gap %.3f, nearest to min_peak %.3f' % (name, slot, path, near))
    assert slot >= 0.05 and path >= 0.05 and near >= 0.01


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def ctx():
    c = pkg('hipabi').Context(0)
    yield c
    c.close()


def _guarded(ctx, name, host):
    """A device buffer holding `host` behind one item of padding, with GUARD items of a fixed pattern behind it."""
    buf = np.frombuffer(bytes([GUARD_BYTE]) * ((1 + len(host) + GUARD) * host.itemsize), dtype=host.dtype).copy()
    d = ctx.dev_scratch('test_bf_' + name, buf.nbytes)
    ctx.h2d(d, buf)
    return d + host.itemsize, d, buf


def _fetch(ctx, handle, n):
    d_first, d, buf = handle
    ctx.d2h(buf, d)
    pattern = np.frombuffer(bytes([GUARD_BYTE]) * buf.itemsize, dtype=buf.dtype)[0]
    assert buf[:1].tobytes() == pattern.tobytes() and buf[1 + n:].tobytes() == pattern.tobytes() * GUARD, 'written around the buffer'
    return buf[1:1 + n].copy()


def _device(ctx, files, refs=None, lead=1, delays=None, curves=True, **track):
    """The three calls on buffers of the test's own: files = [(int16 [n, C], geom)] -> one dictionary per file
    (ref, curve, lag, val, delay, out).  The raw audio lies behind `lead` int16 of padding (an odd count puts the
    first file on an odd element); every output has a guard pattern behind it, checked.  delays: hand-made
    delays [T, C] per file for the sum, in place of the tracker's."""
    hipabi = pkg('hipabi')
    opts = dict(TRACK, **track)
    geoms = sorted(set(g for _, g in files))
    gi = [geoms.index(g) for _, g in files]
    ch = [x.shape[1] for x, _ in files]
    refs = [-1] * len(files) if refs is None else refs
    raw = np.concatenate([np.zeros(lead, dtype=np.int16)] + [x.ravel() for x, _ in files])
    in_off = np.concatenate([[0], np.cumsum([x.size for x, _ in files])]).astype(np.int64)
    T = np.array([B.steps(len(x), x.shape[1], g) for x, g in files], dtype=np.int64)
    wg = np.concatenate([[0], np.cumsum(T * np.array(ch, dtype=np.int64))]).astype(np.int64)
    cv = np.concatenate([[0], np.cumsum(np.diff(wg) * np.array([2 * g[2] + 1 for _, g in files], dtype=np.int64))]).astype(np.int64)
    n_out = np.concatenate([[0], np.cumsum([len(x) for x, _ in files])]).astype(np.int64)
    d_raw = ctx.dev_scratch('test_bf_raw', max(raw.nbytes, 16))
    ctx.h2d(d_raw, raw)
    h_ref = _guarded(ctx, 'ref', np.zeros(len(files), dtype=np.int32))
    h_lag = _guarded(ctx, 'lag', np.zeros(4 * wg[-1], dtype=np.int32))
    h_val = _guarded(ctx, 'val', np.zeros(4 * wg[-1], dtype=np.float32))
    h_cv = _guarded(ctx, 'curve', np.zeros(cv[-1] if curves else 0, dtype=np.float32))
    h_delay = _guarded(ctx, 'delay', np.zeros(wg[-1], dtype=np.int32))
    h_out = _guarded(ctx, 'out', np.zeros(n_out[-1], dtype=np.int16))
    step_off, curve_off = ctx.bf_gcc(d_raw + 2 * lead, in_off, ch, gi, geoms, refs, h_ref[0], h_lag[0], h_val[0],
                                     h_cv[0] if curves else None)
    assert np.array_equal(np.diff(step_off), T) and np.array_equal(curve_off, cv)
    ctx.bf_track(step_off, ch, h_lag[0], h_val[0], opts['n_best'], opts['min_peak'], opts['penalty'], opts['cap'], h_delay[0])
    if delays is not None:
        flat = np.concatenate([np.asarray(d, dtype=np.int32).ravel() for d in delays] + [np.zeros(0, dtype=np.int32)])
        assert len(flat) == wg[-1]
        if len(flat):
            ctx.h2d(h_delay[0], flat)
    out_off = ctx.bf_sum(d_raw + 2 * lead, in_off, ch, gi, geoms, h_delay[0], h_out[0])
    assert np.array_equal(out_off, n_out)
    ref, lag, val = _fetch(ctx, h_ref, len(files)), _fetch(ctx, h_lag, 4 * wg[-1]), _fetch(ctx, h_val, 4 * wg[-1])
    curve, delay, out = _fetch(ctx, h_cv, cv[-1] if curves else 0), _fetch(ctx, h_delay, wg[-1]), _fetch(ctx, h_out, n_out[-1])
    res = []
    for f, (x, g) in enumerate(files):
        shape = (int(T[f]), ch[f])
        res.append(dict(ref=int(ref[f]), lag=lag[4 * wg[f]:4 * wg[f + 1]].reshape(shape + (4,)),
                        val=val[4 * wg[f]:4 * wg[f + 1]].reshape(shape + (4,)),
                        curve=curve[cv[f]:cv[f + 1]].reshape(shape + (2 * g[2] + 1,)) if curves else None,
                        delay=delay[wg[f]:wg[f + 1]].reshape(shape), out=out[n_out[f]:n_out[f + 1]]))
    return res


def _same(a, b, what=('ref', 'lag', 'val', 'delay', 'out')):
    return all(np.array_equal(a[k], b[k]) for k in what)


@pytest.fixture(scope='module')
def on_device(ctx):
    """Every scene through the three calls, once: {name: result}."""
    return {name: _device(ctx, [(_scene(name)[0]['x'], G16)], refs=[0])[0] for name in B.SCENES}


def _curve_bound():
    with open(os.path.join(ROOT, 'profiles', 'beamform_accuracy.json')) as f:
        rec = json.load(f)
    assert sorted(rec['scenes']) == sorted(B.SCENES)
    return 16.0 * rec['max_abs_diff']


@pytest.mark.gpu
@pytest.mark.parametrize('name', B.SCENES)
def test_the_correlation_equals_the_float64_restatement(on_device, name):
    bound = _curve_bound()
    got, want = on_device[name]['curve'], B.curve(_scene(name)[0]['x'], 0, G16, dtype=np.float64)
    diff = float(np.abs(got.astype(np.float64) - want).max())
    print('%s: %d values, largest difference %.3e, bound %.3e' % (name, got.size, diff, bound))
    assert got.shape == want.shape and np.isfinite(got).all()
    assert bound <= MAX_CURVE_BOUND
    assert diff <= bound


@pytest.mark.gpu
@pytest.mark.parametrize('name', B.SCENES)
def test_the_candidates_are_the_rule_applied_to_the_devices_own_curve(on_device, name):
    r = on_device[name]
    lag, val = B.candidates(r['curve'], 0, G16[2])
    assert np.array_equal(r['lag'], lag) and np.array_equal(r['val'], val)
    assert r['lag'][:, 0].tolist() == [[0] * 4] * len(lag) and r['val'][:, 0].tolist() == [[1.0, NEG, NEG, NEG]] * len(lag)
    if name == 'S5':
        assert r['lag'][0, 2].tolist() == [-160] * 4 and r['val'][0, 2].tolist() == [0.0, NEG, NEG, NEG]
    if name == 'S4':
        assert r['lag'][2:5, 1, 0].tolist() == [-160] * 3 and r['val'][2:5, 1].tolist() == [[0.0, NEG, NEG, NEG]] * 3


@pytest.mark.gpu
@pytest.mark.parametrize('name', B.SCENES)
def test_the_delays_are_the_restatements_on_the_devices_candidates_and_the_scenes_own(on_device, name):
    sc, host = _scene(name)
    r = on_device[name]
    delay, _ = B.track(r['lag'], r['val'], **TRACK)
    assert np.array_equal(r['delay'], delay)
    assert np.array_equal(r['out'], B.delay_sum(sc['x'], G16, r['delay']))
    # the guard gives every decision a margin 500 times the correlation's bound: the host's decisions too
    assert np.array_equal(r['delay'], host['delay']) and np.array_equal(r['out'], host['out'])
    H, W, _ = G16
    if name in ('S1', 'S2', 'S3'):
        for t in range(len(delay)):
            for lo, hi, d in sc['truth']:
                if lo <= t * H and t * H + W <= hi:
                    assert r['delay'][t].tolist() == list(d), (name, t)


def _track_tables(ctx, tables, **track):
    """Hand-made candidates straight into spkd_bf_track: tables = [(lag [T, C, 4], val [T, C, 4])] -> [delay [T, C]]."""
    opts = dict(TRACK, **track)
    lag = np.concatenate([np.asarray(l, dtype=np.int32).ravel() for l, _ in tables])
    val = np.concatenate([np.asarray(v, dtype=np.float32).ravel() for _, v in tables])
    shapes = [np.asarray(l).shape[:2] for l, _ in tables]
    step_off = np.concatenate([[0], np.cumsum([s[0] for s in shapes])]).astype(np.int64)
    wg = np.concatenate([[0], np.cumsum([s[0] * s[1] for s in shapes])]).astype(np.int64)
    d_lag, d_val = ctx.dev_scratch('test_bf_tlag', max(lag.nbytes, 16)), ctx.dev_scratch('test_bf_tval', max(val.nbytes, 16))
    ctx.h2d(d_lag, lag)
    ctx.h2d(d_val, val)
    h_delay = _guarded(ctx, 'tdelay', np.zeros(wg[-1], dtype=np.int32))
    ctx.bf_track(step_off, [s[1] for s in shapes], d_lag, d_val, opts['n_best'], opts['min_peak'], opts['penalty'], opts['cap'],
                 h_delay[0])
    delay = _fetch(ctx, h_delay, wg[-1])
    return [delay[wg[f]:wg[f + 1]].reshape(s) for f, s in enumerate(shapes)]


def _hand_tables():
    """Candidate tables for the ties and rules no audio can aim at: [(name, lag [T, C, 4], val [T, C, 4], options)]."""
    f32 = lambda v: np.array(v, dtype=np.float32)
    rng = np.random.default_rng(31)
    out = []
    # equal path scores: two slots with the same value at every step, lags one apart on either side
    lag = np.array([[[5, 7, 6, 6]], [[6, 6, 5, 7]], [[7, 5, 6, 6]]])
    val = np.full((3, 1, 4), 0.5)
    out.append(('equal scores: lower j, lower k', lag, val, {}))
    out.append(('n_best 1', lag, val, dict(n_best=1)))
    out.append(('n_best 2', lag, val, dict(n_best=2)))
    # a later slot that is better than slot 0 unless the cap or the penalty holds it back
    lag = np.array([[[0, 40, 0, 0]], [[40, 0, 40, 40]], [[0, 40, 0, 0]], [[40, 1, 40, 40]]])
    val = np.array([[[0.5, 0.45, NEG, NEG]], [[0.5, 0.45, NEG, NEG]], [[0.5, 0.45, NEG, NEG]], [[0.5, 0.45, NEG, NEG]]])
    for name, kw in (('default', {}), ('jump_cap 0', dict(cap=0)), ('penalty 0', dict(penalty=0.0)), ('cap 1000', dict(cap=1000)),
                     ('penalty 1', dict(penalty=1.0)), ('n_best 1', dict(n_best=1))):
        out.append(('jumps: ' + name, lag, val, kw))
    # -INFINITY slots carry slot 0's lag and must never be chosen, however cheap the jump to them
    out.append(('absent slots', np.array([[[3, 3, 3, 3]], [[90, 3, 90, 90]], [[3, 3, 3, 3]]]),
                np.array([[[0.3, NEG, NEG, NEG]], [[0.3, NEG, NEG, NEG]], [[0.3, NEG, NEG, NEG]]]), dict(penalty=1.0)))
    # no reliable step at all; leading and trailing unreliable runs; T = 1; channels side by side
    lag = rng.integers(-160, 161, (9, 3, 4))
    val = np.sort(rng.uniform(0.2, 0.9, (9, 3, 4)), axis=2)[:, :, ::-1].copy()
    val[:, 0] *= 0.1                              # channel 0: never reliable
    val[:3, 1] *= 0.1                             # channel 1: a leading run
    val[6:, 1] *= 0.1                             # and a trailing one
    val[4, 2] *= 0.1                              # channel 2: one step inside
    out.append(('unreliable runs', lag, val, {}))
    out.append(('T = 1', lag[:1], val[:1], {}))
    out.append(('T = 1, unreliable', lag[:1], val[:1] * 0.01, {}))
    # T = 77: more steps than a wave has lanes; lags drift, values wander around min_peak
    lag = np.cumsum(rng.integers(-3, 4, (77, 2, 4)), axis=0) + rng.integers(-20, 21, (1, 2, 4))
    val = np.sort(rng.uniform(0.02, 0.6, (77, 2, 4)), axis=2)[:, :, ::-1].copy()
    val[:, :, 3] = np.where(rng.random((77, 2)) < 0.3, NEG, val[:, :, 3])
    out.append(('T = 77', lag, val, {}))
    out.append(('T = 77, n_best 2, min_peak 0.3', lag, val, dict(n_best=2, min_peak=0.3)))
    return [(n, np.asarray(l, dtype=np.int32), f32(v), kw) for n, l, v, kw in out]


@pytest.mark.gpu
def test_hand_made_candidates_hold_the_ties_and_rules(ctx):
    for name, lag, val, kw in _hand_tables():
        got = _track_tables(ctx, [(lag, val)], **kw)[0]
        want, _ = B.track(lag, val, **dict(TRACK, **kw))
        assert np.array_equal(got, want), (name, got.T.tolist(), want.T.tolist())
    # what the rules mean, on the restatement itself
    by = {n: B.track(l, v, **dict(TRACK, **kw))[0][:, 0].tolist() for n, l, v, kw in _hand_tables() if l.shape[1] == 1}
    assert by['n_best 1'] == [5, 6, 7] and by['jumps: default'] == [40, 40, 40, 40] and by['jumps: n_best 1'] == [0, 40, 0, 40]
    assert by['jumps: jump_cap 0'] == [0, 40, 0, 40] and by['jumps: penalty 0'] == [0, 40, 0, 40]
    assert by['jumps: penalty 1'] == [40, 40, 40, 40]
    assert by['absent slots'] == [3, 90, 3]
    # several tables in one call are the tables alone
    tables = [(l, v) for _, l, v, kw in _hand_tables() if not kw]
    for got, (l, v) in zip(_track_tables(ctx, tables), tables):
        assert np.array_equal(got, B.track(l, v, **TRACK)[0])


def _sum_files():
    """(name, file, geom, delays, lead): hand-made delays that change at every step and reach +-D."""
    rng = np.random.default_rng(8)
    H, W, D = 300, 500, 40
    geom = (H, W, D)
    out = []

    def add(name, n, Cn, lead=1, loud=False, g=geom):
        x = (rng.integers(-32768, 32768, (n, Cn)) if loud else rng.integers(-9000, 9001, (n, Cn))).astype(np.int16)
        T = B.steps(n, Cn, g)
        delay = rng.integers(-g[2], g[2] + 1, (T, Cn)).astype(np.int32)
        if T:
            delay[0, 0], delay[-1, -1] = -g[2], g[2]
        out.append((name, x, g, delay, lead))

    add('2 channels, aligned base', 2345, 2, lead=2)
    add('2 channels, odd offset', 2345, 2, lead=1)
    add('3 channels', 3 * 2048 + 17, 3)
    add('8 channels', 2049, 8)
    for n in (0, 1, W, W + 1, W + H - 1, W + H, W - 123):
        add('length %d' % n, n, 2 + n % 2)
    add('mono, copied through', 777, 1)
    add('full scale', 1500, 4, loud=True)
    return out


@pytest.mark.gpu
def test_the_sum_is_exact_for_hand_made_delays(ctx):
    files = _sum_files()
    for name, x, g, delay, lead in files:
        got = _device(ctx, [(x, g)], lead=lead, delays=[delay], curves=False)[0]['out']
        assert np.array_equal(got, B.delay_sum(x, g, delay)), name
    # all of them in one call, on either parity
    for lead in (1, 2):
        res = _device(ctx, [(x, g) for _, x, g, _, _ in files], lead=lead, delays=[d for _, _, _, d, _ in files], curves=False)
        for r, (name, x, g, delay, _) in zip(res, files):
            assert np.array_equal(r['out'], B.delay_sum(x, g, delay)), name
    # saturation: four full-scale channels that agree in sign
    x = np.full((1000, 4), 32767, dtype=np.int16)
    x[500:] = -32768
    zero = np.zeros((B.steps(1000, 4, (300, 500, 40)), 4), dtype=np.int32)
    got = _device(ctx, [(x, (300, 500, 40))], delays=[zero], curves=False)[0]['out']
    assert got[:500].tolist() == [32767] * 500 and got[500:].tolist() == [-32768] * 500
    loud = [r for r in files if r[0] == 'full scale'][0]
    assert np.abs(B.delay_sum(loud[1], loud[2], loud[3]).astype(np.int32)).max() > 20000


@pytest.mark.gpu
def test_the_reference_channel_is_the_requested_or_the_loudest(ctx):
    rng = np.random.default_rng(12)
    g = (1000, 2000, 30)
    x = rng.integers(-2000, 2001, (6000, 3)).astype(np.int16)
    x[:, 1] = x[:, 0]                             # two identical channels and a quieter third: index 0 wins
    x[:, 2] //= 2
    assert _device(ctx, [(x, g)], refs=[-1], curves=False)[0]['ref'] == 0 == B.pick_ref(x)
    assert [_device(ctx, [(x, g)], refs=[k], curves=False)[0]['ref'] for k in (0, 1, 2)] == [0, 1, 2]
    z = np.full((3000, 3), 100, dtype=np.int16)   # energies that differ by one: channel 0 has a 1 where the others have a 0
    z[:2] = 0
    z[1, 0] = 1
    e = [sum(int(v) ** 2 for v in z[:, c]) for c in range(3)]
    assert e[0] == e[1] + 1 == e[2] + 1
    files = [z, z[:, ::-1].copy(), z[:, [1, 0, 2]].copy()]
    res = _device(ctx, [(f, g) for f in files], curves=False)
    assert [r['ref'] for r in res] == [0, 2, 1] == [B.pick_ref(f) for f in files]
    for r, f in zip(res, files):
        assert np.array_equal(r['out'], B.delay_sum(f, g, r['delay']))


def _mixed_batch():
    """Geometries for 8, 16, 44.1 and 48 kHz, channel counts 1, 2, 3 and 8, empty files first, in the middle and last."""
    fe = pkg('frontend')
    rng = np.random.default_rng(21)
    rates = (8000, 16000, 44100, 48000)
    plan = [(0, 2, 0), (9000, 2, 1), (30000, 3, 3), (7000, 1, 0), (0, 3, 2), (25000, 8, 2), (12345, 2, 3), (4000, 3, 0), (0, 1, 1)]
    files = []
    for n, Cn, k in plan:
        s = 3000.0 * rng.standard_normal(n + 600)
        d = rng.integers(-60, 61, Cn)
        d[0] = 0
        x = np.stack([s[300 - int(k2):300 - int(k2) + n] for k2 in d], axis=1) + 900.0 * rng.standard_normal((n, Cn))
        files.append((np.clip(np.rint(x), -32768, 32767).astype(np.int16), fe.beamform_geometry(rates[k], pkg('pipeline').BEAMFORM),
                      rates[k]))
    return files


@pytest.mark.gpu
def test_a_file_of_a_mixed_batch_is_the_file_alone_in_any_order_and_grouping(ctx):
    fe = pkg('frontend')
    batch = _mixed_batch()
    files = [(x, g) for x, g, _ in batch]
    assert sorted(set(x.shape[1] for x, _ in files)) == [1, 2, 3, 8] and len(set(g for _, g in files)) == 4
    alone = [_device(ctx, [f])[0] for f in files]
    together = _device(ctx, files)
    for f, (a, b) in enumerate(zip(alone, together)):
        if len(files[f][0]) == 0:                 # alone it is a call without a sample: nothing launched, nothing written
            assert len(a['out']) == len(b['out']) == 0
            alone[f] = b
            continue
        assert _same(a, b) and np.array_equal(a['curve'], b['curve']), f
    order = list(np.random.default_rng(4).permutation(len(files)))
    assert order != sorted(order)
    for slot, r in enumerate(_device(ctx, [files[i] for i in order], lead=2)):
        assert _same(r, alone[order[slot]]), (slot, order[slot])
    # the host entry points: beamform_batch is the three calls, and two groupings give one d_pcm
    audios = [(x, rate) for x, _, rate in batch]
    detail, timings = {}, {}
    d_mono, off = fe.beamform_batch(ctx, audios, pkg('pipeline').BEAMFORM, timings=timings, detail=detail)
    mono = np.zeros(int(off[-1]), dtype=np.int16)
    ctx.d2h(mono, d_mono)
    assert all(len(timings[k]) == 1 and timings[k][0] > 0 for k in ('bf_gcc', 'bf_track', 'bf_sum', 'wall_upload'))
    for f, a in enumerate(alone):
        assert np.array_equal(mono[off[f]:off[f + 1]], a['out']) and detail['ref'][f] == a['ref'], f
        assert np.array_equal(detail['delay'][f], a['delay']), f
        assert np.array_equal(detail['reliable'][f], a['val'][:, :, 0] >= np.float32(B.MIN_PEAK)), f
    pcms = []
    for group_bytes in (1 << 28, sum(x.nbytes for x, _ in files) // 4):
        d_pcm, sample_off = fe.resample_batch(ctx, audios, 16000, group_bytes=group_bytes, beamform=pkg('pipeline').BEAMFORM)
        pcm = np.zeros(int(sample_off[-1]), dtype=np.int16)
        ctx.d2h(pcm, d_pcm)
        pcms.append((pcm, sample_off))
    assert np.array_equal(pcms[0][0], pcms[1][0]) and np.array_equal(pcms[0][1], pcms[1][1]) and pcms[0][0].any()
    # and that d_pcm is the resampler's on the beamformed mono files
    d_pcm, sample_off = fe.resample_batch(ctx, [(a['out'], rate) for a, (_, _, rate) in zip(alone, batch)], 16000)
    pcm = np.zeros(int(sample_off[-1]), dtype=np.int16)
    ctx.d2h(pcm, d_pcm)
    assert np.array_equal(pcm, pcms[0][0]) and np.array_equal(sample_off, pcms[0][1])


@pytest.mark.gpu
def test_refusals_on_a_context_name_their_reason_and_leave_it_usable(ctx, on_device):
    hipabi = pkg('hipabi')
    for name, word, call in _refusals():
        assert call(ctx.lib, ctx.h) == hipabi.SPKD_EINVAL, name
        assert word in ctx.lib.spkd_last_error(ctx.h).decode(), (name, ctx.lib.spkd_last_error(ctx.h).decode())
    # no file, or no sample: nothing is launched (null device pointers would have been refused)
    for n in (0, 2):
        step_off, _ = ctx.bf_gcc(0, [0] * (n + 1), [2, 1][:n], [0, 0][:n], [G16], [-1, 0][:n], 0, 0, 0)
        assert list(step_off) == [0, 1, 1][:n + 1]
        assert list(ctx.bf_sum(0, [0] * (n + 1), [2, 1][:n], [0, 0][:n], [G16], 0, 0)) == [0] * (n + 1)
    ctx.bf_track([0, 0, 0], [2, 3], 0, 0, 4, 0.1, 0.02, 25, 0)
    fe = pkg('frontend')
    assert list(fe.beamform_batch(ctx, [], pkg('pipeline').BEAMFORM)[1]) == [0]
    assert list(fe.beamform_batch(ctx, [(np.zeros((0, 2), dtype=np.int16), 16000)], pkg('pipeline').BEAMFORM)[1]) == [0, 0]
    again = _device(ctx, [(_scene('S5')[0]['x'], G16)], refs=[0])[0]
    assert _same(again, on_device['S5'])


@pytest.fixture(scope='module')
def model(tmp_path_factory):
    d = str(tmp_path_factory.mktemp('vad_model'))
    write_model(d, *_synthetic_mixtures(np.random.default_rng(11)))
    return load_model(d)


def _download(ctx, uploaded):
    d_pcm, sample_off = uploaded
    pcm = np.zeros(int(sample_off[-1]), dtype=np.int16)
    if pcm.size:
        ctx.d2h(pcm, d_pcm)
    return [pcm[sample_off[f]:sample_off[f + 1]].copy() for f in range(len(sample_off) - 1)]


@pytest.mark.gpu
def test_recordings_to_speakers_with_beamforming_equals_the_chain_on_the_aligned_files(ctx, model):
    fe, pipeline = pkg('frontend'), pkg('pipeline')
    cfg = _cfg(400)
    x = _long_file()
    opts = _opts(ref=0)
    detail = {}
    mono = _download(ctx, fe.beamform_batch(ctx, [(x, 16000)], opts, detail=detail))[0]
    host = B.beamform(x, G16, ref=0)
    assert detail['delay'][0].shape == (77, 2) and np.array_equal(detail['delay'][0], host['delay'])
    assert detail['delay'][0][:, 1].tolist() == [37] * 77 and np.array_equal(mono, host['out'])
    timings = {}
    rows = pipeline.diarize_audio_batch(ctx, model, cfg, [(x, 16000)], beamform=opts, timings=timings)
    assert all(len(timings[k]) == 1 for k in ('bf_gcc', 'bf_track', 'bf_sum', 'resample'))
    want = pipeline.diarize_pcm_batch(ctx, model, cfg, [mono])
    print('segments:', [len(r) for r in want])
    assert len(rows) == len(want) == 1 and len(want[0]) >= 2
    assert rows[0].shape == want[0].shape and np.all(rows[0] == want[0])
    # beamform=None is the call without the argument: the plain average, the chain on the resampler's output
    plain = pipeline.diarize_audio_batch(ctx, model, cfg, [(x, 16000)], beamform=None)
    same = pipeline.diarize_audio_batch(ctx, model, cfg, [(x, 16000)])
    ref = pipeline.diarize_pcm_batch(ctx, model, cfg, _download(ctx, fe.resample_batch(ctx, [(x, 16000)], 16000)))
    for a, b in ((plain, same), (plain, ref)):
        assert a[0].shape == b[0].shape and np.all(a[0] == b[0])


def _write_wav(path, samples, rate):
    with wave.open(path, 'wb') as w:
        w.setnchannels(samples.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(samples, dtype='<i2').tobytes())


@pytest.mark.gpu
def test_from_48_khz_and_to16k_beamform_write_the_resampled_aligned_file(ctx, tmp_path):
    fe, pipeline = pkg('frontend'), pkg('pipeline')
    rng = np.random.default_rng(9)
    n, d = 60000, (0, 111, -300)
    s = 3000.0 * rng.standard_normal(n + 1000)
    x = np.stack([s[500 - k:500 - k + n] for k in d], axis=1) + 900.0 * rng.standard_normal((n, 3))
    x = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    detail = {}
    mono = _download(ctx, fe.beamform_batch(ctx, [(x, 48000)], pipeline.BEAMFORM, detail=detail))[0]
    r = detail['ref'][0]
    assert all(row.tolist() == [k - d[r] for k in d] for row in detail['delay'][0]) and len(detail['delay'][0]) == 5
    want = _download(ctx, fe.resample_batch(ctx, [(mono, 48000)], 16000))[0]
    got = _download(ctx, fe.resample_batch(ctx, [(x, 48000)], 16000, beamform=pipeline.BEAMFORM))[0]
    assert len(got) == 20000 and np.array_equal(got, want)
    assert not np.array_equal(got, _download(ctx, fe.resample_batch(ctx, [(x, 48000)], 16000))[0])
    src, dst = str(tmp_path / 'in.wav'), str(tmp_path / 'out.wav')
    _write_wav(src, x, 48000)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'to16k.py'), src, '-o', dst, '--beamform'], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    with wave.open(dst, 'rb') as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 16000)
        assert np.array_equal(np.frombuffer(w.readframes(w.getnframes()), dtype='<i2'), want)
