"""The front-end for a whole batch (spkd_mfcc_batch, frontend.upload_batch / extract_batch,
pipeline.features_batch / diarize_pcm_batch) against the per-file path: for every file of a batch
the features equal spkd_mfcc's on that file alone TO THE BIT, for both window widths -- the file
lengths sit on and around every tile and window of the kernels (static tile 8, post tile 128 and
its halo of 4, mean window 75 to either side) with sample offsets that are no multiple of the hop,
and loud files lie next to nearly silent ones, so a sample or a static row taken from a neighbour
shows.  Nothing here has a tolerance except the comparison with the numpy restatement, which takes
tests/test_mfcc_reference.py's."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from conftest import pkg
from helpers import ROOT
from mfcc_compare import full_chain_bound, full_chain_ratios
from test_frontend import GOLD, _cfg_text, _signal as _tone
from test_generate_exp import _signal, _synthetic_mixtures, load_model, write_model

HOP = 128
GUARD = 64                                          # rows behind the features, which the call must not touch
NAN_PATTERN = 0x7fc0dead
# frames / remainder of the files of the border batch; empty files first, in the middle and last
LENGTHS = [0, 100, HOP * 1, HOP * 7 + 5, HOP * 8, HOP * 9 + 127, HOP * 74, HOP * 75 + 1, 0, HOP * 76, HOP * 127,
           HOP * 128, HOP * 129 + 64, HOP * 137, HOP * 151 + 3, 48017, 0]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _cfg(window):
    return pkg('feaconfig').FeatureConfig(_cfg_text(GOLD).replace('window_width 400', 'window_width %d' % window))


def _border_files():
    """Full-scale noise and near-silence in turn (the level is what a leak across a border carries)."""
    rng = np.random.default_rng(20261017)
    return [(rng.integers(-32768, 32768, n) if i % 2 else rng.integers(-3, 4, n)).astype(np.int16)
            for i, n in enumerate(LENGTHS)]


# ------------------------------------------------------------------ not GPU
def test_entry_point_and_timers_are_declared_and_exported():
    hipabi = pkg('hipabi')
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'spkd.h')).read(), flags=re.S)
    lib = hipabi.load_library()
    assert re.search(r'\bspkd_mfcc_batch\s*\(', code)
    assert 'spkd_mfcc_batch' in hipabi.EXPORTS and hasattr(lib, 'spkd_mfcc_batch')
    names = [n for n, _ in sorted(hipabi.TIMERS.items(), key=lambda kv: kv[1])]
    enum = re.search(r'enum \{\s*SPKD_T_CALL = 0,(.*?)SPKD_N_TIMERS', code, flags=re.S).group(1)
    assert ['call'] + [n.strip()[len('SPKD_T_'):].lower() for n in enum.split(',') if n.strip()] == names
    assert names[-2:] == ['mfcc_static', 'mfcc_post']


def _refusals():
    """(name, call(lib, ctx handle) -> status) of every argument refusal of spkd_mfcc_batch."""
    fe = pkg('frontend')
    cfg = _cfg(400)
    tables = [np.ascontiguousarray(a, dtype=np.float32) for a in
              (fe.mel_filterbank(cfg.sample_rate), fe.dct_matrix(cfg.n_cep), cfg.mean, cfg.scale, cfg.transform)]
    good = np.array([0, 300, 1000], dtype=np.int64)
    dev = C.c_void_p(256)                         # never dereferenced: the refusal comes first
    keep = []

    def call(off=good, n=2, frame_off=True, tabs=None, d_pcm=dev, d_out=dev, params=True, **change):
        p = fe.mfcc_params(cfg)
        for k, v in change.items():
            setattr(p, k, v)
        out = np.zeros(3, dtype=np.int64)
        keep.extend([p, out])
        ptrs = [_ptr(a) for a in tables] if tabs is None else tabs
        return lambda lib, h: lib.spkd_mfcc_batch(h, d_pcm, n, None if off is None else _ptr(off),
                                                  C.byref(p) if params else None, *ptrs, d_out,
                                                  _ptr(out) if frame_off else None)

    return [('a window width this build does not do', call(window_width=300)),
            ('transform length', call(n_fft=1024)),
            ('frame rate that does not divide the sample rate', call(frame_rate=127)),
            ('delta width 3', call(delta_width=(C.c_int32 * 2)(3, 2))),
            ('delta normalization 0', call(delta_norm=(C.c_float * 2)(0.0, 10.0))),
            ('mean window too wide', call(cms_left=2000)),
            ('null parameters', call(params=False)),
            ('null filterbank', call(tabs=[None] + [_ptr(a) for a in tables[1:]])),
            ('null transform', call(tabs=[_ptr(a) for a in tables[:-1]] + [None])),
            ('negative file count', call(n=-1)),
            ('null sample_off', call(off=None)),
            ('null frame_off', call(frame_off=False)),
            ('sample_off not from 0', call(off=np.array([1, 300, 1000], dtype=np.int64))),
            ('decreasing sample_off', call(off=np.array([0, 300, 200], dtype=np.int64))),
            ('null samples with a frame', call(d_pcm=None)),
            ('null features with a frame', call(d_out=None))]


def test_argument_refusals_come_before_any_device_work():
    """No context, no device: every refusal is SPKD_EINVAL.  A null context is itself refused first,
    so this shows only that no case touches a device on its way out; the GPU test below, with a
    context, is the one that tells the refusals apart."""
    hipabi = pkg('hipabi')
    lib = hipabi.load_library()
    for name, call in _refusals():
        assert call(lib, None) == hipabi.SPKD_EINVAL, name


def test_frame_offsets_state_the_layout_on_the_host():
    fe = pkg('frontend')
    counts = [0, 100, 128, 1000, 1151, 0, 0, 129]
    off = np.concatenate([[0], np.cumsum(counts)])
    want, t = [0], 0
    for n in counts:
        t += n // HOP
        want.append(t)
    got = fe.frame_offsets(off, HOP)
    assert got.dtype == np.int64 and list(got) == want == [0, 0, 0, 1, 8, 16, 16, 16, 17]
    # the count is the file's own: 1151 samples are 8 frames wherever the file starts
    assert list(fe.frame_offsets([0, 5, 5 + 1151], HOP)) == [0, 0, 8]
    assert list(fe.frame_offsets([0], HOP)) == [0] and list(fe.frame_offsets([0, 0, 0], HOP)) == [0, 0, 0]


def test_pcm_entry_points_refuse_before_touching_the_context():
    fe, pipeline = pkg('frontend'), pkg('pipeline')
    cfg = _cfg(400)
    model = lambda rate, hop: types.SimpleNamespace(cfg=types.SimpleNamespace(sample_rate=rate, hop=hop))
    pcms = [np.zeros(4000, dtype=np.int16)]
    with pytest.raises(ValueError, match='Hz'):
        pipeline.diarize_pcm_batch(None, model(8000, cfg.hop), cfg, pcms)
    with pytest.raises(ValueError, match='frame'):
        pipeline.diarize_pcm_batch(None, model(cfg.sample_rate, 160), cfg, pcms)
    with pytest.raises(ValueError, match='one-dimensional'):
        fe.upload_batch(None, [np.zeros(10, dtype=np.int16), np.zeros((2, 5), dtype=np.int16)])
    with pytest.raises(ValueError, match='int16'):
        fe.upload_batch(None, [np.zeros(10, dtype=np.float32)])
    with pytest.raises(ValueError, match='int16 range'):
        fe.upload_batch(None, [np.array([0, 40000], dtype=np.int32)])
    with pytest.raises(ValueError, match='int16 range'):
        fe.upload_batch(None, [np.array([1, 65535], dtype=np.uint16)])


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def ctx():
    c = pkg('hipabi').Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def alone(ctx):
    """The border files and, per window width, spkd_mfcc's features of every file on its own."""
    fe = pkg('frontend')
    files = _border_files()
    return files, {w: [fe.extract(p, _cfg(w), ctx) for p in files] for w in (400, 256)}


def _batch(ctx, cfg, pcms):
    """extract_batch into a buffer with GUARD rows of a NaN pattern behind the features ->
    (features [sum T, 39], the guard rows as uint32, frame_off)."""
    fe = pkg('frontend')
    d_pcm, sample_off = fe.upload_batch(ctx, pcms)
    assert list(sample_off) == [0] + list(np.cumsum([len(p) for p in pcms]))
    total = int(fe.frame_offsets(sample_off, cfg.hop)[-1])
    buf = np.full((total + GUARD, cfg.dim), NAN_PATTERN, dtype=np.uint32)
    d_out = ctx.dev_scratch('test_mfcc_batch_out', buf.nbytes)
    ctx.h2d(d_out, buf)
    got_ptr, frame_off = fe.extract_batch(ctx, cfg, d_pcm, sample_off, d_out=d_out)
    assert got_ptr == d_out
    ctx.d2h(buf, d_out)
    return buf[:total].view(np.float32), buf[total:], frame_off


def _same_bits(feats, frame_off, want, order=None):
    order = range(len(want)) if order is None else order
    for slot, i in enumerate(order):
        got = feats[frame_off[slot]:frame_off[slot + 1]]
        assert got.shape == want[i].shape, (slot, i)
        diff = got.view(np.uint32) != want[i].view(np.uint32)
        assert not diff.any(), 'file %d (slot %d, %d frames): first differing frame %d' % (
            i, slot, len(got), int(np.argwhere(diff)[0][0]))


@pytest.mark.gpu
@pytest.mark.parametrize('window', [400, 256])
def test_every_file_of_a_batch_equals_the_file_alone_to_the_bit(ctx, alone, window):
    fe = pkg('frontend')
    files, want = alone
    cfg = _cfg(window)
    feats, guard, frame_off = _batch(ctx, cfg, files)
    assert frame_off.dtype == np.int64 and np.array_equal(frame_off, fe.frame_offsets(
        np.concatenate([[0], np.cumsum(LENGTHS)]), HOP))
    assert [int(n) for n in np.diff(frame_off)] == [n // HOP for n in LENGTHS]
    assert np.all(np.isfinite(feats))
    _same_bits(feats, frame_off, want[window])
    assert np.all(guard == NAN_PATTERN)                 # nothing written behind the last file
    # the loud and the quiet files do differ: the comparison above is not between look-alikes
    assert float(np.abs(want[window][7]).max()) > 0 and not np.array_equal(want[window][6][:8], want[window][9][:8])


@pytest.mark.gpu
@pytest.mark.parametrize('window', [400, 256])
def test_the_order_of_the_files_does_not_matter(ctx, alone, window):
    files, want = alone
    order = list(np.random.default_rng(4).permutation(len(files)))
    assert order != sorted(order)
    feats, guard, frame_off = _batch(ctx, _cfg(window), [files[i] for i in order])
    _same_bits(feats, frame_off, want[window], order)
    assert np.all(guard == NAN_PATTERN)


@pytest.mark.gpu
def test_a_batch_without_a_frame_launches_nothing(ctx):
    fe, hipabi = pkg('frontend'), pkg('hipabi')
    cfg = _cfg(400)
    tables = (fe.mel_filterbank(cfg.sample_rate), fe.dct_matrix(cfg.n_cep), cfg.mean, cfg.scale, cfg.transform)
    # null device pointers: a launch would have been refused (and a kernel would have faulted)
    for off in ([0], [0, 0], [0, 0, 100, 100, 227]):
        frame_off = ctx.mfcc_batch(0, off, fe.mfcc_params(cfg), *tables, 0)
        assert frame_off.dtype == np.int64 and list(frame_off) == [0] * len(off)
    d_pcm, sample_off = fe.upload_batch(ctx, [np.zeros(0, dtype=np.int16), np.ones(100, dtype=np.int16)])
    buf = np.full((GUARD, cfg.dim), NAN_PATTERN, dtype=np.uint32)
    d_out = ctx.dev_scratch('test_mfcc_batch_out', buf.nbytes)
    ctx.h2d(d_out, buf)
    _, frame_off = fe.extract_batch(ctx, cfg, d_pcm, sample_off, d_out=d_out)
    ctx.d2h(buf, d_out)
    assert list(frame_off) == [0, 0, 0] and np.all(buf == NAN_PATTERN)


@pytest.mark.gpu
def test_a_batch_matches_the_numpy_restatement(ctx):
    from oracle import mfcc_numpy as m
    cfg = _cfg(400)
    pcms = [_tone(seconds, seed=seed) for seconds, seed in ((0.9, 5), (2.1, 3), (1.3, 7))]
    feats, _, frame_off = _batch(ctx, cfg, pcms)
    for i, pcm in enumerate(pcms):
        want = m.features(pcm, cfg)
        got = feats[frame_off[i]:frame_off[i + 1]]
        assert got.shape == want.shape and np.all(np.isfinite(got))
        # tests/test_mfcc_reference.py's bound on this file (never above the former 2e-3 of the feature scale)
        r = full_chain_ratios(got, pcm, cfg)
        print('file %d: %d frames, device error / bound at most %.3f (column %d)' % (i, len(got), r.max(), r.argmax()))
        assert np.all(r <= 1.0), (i, int(r.argmax()), float(r.max()))
        assert full_chain_bound(pcm, cfg).max() < 2e-3 * max(1.0, float(np.abs(want).max()))


@pytest.mark.gpu
def test_refusals_on_a_context_name_their_reason_and_leave_it_usable(ctx, alone):
    hipabi = pkg('hipabi')
    for name, call in _refusals():
        assert call(ctx.lib, ctx.h) == hipabi.SPKD_EINVAL, name
        assert ctx.lib.spkd_last_error(ctx.h).decode() != '', name
    fe = pkg('frontend')
    cfg = _cfg(400)
    tables = (fe.mel_filterbank(cfg.sample_rate), fe.dct_matrix(cfg.n_cep), cfg.mean, cfg.scale, cfg.transform)
    with pytest.raises(hipabi.SpkdError, match='non-decreasing'):
        ctx.mfcc_batch(256, [0, 400, 300], fe.mfcc_params(cfg), *tables, 256)
    with pytest.raises(hipabi.SpkdError, match='start at 0'):
        ctx.mfcc_batch(256, [7, 400], fe.mfcc_params(cfg), *tables, 256)
    files, want = alone
    feats, guard, frame_off = _batch(ctx, cfg, files)
    _same_bits(feats, frame_off, want[400])
    assert np.all(guard == NAN_PATTERN)


@pytest.fixture(scope='module')
def model(tmp_path_factory):
    d = str(tmp_path_factory.mktemp('vad_model'))
    write_model(d, *_synthetic_mixtures(np.random.default_rng(11)))
    return load_model(d)


@pytest.mark.gpu
def test_one_upload_serves_the_vad_chain(ctx, model):
    fe, pipeline = pkg('frontend'), pkg('pipeline')
    pcms = [_signal(9.0, 41), np.zeros(0, dtype=np.int16), _signal(6.3, 43)[:-77]]
    want = pipeline.vad_batch(ctx, model, pcms)
    timings = {}
    got = pipeline.vad_batch(ctx, model, None, timings=timings, uploaded=fe.upload_batch(ctx, pcms))
    assert got == want and len(got) == 3 and got[1] == []
    assert any(len(t) > 0 for t in got)
    assert 'wall_upload' not in timings and len(timings['mfcc_static']) == len(timings['mfcc_post']) == 1


def _talk(seconds, seed, rate=16000):
    """Stretches of two harmonic voices (fundamentals 120 and 210 Hz) of 1.5 - 3 s with pauses of
    0.8 - 1.5 s between them, over low noise: several turns for the VAD, several speakers' worth of
    change points for the detector."""
    rng = np.random.default_rng(seed)
    t = np.arange(int(seconds * rate)) / rate
    x = 200 * rng.standard_normal(len(t))
    at, voice = 0.7, 0
    while at < seconds - 1.0:
        length = rng.uniform(1.5, 3.0)
        on = (t > at) & (t < min(at + length, seconds - 0.5))
        f0 = (120.0, 210.0)[voice]
        x += on * sum(2000 / h * np.sin(2 * np.pi * f0 * h * t) for h in range(1, 8))
        at += length + rng.uniform(0.8, 1.5)
        voice = 1 - voice
    return np.clip(x, -32768, 32767).astype(np.int16)


# (seconds, seed): with this module's VAD model each gives several turns, none under 40 frames (whose
# covariance would be singular); the test asserts the counts it needs
TALKS = ((23.0, 114), (27.0, 146), (25.0, 133))


@pytest.mark.gpu
def test_samples_to_speakers_equals_the_stages_fed_by_hand(ctx, model):
    fe, pipeline = pkg('frontend'), pkg('pipeline')
    cfg = _cfg(400)
    pcms = [_talk(seconds, seed) for seconds, seed in TALKS]
    timings = {}
    rows = pipeline.diarize_pcm_batch(ctx, model, cfg, pcms, timings=timings)
    assert len(timings['wall_upload']) == 1 and len(timings['mfcc_static']) == len(timings['mfcc_post']) == 2
    # by hand: the turns of vad_batch, and every file's own features copied into one array
    vad = pipeline.vad_batch(ctx, model, pcms)
    counts = [len(p) // cfg.hop for p in pcms]
    off = np.concatenate([[0], np.cumsum(counts)])
    d_all = ctx.dev_alloc(int(off[-1]) * cfg.dim * 4)
    try:
        for p, o in zip(pcms, off):
            d_one, T = fe.extract_device(p, cfg, ctx)
            try:
                ctx.copy_d2d(d_all + int(o) * cfg.dim * 4, d_one, T * cfg.dim * 4)
            finally:
                ctx.dev_free(d_one)
        files = [pipeline.BatchFile(o, T, v) for o, T, v in zip(off, counts, vad)]
        want = pipeline.diarize_batch(ctx, d_all, int(off[-1]), files, rate=float(cfg.frame_rate))
    finally:
        ctx.dev_free(d_all)
    print('turns per file:', [len(v) for v in vad], 'segments per file:', [len(r) for r in want],
          'speakers per file:', [len(set(r[:, 2])) if len(r) else 0 for r in want])
    assert all(len(v) >= 2 for v in vad) and all(len(r) >= 4 for r in want)      # the signal gives the stages work
    assert len(rows) == len(want) == 3
    for got, ref in zip(rows, want):
        assert got.shape == ref.shape and np.all(got == ref)
