"""The delay stream (include/spkd.h (6b3); frontend.DelayStream; reseg['tdoa']): the beamformer's per-step delays
kept for a whole batch and used as a second stream of the resegmentation stage, against the restatement of
tests/tdoa_numpy.py.

What is compared how:
  the step rule   exactly, against a walk over the steps in Python integers, at four input rates;
  pack            exactly: the stream a batch leaves is beamform_batch(detail=)'s reliable mask, its delays where
                  they are reliable (an unreliable entry holds no delay) and its reference channels, in one group
                  and in several;
  statistics      exactly, against Python integers summed frame by frame;
  models          mean, variance and 1 / (2 var) to the bit against numpy float64 in the stated order; the log
                  term, which goes through the device's log, within 4 ulp of float64;
  scores          every finite entry within one float32 ulp of the 50-digit value rounded once: the fp64 path's
                  error (a few 2^-53 of a sum of a few thousand) is many orders below half a float32 ulp of the
                  result, so the device gives the correctly rounded value or its neighbour.  The share of entries
                  that differ at all goes to profiles/tdoa_accuracy.json, not asserted;
  end to end      two speakers with one acoustic model and two seats: with RESEG_TDOA every boundary lies within
                  32 frames (one step of 31.25, rounded up) of the true one, with RESEG at least one does not; the
                  device decodes the restatement's tokens, whose decisions the CPU test shows to be no ties."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest

import beamform_numpy as B
import reseg_numpy as R
import tdoa_numpy as TD
from conftest import pkg
from helpers import ROOT
from reseg_helpers import RATE, Batch, close_session, displaced, normal_scores
from test_reseg_batch import _StubContext

HOP, WINDOW, RATE_OUT = 128, 400, 16000
CLOCK = (HOP, WINDOW, RATE_OUT)
NAMES = ('spkd_tdoa_pack', 'spkd_tdoa_stats', 'spkd_tdoa_models', 'spkd_tdoa_score')
PROFILE = os.path.join(ROOT, 'profiles', 'tdoa_accuracy.json')
SEAT_A, SEAT_B = (0, 37, -160, 5), (0, -12, 90, 5)
E2E_SEED, E2E_SECONDS, E2E_STREAM_SEED = 2026, 60.0, 7
NEAR = 32                                       # frames: one step of 31.25, rounded up


def _note(key, value):
    """profiles/tdoa_accuracy.json gains one key: the figures, beside what the tests assert of them."""
    try:
        try:
            rec = json.load(open(PROFILE))
        except (OSError, ValueError):
            rec = {}
        rec['what'] = ('written by tests/test_tdoa_stream.py: the share of score entries on which '
                       'spkd_tdoa_score and the 50-digit value rounded once to float32 differ, and the worst distance '
                       'of a decoded boundary from the true one, end to end, for the numpy restatement and the device')
        rec[key] = value
        with open(PROFILE, 'w') as f:
            f.write(json.dumps(rec, indent=1, sort_keys=True) + '\n')
    except OSError:
        pass                                    # (a read-only checkout: the figures are printed)


class _FakeDevice(object):
    """A context for a DelayStream that is never read: hands out an address and keeps what goes up."""

    def __init__(self):
        self.up = []

    def dev_scratch(self, name, nbytes):
        return 1 << 22

    def h2d(self, dptr, arr):
        self.up.append((dptr, np.array(arr)))


def _file(delay, reliable, ref, H, rate_in, frame0=0):
    return dict(delay=np.asarray(delay, dtype=np.int32), reliable=np.asarray(reliable, dtype=bool), ref=ref, H=H,
                rate_in=rate_in, frame0=frame0)


def _stream(ctx, files):
    fe = pkg('frontend')
    return fe.DelayStream.from_arrays(ctx, HOP, WINDOW, [(f['delay'], f['reliable'], f['ref'], f['H'], f['rate_in']) for f in files],
                                      rate_out=RATE_OUT)


# ------------------------------------------------------------------ not GPU
def test_entry_points_and_timers_are_declared_exported_and_bound():
    hipabi = pkg('hipabi')
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'spkd.h')).read(), flags=re.S)
    lib = hipabi.load_library()
    for name in NAMES:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in hipabi.EXPORTS and hasattr(lib, name), name
        assert hasattr(hipabi.Context, name[len('spkd_'):]), name
    assert 'spkd_*' in open(os.path.join(ROOT, 'speaker-diarization_amd', 'csrc', 'libspkd_hip.map')).read()
    names = [n for n, _ in sorted(hipabi.TIMERS.items(), key=lambda kv: kv[1])]
    enum = re.search(r'enum \{\s*SPKD_T_CALL = 0,(.*?)SPKD_N_TIMERS', code, flags=re.S).group(1)
    assert ['call'] + [n.strip()[len('SPKD_T_'):].lower() for n in enum.split(',') if n.strip()] == names
    at = names.index('tdoa_pack')
    assert names[at:at + 4] == ['tdoa_pack', 'tdoa_stats', 'tdoa_models', 'tdoa_score'] and len(names) == len(set(names))
    for define, value in (('NONE', 'INT32_MIN'), ('MAX_CH', hipabi.TDOA_MAX_CH), ('MAX_DELAY', hipabi.TDOA_MAX_DELAY),
                          ('FILE', hipabi.TDOA_FILE), ('MODEL', hipabi.TDOA_MODEL), ('TILE', hipabi.TDOA_TILE)):
        assert re.search(r'#define SPKD_TDOA_%s %s\b' % (define, value), code), define
    assert hipabi.TDOA_NONE == -(1 << 31) == TD.NONE and lib.spkd_abi_version() == 2
    mk = open(os.path.join(ROOT, 'speaker-diarization_amd', 'csrc', 'Makefile')).read()
    assert 'spkd_tdoa.hpp' in re.search(r'^HDR := (.*)$', mk, flags=re.M).group(1)
    pipeline = pkg('pipeline')
    assert pipeline.TDOA == dict(weight=1.0, floor_s=1.0 / 16000.0, min_frames=40)
    assert pipeline.RESEG_TDOA == dict(penalty=50.0, tdoa=pipeline.TDOA)


@pytest.mark.parametrize('rate_in', [8000, 16000, 44100, 48000])
def test_the_step_rule_is_the_walk_over_the_steps(rate_in):
    fe = pkg('frontend')
    H = fe.beamform_geometry(rate_in)[0]                            # a quarter of a second at the input rate
    T = 9
    f = _file(np.zeros((T, 2)), np.ones((T, 2)), 0, H, rate_in)
    last = 0
    for t in range(0, 400):
        want = TD.step_brute(t, CLOCK, f)
        assert TD.step(t, CLOCK, f) == want == fe.frame_step(t, HOP, WINDOW, rate_in, RATE_OUT, H, T), t
        assert want - last in (0, 1)
        last = want
    assert last == T - 1 and TD.step(10 ** 9, CLOCK, f) == T - 1    # the clamp
    # the inverse: a step's first frame is on the step, the frame before is not; frame 0 opens step 0
    for s in range(1, T):
        t0 = fe.step_first_frame(s, HOP, WINDOW, rate_in, RATE_OUT, H)
        assert TD.step_brute(t0, CLOCK, f) == s and TD.step_brute(t0 - 1, CLOCK, f) == s - 1, s
    assert fe.step_first_frame(0, HOP, WINDOW, rate_in, RATE_OUT, H) == 0
    # a frame whose window's centre is a step's first sample exactly: hop 125, window 250, 16 kHz, H 4000: frame 31
    g = _file(np.zeros((3, 2)), np.ones((3, 2)), 0, 4000, 16000)
    assert (31 * 125 + 125) * 16000 == 1 * 16000 * 4000
    assert TD.step(31, (125, 250, 16000), g) == TD.step_brute(31, (125, 250, 16000), g) == 1
    assert TD.step(30, (125, 250, 16000), g) == 0 and fe.step_first_frame(1, 125, 250, 16000, 16000, 4000) == 31


def test_from_arrays_packs_and_refuses():
    fe, hipabi = pkg('frontend'), pkg('hipabi')
    rng = np.random.default_rng(3)
    d0, r0 = rng.integers(-4096, 4097, (5, 3)), rng.random((5, 3)) < 0.7
    d1, r1 = rng.integers(-50, 50, (2, 8)), rng.random((2, 8)) < 0.5
    dev = _FakeDevice()
    s = fe.DelayStream.from_arrays(dev, HOP, WINDOW, [(d0, r0, 1, 4000, 16000), (np.zeros((0, 1), int), np.zeros((0, 1), bool), 0, 4000, 16000),
                                                      (d1, r1, 7, 12000, 48000)])
    assert s.n_files == 3 and s.n_entries == 15 + 16 and len(dev.up) == 1 and dev.up[0][0] == s.d_stream
    want = np.concatenate([np.where(r0, d0, TD.NONE).ravel(), np.where(r1, d1, TD.NONE).ravel()]).astype(np.int32)
    assert dev.up[0][1].dtype == np.int32 and np.array_equal(dev.up[0][1], want)
    assert s.files.tolist() == [[0, 5, 3, 1, 4000, 16000], [15, 0, 1, 0, 4000, 16000], [15, 2, 8, 7, 12000, 48000]]
    assert s.table([0, 100, 100]).tolist() == [[0, 5, 3, 1, 4000, 16000, 0, 0], [15, 0, 1, 0, 4000, 16000, 100, 0],
                                               [15, 2, 8, 7, 12000, 48000, 100, 0]]
    assert s.step_of(2, 40) == TD.step(40, CLOCK, _file(d1, r1, 7, 12000, 48000))
    ok = (np.zeros((2, 2), np.int32), np.ones((2, 2), bool), 0, 4000, 16000)
    for bad, word in (((ok[0], np.ones((2, 3), bool)) + ok[2:], 'expected'), ((ok[0].astype(float),) + ok[1:], 'expected'),
                      ((np.zeros((2, 9), int), np.ones((2, 9), bool)) + ok[2:], 'channels'),
                      (ok[:2] + (2,) + ok[3:], 'reference channel'), (ok[:3] + (0, 16000), 'step'),
                      ((np.full((2, 2), 4097), ok[1]) + ok[2:], 'beyond'), (ok[:3] + (100, 16000), 'shorter than a feature frame'),
                      ((np.zeros((2, 1), int), np.ones((2, 1), bool)) + ok[2:], 'one-channel')):
        with pytest.raises(ValueError, match=word):
            fe.DelayStream.from_arrays(_FakeDevice(), HOP, WINDOW, [bad])
    # a delay beyond the limit on an entry that is not reliable is no delay
    fe.DelayStream.from_arrays(_FakeDevice(), HOP, WINDOW, [(np.full((2, 2), 9999), np.zeros((2, 2), bool), 0, 4000, 16000)])
    with pytest.raises(ValueError, match='hop'):
        fe.DelayStream(None, 0, WINDOW)
    # a context holds one stream at a time: the older one says so instead of reading a buffer that is no longer its
    later = fe.DelayStream.from_arrays(dev, HOP, WINDOW, [ok])
    for stale in (lambda: s.handle([0, 100, 100]), s.to_host):
        with pytest.raises(ValueError, match='a later stream'):
            stale()
    assert later.handle([0])[1] == 4
    assert hipabi.TDOA_NONE == np.iinfo(np.int32).min


class _NoDevice(object):
    """A context that records every call: the refusals below must leave it empty."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append(name)
            raise AssertionError('device work before the refusal: ' + name)
        return call


def _small_batch():
    pipeline = pkg('pipeline')
    files = [pipeline.BatchFile(0, 1000, [(1.0, 3.0)]), pipeline.BatchFile(1000, 1000, [(0.5, 6.0)])]
    labels = [np.array([1, 2]), np.array([1, 2, 1])]
    segments = [np.array([(1.0, 2.0), (2.0, 3.0)]), np.array([(0.5, 2.0), (2.0, 4.0), (4.0, 6.0)])]
    return files, labels, [0, 2, 5], segments


def test_every_value_error_comes_before_any_device_work():
    pipeline, fe = pkg('pipeline'), pkg('frontend')
    files, labels, seg_off, segments = _small_batch()
    two = [(np.zeros((3, 2), np.int32), np.ones((3, 2), bool), 0, 4000, 16000)] * 2
    stream = fe.DelayStream.from_arrays(_FakeDevice(), HOP, WINDOW, two)
    ctx = _NoDevice()

    def run(reseg, delays=stream, segs=segments, rate=125.0, fl=files):
        return pipeline.resegment_batch(ctx, 1 << 20, 2000, fl, 1 << 21, seg_off, labels, rate, reseg, False, None, {}, segs,
                                        delays)

    T = pipeline.TDOA
    cases = [(dict(penalty=50.0, tdoa=T), dict(delays=None), 'delays='),
             (dict(penalty=50.0, tdoa=T), dict(delays=fe.DelayStream.from_arrays(_FakeDevice(), HOP, WINDOW, two[:1])), 'a batch of 2'),
             (dict(penalty=50.0, tdoa=T), dict(delays=fe.DelayStream.from_arrays(_FakeDevice(), 160, WINDOW, two)), 'frames a second'),
             (dict(penalty=50.0, tdoa=T), dict(rate=100.0), 'frames a second'),
             (dict(penalty=50.0, tdoa=T), dict(segs=None), 'segments'),
             (dict(penalty=50.0, tdoa=dict(T, gain=2.0)), {}, 'keys of TDOA'), (dict(penalty=50.0, tdoa=[1.0]), {}, 'keys of TDOA'),
             (dict(penalty=50.0, tdoa=dict(T, weight=-1.0)), {}, 'tdoa weight'),
             (dict(penalty=50.0, tdoa=dict(T, weight=float('nan'))), {}, 'tdoa weight'),
             (dict(penalty=50.0, tdoa=dict(T, weight=float('inf'))), {}, 'tdoa weight'),
             (dict(penalty=50.0, tdoa=dict(T, weight='much')), {}, 'tdoa weight'),
             (dict(penalty=50.0, tdoa=dict(T, floor_s=0.0)), {}, 'tdoa floor_s'),
             (dict(penalty=50.0, tdoa=dict(T, floor_s=float('inf'))), {}, 'tdoa floor_s'),
             (dict(penalty=50.0, tdoa=dict(T, floor_s=float('nan'))), {}, 'tdoa floor_s'),
             (dict(penalty=50.0, tdoa=dict(T, min_frames=0)), {}, 'tdoa min_frames'),
             (dict(penalty=50.0, tdoa=dict(T, min_frames=2.5)), {}, 'tdoa min_frames'),
             (dict(penalty=50.0, tdoa=dict(T, min_frames=True)), {}, 'tdoa min_frames')]
    for reseg, kw, word in cases:
        with pytest.raises(ValueError, match=word):
            run(reseg, **kw)
    # and through diarize_batch, before change detection
    for reseg, kw, word in cases[:2] + cases[5:8]:
        with pytest.raises(ValueError, match=word):
            pipeline.diarize_batch(ctx, 1 << 20, 2000, files, reseg=reseg, detail={}, delays=kw.get('delays', stream))
    assert ctx.calls == []
    # the keys are optional, the defaults are TDOA's; with every other option of a reseg dictionary
    opts = pkg('resegmentation')._reseg_options
    assert opts(dict(penalty=1.0, tdoa={}), 125.0, None).tdoa == (1.0, 1.0 / 16000.0, 40)
    assert opts(dict(penalty=1.0, tdoa=dict(weight=0, min_frames=7)), 125.0, None).tdoa == (0.0, 1.0 / 16000.0, 7)
    assert opts(dict(pipeline.RESEG_GMM, min_dur_s=1.0, passes=3, confidence=True, tdoa=T), 125.0, {}).tdoa == (1.0, 1.0 / 16000.0, 40)
    assert opts(dict(pipeline.RESEG_SOFT, tdoa=T), 125.0, None).tdoa and opts(pipeline.RESEG, 125.0, None).tdoa is None
    # the audio entry point: tdoa takes the beamformer, and a stream only goes with it
    with pytest.raises(ValueError, match='beamform='):
        pipeline.diarize_audio_batch(ctx, dict(pkg('self_vad').SELF_VAD), None, [], reseg=pipeline.RESEG_TDOA)
    with pytest.raises(ValueError, match='beamform='):
        fe.resample_batch(ctx, [], 16000, delays=stream)
    with pytest.raises(ValueError, match='8000 Hz'):
        fe.resample_batch(ctx, [], 8000, beamform=pipeline.BEAMFORM, delays=stream)
    with pytest.raises(ValueError, match='does not resample'):
        fe.beamform_batch(ctx, [(np.zeros((10, 2), np.int16), 48000)], pipeline.BEAMFORM, delays=stream)
    assert ctx.calls == []


def test_a_reseg_without_tdoa_asks_for_exactly_todays_calls():
    pipeline, fe = pkg('pipeline'), pkg('frontend')
    files = [pipeline.BatchFile(0, 1000, [(1.0, 3.0), (9.0, 9.5)]), pipeline.BatchFile(1000, 500, [(0.0, 2.0)]),
             pipeline.BatchFile(1500, 1000, [(0.5, 6.0)])]
    labels = [np.array([5, 2, 5]), np.zeros(0, dtype=np.int32), np.array([3, 1, 2, 1])]
    tokens = [[(0, 1), (100, 0)], [], [(0, 2), (7, 0), (300, 2)]]
    stream = fe.DelayStream.from_arrays(_FakeDevice(), HOP, WINDOW, [(np.zeros((3, 2), np.int32), np.ones((3, 2), bool), 0, 4000, 16000)] * 3)
    got = []
    for kw in ({}, dict(delays=stream), dict(delays=None)):
        stub = _StubContext([1, 1, 1, 0, 1], tokens)
        det = {}
        rows = pipeline.resegment_batch(stub, 1 << 20, 2500, files, 1 << 21, [0, 3, 3, 7], labels, 125.0, dict(penalty=7.0), False,
                                        None, det, **kw)
        assert [c[0] for c in stub.calls] == ['dev_scratch', 'sum_stats', 'dev_scratch', 'gauss_models', 'dev_scratch',
                                              'gauss_loglik', 'vad_viterbi_batch']
        assert 'tdoa_channels' not in det
        got.append((stub.calls, [r.tobytes() for r in rows]))
    assert got[0] == got[1] == got[2]


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def ctx():
    c = pkg('hipabi').Context(0)
    yield c
    c.close()


def _pack_batch():
    rng = np.random.default_rng(8)
    mono = np.clip(np.rint(3000.0 * rng.standard_normal(9000)), -32768, 32767).astype(np.int16)
    return [(B.scene('S2')['x'], 16000), (mono, 16000), (B.scene('S4')['x'], 16000), (np.zeros((0, 2), np.int16), 16000),
            (B.scene('S5')['x'], 16000)]


@pytest.mark.gpu
def test_the_stream_a_batch_leaves_is_the_beamformers_detail_in_one_group_and_in_several(ctx):
    fe, pipeline = pkg('frontend'), pkg('pipeline')
    audios = _pack_batch()
    detail, timings = {}, {}
    stream = fe.DelayStream(ctx, HOP, WINDOW, RATE_OUT)
    fe.beamform_batch(ctx, audios, pipeline.BEAMFORM, timings=timings, detail=detail, delays=stream)
    assert len(timings['tdoa_pack']) == 1 and timings['tdoa_pack'][0] > 0
    assert [d.shape for d in detail['delay']] == [(11, 4), (0, 1), (11, 2), (1, 2), (1, 3)]     # (an empty file of two channels has its one step)
    assert not all(r.all() for r in detail['reliable']) and any(r.any() for r in detail['reliable'])

    def same(s):
        assert s.files[:, 1:3].tolist() == [list(d.shape) for d in detail['delay']]
        assert s.files[:, 4].tolist() == [4000] * 5 and s.files[:, 5].tolist() == [16000] * 5
        for f, (delay, reliable) in enumerate(s.to_host()):
            assert np.array_equal(reliable, detail['reliable'][f]), f
            assert np.array_equal(delay, np.where(reliable, detail['delay'][f], 0)), f
            if delay.shape[1] > 1 and delay.shape[0]:
                assert int(s.files[f, 3]) == detail['ref'][f], f
    same(stream)
    one = stream.to_host()
    for group_bytes in (1 << 28, 200000, 1):
        s = fe.DelayStream(ctx, HOP, WINDOW, RATE_OUT)
        t = {}
        fe.resample_batch(ctx, audios, 16000, group_bytes=group_bytes, beamform=pipeline.BEAMFORM, delays=s, timings=t)
        same(s)
        assert len(t['tdoa_pack']) == 1
        assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(one, s.to_host()))
    # without delays= the calls take the path they took: no timing of the new kernel
    t = {}
    fe.resample_batch(ctx, audios, 16000, beamform=pipeline.BEAMFORM, timings=t)
    assert 'tdoa_pack' not in t


def _stat_files():
    """A 2-channel file of 300 steps at 16 kHz, an 8-channel file at 48 kHz, a one-channel file and a 3-channel file
    at 44.1 kHz, each at its place of the batch's frames."""
    rng = np.random.default_rng(12)
    fe = pkg('frontend')
    out = []
    for (T, Cn, rate, ref), frame0 in zip(((300, 2, 16000, 0), (80, 8, 48000, 3), (0, 1, 16000, 0), (7, 3, 44100, 2)),
                                          (0, 9500, 12100, 12100)):
        d = rng.integers(-4096, 4097, (T, Cn))
        r = rng.random((T, Cn)) < 0.8
        if T:
            d[0], d[-1] = 4096, -4096
            r[0], r[-1] = True, True
        if Cn == 8:
            r[:, 5] = False                              # a channel unreliable everywhere
        out.append(_file(d, r, ref, fe.beamform_geometry(rate)[0], rate, frame0))
    return out


def _first(f, s):
    return pkg('frontend').step_first_frame(s, HOP, WINDOW, f['rate_in'], RATE_OUT, f['H']) + f['frame0']


@pytest.mark.gpu
def test_statistics_are_exact(ctx):
    files = _stat_files()
    f0, f1, _, f3 = files
    rng = np.random.default_rng(5)
    many = sorted(int(v) for v in rng.integers(0, 9300, 120))
    ranges = ([(40, 50, 0, 0),                                              # inside one step
               (_first(f0, 3), _first(f0, 5), 0, 0),                         # from a step's first frame to a step's first frame
               (_first(f0, 7), _first(f0, 7) + 1, 0, 0), (_first(f0, 9) - 1, _first(f0, 9), 0, 0),
               (_first(f0, 298), _first(f0, 299) + 500, 0, 1),               # past the last step: the clamp
               (0, 9400, 0, 2),                                              # more than 256 steps
               (_first(f0, 10) + 3, _first(f0, 80) + 5, 0, 3),               # more than 64 steps
               (700, 700, 0, 3),                                             # empty
               # set 4 has no range
               (9500 + 100, 9500 + 900, 1, 5), (100, 2000, 0, 5),            # two rates, 8 and 2 channels in one set
               (12100, 12100 + 300, 3, 6), (12100 + 5, 12100 + 6, 3, 6),
               (12100, 12200, 2, 7)]                                         # the one-channel file
              + [(a, a + 1 + (a % 70), 0, 8) for a in many])                 # many ranges of one set
    n_sets = 10
    want = TD.moments(files, CLOCK, ranges, n_sets)
    assert want[4] == [[0, 0, 0]] * 8 and want[7] == [[0, 0, 0]] * 8 and want[9] == [[0, 0, 0]] * 8
    assert want[5][5] == [0, 0, 0] and want[5][3] == [0, 0, 0] and want[5][7][0] > 0 and want[2][1][0] > 6000
    stream = _stream(ctx, files)
    handle = stream.handle([f['frame0'] for f in files])
    d_stats = ctx.dev_alloc(n_sets * 8 * 3 * 8)
    try:
        for _ in range(2):                                                   # and the same bits again
            ctx.h2d(d_stats, np.full(n_sets * 24, -7, dtype=np.int64))       # the call clears what it finds
            b, e, fi, st = (np.array(v) for v in zip(*ranges))
            ctx.tdoa_stats(handle, b, e, fi, st, n_sets, d_stats)
            got = np.zeros((n_sets, 8, 3), dtype=np.int64)
            ctx.d2h(got, d_stats)
            assert got.tolist() == want
        assert ctx.last_ms('tdoa_stats') > 0
        # refusals on a context: the statistics stay what they were
        hipabi = pkg('hipabi')
        for bad, word in (((b, e, fi, st[::-1].copy()), 'ascending'), ((b, e, fi + 4, st), 'file index'), ((e, b, fi, st), 'frame range'),
                          ((b - 20000, e, fi, st), 'frame range')):
            with pytest.raises(hipabi.SpkdError, match=word):
                ctx.tdoa_stats(handle, *bad, n_sets, d_stats)
        with pytest.raises(hipabi.SpkdError, match='2\\^31 frames'):
            ctx.tdoa_stats(handle, [0, 0], [1 << 30, 1 << 30], [0, 0], [0, 0], 1, d_stats)
        short = (handle[0], handle[1] - 1) + handle[2:]
        with pytest.raises(hipabi.SpkdError, match='outside the stream'):
            ctx.tdoa_stats(short, b, e, fi, st, n_sets, d_stats)
        again = np.zeros((n_sets, 8, 3), dtype=np.int64)
        ctx.d2h(again, d_stats)
        assert again.tolist() == want
    finally:
        ctx.dev_free(d_stats)


def _model_cases():
    """-> (stats int64 [n, 8, 3], spk_file, ok, files, min_frames, floor_s).  File 0, 4 channels, reference 0, 16 kHz:
    speakers 0 .. 3; file 1, 3 channels, reference 1, 48 kHz: speakers 4, 5; file 2, one channel: speaker 6; file 3, 2
    channels: nobody."""
    z = lambda T, Cn: (np.zeros((T, Cn)), np.ones((T, Cn)))
    files = [_file(*z(2, 4), 0, 4000, 16000), _file(*z(2, 3), 1, 12000, 48000), _file(*z(0, 1), 0, 4000, 16000),
             _file(*z(2, 2), 1, 4000, 16000)]
    mom = lambda xs: [len(xs), sum(xs), sum(x * x for x in xs)]
    st = np.zeros((7, 8, 3), dtype=np.int64)
    rng = np.random.default_rng(9)
    st[0, 1] = mom([37] * 500)                                               # constant: variance 0, the floor
    st[0, 2] = mom([4095, 4096] * 300 + [4096] * 7)                          # a mean near 4096, a variance near the floor
    st[0, 3] = mom([int(v) for v in rng.integers(-4096, 4097, 1000)])
    st[1, 1] = mom([-4096] * 39)                                             # min_frames - 1: not ok, and speaker 1 is ok
    st[1, 2] = mom([5, 6] * 20)                                              # min_frames
    st[1, 3] = mom([int(v) for v in rng.integers(-3, 4, 2000)])
    st[2, 1] = mom([1] * 50)
    st[2, 2] = mom([1] * 10)                                                 # lacks channel 2, but is acoustically not ok
    st[2, 3] = mom([-7, 9] * 100)
    st[3, 1] = mom([4093] * 100 + [4096] * 100)                               # variance 2.25 from two sums near 2^24: the cancellation
    st[3, 2], st[3, 3] = mom([0] * 41), [1 << 20, 1 << 32, 1 << 44]          # 2^20 frames at 4096
    st[4, 0], st[4, 2] = mom([8, 9] * 100), mom([-1, 1] * 30)                # 48 kHz: the floor is 9 samples^2
    st[5, 0], st[5, 2] = mom([100, -100] * 100), mom([-1] * 39)              # speaker 5 lacks channel 2: dropped for file 1
    st[6, 0] = mom([1] * 100)                                                # a one-channel file: nothing
    return st, [0, 0, 0, 0, 1, 1, 2], [1, 1, 0, 1, 1, 1, 1], files, 40, 1.0 / 16000.0


@pytest.mark.gpu
def test_models_equal_the_restatement_to_the_bit(ctx):
    st, spk_file, ok, files, min_frames, floor_s = _model_cases()
    want, live = TD.models(st.tolist(), spk_file, ok, files, min_frames, floor_s)
    assert live == [0b1100, 0b001, 0, 0b01]                                  # channel 1 of file 0 falls to speaker 1, not channel 2
    assert want[0, 1, 1] == 1.0 and want[0, 2, 1] == 1.0 and want[4, 0, 1] == 9.0 and 0.2 < want[0, 2, 0] - 4095 < 0.8
    assert want[1, 1].tolist() == [0.0, 1.0, 0.0, 0.0]
    stream = _stream(ctx, files)
    d_stats, d_models = ctx.dev_alloc(st.nbytes), ctx.dev_alloc(7 * 8 * 4 * 8)
    try:
        ctx.h2d(d_stats, st)
        got_live = ctx.tdoa_models(d_stats, spk_file, ok, stream.table([0, 0, 0, 0]), min_frames, floor_s, d_models)
        got = np.zeros((7, 8, 4))
        ctx.d2h(got, d_models)
        assert got_live.tolist() == live
        assert got[:, :, :3].tobytes() == want[:, :, :3].tobytes()           # mean, variance, 1 / (2 var)
        ln = np.abs(got[:, :, 3] - want[:, :, 3])
        assert (ln <= 4 * np.spacing(np.abs(want[:, :, 3]))).all()
        # everybody acoustically ok: speaker 2 now costs file 0 its channel 2 as well
        assert ctx.tdoa_models(d_stats, spk_file, [1] * 7, stream.table([0, 0, 0, 0]), min_frames, floor_s, d_models).tolist() == \
            [0b1000, 0b001, 0, 0b01]
        assert TD.models(st.tolist(), spk_file, [1] * 7, files, min_frames, floor_s)[1] == [0b1000, 0b001, 0, 0b01]
        hipabi = pkg('hipabi')
        for kw, word in ((dict(min_frames=0), 'min_frames'), (dict(floor_s=0.0), 'floor_s'), (dict(spk_file=[0, 1, 0, 0, 1, 1, 2]), 'ascending')):
            a = dict(dict(spk_file=spk_file, min_frames=min_frames, floor_s=floor_s), **kw)
            with pytest.raises(hipabi.SpkdError, match=word):
                ctx.tdoa_models(d_stats, a['spk_file'], ok, stream.table([0, 0, 0, 0]), a['min_frames'], a['floor_s'], d_models)
    finally:
        ctx.dev_free(d_stats)
        ctx.dev_free(d_models)


def _score_case(n_cols):
    """Files, live masks, models and planted scores for one call: file 0 (4 channels, 16 kHz, 40 steps) has turns of 1,
    31, 32 and 700 frames and one across a step border; file 1 (8 channels, 48 kHz) one of 300; file 2 (2 channels) has
    no live channel; file 3 is a one-channel file."""
    rng = np.random.default_rng(100 + n_cols)
    fe = pkg('frontend')
    mk = lambda T, Cn: (rng.integers(-200, 201, (T, Cn)), rng.random((T, Cn)) < 0.85)
    files = [_file(*mk(40, 4), 0, 4000, 16000, 0), _file(*mk(12, 8), 2, 12000, 48000, 2000), _file(*mk(10, 2), 0, 4000, 16000, 3000),
             _file(np.zeros((0, 1)), np.zeros((0, 1)), 0, 4000, 16000, 4000)]
    live = [0b1010, 0b11111011 & ~(1 << 6), 0, 0]
    border = fe.step_first_frame(5, HOP, WINDOW, 16000, RATE_OUT, 4000)
    n_spk = [min(n_cols, 3), n_cols, min(n_cols, 2), 1]
    first = np.concatenate([[0], np.cumsum(n_spk)])
    seqs = [(0, 10, 11), (0, 20, 51), (0, 60, 92), (0, 100, 800), (0, border - 2, border + 3), (1, 2010, 2310), (2, 3000, 3100),
            (3, 4000, 4050)]
    n_models = int(first[-1])
    mods = np.zeros((n_models, 8, 4))
    mods[:, :, 0] = rng.normal(0.0, 150.0, (n_models, 8))
    mods[:, :, 1] = rng.uniform(1.0, 400.0, (n_models, 8))
    mods[:, :, 2] = 1.0 / (2.0 * mods[:, :, 1])
    mods[:, :, 3] = -0.5 * np.log(TD.TWO_PI * mods[:, :, 1])
    scores = [normal_scores(rng, e - b, n_cols) for _, b, e in seqs]
    return files, live, seqs, first, n_spk, mods, scores


@pytest.mark.gpu
@pytest.mark.parametrize('n_cols', [1, 2, 3, 16])
def test_scores_are_within_an_ulp_of_the_exact_value_rounded_once(ctx, n_cols):
    files, live, seqs, first, n_spk, mods, scores = _score_case(n_cols)
    weight = 0.75
    stream = _stream(ctx, files)
    handle = stream.handle([f['frame0'] for f in files])
    flat = np.concatenate(scores)
    guard = np.full((3, n_cols), 123.5, dtype=np.float32)
    host = np.concatenate([guard, flat, guard])                              # (the scores start 3 rows in: off a 16-byte border for odd n_cols)
    d_scores, d_models = ctx.dev_alloc(host.nbytes), ctx.dev_alloc(mods.nbytes)
    try:
        ctx.h2d(d_scores, host)
        ctx.h2d(d_models, mods)
        fi, b, e = (np.array(v) for v in zip(*seqs))
        ctx.tdoa_score(handle, d_models, len(mods), live, b, e, fi, first[fi], np.array(n_spk)[fi], n_cols, weight,
                       d_scores + 3 * n_cols * 4)
        got = np.zeros_like(host)
        ctx.d2h(got, d_scores)
        assert got[:3].tobytes() == guard.tobytes() and got[-3:].tobytes() == guard.tobytes()
        got = got[3:-3]
        worst, differ, finite, row = 0, 0, 0, 0
        for (f, b0, e0), sc in zip(seqs, scores):
            g = got[row:row + len(sc)]
            row += len(sc)
            k = n_spk[f]
            assert g[:, k:].tobytes() == sc[:, k:].tobytes()                 # the columns past the file's speakers
            if not live[f]:
                assert g.tobytes() == sc.tobytes()                           # no live channel, one channel: untouched
                continue
            for t in range(len(sc)):
                for j in range(k):
                    if not np.isfinite(sc[t, j]):
                        assert g[t, j:j + 1].tobytes() == sc[t, j:j + 1].tobytes()
                        continue
                    want = TD.score_exact(sc[t, j], files[f], CLOCK, live[f], b0 + t, mods[first[f] + j], weight)
                    d = TD.ulps(g[t, j], want)
                    worst, differ, finite = max(worst, d), differ + (d != 0), finite + 1
                    assert g[t, j] == TD.score_f64(sc[t, j], files[f], CLOCK, live[f], b0 + t, mods[first[f] + j], weight)
        print('n_cols %d: %d finite entries, %d differ from the exact value rounded once, worst %d ulp' % (n_cols, finite, differ, worst))
        _note('score_n_cols_%d' % n_cols, dict(entries=finite, differing=differ, share=differ / float(finite), worst_ulp=worst))
        assert finite > 500 * min(n_cols, 3) and worst <= 1
        assert (np.concatenate(scores) != got).any()
        # weight 0 adds nothing
        ctx.h2d(d_scores, host)
        ctx.tdoa_score(handle, d_models, len(mods), live, b, e, fi, first[fi], np.array(n_spk)[fi], n_cols, 0.0, d_scores + 3 * n_cols * 4)
        zero = np.zeros_like(host)
        ctx.d2h(zero, d_scores)
        assert zero.tobytes() == host.tobytes()
        hipabi = pkg('hipabi')
        with pytest.raises(hipabi.SpkdError, match='weight'):
            ctx.tdoa_score(handle, d_models, len(mods), live, b, e, fi, first[fi], np.array(n_spk)[fi], n_cols, -1.0, d_scores)
        with pytest.raises(hipabi.SpkdError, match='live channel'):
            ctx.tdoa_score(handle, d_models, len(mods), [1, 0, 0, 0], b, e, fi, first[fi], np.array(n_spk)[fi], n_cols, 1.0, d_scores)
        with pytest.raises(hipabi.SpkdError, match='model index'):
            ctx.tdoa_score(handle, d_models, len(mods) - 1, live, b, e, fi, first[fi], np.array(n_spk)[fi], n_cols, 1.0, d_scores)
    finally:
        ctx.dev_free(d_scores)
        ctx.dev_free(d_models)


# ------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _session():
    """Two speakers with one acoustic model, segments displaced by 100 frames, and the stream of their two seats: a
    step's delays are those of the speaker at its middle frame (of the speaker before, in a pause), +-1 sample of
    jitter, a tenth of the steps unreliable on a channel."""
    fe = pkg('frontend')
    feats, vad, truth = close_session(E2E_SEED, E2E_SECONDS, 2, eps=0.0)
    segs = displaced(truth, vad, 100)
    T = (len(feats) * HOP - 8000) // 4000 + 1
    rng = np.random.default_rng(E2E_STREAM_SEED)
    seats = np.array([SEAT_A, SEAT_B])
    delay = np.zeros((T, 4), dtype=np.int32)
    who = truth[0][2]
    for s in range(T):
        mid = fe.step_first_frame(s, HOP, WINDOW, 16000, RATE_OUT, 4000) + 15
        for a, b, k in truth:
            if a <= mid:
                who = k
        delay[s] = seats[who] + rng.integers(-1, 2, 4)
    delay[:, 0] = 0
    reliable = rng.random((T, 4)) >= 0.1
    return feats, vad, truth, segs, _file(delay, reliable, 0, 4000, 16000, 0)


def _boundaries(starts_per_turn, vad, truth):
    """(row count matches in every turn, the worst distance of a boundary inside a turn from the true one)."""
    worst, counts = 0, True
    for (a, b), starts in zip(vad, starts_per_turn):
        true = [t[0] for t in truth if a <= t[0] and t[1] <= b]
        if len(true) != len(starts):
            counts = False
            continue
        worst = max([worst] + [abs(x - y) for x, y in zip(starts[1:], true[1:])])
    return counts, worst


def _fused(sc, f, live, frames, mods, weight):
    """spkd_tdoa_score on the float64 scores of one turn, vectorised: the operations and their order are
    tdoa_numpy.score_f64's."""
    sc = sc.astype(np.float32)
    k = np.array([TD.step(t, CLOCK, f) for t in frames])
    x, rel = f['delay'][k].astype(np.float64), f['reliable'][k]
    out = sc.copy()
    for j in range(sc.shape[1]):
        ll = np.zeros(len(sc))
        for c in range(x.shape[1]):
            if (live >> c) & 1:
                d = x[:, c] - mods[j][c][0]
                t = d * d
                t = t * mods[j][c][2]
                ll = ll + np.where(rel[:, c], mods[j][c][3] - t, 0.0)
        fin = np.isfinite(sc[:, j])
        with np.errstate(invalid='ignore'):
            out[fin, j] = (sc[fin, j].astype(np.float64) + 1.0 * weight * ll[fin]).astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def _restated(with_tdoa, passes=3, penalty=50.0, jitter=0):
    """The stage on the CPU: reseg_numpy's records, models, scores and decoder, tdoa_numpy's moments and models ->
    per turn the decoded (first frames, speakers).  jitter: a seed; every finite acoustic score is then moved by up
    to 4 float32 ulp either way before anything reads it -- more than the device's acoustic scores differ from
    these (tests/test_reseg_batch.py holds them to an ulp under one model, and the models differ in the order of
    their float64 sums only).  A decoding that survives it rests on no tie."""
    feats, vad, truth, segs, f = _session()
    tdoa = pkg('pipeline').TDOA
    ranges = [[(a, b) for a, b, k in segs if k == spk] for spk in range(2)]
    tokens = None
    for _ in range(passes):
        models, ok = [], []
        for r in ranges:
            x = np.concatenate([feats[a:b] for a, b in r]) if r else np.zeros((0, 39), np.float32)
            mu, w, c, good = R.model_from_record(R.record_of_frames(x))
            models.append((mu, w, c))
            ok.append(good)
        if with_tdoa:
            st = TD.moments([f], CLOCK, [(a, b, 0, spk) for spk in range(2) for a, b in ranges[spk]], 2)
            mods, live = TD.models(st, [0, 0], ok, [f], tdoa['min_frames'], tdoa['floor_s'])
        new = []
        for a, b in vad:
            sc = R.scores(feats[a:b], models, ok, 2).astype(np.float32)
            if jitter:
                rng = np.random.default_rng(jitter + a)
                fin = np.isfinite(sc)
                sc[fin] = (sc[fin] + rng.integers(-4, 5, int(fin.sum())) * np.spacing(np.abs(sc[fin]))).astype(np.float32)
            if with_tdoa:
                sc = _fused(sc, f, live[0], range(a, b), mods, tdoa['weight'])
            frames, words, _ = R.viterbi(sc, penalty)
            new.append((tuple(frames), tuple(words)))
        same = new == tokens
        tokens = new
        if same:
            break
        ranges = [[], []]
        for (a, b), (frames, words) in zip(vad, tokens):
            ends = list(frames[1:]) + [b - a]
            for fr, en, w in zip(frames, ends, words):
                ranges[w].append((a + fr, a + en))
    return tokens


def test_the_restatement_needs_the_delays_to_find_the_boundaries():
    feats, vad, truth, segs, f = _session()
    assert len(set(k for _, _, k in truth)) == 2 and sum(1 for a, b in vad for t in truth if a < t[0] and t[1] <= b) >= 5
    counts, worst = _boundaries([[a + x for x in fr] for (a, _), (fr, _) in zip(vad, _restated(True))], vad, truth)
    print('restatement with the delays: worst boundary %d frames' % worst)
    assert counts and worst <= NEAR
    counts, plain = _boundaries([[a + x for x in fr] for (a, _), (fr, _) in zip(vad, _restated(False))], vad, truth)
    print('restatement without: row counts match %s, worst boundary %d frames' % (counts, plain))
    assert counts and plain > NEAR
    # no decision of the decoding with the delays is a tie: it survives 4 ulp of noise on the acoustic scores
    assert _restated(True, jitter=11) == _restated(True) == _restated(True, jitter=12)


@pytest.mark.gpu
def test_the_delays_find_the_boundaries_the_acoustics_cannot():
    pipeline = pkg('pipeline')
    feats, vad, truth, segs, f = _session()
    batch = Batch([(feats, vad, segs)])
    try:
        stream = _stream(batch.ctx, [f])

        def run(reseg, detail=None, timings=None):
            rows = pipeline.resegment_batch(batch.ctx, batch.eng.d_frames, len(batch.frames), batch.files, batch.d_stats, batch.seg_off,
                                            batch.labels, RATE, reseg, False, timings, detail, batch.segments, stream)[0]
            starts = np.rint(rows[:, 0] * RATE).astype(np.int64)
            per_turn = [[int(s) for s, r in zip(starts, rows) if a / RATE - 1e-9 <= r[0] and r[1] <= b / RATE + 1e-9] for a, b in vad]
            return rows, per_turn

        detail, timings = {}, {}
        rows, per_turn = run(dict(pipeline.RESEG_TDOA, passes=3), detail, timings)
        counts, worst = _boundaries(per_turn, vad, truth)
        want = _restated(True)
        _, want_worst = _boundaries([[a + x for x in fr] for (a, _), (fr, _) in zip(vad, want)], vad, truth)
        differ = [len(set(g) ^ set(a + x for x in fr)) for g, (a, _), (fr, _) in zip(per_turn, vad, want)]
        print('device: worst boundary %d frames; restatement %d; borders only one of them decodes, per turn: %s' % (worst, want_worst, differ))
        _note('end_to_end', dict(seed=E2E_SEED, stream_seed=E2E_STREAM_SEED, seconds=E2E_SECONDS, passes=3, worst_frames_device=int(worst),
                                 worst_frames_restatement=int(want_worst), borders_differing_per_turn=differ,      # (asserted to be 0 below)
                                 passes_run=detail['passes_run']))
        assert counts and len(rows) == len(truth) and worst <= NEAR
        # the restatement's decisions are no ties (its own test perturbs them), so the device decodes its tokens
        assert differ == [0] * len(vad)
        assert rows[:, 2].tolist() == [t[2] + 1 for t in truth]
        assert detail['tdoa_channels'] == [[1, 2, 3]]
        n = detail['passes_run']
        assert all(len(timings[k]) == n for k in ('reseg_tdoa_stats', 'reseg_tdoa_models', 'reseg_tdoa_score', 'reseg_loglik'))
        # the stream did the work, not the acoustics: the same input without it misses a boundary
        plain_rows, plain_turns = run(dict(pipeline.RESEG, passes=3))
        counts, plain = _boundaries(plain_turns, vad, truth)
        print('without the stream: row counts match %s, worst boundary %d frames' % (counts, plain))
        _note('end_to_end_plain_reseg', dict(row_counts_match=bool(counts), worst_frames_device=int(plain)))
        assert counts and plain > NEAR
        # weight 0: the rows of the call without tdoa, with every other option beside it
        for base in (dict(pipeline.RESEG, passes=2), dict(pipeline.RESEG_MD, passes=2), pipeline.RESEG_SOFT, pipeline.RESEG_GMM):
            d0, d1 = {}, {}
            a = run(dict(base, confidence=True), d0)[0]
            b = run(dict(base, confidence=True, tdoa=dict(pipeline.TDOA, weight=0.0)), d1)[0]
            assert a.tobytes() == b.tobytes() and d0['confidence'][0].tobytes() == d1['confidence'][0].tobytes(), base
            assert d1['tdoa_channels'] == [[1, 2, 3]] and 'tdoa_channels' not in d0
    finally:
        batch.close()


# ------------------------------------------------------------------ the pipeline
@pytest.mark.gpu
def test_recordings_to_speakers_with_the_delays_as_a_second_stream(ctx, tmp_path):
    from test_generate_exp import _synthetic_mixtures, load_model, write_model
    from test_mfcc_batch import _cfg, _talk
    pipeline = pkg('pipeline')
    write_model(str(tmp_path), *_synthetic_mixtures(np.random.default_rng(11)))
    model, cfg = load_model(str(tmp_path)), _cfg(400)
    s = _talk(19.5, 114).astype(np.float64)
    rng = np.random.default_rng(5)
    sh = lambda d: np.concatenate([np.zeros(d), s[:len(s) - d]]) if d >= 0 else np.concatenate([s[-d:], np.zeros(-d)])
    four = np.clip(np.rint(np.stack([sh(d) for d in SEAT_A], axis=1) + 20.0 * rng.standard_normal((len(s), 4))), -32768, 32767).astype(np.int16)
    one = _talk(8.0, 115)
    audios = [(four, 16000), (one, 16000)]
    bf = dict(pipeline.BEAMFORM, ref=0)
    plain = pipeline.diarize_audio_batch(ctx, model, cfg, audios, beamform=bf, reseg=pipeline.RESEG)
    detail, timings = {}, {}
    rows = pipeline.diarize_audio_batch(ctx, model, cfg, audios, beamform=bf, reseg=pipeline.RESEG_TDOA, detail=detail, timings=timings)
    print('rows:', [len(r) for r in rows], 'channels:', detail['tdoa_channels'])
    assert len(rows) == 2 and len(plain[0]) >= 2
    assert detail['tdoa_channels'] == [[1, 2, 3], []]
    assert len(timings['tdoa_pack']) == 1 and len(timings['reseg_tdoa_score']) == 1
    zero = pipeline.diarize_audio_batch(ctx, model, cfg, audios, beamform=bf, reseg=dict(pipeline.RESEG, tdoa=dict(pipeline.TDOA, weight=0.0)))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(zero, plain))
