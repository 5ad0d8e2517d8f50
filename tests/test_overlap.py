"""Overlapped speech from the delay stream (include/spkd.h (6b5); overlap.py; diarize_batch(..., overlap=)): the runner-up
stream and the pair of speakers of every step, against the restatement of tests/overlap_numpy.py.

What is compared how:
  second, pairs   exactly, to the bit: integers, float32 compares and uncontracted fp64 products and compares that numpy
                  reproduces (the near rule has no transcendental in it).
  the scenes      the restatement with true seats as models at the variance floor: on two talkers the detected steps
                  contain every fully overlapped step and lie within the steps that touch the overlap; a silent second
                  speaker is never named (S1, S2, S4); S3's intruder is found in its three steps.  The 6 dB and 10 dB
                  figures go to profiles/overlap_accuracy.json, not asserted.
  end to end      the two-talker scene through the device beamformer with a second=True stream and the truth's rows:
                  the pieces name the other talker, start and end within one step (32 frames) of the true overlap and
                  cover every fully overlapped step."""
import functools
import json
import os
import re

import numpy as np
import pytest

import beamform_numpy as B
import overlap_numpy as ON
import tdoa_numpy as TD
from conftest import pkg
from helpers import ROOT
from test_tdoa_stream import HOP, NEAR, RATE_OUT, WINDOW, _FakeDevice, _file, _NoDevice

NAMES = ('spkd_tdoa_second', 'spkd_tdoa_overlap')
ACCURACY = os.path.join(ROOT, 'profiles', 'overlap_accuracy.json')
TIME = os.path.join(ROOT, 'profiles', 'overlap_time.json')
GATE, RATE = 4.5, 125.0


def _note(path, what, key, value):
    """A profile gains one key: the figures, beside what the tests assert of them."""
    try:
        try:
            rec = json.load(open(path))
        except (OSError, ValueError):
            rec = {}
        rec['what'] = what
        rec[key] = value
        with open(path, 'w') as f:
            f.write(json.dumps(rec, indent=1, sort_keys=True) + '\n')
    except OSError:
        pass                                    # (a read-only checkout: the figures are printed)


ACCURACY_WHAT = ('written by tests/test_overlap.py: the steps the overlap rule names on the synthetic scenes (CPU restatement, true '
                 'seats as models) and on the device end to end; truth: steps 4 - 6 wholly overlapped, 3 and 7 half')


# ------------------------------------------------------------------ not GPU
def test_entry_points_timers_and_settings_are_declared_exported_and_bound():
    hipabi, pipeline, overlap = pkg('hipabi'), pkg('pipeline'), pkg('overlap')
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
    at = names.index('tdoa_split')
    assert names[at + 1:at + 3] == ['tdoa_second', 'tdoa_overlap'] and len(names) == len(set(names))
    for define, value in (('MAX_SPK', hipabi.OVERLAP_MAX_SPK), ('MAX_RUN', hipabi.OVERLAP_MAX_RUN)):
        assert re.search(r'#define SPKD_OVERLAP_%s %d\b' % (define, value), code), define
    assert (hipabi.OVERLAP_MAX_SPK, hipabi.OVERLAP_MAX_RUN) == (16, 64) and lib.spkd_abi_version() == 2
    mk = open(os.path.join(ROOT, 'speaker-diarization_amd', 'csrc', 'Makefile')).read()
    assert 'spkd_overlap.hpp' in re.search(r'^HDR := (.*)$', mk, flags=re.M).group(1)
    assert overlap.OVERLAP == dict(min_second=0.1, guard=3, gate=4.5, min_channels=2, min_steps=2, min_frames=40, floor_s=1 / 16000)
    assert pipeline.OVERLAP is overlap.OVERLAP and pipeline.overlap_batch is overlap.overlap_batch
    assert pipeline.second_rows is overlap.second_rows
    fe = pkg('frontend')
    assert (fe.SECOND['min_second'], fe.SECOND['guard']) == (overlap.OVERLAP['min_second'], overlap.OVERLAP['guard'])


class _Cfg(object):
    """A feature configuration for a call that is refused before it reads more than the frame clock."""
    frame_rate, hop, window_width, sample_rate = 125.0, HOP, WINDOW, RATE_OUT


def _two_files():
    pipeline = pkg('pipeline')
    files = [pipeline.BatchFile(0, 1000, [(1.0, 3.0)]), pipeline.BatchFile(1000, 1000, [(0.5, 6.0)])]
    rows = [np.array([(1.0, 2.0, 1.0), (2.0, 3.0, 2.0)]), np.array([(0.5, 2.0, 1.0), (2.0, 4.0, 2.0), (4.0, 6.0, 1.0)])]
    two = [(np.zeros((3, 2), np.int32), np.ones((3, 2), bool), 0, 4000, 16000)] * 2
    return files, rows, two


def test_every_value_error_comes_before_any_device_work():
    pipeline, fe, overlap = pkg('pipeline'), pkg('frontend'), pkg('overlap')
    files, rows, two = _two_files()
    stream = fe.DelayStream.from_arrays(_FakeDevice(), HOP, WINDOW, two, second=[None, None])
    ctx = _NoDevice()
    O = overlap.OVERLAP
    bad = [(dict(O, gain=1.0), 'keys of OVERLAP'), ([1.0], 'keys of OVERLAP'), (dict(O, min_second=float('nan')), 'overlap min_second'),
           (dict(O, min_second='much'), 'overlap min_second'), (dict(O, guard=-1), 'overlap guard'), (dict(O, guard=1.5), 'overlap guard'),
           (dict(O, guard=True), 'overlap guard'), (dict(O, gate=0.0), 'overlap gate'), (dict(O, gate=float('inf')), 'overlap gate'),
           (dict(O, gate=float('nan')), 'overlap gate'), (dict(O, min_channels=0), 'overlap min_channels'),
           (dict(O, min_channels=2.5), 'overlap min_channels'), (dict(O, min_steps=0), 'overlap min_steps'),
           (dict(O, min_steps=65), 'overlap min_steps'), (dict(O, min_frames=0), 'overlap min_frames'),
           (dict(O, floor_s=0.0), 'overlap floor_s'), (dict(O, floor_s=float('nan')), 'overlap floor_s')]
    streams = [(None, 'delays='), (fe.DelayStream.from_arrays(_FakeDevice(), HOP, WINDOW, two), 'second=True'),
               (fe.DelayStream.from_arrays(_FakeDevice(), HOP, WINDOW, two[:1], second=[None]), 'a batch of 2'),
               (fe.DelayStream.from_arrays(_FakeDevice(), 160, WINDOW, two, second=[None, None]), 'frames a second')]
    for o, word in bad:
        with pytest.raises(ValueError, match=word):
            overlap.overlap_batch(ctx, files, rows, stream, 125.0, o)
        with pytest.raises(ValueError, match=word):
            pipeline.diarize_batch(ctx, 1 << 20, 2000, files, overlap=o, delays=stream)
        with pytest.raises(ValueError, match=word):
            pipeline.diarize_audio_batch(ctx, dict(pkg('self_vad').SELF_VAD), _Cfg(), [], overlap=o, beamform=pipeline.BEAMFORM)
    for d, word in streams:
        with pytest.raises(ValueError, match=word):
            overlap.overlap_batch(ctx, files, rows, d, 125.0, O)
        with pytest.raises(ValueError, match=word):
            pipeline.diarize_batch(ctx, 1 << 20, 2000, files, overlap=O, delays=d)
    with pytest.raises(ValueError, match='frames a second'):
        pipeline.diarize_batch(ctx, 1 << 20, 2000, files, rate=100.0, overlap=O, delays=stream)
    with pytest.raises(ValueError, match='host hand-off'):
        pipeline.diarize_batch(ctx, 1 << 20, 2000, files, overlap=O, delays=stream, fused=True)
    with pytest.raises(ValueError, match='one row array'):
        overlap.overlap_batch(ctx, files, rows[:1], stream, 125.0, O)
    many = [rows[0], np.array([(0.1 * i, 0.1 * i + 0.1, float(i)) for i in range(17)])]
    with pytest.raises(ValueError, match='17 speakers'):
        overlap.overlap_batch(ctx, files, many, stream, 125.0, O)
    # a stream the beamformer filled knows the settings of its runner-ups
    filled = fe.DelayStream(_FakeDevice(), HOP, WINDOW, RATE_OUT, second=True, min_second=0.2, guard=3)
    filled._reserve(_FakeDevice(), [(np.zeros((9000, 2), np.int16), 16000)] * 2, [0, 0], [(4000, 8000, 160)])
    with pytest.raises(ValueError, match='min_second 0.2'):
        overlap.overlap_batch(ctx, files, rows, filled, 125.0, O)
    # the audio entry point: overlap takes the beamformer and a stream that keeps the runner-ups
    with pytest.raises(ValueError, match='beamform='):
        pipeline.diarize_audio_batch(ctx, dict(pkg('self_vad').SELF_VAD), _Cfg(), [], overlap=O)
    with pytest.raises(ValueError, match='second=True'):
        pipeline.diarize_audio_batch(ctx, dict(pkg('self_vad').SELF_VAD), _Cfg(), [], overlap=O, beamform=pipeline.BEAMFORM,
                                     delays=fe.DelayStream(None, HOP, WINDOW))
    with pytest.raises(ValueError, match='second=True'):
        fe.DelayStream(None, HOP, WINDOW).handle_second()
    with pytest.raises(ValueError, match='second'):
        fe.DelayStream(None, HOP, WINDOW, second=1)
    assert ctx.calls == []
    # the keys are optional, the defaults are OVERLAP's
    assert overlap._overlap_options({}) == (0.1, 3, 4.5, 2, 2, 40, 1.0 / 16000.0)
    assert overlap._overlap_options(dict(min_steps=64, guard=0, min_second=float('-inf')))[:5] == (float('-inf'), 0, 4.5, 2, 64)


class _Recorder(object):
    """A context that answers change detection and clustering with the least there is, the overlap calls with canned
    results, and records every call."""

    def __init__(self, pairs=None):
        self.calls, self.pairs = [], pairs

    def _rec(self, name, *a):
        self.calls.append((name,) + tuple(np.array(x).tolist() if isinstance(x, (np.ndarray, list, tuple)) else x for x in a))

    def dev_scratch(self, name, nbytes):
        self._rec('dev_scratch', name, nbytes)
        return 1 << 22

    def gw(self, d_frames, total, tb, te, p, **kw):
        self._rec('gw', d_frames, total, tb, te)
        n = len(tb)
        z = np.zeros(n)
        return dict(status=0, off=np.arange(n + 1, dtype=np.int64), n_win=np.zeros(n, dtype=np.int32), win_det=np.zeros(n, dtype=np.int32),
                    det_start=z, det_maxi=z, final_start=z)

    def set_stats(self, d_frames, n_frames, begins, ends, sets, n_sets, d_stats):
        self._rec('set_stats', begins, ends, sets, n_sets)

    def ahc(self, d_stats, seg_off, params):
        self._rec('ahc', seg_off)
        n = int(seg_off[-1])
        return dict(status=0, n_merges=np.zeros(len(seg_off) - 1, dtype=np.int32), a=np.zeros(n, dtype=np.int32),
                    b=np.zeros(n, dtype=np.int32), d=np.zeros(n))

    def tdoa_stats(self, stream, begins, ends, files, sets, n_sets, d_stats):
        self._rec('tdoa_stats', begins, ends, files, sets, n_sets)

    def tdoa_models(self, d_stats, spk_file, ok, table, min_frames, floor_s, d_models):
        self._rec('tdoa_models', spk_file, ok, min_frames, floor_s)
        return np.full(len(table), 2, dtype=np.int32)

    def tdoa_overlap(self, stream, d_second, d_models, live, spk_off, gate, min_channels, min_steps, d_pair):
        self._rec('tdoa_overlap', d_second, live, spk_off, gate, min_channels, min_steps)

    def d2h(self, arr, dptr):
        self._rec('d2h', arr.shape)
        if self.pairs is not None:
            arr[:] = self.pairs

    def last_ms(self, which='call'):
        return 0.25

    def last_gw_items(self):
        return 0


def test_a_call_without_overlap_asks_for_exactly_todays_calls_and_one_with_it_for_the_stage():
    pipeline, fe = pkg('pipeline'), pkg('frontend')
    files = [pipeline.BatchFile(0, 1000, [(1.0, 3.0), (4.0, 7.0)]), pipeline.BatchFile(1000, 1000, [(0.5, 6.0)])]
    many = (np.zeros((40, 2), np.int32), np.ones((40, 2), bool), 0, 4000, 16000)
    mono = (np.zeros((0, 1), np.int32), np.zeros((0, 1), bool), 0, 4000, 16000)
    dev = _FakeDevice()
    stream = fe.DelayStream.from_arrays(dev, HOP, WINDOW, [many, mono], second=[np.full((40, 2), TD.NONE), None])
    assert len(dev.up) == 2 and dev.up[1][1].dtype == np.int32 and (dev.up[1][1] == TD.NONE).all()
    plain = fe.DelayStream.from_arrays(_FakeDevice(), HOP, WINDOW, [many, mono])
    got = []
    for kw in ({}, dict(delays=stream), dict(overlap=None, delays=stream), dict(overlap=None, delays=plain)):
        rec = _Recorder()
        rows = pipeline.diarize_batch(rec, 1 << 20, 2000, files, **kw)
        assert [c[0] for c in rec.calls] == ['gw', 'dev_scratch', 'set_stats', 'ahc']
        got.append((rec.calls, [r.tobytes() for r in rows]))
    assert got[0] == got[1] == got[2] == got[3]
    # with the stage: steps 20 - 23 of file 0 name the pair (0, 1); the rows are the same bytes
    pairs = np.full((40, 2), -1, dtype=np.int32)
    pairs[20:24] = (0, 1)
    rec = _Recorder(pairs)
    detail = {}
    rows = pipeline.diarize_batch(rec, 1 << 20, 2000, files, overlap=pipeline.OVERLAP, delays=stream, detail=detail)
    assert [r.tobytes() for r in rows] == got[0][1]
    names = [c[0] for c in rec.calls]
    assert names == ['gw', 'dev_scratch', 'set_stats', 'ahc', 'dev_scratch', 'dev_scratch', 'dev_scratch', 'tdoa_stats', 'tdoa_models',
                     'tdoa_overlap', 'd2h']
    st = [c for c in rec.calls if c[0] == 'tdoa_stats'][0]
    # no merge: every segment its own speaker; file 0's rows are speakers 1 and 2, file 1's row speaker 1
    assert st[1:] == ([125, 500, 1062], [375, 875, 1750], [0, 0, 1], [0, 1, 2], 3)
    assert [c for c in rec.calls if c[0] == 'tdoa_models'][0][1:] == ([0, 0, 1], [1, 1, 1], 40, 1.0 / 16000.0)
    assert [c for c in rec.calls if c[0] == 'tdoa_overlap'][0][1:] == (1 << 22, [2, 2], [0, 2, 3], 4.5, 2, 2)
    # steps 20 - 23 are the frames [624, 749): inside the silence between the rows but for the second row's start at 500 .. 875
    first = [fe.step_first_frame(s, HOP, WINDOW, 16000, RATE_OUT, 4000) for s in (20, 24)]
    assert first == [624, 749]
    ov = detail['overlap']
    assert ov['rows'][0].tolist() == [[624 / 125.0, 749 / 125.0, 2.0, 1.0]] and ov['rows'][1].shape == (0, 4)
    assert ov['speakers'] == [[1.0, 2.0], [1.0]] and ov['unassigned'] == [0, 0] and ov['seconds'] == [1.0, 0.0]
    assert ov['steps'][0].tolist() == pairs.tolist() and ov['steps'][1].shape == (0, 2)
    assert pipeline.second_rows(ov['rows'])[0].tolist() == [[624 / 125.0, 749 / 125.0, 1.0]]


class _Beamformer(object):
    """A context for the front end's calls of one batch: answers with the offsets the kernels would, records the names."""

    def __init__(self):
        self.calls = []

    def dev_scratch(self, name, nbytes):
        return 1 << 22

    def h2d(self, dptr, arr):
        self.calls.append('h2d')

    def d2h(self, arr, dptr):
        pass

    def bf_gcc(self, d_in, in_off, channels, geom, geoms, ref, d_ref, d_lag, d_val, d_curve=None):
        self.calls.append('bf_gcc')
        fe = pkg('frontend')
        ch = np.asarray(channels, dtype=np.int64)
        T = fe._beamform_steps(np.diff(in_off) // ch, ch, geom, geoms)
        return np.concatenate([[0], np.cumsum(T)]).astype(np.int64), None

    def bf_track(self, *a):
        self.calls.append('bf_track')

    def bf_sum(self, d_in, in_off, channels, geom, geoms, d_delay, d_out):
        self.calls.append('bf_sum')
        return np.concatenate([[0], np.cumsum(np.diff(in_off) // np.asarray(channels, dtype=np.int64))]).astype(np.int64)

    def resample_batch(self, d_in, in_off, channels, conv, convs, taps, d_out):
        self.calls.append('resample')
        return np.asarray(in_off, dtype=np.int64)

    def tdoa_pack(self, d_delay, d_val, min_peak, n, d_out):
        self.calls.append('tdoa_pack')

    def tdoa_second(self, d_delay, d_lag, d_val, n_best, min_peak, min_second, guard, n, d_out):
        self.calls.append(('tdoa_second', n_best, min_second, guard, n))

    def last_ms(self, which='call'):
        return 0.5


def test_a_stream_with_runner_ups_adds_one_call_per_group_and_one_without_none():
    fe, pipeline = pkg('frontend'), pkg('pipeline')
    audios = [(np.ones((20000, 4), np.int16), 16000), (np.ones((9000,), np.int16), 16000), (np.ones((12000, 2), np.int16), 16000)]
    runs = {}
    for second in (False, True):
        for group_bytes in (1 << 28, 1):
            ctx = _Beamformer()
            t = {}
            stream = fe.DelayStream(ctx, HOP, WINDOW, RATE_OUT, second=second, min_second=0.25, guard=5)
            fe.resample_batch(ctx, audios, 16000, group_bytes=group_bytes, beamform=pipeline.BEAMFORM, delays=stream, timings=t)
            runs[second, group_bytes] = ctx.calls
            assert ('tdoa_second' in t) == second and (stream.d_second is not None) == second
    for group_bytes in (1 << 28, 1):
        plain, more = runs[False, group_bytes], runs[True, group_bytes]
        assert [c for c in more if not isinstance(c, tuple)] == plain and 'tdoa_second' not in plain
        added = [c for c in more if isinstance(c, tuple)]
        # one group: 4 * 4 + 2 * 2 entries; a group per file: the one-channel file has no entry and no call
        assert added == ([('tdoa_second', 4, 0.25, 5, 20)] if group_bytes > 1 else [('tdoa_second', 4, 0.25, 5, 16), ('tdoa_second', 4, 0.25, 5, 4)])
        at = [i for i, c in enumerate(more) if isinstance(c, tuple)]
        assert all(more[i + 1] == 'tdoa_pack' or more[i - 1] == 'tdoa_pack' for i in at)
    # a group without a sample: no candidates, every entry NONE, by one upload and no kernel
    ctx = _Beamformer()
    stream = fe.DelayStream(ctx, HOP, WINDOW, RATE_OUT, second=True)
    fe.beamform_batch(ctx, [(np.zeros((0, 2), np.int16), 16000)], pipeline.BEAMFORM, delays=stream)
    assert ctx.calls.count('h2d') == 2 and not any(isinstance(c, tuple) for c in ctx.calls)


@functools.lru_cache(maxsize=None)
def _two(db_down=0.0):
    f, lag, val = ON.analysed(ON.two_talkers(db_down))
    return f, lag, val


def _named(f, seats, min_steps=2):
    C = np.asarray(f['delay']).shape[1]
    live = ((1 << C) - 1) & ~(1 << int(f['ref']))
    m = ON.seat_models([s[:C] for s in seats])
    return ON.detected(ON.overlap([f], m, [live], [0, len(seats)], GATE, 2, min_steps)[0])


def test_the_restatement_finds_the_overlap_on_the_scenes():
    f, lag, val = _two()
    # the runner-up is the other seat, to the sample, in every wholly overlapped step; outside the overlap there is none
    for t in ON.FULL:
        for c in (1, 2, 3):                                # (each channel is tracked on its own)
            assert {int(f['delay'][t, c]), int(f['second'][t, c])} == {ON.SEAT_1[c], ON.SEAT_2[c]}, (t, c)
        assert f['second'][t, 0] == TD.NONE and f['reliable'][t].all()
    outside = [t for t in range(len(f['delay'])) if t not in ON.PART]
    assert (f['second'][outside] == TD.NONE).all() and float(val[outside][:, 1:, 1].max()) < 0.05
    figures = {}
    for db in (0.0, 6.0, 10.0):
        g = _two(db)[0]
        figures['%g dB down' % db] = dict(min_steps_1=_named(g, [ON.SEAT_1, ON.SEAT_2], 1), min_steps_2=_named(g, [ON.SEAT_1, ON.SEAT_2], 2))
    print(figures)
    _note(ACCURACY, ACCURACY_WHAT, 'two_talkers', figures)
    for got in figures['0 dB down'].values():
        assert set(ON.FULL) <= set(got) <= set(ON.PART), got
    # one talker and a second speaker who is silent: never named -- also where the one talker changes seat (S2)
    for name in ('S1', 'S2', 'S4'):
        sc = B.scene(name)
        g = ON.analysed(sc['x'])[0]
        assert _named(g, [sc['truth'][0][2], ON.SEAT_2], 1) == [], name
    assert (ON.analysed(B.scene('S1')['x'])[0]['second'] == TD.NONE).all()
    # S3: the intruder's seat as a second speaker: its three steps
    s3 = ON.analysed(B.scene('S3')['x'])[0]
    assert _named(s3, [ON.SEAT_1, ON.SEAT_2]) == [4, 5, 6] == _named(s3, [ON.SEAT_1, ON.SEAT_2], 1)
    # a limit, recorded: S2's talker as two speakers, one per seat, reads as overlap where a window holds both seats
    s2 = B.scene('S2')
    _note(ACCURACY, ACCURACY_WHAT, 'S2_one_talker_as_two_speakers', _named(ON.analysed(s2['x'])[0], [s2['truth'][0][2], s2['truth'][1][2]], 1))


def test_the_restated_rules_on_small_cases():
    lag = np.array([[10, 50, 12, 90], [10, 11, 12, 13], [10, 50, 60, 70], [10, 50, 60, 70], [10, 50, 60, 70], [10, 50, 60, 70]])
    val = np.array([[0.9, 0.3, 0.2, 0.1], [0.9, 0.8, 0.7, 0.6], [0.05, 0.5, 0.4, 0.3], [0.9, -np.inf, 0.4, 0.3], [0.9, 0.05, 0.4, 0.3],
                    [0.9, np.float32(0.1), 0.4, 0.3]], dtype=np.float32)
    delay = np.array([10, 10, 10, 10, 10, 50])
    assert ON.second(delay, lag, val, 4, 0.1, 0.1, 3).tolist() == [50, TD.NONE, TD.NONE, 60, TD.NONE, 10]
    assert ON.second(delay, lag, val, 1, 0.1, 0.1, 3).tolist() == [TD.NONE] * 5 + [10]
    assert ON.second(delay, lag, val, 4, 0.1, 0.1, 45).tolist() == [90, TD.NONE, TD.NONE, 60, 60, TD.NONE]
    m = ON.seat_models([(0, 10), (0, 20)])
    assert ON.near(13, m[0][1], GATE) and not ON.near(14, m[0][1], GATE) and ON.near(7, m[0][1], GATE)      # (3^2 / 2 is the gate)
    raw = [(0, 1), (0, 1), (-1, -1), (0, 1), (0, 2), (0, 2), (0, 2)]
    assert ON.run_filter(raw, 1) == raw
    assert ON.run_filter(raw, 2) == [(0, 1), (0, 1), (-1, -1), (-1, -1), (0, 2), (0, 2), (0, 2)]
    assert ON.run_filter(raw, 3) == [(-1, -1)] * 4 + [(0, 2)] * 3


def test_the_host_intersection():
    overlap = pkg('overlap')
    first = lambda s: 10 * s
    steps = np.full((12, 2), -1, dtype=np.int32)
    steps[2:5] = (0, 2)                    # frames [20, 50): across the rows of speakers 0 and 2
    steps[6:8] = (1, 2)                    # frames [60, 80): a row of speaker 0, neither of the pair
    steps[10:12] = (0, 1)                  # frames [100, 120) clipped to the file's 113
    assert overlap.step_runs(steps) == [(2, 4, 0, 2), (6, 7, 1, 2), (10, 11, 0, 1)]
    rb, re_, sp = [0, 35, 55, 90], [35, 55, 90, 113], [0, 2, 0, 1]
    got, lost = overlap.pieces_of_file(steps, first, 113, rb, re_, sp)
    assert got == [(20, 35, 0, 2), (35, 50, 2, 0), (100, 113, 1, 0)] and lost == 20
    # through overlap_batch: the times give back the frames, with the text contract and without
    pipeline, fe, tables = pkg('pipeline'), pkg('frontend'), pkg('tables')
    many = (np.zeros((12, 2), np.int32), np.ones((12, 2), bool), 0, 4000, 16000)
    stream = fe.DelayStream.from_arrays(_FakeDevice(), HOP, WINDOW, [many], second=[None])
    f = pipeline.BatchFile(40, 350, [])
    ff = [stream.first_frame_of(0, s) for s in range(13)]
    assert ff[:4] == [0, 30, 61, 93] and ff[12] == 374
    rows = [np.array([(0.0, 0.8, 7.0), (0.8, 1.6, 9.0), (1.6, 2.5, 7.0), (2.5, 2.9, 8.0)])]        # frames 0, 100, 200, 312, 362
    for contract in (True, False):
        detail, timings = {}, {}
        out = pkg('overlap').overlap_batch(_Recorder(steps), [f], rows, stream, 125.0, pipeline.OVERLAP, contract, timings, detail)
        assert timings == dict(overlap_stats=[0.25], overlap_models=[0.25], overlap_match=[0.25])
        fr = lambda t: int(t * 125.0)
        got = [(fr(a), fr(b), p, q) for a, b, p, q in out[0].tolist()]
        # speakers 7, 8, 9 are indices 0, 1, 2: run (0, 2) over [61, 155), run (1, 2) over [186, 249), run (0, 1) over [311, 350)
        assert got == [(61, 100, 7.0, 9.0), (100, 155, 9.0, 7.0), (186, 200, 9.0, 8.0), (311, 312, 7.0, 8.0), (312, 350, 8.0, 7.0)]
        assert detail['overlap']['unassigned'] == [49] and detail['overlap']['seconds'] == [(39 + 55 + 14 + 1 + 38) / 125.0]
        _, _, b, e = tables._segment_ranges([f], [out[0][:, :2]], 125.0)
        assert (b - 40).tolist() == [g[0] for g in got] and (e - 40).tolist() == [g[1] for g in got]
        if contract:
            assert np.array_equal(pkg('hipabi').py2_roundtrip(out[0][:, :2].ravel().copy()), out[0][:, :2].ravel())


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def ctx():
    c = pkg('hipabi').Context(0)
    yield c
    c.close()


def _second_cases():
    """1000 entries: random candidates, and in front the named ones."""
    rng = np.random.default_rng(91)
    n = 1000
    lag = rng.integers(-160, 161, (n, 4)).astype(np.int32)
    val = np.sort(rng.random((n, 4)).astype(np.float32) * np.float32(0.6), axis=1)[:, ::-1].copy()
    val[rng.random((n, 4)) < 0.15] = -np.inf
    val[rng.random(n) < 0.1, 0] = np.float32(0.05)                         # an unreliable slot 0
    delay = lag[np.arange(n), rng.integers(0, 4, n)].copy()
    close = rng.random(n) < 0.2                                            # a guard that excludes every slot
    lag[close] = delay[close, None] + rng.integers(-3, 4, (int(close.sum()), 4))
    val[5] = (0.9, np.float32(0.1), 0.3, 0.2)                              # a value equal to min_second
    lag[5], delay[5] = (7, 40, 80, 90), 7
    val[6] = (0.9, np.nextafter(np.float32(0.1), np.float32(0)), 0.3, 0.2)
    lag[6], delay[6] = (7, 40, 80, 90), 7
    val[7], lag[7], delay[7] = (0.9, -np.inf, -np.inf, 0.5), (7, 0, 0, 90), 7
    val[8], lag[8], delay[8] = (np.float32(0.1), 0.5, 0.4, 0.3), (3, 7, 90, 100), 7    # min_peak itself is reliable; slot 0 is beyond the guard
    return delay.astype(np.int32), lag, val


@pytest.mark.gpu
def test_the_runner_up_stream_equals_the_restatement(ctx):
    hipabi = pkg('hipabi')
    delay, lag, val = _second_cases()
    d = [ctx.dev_alloc(4 * 4 * 1000 + 64) for _ in range(4)]
    try:
        ctx.h2d(d[0], delay), ctx.h2d(d[1], lag), ctx.h2d(d[2], val)
        seen = set()
        for n in (1, 63, 64, 65, 1000):
            for n_best, guard, min_second in ((4, 3, 0.1), (1, 3, 0.1), (4, 0, 0.3), (2, 400, -1.0)):
                want = ON.second(delay[:n], lag[:n], val[:n], n_best, 0.1, min_second, guard)
                ctx.h2d(d[3], np.full(n + 1, 12345, dtype=np.int32))
                ctx.tdoa_second(d[0], d[1], d[2], n_best, 0.1, min_second, guard, n, d[3])
                got = np.zeros(n + 1, dtype=np.int32)
                ctx.d2h(got, d[3])
                assert got[:n].tobytes() == want.tobytes() and got[n] == 12345, (n, n_best, guard)
                seen.add((n_best, guard, int((want != TD.NONE).sum()) > 0))
        assert ctx.last_ms('tdoa_second') > 0
        full = ON.second(delay, lag, val, 4, 0.1, 0.1, 3)
        assert full[5] == 40 and full[6] == TD.NONE and full[7] == 90 and full[8] == 3
        assert (4, 3, True) in seen and (2, 400, False) in seen                 # (a guard no slot passes: all NONE)
        assert 0.2 < (full != TD.NONE).mean() < 0.8
        for kw, word in ((dict(n_best=0), 'n_best'), (dict(n_best=5), 'n_best'), (dict(guard=-1), 'guard'),
                         (dict(min_peak=float('nan')), 'min_peak'), (dict(min_second=float('nan')), 'min_second')):
            a = dict(dict(n_best=4, min_peak=0.1, min_second=0.1, guard=3), **kw)
            with pytest.raises(hipabi.SpkdError, match=word):
                ctx.tdoa_second(d[0], d[1], d[2], a['n_best'], a['min_peak'], a['min_second'], a['guard'], 10, d[3])
        with pytest.raises(hipabi.SpkdError, match='null'):
            ctx.tdoa_second(d[0], 0, d[2], 4, 0.1, 0.1, 3, 10, d[3])
        with pytest.raises(hipabi.SpkdError, match='misaligned'):
            ctx.tdoa_second(d[0], d[1] + 2, d[2], 4, 0.1, 0.1, 3, 10, d[3])
        with pytest.raises(hipabi.SpkdError):
            ctx.tdoa_second(d[0], d[1], d[2], 4, 0.1, 0.1, 3, -1, d[3])
        ctx.tdoa_second(0, 0, 0, 4, 0.1, 0.1, 3, 0, 0)                         # nothing to do
    finally:
        for p in d:
            ctx.dev_free(p)


def _planted(rng, T, C, ref, n_spk, seats, holes=0.1):
    """Delays and runner-ups of T steps: per step a talker's seat, and for a third of the steps another talker's as the
    runner-up, both +-4 samples (3 is on the gate of a model at the floor, 4 beyond it); a tenth of the entries NONE."""
    a = rng.integers(0, n_spk, T)
    b = (a + rng.integers(1, max(n_spk, 2), T)) % max(n_spk, 1)
    both = rng.random(T) < 0.35
    for t in range(1, T):                                  # stretches, so that runs of several steps exist
        if rng.random() < 0.7:
            a[t], b[t], both[t] = a[t - 1], b[t - 1], both[t - 1]
    delay = seats[a][:, :C] + rng.integers(-4, 5, (T, C)) * (rng.random((T, C)) < 0.3)
    sec = np.where(both[:, None], seats[b][:, :C] + rng.integers(-4, 5, (T, C)) * (rng.random((T, C)) < 0.3), TD.NONE)
    reliable = rng.random((T, C)) >= holes
    sec = np.where(rng.random((T, C)) < holes, TD.NONE, sec)
    delay[:, ref] = 0
    sec[:, ref] = TD.NONE
    return delay.astype(np.int32), reliable, sec.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _overlap_files():
    """-> (files with `second`, speakers per file, models float64 [n, 8, 4], live masks).
    0: one channel.  1: C = 2, T = 1, two speakers, a pair.  2: C = 8, T = 255, ONE speaker.  3: C = 8, T = 256, 16 speakers.
    4: C = 8, T = 257, three speakers, channel 5 dead, planted ties, runs at both ends.  5: C = 8, T = 700, four
    speakers, a run at its first step, runs of 63 and of 64 steps.  6: C = 4, no live channel."""
    rng = np.random.default_rng(47)
    shapes = [(0, 1, 0, 0), (1, 2, 0, 2), (255, 8, 3, 1), (256, 8, 0, 16), (257, 8, 2, 3), (700, 8, 7, 4), (30, 4, 1, 2)]
    files, models, live, counts = [], [], [], []
    frame0 = 0
    for i, (T, C, ref, n_spk) in enumerate(shapes):
        # per channel the speakers sit at distinct lags, ten samples apart at the least
        seats = np.stack([rng.permutation(np.arange(-160, 161, 10))[:max(n_spk, 1)] for _ in range(8)], axis=1)
        if C > 1:
            delay, reliable, sec = _planted(rng, T, C, ref, n_spk, seats)
        else:
            delay, reliable, sec = np.zeros((0, 1), np.int32), np.zeros((0, 1), bool), np.zeros((0, 1), np.int64)
        m = ON.seat_models([tuple(int(v) for v in s) for s in seats[:n_spk]]) if n_spk else np.zeros((0, 8, 4))
        if i == 3:                                          # wider models too: var 1 .. 16
            for j in range(n_spk):
                var = np.float64(1 + j)
                m[j, :, 1], m[j, :, 2] = var, np.float64(1.0) / (np.float64(2.0) * var)
        mask = (((1 << C) - 1) & ~(1 << ref)) if C > 1 else 0
        if i == 1:                                          # one live channel: it alone decides (min_channels is capped)
            reliable[0], delay[0, 1], sec[0, 1] = True, seats[0][1], seats[1][1]
        if i == 4:
            mask &= ~(1 << 5)
            s = seats
            def put(t, pq):
                reliable[t] = True
                sec[t] = TD.NONE
                for c, (p, q) in pq.items():
                    delay[t, c], sec[t, c] = s[p][c], s[q][c]
            # ties in n_jk: two channels for (0, 1) and two for (0, 2): (0, 1); two for (1, 2), found first, and two for (0, 2): (0, 2)
            put(100, {0: (0, 1), 1: (1, 0), 3: (0, 2), 4: (2, 0)})
            put(101, {0: (1, 2), 1: (2, 1), 3: (0, 2), 4: (2, 0)})
            # the dead channel does not count: one live channel agrees, below min_channels
            put(103, {5: (0, 1), 6: (0, 1)})
            for t in (0, 1, 2, 254, 255, 256):              # runs that touch both ends of the file
                put(t, {c: (1, 2) for c in (0, 1, 3, 4, 6, 7)})
        if i == 5:
            s = seats
            for lo, hi in ((0, 3), (200, 263), (400, 464)): # the neighbour's first step goes on with other speakers' seats; 63; 64
                for t in range(lo, hi):
                    reliable[t] = True
                    for c in range(7):
                        delay[t, c], sec[t, c] = s[1][c], s[2][c]
                for t in (lo - 1, hi):
                    if 0 <= t < T:
                        sec[t] = TD.NONE
        if i == 6:
            mask = 0
        f = _file(delay, reliable, ref, 4000, 16000, frame0)
        f['second'] = sec
        files.append(f), models.append(m), live.append(mask), counts.append(n_spk)
        frame0 += 32 * T + 7
    return files, counts, models, live


@functools.lru_cache(maxsize=None)
def _overlap_raw(min_channels=2):
    files, counts, models, live = _overlap_files()
    return [ON.raw_pairs(f, m, lv, GATE, min_channels) for f, m, lv in zip(files, models, live)]


def _run_overlap(ctx, order, min_channels, min_steps, d_models):
    fe = pkg('frontend')
    files, counts, models, live = _overlap_files()
    fs = [files[i] for i in order]
    stream = fe.DelayStream.from_arrays(ctx, HOP, WINDOW, [(f['delay'], f['reliable'], f['ref'], f['H'], f['rate_in']) for f in fs],
                                        rate_out=RATE_OUT, second=[f['second'] for f in fs])
    spk_off = np.concatenate([[0], np.cumsum([counts[i] for i in order])]).astype(np.int64)
    ctx.h2d(d_models, np.concatenate([models[i] for i in order] + [np.zeros((1, 8, 4))]))
    T = [len(f['delay']) for f in fs]
    d_pair = ctx.dev_scratch('test_overlap_pair', 8 * sum(T) + 16)
    ctx.h2d(d_pair, np.full(2 * sum(T) + 2, 777, dtype=np.int32))
    ctx.tdoa_overlap(stream.handle([f['frame0'] for f in fs]), stream.handle_second(), d_models, [live[i] for i in order], spk_off,
                     GATE, min_channels, min_steps, d_pair)
    got = np.zeros(2 * sum(T) + 2, dtype=np.int32)
    ctx.d2h(got, d_pair)
    assert got[-2:].tolist() == [777, 777]
    off = np.concatenate([[0], np.cumsum(T)])
    assert [a.tolist() for a in stream.to_host_second()] == [np.asarray(f['second']).tolist() for f in fs]
    return {i: got[2 * off[k]:2 * off[k + 1]].reshape(-1, 2) for k, i in enumerate(order)}, stream


@pytest.mark.gpu
def test_the_pairs_equal_the_restatement_and_do_not_depend_on_the_other_files(ctx):
    hipabi = pkg('hipabi')
    files, counts, models, live = _overlap_files()
    raw = _overlap_raw()
    # the cases are what they are called
    assert raw[4][100] == (0, 1) and raw[4][101] == (0, 2) and raw[4][103] == (-1, -1)
    assert raw[4][:3] == [(1, 2)] * 3 == raw[4][254:] and raw[5][:3] == [(1, 2)] * 3 and raw[5][3] != (1, 2)
    assert all(p == (-1, -1) for i in (2, 6) for p in raw[i]) and raw[1] == [(0, 1)] and len(raw[0]) == 0
    assert len(set(raw[3])) >= 15 and sum(p[0] >= 0 for p in raw[3]) > 40           # many of the 120 pairs are named
    off_by = np.abs(files[5]['delay'][:, :, None] - models[5][:, :, 0].T[None])      # [T, C, speakers]: 3 is on the gate, 4 beyond
    assert (off_by == 3).any() and (off_by == 4).any() and ON.near(3, (0.0, 1.0, 0.5, 0.0), GATE) and not ON.near(4, (0.0, 1.0, 0.5, 0.0), GATE)
    want64 = ON.run_filter(raw[5], 64)
    assert ON.detected(want64) == list(range(400, 464)) and set(range(200, 263)) <= set(ON.detected(ON.run_filter(raw[5], 63)))
    d_models = ctx.dev_alloc((sum(counts) + 1) * 8 * 4 * 8)
    try:
        everything = list(range(len(files)))
        base = {}
        for min_steps in (1, 2, 4, 64):
            got, stream = _run_overlap(ctx, everything, 2, min_steps, d_models)
            assert ctx.last_ms('tdoa_overlap') > 0
            for i in everything:
                want = np.array(ON.run_filter(raw[i], min_steps), dtype=np.int32).reshape(-1, 2)
                assert got[i].tobytes() == want.tobytes(), (min_steps, i, np.nonzero((got[i] != want).any(axis=1))[0][:5])
            base[min_steps] = got
        # min_channels beyond the live channels of a file: all of them must agree
        got, _ = _run_overlap(ctx, everything, 7, 1, d_models)
        raw7 = _overlap_raw(7)
        for i in everything:
            assert got[i].tobytes() == np.array(raw7[i], dtype=np.int32).reshape(-1, 2).tobytes(), i
        # the same files in another order, and alone: the same bits per file
        got, _ = _run_overlap(ctx, everything[::-1], 2, 2, d_models)
        assert all(got[i].tobytes() == base[2][i].tobytes() for i in everything)
        for i in (1, 4, 5):
            got, _ = _run_overlap(ctx, [i], 2, 2, d_models)
            assert got[i].tobytes() == base[2][i].tobytes(), i
        # refusals, before any device work; and nothing to do
        got, stream = _run_overlap(ctx, everything, 2, 2, d_models)
        handle, d_second = stream.handle([f['frame0'] for f in files]), stream.handle_second()
        spk_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        d_pair = ctx.dev_scratch('test_overlap_pair', 16)
        ok = dict(live=live, spk_off=spk_off, gate=GATE, min_channels=2, min_steps=2)
        up = spk_off.copy()
        up[1:] += 1
        down = spk_off.copy()
        down[3] = down[2] - 1
        wide = np.concatenate([[0], np.cumsum([17] + counts[1:])])
        for kw, word in ((dict(gate=0.0), 'gate'), (dict(gate=float('nan')), 'gate'), (dict(min_channels=0), 'min_channels'),
                         (dict(min_steps=0), 'min_steps'), (dict(min_steps=65), 'min_steps'), (dict(spk_off=up + 1), 'start at 0'),
                         (dict(spk_off=down), 'non-decreasing'), (dict(spk_off=wide), '16 speakers'),
                         (dict(live=[1] + live[1:]), 'live channel')):
            a = dict(ok, **kw)
            with pytest.raises(hipabi.SpkdError, match=word):
                ctx.tdoa_overlap(handle, d_second, d_models, a['live'], a['spk_off'], a['gate'], a['min_channels'], a['min_steps'], d_pair)
        with pytest.raises(hipabi.SpkdError, match='null'):
            ctx.tdoa_overlap(handle, 0, d_models, live, spk_off, GATE, 2, 2, d_pair)
        bad = handle[2].copy()
        bad[1, 3] = 5
        with pytest.raises(hipabi.SpkdError, match='reference channel'):
            ctx.tdoa_overlap((handle[0], handle[1], bad, handle[3]), d_second, d_models, live, spk_off, GATE, 2, 2, d_pair)
        mono = (0, 0, handle[2][:1], handle[3])
        ctx.tdoa_overlap(mono, 0, 0, [0], [0, 0], GATE, 2, 2, 0)                 # no step: nothing launched
    finally:
        ctx.dev_free(d_models)


@pytest.mark.gpu
def test_the_stage_finds_the_second_talker_on_the_device(ctx):
    fe, pipeline, overlap = pkg('frontend'), pkg('pipeline'), pkg('overlap')
    x = ON.two_talkers()
    stream = fe.DelayStream(ctx, HOP, WINDOW, RATE_OUT, second=True)
    timings = {}
    fe.beamform_batch(ctx, [(x, 16000)], dict(pipeline.BEAMFORM, ref=0), timings=timings, delays=stream)
    assert len(timings['tdoa_second']) == 1 and timings['tdoa_second'][0] > 0
    # the stream is the restatement's, runner-ups included
    f = _two()[0]
    (delay, reliable), sec = stream.to_host()[0], stream.to_host_second()[0]
    assert np.array_equal(reliable, f['reliable']) and np.array_equal(delay, np.where(f['reliable'], f['delay'], 0))
    assert np.array_equal(sec, f['second'])
    n_frames = len(x) // HOP
    files = [pipeline.BatchFile(0, n_frames, [(0.0, 3.0)])]
    rows = [np.array([(0.0, 1.5, 1.0), (1.5, 3.0, 2.0)])]              # the truth, a speaker a frame: 1 talks to 2 s, 2 from 1 s on
    detail, t2 = {}, {}
    out = overlap.overlap_batch(ctx, files, rows, stream, RATE, pipeline.OVERLAP, True, t2, detail)
    print('overlap rows', out[0].tolist(), 'steps', ON.detected(detail['overlap']['steps'][0]))
    _note(ACCURACY, ACCURACY_WHAT, 'device_end_to_end', dict(rows=out[0].tolist(), steps=ON.detected(detail['overlap']['steps'][0])))
    assert all(len(t2[k]) == 1 and t2[k][0] > 0 for k in ('overlap_stats', 'overlap_models', 'overlap_match'))
    got = out[0]
    assert len(got) == 2 and got[:, 2:].tolist() == [[1.0, 2.0], [2.0, 1.0]]          # each row's piece names the other talker
    lo, hi = int(got[0, 0] * RATE), int(got[-1, 1] * RATE)
    assert int(got[0, 1] * RATE) == int(got[1, 0] * RATE) == 187           # the pieces meet where the rows do
    assert abs(lo - ON.LO // HOP) <= NEAR and abs(hi - ON.HI // HOP) <= NEAR      # within one step of the true overlap
    assert set(ON.FULL) <= set(ON.detected(detail['overlap']['steps'][0])) <= set(ON.PART)
    assert lo <= stream.first_frame_of(0, ON.FULL[0]) and hi >= stream.first_frame_of(0, ON.FULL[-1] + 1) - 1
    assert detail['overlap']['unassigned'] == [0] and pipeline.second_rows(out)[0][:, 2].tolist() == [2.0, 1.0]


@pytest.mark.gpu
def test_recordings_to_rows_the_stage_leaves_the_rows_alone(ctx, tmp_path):
    from test_generate_exp import _synthetic_mixtures, load_model, write_model
    from test_mfcc_batch import _cfg, _talk
    pipeline = pkg('pipeline')
    write_model(str(tmp_path), *_synthetic_mixtures(np.random.default_rng(11)))
    model, cfg = load_model(str(tmp_path)), _cfg(400)
    audios = [(ON.two_talkers(), 16000), (_talk(8.0, 115), 16000)]
    bf = dict(pipeline.BEAMFORM, ref=0)
    plain = pipeline.diarize_audio_batch(ctx, model, cfg, audios, beamform=bf)
    detail, timings = {}, {}
    rows = pipeline.diarize_audio_batch(ctx, model, cfg, audios, beamform=bf, overlap=pipeline.OVERLAP, detail=detail, timings=timings)
    print('rows', [r.tolist() for r in rows], 'overlap', [r.tolist() for r in detail['overlap']['rows']])
    assert len(plain) == len(rows) == 2 and all(a.tobytes() == b.tobytes() for a, b in zip(plain, rows))
    ov = detail['overlap']
    assert set(ov) == {'rows', 'speakers', 'steps', 'seconds', 'unassigned'}
    assert [s.shape for s in ov['steps']] == [(11, 2), (0, 2)] and len(ov['rows']) == 2 and ov['rows'][1].shape == (0, 4)
    assert len(timings['tdoa_second']) == 1 and len(timings['tdoa_pack']) == 1
    # one stream serves seats and overlap
    both = pipeline.diarize_audio_batch(ctx, model, cfg, audios, beamform=bf, overlap=pipeline.OVERLAP,
                                        seats=dict(pipeline.SEATS, cut=False, split=False))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, both))


@pytest.mark.gpu
def test_the_time_of_a_batch_of_hours_is_recorded(ctx):
    """64 files x 14 400 steps (an hour each) x 4 channels of generated streams, two speakers a file: the time of
    spkd_tdoa_second on as many entries and of spkd_tdoa_overlap (both launches) go to profiles/overlap_time.json.  A
    record with no bound."""
    fe = pkg('frontend')
    rng = np.random.default_rng(5)
    n_files, T, C = 64, 14400, 4
    seats = np.array([ON.SEAT_1, ON.SEAT_2])
    who = np.repeat(rng.integers(0, 2, T // 40), 40)
    delay = (seats[who] + rng.integers(-1, 2, (T, C))).astype(np.int32)
    delay[:, 0] = 0
    sec = np.where((rng.random(T) < 0.1)[:, None], seats[1 - who], TD.NONE).astype(np.int64)
    sec[:, 0] = TD.NONE
    one = (delay, rng.random((T, C)) < 0.95, 0, 4000, 16000)
    stream = fe.DelayStream.from_arrays(ctx, HOP, WINDOW, [one] * n_files, rate_out=RATE_OUT, second=[sec] * n_files)
    models = np.concatenate([ON.seat_models([ON.SEAT_1, ON.SEAT_2])] * n_files)
    n = n_files * T * C
    d = [ctx.dev_alloc(models.nbytes), ctx.dev_alloc(8 * n_files * T), ctx.dev_alloc(16 * n), ctx.dev_alloc(16 * n), ctx.dev_alloc(4 * n)]
    try:
        ctx.h2d(d[0], models)
        handle = stream.handle(np.arange(n_files) * 450000)
        args = (handle, stream.handle_second(), d[0], [0b1110] * n_files, np.arange(n_files + 1) * 2, GATE, 2, 2, d[1])
        ctx.tdoa_overlap(*args)
        ms = []
        for _ in range(3):
            ctx.tdoa_overlap(*args)
            ms.append(ctx.last_ms('tdoa_overlap'))
        pair = np.zeros((n_files * T, 2), dtype=np.int32)
        ctx.d2h(pair, d[1])
        assert (pair[:T] == pair[-T:]).all() and (pair[:, 0] >= 0).any()
        lag = np.tile(np.concatenate([delay.reshape(-1, 1), np.where(sec == TD.NONE, 0, sec).reshape(-1, 1), np.zeros((T * C, 2), np.int64)], axis=1), (n_files, 1)).astype(np.int32)
        val = np.tile(np.array([0.8, 0.3, -np.inf, -np.inf], dtype=np.float32), (n, 1))
        ctx.h2d(d[2], lag), ctx.h2d(d[3], val)
        ctx.tdoa_second(stream.d_stream, d[2], d[3], 4, 0.1, 0.1, 3, n, d[4])
        ms2 = []
        for _ in range(3):
            ctx.tdoa_second(stream.d_stream, d[2], d[3], 4, 0.1, 0.1, 3, n, d[4])
            ms2.append(ctx.last_ms('tdoa_second'))
        rec = dict(files=n_files, steps_per_file=T, channels=C, speakers_per_file=2, tdoa_overlap_ms=min(ms), tdoa_overlap_ms_all=ms,
                   tdoa_second_ms=min(ms2), tdoa_second_ms_all=ms2)
        print(rec)
        _note(TIME, 'written by tests/test_overlap.py: device-event milliseconds of spkd_tdoa_overlap (match and run filter) and of '
                    'spkd_tdoa_second on 64 files x 14 400 steps x 4 channels; three calls after one warm-up, the least', 'batch', rec)
        assert min(ms) > 0 and min(ms2) > 0
    finally:
        for p in d:
            ctx.dev_free(p)
