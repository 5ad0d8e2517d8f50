"""Seats from the delay stream (include/spkd.h (6b4); seats.py; diarize_batch(..., seats=)): the seat cut behind change
detection and the seat split behind clustering, against the restatement of tests/seat_numpy.py.

What is compared how:
  decisions   exactly: every cut frame, every placed flag, every (a, b) of every merge log and every merge count.  The
              CPU tests show that no decision of the scenes is a tie: every Delta moved by a relative 1e-9, seven
              orders above the tolerance below, leaves them as they are.
  values      device and numpy share every operation of the statistic but log, which tests/test_tdoa_stream.py holds
              within 4 ulp of float64 on the device.  A 4-ulp log moves g = n log(var) by 4 * 2^-52 |g| and the
              product's own rounding by another 2^-53 |g|; the three g of a channel, halved and divided by w, so move
              the channel's t by at most 4.5 * 2^-52 (|g(A+B)| + |g(A)| + |g(B)|) / (2 w), and lambdac log(n / w) by at
              most 4.5 * 2^-52 of itself.  The roundings of the few subtractions and of the sum over at most seven
              channels act on values that differ by that much already and add at most half an ulp of a partial sum
              each, below 3.5 * 2^-52 S in all.  So |Delta_dev - Delta_np| <= 8 * 2^-52 * S with S = sum over counted
              channels of (|g(A+B)| + |g(A)| + |g(B)|) / (2 w) + |lambdac log(n / w)|: asserted for every Delta compared,
              the worst ratio to the bound written to profiles/seat_accuracy.json.
  end to end  the two-seat scene of tests/test_tdoa_stream.py with no truth fed anywhere: two speakers with seats,
              one without."""
import functools
import json
import os
import re

import numpy as np
import pytest

import seat_numpy as SN
import tdoa_numpy as TD
from conftest import pkg
from helpers import ROOT
from reseg_helpers import RATE, Batch
from test_tdoa_stream import (CLOCK, HOP, NEAR, RATE_OUT, SEAT_A, SEAT_B, WINDOW, _boundaries, _FakeDevice, _file, _NoDevice,
                              _session, _stream)

NAMES = ('spkd_tdoa_cuts', 'spkd_tdoa_split')
PROFILE = os.path.join(ROOT, 'profiles', 'seat_accuracy.json')
BOUND = 8.0 * 2.0 ** -52
M, FLOOR_S, LAMBDAC = 40, 1.0 / 16000.0, 1.0


def _note(key, value):
    """profiles/seat_accuracy.json gains one key: the figures, beside what the tests assert of them."""
    try:
        try:
            rec = json.load(open(PROFILE))
        except (OSError, ValueError):
            rec = {}
        rec['what'] = ('written by tests/test_seats.py: the worst |Delta_device - Delta_numpy| of spkd_tdoa_cuts and '
                       'spkd_tdoa_split as a share of the asserted bound 8 * 2^-52 * S, and the end-to-end figures')
        rec[key] = value
        with open(PROFILE, 'w') as f:
            f.write(json.dumps(rec, indent=1, sort_keys=True) + '\n')
    except OSError:
        pass                                    # (a read-only checkout: the figures are printed)


def _ratio(dev, want, S):
    """|dev - want| as a share of the bound; asserts it."""
    err = abs(float(dev) - float(want))
    assert err <= BOUND * S, (dev, want, S, err / (BOUND * S) if S else float('inf'))
    return err / (BOUND * S) if S else 0.0


# ------------------------------------------------------------------ not GPU
def test_entry_points_timers_and_settings_are_declared_exported_and_bound():
    hipabi, pipeline, seats = pkg('hipabi'), pkg('pipeline'), pkg('seats')
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'spkd.h')).read(), flags=re.S)
    lib = hipabi.load_library()
    for name in NAMES:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in hipabi.EXPORTS and hasattr(lib, name), name
        assert hasattr(hipabi.Context, name[len('spkd_'):]), name
    names = [n for n, _ in sorted(hipabi.TIMERS.items(), key=lambda kv: kv[1])]
    enum = re.search(r'enum \{\s*SPKD_T_CALL = 0,(.*?)SPKD_N_TIMERS', code, flags=re.S).group(1)
    assert ['call'] + [n.strip()[len('SPKD_T_'):].lower() for n in enum.split(',') if n.strip()] == names
    # behind the stream's other timers: the suite pins the enum's last entries, so nothing can follow them
    at = names.index('tdoa_score')
    assert names[at + 1:at + 3] == ['tdoa_cuts', 'tdoa_split'] and len(names) == len(set(names))
    assert re.search(r'#define SPKD_SEAT_MAX_N %d\b' % hipabi.SEAT_MAX_N, code) and hipabi.SEAT_MAX_N == 4096
    assert lib.spkd_abi_version() == 2
    mk = open(os.path.join(ROOT, 'speaker-diarization_amd', 'csrc', 'Makefile')).read()
    assert 'spkd_seat.hpp' in re.search(r'^HDR := (.*)$', mk, flags=re.M).group(1)
    assert seats.SEATS == dict(lambdac=1.0, threshold=0.0, min_frames=40, floor_s=1.0 / 16000.0, min_piece_s=1.0, max_passes=8,
                               cut=True, split=True)
    assert pipeline.SEATS is seats.SEATS and pipeline.seat_cut_batch is seats.seat_cut_batch
    assert pipeline.seat_split_batch is seats.seat_split_batch


def _true_changes(vad, truth):
    return [t[0] for a, b in vad for t in truth if a < t[0] and t[1] <= b]


def _perturb(seed):
    if seed is None:
        return None
    rng = np.random.default_rng(seed)
    return lambda d: d * (1.0 + 1e-9 * float(rng.uniform(-1.0, 1.0)))


@functools.lru_cache(maxsize=None)
def _restated(seed=None):
    """The two stages on the CPU, on the VAD turns and nothing else: (pieces, cut frames, calls, seats per piece, merge
    log, placed flags).  seed: every Delta is moved by up to a relative 1e-9 before anything reads it."""
    feats, vad, truth, segs, f = _session()
    S = pkg('seats').SEATS
    args = (S['min_frames'], S['floor_s'], S['lambdac'], S['threshold'])
    pieces, found, passes = SN.cut_loop(f, CLOCK, list(vad), int(S['min_piece_s'] * RATE), *args, S['max_passes'], _perturb(seed))
    seat, merges, flags = SN.split_labels(f, CLOCK, pieces, *args, _perturb(None if seed is None else seed + 100))
    return pieces, found, passes, seat, merges, flags


def test_the_restatement_finds_the_seats_without_any_truth():
    feats, vad, truth, segs, f = _session()
    pieces, found, passes, seat, merges, flags = _restated()
    true = _true_changes(vad, truth)
    print('true changes %s, cuts %s in %d calls' % (true, found, passes))
    assert len(true) >= 5 and len(found) == len(true)                       # a cut at every change and none elsewhere
    assert all(abs(a - b) <= NEAR for a, b in zip(found, true))
    # the single acoustic cluster holds every piece: two seats, whose members are the truth's
    who = [max(truth, key=lambda t: min(t[1], e) - max(t[0], b))[2] for b, e in pieces]
    assert all(flags) and len(set(seat)) == 2 == len(set(who))
    assert len(set(zip(seat, who))) == 2
    assert len(merges) == len(pieces) - 2


def test_no_decision_of_the_restatement_is_a_tie():
    base = _restated()
    for seed in (11, 12):
        moved = _restated(seed)
        assert moved[0] == base[0] and moved[1] == base[1] and moved[2] == base[2]
        assert moved[3] == base[3] and moved[5] == base[5]
        assert [m[:2] for m in moved[4]] == [m[:2] for m in base[4]]
        assert any(a[2] != b[2] for a, b in zip(moved[4], base[4]))         # (the perturbation did reach the values)


def _two_files():
    pipeline = pkg('pipeline')
    files = [pipeline.BatchFile(0, 1000, [(1.0, 3.0)]), pipeline.BatchFile(1000, 1000, [(0.5, 6.0)])]
    segments = [np.array([(1.0, 2.0), (2.0, 3.0)]), np.array([(0.5, 2.0), (2.0, 4.0), (4.0, 6.0)])]
    labels = [np.array([1, 2]), np.array([1, 2, 1])]
    two = [(np.zeros((3, 2), np.int32), np.ones((3, 2), bool), 0, 4000, 16000)] * 2
    return files, segments, labels, two


def test_every_value_error_comes_before_any_device_work():
    pipeline, fe, seats = pkg('pipeline'), pkg('frontend'), pkg('seats')
    files, segments, labels, two = _two_files()
    stream = fe.DelayStream.from_arrays(_FakeDevice(), HOP, WINDOW, two)
    ctx = _NoDevice()
    S = seats.SEATS
    bad = [(dict(S, gain=1.0), 'keys of SEATS'), ([1.0], 'keys of SEATS'), (dict(S, lambdac=float('inf')), 'seats lambdac'),
           (dict(S, lambdac='much'), 'seats lambdac'), (dict(S, threshold=float('nan')), 'seats threshold'),
           (dict(S, min_frames=0), 'seats min_frames'), (dict(S, min_frames=2.5), 'seats min_frames'),
           (dict(S, min_frames=True), 'seats min_frames'), (dict(S, floor_s=0.0), 'seats floor_s'),
           (dict(S, floor_s=float('nan')), 'seats floor_s'), (dict(S, min_piece_s=-1.0), 'seats min_piece_s'),
           (dict(S, min_piece_s=float('inf')), 'seats min_piece_s'), (dict(S, max_passes=0), 'seats max_passes'),
           (dict(S, max_passes=1.5), 'seats max_passes'), (dict(S, cut=1), 'seats cut'), (dict(S, split='yes'), 'seats split')]
    streams = [(None, 'delays='), (fe.DelayStream.from_arrays(_FakeDevice(), HOP, WINDOW, two[:1]), 'a batch of 2'),
               (fe.DelayStream.from_arrays(_FakeDevice(), 160, WINDOW, two), 'frames a second')]
    for s, word in bad:
        with pytest.raises(ValueError, match=word):
            seats.seat_cut_batch(ctx, files, segments, stream, 125.0, s)
        with pytest.raises(ValueError, match=word):
            seats.seat_split_batch(ctx, files, segments, labels, stream, 125.0, s)
        with pytest.raises(ValueError, match=word):
            pipeline.diarize_batch(ctx, 1 << 20, 2000, files, seats=s, delays=stream)
    for d, word in streams:
        with pytest.raises(ValueError, match=word):
            seats.seat_cut_batch(ctx, files, segments, d, 125.0, S)
        with pytest.raises(ValueError, match=word):
            seats.seat_split_batch(ctx, files, segments, labels, d, 125.0, S)
        with pytest.raises(ValueError, match=word):
            pipeline.diarize_batch(ctx, 1 << 20, 2000, files, seats=S, delays=d)
    with pytest.raises(ValueError, match='frames a second'):
        pipeline.diarize_batch(ctx, 1 << 20, 2000, files, rate=100.0, seats=S, delays=stream)
    # the pipeline's own rules: host hand-off, not fused, method hi
    for kw, word in ((dict(fused=True), 'not fused'), (dict(handoff='device', fused=True), 'not fused'),
                     (dict(fused=True, handoff='host'), 'not fused'), (dict(cl=dict(pipeline.DIA2_CL, method='in')), 'method hi')):
        with pytest.raises(ValueError, match=word):
            pipeline.diarize_batch(ctx, 1 << 20, 2000, files, seats=S, delays=stream, **kw)
    with pytest.raises(ValueError, match='one segment array'):
        seats.seat_cut_batch(ctx, files, segments[:1], stream, 125.0, S)
    # the audio entry point: seats take the beamformer, and their refusals come first
    with pytest.raises(ValueError, match='beamform='):
        pipeline.diarize_audio_batch(ctx, dict(pkg('self_vad').SELF_VAD), _Cfg(), [], seats=S)
    with pytest.raises(ValueError, match='keys of SEATS'):
        pipeline.diarize_audio_batch(ctx, dict(pkg('self_vad').SELF_VAD), _Cfg(), [], seats=dict(S, gain=1), beamform=pipeline.BEAMFORM)
    assert ctx.calls == []
    # the keys are optional, the defaults are SEATS'; min_piece is in frames
    o = seats._seat_options({}, 125.0)
    assert o == (1.0, 0.0, 40, 1.0 / 16000.0, 125, 8, True, True)
    assert seats._seat_options(dict(min_piece_s=0.0, threshold=float('-inf'), cut=False), 100.0)[4:7] == (1, 8, False)


class _Cfg(object):
    """A feature configuration for a call that is refused before it reads more than the frame clock."""
    frame_rate, hop, window_width, sample_rate = 125.0, HOP, WINDOW, RATE_OUT


class _Recorder(object):
    """A context that answers change detection and clustering with the least there is -- no detection in any turn, no
    merge -- and the seat calls with canned results, and records every call with its arguments."""

    def __init__(self, cuts=()):
        self.calls, self.cuts = [], list(cuts)

    def _rec(self, name, *a):
        self.calls.append((name,) + tuple(np.array(x).tolist() if isinstance(x, (np.ndarray, list, tuple)) else x for x in a))

    def dev_scratch(self, name, nbytes):
        self._rec('dev_scratch', name, nbytes)
        return 1 << 22

    def gw(self, d_frames, total, tb, te, p, **kw):
        self._rec('gw', d_frames, total, tb, te, sorted(k for k in kw))
        n = len(tb)
        z = np.zeros(n)
        return dict(status=0, off=np.arange(n + 1, dtype=np.int64), n_win=np.zeros(n, dtype=np.int32), win_det=np.zeros(n, dtype=np.int32),
                    det_start=z, det_maxi=z, final_start=z)

    def set_stats(self, d_frames, n_frames, begins, ends, sets, n_sets, d_stats):
        self._rec('set_stats', d_frames, n_frames, begins, ends, sets, n_sets, d_stats)

    def ahc(self, d_stats, seg_off, params):
        self._rec('ahc', d_stats, seg_off)
        n = int(seg_off[-1])
        return dict(status=0, n_merges=np.zeros(len(seg_off) - 1, dtype=np.int32), a=np.zeros(n, dtype=np.int32),
                    b=np.zeros(n, dtype=np.int32), d=np.zeros(n))

    def tdoa_cuts(self, stream, begins, ends, files, min_piece, min_frames, floor_s, lambdac, threshold):
        self._rec('tdoa_cuts', begins, ends, files, min_piece, min_frames, floor_s, lambdac, threshold)
        want = self.cuts.pop(0) if self.cuts else [-1] * len(begins)
        return np.array(want, dtype=np.int64), np.zeros(len(begins))

    def tdoa_stats(self, stream, begins, ends, files, sets, n_sets, d_stats):
        self._rec('tdoa_stats', begins, ends, files, sets, n_sets, d_stats)

    def tdoa_split(self, d_stats, off, prob_file, table, clock, min_frames, floor_s, lambdac, threshold):
        self._rec('tdoa_split', d_stats, off, prob_file, clock, min_frames, floor_s, lambdac, threshold)
        n = int(off[-1])
        return dict(n_merges=np.zeros(len(prob_file), dtype=np.int32), a=np.zeros(n, dtype=np.int32), b=np.zeros(n, dtype=np.int32),
                    d=np.zeros(n), placed=np.ones(n, dtype=np.int32))

    def last_ms(self, which='call'):
        return 0.25


def test_a_call_without_seats_asks_for_exactly_todays_calls_and_one_with_them_for_the_stages():
    pipeline, fe = pkg('pipeline'), pkg('frontend')
    files = [pipeline.BatchFile(0, 1000, [(1.0, 3.0), (4.0, 7.0)]), pipeline.BatchFile(1000, 1000, [(0.5, 6.0)])]
    many = (np.zeros((40, 2), np.int32), np.ones((40, 2), bool), 0, 4000, 16000)
    mono = (np.zeros((0, 1), np.int32), np.zeros((0, 1), bool), 0, 4000, 16000)
    stream = fe.DelayStream.from_arrays(_FakeDevice(), HOP, WINDOW, [many, mono])
    got = []
    for kw in ({}, dict(delays=stream), dict(seats=None, delays=stream), dict(seats=dict(pipeline.SEATS, cut=False, split=False), delays=stream)):
        rec = _Recorder()
        rows = pipeline.diarize_batch(rec, 1 << 20, 2000, files, **kw)
        assert [c[0] for c in rec.calls] == ['gw', 'dev_scratch', 'set_stats', 'ahc']
        got.append((rec.calls, [r.tobytes() for r in rows]))
    assert got[0] == got[1] == got[2] == got[3]
    assert [len(r) for r in pipeline.diarize_batch(_Recorder(), 1 << 20, 2000, files)] == [2, 1]
    # with seats: the first call cuts file 0's first segment at frame 200 and its second at 600, the second call the
    # piece [200, 375) at 300, the third nothing; the one-channel file is never handed in and keeps its object
    rec = _Recorder(cuts=[[200, 600], [-1, 300, -1, -1], [-1, -1]])
    detail, timings = {}, {}
    rows = pipeline.diarize_batch(rec, 1 << 20, 2000, files, seats=pipeline.SEATS, delays=stream, detail=detail, timings=None)
    names = [c[0] for c in rec.calls]
    assert names == ['gw', 'tdoa_cuts', 'tdoa_cuts', 'tdoa_cuts', 'dev_scratch', 'set_stats', 'ahc', 'dev_scratch', 'tdoa_stats', 'tdoa_split']
    cuts = [c for c in rec.calls if c[0] == 'tdoa_cuts']
    assert cuts[0][1:] == ([125, 500], [375, 875], [0, 0], 125, 40, 1.0 / 16000.0, 1.0, 0.0)
    assert cuts[1][1:4] == ([125, 200, 500, 600], [200, 375, 600, 875], [0, 0, 0, 0])
    assert cuts[2][1:4] == ([200, 300], [300, 375], [0, 0])
    assert detail['seats']['cuts'] == [[200 / 125.0, 300 / 125.0, 600 / 125.0], []] and detail['seats']['passes_run'] == 3
    st = [c for c in rec.calls if c[0] == 'set_stats'][0]
    assert st[3] == [125, 200, 300, 500, 600, 1062] and st[4] == [200, 300, 375, 600, 875, 1750]
    # no merge anywhere: every piece is a cluster of its own and a problem of one record; nothing splits
    sp = [c for c in rec.calls if c[0] == 'tdoa_split'][0]
    assert sp[2] == [0, 1, 2, 3, 4, 5, 6] and sp[3] == [0, 0, 0, 0, 0, 1]
    assert [r[:, 2].tolist() for r in rows] == [[1.0, 2.0, 3.0, 4.0, 5.0], [1.0]]
    assert detail['seats']['split'] == [[], []] and detail['seats']['unplaced'] == [0, 0]
    # max_passes bounds the calls
    rec = _Recorder(cuts=[[200, 600], [-1, 300, -1, -1]])
    pipeline.diarize_batch(rec, 1 << 20, 2000, files, seats=dict(pipeline.SEATS, max_passes=1, split=False), delays=stream)
    assert [c[0] for c in rec.calls].count('tdoa_cuts') == 1


def test_a_cut_time_gives_back_its_frame_with_and_without_the_text_contract():
    seats, pipeline, tables = pkg('seats'), pkg('pipeline'), pkg('tables')
    assert int((29 / 100.0) * 100.0) == 28                                  # a frame whose own time falls short of it
    f = pipeline.BatchFile(50, 10 ** 7, [])
    for rate in (125.0, 100.0, 125.0 / 3.0, 62.5):
        for frame in (1, 29, 57, 58, 113, 114, 200, 4093, 6218, 123457, 9999999):
            for contract in (False, True):
                t = seats.cut_time(frame, rate, contract)
                assert int(t * rate) == frame, (frame, rate, contract)
                if contract:
                    assert float(pkg('hipabi').py2_roundtrip(np.array([t]))[0]) == t
                _, _, b, e = tables._segment_ranges([f], [np.array([(0.0, t), (t, 10.0 ** 6)])], rate)
                assert b[1] == e[0] == 50 + frame
    assert seats.cut_time(29, 100.0, False) != 0.29 and seats.cut_time(200, 125.0, True) == 1.6


def test_a_split_orders_the_new_labels_and_leaves_other_files_alone():
    seats, pipeline, fe = pkg('seats'), pkg('pipeline'), pkg('frontend')
    many = (np.zeros((40, 2), np.int32), np.ones((40, 2), bool), 0, 4000, 16000)
    stream = fe.DelayStream.from_arrays(_FakeDevice(), HOP, WINDOW, [many, many])
    files = [pipeline.BatchFile(0, 2000, []), pipeline.BatchFile(2000, 2000, [])]
    segments = [np.array([(0.0, 1.0), (1.0, 2.0), (2.0, 4.0), (4.0, 5.0), (5.0, 6.0), (6.0, 7.0)]), np.array([(0.0, 1.0), (1.0, 2.0)])]
    labels = [np.array([2, 1, 2, 2, 1, 2], dtype=np.int32), np.array([1, 1], dtype=np.int32)]

    class Split(_Recorder):
        def tdoa_split(self, d_stats, off, prob_file, table, clock, *a):
            # problems: file 0 label 1 (segments 1, 4), file 0 label 2 (segments 0, 2, 3, 5), file 1 label 1 (0, 1).
            # label 2 of file 0: records 0 and 3 merge (positions 0, 3), record 2 is unplaced; the others keep apart
            assert np.array(off).tolist() == [0, 2, 6, 8] and np.array(prob_file).tolist() == [0, 0, 1]
            r = _Recorder.tdoa_split(self, d_stats, off, prob_file, table, clock, *a)
            r['n_merges'][:] = [1, 1, 1]
            r['a'][[0, 2, 6]], r['b'][[0, 2, 6]] = [0, 0, 0], [1, 3, 1]
            r['placed'][4] = 0
            return r

    detail = {}
    out = seats.seat_split_batch(Split(), files, segments, labels, stream, 125.0, seats.SEATS, None, detail)
    # file 0: label 1 stays whole (speaker 1); label 2 becomes the seat of segments 0 and 5 (250 frames, speaker 2) and
    # the seat of segment 2 (250 frames, speaker 3); the unplaced segment 3 joins the lower of the two equals
    assert out[0].tolist() == [2, 1, 3, 2, 1, 2] and out[0].dtype == np.int32
    assert out[1] is labels[1]
    assert detail['seats']['split'] == [[(2, 2)], []] and detail['seats']['unplaced'] == [1, 0]


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def ctx():
    c = pkg('hipabi').Context(0)
    yield c
    c.close()


def _seated(rng, T, C, ref, changes, jitter=2, reliable=0.9):
    """Delays of T steps: a seat (a delay per channel) per stretch between `changes`, +-jitter, a share unreliable."""
    delay = np.zeros((T, C), dtype=np.int64)
    edges = [0] + list(changes) + [T]
    for a, b in zip(edges[:-1], edges[1:]):
        delay[a:b] = rng.integers(-300, 301, C)
    delay += rng.integers(-jitter, jitter + 1, (T, C))
    delay[:, ref] = 0
    return delay.astype(np.int32), rng.random((T, C)) < reliable


@functools.lru_cache(maxsize=None)
def _cut_files():
    """0: 4 channels, 16 kHz, 400 steps of 31.25 frames.  1: 8 channels, 48 kHz, 3100 steps of 15.625 frames.  2: one
    channel.  3: 4 channels, channel 1 unreliable on steps 0 .. 49, one change at step 30.  4: 2 channels, the one that
    could count never reliable.  5: 3 channels, constant delays, all reliable."""
    rng = np.random.default_rng(61)
    d0, r0 = _seated(rng, 400, 4, 0, [3, 4, 33, 47, 120, 250, 398])
    d1, r1 = _seated(rng, 3100, 8, 3, [700, 1500, 1501, 2900])
    d3, r3 = _seated(rng, 80, 4, 0, [30], reliable=1.1)
    r3[:50, 1] = False
    d4, r4 = _seated(rng, 60, 2, 0, [20])
    r4[:, 1] = False
    d5 = np.tile(np.array([[0, 17, -40]], dtype=np.int32), (20, 1))
    return [_file(d0, r0, 0, 4000, 16000, 0), _file(d1, r1, 3, 6000, 48000, 20000),
            _file(np.zeros((0, 1), np.int32), np.zeros((0, 1), bool), 0, 4000, 16000, 70000), _file(d3, r3, 0, 4000, 16000, 71000),
            _file(d4, r4, 0, 4000, 16000, 75000), _file(d5, np.ones((20, 3), bool), 0, 4000, 16000, 78000)]


def _first(f, s):
    return pkg('frontend').step_first_frame(s, HOP, WINDOW, f['rate_in'], RATE_OUT, f['H']) + f['frame0']


def _cut_ranges():
    f0, f1, f2, f3, f4, f5 = _cut_files()
    return [(40, 50, 0),                                                     # inside one step
            (_first(f0, 3), _first(f0, 5), 0),                               # exactly two steps, a change between them
            (_first(f0, 30) + 7, _first(f0, 36) + 2, 0),                     # a few steps, a change inside
            (_first(f0, 390), _first(f0, 399) + 500, 0),                     # past the last step: the clamp
            (_first(f0, 10) + 3, _first(f0, 80) + 5, 0),                     # 70 steps: more candidates than a wave
            (0, _first(f0, 399) + 31, 0),                                    # the whole file: 400 steps, two tiles
            (_first(f1, 20) + 1, _first(f1, 3050) + 4, 1),                   # 3030 steps of 8 channels: twelve tiles
            (_first(f1, 1400), _first(f1, 1600), 1),
            (_first(f0, 100), _first(f0, 100) + 79, 0),                      # every candidate leaves a piece below min_piece
            (70000, 70500, 2),                                               # the one-channel file
            (71000, _first(f3, 79) + 31, 3),                                 # a channel unreliable on the whole left side
            (75000, _first(f4, 59) + 31, 4),                                 # no channel ever counts
            (300, 300, 0)]                                                   # empty


@pytest.mark.gpu
def test_cuts_equal_the_restatement_at_every_shape(ctx):
    files, ranges = _cut_files(), _cut_ranges()
    stream = _stream(ctx, files)
    handle = stream.handle([f['frame0'] for f in files])
    want = SN.cuts(files, CLOCK, ranges, 40, M, FLOOR_S, LAMBDAC, 0.0)
    # the cases are what they are called
    assert want[0][:2] == (-1, None) and want[8][:2] == (-1, None) and want[9][:2] == (-1, None) and want[11][:2] == (-1, None)
    assert want[12][:2] == (-1, None) and want[1][:2] == (-1, None)         # (two steps are below min_piece: see `other`)
    assert want[10][0] == _first(files[3], 30)
    assert all(w[0] >= 0 for w in (want[2], want[3], want[4], want[5], want[6], want[7]))
    assert SN.file_w(files[0], CLOCK) == 31.25 and SN.file_w(files[1], CLOCK) == 15.625
    b, e, fi = (np.array(v) for v in zip(*ranges))
    cut, delta = ctx.tdoa_cuts(handle, b, e, fi, 40, M, FLOOR_S, LAMBDAC, 0.0)
    assert ctx.last_ms('tdoa_cuts') > 0
    worst = 0.0
    for r, (t, d, S) in enumerate(want):
        assert cut[r] == t, (r, cut[r], t)
        if d is None:
            assert np.isnan(delta[r]), r
        else:
            worst = max(worst, _ratio(delta[r], d, S))
    # a threshold above every Delta: the values stay, nothing is cut
    high, delta_high = ctx.tdoa_cuts(handle, b, e, fi, 40, M, FLOOR_S, LAMBDAC, 1e12)
    assert (high == -1).all() and delta_high.tobytes() == delta.tobytes()
    # the same ranges in another order: the same per-range outputs, to the bit
    order = np.random.default_rng(2).permutation(len(ranges))
    cut2, delta2 = ctx.tdoa_cuts(handle, b[order], e[order], fi[order], 40, M, FLOOR_S, LAMBDAC, 0.0)
    assert cut2.tolist() == cut[order].tolist() and delta2.tobytes() == delta[order].tobytes()
    # other settings move the values as the restatement says; pieces of one step: the range of exactly two steps is cut
    other = SN.cuts(files, CLOCK, ranges[:6], 1, 10, FLOOR_S, 2.5, 0.0)
    assert other[1][0] == _first(files[0], 4) and other[0][:2] == (-1, None)
    cut3, delta3 = ctx.tdoa_cuts(handle, b[:6], e[:6], fi[:6], 1, 10, FLOOR_S, 2.5, 0.0)
    for r, (t, d, S) in enumerate(other):
        assert cut3[r] == t, r
        if d is not None:
            worst = max(worst, _ratio(delta3[r], d, S))
    # constant delays under a threshold below every Delta: all are equal, the lowest candidate frame is cut
    f5 = files[5]
    tie = [(78000, _first(f5, 19) + 31, 5)]
    (t, d, S), = SN.cuts(files, CLOCK, tie, 40, M, FLOOR_S, LAMBDAC, -1e9)
    assert t == _first(f5, 2)                                               # (the first step border 40 frames in)
    cut4, delta4 = ctx.tdoa_cuts(handle, [tie[0][0]], [tie[0][1]], [5], 40, M, FLOOR_S, LAMBDAC, -1e9)
    assert cut4[0] == t
    worst = max(worst, _ratio(delta4[0], d, S))
    print('cuts: worst |dev - np| = %.3f of the bound' % worst)
    _note('cuts_worst_share_of_bound', worst)
    hipabi = pkg('hipabi')
    for kw, word in ((dict(min_piece=0), 'min_piece'), (dict(min_frames=0), 'min_frames'), (dict(floor_s=float('inf')), 'floor_s'),
                     (dict(lambdac=float('nan')), 'lambdac'), (dict(threshold=float('nan')), 'threshold')):
        a = dict(dict(min_piece=40, min_frames=M, floor_s=FLOOR_S, lambdac=LAMBDAC, threshold=0.0), **kw)
        with pytest.raises(hipabi.SpkdError, match=word):
            ctx.tdoa_cuts(handle, b, e, fi, a['min_piece'], a['min_frames'], a['floor_s'], a['lambdac'], a['threshold'])
    for bad, word in (((b, e, fi + 9), 'file index'), ((e, b, fi), 'frame range'), ((b - 80000, e, fi), 'frame range')):
        with pytest.raises(hipabi.SpkdError, match=word):
            ctx.tdoa_cuts(handle, *bad, 40, M, FLOOR_S, LAMBDAC, 0.0)
    assert ctx.tdoa_cuts(handle, [], [], [], 40, M, FLOOR_S, LAMBDAC, 0.0)[0].shape == (0,)


def _record(rng, seat, n, channels, jitter=2):
    """A record of n frames at `seat` on `channels` (the others hold nothing)."""
    rec = np.zeros((8, 3), dtype=np.int64)
    for c in channels:
        x = seat[c] + rng.integers(-jitter, jitter + 1, n)
        rec[c] = (n, x.sum(), (x * x).sum())
    return rec


@functools.lru_cache(maxsize=None)
def _split_problems():
    """-> (files, problems): a problem is (file, records int64 [n, 8, 3]).  The first ten are the named shapes, 300 of
    mixed sizes follow."""
    rng = np.random.default_rng(77)
    z = lambda C: (np.zeros((2, C), np.int32), np.ones((2, C), bool))
    files = [_file(*z(4), 0, 4000, 16000, 0), _file(*z(8), 3, 6000, 48000, 0), _file(np.zeros((0, 1), np.int32), np.zeros((0, 1), bool), 0, 4000, 16000, 0)]
    live = [[1, 2, 3], [0, 1, 2, 4, 5, 6, 7], []]
    seats = [rng.integers(-300, 301, 8) for _ in range(4)]

    def recs(fi, n, n_seats=3, lo=60, hi=900, unplaced=0.0):
        out = []
        for _ in range(n):
            few = rng.random() < unplaced
            out.append(_record(rng, seats[int(rng.integers(0, n_seats))], int(rng.integers(5, 39)) if few else int(rng.integers(lo, hi)), live[fi]))
        return (fi, np.array(out, dtype=np.int64).reshape(n, 8, 3))

    disjoint = np.array([_record(rng, seats[0], 300, [1]), _record(rng, seats[0], 300, [2]), _record(rng, seats[0], 200, [1])])
    named = [recs(0, 0), recs(0, 1), recs(0, 2, n_seats=1), recs(0, 2, n_seats=2), recs(0, 65), recs(1, 130, n_seats=4),
             recs(0, 12, unplaced=0.4), recs(0, 5, lo=5, hi=39), (0, disjoint), recs(2, 3)]
    mixed = [recs(int(rng.integers(0, 2)), int(rng.integers(0, 13)), n_seats=int(rng.integers(1, 4)), unplaced=0.15) for _ in range(300)]
    return files, named + mixed


@functools.lru_cache(maxsize=None)
def _split_wanted():
    files, problems = _split_problems()
    return [SN.split(r.tolist(), files[fi], CLOCK, M, FLOOR_S, LAMBDAC, 0.0) for fi, r in problems]


def _run_split(ctx, files, problems, d_stats, table):
    off = np.concatenate([[0], np.cumsum([len(r) for _, r in problems])]).astype(np.int64)
    flat = np.concatenate([r.reshape(-1, 8, 3) for _, r in problems]) if off[-1] else np.zeros((0, 8, 3), np.int64)
    if off[-1]:
        ctx.h2d(d_stats, flat)
    r = ctx.tdoa_split(d_stats, off, [fi for fi, _ in problems], table, CLOCK, M, FLOOR_S, LAMBDAC, 0.0)
    after = np.zeros_like(flat)
    if off[-1]:
        ctx.d2h(after, d_stats)
    assert after.tobytes() == flat.tobytes()                                # d_stats is not modified
    return off, r


@pytest.mark.gpu
def test_split_chains_equal_the_restatement_and_do_not_depend_on_the_launch(ctx):
    files, problems = _split_problems()
    want = _split_wanted()
    # the cases are what they are called
    assert [len(w[0]) for w in want[:4]] == [0, 0, 1, 0] and len(want[4][0]) == 62 and len(want[5][0]) == 126
    assert not all(want[6][1]) and any(want[6][1]) and not any(want[7][1]) and not any(want[9][1])
    assert all(want[8][1]) and [m[:2] for m in want[8][0]] == [(0, 2)]       # channels 1 and 2 never meet: undefined, no merge
    stream = _stream(ctx, files)
    table = stream.table([0, 0, 0])
    total = sum(len(r) for _, r in problems)
    d_stats = ctx.dev_alloc(max(total, 1) * 24 * 8)
    try:
        off, r = _run_split(ctx, files, problems, d_stats, table)
        assert ctx.last_ms('tdoa_split') > 0
        worst, merges = 0.0, 0
        for p, (mg, flags) in enumerate(want):
            o = int(off[p])
            assert r['placed'][o:int(off[p + 1])].tolist() == [int(v) for v in flags], p
            assert int(r['n_merges'][p]) == len(mg), p
            for k, (a, b, d, S) in enumerate(mg):
                assert (int(r['a'][o + k]), int(r['b'][o + k])) == (a, b), (p, k)
                worst = max(worst, _ratio(r['d'][o + k], d, S))
            merges += len(mg)
        print('split: %d merges in %d problems, worst |dev - np| = %.3f of the bound' % (merges, len(problems), worst))
        _note('split_worst_share_of_bound', worst)
        # each problem's log is the log of the same problem called alone, bit for bit
        for p in list(range(10)) + list(range(10, 310, 13)):
            _, alone = _run_split(ctx, files, [problems[p]], d_stats, table)
            o, k = int(off[p]), int(r['n_merges'][p])
            assert int(alone['n_merges'][0]) == k, p
            assert alone['a'][:k].tolist() == r['a'][o:o + k].tolist() and alone['b'][:k].tolist() == r['b'][o:o + k].tolist(), p
            assert alone['d'][:k].tobytes() == r['d'][o:o + k].tobytes(), p
            assert alone['placed'].tolist() == r['placed'][o:int(off[p + 1])].tolist(), p
        # and in the reverse order of problems
        back = problems[::-1]
        off_b, rb = _run_split(ctx, files, back, d_stats, table)
        for p in range(len(problems)):
            q = len(problems) - 1 - p
            o, ob, k = int(off[p]), int(off_b[q]), int(r['n_merges'][p])
            assert int(rb['n_merges'][q]) == k and rb['d'][ob:ob + k].tobytes() == r['d'][o:o + k].tobytes(), p
        # the replay of a log gives the restatement's clusters
        hipabi = pkg('hipabi')
        lab = hipabi.labels_from_merges_batch(off, r['n_merges'], r['a'], r['b'])
        for p in (4, 5, 6):
            clusters = SN.replay(len(problems[p][1]), want[p][0])
            got = lab[int(off[p]):int(off[p + 1])]
            assert all(len(set(got[c].tolist())) == 1 for c in clusters) and len(set(got.tolist())) == len(clusters)
        # refusals, and nothing to do
        big = np.array([0, hipabi.SEAT_MAX_N + 1], dtype=np.int64)
        for a, word in (((big, [0]), '4096'), (([0, 2, 1], [0, 0]), 'non-decreasing'), (([1, 2], [0]), 'start at 0'), (([0, 2], [3]), 'file index')):
            with pytest.raises(hipabi.SpkdError, match=word):
                ctx.tdoa_split(d_stats, a[0], a[1], table, CLOCK, M, FLOOR_S, LAMBDAC, 0.0)
        with pytest.raises(hipabi.SpkdError, match='lambdac'):
            ctx.tdoa_split(d_stats, [0, 2], [0], table, CLOCK, M, FLOOR_S, float('inf'), 0.0)
        assert ctx.tdoa_split(d_stats, [0], [], table, CLOCK, M, FLOOR_S, LAMBDAC, 0.0)['n_merges'].shape == (0,)
        assert ctx.tdoa_split(0, [0, 0, 0], [0, 1], table, CLOCK, M, FLOOR_S, LAMBDAC, 0.0)['n_merges'].tolist() == [0, 0]
    finally:
        ctx.dev_free(d_stats)


# ------------------------------------------------------------------ end to end
@pytest.mark.gpu
def test_the_stage_finds_two_speakers_where_the_acoustics_find_one():
    pipeline = pkg('pipeline')
    feats, vad, truth, segs, f = _session()
    batch = Batch([(feats, vad, [(a, b, 0) for a, b in vad])])
    try:
        ctx, d_frames, total = batch.ctx, batch.eng.d_frames, len(batch.frames)
        stream = _stream(ctx, [f])

        def run(seats):
            detail, timings = {}, {}
            segments = pipeline.change_detect_batch(ctx, d_frames, total, batch.files, RATE, pipeline.DIA2_CD, timings, False)
            n_cd = len(segments[0])
            if seats is not None:
                segments = pipeline.seat_cut_batch(ctx, batch.files, segments, stream, RATE, seats, False, timings, detail)
            box = []
            res = pipeline.cluster_batch(ctx, d_frames, total, batch.files, segments, RATE, pipeline.DIA2_CL, timings, stats_out=box)
            acoustic = [lab for lab, _ in res]
            labels = acoustic
            if seats is not None:
                labels = pipeline.seat_split_batch(ctx, batch.files, segments, acoustic, stream, RATE, seats, timings, detail)
            rows = pipeline.resegment_batch(ctx, d_frames, total, batch.files, box[0][0], box[0][1], labels, RATE,
                                            dict(pipeline.RESEG_TDOA, passes=3), False, timings, detail, segments, stream)[0]
            return rows, n_cd, acoustic[0], labels[0], segments[0], detail, timings

        rows, n_cd, acoustic, labels, segments, detail, timings = run(pipeline.SEATS)
        # the acoustic stages see one voice: no cut inside a turn, one cluster
        assert n_cd == len(vad) and set(acoustic.tolist()) == {1}
        pieces, found, passes, seat, merges, flags = _restated()
        got_cuts = [int(t * RATE) for t in detail['seats']['cuts'][0]]
        print('cuts %s in %d calls; seats of the pieces %s' % (got_cuts, detail['seats']['passes_run'], labels.tolist()))
        assert got_cuts == found and detail['seats']['passes_run'] == passes == len(timings['seat_cuts'])
        assert [(int(s * RATE), int(e * RATE)) for s, e in segments] == pieces
        assert (labels - 1).tolist() == seat and detail['seats']['split'] == [[(1, 2)]] and detail['seats']['unplaced'] == [0]
        assert len(timings['seat_stats']) == len(timings['seat_split']) == 1
        # two speakers, every boundary inside a turn near the true one, the labels the truth's up to naming
        starts = np.rint(rows[:, 0] * RATE).astype(np.int64)
        per_turn = [[int(s) for s, r in zip(starts, rows) if a / RATE - 1e-9 <= r[0] and r[1] <= b / RATE + 1e-9] for a, b in vad]
        counts, worst = _boundaries(per_turn, vad, truth)
        print('with seats: %d rows, worst boundary %d frames' % (len(rows), worst))
        _note('end_to_end', dict(rows=len(rows), worst_boundary_frames=int(worst), cuts=got_cuts, passes_run=detail['seats']['passes_run']))
        assert counts and len(rows) == len(truth) and worst <= NEAR
        assert len(set(rows[:, 2].tolist())) == 2
        assert len(set(zip(rows[:, 2].tolist(), [t[2] for t in truth]))) == 2
        # the same without seats: one speaker
        plain = run(None)[0]
        assert len(set(plain[:, 2].tolist())) == 1 and len(plain) == len(vad)
    finally:
        batch.close()


@pytest.mark.gpu
def test_recordings_to_speakers_a_talker_who_changes_seat_becomes_two(ctx, tmp_path):
    from test_generate_exp import _synthetic_mixtures, load_model, write_model
    from test_mfcc_batch import _cfg, _talk
    pipeline = pkg('pipeline')
    write_model(str(tmp_path), *_synthetic_mixtures(np.random.default_rng(11)))
    model, cfg = load_model(str(tmp_path)), _cfg(400)
    s = _talk(19.5, 114).astype(np.float64)
    rng = np.random.default_rng(5)
    sh = lambda d: np.concatenate([np.zeros(d), s[:len(s) - d]]) if d >= 0 else np.concatenate([s[-d:], np.zeros(-d)])
    half = len(s) // 2
    at = lambda seat: np.stack([sh(d) for d in seat], axis=1)
    four = np.concatenate([at(SEAT_A)[:half], at(SEAT_B)[half:]])
    four = np.clip(np.rint(four + 20.0 * rng.standard_normal((len(s), 4))), -32768, 32767).astype(np.int16)
    audios = [(four, 16000), (_talk(8.0, 115), 16000)]
    bf = dict(pipeline.BEAMFORM, ref=0)
    plain = pipeline.diarize_audio_batch(ctx, model, cfg, audios, beamform=bf)
    detail, timings = {}, {}
    stream = pkg('frontend').DelayStream(ctx, cfg.hop, cfg.window_width, cfg.sample_rate)
    rows = pipeline.diarize_audio_batch(ctx, model, cfg, audios, beamform=bf, seats=pipeline.SEATS, detail=detail, timings=timings,
                                        delays=stream)
    delay, reliable = stream.to_host()[0]
    print('tracked delays, every fourth step:', delay[::4].tolist(), 'reliable share %.2f' % reliable[:, 1:].mean())
    print('plain rows:', [r.tolist() for r in plain])
    print('rows with seats:', [r.tolist() for r in rows], 'seats:', detail['seats'])
    assert len(set(rows[0][:, 2].tolist())) > 1
    # the seats did it: more speakers than the acoustics alone find, and none that speaks from both seats
    half_s = half / 16000.0
    early, late = set(rows[0][rows[0][:, 1] <= half_s, 2].tolist()), set(rows[0][rows[0][:, 0] >= half_s, 2].tolist())
    assert early and late and not (early & late)
    assert len(set(rows[0][:, 2].tolist())) > len(set(plain[0][:, 2].tolist())) and detail['seats']['split'][0]
    assert rows[1].tobytes() == plain[1].tobytes()
    assert len(timings['tdoa_pack']) == 1 and len(timings['seat_cuts']) >= 1
    off = pipeline.diarize_audio_batch(ctx, model, cfg, audios, beamform=bf, seats=dict(pipeline.SEATS, cut=False, split=False))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(off, plain))
