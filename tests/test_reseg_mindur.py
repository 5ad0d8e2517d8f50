"""The speaker loop with a minimum duration: spkd_mindur_viterbi_batch, its restatement
(tests/reseg_mindur_numpy.py) against a brute-force decoder over the expanded states, and
reseg['min_dur_s'] in pipeline.resegment_batch / diarize_batch.  PARITY: no reference counterpart."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import reseg_mindur_numpy as M
import reseg_numpy as R
from helpers import ROOT
from conftest import pkg
from reseg_helpers import (Batch, StubContext, close_session as _close_session, normal_scores as _normal_scores,
                           ptr as _ptr)

RATE = 125.0


def _lengths(D):
    return [0, 1, D - 1, D, D + 1, 2 * D - 1, 2 * D, 2 * D + 1]


def _dyadic(rng, T, W):
    """Multiples of 1/8 in [-20, 0] (every fp64 sum of them is exact) with planted ties, a -inf
    column, frames nobody can score and a NaN."""
    sc = (-rng.integers(0, 161, (T, W)) / 8.0).astype(np.float32)
    if T >= 4:
        sc[T // 2:T // 2 + 2] = sc[T // 2 - 1]                              # repeated frames
        sc[T // 4] = sc[T // 4, 0]                                          # a frame that ties every word
    if W > 1 and rng.integers(0, 3) == 0:
        sc[:, int(rng.integers(0, W))] = -np.inf                            # a speaker that is not ok
    if T >= 3 and rng.integers(0, 2) == 0:
        t = int(rng.integers(0, T - 1))
        sc[t:t + 2] = -np.inf                                               # frames nobody can score
    if T >= 2 and rng.integers(0, 3) == 0:
        sc[int(rng.integers(0, T)), int(rng.integers(0, W))] = np.nan
    if W > 1 and T >= 6 and rng.integers(0, 3) == 0:
        sc[T // 3, 0] = -np.inf                                             # one -inf inside a word's windows
    return sc


def _check_path(sc, penalty, D, frames, words, score):
    T = len(sc)
    if T == 0:
        assert (frames, words, score) == ([], [], -np.inf)
        return
    assert frames[0] == 0 and all(a < b for a, b in zip(frames[:-1], frames[1:])) and frames[-1] < T   # tiles the sequence
    ends = frames[1:] + [T]
    assert len(frames) == 1 or all(e - f >= D for f, e in zip(frames, ends))
    assert all(0 <= w < sc.shape[1] for w in words)
    assert M.path_score(sc, penalty, frames, words) == score


# ------------------------------------------------------------------ not GPU
def test_entry_point_and_timers_are_declared_exported_and_bound():
    hipabi = pkg('hipabi')
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'spkd.h')).read(), flags=re.S)
    lib = hipabi.load_library()
    name = 'spkd_mindur_viterbi_batch'
    assert re.search(r'\b%s\s*\(' % name, code)
    assert name in hipabi.EXPORTS and hasattr(lib, name) and hasattr(hipabi.Context, 'mindur_viterbi_batch')
    assert lib.spkd_abi_version() == 2 and re.search(r'#define SPKD_ABI_VERSION 2\b', code)
    enum = re.search(r'enum \{\s*SPKD_T_CALL = 0,(.*?)SPKD_N_TIMERS', code, flags=re.S).group(1)
    names = ['call'] + [n.strip()[len('SPKD_T_'):].lower() for n in enum.split(',') if n.strip()]
    # behind the resegmentation and linking timers, as those were added: the front-end's two stay last
    # (tests/test_mfcc_batch.py holds them there)
    at = names.index('clr_link')
    assert names[at + 1:at + 3] == ['mindur_viterbi', 'mindur_backtrack'] and len(names) == len(set(names))
    assert [n for n, _ in sorted(hipabi.TIMERS.items(), key=lambda kv: kv[1])] == names
    kern = open(os.path.join(ROOT, 'speaker-diarization_amd', 'csrc', 'spkd_mindur.hpp')).read()
    tile = int(re.search(r'#define SPKD_MINDUR_TILE (\d+)', code).group(1))
    assert tile == hipabi.MINDUR_TILE == int(re.search(r'constexpr int MD_TILE = (\d+);', kern).group(1))
    assert 'PARITY: no reference counterpart' in kern


def _refusals():
    """(name, call(lib, ctx handle) -> status) of every argument refusal of the entry point."""
    dev = C.c_void_p(4096)                        # never dereferenced: the refusal comes first
    keep = []

    def dec(n_seq=2, off=(0, 10, 30), n_cols=3, penalty=1.0, D=5, scores=dev, outs=(1, 1, 1, 1)):
        arr = None if off is None else np.array(off, dtype=np.int64)
        out = [C.c_void_p() for _ in range(4)]
        keep.append((arr, out))
        return lambda lib, h: lib.spkd_mindur_viterbi_batch(h, scores, n_seq, None if arr is None else _ptr(arr), n_cols,
                                                            penalty, D, *[C.byref(o) if k else None for o, k in zip(out, outs)])

    return [
        ('negative sequence count', dec(n_seq=-1)), ('null frame_off', dec(off=None)),
        ('frame_off not from 0', dec(off=(1, 10, 30))), ('frame_off decreases', dec(off=(0, 10, 9))),
        ('no column', dec(n_cols=0)), ('a 17th column', dec(n_cols=17)),
        ('negative penalty', dec(penalty=-1.0)), ('NaN penalty', dec(penalty=float('nan'))),
        ('infinite penalty', dec(penalty=float('inf'))),
        ('min_frames 0', dec(D=0)), ('min_frames negative', dec(D=-3)),
        ('null scores', dec(scores=None)),
        ('null tok_off', dec(outs=(0, 1, 1, 1))), ('null tok_frame', dec(outs=(1, 0, 1, 1))),
        ('null tok_word', dec(outs=(1, 1, 0, 1))), ('null score', dec(outs=(1, 1, 1, 0))),
    ]


def test_every_refusal_is_einval_without_a_context():
    hipabi = pkg('hipabi')
    lib = hipabi.load_library()
    for name, call in _refusals():
        assert call(lib, None) == hipabi.SPKD_EINVAL, name


@pytest.mark.parametrize('D', [1, 2, 3, 5])
def test_restatement_finds_the_brute_force_optimum(D):
    """Exact arithmetic (dyadic scores and penalties): the restated path's score is the optimum over
    all paths of stretches >= D, the tokens tile the sequence in stretches >= D (or are one stretch),
    and the score recomputed from the tokens is the reported one."""
    rng = np.random.default_rng(1000 + D)
    n = 0
    for W in (1, 2, 3):
        for T in _lengths(D) + [40]:
            for penalty in (0.0, 2.5, 50.0):
                for _ in range(3):
                    sc = _dyadic(rng, T, W)
                    frames, words, score = M.viterbi(sc, penalty, D)
                    assert score == M.brute_force(sc, penalty, D), (W, T, penalty)
                    _check_path(sc, penalty, D, frames, words, score)
                    n += 1
    assert n == 3 * 9 * 3 * 3
    # the degenerate input of the header: every window of every word holds a -inf -> one token (0, 0)
    sc = np.zeros((12, 2), dtype=np.float32)
    sc[0::2, 0] = -np.inf
    sc[1::2, 1] = -np.inf
    if D > 1:
        assert M.viterbi(sc, 1.0, D) == ([0], [0], -np.inf) and M.brute_force(sc, 1.0, D) == -np.inf


def test_min_duration_one_is_the_plain_decoder():
    """D = 1 on sums that are exact: tokens and score of spkd_vad_viterbi and of reseg_numpy.viterbi."""
    hipabi = pkg('hipabi')
    rng = np.random.default_rng(77)
    for W in (1, 2, 3):
        for T in (0, 1, 2, 3, 40):
            for penalty in (0.0, 2.5, 50.0):
                sc = _dyadic(rng, T, W)
                got = M.viterbi(sc, penalty, 1)
                want = R.viterbi(sc, penalty)
                assert got[0] == want[0] and got[1] == want[1], (W, T, penalty)
                assert got[2] == want[2], (W, T, penalty)
                if T:
                    zero = np.zeros(W)
                    tf, tw, score = hipabi.vad_viterbi(sc, np.arange(W), zero, zero, zero - penalty)
                    assert tf.tolist() == got[0] and tw.tolist() == got[1] and score == got[2]


def test_value_errors_come_before_any_device_work():
    pipeline = pkg('pipeline')
    assert pipeline.RESEG_MD == dict(penalty=50.0, min_dur_s=1.0) and pipeline.RESEG == dict(penalty=50.0)
    files = [pipeline.BatchFile(0, 1000, [(0.0, 8.0)])]
    labels = [np.array([1, 2])]
    for bad in (-1.0, float('nan'), float('inf'), -float('inf'), 'long'):
        with pytest.raises(ValueError, match='reseg min_dur_s'):
            pipeline.resegment_batch(None, 0, 1000, files, 0, [0, 2], labels, reseg=dict(penalty=50.0, min_dur_s=bad))
        with pytest.raises(ValueError, match='reseg min_dur_s'):
            pipeline.diarize_batch(None, 0, 0, [], reseg=dict(penalty=50.0, min_dur_s=bad))
    stage = pkg('resegmentation')
    assert stage._reseg_min_frames(dict(penalty=1.0), RATE) == 0
    assert stage._reseg_min_frames(dict(penalty=1.0, min_dur_s=0), RATE) == 0
    assert stage._reseg_min_frames(pipeline.RESEG_MD, RATE) == 125
    assert stage._reseg_min_frames(dict(min_dur_s=0.001), RATE) == 1                # never below one frame
    assert stage._reseg_min_frames(dict(min_dur_s=0.29), 100.0) == 28               # floor(0.29 * 100.0 = 28.999...)
    det = {}
    assert pipeline.diarize_batch(None, 0, 0, [], reseg=pipeline.RESEG_MD, detail=det) == []
    assert det['dropped'] == [] and det['passes_run'] == 0


class _StubContext(StubContext):
    """One canned decoding; records which decoder resegment_batch asks a context for, on which scores."""
    MS = {'mindur_viterbi': 0.25, 'mindur_backtrack': 0.125}

    def __init__(self, tokens):
        StubContext.__init__(self, [tokens])

    def dev_scratch(self, name, nbytes):
        return 4096

    def gauss_loglik(self, d_frames, n_frames, d_models, ok, b, e, m, k, n_cols, d_scores):
        self.calls.append(('gauss_loglik',))
        return self._frame_off(b, e)

    def vad_viterbi_batch(self, d_scores, frame_off, n_states, word_state, stay, exit_, enter):
        self.calls.append(('vad_viterbi_batch', d_scores, np.array(frame_off).tolist(), n_states, np.array(enter).tolist()))
        return self._answer()

    def mindur_viterbi_batch(self, d_scores, frame_off, n_cols, penalty, min_frames):
        self.calls.append(('mindur_viterbi_batch', d_scores, np.array(frame_off).tolist(), n_cols, penalty, min_frames))
        return self._answer()


def test_defaults_keep_the_plain_decoder_and_min_dur_takes_the_new_one():
    pipeline = pkg('pipeline')
    files = [pipeline.BatchFile(0, 1000, [(1.0, 3.0)])]
    labels = [np.array([2, 5])]
    tokens = [[(0, 1), (130, 0)]]
    for reseg in (pipeline.RESEG, dict(penalty=50.0, min_dur_s=0), dict(penalty=50.0, min_dur_s=0.0, passes=1)):
        stub, timings = _StubContext(tokens), {}
        plain = pipeline.resegment_batch(stub, 1 << 20, 1000, files, 1 << 21, [0, 2], labels, RATE, reseg, False, timings)
        assert [c[0] for c in stub.calls] == ['sum_stats', 'gauss_models', 'gauss_loglik', 'vad_viterbi_batch']
        assert stub.calls[-1][1:] == (4096, [0, 250], 2, [-50.0, -50.0])
        assert timings['reseg_viterbi'] == [0.5] and timings['reseg_backtrack'] == [0.5]
    stub, timings, det = _StubContext(tokens), {}, {}
    rows = pipeline.resegment_batch(stub, 1 << 20, 1000, files, 1 << 21, [0, 2], labels, RATE,
                                    dict(penalty=7.0, min_dur_s=0.5), False, timings, det)
    assert [c[0] for c in stub.calls] == ['sum_stats', 'gauss_models', 'gauss_loglik', 'mindur_viterbi_batch']
    assert stub.calls[-1][1:] == (4096, [0, 250], 2, 7.0, 62)                # the same scores and offsets; floor(0.5 * 125)
    assert timings['reseg_viterbi'] == [0.25] and timings['reseg_backtrack'] == [0.125]
    assert rows[0].tobytes() == plain[0].tobytes() and det['passes_run'] == 1        # the same row builder
    assert rows[0].tolist() == [[1.0, 1.0 + 130 / 125.0, 5.0], [1.0 + 130 / 125.0, 3.0, 2.0]]


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def ctx():
    c = pkg('hipabi').Context(0)
    yield c
    c.close()


# k_mindur_viterbi reads g back from its LDS ring below D = 2 MINDUR_TILE and from the prefetched
# scratch from there on: one below uses the whole ring, the boundary is the tightest case of the
# prefetch (one lane a sequence, a group with idle lanes, the widest group).  'ring', 'ring-1',
# 'ring+1': D relative to 2 * hipabi.MINDUR_TILE, read when the test runs.
_RING = {'ring-1': -1, 'ring': 0, 'ring+1': 1}
_WD = ([(W, D) for D in (1, 2, 31, 32, 33, 125) for W in (1, 2, 3, 8, 16)]
       + [(W, D) for D in _RING for W in (1, 3, 16)])


@pytest.mark.gpu
@pytest.mark.parametrize('W,D', _WD)
def test_device_is_the_restatement_to_the_bit(ctx, W, D):
    """About 70 ragged sequences in one call (several share a wave, more than one wave): tokens and
    scores of every sequence equal the restatement's, the scores to the bit."""
    if D in _RING:
        D = 2 * pkg('hipabi').MINDUR_TILE + _RING[D]
    rng = np.random.default_rng(100 * W + D)
    choice = _lengths(D) + [700]
    lens = [int(choice[i]) for i in rng.integers(0, len(choice), 70)]
    lens[3], lens[40], lens[69] = 700, 700, 0
    penalty = 0.0 if (W, D) in ((3, 33), (2, 125)) else float(rng.choice([1.0, 2.5, 50.0]))
    seqs = [_normal_scores(rng, T, W) for T in lens]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    flat = np.concatenate(seqs + [np.zeros((1, W), dtype=np.float32)])
    d = ctx.dev_alloc(flat.nbytes)
    try:
        ctx.h2d(d, flat)
        tok_off, tok_frame, tok_word, score = ctx.mindur_viterbi_batch(d, off, W, penalty, D)
        assert ctx.last_ms('mindur_viterbi') > 0.0 and ctx.last_ms('mindur_backtrack') > 0.0
    finally:
        ctx.dev_free(d)
    assert len(tok_off) == 71 and tok_off[0] == 0 and len(tok_frame) == len(tok_word) == tok_off[-1]
    for q, sc in enumerate(seqs):
        frames, words, want = M.viterbi(sc, penalty, D)
        a, b = int(tok_off[q]), int(tok_off[q + 1])
        assert tok_frame[a:b].tolist() == frames and tok_word[a:b].tolist() == words, (q, lens[q])
        assert np.float64(score[q]).tobytes() == np.float64(want).tobytes(), (q, lens[q])


@pytest.mark.gpu
def test_refusals_and_empty_calls_with_a_context(ctx):
    hipabi = pkg('hipabi')
    for name, call in _refusals():
        assert call(ctx.lib, ctx.h) == hipabi.SPKD_EINVAL, name
    tok_off, tok_frame, tok_word, score = ctx.mindur_viterbi_batch(0, [0], 3, 1.0, 5)
    assert tok_off.tolist() == [0] and len(tok_frame) == len(tok_word) == len(score) == 0
    tok_off, tok_frame, tok_word, score = ctx.mindur_viterbi_batch(0, [0, 0, 0], 3, 1.0, 5)
    assert tok_off.tolist() == [0, 0, 0] and len(tok_frame) == 0 and score.tolist() == [-np.inf, -np.inf]


@pytest.mark.gpu
@pytest.mark.parametrize('mindur_first', [False, True])
def test_neither_decoder_ends_the_results_of_the_other(ctx, mindur_first):
    """include/spkd.h: the arrays a decoder hands back live until the same call is made again.  The
    four arrays of one decoder, read through the pointers it returned, are what they were after the
    other decoder has run on other scores (3 sequences of 0, 40 and 100 frames, 3 words, D = 16)."""
    rng = np.random.default_rng(16)
    off = np.array([0, 0, 40, 140], dtype=np.int64)
    sc = [rng.normal(-60.0, 4.0, (140, 3)).astype(np.float32) for _ in range(2)]
    zero, enter, ws = np.zeros(3), np.full(3, -2.5), np.arange(3, dtype=np.int32)

    def raw(which, d):
        out = [C.c_void_p() for _ in range(4)]
        byref = [C.byref(o) for o in out]
        if which:
            st = ctx.lib.spkd_mindur_viterbi_batch(ctx.h, C.c_void_p(d), 3, _ptr(off), 3, 2.5, 16, *byref)
        else:
            st = ctx.lib.spkd_vad_viterbi_batch(ctx.h, C.c_void_p(d), 3, _ptr(off), 3, 3, _ptr(ws), _ptr(zero), _ptr(zero),
                                                _ptr(enter), *byref)
        assert st == 0
        return out

    def read(out):
        n_tok = int(np.ctypeslib.as_array(C.cast(out[0], C.POINTER(C.c_int64)), shape=(4,))[3])
        return [np.ctypeslib.as_array(C.cast(o, C.POINTER(t)), shape=(n,)).copy()
                for o, t, n in zip(out, (C.c_int64, C.c_int64, C.c_int32, C.c_double), (4, n_tok, n_tok, 3))]

    d = [ctx.dev_alloc(a.nbytes) for a in sc]
    try:
        for p, a in zip(d, sc):
            ctx.h2d(p, a)
        kept = raw(mindur_first, d[0])
        first = read(kept)
        assert first[0][0] == 0 and first[0][3] >= 2 and first[3][0] == -np.inf and np.isfinite(first[3][1:]).all()
        other = read(raw(not mindur_first, d[1]))
        again = read(kept)
    finally:
        for p in d:
            ctx.dev_free(p)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    assert other[3].tolist() != first[3].tolist()                          # (it was another decode)


@pytest.fixture(scope='module')
def batch():
    """Two 40 s files of 2 and 3 close speakers (turns >= 3 s) resident on the device, their truth
    segments' records and labels."""
    b = Batch([_close_session(7000, 40.0, 2), _close_session(7001, 40.0, 3)])
    yield b
    b.close()


def _frame_errors(batch, rows):
    """Frames of the turns whose row carries another speaker than the generator's truth."""
    wrong = 0
    for f, (feats, vad, truth) in enumerate(batch.sess):
        want, got = np.full(len(feats), -1), np.full(len(feats), -1)
        for s, e, k in truth:
            want[s:e] = k + 1
        for s, e, lab in rows[f]:
            got[int(round(s * RATE)):int(round(e * RATE))] = int(lab)
        wrong += int((got != want).sum())
    return wrong


def _rows_of_the_restated_decoder(batch, reseg):
    """The rows of a pass from the scores the device left, decoded on the host (as test_reseg_batch
    compares a pass): reseg_mindur_numpy.viterbi with a minimum duration, spkd_vad_viterbi without."""
    p, ctx, hipabi = batch.pipeline, batch.ctx, batch.hipabi
    owner, _, _, ls, le, tb, te = p._turn_table(batch.files, RATE)
    n_cols = 3
    sc = np.empty((int((te - tb).sum()), n_cols), dtype=np.float32)
    ctx.d2h(sc, ctx.dev_scratch('reseg_scores', 0))
    off = np.concatenate([[0], np.cumsum(te - tb)])
    D = pkg('resegmentation')._reseg_min_frames(reseg, RATE)
    want = [[] for _ in batch.files]
    for q in range(len(owner)):
        f = int(owner[q])
        if D:
            tf, tw, _ = M.viterbi(sc[off[q]:off[q + 1]], reseg['penalty'], D)
        else:
            zero = np.zeros(n_cols)
            tf, tw, _ = hipabi.vad_viterbi(sc[off[q]:off[q + 1]], np.arange(n_cols), zero, zero, zero - reseg['penalty'])
            tf, tw = tf.tolist(), tw.tolist()
        labs = sorted(set(batch.labels[f].tolist()))
        want[f].append(R.rows_of_turn(tf, tw, float(ls[q]), float(le[q]), labs + [0] * 3, RATE, False))
    return [np.concatenate(w) for w in want]


@pytest.mark.gpu
def test_min_duration_in_the_pipeline(batch):
    """reseg = dict(penalty=0.0, min_dur_s=1.0) against the same call without min_dur_s.  Measured on
    the restatement (CPU, float64 scores): 1134 wrong frames in the turns without the minimum duration,
    hundreds of rows shorter than 125 frames; 2 wrong frames with it."""
    p, ctx = batch.pipeline, batch.ctx
    args = (ctx, batch.eng.d_frames, batch.frames.shape[0], batch.files, batch.d_stats, batch.seg_off, batch.labels, RATE)
    md, plain0 = dict(penalty=0.0, min_dur_s=1.0), dict(penalty=0.0)
    timings, det = {}, {}
    rows = p.resegment_batch(*args, md, False, timings, det)
    assert det['dropped'] == [] and det['passes_run'] == 1
    assert all(len(timings[k]) == 1 and timings[k][0] > 0.0 for k in ('reseg_viterbi', 'reseg_backtrack'))
    want = _rows_of_the_restated_decoder(batch, md)
    for f in range(2):
        assert rows[f].shape == want[f].shape
        assert rows[f][:, :2].tobytes() == want[f][:, :2].tobytes() and np.array_equal(rows[f][:, 2], want[f][:, 2])
        k = 0
        for a, b in batch.sess[f][1]:                                      # rows tile each turn, none short
            n = int(((rows[f][:, 0] >= a / RATE) & (rows[f][:, 0] < b / RATE)).sum())
            r = rows[f][k:k + n]
            assert r[0, 0] == a / RATE and r[-1, 1] == b / RATE and r[1:, 0].tobytes() == r[:-1, 1].tobytes()
            length = np.rint((r[:, 1] - r[:, 0]) * RATE)
            assert n == 1 or (length >= 125).all()
            k += n
        assert k == len(rows[f])
    plain = p.resegment_batch(*args, plain0, False)
    want = _rows_of_the_restated_decoder(batch, plain0)
    for f in range(2):
        assert plain[f].tobytes() == want[f].tobytes()                      # today's rows
    short = sum(int((np.rint((r[:, 1] - r[:, 0]) * RATE) < 125).sum()) for r in plain)
    assert short >= 1                                                       # what the key is for
    e_md, e_plain = _frame_errors(batch, rows), _frame_errors(batch, plain)
    print('wrong frames: %d with min_dur_s=1.0, %d without (penalty 0); %d short rows without' % (e_md, e_plain, short))
    assert e_md <= e_plain
    # min_dur_s = 0 is the key's absence
    zero = p.resegment_batch(*args, dict(penalty=0.0, min_dur_s=0.0), False)
    assert [r.tobytes() for r in zero] == [r.tobytes() for r in plain]


@pytest.mark.gpu
def test_diarize_batch_with_min_duration_and_link(batch):
    p, ctx = batch.pipeline, batch.ctx
    args = (ctx, batch.eng.d_frames, batch.frames.shape[0], batch.files)
    det = {}
    got = p.diarize_batch(*args, rate=RATE, reseg=p.RESEG_MD, detail=det)
    assert det['passes_run'] == 1 and all(len(r) for r in got)
    for f, r in enumerate(got):
        length = np.rint((r[:, 1] - r[:, 0]) * RATE)
        turns = {(a / RATE, b / RATE) for a, b in batch.sess[f][1]}
        assert all(n >= 125 or (s, e) in turns for n, (s, e) in zip(length, r[:, :2].tolist()))
    det = {}
    linked = p.diarize_batch(*args, rate=RATE, reseg=p.RESEG_MD, link=p.LINK_CL, detail=det)
    maps = det['link']['maps']
    for f in range(2):
        assert linked[f][:, :2].tobytes() == got[f][:, :2].tobytes()
        assert np.array_equal(linked[f][:, 2], maps[f][got[f][:, 2].astype(np.int64)])
    # the existing settings go through the calls they made before
    assert [r.tobytes() for r in p.diarize_batch(*args, rate=RATE, reseg=dict(penalty=50.0, min_dur_s=0))] == \
        [r.tobytes() for r in p.diarize_batch(*args, rate=RATE, reseg=p.RESEG)]
