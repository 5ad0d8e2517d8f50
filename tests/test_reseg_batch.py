"""Viterbi resegmentation of a batch's speakers: spkd_gauss_models (records -> full-covariance
Gaussian models), spkd_gauss_loglik (every frame of every turn under the speakers of its file),
pipeline.resegment_batch and diarize_batch(..., reseg=...).  PARITY: no reference counterpart; the
numpy restatement is tests/reseg_numpy.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import reseg_numpy as R
from helpers import ROOT
from conftest import pkg
from reseg_helpers import Batch, Dev as _Dev, StubContext, displaced as _displaced, ptr as _ptr

RATE = 125.0
TILE = 64


def _close(got, want, rel=1e-9):
    """The bar test_oracle_golden.py holds the numpy oracle to: 1e-9 relative, floored at 1."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool((np.abs(got - want) <= rel * np.maximum(1.0, np.maximum(np.abs(got), np.abs(want)))).all())


# ------------------------------------------------------------------ not GPU
def test_entry_points_and_timers_are_declared_and_exported():
    hipabi = pkg('hipabi')
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'spkd.h')).read(), flags=re.S)
    lib = hipabi.load_library()
    for name in ('spkd_gauss_models', 'spkd_gauss_loglik'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in hipabi.EXPORTS and hasattr(lib, name)
    assert lib.spkd_abi_version() == 2 and re.search(r'#define SPKD_ABI_VERSION 2\b', code)
    enum = re.search(r'enum \{\s*SPKD_T_CALL = 0,(.*?)SPKD_N_TIMERS', code, flags=re.S).group(1)
    names = ['call'] + [n.strip()[len('SPKD_T_'):].lower() for n in enum.split(',') if n.strip()]
    assert 'gauss_models' in names and 'gauss_loglik' in names
    assert [n for n, _ in sorted(hipabi.TIMERS.items(), key=lambda kv: kv[1])] == names
    # tile and model size are named constants: header, kernels, binding and restatement agree
    kern = open(os.path.join(ROOT, 'speaker-diarization_amd', 'csrc', 'spkd_gauss.hpp')).read()
    tile = int(re.search(r'#define SPKD_GAUSS_TILE (\d+)', code).group(1))
    assert tile == hipabi.GAUSS_TILE == TILE == int(re.search(r'constexpr int GS_TILE = (\d+);', kern).group(1))
    model = int(re.search(r'#define SPKD_GAUSS_MODEL (\d+)', code).group(1))
    assert model == hipabi.GAUSS_MODEL == R.MODEL == int(re.search(r'constexpr int GS_MODEL = (\d+);', kern).group(1))
    assert hasattr(hipabi.Context, 'gauss_models') and hasattr(hipabi.Context, 'gauss_loglik')
    assert 'PARITY: no reference counterpart' in kern


def _refusals():
    """(name, call(lib, ctx handle) -> status) of every argument refusal of the two entry points."""
    dev = C.c_void_p(4096)                        # never dereferenced: the refusal comes first
    odd = C.c_void_p(4104)
    ok = np.ones(4, dtype=np.int32)
    keep = {}

    def lik(n_frames=100, models=dev, n_models=4, h_ok=ok, n_seq=2, b=(0, 10), e=(10, 100), m=(0, 1), k=(1, 3),
            n_cols=4, frames=dev, scores=dev):
        arr = [None if v is None else np.array(v, dtype=t) for v, t in
               ((b, np.int64), (e, np.int64), (m, np.int32), (k, np.int32))]
        keep[len(keep)] = arr
        p = [None if a is None else _ptr(a) for a in arr]
        return lambda lib, h: lib.spkd_gauss_loglik(h, frames, n_frames, models, n_models,
                                                    None if h_ok is None else _ptr(h_ok), n_seq, p[0], p[1], p[2], p[3],
                                                    n_cols, scores)

    out = [
        ('models: null records', lambda lib, h: lib.spkd_gauss_models(h, None, 2, dev, _ptr(ok))),
        ('models: null models', lambda lib, h: lib.spkd_gauss_models(h, dev, 2, None, _ptr(ok))),
        ('models: null ok', lambda lib, h: lib.spkd_gauss_models(h, dev, 2, dev, None)),
        ('models: negative count', lambda lib, h: lib.spkd_gauss_models(h, dev, -1, dev, _ptr(ok))),
        ('models: misaligned records', lambda lib, h: lib.spkd_gauss_models(h, odd, 2, dev, _ptr(ok))),
        ('models: misaligned models', lambda lib, h: lib.spkd_gauss_models(h, dev, 2, odd, _ptr(ok))),
        ('loglik: null frames', lik(frames=None)), ('loglik: null models', lik(models=None)),
        ('loglik: null ok', lik(h_ok=None)), ('loglik: null scores', lik(scores=None)),
        ('loglik: null begin', lik(b=None)), ('loglik: null end', lik(e=None)),
        ('loglik: null first model', lik(m=None)), ('loglik: null model count', lik(k=None)),
        ('loglik: negative sequence count', lik(n_seq=-1)),
        ('loglik: no column', lik(n_cols=0)), ('loglik: a 17th column', lik(n_cols=17, k=(1, 17), n_models=40)),
        ('loglik: more models than columns', lik(k=(1, 5), n_models=8)),
        ('loglik: begin below 0', lik(b=(-1, 10))), ('loglik: end past the frames', lik(e=(10, 101))),
        ('loglik: end before begin', lik(b=(0, 50), e=(10, 49))),
        ('loglik: model below 0', lik(m=(-1, 1))), ('loglik: model past the models', lik(m=(0, 2))),
        ('loglik: misaligned models', lik(models=odd)),
    ]
    return out


def test_every_refusal_is_einval_without_a_context():
    hipabi = pkg('hipabi')
    lib = hipabi.load_library()
    for name, call in _refusals():
        assert call(lib, None) == hipabi.SPKD_EINVAL, name


def test_restated_decoder_is_the_host_decoder():
    """reseg_numpy.viterbi against spkd_vad_viterbi with stay = exit = 0, enter = -penalty: tokens
    equal, score bit-equal, on random scores with planted ties, -inf columns, all--inf frames, NaNs."""
    hipabi = pkg('hipabi')
    rng = np.random.default_rng(20261018)
    for W, T, pen in ((1, 40, 5.0), (2, 300, 0.0), (3, 500, 2.5), (4, 700, 50.0), (16, 200, 1.0)):
        sc = rng.normal(-100.0, 3.0, (T, W)).astype(np.float32)
        sc = np.round(sc * 2.0) / 2.0 if W > 1 else sc                     # a coarse grid: exact ties
        sc = sc.astype(np.float32)
        if W > 2:
            sc[:, 1] = -np.inf                                             # a speaker that is not ok
            sc[T // 3:T // 3 + 5] = -np.inf                                # frames nobody can score
            sc[T // 2, 0] = np.nan
        sc[5:9] = sc[4]                                                    # repeated frames
        zero = np.zeros(W)
        tf, tw, score = hipabi.vad_viterbi(sc, np.arange(W), zero, zero, zero - pen)
        frames, words, want = R.viterbi(sc, pen)
        assert tf.tolist() == frames and tw.tolist() == words, W
        assert np.float64(score).tobytes() == np.float64(want).tobytes(), W
        assert all(a != b for a, b in zip(words[:-1], words[1:]))          # never re-enters the word it is in
    assert R.viterbi(np.zeros((0, 3), dtype=np.float32), 1.0) == ([], [], -np.inf)


@pytest.mark.parametrize('penalty', [10.0, 50.0, 200.0])
def test_restatement_moves_displaced_boundaries_back(penalty):
    """What the stage is for: segments labelled by truth but with every boundary inside a turn 100
    frames late give contaminated models; decoding under them puts every boundary back."""
    synth = pkg('synth')
    feats, vad, truth = synth.make_session(1234, 60.0, 3)
    segs = _displaced(truth, vad)
    assert [s[:2] for s in segs] != [t[:2] for t in truth]
    spk = sorted(set(t[2] for t in truth))
    models = [R.model_from_record(sum(R.record_of_frames(feats[s:e]) for s, e, k in segs if k == sp)) for sp in spk]
    assert all(m[3] for m in models)
    right = total = n_rows = 0
    for a, b in vad:
        inside = [t for t in truth if a <= t[0] and t[1] <= b]
        sc = R.scores(feats[a:b], [m[:3] for m in models], [True] * 3, 3).astype(np.float32)
        frames, words, _ = R.viterbi(sc, penalty)
        assert [a + f for f in frames] == [t[0] for t in inside]           # worst boundary error: 0
        assert [spk[w] for w in words] == [t[2] for t in inside]
        got = np.repeat([spk[w] for w in words], np.diff(frames + [b - a]))
        want = np.concatenate([np.full(e - s, k) for s, e, k in inside])
        right += int((got == want).sum())
        total += b - a
        n_rows += len(frames)
    assert (right, total) == (7125, 7125) and n_rows == len(truth)


def test_rows_of_a_turn():
    rows = R.rows_of_turn([0, 30, 31], [2, 0, 1], 1.0, 3.0, [4, 7, 9], 125.0, False)
    assert rows.tolist() == [[1.0, 1.0 + 30 / 125.0, 9.0], [1.0 + 30 / 125.0, 1.0 + 31 / 125.0, 4.0],
                             [1.0 + 31 / 125.0, 3.0, 7.0]]
    third = R.rows_of_turn([0, 1], [0, 1], 1.0 / 3.0, 2.0 / 3.0, [1, 2], 125.0, True)
    assert third[0, 0] == 0.333333333333 and third[1, 1] == 0.666666666667
    assert R.rows_of_turn([], [], 0.0, 1.0, [1], 125.0, True).shape == (0, 3)


class _StubContext(StubContext):
    """One canned decoding; every call with all its arguments, the scratch requests among them."""

    def __init__(self, ok, tokens):
        StubContext.__init__(self, [tokens], [ok])
        self.tokens = tokens

    def dev_scratch(self, name, nbytes):
        self.calls.append(('dev_scratch', name, nbytes))
        return self.SCRATCH[name]

    def sum_stats(self, d_src, n_src, member, set_off, d_dst):
        self.calls.append(('sum_stats', d_src, n_src, np.array(member).tolist(), np.array(set_off).tolist(), d_dst))

    def gauss_loglik(self, d_frames, n_frames, d_models, ok, b, e, m, k, n_cols, d_scores):
        self.calls.append(('gauss_loglik', d_frames, n_frames, d_models, np.array(ok).tolist(), np.array(b).tolist(),
                           np.array(e).tolist(), np.array(m).tolist(), np.array(k).tolist(), n_cols, d_scores))
        return self._frame_off(b, e)

    def vad_viterbi_batch(self, d_scores, frame_off, n_states, word_state, stay, exit_, enter):
        self.calls.append(('vad_viterbi_batch', d_scores, np.array(frame_off).tolist(), n_states,
                           np.array(word_state).tolist(), np.array(stay).tolist(), np.array(exit_).tolist(),
                           np.array(enter).tolist()))
        return self._answer()


def test_stages_and_rows_on_the_host():
    pipeline, hipabi = pkg('pipeline'), pkg('hipabi')
    # file 0: labels 2 and 5, two turns (the second without frames); file 1: no segment; file 2: labels 1, 2, 3
    files = [pipeline.BatchFile(0, 1000, [(1.0, 3.0), (9.0, 9.5)]), pipeline.BatchFile(1000, 500, [(0.0, 2.0)]),
             pipeline.BatchFile(1500, 1000, [(0.5, 6.0)])]
    labels = [np.array([5, 2, 5]), np.zeros(0, dtype=np.int32), np.array([3, 1, 2, 1])]
    stub = _StubContext([1, 1, 1, 0, 1], [[(0, 1), (100, 0)], [], [(0, 2), (7, 0), (300, 2)]])
    timings, det = {}, {}
    rows = pipeline.resegment_batch(stub, 1 << 20, 2500, files, 1 << 21, [0, 3, 3, 7], labels, 125.0, dict(penalty=7.0),
                                    False, timings, det)
    assert [c[0] for c in stub.calls] == ['dev_scratch', 'sum_stats', 'dev_scratch', 'gauss_models', 'dev_scratch',
                                          'gauss_loglik', 'vad_viterbi_batch']
    assert stub.calls[1][1:] == (1 << 21, 7, [1, 0, 2, 4, 6, 5, 3], [0, 1, 3, 5, 6, 7], 4096)
    assert stub.calls[0][2] == 5 * hipabi.REC * 8 and stub.calls[2][2] == 5 * hipabi.GAUSS_MODEL * 8
    assert stub.calls[3][1:] == (4096, 5, 8192)
    assert stub.calls[4][2] == (250 + 0 + 688) * 3 * 4
    # the turns of the files with speakers, absolute frames; the file's first model and its count; 3 columns
    assert stub.calls[5][1:] == (1 << 20, 2500, 8192, [1, 1, 1, 0, 1], [125, 1000, 1562], [375, 1000, 2250], [0, 0, 2],
                                 [2, 2, 3], 3, 12288)
    assert stub.calls[6][1:] == (12288, [0, 250, 250, 938], 3, [0, 1, 2], [0.0] * 3, [0.0] * 3, [-7.0] * 3)
    assert rows[0].tolist() == [[1.0, 1.0 + 100 / 125.0, 5.0], [1.0 + 100 / 125.0, 3.0, 2.0]]
    assert rows[1].shape == (0, 3)
    assert rows[2].tolist() == [[0.5, 0.5 + 7 / 125.0, 3.0], [0.5 + 7 / 125.0, 0.5 + 300 / 125.0, 1.0],
                                [0.5 + 300 / 125.0, 6.0, 3.0]]
    assert det['dropped'] == [(2, 2)]
    assert all(timings[k] == [0.5] for k in ('reseg_models', 'reseg_loglik', 'reseg_viterbi', 'reseg_backtrack'))
    # the same rows as the restatement's builder, with the text contract too
    stub = _StubContext([1] * 5, stub.tokens)
    rows = pipeline.resegment_batch(stub, 1 << 20, 2500, files, 1 << 21, [0, 3, 3, 7], labels, 125.0 / 3.0)
    want = R.rows_of_turn([0, 7, 300], [2, 0, 2], 0.5, 6.0, [1, 2, 3], 125.0 / 3.0, True)
    assert rows[2].tobytes() == want.tobytes()


def test_refusals_of_the_pipeline_need_no_device():
    pipeline = pkg('pipeline')
    assert pipeline.RESEG == dict(penalty=50.0)
    for kw in (dict(handoff='device', fused=True), dict(fused=True), dict(handoff='device')):
        with pytest.raises(ValueError, match='reseg takes the host hand-off'):
            pipeline.diarize_batch(None, 0, 0, [], reseg=pipeline.RESEG, **kw)
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='reseg penalty'):
            pipeline.diarize_batch(None, 0, 0, [], reseg=dict(penalty=bad))
        with pytest.raises(ValueError, match='reseg penalty'):
            pipeline.resegment_batch(None, 0, 0, [], 0, [0], [], reseg=dict(penalty=bad))
    # a 17th speaker in one file: refused before the context is touched
    files = [pipeline.BatchFile(0, 1000, [(0.0, 8.0)]), pipeline.BatchFile(1000, 1000, [(0.0, 8.0)])]
    with pytest.raises(ValueError, match='at most 16 speakers'):
        pipeline.resegment_batch(None, 0, 2000, files, 0, [0, 2, 19], [np.array([1, 2]), np.arange(1, 18)])
    # nothing to decode: no device work either
    det = {}
    assert pipeline.diarize_batch(None, 0, 0, [], reseg=pipeline.RESEG, detail=det) == [] and det['dropped'] == []
    out = pipeline.resegment_batch(None, 0, 2000, files, 0, [0, 0, 0], [np.zeros(0, int)] * 2, detail=det)
    assert [o.shape for o in out] == [(0, 3)] * 2 and det['dropped'] == []
    quiet = [pipeline.BatchFile(0, 1000, [])]
    assert pipeline.resegment_batch(None, 0, 1000, quiet, 0, [0, 2], [np.array([1, 2])])[0].shape == (0, 3)


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def one():
    """One 60 s session of two speakers and 64 constant frames behind it."""
    feats = pkg('synth').make_session(909, 60.0, 2)[0]
    d = _Dev(np.concatenate([feats, np.repeat(feats[777:778], 64, axis=0)]))
    yield d
    d.close()


@pytest.mark.gpu
def test_models_match_the_restatement(one):
    hipabi, ctx = one.hipabi, one.ctx
    ranges = [(200, 700), (1000, 6000), (300, 330), (300, 301), (7500, 7564)]
    d_rec = one.records(ranges)
    rec = np.empty((5, hipabi.REC))
    ctx.d2h(rec, d_rec)
    assert rec[:, 819].tolist() == [500, 5000, 30, 1, 64]
    d_models = one.alloc(5 * hipabi.GAUSS_MODEL * 8)
    ok = ctx.gauss_models(d_rec, 5, d_models)
    assert ok.tolist() == [1, 1, 0, 0, 0]
    assert ctx.last_ms('gauss_models') > 0.0
    got = np.empty((5, hipabi.GAUSS_MODEL))
    ctx.d2h(got, d_models)
    for i in range(5):
        mu, w, c, good = R.model_from_record(rec[i])
        assert good == bool(ok[i]), i
        if good:
            gmu, gw, gc = R.unpack_model(got[i])
            err = [float(np.abs(np.asarray(a) - np.asarray(b)).max()) for a, b in ((gmu, mu), (gw, w), (gc, c))]
            print('record %d: max abs error mu %.3g, W %.3g, c %.3g' % (i, err[0], err[1], err[2]))
            assert _close(gmu, mu) and _close(gw, w) and _close(gc, c), i
            assert _close(got[i], R.pack_model(mu, w, c))
    # a record that is not finite, and digital silence: not ok, and no error status
    bad = rec[:2].copy()
    bad[0, 17] = np.nan
    bad[1, :] = 0.0
    bad[1, 819] = 500.0
    ctx.h2d(d_rec, bad)
    assert ctx.gauss_models(d_rec, 2, d_models).tolist() == [0, 0]
    assert ctx.lib.spkd_gauss_models(ctx.h, C.c_void_p(d_rec), 0, C.c_void_p(d_models), None) == hipabi.SPKD_OK
    for name, call in _refusals():
        assert call(ctx.lib, ctx.h) == hipabi.SPKD_EINVAL, name


@pytest.mark.gpu
def test_scores_match_the_restatement_to_an_ulp(one):
    hipabi, ctx = one.hipabi, one.ctx
    n_frames = one.frames.shape[0]
    # file A: one speaker; file B: three, the second of them (30 frames) not ok
    d_rec = one.records([(200, 700), (1000, 3000), (300, 330), (4000, 6000)])
    d_models = one.alloc(4 * hipabi.GAUSS_MODEL * 8)
    ok = ctx.gauss_models(d_rec, 4, d_models)
    assert ok.tolist() == [1, 1, 0, 1]
    packed = np.empty((4, hipabi.GAUSS_MODEL))
    ctx.d2h(packed, d_models)                                              # the device's models: their error is excluded
    models = [R.unpack_model(v) for v in packed]
    lens = [1, 2, TILE - 1, TILE, TILE + 1, 0, 2 * TILE + 1, 777]
    begin = np.array([5000, 4990, 3000, 3100, 2000, 2500, n_frames - (2 * TILE + 1), 100], dtype=np.int64)
    end = begin + lens
    assert int(end.max()) == n_frames and sorted(begin.tolist()) != begin.tolist()
    owner_b = np.array([0, 1, 1, 0, 1, 1, 1, 1], dtype=bool)
    first, count = np.where(owner_b, 1, 0), np.where(owner_b, 3, 1)
    total, n_cols, pad = int(sum(lens)), 4, 8
    nan_row = int(np.cumsum(lens)[6]) + 300                                # a frame of the last sequence
    frames = one.frames.copy()
    frames[100 + 300, 7] = np.nan
    d_frames = one.alloc(frames.nbytes)
    ctx.h2d(d_frames, frames)
    d_scores = one.alloc((total + pad) * n_cols * 4)
    mark = np.full((total + pad, n_cols), 12345.0, dtype=np.float32)
    ctx.h2d(d_scores, mark)
    off = ctx.gauss_loglik(d_frames, n_frames, d_models, ok, begin, end, first, count, n_cols, d_scores)
    assert off.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
    assert ctx.last_ms('gauss_loglik') > 0.0
    got = np.empty_like(mark)
    ctx.d2h(got, d_scores)
    assert np.array_equal(got[total:], mark[total:])                       # rows beyond the total: untouched
    want = np.full((total, n_cols), -np.inf)
    for q in range(len(lens)):
        k = int(count[q])
        want[off[q]:off[q + 1], :k] = R.scores(frames[begin[q]:end[q]], models[first[q]:first[q] + k],
                                               ok[first[q]:first[q] + k], k)
    want32 = want.astype(np.float32)
    inf = np.isinf(want32)
    assert np.array_equal(np.isneginf(got[:total]), inf)
    rows_b = np.repeat(owner_b, lens)
    assert inf[rows_b][:, [1, 3]].all() and not inf[rows_b][:, [0, 2]].any()     # not ok, padding
    assert inf[~rows_b][:, 1:].all() and not inf[~rows_b][:, 0].any()
    nan = np.isnan(got[:total])
    assert np.array_equal(nan, np.isnan(want32)) and np.nonzero(nan.any(axis=1))[0].tolist() == [nan_row]
    assert nan[nan_row].tolist() == [True, False, True, False]
    fin = np.isfinite(want32)
    ulps = np.abs(got[:total][fin].view(np.int32).astype(np.int64) - want32[fin].view(np.int32).astype(np.int64))
    print('%d finite scores in %.1f .. %.1f, %d differ from float32(restatement), worst %d ulp' % (
        fin.sum(), want32[fin].min(), want32[fin].max(), int((ulps > 0).sum()), int(ulps.max())))
    assert int(ulps.max()) <= 1
    # nothing to score: SPKD_OK, nothing written
    ctx.h2d(d_scores, mark)
    assert ctx.gauss_loglik(d_frames, n_frames, d_models, ok, [7, 9], [7, 9], [0, 1], [1, 3], n_cols, d_scores).tolist() == [0, 0, 0]
    assert ctx.gauss_loglik(d_frames, n_frames, d_models, ok, [], [], [], [], n_cols, d_scores).tolist() == [0]
    with pytest.raises(hipabi.SpkdError) as ei:
        ctx.gauss_loglik(d_frames, n_frames, d_models, ok, [0, 10], [10, n_frames + 1], [0, 1], [1, 3], n_cols, d_scores)
    assert ei.value.status == hipabi.SPKD_EINVAL
    ctx.d2h(got, d_scores)
    assert np.array_equal(got, mark)


@pytest.fixture(scope='module')
def three():
    """Three 60 s files of 2, 3 and 4 speakers as one batch, their truth segments' records."""
    synth = pkg('synth')
    d = Batch([synth.make_session(4100 + k, 60.0, k) for k in (2, 3, 4)])
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize('text_contract', [True, False])
def test_rows_are_the_host_decoder_on_the_device_scores(three, text_contract):
    p, ctx, hipabi = three.pipeline, three.ctx, three.hipabi
    timings, det = {}, {}
    rows = p.resegment_batch(ctx, three.eng.d_frames, three.frames.shape[0], three.files, three.d_stats, three.seg_off,
                             three.labels, RATE, p.RESEG, text_contract, timings, det)
    assert det['dropped'] == [] and all(len(timings[k]) == 1 for k in
                                        ('reseg_models', 'reseg_loglik', 'reseg_viterbi', 'reseg_backtrack'))
    owner, _, _, ls, le, tb, te = p._turn_table(three.files, RATE)
    total, n_cols = int((te - tb).sum()), max(len(set(l.tolist())) for l in three.labels)
    assert n_cols == 4
    sc = np.empty((total, n_cols), dtype=np.float32)
    ctx.d2h(sc, ctx.dev_scratch('reseg_scores', 0))
    off = np.concatenate([[0], np.cumsum(te - tb)])
    zero = np.zeros(n_cols)
    want = [[] for _ in three.files]
    for q in range(len(owner)):
        f = int(owner[q])
        tf, tw, _ = hipabi.vad_viterbi(sc[off[q]:off[q + 1]], np.arange(n_cols), zero, zero, zero - 50.0)
        labs = sorted(set(three.labels[f].tolist()))
        want[f].append(R.rows_of_turn(tf.tolist(), tw.tolist(), float(ls[q]), float(le[q]), labs + [0] * 4, RATE, text_contract))
    for f in range(3):
        w = np.concatenate(want[f])
        assert rows[f].shape == w.shape and len(w) >= len(three.sess[f][1])
        assert rows[f][:, :2].tobytes() == w[:, :2].tobytes()
        assert np.array_equal(rows[f][:, 2], w[:, 2]) and rows[f][:, 2].min() >= 1


@pytest.mark.gpu
def test_stage_moves_displaced_boundaries_back_on_the_device():
    synth, pipeline = pkg('synth'), pkg('pipeline')
    feats, vad, truth = synth.make_session(1234, 60.0, 3)
    segs = _displaced(truth, vad)
    d = _Dev(feats)
    try:
        d_stats = d.records([(a, b) for a, b, _ in segs])
        files = [pipeline.BatchFile(0, len(feats), [(a / RATE, b / RATE) for a, b in vad])]
        labels = [np.array([k + 1 for _, _, k in segs])]
        rows = pipeline.resegment_batch(d.ctx, d.eng.d_frames, len(feats), files, d_stats, [0, len(segs)], labels, RATE,
                                        pipeline.RESEG, False)[0]
        starts = np.rint(rows[:, 0] * RATE).astype(np.int64)
        assert np.abs(rows[:, 0] * RATE - starts).max() < 1e-6
        assert starts.tolist() == [t[0] for t in truth]                    # every boundary back on its true frame
        assert rows[:, 2].tolist() == [t[2] + 1 for t in truth]
        k = 0
        for a, b in vad:                                                   # the rows tile each turn
            n = len([t for t in truth if a <= t[0] and t[1] <= b])
            r = rows[k:k + n]
            assert r[0, 0] == a / RATE and r[-1, 1] == b / RATE
            assert r[1:, 0].tobytes() == r[:-1, 1].tobytes() and (r[:, 1] > r[:, 0]).all()
            assert (r[1:, 2] != r[:-1, 2]).all()
            k += n
        assert k == len(rows)
    finally:
        d.close()


@pytest.mark.gpu
def test_diarize_batch_with_reseg(three):
    p, ctx = three.pipeline, three.ctx
    f0, f1, f2 = three.files
    files = [f0, p.BatchFile(f1.frame_off, f1.n_frames, []), f1, f2]       # a file with no turns inside the batch
    args = (ctx, three.eng.d_frames, three.frames.shape[0], files)
    plain = p.diarize_batch(*args, rate=RATE)
    none = p.diarize_batch(*args, rate=RATE, reseg=None)
    assert [r.tobytes() for r in none] == [r.tobytes() for r in plain]
    det = {}
    got = p.diarize_batch(*args, rate=RATE, reseg=p.RESEG, detail=det)
    assert det['dropped'] == [] and got[1].shape == (0, 3) and all(len(got[i]) for i in (0, 2, 3))
    # the stages one by one
    segs = p.change_detect_batch(ctx, three.eng.d_frames, three.frames.shape[0], files, RATE)
    box = []
    res = p.cluster_batch(ctx, three.eng.d_frames, three.frames.shape[0], files, segs, RATE, stats_out=box)
    labels = [lab for lab, _ in res]
    want = p.resegment_batch(ctx, three.eng.d_frames, three.frames.shape[0], files, box[0][0], box[0][1], labels, RATE)
    assert [r.tobytes() for r in got] == [r.tobytes() for r in want]
    for f, r in enumerate(got):
        assert set(r[:, 2].astype(int).tolist()) <= set(labels[f].tolist())
    # another detector goes through the same path
    r = p.diarize_batch(*args, rate=RATE, reseg=p.RESEG, cd=p.SW_CD)
    assert r[1].shape == (0, 3) and all(len(r[i]) for i in (0, 2, 3))
    # with link: the third column through the maps, the times untouched
    det = {}
    linked = p.diarize_batch(*args, rate=RATE, reseg=p.RESEG, link=p.LINK_CL, detail=det)
    maps = det['link']['maps']
    for f in range(4):
        assert linked[f][:, :2].tobytes() == got[f][:, :2].tobytes()
        assert np.array_equal(linked[f][:, 2], maps[f][got[f][:, 2].astype(np.int64)])
    with pytest.raises(ValueError, match='reseg takes the host hand-off'):
        p.diarize_batch(*args, rate=RATE, reseg=p.RESEG, fused=True)
    # a file with turns but no segments inside the batch: empty rows, the others as alone
    seg_off = np.array([0, three.seg_off[1], three.seg_off[1], three.seg_off[2]])
    rows = p.resegment_batch(ctx, three.eng.d_frames, three.frames.shape[0], [f0, f2, f1], three.d_stats, seg_off,
                             [three.labels[0], np.zeros(0, int), three.labels[1]], RATE)
    alone = p.resegment_batch(ctx, three.eng.d_frames, three.frames.shape[0], [f0, f1], three.d_stats, three.seg_off[:3],
                              three.labels[:2], RATE)
    assert rows[1].shape == (0, 3)
    assert rows[0].tobytes() == alone[0].tobytes() and rows[2].tobytes() == alone[1].tobytes()
