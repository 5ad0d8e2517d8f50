"""Resegmentation under mixture speaker models: spkd_gmm_train (EM training of a diagonal-covariance
GMM per speaker for a whole batch on the device), spkd_gmm_loglik_seq (every frame of every turn under
the mixtures of its file's speakers), pipeline.resegment_batch / diarize_batch with RESEG_GMM.
PARITY: no reference counterpart; the numpy restatement is tests/reseg_gmm_numpy.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import reseg_numpy as R
import reseg_gmm_numpy as G
from helpers import ROOT
from conftest import pkg
from reseg_helpers import Batch, Dev as _Dev, StubContext, displaced as _displaced, ptr as _ptr
from test_reseg_batch import _close

RATE = 125.0


def _same(got, want):
    """_close on the finite entries, the same entries infinite (ln w = -inf) with the same sign."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    return bool(np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin])
                and _close(got[fin], want[fin]))


def _frame_accuracy(vad, truth, pieces):
    """The share of turn frames that carry the truth speaker; pieces: [(begin, end, speaker)] in frames."""
    n = max(b for _, b in vad)
    want, got, turn = np.full(n, -1), np.full(n, -2), np.zeros(n, dtype=bool)
    for s, e, k in truth:
        want[s:e] = k
    for s, e, k in pieces:
        got[s:e] = k
    for a, b in vad:
        turn[a:b] = True
    return float((got[turn] == want[turn]).mean())


def _purpose_inputs():
    """(name, feats, vad, truth, displaced input segmentation): the Gaussian stage's three-speaker
    session, and a four-source session whose sources {0, 1} and {2, 3} are two speakers -- each
    speaker bimodal, what one Gaussian spreads across."""
    synth = pkg('synth')
    feats, vad, truth = synth.make_session(1234, 60.0, 3)
    out = [('three speakers', feats, vad, truth, _displaced(truth, vad))]
    feats, vad, truth = synth.make_session(1234, 60.0, 4)
    truth = [(s, e, k // 2) for s, e, k in truth]
    out.append(('two bimodal speakers', feats, vad, truth, _displaced(truth, vad)))
    return out


# ------------------------------------------------------------------ not GPU
def test_entry_points_timers_and_constants_are_declared_and_exported():
    hipabi = pkg('hipabi')
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'spkd.h')).read(), flags=re.S)
    lib = hipabi.load_library()
    for name in ('spkd_gmm_train', 'spkd_gmm_loglik_seq'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in hipabi.EXPORTS and hasattr(lib, name)
    assert lib.spkd_abi_version() == 2 and re.search(r'#define SPKD_ABI_VERSION 2\b', code)
    enum = re.search(r'enum \{\s*SPKD_T_CALL = 0,(.*?)SPKD_N_TIMERS', code, flags=re.S).group(1)
    names = ['call'] + [n.strip()[len('SPKD_T_'):].lower() for n in enum.split(',') if n.strip()]
    assert 'gmm_train' in names and 'gmm_seq_loglik' in names
    assert [n for n, _ in sorted(hipabi.TIMERS.items(), key=lambda kv: kv[1])] == names
    kern = open(os.path.join(ROOT, 'speaker-diarization_amd', 'csrc', 'spkd_gmm_train.hpp')).read()
    for macro, const, bound, restated, want in (
            ('SPKD_GMM_COMP', 'GT_COMP', hipabi.GMM_COMP, G.COMP, 80),
            ('SPKD_GMM_MAX_COMP', 'GT_MAX_COMP', hipabi.GMM_MAX_COMP, G.MAX_COMP, 8),
            ('SPKD_GMM_TILE', 'GT_TILE', hipabi.GMM_TILE, G.TILE, 64),
            ('SPKD_GMM_CHUNK_TILES', 'GT_CHUNK_TILES', hipabi.GMM_CHUNK_TILES, G.CHUNK_TILES, 16)):
        header = int(re.search(r'#define %s (\d+)' % macro, code).group(1))
        kernel = int(re.search(r'constexpr int %s = (\d+);' % const, kern).group(1))
        assert header == kernel == bound == restated == want, macro
    assert hasattr(hipabi.Context, 'gmm_train') and hasattr(hipabi.Context, 'gmm_loglik_seq')
    assert 'PARITY: no reference counterpart' in kern and 'PARITY: no reference counterpart' in G.__doc__
    pipeline = pkg('pipeline')
    assert pipeline.RESEG_GMM == dict(penalty=50.0, model='gmm', components=4, iterations=5, var_floor=0.01)
    assert pipeline.RESEG == dict(penalty=50.0)


def _refusals():
    """(name, call(lib, ctx handle) -> status) of every argument refusal of the two entry points."""
    dev = C.c_void_p(4096)                        # never dereferenced: the refusal comes first
    odd = C.c_void_p(4104)
    ok = np.ones(4, dtype=np.int32)
    ll = np.zeros(8)
    keep = {}

    def train(n_frames=100, n_spk=2, off=(0, 1, 3), b=(0, 10, 50), e=(10, 50, 100), K=2, n_iter=2, floor=0.01,
              frames=dev, gmm=dev, h_ok=ok, h_ll=ll):
        arr = [None if v is None else np.array(v, dtype=np.int64) for v in (off, b, e)]
        keep[len(keep)] = arr
        p = [None if a is None else _ptr(a) for a in arr]
        return lambda lib, h: lib.spkd_gmm_train(h, frames, n_frames, n_spk, p[0], p[1], p[2], K, n_iter, 0, floor, gmm,
                                                 None if h_ok is None else _ptr(h_ok), None if h_ll is None else _ptr(h_ll))

    def lik(n_frames=100, models=dev, K=2, n_models=4, h_ok=ok, n_seq=2, b=(0, 10), e=(10, 100), m=(0, 1), k=(1, 3),
            n_cols=4, frames=dev, scores=dev):
        arr = [None if v is None else np.array(v, dtype=t) for v, t in
               ((b, np.int64), (e, np.int64), (m, np.int32), (k, np.int32))]
        keep[len(keep)] = arr
        p = [None if a is None else _ptr(a) for a in arr]
        return lambda lib, h: lib.spkd_gmm_loglik_seq(h, frames, n_frames, models, K, n_models,
                                                      None if h_ok is None else _ptr(h_ok), n_seq, p[0], p[1], p[2], p[3],
                                                      n_cols, scores)

    return [
        ('train: null frames', train(frames=None)), ('train: null offsets', train(off=None)),
        ('train: null begin', train(b=None)), ('train: null end', train(e=None)),
        ('train: null models', train(gmm=None)), ('train: null ok', train(h_ok=None)),
        ('train: null log-likelihoods', train(h_ll=None)), ('train: negative speaker count', train(n_spk=-1)),
        ('train: no component', train(K=0)), ('train: a 9th component', train(K=9)),
        ('train: negative iterations', train(n_iter=-1)),
        ('train: negative floor', train(floor=-0.01)), ('train: floor NaN', train(floor=float('nan'))),
        ('train: floor inf', train(floor=float('inf'))),
        ('train: offsets not from 0', train(off=(1, 2, 3))), ('train: offsets go back', train(off=(0, 2, 1))),
        ('train: an empty set', train(off=(0, 0, 3))), ('train: an empty last set', train(off=(0, 3, 3))),
        ('train: begin below 0', train(b=(-1, 10, 50))), ('train: end past the frames', train(e=(10, 50, 101))),
        ('train: end before begin', train(b=(0, 20, 50), e=(10, 19, 100))),
        ('train: misaligned models', train(gmm=odd)),
        ('seq: null frames', lik(frames=None)), ('seq: null models', lik(models=None)),
        ('seq: null ok', lik(h_ok=None)), ('seq: null scores', lik(scores=None)),
        ('seq: null begin', lik(b=None)), ('seq: null end', lik(e=None)),
        ('seq: null first model', lik(m=None)), ('seq: null model count', lik(k=None)),
        ('seq: negative sequence count', lik(n_seq=-1)),
        ('seq: no component', lik(K=0)), ('seq: a 9th component', lik(K=9)),
        ('seq: no column', lik(n_cols=0)), ('seq: a 17th column', lik(n_cols=17, k=(1, 17), n_models=40)),
        ('seq: more models than columns', lik(k=(1, 5), n_models=8)),
        ('seq: begin below 0', lik(b=(-1, 10))), ('seq: end past the frames', lik(e=(10, 101))),
        ('seq: end before begin', lik(b=(0, 50), e=(10, 49))),
        ('seq: model below 0', lik(m=(-1, 1))), ('seq: model past the models', lik(m=(0, 2))),
        ('seq: misaligned models', lik(models=odd)),
    ]


def test_every_refusal_is_einval_without_a_context():
    hipabi = pkg('hipabi')
    lib = hipabi.load_library()
    for name, call in _refusals():
        assert call(lib, None) == hipabi.SPKD_EINVAL, name


def test_one_component_is_the_maximum_likelihood_gaussian():
    """K = 1: one EM step from any start gives the ML mean and variance of the frames, as their
    statistics record states them; a second step changes the log-likelihood no more."""
    x = pkg('synth').make_session(909, 60.0, 2)[0][1000:3000]
    rec = np.zeros((40, 40))
    rec[np.triu_indices(40)] = R.record_of_frames(x)
    n = rec[39, 39]
    mean = rec[:39, 39] / n
    var = np.diag(rec)[:39] / n - mean * mean
    rng = np.random.default_rng(5)
    start = np.concatenate([[0.0], rng.normal(0.0, 2.0, 39), rng.uniform(0.2, 5.0, 39), [-40.0]])[None, :]
    m1, l0, fin = G.em_step(x, start, 0.01)
    assert fin and m1[0, 0] == 0.0
    assert _close(m1[0, G.MEAN:G.IVAR], mean) and _close(1.0 / m1[0, G.IVAR:G.NORM], var)
    assert _close(m1[0, G.NORM], -0.5 * (39 * np.log(2 * np.pi) + np.log(var).sum()))
    m2, l1, fin = G.em_step(x, m1, 0.01)
    m3, l2, fin = G.em_step(x, m2, 0.01)
    assert fin and l1 > l0 and abs(l2 - l1) <= 1e-9 * abs(l1)
    assert _same(m2, m1)
    # the same model from the segmental start, whose one component takes every frame
    m0, ok = G.init_model(x, 1, 0.01)
    assert ok and _same(m0, m1)
    assert _close(G.train(x, 1, 2, 0.01)[2], [l1, l2])


@pytest.mark.parametrize('K', [2, 4])
def test_restated_em_never_lowers_the_loglikelihood(K):
    """Seed 909 (the first tried): the floor and the G_k < 2 rule stay inactive over the 5 steps.
    (Where the two rules ARE exercised: tests/mixture_cases.py's floor, starved and K = 7 cases, on the
    CPU in tests/test_exact_mixture.py and on the device in tests/test_mixture_exact.py.)"""
    x = pkg('synth').make_session(909, 60.0, 2)[0]
    assert len(x) == 7500
    floor = G.variance_floor(x, 0.01)[0]
    model, ok = G.init_model(x, K, 0.01)
    lls = []
    for _ in range(5):
        model, total, fin = G.em_step(x, model, 0.01)
        ok = ok and fin
        lls.append(total)
        assert (np.exp(model[:, 0]) * len(x) >= 2.0).all() and (1.0 / model[:, G.IVAR:G.NORM] > floor).all()
    print('K = %d: L = %s' % (K, ', '.join('%.3f' % v for v in lls)))
    assert ok and all(b >= a - 1e-9 * abs(a) for a, b in zip(lls[:-1], lls[1:]))
    assert lls[-1] > lls[0]


def _restated_pieces(feats, vad, segs, reseg):
    spk, decoded, oks, _ = G.resegment(feats, vad, segs, reseg)
    assert all(oks)
    out = []
    for (a, b), (frames, words) in zip(vad, decoded):
        ends = frames[1:] + [b - a]
        out += [(a + f, a + e, spk[w]) for f, e, w in zip(frames, ends, words)]
    return out


def test_restatement_beats_the_displaced_input():
    """What the stage is for: every boundary inside a turn of the input is 100 frames late; decoding
    under mixtures trained on that input labels more turn frames with the truth speaker than the input."""
    reseg = pkg('pipeline').RESEG_GMM
    for name, feats, vad, truth, segs in _purpose_inputs():
        before = _frame_accuracy(vad, truth, segs)
        after = _frame_accuracy(vad, truth, _restated_pieces(feats, vad, segs, reseg))
        print('%s: frame accuracy %.4f of the input, %.4f resegmented' % (name, before, after))
        assert before < 1.0 and after > before, name


class _StubContext(StubContext):
    """One canned decoding under model 'gmm'; every call with all its arguments, the scratch requests among
    them.  A context without the Gaussian path: asking it for sum_stats is an AttributeError."""
    MS = {'gmm_train': 0.25, 'gmm_seq_loglik': 0.75}

    def __init__(self, ok, tokens):
        StubContext.__init__(self, [tokens], [ok])
        self.tokens = tokens

    @property
    def sum_stats(self):
        raise AttributeError('sum_stats')

    def dev_scratch(self, name, nbytes):
        self.calls.append(('dev_scratch', name, nbytes))
        return self.SCRATCH[name]

    def gmm_train(self, d_frames, n_frames, set_off, b, e, n_comp, n_iter, var_floor, d_gmm, from_model=False):
        self.calls.append(('gmm_train', d_frames, n_frames, np.array(set_off).tolist(), np.array(b).tolist(),
                           np.array(e).tolist(), n_comp, n_iter, var_floor, d_gmm, from_model))
        ok = self._ok(len(set_off) - 1)
        return ok, np.arange(len(ok) * n_iter, dtype=np.float64).reshape(len(ok), n_iter)

    def gmm_loglik_seq(self, d_frames, n_frames, d_gmm, n_comp, ok, b, e, m, k, n_cols, d_scores):
        self.calls.append(('gmm_loglik_seq', d_frames, n_frames, d_gmm, n_comp, np.array(ok).tolist(),
                           np.array(b).tolist(), np.array(e).tolist(), np.array(m).tolist(), np.array(k).tolist(),
                           n_cols, d_scores))
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
    segments = [np.array([(1.0, 2.0), (2.0, 2.5), (2.5, 3.0)]), np.zeros((0, 2)),
                np.array([(0.5, 2.0), (2.0, 3.0), (3.0, 4.0), (4.0, 9.0)])]
    stub = _StubContext([1, 1, 1, 0, 1], [[(0, 1), (100, 0)], [], [(0, 2), (7, 0), (300, 2)]])
    timings, det = {}, {}
    reseg = dict(penalty=7.0, model='gmm', components=3, iterations=2, var_floor=0.05)
    rows = pipeline.resegment_batch(stub, 1 << 20, 2500, files, 1 << 21, [0, 3, 3, 7], labels, 125.0, reseg,
                                    False, timings, det, segments)
    assert [c[0] for c in stub.calls] == ['dev_scratch', 'gmm_train', 'dev_scratch', 'gmm_loglik_seq', 'vad_viterbi_batch']
    assert stub.calls[0][1:] == ('reseg_gmm', 5 * 3 * hipabi.GMM_COMP * 8)
    # a speaker's ranges: its segments' frames as segment_stats cuts them, in segment order (2.5 s = frame 312; the
    # last segment ends with its file)
    assert stub.calls[1][1:] == (1 << 20, 2500, [0, 1, 3, 5, 6, 7], [250, 125, 312, 1750, 2000, 1875, 1562],
                                 [312, 250, 375, 1875, 2500, 2000, 1750], 3, 2, 0.05, 8192, False)
    assert stub.calls[2][1:] == ('reseg_scores', (250 + 0 + 688) * 3 * 4)
    assert stub.calls[3][1:] == (1 << 20, 2500, 8192, 3, [1, 1, 1, 0, 1], [125, 1000, 1562], [375, 1000, 2250], [0, 0, 2],
                                 [2, 2, 3], 3, 12288)
    assert stub.calls[4][1:] == (12288, [0, 250, 250, 938], 3, [0, 1, 2], [0.0] * 3, [0.0] * 3, [-7.0] * 3)
    assert rows[0].tolist() == [[1.0, 1.0 + 100 / 125.0, 5.0], [1.0 + 100 / 125.0, 3.0, 2.0]]
    assert rows[1].shape == (0, 3)
    assert rows[2].tolist() == [[0.5, 0.5 + 7 / 125.0, 3.0], [0.5 + 7 / 125.0, 0.5 + 300 / 125.0, 1.0],
                                [0.5 + 300 / 125.0, 6.0, 3.0]]
    assert det['dropped'] == [(2, 2)] and det['loglik'].tolist() == np.arange(10.0).reshape(5, 2).tolist()
    assert timings['reseg_gmm_train'] == [0.25] and timings['reseg_loglik'] == [0.75]
    assert timings['reseg_viterbi'] == [0.5] and timings['reseg_backtrack'] == [0.5] and 'reseg_models' not in timings
    # RESEG_GMM's own values where a key is absent; the rows of the restatement's builder under the text contract
    stub = _StubContext([1] * 5, stub.tokens)
    rows = pipeline.resegment_batch(stub, 1 << 20, 2500, files, 1 << 21, [0, 3, 3, 7], labels, 125.0 / 3.0,
                                    dict(penalty=50.0, model='gmm'), segments=segments)
    assert stub.calls[1][6:9] == (4, 5, 0.01)
    want = R.rows_of_turn([0, 7, 300], [2, 0, 2], 0.5, 6.0, [1, 2, 3], 125.0 / 3.0, True)
    assert rows[2].tobytes() == want.tobytes()
    # model 'gauss' and no model at all: the Gaussian path, which asks for none of the above
    for reseg in (dict(penalty=7.0, model='gauss'), dict(penalty=7.0)):
        with pytest.raises(AttributeError, match='sum_stats'):
            pipeline.resegment_batch(_StubContext([1] * 5, stub.tokens), 1 << 20, 2500, files, 1 << 21, [0, 3, 3, 7],
                                     labels, 125.0, reseg, segments=segments)


def test_refusals_of_the_pipeline_need_no_device():
    pipeline = pkg('pipeline')
    files = [pipeline.BatchFile(0, 1000, [(0.0, 8.0)])]
    segments = [np.array([(0.0, 4.0), (4.0, 8.0)])]
    labels = [np.array([1, 2])]
    bad = [(dict(model='mixture'), 'reseg model'), (dict(components=0), 'reseg components'),
           (dict(components=9), 'reseg components'), (dict(components=2.5), 'reseg components'),
           (dict(iterations=-1), 'reseg iterations'), (dict(var_floor=-0.1), 'reseg var_floor'),
           (dict(var_floor=float('nan')), 'reseg var_floor'), (dict(var_floor=float('inf')), 'reseg var_floor'),
           (dict(penalty=-1.0), 'reseg penalty')]
    for change, match in bad:
        reseg = dict(pipeline.RESEG_GMM, **change)
        with pytest.raises(ValueError, match=match):
            pipeline.resegment_batch(None, 0, 1000, files, 0, [0, 2], labels, reseg=reseg, segments=segments)
        with pytest.raises(ValueError, match=match):
            pipeline.diarize_batch(None, 0, 0, [], reseg=reseg)
    with pytest.raises(ValueError, match='it takes segments'):
        pipeline.resegment_batch(None, 0, 1000, files, 0, [0, 2], labels, reseg=pipeline.RESEG_GMM)
    with pytest.raises(ValueError, match='one per label'):
        pipeline.resegment_batch(None, 0, 1000, files, 0, [0, 2], labels, reseg=pipeline.RESEG_GMM,
                                 segments=[segments[0][:1]])
    with pytest.raises(ValueError, match='reseg takes the host hand-off'):
        pipeline.diarize_batch(None, 0, 0, [], reseg=pipeline.RESEG_GMM, fused=True)
    many = [pipeline.BatchFile(0, 1000, [(0.0, 8.0)]), pipeline.BatchFile(1000, 1000, [(0.0, 8.0)])]
    with pytest.raises(ValueError, match='at most 16 speakers'):
        pipeline.resegment_batch(None, 0, 2000, many, 0, [0, 2, 19], [np.array([1, 2]), np.arange(1, 18)],
                                 reseg=pipeline.RESEG_GMM, segments=[np.zeros((2, 2)), np.zeros((17, 2))])
    # nothing to decode: no device work either
    det = {}
    assert pipeline.diarize_batch(None, 0, 0, [], reseg=pipeline.RESEG_GMM, detail=det) == [] and det['dropped'] == []
    out = pipeline.resegment_batch(None, 0, 2000, many, 0, [0, 0, 0], [np.zeros(0, int)] * 2, reseg=pipeline.RESEG_GMM,
                                   detail=det, segments=[np.zeros((0, 2))] * 2)
    assert [o.shape for o in out] == [(0, 3)] * 2 and det['dropped'] == []
    quiet = [pipeline.BatchFile(0, 1000, [])]
    assert pipeline.resegment_batch(None, 0, 1000, quiet, 0, [0, 2], labels, reseg=pipeline.RESEG_GMM,
                                    segments=segments)[0].shape == (0, 3)


# ------------------------------------------------------------------ GPU
N_SESSION = 7500


@pytest.fixture(scope='module')
def one():
    """One 60 s session of two speakers, 64 constant frames behind it, then 400 frames with a NaN among them."""
    feats = pkg('synth').make_session(909, 60.0, 2)[0]
    assert len(feats) == N_SESSION
    tail = feats[1000:1400].copy()
    tail[123, 5] = np.nan
    d = _Dev(np.concatenate([feats, np.repeat(feats[777:778], 64, axis=0), tail]))
    yield d
    d.close()


def _speakers(K):
    """The speakers of the training test: per speaker its ranges, in the caller's order."""
    edges = [(5000, 1), (100, 63), (4000, 64), (200, 65), (1000, 1023), (6000, 1024), (2100, 1025)]
    return [[(b, b + n) for b, n in edges],                        # range, tile and chunk edges inside a speaker
            [(300, 300 + 40 * K - 7), (900, 907)],                 # exactly 40 K frames
            [(400, 400 + 40 * K - 1)],                             # one frame short
            [(N_SESSION, N_SESSION + 64)],                         # constant frames
            [(N_SESSION + 64, N_SESSION + 464)],                   # a NaN frame; the range ends at n_frames
            [(3000, 7000)]]                                        # four chunks, the last one short


def _train(dev, spk, K, n_iter, d_gmm, from_model=False, var_floor=0.01):
    off = np.concatenate([[0], np.cumsum([len(r) for r in spk])])
    flat = [r for rs in spk for r in rs]
    return dev.ctx.gmm_train(dev.eng.d_frames, dev.frames.shape[0], off, [b for b, _ in flat], [e for _, e in flat], K,
                             n_iter, var_floor, d_gmm, from_model)


def _download(dev, d_gmm, n, K):
    out = np.empty((n, K, G.COMP))
    dev.ctx.d2h(out, d_gmm)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('K', [1, 2, 8])
def test_initial_model_and_single_steps_match_the_restatement(one, K):
    spk = _speakers(K)
    assert spk[4][0][1] == one.frames.shape[0]
    x = [np.concatenate([one.frames[b:e] for b, e in rs]) for rs in spk]
    assert [len(v) for v in x] == [3265, 40 * K, 40 * K - 1, 64, 400, 4000]
    d_gmm = one.alloc(len(spk) * K * G.COMP * 8)
    ok, ll = _train(one, spk, K, 0, d_gmm)
    assert ok.tolist() == [1, 1, 0, 0, 0, 1] and ll.shape == (6, 0)
    assert one.ctx.last_ms('gmm_train') > 0.0
    got = _download(one, d_gmm, len(spk), K)
    for s in range(len(spk)):
        want, good = G.init_model(x[s], K, 0.01)
        assert good == bool(ok[s]), s
        if good:
            assert _same(got[s], want), s
    for step in range(3):                                              # single steps: no error accumulates
        prev = got
        ok, ll = _train(one, spk, K, 1, d_gmm, from_model=True)
        assert ok.tolist() == [1, 1, 0, 0, 0, 1] and ll.shape == (6, 1)
        got = _download(one, d_gmm, len(spk), K)
        for s in np.nonzero(ok)[0]:
            want, total, fin = G.em_step(x[s], prev[s], 0.01)
            err = float(np.abs(got[s][np.isfinite(want)] - want[np.isfinite(want)]).max())
            print('K %d step %d speaker %d: L %.6f (restated %.6f), max abs model error %.3g' % (K, step, s, ll[s, 0], total, err))
            assert fin and _same(got[s], want), (step, s)
            assert _close(ll[s, 0], total), (step, s)


@pytest.mark.gpu
def test_training_is_reproducible_to_the_bit(one):
    K = 4
    spk = _speakers(K)
    n = len(spk)
    d_a, d_b = one.alloc(n * K * G.COMP * 8), one.alloc(n * K * G.COMP * 8)
    ok_a, ll_a = _train(one, spk, K, 3, d_a)
    ok_b, ll_b = _train(one, spk, K, 3, d_b)
    a, b = _download(one, d_a, n, K), _download(one, d_b, n, K)
    good = np.nonzero(ok_a)[0]
    assert good.tolist() == [0, 1, 5] and ok_a.tolist() == ok_b.tolist()
    assert a[good].tobytes() == b[good].tobytes() and ll_a[good].tobytes() == ll_b[good].tobytes()
    # a speaker alone and among the others
    for s in (0, 5):
        ok_s, ll_s = _train(one, [spk[s]], K, 3, d_b)
        assert ok_s.tolist() == [1] and ll_s.tobytes() == ll_a[s:s + 1].tobytes()
        assert _download(one, d_b, 1, K).tobytes() == a[s:s + 1].tobytes()
    # three steps in one call and three calls of one step
    ok_c, _ = _train(one, spk, K, 0, d_b)
    chained = []
    for _ in range(3):
        ok_c, ll_c = _train(one, spk, K, 1, d_b, from_model=True)
        chained.append(ll_c[:, 0])
    assert ok_c.tolist() == ok_a.tolist()
    assert _download(one, d_b, n, K)[good].tobytes() == a[good].tobytes()
    assert np.column_stack(chained)[good].tobytes() == ll_a[good].tobytes()
    # nothing to train, and every refusal with a context: SPKD_EINVAL, nothing written
    hipabi, ctx = one.hipabi, one.ctx
    assert ctx.lib.spkd_gmm_train(ctx.h, None, 0, 0, None, None, None, K, 1, 0, 0.01, None, None, None) == hipabi.SPKD_OK
    for name, call in _refusals():
        assert call(ctx.lib, ctx.h) == hipabi.SPKD_EINVAL, name
    assert _download(one, d_a, n, K).tobytes() == a.tobytes()


@pytest.mark.gpu
def test_scores_match_the_restatement_to_an_ulp(one):
    hipabi, ctx = one.hipabi, one.ctx
    n_frames, K, TILE = one.frames.shape[0], 4, G.TILE
    # file A: one speaker; file B: three, the second of them (30 frames) not ok
    spk = [[(200, 700)], [(1000, 3000)], [(300, 330)], [(4000, 6000)]]
    d_gmm = one.alloc(4 * K * G.COMP * 8)
    ok, _ = _train(one, spk, K, 2, d_gmm)
    assert ok.tolist() == [1, 1, 0, 1]
    models = _download(one, d_gmm, 4, K)                                   # the device's models: their error is excluded
    lens = [1, 2, TILE - 1, TILE, TILE + 1, 0, 2 * TILE + 1, 777]
    begin = np.array([5000, 4990, 3000, 3100, 2000, 2500, n_frames - (2 * TILE + 1), 100], dtype=np.int64)
    end = begin + lens
    assert int(end.max()) == n_frames and sorted(begin.tolist()) != begin.tolist()
    owner_b = np.array([0, 1, 1, 0, 1, 1, 1, 1], dtype=bool)
    first, count = np.where(owner_b, 1, 0), np.where(owner_b, 3, 1)
    total, n_cols, pad = int(sum(lens)), 4, 8
    nan_row = int(np.cumsum(lens)[6]) + 300                                # a frame of the last sequence
    frames = one.frames.copy()
    frames[N_SESSION + 64:] = frames[1000:1400]                            # (the tail without its NaN)
    frames[100 + 300, 7] = np.nan
    d_frames = one.alloc(frames.nbytes)
    ctx.h2d(d_frames, frames)
    d_scores = one.alloc((total + pad) * n_cols * 4)
    mark = np.full((total + pad, n_cols), 12345.0, dtype=np.float32)
    ctx.h2d(d_scores, mark)
    off = ctx.gmm_loglik_seq(d_frames, n_frames, d_gmm, K, ok, begin, end, first, count, n_cols, d_scores)
    assert off.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
    assert ctx.last_ms('gmm_seq_loglik') > 0.0
    got = np.empty_like(mark)
    ctx.d2h(got, d_scores)
    assert np.array_equal(got[total:], mark[total:])                       # rows beyond the total: untouched
    want = np.full((total, n_cols), -np.inf)
    for q in range(len(lens)):
        k = int(count[q])
        want[off[q]:off[q + 1], :k] = G.scores(frames[begin[q]:end[q]], models[first[q]:first[q] + k],
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
    assert ctx.gmm_loglik_seq(d_frames, n_frames, d_gmm, K, ok, [7, 9], [7, 9], [0, 1], [1, 3], n_cols, d_scores).tolist() == [0, 0, 0]
    assert ctx.gmm_loglik_seq(d_frames, n_frames, d_gmm, K, ok, [], [], [], [], n_cols, d_scores).tolist() == [0]
    with pytest.raises(hipabi.SpkdError) as ei:
        ctx.gmm_loglik_seq(d_frames, n_frames, d_gmm, K, ok, [0, 10], [10, n_frames + 1], [0, 1], [1, 3], n_cols, d_scores)
    assert ei.value.status == hipabi.SPKD_EINVAL
    ctx.d2h(got, d_scores)
    assert np.array_equal(got, mark)


@pytest.fixture(scope='module')
def three():
    """Three 60 s files of 2, 3 and 4 speakers as one batch, their truth segments and those segments' records."""
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
                             three.labels, RATE, p.RESEG_GMM, text_contract, timings, det, three.segments)
    assert det['dropped'] == [] and det['loglik'].shape == (9, 5) and np.isfinite(det['loglik']).all()
    assert all(len(timings[k]) == 1 for k in ('reseg_gmm_train', 'reseg_loglik', 'reseg_viterbi', 'reseg_backtrack'))
    assert 'reseg_models' not in timings
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
def test_stage_beats_the_displaced_input_on_the_device():
    pipeline = pkg('pipeline')
    for name, feats, vad, truth, segs in _purpose_inputs():
        d = _Dev(feats)
        try:
            files = [pipeline.BatchFile(0, len(feats), [(a / RATE, b / RATE) for a, b in vad])]
            labels = [np.array([k + 1 for _, _, k in segs])]
            segments = [np.array([(a / RATE, b / RATE) for a, b, _ in segs])]
            det = {}
            rows = pipeline.resegment_batch(d.ctx, d.eng.d_frames, len(feats), files, 0, [0, len(segs)], labels, RATE,
                                            pipeline.RESEG_GMM, False, None, det, segments)[0]
            assert det['dropped'] == []
            pieces = [(int(round(r[0] * RATE)), int(round(r[1] * RATE)), int(r[2]) - 1) for r in rows]
            before, after = _frame_accuracy(vad, truth, segs), _frame_accuracy(vad, truth, pieces)
            print('%s: frame accuracy %.4f of the input, %.4f resegmented on the device' % (name, before, after))
            assert before < 1.0 and after > before, name
        finally:
            d.close()


@pytest.mark.gpu
def test_diarize_batch_with_gmm_reseg(three):
    p, ctx = three.pipeline, three.ctx
    f0, f1, f2 = three.files
    files = [f0, p.BatchFile(f1.frame_off, f1.n_frames, []), f1, f2]       # a file with no turns inside the batch
    n = three.frames.shape[0]
    args = (ctx, three.eng.d_frames, n, files)
    plain = p.diarize_batch(*args, rate=RATE)
    det = {}
    got = p.diarize_batch(*args, rate=RATE, reseg=p.RESEG_GMM, detail=det)
    assert det['dropped'] == [] and got[1].shape == (0, 3) and all(len(got[i]) for i in (0, 2, 3))
    assert det['loglik'].shape[1] == 5
    # the stages one by one
    segs = p.change_detect_batch(ctx, three.eng.d_frames, n, files, RATE)
    box = []
    res = p.cluster_batch(ctx, three.eng.d_frames, n, files, segs, RATE, stats_out=box)
    labels = [lab for lab, _ in res]
    want = p.resegment_batch(ctx, three.eng.d_frames, n, files, box[0][0], box[0][1], labels, RATE, p.RESEG_GMM,
                             segments=segs)
    assert [r.tobytes() for r in got] == [r.tobytes() for r in want]
    for f, r in enumerate(got):
        assert set(r[:, 2].astype(int).tolist()) <= set(labels[f].tolist())
    # the Gaussian stage and no stage at all return what they return without the mixture path
    gauss = p.resegment_batch(ctx, three.eng.d_frames, n, files, box[0][0], box[0][1], labels, RATE)
    assert [r.tobytes() for r in p.diarize_batch(*args, rate=RATE, reseg=p.RESEG)] == [r.tobytes() for r in gauss]
    assert [r.tobytes() for r in p.diarize_batch(*args, rate=RATE, reseg=dict(penalty=50.0, model='gauss'))] == \
        [r.tobytes() for r in gauss]
    assert [r.tobytes() for r in p.diarize_batch(*args, rate=RATE, reseg=None)] == [r.tobytes() for r in plain]
    # another detector goes through the same path
    r = p.diarize_batch(*args, rate=RATE, reseg=p.RESEG_GMM, cd=p.SW_CD)
    assert r[1].shape == (0, 3) and all(len(r[i]) for i in (0, 2, 3))
    # with link: the third column through the maps, the times untouched
    det = {}
    linked = p.diarize_batch(*args, rate=RATE, reseg=p.RESEG_GMM, link=p.LINK_CL, detail=det)
    maps = det['link']['maps']
    for f in range(4):
        assert linked[f][:, :2].tobytes() == got[f][:, :2].tobytes()
        assert np.array_equal(linked[f][:, 2], maps[f][got[f][:, 2].astype(np.int64)])
