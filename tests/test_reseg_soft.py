"""Soft resegmentation: spkd_post_stats (posterior-weighted statistics records), its restatement
(tests/reseg_soft_numpy.py) and reseg['soft'] in pipeline.resegment_batch / diarize_batch -- the speakers
retrained between the passes on frame posteriors instead of decoded rows.  PARITY: no reference counterpart."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import reseg_mindur_numpy as M
import reseg_numpy as R
import reseg_soft_numpy as S
from helpers import ROOT
from conftest import pkg
from reseg_helpers import Batch, StubContext, close_session as _close_session, displaced as _displaced, ptr as _ptr

RATE = 125.0
L = np.longdouble
REC = 820
CHUNK = 1024         # SPKD_POST_CHUNK
U = 2.0 ** -53
# the two fixtures of the issue's table: (seed, eps, speakers, shift); hard ends at HARD_WRONG wrong frames
FIXTURES = [(7002, 0.10, 2, 300), (7006, 0.15, 3, 300)]
HARD_WRONG = [370, 300]
GAIN = 50
SOFT8 = dict(penalty=50.0, passes=8, soft=True, soft_scale=0.1)


@functools.lru_cache(maxsize=None)
def _fixture(i):
    """(feats, vad, truth, displaced segments, the restated hard loop, the restated soft loop) of fixture i,
    computed once; nothing changes them."""
    seed, eps, n, shift = FIXTURES[i]
    feats, vad, truth = _close_session(seed, 40.0, n, eps)
    segs = _displaced(truth, vad, shift)
    hard = M.resegment(feats, vad, segs, dict(penalty=50.0, passes=8))
    soft = S.resegment_soft(feats, vad, segs, SOFT8)
    return feats, vad, truth, segs, hard, soft


def _wrong(feats, vad, truth, spk, decoded):
    return int((S.frame_labels(vad, decoded, spk, len(feats)) != S.truth_labels(truth, len(feats))).sum())


# ------------------------------------------------------------------ not GPU
def test_entry_point_timer_and_chunk_are_declared_exported_and_bound():
    hipabi = pkg('hipabi')
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'spkd.h')).read(), flags=re.S)
    lib = hipabi.load_library()
    name = 'spkd_post_stats'
    assert re.search(r'\b%s\s*\(' % name, code)
    assert name in hipabi.EXPORTS and hasattr(lib, name) and hasattr(hipabi.Context, 'post_stats')
    assert lib.spkd_abi_version() == 2 and re.search(r'#define SPKD_ABI_VERSION 2\b', code)
    enum = re.search(r'enum \{\s*SPKD_T_CALL = 0,(.*?)SPKD_N_TIMERS', code, flags=re.S).group(1)
    names = ['call'] + [n.strip()[len('SPKD_T_'):].lower() for n in enum.split(',') if n.strip()]
    assert 'post_stats' in names and len(names) == len(set(names))
    assert [n for n, _ in sorted(hipabi.TIMERS.items(), key=lambda kv: kv[1])] == names
    csrc = os.path.join(ROOT, 'speaker-diarization_amd', 'csrc')
    kern, stats = open(os.path.join(csrc, 'spkd_post_stats.hpp')).read(), open(os.path.join(csrc, 'spkd_stats.hpp')).read()
    chunk = int(re.search(r'#define SPKD_POST_CHUNK (\d+)', code).group(1))
    assert chunk == CHUNK == hipabi.POST_CHUNK == int(re.search(r'constexpr int STATS_CHUNK = (\d+);', stats).group(1))
    # the kernel is made of spkd_stats.hpp's pieces, not of copies of them
    assert 'chunk_stats_accumulate(' in kern and 'fma(' not in kern and 'k_reduce_sets' in kern
    pipeline = pkg('pipeline')
    assert pipeline.RESEG_SOFT == dict(penalty=50.0, passes=5, soft=True)


def _refusals():
    """(name, call(lib, ctx handle) -> status) of every argument refusal of the entry point.  The valid call:
    100 frames; 3 sequences (0, 10), (20, 20), (50, 90) with the model ranges (0, 2), (0, 2), (2, 1); 2 columns;
    3 models."""
    dev = C.c_void_p(4096)                        # never dereferenced: the refusal comes first
    keep = []

    def ps(n_frames=100, n_seq=3, b=(0, 20, 50), e=(10, 20, 90), m=(0, 0, 2), k=(2, 2, 1), n_cols=2, n_models=3,
           frames=dev, post=dev, stats=dev):
        arr = lambda v, t: None if v is None else np.array(v, dtype=t)
        a = [arr(b, np.int64), arr(e, np.int64), arr(m, np.int32), arr(k, np.int32)]
        keep.append(a)
        p = [None if x is None else _ptr(x) for x in a]
        return lambda lib, h: lib.spkd_post_stats(h, frames, n_frames, post, n_seq, p[0], p[1], p[2], p[3], n_cols, n_models,
                                                  stats)

    return [
        ('no column', ps(n_cols=0)), ('a 17th column', ps(n_cols=17)),
        ('negative frame count', ps(n_frames=-1)), ('negative sequence count', ps(n_seq=-1)),
        ('negative model count', ps(n_models=-1)),
        ('null frames', ps(frames=None)), ('null posteriors', ps(post=None)), ('null records', ps(stats=None)),
        ('null begins', ps(b=None)), ('null ends', ps(e=None)), ('null first models', ps(m=None)),
        ('null model counts', ps(k=None)),
        ('records not 16-byte aligned', ps(stats=C.c_void_p(4096 + 8))),
        ('negative begin', ps(b=(-1, 20, 50))), ('end before begin', ps(e=(10, 19, 90))),
        ('end behind the frames', ps(e=(10, 20, 101))),
        ('negative n(q)', ps(k=(2, 2, -1))), ('n(q) above n_cols', ps(k=(2, 2, 3), n_models=8)),
        ('negative model', ps(m=(0, 0, -1))), ('model range behind n_models', ps(m=(0, 0, 3))),
        ('model ranges that overlap in part', ps(m=(0, 1, 2), k=(2, 2, 1), n_models=4)),
        ('model ranges that nest', ps(m=(0, 0, 2), k=(2, 1, 1))),
    ]


def test_every_refusal_is_einval_without_a_context():
    hipabi = pkg('hipabi')
    lib = hipabi.load_library()
    for name, call in _refusals():
        assert call(lib, None) == hipabi.SPKD_EINVAL, name


def test_value_errors_come_before_any_device_work():
    pipeline = pkg('pipeline')
    files = [pipeline.BatchFile(0, 1000, [(0.0, 8.0)])]
    labels = [np.array([1, 2])]
    segments = [np.array([(0.0, 4.0), (4.0, 8.0)])]
    cases = [(dict(soft=bad), 'reseg soft:') for bad in (1, 0, 'yes', None, 1.0)]
    cases += [(dict(soft=on, soft_scale=bad), 'reseg soft_scale:') for on in (True, False)
              for bad in (0.0, -0.1, float('nan'), float('inf'), 'x', None)]
    cases += [(dict(soft=True, soft_scale=12.5), 'reseg soft_scale \\* penalty'),
              (dict(soft=True, soft_scale=0.1, penalty=6000.5), 'reseg soft_scale \\* penalty')]
    for extra, match in cases:
        reseg = dict(dict(penalty=50.0, passes=3), **extra)
        with pytest.raises(ValueError, match=match):
            pipeline.resegment_batch(None, 0, 1000, files, 0, [0, 2], labels, reseg=reseg)
        with pytest.raises(ValueError, match=match):
            pipeline.diarize_batch(None, 0, 0, [], reseg=reseg)
    gmm = dict(pipeline.RESEG_GMM, soft=True)
    with pytest.raises(ValueError, match='reseg soft: the Gaussian speakers only'):
        pipeline.resegment_batch(None, 0, 1000, files, 0, [0, 2], labels, reseg=gmm, segments=segments)
    with pytest.raises(ValueError, match='reseg soft: the Gaussian speakers only'):
        pipeline.diarize_batch(None, 0, 0, [], reseg=gmm)
    stage = pkg('resegmentation')
    assert stage._reseg_soft(dict(penalty=50.0), ('gauss',)) == (False, 0.1)
    assert stage._reseg_soft(dict(penalty=50.0, soft=True, soft_scale=12.0), ('gauss',)) == (True, 12.0)
    assert stage._reseg_soft(dict(penalty=7000.0), ('gauss',)) == (False, 0.1)         # (the product binds soft only)
    assert stage._reseg_soft(dict(pipeline.RESEG_GMM, soft=False), ('gmm', 4, 5, 0.01)) == (False, 0.1)


class _StubContext(StubContext):
    """Both posterior calls and spkd_post_stats with all their arguments; either decoder is 'decode'."""
    MS = {'fb_posterior': 0.75, 'post_stats': 0.25}

    def __init__(self, answers, ok):
        StubContext.__init__(self, answers, ok)
        self.masses = []

    def mindur_viterbi_batch(self, d_scores, frame_off, n_cols, penalty, min_frames):
        self.calls.append(('decode',))
        return self._answer()

    def fb_posterior_batch(self, d_scores, frame_off, n_cols, penalty, tokens=None, seq_n_cols=None, scale=1.0, d_post=0):
        self.calls.append(('fb_posterior', d_scores, np.array(frame_off).tolist(), n_cols, penalty, tokens,
                           np.array(seq_n_cols).tolist(), scale, d_post))
        if tokens is None:
            return None, np.zeros(len(frame_off) - 1)
        return np.full(len(tokens[1]), 0.5), np.zeros(len(frame_off) - 1)

    def post_stats(self, d_frames, n_frames, d_post, b, e, m, k, n_cols, n_models, d_stats, masses=True):
        self.calls.append(('post_stats', d_frames, n_frames, d_post, np.array(b).tolist(), np.array(e).tolist(),
                           np.array(m).tolist(), np.array(k).tolist(), n_cols, n_models, d_stats))
        self.masses.append(masses)
        return np.arange(n_models) + 100.0 * self.n if masses else None


def test_the_soft_loop_on_the_host():
    """test_reseg_passes.test_the_loop_on_the_host's file: three speakers (labels 1, 2, 3), two turns.  With
    soft=True every retraining is fb_posterior + post_stats on the scores of the pass before, set_stats is
    never called, and the loop stops when pass 3 decodes what pass 2 did."""
    pipeline = pkg('pipeline')
    files = [pipeline.BatchFile(1000, 1000, [(1.0, 3.0), (4.0, 6.0)])]
    labels = [np.array([3, 1, 2, 1])]
    first = [[(0, 1), (100, 0)], [(0, 0), (50, 1)]]
    second = [[(0, 1), (90, 0)], [(0, 0), (50, 1)]]
    args = (1 << 20, 2000, files, 1 << 21, [0, 4], labels, RATE)
    base = dict(penalty=7.0, passes=5)
    for extra in (dict(soft=True), dict(soft=True, soft_scale=0.25, min_dur_s=0.5)):
        stub = _StubContext([first, second, second, first], [[1, 1, 1], [1, 1, 0]])
        timings, det = {}, {}
        rows = pipeline.resegment_batch(stub, *args, dict(base, **extra), False, timings, det)
        names = [c[0] for c in stub.calls]
        assert names == ['sum_stats', 'gauss_models', 'loglik', 'decode'] + \
            ['fb_posterior', 'post_stats', 'gauss_models', 'loglik', 'decode'] * 2
        assert 'set_stats' not in names
        scale = extra.get('soft_scale', 0.1)
        for at in (4, 9):
            # no tokens, every turn's speaker count, the scale, d_post the reseg_post buffer
            assert stub.calls[at][1:] == (12288, [0, 250, 500], 3, 7.0, None, [3, 3], scale, 16384), at
            assert stub.calls[at + 1][1:] == (1 << 20, 2000, 16384, [1125, 1500], [1375, 1750], [0, 0], [3, 3], 3, 3, 4096), at
            assert stub.calls[at + 2][1:] == (4096, 3, 8192)
        assert ('reseg_post', 500 * 3 * 4) in stub.scratch
        assert stub.calls[7][1] == [1, 1, 0] and stub.calls[2][1] == [1, 1, 1]
        assert det['passes_run'] == 3 and det['dropped'] == [(0, 3)]
        assert [m.tolist() for m in det['soft_mass']] == [[100.0, 101.0, 102.0], [200.0, 201.0, 202.0]]
        assert all(m.dtype == np.float64 for m in det['soft_mass'])
        assert timings['reseg_soft_posterior'] == [0.75] * 2 and timings['reseg_soft_stats'] == [0.25] * 2
        assert all(timings[k] == [0.5] * 3 for k in ('reseg_models', 'reseg_loglik', 'reseg_viterbi', 'reseg_backtrack'))
        assert rows[0].tolist() == [[1.0, 1.0 + 90 / 125.0, 2.0], [1.0 + 90 / 125.0, 3.0, 1.0],
                                    [4.0, 4.0 + 50 / 125.0, 1.0], [4.0 + 50 / 125.0, 6.0, 2.0]]
    # passes=2: one retraining, behind the first decode only (the last decode is followed by none)
    stub, det = _StubContext([first, second, first], [[1, 1, 1]]), {}
    pipeline.resegment_batch(stub, *args, dict(penalty=7.0, passes=2, soft=True), False, None, det)
    assert [c[0] for c in stub.calls].count('fb_posterior') == 1 and det['passes_run'] == 2 and len(det['soft_mass']) == 1
    # without a detail dictionary nobody reads the masses: the records stay on the device
    stub = _StubContext([first, second, first], [[1, 1, 1]])
    pipeline.resegment_batch(stub, *args, dict(penalty=7.0, passes=2, soft=True), False)
    assert stub.masses == [False] and [c[0] for c in stub.calls].count('post_stats') == 1
    # passes=1 with soft: pass 1 alone, no posterior
    stub, det = _StubContext([first], [[1, 1, 1]]), {}
    pipeline.resegment_batch(stub, *args, dict(penalty=7.0, soft=True), False, None, det)
    assert [c[0] for c in stub.calls] == ['sum_stats', 'gauss_models', 'loglik', 'decode'] and det['soft_mass'] == []
    # confidence keeps its own final call, with the tokens, at conf_scale
    stub, det = _StubContext([first, second, second], [[1, 1, 1]]), {}
    pipeline.resegment_batch(stub, *args, dict(base, soft=True, confidence=True, conf_scale=0.5), False, None, det)
    fb = [c for c in stub.calls if c[0] == 'fb_posterior']
    assert len(fb) == 3 and [c[7] for c in fb] == [0.1, 0.1, 0.5] and fb[-1][5] is not None and fb[-1][8] == 0
    assert stub.calls[-1][0] == 'fb_posterior'
    # the same dictionary without soft, or with soft=False: exactly today's calls
    plain, off, hard = [_StubContext([first, second, second, first], [[1, 1, 1], [1, 1, 0]]) for _ in range(3)]
    d0, d1 = {}, {}
    a = pipeline.resegment_batch(plain, *args, base, False, None, d0)
    b = pipeline.resegment_batch(off, *args, dict(base, soft=False, soft_scale=0.3), False, None, d1)
    assert [c[0] for c in plain.calls] == ['sum_stats', 'gauss_models', 'loglik', 'decode'] + \
        ['set_stats', 'gauss_models', 'loglik', 'decode'] * 2
    assert plain.calls == off.calls and plain.scratch == off.scratch and a[0].tobytes() == b[0].tobytes()
    assert 'soft_mass' not in d0 and 'soft_mass' not in d1 and d0 == d1
    assert plain.calls[4][1:] == (1 << 20, 2000, [1225, 1500, 1125, 1550], [1375, 1550, 1225, 1750], [0, 0, 1, 1], 3, 4096)


def test_restatement_of_post_stats_on_one_hot_weights_is_the_hard_record():
    rng = np.random.default_rng(5)
    feats = rng.normal(0.0, 2.0, (300, 39)).astype(np.float32)
    seqs = [(10, 110, 0, 2), (150, 300, 0, 2)]
    post = np.zeros((250, 2), dtype=np.float32)
    post[:60, 0] = post[60:130, 1] = post[130:, 0] = 1.0
    rec = S.post_stats(feats, post, seqs, 3)
    want0 = R.record_of_frames(feats[10:70]) + R.record_of_frames(feats[180:300])
    want1 = R.record_of_frames(np.concatenate([feats[70:110], feats[150:180]]))
    assert np.allclose(rec[0], want0, rtol=1e-12, atol=1e-9) and np.allclose(rec[1], want1, rtol=1e-12, atol=1e-9)
    assert rec[0][REC - 1] == 180.0 and rec[1][REC - 1] == 70.0 and (rec[2] == 0.0).all()
    assert S.post_terms(post, seqs, 3).tolist() == [180, 70, 0]
    bad = feats.copy()
    bad[20] = np.nan                                                       # weight 0 in column 1: no part of model 1
    rec = S.post_stats(bad, post, seqs, 3)
    assert np.isnan(rec[0]).any() and np.isfinite(rec[1]).all()


def test_restated_soft_loop_beats_the_hard_one_on_the_two_fixtures():
    """The 7002 and 7006 rows of the issue's table at penalty 50, scale 0.1, passes=8: hard is a fixed point
    of the displaced input (370 and 300 wrong frames), soft ends at least 50 fewer in each (measured: 80 and
    163) and stops before 8 passes."""
    for i, want in enumerate(HARD_WRONG):
        feats, vad, truth, segs, hard, soft = _fixture(i)
        w_hard = _wrong(feats, vad, truth, hard[0], hard[1][-1])
        per_pass = [_wrong(feats, vad, truth, soft[0], d) for d in soft[1]]
        print('fixture %d: hard %d wrong after %d passes, soft %s' % (FIXTURES[i][0], w_hard, hard[3], per_pass))
        assert w_hard == want
        assert per_pass[-1] <= w_hard - GAIN
        assert soft[3] < 8 and soft[1][-1] == soft[1][-2] and all(soft[2])
        assert len(soft[4]) == soft[3] - 1
        turn_frames = sum(b - a for a, b in vad)
        assert all(abs(m.sum() - turn_frames) <= 1e-3 * turn_frames for m in soft[4])


def test_restated_soft_and_hard_loops_both_reach_the_truth_on_the_easy_session():
    synth = pkg('synth')
    feats, vad, truth = synth.make_session(1234, 60.0, 3)
    segs = _displaced(truth, vad, 100)
    want = [t[0] for t in truth]
    hard = M.resegment(feats, vad, segs, dict(penalty=50.0, passes=8))
    soft = S.resegment_soft(feats, vad, segs, SOFT8)
    for out in (hard[1][-1], soft[1][-1]):
        assert [a + f for (a, b), (fr, _) in zip(vad, out) for f in fr] == want
    assert soft[3] < 8


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def ctx():
    c = pkg('hipabi').Context(0)
    yield c
    c.close()


LENGTHS = [0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]


@functools.lru_cache(maxsize=None)
def _case(W):
    """One call of 40 sequences, W columns.  Four groups of sequences that share a model range -- of W,
    max(1, W // 2), 1 and W models -- one model between them that nobody covers, and two sequences without
    models.  Every length of LENGTHS at least once, the longer ones in the narrow groups; the sequences sit
    in shuffled, disjoint places of the frames with gaps between them, so they neither ascend nor touch.
    The weights are float32 rows that sum to 1 (to rounding), with rows that are exactly one-hot and
    exact zeros planted; the columns >= n(q) hold NaN (they are never read).  Returns the inputs and the
    np.longdouble restatement with its bound, computed once."""
    rng = np.random.default_rng(900 + W)
    widths = [W, max(1, W // 2), 1, W]
    first = [0, W, W + widths[1], W + widths[1] + 2]          # (model W + widths[1] + 1: nobody's)
    n_models = first[3] + W
    uncovered = W + widths[1] + 1
    lens = LENGTHS + [CHUNK + 1, CHUNK - 1, 65, 64, 63, 1, 0] + [int(v) for v in rng.integers(2, 200, 24)]
    group = [0, 0, 0, 0, 0, 1, 2, 1, 2] + [0, 2, 3, 3, 3, 3, 3] + [int(v) for v in rng.integers(0, 4, 24)]
    assert len(lens) == len(group) == 40
    n_q = [widths[g] for g in group]
    m_q = [first[g] for g in group]
    n_q[20], n_q[21] = 0, 0                                   # two sequences without models
    place = rng.permutation(40)
    begin, at = [0] * 40, 7
    for q in place:
        begin[q] = at
        at += lens[q] + int(rng.integers(0, 9))
    n_frames = at + 5
    feats = (rng.normal(0.0, 3.0, (n_frames, 39)) + rng.normal(0.0, 5.0, 39)).astype(np.float32)
    seqs = [(begin[q], begin[q] + lens[q], m_q[q], n_q[q]) for q in range(40)]
    rows = []
    for q in range(40):
        T, n = lens[q], n_q[q]
        p = np.full((T, W), np.nan, dtype=np.float32)
        if n:
            g = rng.gamma(0.3, 1.0, (T, n)) + 1e-30
            g[rng.random((T, n)) < 0.2] = 0.0                 # exact zeros
            g[np.arange(T), rng.integers(0, n, T)] += 1e-3    # (no row of zeros only)
            g = g / g.sum(axis=1, keepdims=True)
            hot = rng.random(T) < 0.15                        # exact 1 beside exact 0
            g[hot] = 0.0
            g[hot, rng.integers(0, n, int(hot.sum()))] = 1.0
            p[:, :n] = g.astype(np.float32)
        rows.append(p)
    post = np.concatenate(rows)
    assert (post == 1.0).any() and (W == 1 or (post == 0.0).any())       # (one column: every weight is 1)
    want = S.post_stats(feats, post, seqs, n_models, L)
    mag = S.post_stats(feats, post, seqs, n_models, L, absolute=True)
    terms = np.zeros(n_models)
    for b, e, m, k in seqs:
        terms[m:m + k] += e - b
    bound = (terms[:, None] + 3.0) * U * mag
    return dict(W=W, feats=feats, post=post, seqs=seqs, n_models=n_models, uncovered=uncovered, want=want, bound=bound,
                group=group, first=first, widths=widths)


def _run_post_stats(ctx, feats, post, seqs, W, n_models, spare=1):
    """-> (records [n_models + spare, 820] as the device left a buffer filled with -7, the masses returned)."""
    out = np.full((n_models + spare, REC), -7.0)
    pad = np.zeros((1, post.shape[1]), dtype=np.float32)
    d_f, d_p, d_s = ctx.dev_alloc(feats.nbytes), ctx.dev_alloc(post.nbytes + pad.nbytes), ctx.dev_alloc(out.nbytes)
    try:
        ctx.h2d(d_f, feats)
        ctx.h2d(d_p, np.concatenate([post, pad]))
        ctx.h2d(d_s, out)
        b, e, m, k = [[s[i] for s in seqs] for i in range(4)]
        mass = ctx.post_stats(d_f, len(feats), d_p, b, e, m, k, W, n_models, d_s)
        ms = ctx.last_ms('post_stats')
        ctx.d2h(out, d_s)
    finally:
        for p in (d_f, d_p, d_s):
            ctx.dev_free(p)
    return out, mass, ms


@pytest.mark.gpu
@pytest.mark.parametrize('W', [1, 2, 3, 16])
def test_device_is_the_restatement(ctx, W):
    """Every entry of every record within the a-priori bound of a sum in any order against the np.longdouble
    restatement: (terms + 3) 2^-53 sum |w x~_i x~_j|, terms the frames of the model's sequences (the +3: the
    product w x~_i rounds once ahead of the FMA, and the restatement's own rounding)."""
    c = _case(W)
    out, mass, ms = _run_post_stats(ctx, c['feats'], c['post'], c['seqs'], W, c['n_models'])
    got = out[:c['n_models']]
    assert np.isfinite(got).all()
    err = np.abs(got.astype(L) - c['want']).astype(np.float64)
    ratio = np.where(c['bound'] > 0, err / np.where(c['bound'] > 0, c['bound'], 1.0), np.where(err > 0, np.inf, 0.0))
    print('post_stats W=%d: largest error / bound %.4f over %d records (kernel %.3f ms)' % (W, ratio.max(), c['n_models'], ms))
    assert ratio.max() <= 1.0
    assert (got[c['uncovered']] == 0.0).all()                              # nobody's model: exactly 0
    assert (out[c['n_models']:] == -7.0).all()                             # nothing behind n_models
    assert mass.dtype == np.float64 and mass.tobytes() == got[:, REC - 1].tobytes() and ms > 0.0


def _one_hot_case():
    """_case(3)'s sequences under one-hot posteriors in stretches -> (post, per model its frame ranges)."""
    c = _case(3)
    rng = np.random.default_rng(77)
    rows, ranges = [], [[] for _ in range(c['n_models'])]
    for b, e, m, k in c['seqs']:
        p = np.zeros((e - b, 3), dtype=np.float32)
        t = 0
        while k and t < e - b:
            n, j = int(rng.integers(1, 400)), int(rng.integers(0, k))
            n = min(n, e - b - t)
            p[t:t + n, j] = 1.0
            ranges[m + j].append((b + t, b + t + n))
            t += n
        rows.append(p)
    return c, np.concatenate(rows), ranges


@pytest.mark.gpu
def test_one_hot_posteriors_give_the_hard_records(ctx):
    c, post, ranges = _one_hot_case()
    out, mass, _ = _run_post_stats(ctx, c['feats'], post, c['seqs'], 3, c['n_models'])
    got = out[:c['n_models']]
    counts = np.array([sum(e - b for b, e in r) for r in ranges], dtype=np.float64)
    assert got[:, REC - 1].tolist() == counts.tolist() and mass.tolist() == counts.tolist()
    flat = [(b, e, m) for m, r in enumerate(ranges) for b, e in r]
    hard = np.empty((c['n_models'], REC))
    d_f, d_s = ctx.dev_alloc(c['feats'].nbytes), ctx.dev_alloc(hard.nbytes)
    try:
        ctx.h2d(d_f, c['feats'])
        ctx.set_stats(d_f, len(c['feats']), [f[0] for f in flat], [f[1] for f in flat],
                      np.array([f[2] for f in flat], dtype=np.int32), c['n_models'], d_s)
        ctx.d2h(hard, d_s)
    finally:
        ctx.dev_free(d_f)
        ctx.dev_free(d_s)
    mag = S.post_stats(c['feats'], post, c['seqs'], c['n_models'], L, absolute=True)
    bound = ((counts[:, None] + 3.0) * U * mag).astype(np.float64)
    err = np.abs(got - hard)
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print('post_stats on one-hot weights against set_stats: largest difference / bound %.4f' % ratio)
    assert ratio <= 1.0 and (err[bound == 0] == 0.0).all()


@pytest.mark.gpu
def test_the_bits_depend_on_neither_the_run_nor_the_other_files(ctx):
    c = _case(3)
    full, _, _ = _run_post_stats(ctx, c['feats'], c['post'], c['seqs'], 3, c['n_models'])
    again, _, _ = _run_post_stats(ctx, c['feats'], c['post'], c['seqs'], 3, c['n_models'])
    assert full.tobytes() == again.tobytes()
    off = np.concatenate([[0], np.cumsum([e - b for b, e, _, _ in c['seqs']])])
    for g in range(4):
        mine = [q for q in range(40) if c['group'][q] == g]
        assert len(mine) >= 3
        post = np.concatenate([c['post'][off[q]:off[q + 1]] for q in mine] + [np.zeros((0, 3), dtype=np.float32)])
        alone, _, _ = _run_post_stats(ctx, c['feats'], post, [c['seqs'][q] for q in mine], 3, c['n_models'])
        lo, hi = c['first'][g], c['first'][g] + c['widths'][g]
        assert alone[lo:hi].tobytes() == full[lo:hi].tobytes(), g
        rest = np.ones(c['n_models'], dtype=bool)
        rest[lo:hi] = False
        assert (alone[:c['n_models']][rest] == 0.0).all()


@pytest.mark.gpu
def test_a_frame_that_is_not_finite_counts_only_where_its_weight_is_not_zero(ctx):
    c = _case(3)
    q = next(i for i in range(40) if c['seqs'][i][3] == 3 and c['seqs'][i][1] - c['seqs'][i][0] > 80)
    b, e, m, k = c['seqs'][q]
    off = np.concatenate([[0], np.cumsum([s[1] - s[0] for s in c['seqs']])])
    feats, post = c['feats'].copy(), c['post'].copy()
    t = 70
    feats[b + t] = np.nan
    post[off[q] + t] = [0.0, 0.75, 0.25]
    out, _, _ = _run_post_stats(ctx, feats, post, c['seqs'], 3, c['n_models'])
    got = out[:c['n_models']]
    assert np.isfinite(got[m]).all() and np.isnan(got[m + 1]).any() and np.isnan(got[m + 2]).any()
    others = np.ones(c['n_models'], dtype=bool)
    others[m + 1:m + 3] = False
    assert np.isfinite(got[others]).all()
    models = np.empty((c['n_models'], 820))
    d_s, d_m = ctx.dev_alloc(got.nbytes), ctx.dev_alloc(models.nbytes)
    try:
        ctx.h2d(d_s, np.ascontiguousarray(got))
        ok = ctx.gauss_models(d_s, c['n_models'], d_m)
    finally:
        ctx.dev_free(d_s)
        ctx.dev_free(d_m)
    assert ok[m + 1] == 0 and ok[m + 2] == 0 and ok[m] == 1


@pytest.mark.gpu
def test_refusals_and_empty_calls_with_a_context(ctx):
    hipabi = pkg('hipabi')
    for name, call in _refusals():
        assert call(ctx.lib, ctx.h) == hipabi.SPKD_EINVAL, name
    none = np.zeros(0, dtype=np.int64)
    assert len(ctx.post_stats(0, 0, 0, none, none, none, none, 3, 0, 4096)) == 0       # no model: no launch
    feats = np.zeros((10, 39), dtype=np.float32)
    for seqs in ([], [(3, 3, 0, 2), (5, 5, 0, 2)], [(0, 10, 0, 0)]):
        out, mass, _ = _run_post_stats(ctx, feats, np.zeros((sum(e - b for b, e, _, _ in seqs), 2), dtype=np.float32), seqs, 2, 2)
        assert (out[:2] == 0.0).all() and (out[2] == -7.0).all() and mass.tolist() == [0.0, 0.0]


@pytest.fixture(scope='module')
def batch():
    """The two fixtures as one two-file batch resident on the device, with the records, labels and
    segments of their displaced input."""
    fix = [_fixture(i) for i in range(len(FIXTURES))]
    b = Batch([(feats, vad, segs) for feats, vad, _, segs, _, _ in fix])
    b.fix = fix
    yield b
    b.close()


def _rows_wrong(rows, truth, n_frames):
    lab = np.full(n_frames, -1, dtype=np.int64)
    for s, e, k in rows:
        lab[int(round(s * RATE)):int(round(e * RATE))] = int(k) - 1
    return int((lab != S.truth_labels(truth, n_frames)).sum())


@pytest.mark.gpu
def test_soft_resegmentation_end_to_end(batch):
    """RESEG_SOFT at passes=8 on the two fixtures as one batch: per file the rows of the restated loop --
    their count and labels, every boundary within 2 frames (the weights pass through a float32 posterior that
    device and numpy agree on to 2^-23, not to the bit) -- at least 50 wrong frames fewer than the same call
    with soft=False, masses that add up to the file's turn frames, fewer than 8 passes."""
    p = batch.pipeline
    reseg = dict(p.RESEG_SOFT, passes=8)
    det, timings = {}, {}
    rows = batch.run(reseg, det, timings)
    hard_det = {}
    hard_rows = batch.run(dict(reseg, soft=False), hard_det)
    assert 'soft_mass' not in hard_det
    assert det['passes_run'] < 8 and det['dropped'] == []
    n_train = det['passes_run'] - 1
    assert len(det['soft_mass']) == n_train >= 1
    assert len(timings['reseg_soft_posterior']) == len(timings['reseg_soft_stats']) == n_train
    assert all(v > 0.0 for k in ('reseg_soft_posterior', 'reseg_soft_stats') for v in timings[k])
    assert len(timings['reseg_models']) == len(timings['reseg_loglik']) == det['passes_run']
    print('soft stage per pass (ms): %s' % {k: [round(v, 4) for v in timings[k]] for k in sorted(timings)})
    spk_base = 0
    for i, (feats, vad, truth, segs, hard, soft) in enumerate(batch.fix):
        spk, out = soft[0], soft[1][-1]
        want = np.concatenate([R.rows_of_turn(fr, words, a / RATE, b / RATE, [k + 1 for k in spk], RATE, False)
                               for (a, b), (fr, words) in zip(vad, out)])
        got = rows[i]
        assert len(got) == len(want) and got[:, 2].tolist() == want[:, 2].tolist(), i
        shift = np.abs(np.rint(got[:, :2] * RATE) - np.rint(want[:, :2] * RATE))
        print('file %d: %d of %d boundaries differ from the restatement (largest %d frames)'
              % (i, int((shift[:, 0] > 0).sum()), len(got), int(shift.max())))
        assert shift.max() <= 2, i
        w_soft, w_hard = _rows_wrong(got, truth, len(feats)), _rows_wrong(hard_rows[i], truth, len(feats))
        print('file %d: wrong frames soft %d, hard %d' % (i, w_soft, w_hard))
        assert w_soft <= w_hard - GAIN, i
        turn_frames = sum(b - a for a, b in vad)
        n = len(spk)
        for mass in det['soft_mass']:
            assert mass.dtype == np.float64
            assert abs(mass[spk_base:spk_base + n].sum() - turn_frames) <= 1e-3 * turn_frames, i
        spk_base += n
    assert all(len(m) == spk_base for m in det['soft_mass'])
    # diarize_batch passes the dictionary through
    d2 = {}
    got = p.diarize_batch(batch.ctx, batch.eng.d_frames, len(batch.frames), batch.files, rate=RATE, reseg=p.RESEG_SOFT, detail=d2)
    assert 'soft_mass' in d2 and len(d2['soft_mass']) == d2['passes_run'] - 1 and all(len(r) for r in got)


@pytest.mark.gpu
def test_without_soft_the_rows_are_unchanged_to_the_byte(batch):
    p = batch.pipeline
    base = dict(p.RESEG, passes=2)
    absent, off = batch.run(base, {}), batch.run(dict(base, soft=False), {})
    assert [r.tobytes() for r in absent] == [r.tobytes() for r in off]
    assert all(len(r) for r in absent)
