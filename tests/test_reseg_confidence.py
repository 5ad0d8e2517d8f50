"""Speaker posteriors on the device: spkd_fb_posterior_batch, its restatement (tests/reseg_fb_numpy.py)
against an enumeration of all paths, and reseg['confidence'] in pipeline.resegment_batch /
diarize_batch.  PARITY: no reference counterpart."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import reseg_fb_numpy as F
import reseg_numpy as R
from helpers import ROOT
from conftest import pkg
from reseg_helpers import (Batch, StubContext, close_session as _close_session, normal_scores as _normal_scores,
                           ptr as _ptr)

RATE = 125.0
L = np.longdouble
EPS = 2.0 ** -52
MARGIN = 64.0        # device against the np.longdouble restatement, in units of max(CPU fp64 error, 2^-52)


# ------------------------------------------------------------------ not GPU
def test_entry_point_timer_and_tile_are_declared_exported_and_bound():
    hipabi = pkg('hipabi')
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'spkd.h')).read(), flags=re.S)
    lib = hipabi.load_library()
    name = 'spkd_fb_posterior_batch'
    assert re.search(r'\b%s\s*\(' % name, code)
    assert name in hipabi.EXPORTS and hasattr(lib, name) and hasattr(hipabi.Context, 'fb_posterior_batch')
    assert lib.spkd_abi_version() == 2 and re.search(r'#define SPKD_ABI_VERSION 2\b', code)
    enum = re.search(r'enum \{\s*SPKD_T_CALL = 0,(.*?)SPKD_N_TIMERS', code, flags=re.S).group(1)
    names = ['call'] + [n.strip()[len('SPKD_T_'):].lower() for n in enum.split(',') if n.strip()]
    at = names.index('clr_link')
    assert names[at:at + 4] == ['clr_link', 'mindur_viterbi', 'mindur_backtrack', 'fb_posterior']
    assert names[-2:] == ['mfcc_static', 'mfcc_post'] and len(names) == len(set(names))
    assert [n for n, _ in sorted(hipabi.TIMERS.items(), key=lambda kv: kv[1])] == names
    kern = open(os.path.join(ROOT, 'speaker-diarization_amd', 'csrc', 'spkd_fb.hpp')).read()
    tile = int(re.search(r'#define SPKD_FB_TILE (\d+)', code).group(1))
    assert tile == hipabi.FB_TILE == int(re.search(r'constexpr int FB_TILE = (\d+);', kern).group(1))
    assert 'PARITY: no reference counterpart' in kern


def _refusals():
    """(name, call(lib, ctx handle) -> status) of every argument refusal of the entry point.  The valid
    call: 3 sequences of 10, 0 and 20 frames, 3 columns, tokens (0, 4 | | 0)."""
    dev = C.c_void_p(4096)                        # never dereferenced: the refusal comes first
    keep = []

    def fb(n_seq=3, off=(0, 10, 10, 30), n_cols=3, penalty=1.0, scale=1.0, ncol=None, tok_off=(0, 2, 2, 3),
           tok_frame=(0, 4, 0), tok_word=(1, 0, 2), scores=dev, conf=True, logz=True):
        arr = lambda v, t: None if v is None else np.array(v, dtype=t)
        a = [arr(off, np.int64), arr(ncol, np.int32), arr(tok_off, np.int64), arr(tok_frame, np.int64),
             arr(tok_word, np.int32), np.zeros(8) if conf else None, np.zeros(8) if logz else None]
        keep.append(a)
        p = [None if x is None else _ptr(x) for x in a]
        return lambda lib, h: lib.spkd_fb_posterior_batch(h, scores, n_seq, p[0], n_cols, penalty, scale, p[1], p[2], p[3],
                                                          p[4], None, p[5], p[6])

    return [
        ('negative sequence count', fb(n_seq=-1)), ('null frame_off', fb(off=None)),
        ('frame_off not from 0', fb(off=(1, 10, 10, 30))), ('frame_off decreases', fb(off=(0, 10, 9, 30))),
        ('no column', fb(n_cols=0)), ('a 17th column', fb(n_cols=17)),
        ('n(q) of 0', fb(ncol=(3, 0, 1))), ('n(q) above n_cols', fb(ncol=(3, 1, 4))),
        ('negative penalty', fb(penalty=-1.0)), ('NaN penalty', fb(penalty=float('nan'))),
        ('infinite penalty', fb(penalty=float('inf'))),
        ('scale 0', fb(scale=0.0)), ('negative scale', fb(scale=-1.0)), ('NaN scale', fb(scale=float('nan'))),
        ('infinite scale', fb(scale=float('inf'))), ('scale * penalty above 600', fb(penalty=50.0, scale=12.5)),
        ('tokens without tok_off', fb(tok_off=None)), ('tokens without frames', fb(tok_frame=None)),
        ('tokens without words', fb(tok_word=None)),
        ('tok_off not from 0', fb(tok_off=(1, 2, 2, 3))), ('tok_off decreases', fb(tok_off=(0, 2, 1, 3))),
        ('tokens not from frame 0', fb(tok_frame=(1, 4, 0))), ('tokens do not ascend', fb(tok_frame=(0, 0, 0))),
        ('tokens descend', fb(tok_off=(0, 3, 3, 4), tok_frame=(0, 5, 4, 0), tok_word=(0, 1, 0, 0))),
        ('a token at T', fb(tok_frame=(0, 10, 0))),
        ('a sequence with frames and no token', fb(tok_off=(0, 2, 2, 2), tok_frame=(0, 4), tok_word=(1, 0))),
        ('tokens on a sequence without frames', fb(tok_off=(0, 1, 2, 3), tok_frame=(0, 0, 0))),
        ('negative word', fb(tok_word=(1, -1, 2))), ('word at n_cols', fb(tok_word=(1, 0, 3))),
        ('null conf with tokens', fb(conf=False)), ('null logz', fb(logz=False)),
        ('null scores', fb(scores=None)),
    ]


def test_every_refusal_is_einval_without_a_context():
    hipabi = pkg('hipabi')
    lib = hipabi.load_library()
    for name, call in _refusals():
        assert call(lib, None) == hipabi.SPKD_EINVAL, name


def _planted(rng, T, W):
    """normal(-60, 8) scores with a -inf, a frame nobody can score and a NaN planted."""
    sc = rng.normal(-60.0, 8.0, (T, W)).astype(np.float32)
    if T >= 2:
        sc[int(rng.integers(0, T)), int(rng.integers(0, W))] = -np.inf
    if T >= 3 and rng.integers(0, 2) == 0:
        sc[int(rng.integers(0, T))] = -np.inf
    if T >= 2 and rng.integers(0, 2) == 0:
        sc[int(rng.integers(0, T)), int(rng.integers(0, W))] = np.nan
    return sc


def test_restatement_is_the_enumeration_of_all_paths():
    """|gamma - brute| <= 1e-12, |logz - brute| <= 1e-10: both about 1e4 over what the fp64 recursion
    measured against the enumeration (1.2e-16, 3e-14), room for another libm."""
    rng = np.random.default_rng(2026)
    worst_g = worst_z = 0.0
    n = 0
    for W in (1, 2, 3):
        for T in (1, 2, 5, 7):
            for penalty in (0.0, 2.5, 50.0):
                for scale in (1.0, 0.25):
                    for nq in sorted({W, max(1, W - 1)}):
                        sc = _planted(rng, T, W)
                        gamma, logz = F.posterior(sc, penalty, scale, nq)
                        bg, bz = F.brute_force(sc, penalty, scale, nq)
                        assert np.isfinite(gamma).all() and np.isfinite(logz)
                        dg, dz = float(np.abs(gamma - bg).max()), float(abs(logz - bz))
                        assert dg <= 1e-12 and dz <= 1e-10, (W, T, penalty, scale, nq, dg, dz)
                        assert (gamma[:, nq:] == 0.0).all()
                        worst_g, worst_z = max(worst_g, dg), max(worst_z, dz)
                        n += 1
    print('restatement against all paths, %d cases: gamma %.3g, logz %.3g' % (n, worst_g, worst_z))
    assert n == 3 * 4 * 3 * 2 * 2 - 4 * 3 * 2           # (W = 1 has one n(q))
    g, z = F.posterior(np.zeros((0, 3), dtype=np.float32), 1.0)
    assert g.shape == (0, 3) and z == -np.inf


@pytest.mark.parametrize('W', [1, 4, 16])
def test_invariants_of_the_restatement(W):
    rng = np.random.default_rng(300 + W)
    T = 300
    for penalty, scale in ((0.0, 1.0), (2.5, 1.0), (50.0, 1.0), (50.0, 0.25)):
        sc = rng.normal(-60.0, 8.0, (T, W)).astype(np.float32)
        who = np.repeat(rng.integers(0, W, T // 50 + 1), 50)[:T]
        sc[np.arange(T), who] += 6.0
        nq = max(1, W - 1)
        for n in sorted({W, nq}):
            gamma, logz = F.posterior(sc, penalty, scale, n)
            assert (np.abs(gamma.sum(axis=1) - 1.0) <= 4 * EPS).all()          # rows sum to 1 within 4 ulp
            assert (gamma >= 0.0).all() and (gamma[:, n:] == 0.0).all()        # columns >= n(q): exactly 0
            if scale == 1.0:
                assert logz >= R.viterbi(sc[:, :n], penalty)[2]
        if W == 1:
            gamma, logz = F.posterior(sc, penalty, scale)
            want = scale * (-penalty + float(sc.astype(np.float64).sum()))
            assert (gamma == 1.0).all() and abs(logz - want) <= 1e-9 * abs(want)


def test_value_errors_come_before_any_device_work():
    pipeline = pkg('pipeline')
    assert pipeline.RESEG_CONF == dict(penalty=50.0, confidence=True) and pipeline.RESEG == dict(penalty=50.0)
    files = [pipeline.BatchFile(0, 1000, [(0.0, 8.0)])]
    labels = [np.array([1, 2])]

    def both(reseg, match, detail):
        with pytest.raises(ValueError, match=match):
            pipeline.resegment_batch(None, 0, 1000, files, 0, [0, 2], labels, reseg=reseg, detail=detail)
        with pytest.raises(ValueError, match=match):
            pipeline.diarize_batch(None, 0, 0, [], reseg=reseg, detail=detail)

    both(pipeline.RESEG_CONF, 'reseg confidence', None)                    # nowhere to put them
    for bad in (1, 0, 'yes', None, 1.0):
        both(dict(penalty=50.0, confidence=bad), 'reseg confidence', {})
    for bad in (0.0, -1.0, float('nan'), float('inf'), 'half'):
        both(dict(penalty=50.0, confidence=True, conf_scale=bad), 'reseg conf_scale', {})
        both(dict(penalty=50.0, conf_scale=bad), 'reseg conf_scale', {})
    both(dict(penalty=50.0, confidence=True, conf_scale=12.5), 'conf_scale \\* penalty', {})
    both(dict(penalty=601.0, confidence=True), 'conf_scale \\* penalty', {})
    stage = pkg('resegmentation')
    assert stage._reseg_confidence(dict(penalty=50.0), None) == (False, 1.0)
    assert stage._reseg_confidence(dict(penalty=601.0), None) == (False, 1.0)           # (the limit is the posterior's)
    assert stage._reseg_confidence(dict(penalty=50.0, confidence=True, conf_scale=12), {}) == (True, 12.0)
    # an empty batch, and a batch without speakers: empty arrays
    det = {}
    assert pipeline.diarize_batch(None, 0, 0, [], reseg=pipeline.RESEG_CONF, detail=det) == []
    assert det['confidence'] == [] and det['log_evidence'] == [] and det['passes_run'] == 0
    det = {}
    rows = pipeline.resegment_batch(None, 0, 1000, files, 0, [0, 0], [np.zeros(0, dtype=np.int32)], reseg=pipeline.RESEG_CONF,
                                    detail=det)
    assert [r.shape for r in rows] == [(0, 3)]
    assert [a.shape for a in det['confidence']] == [(0,)] and [a.shape for a in det['log_evidence']] == [(0,)]
    det = {}
    pipeline.resegment_batch(None, 0, 1000, files, 0, [0, 0], [np.zeros(0, dtype=np.int32)], detail=det)
    assert 'confidence' not in det and 'log_evidence' not in det


class _StubContext(StubContext):
    """The final posterior call with all its arguments; a confidence and a log-evidence that tell the rows and
    the turns apart."""
    MS = {'fb_posterior': 0.75}

    def fb_posterior_batch(self, d_scores, frame_off, n_cols, penalty, tokens=None, seq_n_cols=None, scale=1.0, d_post=0):
        self.calls.append(('fb', d_scores, np.array(frame_off).tolist(), n_cols, penalty, [np.array(t).tolist() for t in tokens],
                           np.array(seq_n_cols).tolist(), scale, d_post))
        n_tok = len(tokens[1])
        return 0.5 + np.arange(n_tok) / 16.0, -100.0 - np.arange(len(frame_off) - 1)


def test_the_pipeline_calls_the_posterior_once_behind_the_last_decode():
    """Two files: file 0 has speakers 1 and 2 and the turns (1, 3) and (4, 6) s; file 1 has speakers 3, 5, 7
    and one turn (0, 2) s.  The confidences come back split per file in row order, the log-evidences per
    file in turn order, and the rows are those of the call without confidence to the byte."""
    pipeline = pkg('pipeline')
    files = [pipeline.BatchFile(0, 1000, [(1.0, 3.0), (4.0, 6.0)]), pipeline.BatchFile(1000, 1000, [(0.0, 2.0)])]
    labels = [np.array([2, 1, 2]), np.array([7, 3, 5])]
    first = [[(0, 1), (100, 0)], [(0, 0)], [(0, 2), (60, 0), (200, 1)]]
    second = [[(0, 1), (90, 0)], [(0, 0)], [(0, 2), (60, 0), (200, 1)]]
    args = (1 << 20, 2000, files, 1 << 21, [0, 3, 6], labels, RATE)
    for reseg in (pipeline.RESEG, pipeline.RESEG_MD, dict(penalty=7.0, passes=3), dict(penalty=7.0, confidence=False)):
        stub, det = _StubContext([first, second, second]), {}
        pipeline.resegment_batch(stub, *args, reseg, False, None, det)
        assert 'fb' not in [c[0] for c in stub.calls] and 'confidence' not in det and 'log_evidence' not in det
    for base, decode, n_dec in ((dict(penalty=7.0), 'decode', 1), (dict(penalty=7.0, min_dur_s=0.5), 'decode_md', 1),
                                (dict(penalty=7.0, passes=5), 'decode', 3)):
        stub, plain_stub, det, timings = _StubContext([first, second, second]), _StubContext([first, second, second]), {}, {}
        rows = pipeline.resegment_batch(stub, *args, dict(base, confidence=True), False, timings, det)
        plain = pipeline.resegment_batch(plain_stub, *args, base, False)
        names = [c[0] for c in stub.calls]
        assert names.count('fb') == 1 and names[-1] == 'fb' and names[-2] == decode and names.count(decode) == n_dec
        assert names[:-1] == [c[0] for c in plain_stub.calls]
        last = second if n_dec > 1 else first
        want_tokens = [[0, 2, 3, 6], [f for t in last for f, _ in t], [w for t in last for _, w in t]]
        assert stub.calls[-1][1:] == (12288, [0, 250, 500, 750], 3, 7.0, want_tokens, [2, 2, 3], 1.0, 0)
        assert [r.tobytes() for r in rows] == [r.tobytes() for r in plain]
        assert [len(r) for r in rows] == [3, 3]
        assert [c.tolist() for c in det['confidence']] == [[0.5, 0.5625, 0.625], [0.6875, 0.75, 0.8125]]
        assert [z.tolist() for z in det['log_evidence']] == [[-100.0, -101.0], [-102.0]]
        assert timings['reseg_posterior'] == [0.75]
    stub, det = _StubContext([first]), {}
    pipeline.resegment_batch(stub, *args, dict(penalty=12.0, confidence=True, conf_scale=0.25), False, None, det)
    assert stub.calls[-1][4] == 12.0 and stub.calls[-1][7] == 0.25


# ------------------------------------------------------------------ GPU
def _host_tokens(hipabi, seqs, ncol, penalty):
    """The tokens of the host decoder on every sequence's first n(q) columns, as a decoder hands them back."""
    tok_off, frames, words = [0], [], []
    for sc, n in zip(seqs, ncol):
        if len(sc):
            zero = np.zeros(n)
            tf, tw, _ = hipabi.vad_viterbi(sc[:, :n], np.arange(n), zero, zero, zero - penalty)
            frames += tf.tolist()
            words += tw.tolist()
        tok_off.append(len(frames))
    return np.array(tok_off, dtype=np.int64), np.array(frames, dtype=np.int64), np.array(words, dtype=np.int32)


def _ragged(W, seed):
    T = pkg('hipabi').FB_TILE
    rng = np.random.default_rng(seed)
    choice = [0, 1, 2, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 700]
    lens = [int(choice[i]) for i in rng.integers(0, len(choice), 70)]
    lens[3], lens[40], lens[69] = 700, 700, 0
    seqs = [_normal_scores(rng, n, W) for n in lens]
    ncol = rng.integers(1, W + 1, 70).astype(np.int32)
    ncol[3] = W
    return lens, seqs, ncol


def _restated(seqs, ncol, tokens, penalty, scale, dtype):
    """(gamma per sequence, conf of all tokens, logz per sequence) of the restatement in `dtype`."""
    tok_off, tok_frame, tok_word = tokens
    gammas, conf, logz = [], [], []
    for q, (sc, n) in enumerate(zip(seqs, ncol)):
        g, z = F.posterior(sc, penalty, scale, int(n), dtype)
        a, b = int(tok_off[q]), int(tok_off[q + 1])
        gammas.append(g)
        conf.append(F.confidence(g, tok_frame[a:b], tok_word[a:b]))
        logz.append(z)
    return gammas, np.concatenate(conf), np.array(logz, dtype=dtype)


@pytest.fixture(scope='module')
def ctx():
    c = pkg('hipabi').Context(0)
    yield c
    c.close()


CASES = [(W, p, 1.0) for W in (1, 2, 3, 8, 16) for p in (0.0, 2.5, 50.0)] + [(3, 50.0, 0.25)]


@pytest.mark.gpu
@pytest.mark.parametrize('W,penalty,scale', CASES)
def test_device_is_the_restatement(ctx, W, penalty, scale):
    """70 ragged sequences in one call (several share a wave, more than one wave), n(q) ragged, against the
    restatement in np.longdouble: d_post within 2^-23 (the float32 rounding), conf within 64 max(e, 2^-52)
    and logz within 64 max(e_z, 2^-52 |logz|), e and e_z what the fp64 restatement differs by on the same
    inputs.  64: the device's exp and log are good to about 1 ulp where glibc's are to about 0.5, the order
    of the sums and the reciprocals add a few ulp a frame, the recursion forgets old errors, and logz adds
    them over at most 700 frames, which its relative form covers."""
    hipabi = pkg('hipabi')
    lens, seqs, ncol = _ragged(W, 1000 * W + int(10 * penalty) + int(100 * scale))
    tokens = _host_tokens(hipabi, seqs, ncol, penalty)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    flat = np.concatenate(seqs + [np.zeros((1, W), dtype=np.float32)])
    post = np.full((int(off[-1]) + 1, W), -7.0, dtype=np.float32)
    d, d_post = ctx.dev_alloc(flat.nbytes), ctx.dev_alloc(post.nbytes)
    try:
        ctx.h2d(d, flat)
        ctx.h2d(d_post, post)
        conf, logz = ctx.fb_posterior_batch(d, off, W, penalty, tokens=tokens, seq_n_cols=ncol, scale=scale, d_post=d_post)
        assert ctx.last_ms('fb_posterior') > 0.0
        ctx.d2h(post, d_post)
    finally:
        ctx.dev_free(d)
        ctx.dev_free(d_post)
    g_l, conf_l, logz_l = _restated(seqs, ncol, tokens, penalty, scale, L)
    _, conf_d, logz_d = _restated(seqs, ncol, tokens, penalty, scale, np.float64)
    e = float(np.abs(conf_d.astype(L) - conf_l).max())
    finite = np.isfinite(logz_l)
    e_z = float(np.abs(logz_d.astype(L)[finite] - logz_l[finite]).max())
    want_post = np.concatenate(g_l)
    r_post = float(np.abs(post[:-1].astype(L) - want_post).max() / L(2.0 ** -23))
    r_conf = float(np.abs(conf.astype(L) - conf_l).max() / L(MARGIN * max(e, EPS)))
    bound_z = MARGIN * np.maximum(e_z, EPS * np.abs(logz_l[finite]).astype(np.float64))
    r_logz = float((np.abs(logz.astype(L)[finite] - logz_l[finite]).astype(np.float64) / bound_z).max())
    print('fb ratios W=%d penalty=%g scale=%g: post %.3f conf %.3f logz %.3f of the bounds (e %.3g, e_z %.3g)'
          % (W, penalty, scale, r_post, r_conf, r_logz, e, e_z))
    assert (post[-1] == -7.0).all()                                        # nothing behind the last frame
    for q, n in enumerate(ncol):
        assert (post[off[q]:off[q + 1], n:] == 0.0).all(), q               # columns >= n(q): exactly 0
    assert (logz[~finite] == -np.inf).all() and [lens[q] for q in np.nonzero(~finite)[0]] == [0] * int((~finite).sum())
    assert np.isfinite(post[:-1]).all() and np.isfinite(conf).all()
    assert r_post <= 1.0 and r_conf <= 1.0 and r_logz <= 1.0


@pytest.mark.gpu
def test_consistency_empty_calls_and_refusals_with_a_context(ctx):
    hipabi = pkg('hipabi')
    for name, call in _refusals():
        assert call(ctx.lib, ctx.h) == hipabi.SPKD_EINVAL, name
    # empty calls: no sequence; sequences without frames
    conf, logz = ctx.fb_posterior_batch(0, [0], 3, 1.0)
    assert conf is None and len(logz) == 0
    empty = (np.zeros(3, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32))
    conf, logz = ctx.fb_posterior_batch(0, [0, 0, 0], 3, 1.0, tokens=empty)
    assert len(conf) == 0 and logz.tolist() == [-np.inf, -np.inf]
    W, penalty = 3, 2.5
    lens, seqs, ncol = _ragged(W, 4242)
    tokens = _host_tokens(hipabi, seqs, ncol, penalty)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    flat = np.concatenate(seqs + [np.zeros((1, W), dtype=np.float32)])
    d, d_post = ctx.dev_alloc(flat.nbytes), ctx.dev_alloc(flat.nbytes)
    try:
        ctx.h2d(d, flat)
        with_post = ctx.fb_posterior_batch(d, off, W, penalty, tokens=tokens, seq_n_cols=ncol, d_post=d_post)
        without = ctx.fb_posterior_batch(d, off, W, penalty, tokens=tokens, seq_n_cols=ncol)
        again = ctx.fb_posterior_batch(d, off, W, penalty, tokens=tokens, seq_n_cols=ncol)
        none, logz_only = ctx.fb_posterior_batch(d, off, W, penalty, seq_n_cols=ncol)
        # a +inf score: that sequence's outputs are NaN and nothing else is
        q = 40
        assert lens[q] == 700
        bad = flat.copy()
        bad[off[q] + 350, 0] = np.inf
        ctx.h2d(d, bad)
        conf_i, logz_i = ctx.fb_posterior_batch(d, off, W, penalty, tokens=tokens, seq_n_cols=ncol, d_post=d_post)
        post = np.empty_like(flat)
        ctx.d2h(post, d_post)
    finally:
        ctx.dev_free(d)
        ctx.dev_free(d_post)
    for got in (without, again):
        assert got[0].tobytes() == with_post[0].tobytes() and got[1].tobytes() == with_post[1].tobytes()
    assert none is None and logz_only.tobytes() == with_post[1].tobytes()
    a, b = int(tokens[0][q]), int(tokens[0][q + 1])
    mine = np.zeros(len(conf_i), dtype=bool)
    mine[a:b] = True
    assert np.isnan(conf_i[mine]).all() and conf_i[~mine].tobytes() == with_post[0][~mine].tobytes()
    assert np.isnan(logz_i[q]) and np.delete(logz_i, q).tobytes() == np.delete(with_post[1], q).tobytes()
    assert np.isnan(post[off[q]:off[q + 1], :ncol[q]]).all() and np.isfinite(post[:off[q]]).all()
    assert np.isfinite(post[off[q + 1]:-1]).all()


@pytest.fixture(scope='module')
def batch():
    """Two 40 s files of 2 and 3 close speakers resident on the device, their truth segments' records,
    labels and segments."""
    b = Batch([_close_session(7000, 40.0, 2), _close_session(7001, 40.0, 3)])
    yield b
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['RESEG_CONF', 'RESEG_MD', 'RESEG_GMM'])
def test_confidence_end_to_end(batch, name):
    """The rows are those of the same configuration without confidence; every row has a confidence in
    (0, 1] that is the restatement's on the scores the last pass left and the returned rows' tokens; for
    the plain decoder the log-evidence is not below the decoder's path score."""
    p, ctx, hipabi = batch.pipeline, batch.ctx, batch.hipabi
    base = dict(dict(p.RESEG_MD, passes=2) if name == 'RESEG_MD' else getattr(p, name))
    base.pop('confidence', None)
    args = (ctx, batch.eng.d_frames, batch.frames.shape[0], batch.files, batch.d_stats, batch.seg_off, batch.labels, RATE)
    plain = p.resegment_batch(*args, base, False, None, {}, batch.segments)
    det, timings = {}, {}
    rows = p.resegment_batch(*args, dict(base, confidence=True), False, timings, det, batch.segments)
    assert [r.tobytes() for r in rows] == [r.tobytes() for r in plain]
    assert len(timings['reseg_posterior']) == 1 and timings['reseg_posterior'][0] > 0.0
    owner, _, _, ls, le, tb, te = p._turn_table(batch.files, RATE)
    n_cols = 3
    sc = np.empty((int((te - tb).sum()), n_cols), dtype=np.float32)
    ctx.d2h(sc, ctx.dev_scratch('reseg_scores', 0))
    off = np.concatenate([[0], np.cumsum(te - tb)])
    n_spk = [2, 3]
    penalty = base['penalty']
    for f in range(2):
        conf, logz = det['confidence'][f], det['log_evidence'][f]
        assert conf.dtype == np.float64 and len(conf) == len(rows[f]) and ((conf > 0.0) & (conf <= 1.0)).all()
        turns = np.nonzero(owner == f)[0]
        assert len(logz) == len(turns) and np.isfinite(logz).all()
        labs = sorted(set(batch.labels[f].tolist()))
        k = 0
        for i, q in enumerate(turns):
            s = sc[off[q]:off[q + 1]]
            mine = (rows[f][:, 0] >= ls[q]) & (rows[f][:, 0] < le[q])
            r = rows[f][mine]
            frames = np.rint((r[:, 0] - ls[q]) * RATE).astype(np.int64)
            words = np.array([labs.index(int(v)) for v in r[:, 2]])
            g_l, z_l = F.posterior(s, penalty, 1.0, n_spk[f], L)
            g_d, z_d = F.posterior(s, penalty, 1.0, n_spk[f], np.float64)
            c_l, c_d = F.confidence(g_l, frames, words), F.confidence(g_d, frames, words)
            e = float(np.abs(c_d.astype(L) - c_l).max())
            assert (np.abs(conf[k:k + len(r)].astype(L) - c_l) <= MARGIN * max(e, EPS)).all(), (f, q)
            e_z = float(abs(L(z_d) - z_l))
            assert abs(L(logz[i]) - z_l) <= MARGIN * max(e_z, EPS * float(abs(z_l))), (f, q)
            if name == 'RESEG_CONF':
                zero = np.zeros(n_spk[f])
                best = hipabi.vad_viterbi(s[:, :n_spk[f]], np.arange(n_spk[f]), zero, zero, zero - penalty)[2]
                assert logz[i] >= best
            k += len(r)
        assert k == len(rows[f])
    expected_wrong = sum(float((1.0 - c).dot(np.rint((r[:, 1] - r[:, 0]) * RATE))) for c, r in zip(det['confidence'], rows))
    print('%s: expected wrong frames sum((1 - conf) * length) = %.2f' % (name, expected_wrong))


@pytest.mark.gpu
def test_diarize_batch_hands_the_confidences_through(batch):
    p, ctx = batch.pipeline, batch.ctx
    args = (ctx, batch.eng.d_frames, batch.frames.shape[0], batch.files)
    det = {}
    got = p.diarize_batch(*args, rate=RATE, reseg=p.RESEG_CONF, detail=det)
    plain = p.diarize_batch(*args, rate=RATE, reseg=p.RESEG)
    assert [r.tobytes() for r in got] == [r.tobytes() for r in plain] and all(len(r) for r in got)
    assert [len(c) for c in det['confidence']] == [len(r) for r in got]
    assert all(((c > 0.0) & (c <= 1.0)).all() for c in det['confidence'])
    assert [len(z) for z in det['log_evidence']] == [len(f.vad) for f in batch.files]
