"""The decision part of stage 1 for a whole batch on the device (spkd_vad_shift_batch,
spkd_vad_viterbi_batch, exp_generator.decode_batch, pipeline.vad_batch) against the per-file path:
the host decoder spkd_vad_viterbi on every file's slice (tokens and scores equal to the bit) and
shift_dec_bord's arithmetic in numpy.

Shift tolerance, derived: |got - want| <= spacing32(want) + 2e-15.  The first term is the one
rounding to float32 both sides end with.  The second covers a few fp64 ulp between the device
library's exp / log and the host's: where the ratio is near 1 the log has unit gain, so an error of
k * 2^-53 in the ratio is k * 1.1e-16 in a result near 0, below any float32 spacing there.  Because
of that slack every decoder comparison here decodes the DEVICE's shifted scores on the host."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import vad_numpy as vn
from conftest import pkg
from helpers import ROOT
from test_generate_exp import CONSTS, _signal, _synthetic_mixtures, _write_wav, load_model, write_model

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SHIFT = 0.2


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------ not GPU
def test_entry_points_are_declared_and_exported():
    hipabi = pkg('hipabi')
    text = open(os.path.join(ROOT, 'include', 'spkd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    vmap = open(os.path.join(ROOT, 'speaker-diarization_amd', 'csrc', 'libspkd_hip.map')).read()
    lib = hipabi.load_library()
    for name in ('spkd_vad_shift_batch', 'spkd_vad_viterbi_batch'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in hipabi.EXPORTS and hasattr(lib, name)
    assert re.search(r'global:\s*spkd_\*;', vmap)
    assert lib.spkd_abi_version() == 2 and re.search(r'#define SPKD_ABI_VERSION 2\b', code)
    for t in ('vad_shift', 'vad_viterbi', 'vad_backtrack'):
        assert t in hipabi.TIMERS
    # the tile is one named constant: header, kernels and binding agree
    kern = open(os.path.join(ROOT, 'speaker-diarization_amd', 'csrc', 'spkd_vad_batch.hpp')).read()
    tile = int(re.search(r'#define SPKD_VAD_TILE (\d+)', code).group(1))
    assert tile == hipabi.VAD_TILE == int(re.search(r'constexpr int VB_TILE = (\d+);', kern).group(1))
    names = [n for n, _ in sorted(hipabi.TIMERS.items(), key=lambda kv: kv[1])]
    enum = re.search(r'enum \{\s*SPKD_T_CALL = 0,(.*?)SPKD_N_TIMERS', code, flags=re.S).group(1)
    assert ['call'] + [n.strip()[len('SPKD_T_'):].lower() for n in enum.split(',') if n.strip()] == names


def _refusals(hipabi):
    """(name, call(lib, ctx handle) -> status) of every argument refusal."""
    ws = np.array([0, 1], dtype=np.int32)
    k = [np.zeros(16) for _ in range(3)]
    good = np.array([0, 3, 5], dtype=np.int64)
    down = np.array([0, 3, 2], dtype=np.int64)
    late = np.array([1, 3, 5], dtype=np.int64)
    many = np.zeros(17, dtype=np.int32)
    out = [C.c_void_p() for _ in range(4)]
    refs = [C.byref(o) for o in out]
    dev = C.c_void_p(256)                         # never dereferenced: the refusal comes first

    def vit(off, S, W, wst):
        return lambda lib, h: lib.spkd_vad_viterbi_batch(h, dev, 2, _ptr(off), S, W, _ptr(wst), _ptr(k[0]), _ptr(k[1]),
                                                         _ptr(k[2]), *refs)

    def shift(off, S):
        return lambda lib, h: lib.spkd_vad_shift_batch(h, dev, 2, _ptr(off), S, SHIFT, dev)

    return [('decreasing frame_off, decoder', vit(down, 2, 2, ws)),
            ('decreasing frame_off, shift', shift(down, 2)),
            ('frame_off not from 0', vit(late, 2, 2, ws)),
            ('word state out of range', vit(good, 2, 2, np.array([0, 2], dtype=np.int32))),
            ('negative word state', vit(good, 2, 2, np.array([-1, 1], dtype=np.int32))),
            ('one state for the shift', shift(good, 1)),
            ('17 words', vit(good, 2, 17, many)),
            ('17 states', vit(good, 17, 2, ws)),
            ('no words', vit(good, 2, 0, ws))]


def test_argument_refusals_come_before_any_device_work():
    """No context, no device: every refusal is SPKD_EINVAL (with a context: the GPU test below)."""
    hipabi = pkg('hipabi')
    lib = hipabi.load_library()
    for name, call in _refusals(hipabi):
        assert call(lib, None) == hipabi.SPKD_EINVAL, name


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def ctx():
    c = pkg('hipabi').Context(0)
    yield c
    c.close()


def _upload(ctx, files, name='test_scores'):
    """Files [T, S] float32 concatenated on the device -> (pointer, frame_off)."""
    S = files[0].shape[1]
    off = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
    flat = np.concatenate(files).astype(np.float32).reshape(-1, S)
    d = ctx.dev_scratch(name, max(flat.nbytes, 16))
    if flat.size:
        ctx.h2d(d, flat)
    return d, off


def _same_score(a, b):
    return (math.isnan(a) and math.isnan(b)) or np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def _check_batch(ctx, files, word_state, consts):
    """The batch call against the host decoder on every file's slice: lists equal, scores bit-equal."""
    hipabi = pkg('hipabi')
    d, off = _upload(ctx, files)
    S = files[0].shape[1]
    tok_off, frames, words, scores = ctx.vad_viterbi_batch(d, off, S, list(word_state), *consts)
    assert len(tok_off) == len(files) + 1 and tok_off[0] == 0 and len(scores) == len(files)
    for i, f in enumerate(files):
        hf, hw, hs = hipabi.vad_viterbi(f, list(word_state), *consts)
        a, b = int(tok_off[i]), int(tok_off[i + 1])
        assert list(frames[a:b]) == list(hf) and list(words[a:b]) == list(hw), (i, len(f))
        assert _same_score(scores[i], hs), (i, len(f), scores[i], hs)
    return tok_off, frames, words, scores


def _lengths(hipabi):
    t = hipabi.VAD_TILE
    return [1, 2, 3, t - 1, 0, t, t + 1, 2 * t + 1, 777]          # the empty file in the middle


@pytest.mark.gpu
def test_decoder_equals_the_host_decoder_exactly(ctx):
    hipabi = pkg('hipabi')
    rng = np.random.default_rng(17)
    lengths = _lengths(hipabi)
    zero = (np.zeros(2), np.zeros(2), np.zeros(2))
    minus = (np.full(2, -1.0), np.full(2, -1.0), np.full(2, -1.0))
    for scale in (0.5, 5.0, 40.0):
        _check_batch(ctx, [(-3.0 + scale * rng.standard_normal((T, 2))).astype(np.float32) for T in lengths], (0, 1), CONSTS)
    # ties everywhere: equal scores and symmetric constants
    tok_off, frames, words, _ = _check_batch(ctx, [np.zeros((T, 2), np.float32) for T in lengths], (0, 1), zero)
    assert list(np.diff(tok_off)) == [min(T, 1) for T in lengths] and not frames.any() and not words.any()
    _check_batch(ctx, [np.ones((T, 2), np.float32) for T in lengths], (0, 1), minus)
    # NaN rows, -inf rows, -inf mixed in -- at positions that exist in every length
    files = []
    for T in lengths:
        sc = (-2.0 + rng.standard_normal((T, 2))).astype(np.float32)
        for frac, rows, col, val in ((0.03, 1, None, np.nan), (0.04, 1, 0, np.nan), (0.17, 5, None, -np.inf),
                                     (0.27, 1, 1, -np.inf), (0.4, 10, 0, -np.inf), (0.0, 1, None, -np.inf),
                                     (0.999, 1, 1, np.nan)):
            a = int(frac * T)
            if col is None:
                sc[a:a + rows] = val
            else:
                sc[a:a + rows, col] = val
        files.append(sc)
    _check_batch(ctx, files, (0, 1), CONSTS)
    _, _, _, scores = _check_batch(ctx, [np.full((T, 2), np.nan, np.float32) for T in lengths], (0, 1), CONSTS)
    assert scores[lengths.index(0)] == -np.inf
    _check_batch(ctx, [np.full((T, 2), -np.inf, np.float32) for T in lengths], (0, 1), CONSTS)


@pytest.mark.gpu
@pytest.mark.parametrize('S,word_state', [(3, (2, 0, 1)), (1, (0,)), (2, (1, 0, 1, 1)), (5, (4, 0, 1, 3, 2, 2, 0)),
                                          (4, (0, 1, 2, 3, 3, 2, 1, 0, 2, 1, 3)), (16, tuple(range(15, -1, -1)))])
def test_decoder_with_other_word_loops(ctx, S, word_state):
    """Three words over three states, word_state (2, 0, 1), random constants -- and every group
    width of the kernel (1, 4, 8, 16 lanes per file; 2-byte and 4-byte back-pointer records)."""
    rng = np.random.default_rng(170 + len(word_state))
    W = len(word_state)
    for _ in range(2):
        files = [(rng.standard_normal((T, S)) * 4).astype(np.float32) for T in (200, 33, 0, 200, 1, 95)]
        files[3][40:44] = -np.inf
        files[3][90, 0] = np.nan
        _check_batch(ctx, files, word_state, tuple(rng.standard_normal(W) * 3 for _ in range(3)))


@pytest.mark.gpu
def test_decoder_across_waves_and_workgroups(ctx):
    """More files than a wave holds groups (32 for two words): 40 files of 50 frames, all different."""
    rng = np.random.default_rng(19)
    files = [(-3.0 + 5.0 * rng.standard_normal((50, 2))).astype(np.float32) for _ in range(40)]
    tok_off, _, _, _ = _check_batch(ctx, files, (0, 1), CONSTS)
    assert len(set(np.diff(tok_off))) > 1
    # and more files than the backtrack's one wave of lanes
    files = [(-3.0 + 5.0 * rng.standard_normal((5 + i % 7, 2))).astype(np.float32) for i in range(150)]
    _check_batch(ctx, files, (0, 1), CONSTS)


@pytest.mark.gpu
def test_decoder_finds_planted_speech_in_both_files(ctx):
    T = 1000
    sc = np.zeros((T, 2), np.float32)
    sc[:, 0], sc[:, 1] = -1.0, -60.0
    for a, b in ((100, 250), (400, 401 + 300), (900, 1000)):
        sc[a:b, 0], sc[a:b, 1] = -60.0, -1.0
    late = np.concatenate([np.tile(np.array([[-1.0, -60.0]], np.float32), (7, 1)), sc])
    tok_off, frames, words, _ = _check_batch(ctx, [sc, late], (0, 1), CONSTS)
    texts = [vn.exp_text(list(frames[a:b]), list(words[a:b]), ['<w>', 'p']) for a, b in zip(tok_off[:-1], tok_off[1:])]
    assert texts == ['0 <w> 100 p 250 <w> 400 p 701 <w> 900 p', '0 <w> 107 p 257 <w> 407 p 708 <w> 907 p']


def _host_shift(block):
    """shift_dec_bord's arithmetic (exp_generator.shift_dec_bord, generate_exp.py:177-186) on one
    file's frame-major [T, S] float32 scores, reshape quirk included."""
    T, S = block.shape
    l = block.reshape(-1).reshape((S, -1)).astype(np.float64)
    with np.errstate(all='ignore'):
        l = np.exp(l)
        l[1, :] *= SHIFT
        l /= sum(l)
        l = np.log(l)
    return l.astype(np.float32).reshape(T, S)


def _shift_files():
    cases = json.load(open(os.path.join(GOLDEN, 'generate_exp_cases.json')))['cases']
    assert sorted({c['frames'] for c in cases} & {0, 1, 7, 10}) == [0, 1, 7, 10]
    files = [np.frombuffer(bytes.fromhex(c['lna_in'])[5:], dtype='<f4').reshape(c['frames'], 2).astype(np.float32)
             for c in cases]
    rng = np.random.default_rng(23)
    files.append((-200.0 * rng.random((300, 2))).astype(np.float32))
    # underflow (-800: exp gives 0 on both sides, 55 below the -745 boundary), -inf and NaN: alone in
    # a column of the (S, T) view (-inf out), in both of its entries (0 / 0: NaN out)
    odd = (-200.0 * rng.random((65, 2))).astype(np.float32)
    flat = odd.reshape(-1)
    flat[[3, 9, 65 + 9, 70]] = -800.0
    flat[[20, 65 + 20, 31, 65 + 40]] = -np.inf
    flat[[50, 65 + 52, 53, 65 + 53]] = np.nan
    flat[[60, 65 + 60]] = [-800.0, -np.inf]
    files.append(odd)
    return files


def _run_shift(ctx, files, in_place):
    d, off = _upload(ctx, files)
    total = int(off[-1])
    d_out = d if in_place else ctx.dev_scratch('test_shifted', total * 2 * 4)
    ctx.vad_shift_batch(d, off, 2, SHIFT, None if in_place else d_out)
    got = np.empty((total, 2), dtype=np.float32)
    ctx.d2h(got, d_out)
    return got, off


@pytest.mark.gpu
def test_shift_matches_the_reference_arithmetic_per_file(ctx):
    files = _shift_files()
    got, off = _run_shift(ctx, files, in_place=False)
    seen_nan = seen_inf = 0
    for i, f in enumerate(files):
        g, want = got[off[i]:off[i + 1]], _host_shift(f)
        assert np.array_equal(np.isnan(g), np.isnan(want)), i
        assert np.array_equal(np.isposinf(g), np.isposinf(want)) and np.array_equal(np.isneginf(g), np.isneginf(want)), i
        fin = np.isfinite(want)
        err = np.abs(g[fin].astype(np.float64) - want[fin].astype(np.float64))
        bound = np.spacing(np.abs(want[fin])).astype(np.float64) + 2e-15
        print('file %d: %d frames, max error / bound %.3f' % (i, len(f), float((err / bound).max()) if err.size else 0.0))
        assert np.all(err <= bound), (i, float(err.max()))
        seen_nan += int(np.isnan(want).sum())
        seen_inf += int(np.isinf(want).sum())
    assert seen_nan >= 4 and seen_inf >= 4            # the planted patterns are there
    # in place: the same bytes
    again, _ = _run_shift(ctx, files, in_place=True)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))


@pytest.mark.gpu
def test_refusals_on_a_context_name_their_reason(ctx):
    hipabi = pkg('hipabi')
    for name, call in _refusals(hipabi):
        assert call(ctx.lib, ctx.h) == hipabi.SPKD_EINVAL, name
        assert ctx.lib.spkd_last_error(ctx.h).decode() != '', name
    with pytest.raises(hipabi.SpkdError, match='non-decreasing'):
        ctx.vad_shift_batch(256, [0, 4, 2], 2, SHIFT)
    with pytest.raises(hipabi.SpkdError, match='out of range'):
        ctx.vad_viterbi_batch(256, [0, 4], 2, [0, 2], *CONSTS)
    # no file: nothing to do, and a batch of empty files has no tokens
    tok_off, frames, words, scores = ctx.vad_viterbi_batch(0, [0], 2, [0, 1], *CONSTS)
    assert list(tok_off) == [0] and len(frames) == len(words) == len(scores) == 0
    tok_off, frames, _, scores = ctx.vad_viterbi_batch(0, [0, 0, 0], 2, [0, 1], *CONSTS)
    assert list(tok_off) == [0, 0, 0] and len(frames) == 0 and np.all(scores == -np.inf)


@pytest.mark.gpu
def test_vad_batch_equals_the_per_file_composition(ctx, tmp_path):
    """Two wavs of different lengths through pipeline.vad_batch against, per file: device_scores,
    the batch shift of those scores, the HOST decoder on the shifted scores copied back,
    turns_from_tokens, py2_roundtrip."""
    hipabi, eg, vd, pipeline, fe = (pkg(n) for n in ('hipabi', 'exp_generator', 'voice_detection', 'pipeline', 'frontend'))
    rng = np.random.default_rng(11)
    write_model(str(tmp_path), *_synthetic_mixtures(rng))
    model = load_model(str(tmp_path))
    pcms = []
    for name, seconds, seed in (('a.wav', 9.0, 41), ('b.wav', 6.3, 43)):
        _write_wav(os.path.join(str(tmp_path), name), _signal(seconds, seed))
        pcm, rate = fe.read_wav(os.path.join(str(tmp_path), name))
        assert rate == model.cfg.sample_rate
        pcms.append(pcm)
    opt = vd.VadOptions()
    timings = {}
    got = pipeline.vad_batch(ctx, model, pcms, opt, timings=timings)
    assert all(len(timings[k]) == 1 for k in ('vad_shift', 'vad_viterbi', 'vad_backtrack'))
    tokens, last_frames = eg.decode_batch(ctx, model, pcms)
    assert last_frames == [len(p) // model.cfg.hop for p in pcms]
    # the scores decode_batch left (shifted in place), against the batch shift of the per-file scores
    files = [eg.device_scores(ctx, model, p) for p in pcms]
    assert [len(f) for f in files] == last_frames
    assert model.n_states == 2
    shifted, off = _run_shift(ctx, files, in_place=True)
    left = np.empty_like(shifted)
    ctx.d2h(left, ctx.dev_scratch('vad_scores', 0))
    assert np.array_equal(left.view(np.uint32), shifted.view(np.uint32))
    stay, exit_, enter = model.decoder_constants()
    want = []
    for i, last in enumerate(last_frames):
        hf, hw, _ = hipabi.vad_viterbi(shifted[off[i]:off[i + 1]], model.word_state, stay, exit_, enter)
        toks = [(int(t), model.words[w]) for t, w in zip(hf, hw)]
        assert tokens[i] == toks, i
        turns = vd.turns_from_tokens(((str(t), w) for t, w in toks), 'a', opt, lambda: str(last))
        times = hipabi.py2_roundtrip(np.array([(s, e) for _, s, e in turns], dtype=np.float64).ravel()).reshape(-1, 2)
        want.append([(float(s), float(e)) for s, e in times])
    print('turns per file:', [len(w) for w in want], 'tokens per file:', [len(t) for t in tokens])
    assert got == want and len(got) == 2
    assert any(len(t) > 1 for t in tokens)            # the decoder switched somewhere
    # ready for BatchFile, and without the text contract the raw sums
    assert all(pipeline.BatchFile(0, n, v).vad == v for n, v in zip(last_frames, got))
    raw = pipeline.vad_batch(ctx, model, pcms, opt, text_contract=False)
    assert [len(r) for r in raw] == [len(w) for w in want]
