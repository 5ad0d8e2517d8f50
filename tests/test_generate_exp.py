"""The generate_exp.py stand-in (exp_generator.py): model readers, the .lna post-processing the
reference's own code pins (tests/golden/generate_exp_cases.json), the exact Viterbi against the
numpy restatement (tests/vad_numpy.py), the command line, and -- on the GPU -- the 256-sample
front-end, the frame scoring kernel and the stage end to end.  The reference's model files are
not stored: synthetic models of the same structure (tests/golden/vad_model.json) are written
in the same text formats."""
import json
import math
import os
import stat
import struct
import subprocess
import sys
import wave

import numpy as np
import pytest

import vad_numpy as vn
from conftest import pkg
from helpers import ROOT
from mfcc_compare import full_chain_bound, full_chain_ratios
from test_frontend import GOLD as FEA_GOLD, _cfg_text

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
VAD_GOLD = json.load(open(os.path.join(GOLDEN, 'vad_model.json')))
MODEL = os.path.join('hmms', 'mfcc_16g_11.10.2007_10')      # the name generate_exp.py defaults to


def _synthetic_mixtures(rng, n_kernels=48, dim=39):
    """Two states of 24 kernels (as the reference's model), plus a kernel each borrows from the
    other, a weight of 0 and a tiny weight; state 0's means around -1, state 1's around +1."""
    means = rng.standard_normal((n_kernels, dim)) * 0.5
    means[:24] -= 1.0
    means[24:] += 1.0
    variances = 0.3 + rng.random((n_kernels, dim))
    mix = []
    for s, ks in enumerate((list(range(24)) + [30], list(range(24, 48)) + [5])):
        w = rng.random(len(ks)) + 0.1
        w[3] = 0.0
        w[7] = 2.11808e-24
        mix.append((np.array(ks), w / w.sum()))
    return means, variances, mix


def _binlm(words, log10p, order=1):
    head = 'cis-binlm2\nbackoff\n%d\n%s\n%d %d\n%s\n' % (len(words), '\n'.join(words), order, len(words),
                                                        '\n'.join([str(len(words))] * order))
    return head.encode() + b''.join(struct.pack('<iffi', i, p, 0.0, -1) for i, p in enumerate(log10p))


def write_model(d, means, variances, mix, stay=(0.993663, 0.999217), exit_=(0.00633736, 0.001),
                words=('<UNK>', 'p', '<w>'), log10p=(-99.0, -1.0, -1.0), window=256, cov='diagonal_cov'):
    """MODEL.{gk,mc,ph,cfg} under d/hmms and the lexicon / LM under d/vad_models."""
    os.makedirs(os.path.join(d, 'hmms'), exist_ok=True)
    os.makedirs(os.path.join(d, 'vad_models'), exist_ok=True)
    m = os.path.join(d, MODEL)
    K, D = means.shape
    with open(m + '.gk', 'w') as f:
        f.write('%d %d %s\n' % (K, D, cov))
        for k in range(K):
            f.write(' '.join(repr(float(v)) for v in np.concatenate([means[k], variances[k]])) + '\n')
    with open(m + '.mc', 'w') as f:
        f.write('%d\n' % len(mix))
        for ks, ws in mix:
            f.write('%d %s\n' % (len(ks), ' '.join('%d %r' % (k, float(w)) for k, w in zip(ks, ws))))
    with open(m + '.ph', 'w') as f:
        f.write('PHONE\n2\n')
        for i, (lab, st) in enumerate((('__', 0), ('p', 1))):
            f.write('%d 3 %s\n-1 -2 %d\n0 1 2 1\n1 0\n2 2 2 %r 1 %r\n' % (i + 1, lab, st, stay[i], exit_[i]))
    with open(m + '.cfg', 'w') as f:
        f.write(_cfg_text(FEA_GOLD).replace('window_width 400', 'window_width %d' % window))
    with open(os.path.join(d, 'vad_models', 'sp_nsp.lex'), 'w') as f:
        f.write('<w>(1.0) __\np(1.0) p\n')
    with open(os.path.join(d, 'vad_models', 'malli.bin'), 'wb') as f:
        f.write(_binlm(words, log10p))
    return m


def load_model(d):
    old = os.getcwd()
    os.chdir(d)
    try:
        return pkg('vad_model').VadModel.load(MODEL)
    finally:
        os.chdir(old)


@pytest.fixture()
def model_dir(tmp_path):
    rng = np.random.default_rng(11)
    means, variances, mix = _synthetic_mixtures(rng)
    write_model(str(tmp_path), means, variances, mix)
    return str(tmp_path), means, variances, mix


# ---------------------------------------------------------------------------- readers
def test_readers_parse_a_synthetic_model_in_all_five_formats(model_dir):
    d, means, variances, mix = model_dir
    m = load_model(d)
    assert (m.n_kernels, m.dim, m.n_states) == (48, 39, 2)
    assert np.array_equal(m.means, means) and np.array_equal(m.variances, variances)
    for (ks, ws), (gk, gw) in zip(m.mixtures, mix):
        assert np.array_equal(ks, gk) and np.array_equal(ws, gw)
    assert 30 in m.mixtures[0][0] and 5 in m.mixtures[1][0]                 # shared kernels
    assert m.words == ['<w>', 'p'] and m.word_state == [0, 1]
    assert m.a_stay == [0.993663, 0.999217] and m.a_exit == [0.00633736, 0.001]
    assert m.log10p == [-1.0, -1.0] and m.cfg.window_width == 256
    g = m.gmm_arrays()
    assert list(g['state_off']) == [0, 25, 50] and g['kernel'][24] == 30 and g['kernel'][49] == 5
    assert g['log_weight'][3] == -np.inf and g['log_weight'][28] == -np.inf
    assert 0 < mix[0][1][7] < 1e-23 and g['log_weight'][7] == np.float32(math.log(mix[0][1][7]))
    want_c = -0.5 * (39 * math.log(2 * math.pi) + np.log(variances).sum(axis=1))
    assert np.array_equal(g['log_norm'], want_c.astype(np.float32))
    assert np.array_equal(g['inv_var'], (1.0 / variances).astype(np.float32))
    stay, exit_, enter = m.decoder_constants()
    for a, b in zip((stay, exit_, enter), vn.decoder_constants(m.a_stay, m.a_exit, m.log10p)):
        assert np.array_equal(a, b)
    assert enter[0] == 10 * math.log(10.0) * -1.0 - 1.0


def test_readers_refuse_what_the_decoder_does_not_model(model_dir):
    d, means, variances, mix = model_dir
    vm = pkg('vad_model')
    m = os.path.join(d, MODEL)
    gk = open(m + '.gk').read()
    for kind in ('single_cov', 'full_cov', 'pcgmm', 'scgmm'):
        with open(m + '.gk', 'w') as f:
            f.write(gk.replace('diagonal_cov', kind, 1))
        with pytest.raises(ValueError, match=kind):
            vm.read_gk(m + '.gk')
    with open(m + '.gk', 'w') as f:
        f.write(gk)
    ph = open(m + '.ph').read()
    three = ph.replace('2 3 p\n-1 -2 1\n0 1 2 1\n1 0\n2 2 2 0.999217 1 0.001\n',
                       '2 4 p\n-1 -2 1 0\n0 1 2 1\n1 0\n2 2 2 0.5 3 0.5\n3 2 3 0.9 1 0.1\n')
    assert three != ph
    with open(m + '.ph', 'w') as f:
        f.write(three)
    with pytest.raises(ValueError, match='one emitting state'):
        load_model(d)
    with open(m + '.ph', 'w') as f:
        f.write(ph.replace('2 2 2 0.999217 1 0.001', '2 1 1 1.0'))   # no self loop
    with pytest.raises(ValueError):
        load_model(d)
    with open(m + '.ph', 'w') as f:
        f.write(ph)
    lm = os.path.join(d, 'vad_models', 'malli.bin')
    with open(lm, 'wb') as f:
        f.write(_binlm(['<UNK>', 'p', '<w>'], [-99.0, -1.0, -1.0], order=2))
    with pytest.raises(ValueError, match='order 2'):
        vm.read_binlm(lm)
    with open(lm, 'wb') as f:
        f.write(_binlm(['<UNK>', 'p', '<w>'], [-99.0, -1.0, -1.0]))
    lex = os.path.join(d, 'vad_models', 'sp_nsp.lex')
    with open(lex, 'w') as f:
        f.write('<w>(1.0) __\np(1.0) p __\n')
    with pytest.raises(ValueError, match='one-phone words'):
        load_model(d)


def test_model_structure_matches_the_reference_fixture(tmp_path):
    """vad_model.json is what the readers make of the reference's files (make_golden_vad_model.py).
    A synthetic model written with that structure reads back to the same structural facts; where
    the reference tree is named (SPKD_REFERENCE) its own files must reproduce the fixture in full."""
    g = VAD_GOLD
    rng = np.random.default_rng(5)
    K, D = g['gk']['n_kernels'], g['gk']['dim']
    means = rng.standard_normal((K, D))
    variances = 0.5 + rng.random((K, D))
    mix = [(np.array(ks), np.full(len(ks), 1.0 / len(ks))) for ks in g['mc']['kernels']]
    write_model(str(tmp_path), means, variances, mix, window=g['cfg']['window_width'])
    got = vn.model_structure(load_model(str(tmp_path)))
    strip = lambda d: {k: strip(v) if isinstance(v, dict) else v for k, v in d.items() if 'sha256' not in k}
    want = strip({k: v for k, v in g.items() if k not in ('model', 'source')})
    want['mc']['zero_weights'] = [0] * len(want['mc']['kernels'])
    assert strip(got) == want
    ref = os.environ.get('SPKD_REFERENCE')
    if ref and os.path.isfile(os.path.join(ref, g['model'] + '.gk')):
        old = os.getcwd()
        os.chdir(ref)
        try:
            real = vn.model_structure(pkg('vad_model').VadModel.load(g['model']))
        finally:
            os.chdir(old)
        assert real == {k: v for k, v in g.items() if k not in ('model', 'source')}


def test_feature_configuration_accepts_the_vad_window():
    fc = pkg('feaconfig')
    cfg = fc.FeatureConfig(_cfg_text(FEA_GOLD).replace('window_width 400', 'window_width 256'))
    assert cfg.window_width == 256 and cfg.hop == 128
    assert fc.FeatureConfig(_cfg_text(FEA_GOLD)).window_width == 400


# ---------------------------------------------------------------------------- .lna and the shift
def _ulps_apart(a, b):
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def test_lna_shift_reproduces_the_reference_bytes(tmp_path):
    eg = pkg('exp_generator')
    cases = json.load(open(os.path.join(GOLDEN, 'generate_exp_cases.json')))['cases']
    assert {c['frames'] for c in cases} >= {0, 1, 7, 10}
    for c in cases:
        raw = bytes.fromhex(c['lna_in'])
        T = c['frames']
        # the scores as phone_probs would leave them, written by the stand-in's writer
        scores = np.frombuffer(raw[5:], dtype='<f4').reshape(T, 2)
        lna = os.path.join(str(tmp_path), c['name'] + '.lna')
        eg.write_scores_lna(lna, scores)
        assert open(lna, 'rb').read() == raw, c['name']
        eg.shift_dec_bord(lna, str(tmp_path))
        got = open(lna, 'rb').read()
        want = bytes.fromhex(c['lna_out'])
        assert got[:5] == want[:5] and len(got) == len(want), c['name']
        a = np.frombuffer(got[5:], dtype='<f4')
        b = np.frombuffer(want[5:], dtype='<f4')
        assert np.array_equal(np.isnan(a), np.isnan(b)), c['name']
        fin = ~np.isnan(a)
        assert np.array_equal(np.isinf(a[fin]), np.isinf(b[fin])) and np.all(_ulps_apart(a[fin], b[fin]) <= 1), c['name']
        assert open(os.path.join(str(tmp_path), c['name'] + '.last_frame')).read() == c['last_frame']
        assert eg.lna_scores(lna).shape == (T, 2)


# ---------------------------------------------------------------------------- decoder
CONSTS = vn.decoder_constants([0.993663, 0.999217], [0.00633736, 0.001], [-1.0, -1.0])


def _both(scores, consts=CONSTS, word_state=(0, 1)):
    hipabi = pkg('hipabi')
    f, w, s = hipabi.vad_viterbi(scores, list(word_state), *consts)
    rf, rw, rs = vn.viterbi(scores, list(word_state), *consts)
    assert list(f) == rf and list(w) == rw
    assert s == rs or (math.isnan(s) and math.isnan(rs)), (s, rs)
    return rf, rw, rs


def test_viterbi_equals_the_restatement_exactly():
    rng = np.random.default_rng(17)
    for T in (1, 2, 3, 50, 777):
        for scale in (0.5, 5.0, 40.0):
            _both((-3.0 + scale * rng.standard_normal((T, 2))).astype(np.float32))
    # three words over three states, random constants
    for _ in range(5):
        sc = rng.standard_normal((200, 3)).astype(np.float32) * 4
        consts = tuple(rng.standard_normal(3) * 3 for _ in range(3))
        _both(sc, consts, (2, 0, 1))
    # ties everywhere: equal scores and symmetric constants
    _both(np.zeros((40, 2), np.float32), (np.zeros(2), np.zeros(2), np.zeros(2)))
    _both(np.ones((40, 2), np.float32), (np.array([-1.0, -1.0]), np.array([-1.0, -1.0]), np.array([-1.0, -1.0])))
    f, w, _ = _both(np.zeros((5, 2), np.float32), (np.zeros(2), np.zeros(2), np.zeros(2)))
    assert (f, w) == ([0], [0])                   # stay beats switch, the lowest word wins
    # NaN scores, all -inf frames, -inf mixed in
    sc = (-2.0 + rng.standard_normal((300, 2))).astype(np.float32)
    sc[10] = np.nan
    sc[11, 0] = np.nan
    sc[50:55] = -np.inf
    sc[80, 1] = -np.inf
    sc[120:130, 0] = -np.inf
    _both(sc)
    _both(np.full((4, 2), -np.inf, np.float32))
    _both(np.full((4, 2), np.nan, np.float32))
    assert _both(np.zeros((0, 2), np.float32)) == ([], [], -math.inf)


def test_viterbi_finds_planted_speech():
    """Scores that strongly favour p inside known ranges give exactly those start frames."""
    T = 1000
    sc = np.zeros((T, 2), np.float32)
    sc[:, 0], sc[:, 1] = -1.0, -60.0
    for a, b in ((100, 250), (400, 401 + 300), (900, 1000)):
        sc[a:b, 0], sc[a:b, 1] = -60.0, -1.0
    f, w, _ = _both(sc)
    names = ['<w>', 'p']
    assert vn.exp_text(f, w, names) == '0 <w> 100 p 250 <w> 400 p 701 <w> 900 p'


def test_viterbi_refuses_bad_arguments():
    hipabi = pkg('hipabi')
    with pytest.raises(hipabi.SpkdError):
        hipabi.vad_viterbi(np.zeros((3, 2), np.float32), [0, 2], *CONSTS)
    with pytest.raises(hipabi.SpkdError):
        hipabi.vad_viterbi(np.zeros((3, 2), np.float32), [0, 1], CONSTS[0][:1], CONSTS[1], CONSTS[2])


# ---------------------------------------------------------------------------- command line
def test_command_line_refusals_and_messages(tmp_path, monkeypatch):
    eg = pkg('exp_generator')
    out = []
    say = lambda *a: out.append(' '.join(str(x) for x in a))
    d = str(tmp_path)
    missing = os.path.join(d, 'none.recipe')
    assert eg.main([missing], say=say) == 0 and out == ['ERROR: %s does not exist.' % missing]
    recipe = os.path.join(d, 'r.recipe')
    with open(recipe, 'w') as f:
        f.write('audio=%s/a.wav\n' % d)
    del out[:]
    lna = os.path.join(d, 'lna')
    assert eg.main([recipe, '-l', lna], say=say, ask=lambda q: 'n') == 0
    assert out == ['ERROR: %s is not a valid directory.' % lna, 'Unable to continue without valid %s' % lna]
    del out[:]
    asked = []
    exp = os.path.join(d, 'exp')
    model = os.path.join(d, 'nomodel')
    assert eg.main([recipe, '-l', lna, '-e', exp, '-m', model], say=say,
                   ask=lambda q: asked.append(q) or 'y') == 0
    assert asked == ['Attempt to create? [y/N]: '] * 2 and os.path.isdir(lna) and os.path.isdir(exp)
    assert out == ['ERROR: %s is not a valid directory.' % lna, 'ERROR: %s is not a valid directory.' % exp,
                   'ERROR: %s does not exist.' % model]
    # -a and -t are accepted and not used; the progress lines
    calls = []
    monkeypatch.setattr(eg, 'run', lambda *a: calls.append(a))
    open(model + '.cfg', 'w').close()
    del out[:]
    assert eg.main([recipe, '-l', lna, '-e', exp, '-m', model, '-a', '/nowhere', '-t', '/nowhere/tp'], say=say) == 0
    assert calls == [(recipe, lna, exp, model)]
    assert out == ['Reading recipe: %s' % recipe, 'Using model: %s' % model, 'Writing `.lna` files in: %s' % lna,
                   'Writing `.exp` files in: %s' % exp]
    # a recipe line without audio= fails the way get_lnas does
    with open(recipe, 'w') as f:
        f.write('file=x.wav\n')
    with pytest.raises(AttributeError):
        eg.get_lnas(recipe, lna)
    # the executable shim and its defaults
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'generate_exp.py'), '--help'], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and 'RECIPE' in r.stdout and '--tokenpass' in r.stdout and '--asrpath' in r.stdout
    assert os.stat(os.path.join(ROOT, 'generate_exp.py')).st_mode & stat.S_IXUSR


# ---------------------------------------------------------------------------- GPU
def _tol(ref):
    return 1e-3 + 1e-5 * np.abs(ref)


def _close(got, ref):
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(got == -np.inf, ref == -np.inf)
    fin = np.isfinite(ref)
    err = np.abs(got[fin] - ref[fin])
    assert np.all(err <= _tol(ref[fin])), float(np.max(err - _tol(ref[fin])))


def _device_gmm(feats, gmm):
    hipabi = pkg('hipabi')
    ctx = hipabi.Context(0)
    try:
        feats = np.ascontiguousarray(feats, np.float32)
        S = len(gmm['state_off']) - 1
        out = np.zeros((len(feats), S), np.float32)
        d_x = ctx.dev_alloc(max(feats.nbytes, 16))
        d_o = ctx.dev_alloc(max(out.nbytes, 16))
        try:
            ctx.h2d(d_x, feats)
            ctx.gmm_loglik(d_x, len(feats), gmm, d_o)
            ctx.d2h(out, d_o)
        finally:
            ctx.dev_free(d_x)
            ctx.dev_free(d_o)
        return out
    finally:
        ctx.close()


def _sample(rng, means, variances, ks, ws, n):
    pick = rng.choice(ks, size=n, p=ws / ws.sum())
    return means[pick] + np.sqrt(variances[pick]) * rng.standard_normal((n, means.shape[1]))


def _signal(seconds, seed, rate=16000):
    """Speech-like bursts (harmonic tones) over low noise, bursts at 1.0-2.5 s and 4.0-6.0 s."""
    rng = np.random.default_rng(seed)
    t = np.arange(int(seconds * rate)) / rate
    on = ((t > 1.0) & (t < 2.5)) | ((t > 4.0) & (t < 6.0))
    x = 200 * rng.standard_normal(len(t)) + on * sum(2000 / h * np.sin(2 * np.pi * 150 * h * t) for h in range(1, 8))
    return np.clip(x, -32768, 32767).astype(np.int16)


def _write_wav(path, pcm):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm.tobytes())


@pytest.mark.gpu
def test_hip_front_end_does_256_sample_windows():
    from oracle import mfcc_numpy as m
    fe = pkg('frontend')
    cfg = pkg('feaconfig').FeatureConfig(_cfg_text(FEA_GOLD).replace('window_width 400', 'window_width 256'))
    for seconds, seed in ((4.0, 3), (0.9, 5), (21.3, 7)):
        pcm = _signal(seconds, seed)
        want = m.features(pcm, cfg)
        got = fe.extract(pcm, cfg)
        assert got.shape == want.shape and np.all(np.isfinite(got))
        # test_mfcc_reference's bound on this signal (never above the former 2e-3 of the feature scale)
        r = full_chain_ratios(got, pcm, cfg)
        print('%.1f s: device error / bound at most %.3f (column %d)' % (seconds, r.max(), r.argmax()))
        assert np.all(r <= 1.0), (seconds, int(r.argmax()), float(r.max()))
        assert full_chain_bound(pcm, cfg).max() < 2e-3 * max(1.0, float(np.abs(want).max()))


@pytest.mark.gpu
def test_hip_gmm_scores_match_the_restatement(model_dir):
    d, means, variances, mix = model_dir
    m = load_model(d)
    gmm = m.gmm_arrays()
    rng = np.random.default_rng(23)
    # frames sampled from the model's mixtures (and a few far outliers), odd count for a partial tile
    x = np.concatenate([_sample(rng, means, variances, *mix[0], 700), _sample(rng, means, variances, *mix[1], 611),
                        6.0 * rng.standard_normal((20, 39))]).astype(np.float32)
    _close(_device_gmm(x, gmm), vn.gmm_loglik(x, means, variances, mix))
    # front-end frames of the 256-sample configuration
    fe = pkg('frontend')
    feats = fe.extract(_signal(7.0, 9), m.cfg)
    _close(_device_gmm(feats, gmm), vn.gmm_loglik(feats, means, variances, mix))
    # several files in one launch give what they give one by one
    files = [fe.extract(_signal(s, 30 + i), m.cfg) for i, s in enumerate((0.5, 3.3, 1.0, 2.1))]
    batch = _device_gmm(np.concatenate(files), gmm)
    assert np.array_equal(batch, np.concatenate([_device_gmm(f, gmm) for f in files]))
    _close(batch, vn.gmm_loglik(np.concatenate(files), means, variances, mix))
    # a state whose weights are all 0 scores -inf; non-finite features propagate
    zmix = [mix[0], (mix[1][0], np.zeros(len(mix[1][1])))]
    zg = dict(gmm, log_weight=np.concatenate([gmm['log_weight'][:25], np.full(25, -np.inf, np.float32)]))
    xz = x[:300].copy()
    xz[5, 3] = np.nan
    xz[6, 0] = np.inf
    got = _device_gmm(xz, zg)
    ref = vn.gmm_loglik(xz, means, variances, zmix)
    assert np.all(got[:, 1] == -np.inf) and np.isnan(got[5, 0])
    _close(got, ref)


@pytest.mark.gpu
def test_planted_boundaries_through_scoring_and_decoding(model_dir):
    d, means, variances, mix = model_dir
    m = load_model(d)
    rng = np.random.default_rng(29)
    bounds = [0, 400, 1100, 1500, 2300, 2600]          # mixture 0 / 1 alternating, starting with 0
    x = np.concatenate([_sample(rng, means, variances, *mix[i % 2], b - a)
                        for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:]))]).astype(np.float32)
    scores = _device_gmm(x, m.gmm_arrays())
    f, w, _ = pkg('hipabi').vad_viterbi(scores, m.word_state, *m.decoder_constants())
    assert [m.words[i] for i in w] == ['<w>', 'p'] * 2 + ['<w>']
    assert all(abs(int(a) - b) <= 2 for a, b in zip(f, bounds[:-1])), list(f)


@pytest.mark.gpu
def test_generate_exp_and_the_whole_pipeline_as_child_processes(model_dir):
    """./generate_exp.py in a scratch working directory with a synthetic wav and model; its .lna,
    .last_frame and .exp agree with the stages restated on the device's own intermediates; then
    ./spk-diarization2.py runs all seven stages from this repository."""
    d, means, variances, mix = model_dir
    eg = pkg('exp_generator')
    for name in ('generate_exp.py', 'feacat', 'voice-detection2.py', 'spk-change-detection.py', 'spk-clustering.py',
                 'aku2ann.py', 'aku2elan.py', 'spk-diarization2.py'):
        os.symlink(os.path.join(ROOT, name), os.path.join(d, name))
    for sub in ('lna', 'exp', 'fea'):
        os.makedirs(os.path.join(d, sub))
    with open(os.path.join(d, 'fconfig.cfg'), 'w') as f:
        f.write(_cfg_text(FEA_GOLD))
    pcm = _signal(9.0, 41)
    _write_wav(os.path.join(d, 'talk.wav'), pcm)
    with open(os.path.join(d, 'talk.recipe'), 'w') as f:
        f.write('audio=talk.wav\n')
    r = subprocess.run(['./generate_exp.py', 'talk.recipe', '-m', MODEL], cwd=d, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    assert 'Reading recipe: talk.recipe' in r.stdout
    # the restatement chain on the device's own intermediates
    m = load_model(d)
    feats = pkg('frontend').extract(pcm, m.cfg)
    T = len(feats)
    assert T == len(pcm) // 128
    scores = _device_gmm(feats, m.gmm_arrays())
    _close(scores, vn.gmm_loglik(feats, means, variances, mix))
    chk = os.path.join(d, 'check')
    os.makedirs(chk)
    eg.write_scores_lna(os.path.join(chk, 'talk.lna'), scores)
    eg.shift_dec_bord(os.path.join(chk, 'talk.lna'), chk)
    assert open(os.path.join(d, 'lna', 'talk.lna'), 'rb').read() == open(os.path.join(chk, 'talk.lna'), 'rb').read()
    assert open(os.path.join(d, 'exp', 'talk.last_frame')).read() == str(T)
    frames, words, _ = vn.viterbi(eg.lna_scores(os.path.join(chk, 'talk.lna')), m.word_state, *m.decoder_constants())
    exp = open(os.path.join(d, 'exp', 'talk.exp')).read()
    assert exp == vn.exp_text(frames, words, m.words) and exp.startswith('0 ')
    # the whole pipeline
    os.remove(os.path.join(d, 'exp', 'talk.exp'))
    r = subprocess.run(['./spk-diarization2.py', 'talk.wav', '-o', 'talk.out.recipe'], cwd=d, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.isfile(os.path.join(d, 'exp', 'talk.exp')), r.stdout + r.stderr
    assert open(os.path.join(d, 'exp', 'talk.exp')).read() == exp
    lines = [l for l in open(os.path.join(d, 'talk.out.recipe')).read().splitlines() if l.strip()]
    for line in lines:
        assert 'audio=' in line and 'start-time=' in line and 'end-time=' in line and 'speaker=' in line, line
        s = float(line.split('start-time=')[1].split()[0])
        e = float(line.split('end-time=')[1].split()[0])
        assert 0 <= s <= e <= 9.0 + 1e-6
