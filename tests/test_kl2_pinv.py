"""KL2 with the reference's pseudo-inverse (SPKD_KL2_PINV, HipEngine(kl2_pinv=True),
--kl2-pinv): covariances that are not positive definite -- digital silence, sets shorter
than 40 frames, zeroed stretches -- give the reference's finite distances instead of the
default mode's NaN.  The CPU oracles' 'KL2' already is the reference's pinv KL2, so they
check the device mode; kl2_pinv_cases.json holds the reference's own outputs.

Scores are compared to 1e-5 relative, the project's KL2 bar (the device
rounds fp64 means to float32 where np.mean accumulates in float32, a few 1e-6 on ordinary
pairs in either mode); merge sequences and recipes must be identical."""
import io
import json
import math
import os

import numpy as np
import pytest

from helpers import ROOT, session, assert_stdout_close, cli, synth
from conftest import pkg

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
with open(os.path.join(GOLDEN, 'kl2_pinv_cases.json')) as _f:
    PCASES = json.load(_f)['cases']

_EDITED = {}
KL2_REL = 1e-5


def edited_session(meta):
    """The frames of a kl2_pinv_cases.json session: synth.make_session, then the zeroed ranges."""
    key = json.dumps(meta, sort_keys=True)
    if key not in _EDITED:
        feats, _, truth = session(meta)
        f = feats.copy()
        for b, e in meta['edits']['zero']:
            f[b:e] = 0.0
        assert synth.fea_sha256(f) == meta['edited_sha256']
        _EDITED[key] = (f, truth)
    return _EDITED[key]


def run_pcase(case, tmp, engine, extra=()):
    tmp = str(tmp)
    feats, _ = edited_session(case['session'])
    feadir = os.path.join(tmp, 'fea')
    os.makedirs(feadir, exist_ok=True)
    fea = os.path.join(feadir, os.path.splitext(case['audio'])[0] + '.fea')
    if not os.path.exists(fea):
        synth.write_fea(fea, feats)
    rin = os.path.join(tmp, case['name'] + '.in.recipe')
    rout = os.path.join(tmp, case['name'] + '.out.recipe')
    with open(rin, 'w') as f:
        f.write(case['input_recipe'])
    argv = [rin, feadir + '/', '-o', rout] + list(case['argv_tail']) + list(extra)
    buf = io.StringIO()
    if case['script'] == 'spk-change-detection.py':
        cli.main_change_detection(argv, engine=engine, stdout=buf)
    else:
        cli.main_clustering(argv, variant=2 if case['script'].endswith('2.py') else 1,
                            engine=engine, stdout=buf)
    return buf.getvalue().replace(tmp, '<TMP>'), open(rout).read()


def _rel(a, b):
    return abs(a - b) / max(1.0, abs(a), abs(b))


# ---------------------------------------------------------------- no GPU needed
def test_header_declares_the_mode():
    with open(os.path.join(ROOT, 'include', 'spkd.h')) as f:
        h = f.read()
    assert 'SPKD_KL2_PINV = 3' in h
    assert '#define SPKD_WANT_KL2_PINV 4' in h


def test_hipabi_kind_and_flag():
    hipabi = pkg('hipabi')
    assert hipabi.KINDS['KL2P'] == 3
    assert hipabi.WANT_KL2_PINV == 4
    assert hipabi.KINDS['KL2'] == 2


def test_cli_parsers_take_the_long_option():
    for p in (cli.build_cd_parser(), cli.build_cl_parser(1), cli.build_cl_parser(2)):
        assert p.parse_args(['r', 'f', '--kl2-pinv']).kl2_pinv is True
        assert p.parse_args(['r', 'f']).kl2_pinv is False


def test_cli_refuses_an_engine_without_the_mode(tmp_path):
    from oracle.numpy_engine import NumpyEngine
    case = PCASES[0]
    with pytest.raises(ValueError, match='kl2-pinv'):
        run_pcase(case, tmp_path, NumpyEngine(), extra=['--kl2-pinv'])


@pytest.mark.parametrize('case', PCASES, ids=[c['name'] for c in PCASES])
def test_numpy_oracle_reproduces_reference(case, tmp_path):
    from oracle.numpy_engine import NumpyEngine
    assert case['status'] == 'ok'
    stdout, recipe = run_pcase(case, tmp_path, NumpyEngine())
    assert recipe == case['output_recipe']
    assert_stdout_close(stdout, case['stdout'], rel=1e-5)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope='module')
def peng():
    e = pkg('engine').HipEngine(0, kl2_pinv=True)
    yield e
    e.close()


@pytest.fixture(scope='module')
def deng():
    e = pkg('engine').HipEngine(0)
    yield e
    e.close()


@pytest.fixture(scope='module')
def coracle():
    from oracle.c_engine import COracleEngine
    return COracleEngine()


@pytest.mark.gpu
def test_pair_terms_pinv_matches_reference_function_values(peng):
    """Every pair of functions.json, the 30-frame pair (reference 343.811) included."""
    assert peng.kl2_pinv
    g = json.load(open(os.path.join(GOLDEN, 'functions.json')))
    feats, _, _ = session(g['session'])
    peng.set_features(feats)
    short = 0
    for p in g['pairs']:
        t = peng.pair_terms([([tuple(p['a'])], [tuple(p['b'])])], want_kl2=True)[0]
        want = float.fromhex(p['kl2'])
        assert math.isfinite(t.kl2) and _rel(t.kl2, want) < KL2_REL, (p['a'], p['b'], t.kl2, want)
        short += min(p['a'][1] - p['a'][0], p['b'][1] - p['b'][0]) < 40
    assert short


@pytest.mark.gpu
def test_pair_terms_flags_exclude_each_other(peng):
    hipabi = pkg('hipabi')
    g = json.load(open(os.path.join(GOLDEN, 'functions.json')))
    feats, _, _ = session(g['session'])
    peng.set_features(feats)
    slots = peng._record_slots([[tuple(g['pairs'][0]['a'])], [tuple(g['pairs'][0]['b'])]])
    with pytest.raises(hipabi.SpkdError):
        peng.ctx.pair_terms(peng._rec_buf, slots[:1], slots[1:], hipabi.WANT_KL2 | hipabi.WANT_KL2_PINV)


def _degenerate_problem():
    """The first 20 speaker turns of a session, two of them digital silence and two cut below
    40 frames: every KL2 entry point meets all-zero and rank-deficient covariances."""
    feats, _, truth = synth.make_session(4242, 600, 4)
    segs = [(a, b) for a, b, _ in truth][:20]
    f = feats.copy()
    for z in (3, 11):
        f[segs[z][0]:segs[z][1]] = 0.0
    segs[6] = (segs[6][0], segs[6][0] + 30)
    segs[15] = (segs[15][0], segs[15][0] + 25)
    return f, segs


def _same_merges(got, want, rel):
    assert len(got.merges) == len(want.merges), (got.merges, want.merges)
    for (a, b, d), (a2, b2, d2) in zip(got.merges, want.merges):
        assert (a, b) == (a2, b2)
        assert _rel(d, d2) < rel, (d, d2)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [1, 2])
@pytest.mark.parametrize('max_spk', [0, 3])
def test_cluster_hi_degenerate_matches_oracle(peng, coracle, variant, max_spk):
    f, segs = _degenerate_problem()
    peng.set_features(f)
    coracle.set_features(f)
    got = peng.cluster_hi(segs, variant, 'KL2', 1.3, 12.0, max_spk)
    want = coracle.cluster_hi(segs, variant, 'KL2', 1.3, 12.0, max_spk)
    assert want.merges and all(math.isfinite(d) for _, _, d in want.merges)
    _same_merges(got, want, KL2_REL)
    for x, y in ((got.max_dist, want.max_dist), (got.min_dist, want.min_dist)):
        assert x == y or _rel(x, y) < KL2_REL, (x, y)


@pytest.mark.gpu
@pytest.mark.parametrize('path', ['MONO', 'WIDE'])
def test_cluster_hi_both_launch_shapes(peng, coracle, path):
    hipabi = pkg('hipabi')
    f, segs = _degenerate_problem()
    peng.set_features(f)
    coracle.set_features(f)
    old = peng.ahc_path
    peng.ahc_path = getattr(hipabi, 'AHC_' + path)
    try:
        got = peng.cluster_hi(segs, 1, 'KL2', 1.3, 12.0, 3)
    finally:
        peng.ahc_path = old
    _same_merges(got, coracle.cluster_hi(segs, 1, 'KL2', 1.3, 12.0, 3), KL2_REL)


@pytest.mark.gpu
def test_cluster_in_degenerate_matches_reference_case(peng, tmp_path):
    case = [c for c in PCASES if c['name'] == 'P_cl1_in_kl2'][0]
    stdout, recipe = run_pcase(case, tmp_path, peng, extra=['--kl2-pinv'])
    assert recipe == case['output_recipe']
    assert_stdout_close(stdout, case['stdout'], rel=KL2_REL)


@pytest.mark.gpu
def test_gw_and_sw_degenerate_match_oracle(peng, deng, coracle):
    """A digital-silence turn (against the C oracle) and a speech turn (against the default
    KL2: the fast path) through spkd_sw and spkd_gw.  (Windows that
    straddle a silence edge are covered against the reference itself by the P_cd_sw_kl2 /
    P_cd_gw_kl2 cases: there the sufficient-statistics covariance of the oracle and of the
    device can carry rounding-noise eigenvalues next to the cut-off, include/spkd.h.)"""
    f, segs = _degenerate_problem()
    for e in (peng, deng, coracle):
        e.set_features(f)
    turns = [segs[3], (segs[0][0], segs[2][1])]
    got = peng.sw(turns, 'KL2', 1.3, 250.0, 31.0)
    want = coracle.sw(turns, 'KL2', 1.3, 250.0, 31.0)
    want[1] = deng.sw(turns[1:], 'KL2', 1.3, 250.0, 31.0)[0]
    assert [len(x) for x in got] == [len(x) for x in want] and len(want[0]) > 10
    assert all(float(x) == 0.0 for x in got[0])             # silence against silence
    for g, w in zip(got, want):
        for x, y in zip(g, w):
            assert math.isfinite(y) and _rel(float(x), float(y)) < 1e-9, (x, y)
    g1 = peng.gw(turns, 'KL2', 1.3, 60.0, 125.0, 375.0, 12.0, 125.0, trace=True)
    g2 = coracle.gw(turns[:1], 'KL2', 1.3, 60.0, 125.0, 375.0, 12.0, 125.0, trace=True)
    g2 += deng.gw(turns[1:], 'KL2', 1.3, 60.0, 125.0, 375.0, 12.0, 125.0, trace=True)
    for r1, r2 in zip(g1, g2):
        assert len(r1.events) == len(r2.events) and r1.final_start == r2.final_start
        for e1, e2 in zip(r1.events, r2.events):
            assert e1[0] == e2[0]
            for x, y in zip(e1[1:], e2[1:]):
                if isinstance(y, float) and isinstance(x, float) and x != y:
                    assert _rel(x, y) < KL2_REL, (e1, e2)
                else:
                    assert x == y, (e1, e2)


def _kl2_matrix(eng, kind, segs):
    n = len(segs)
    d_stats = eng._stats_of_sets([[s] for s in segs])
    d_mat = eng.ctx.dev_alloc(n * n * 8)
    try:
        eng.ctx.distance_matrix(kind, 1.3, d_stats, n, d_mat)
        m = np.empty((n, n), dtype=np.float64)
        eng.ctx.d2h(m, d_mat)
    finally:
        eng.ctx.dev_free(d_mat)
        eng.ctx.dev_free(d_stats)
    return m


@pytest.mark.gpu
def test_distance_matrix_wrapper_takes_kl2p(peng, coracle):
    """Pairs with a degenerate record against the C oracle; the others are the default
    KL2's values (the fast path)."""
    f, segs = _degenerate_problem()
    peng.set_features(f)
    coracle.set_features(f)
    m = _kl2_matrix(peng, 'KL2P', segs)
    m0 = _kl2_matrix(peng, 'KL2', segs)
    degenerate = {3, 6, 11, 15}
    n = len(segs)
    for i in range(n):
        for j in range(i + 1, n):
            assert math.isfinite(m[i, j]), (i, j)
            if i in degenerate or j in degenerate:
                assert math.isnan(m0[i, j])
                want = coracle.pair_terms([([segs[i]], [segs[j]])], want_kl2=True)[0].kl2
                assert _rel(m[i, j], want) < KL2_REL, (i, j, m[i, j], want)
            else:
                assert _rel(m[i, j], m0[i, j]) < 1e-9, (i, j, m[i, j], m0[i, j])


@pytest.mark.gpu
@pytest.mark.parametrize('case', PCASES, ids=[c['name'] for c in PCASES])
def test_hip_cli_kl2_pinv_matches_reference(case, tmp_path, peng):
    stdout, recipe = run_pcase(case, tmp_path, peng, extra=['--kl2-pinv'])
    assert recipe == case['output_recipe']
    assert_stdout_close(stdout, case['stdout'], rel=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['A_cl1_hi_kl2', 'A_cd_gw_kl2'])
def test_well_conditioned_inputs_take_the_fast_path(name, tmp_path, peng, deng):
    """Every covariance positive definite and well conditioned: KL2P is the default KL2."""
    from helpers import load_cases, run_case
    case = [c for c in load_cases() if c['name'] == name][0]
    s1, o1, r1, _ = run_case(case, tmp_path / 'p', peng)
    s2, o2, r2, _ = run_case(case, tmp_path / 'd', deng)
    assert s1 == s2 == 'ok'
    assert r1 == r2
    assert_stdout_close(o1, o2, rel=1e-9)


@pytest.mark.gpu
def test_pinv_mode_is_reproducible(peng):
    f, segs = _degenerate_problem()
    peng.set_features(f)
    r1 = peng.cluster_hi(segs, 1, 'KL2', 1.3, 12.0, 3)
    r2 = peng.cluster_hi(segs, 1, 'KL2', 1.3, 12.0, 3)
    assert [(a, b, d.hex()) for a, b, d in r1.merges] == [(a, b, d.hex()) for a, b, d in r2.merges]
    jobs = [([segs[i]], [segs[j]]) for i in range(len(segs)) for j in range(i + 1, len(segs))]
    t1 = peng.pair_terms(jobs, want_kl2=True)
    t2 = peng.pair_terms(jobs, want_kl2=True)
    assert [t.kl2.hex() for t in t1] == [t.kl2.hex() for t in t2]
