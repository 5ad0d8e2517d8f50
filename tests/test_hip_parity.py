"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through
the C ABI, against (a) the golden vectors produced by the reference scripts and
(b) the CPU oracle on the same seeded inputs.

Bars (BASELINE.json north_star): recipes byte-identical (integer boundaries,
labels), scores within 1e-5 relative (fp64); the tests assert tighter bounds."""
import json
import math
import os
import re

import numpy as np
import pytest

from helpers import ROOT, load_cases, run_case, session, assert_stdout_close
from conftest import pkg

pytestmark = pytest.mark.gpu

CASES = load_cases()
# reference modes not on the device yet (growing window with KL2)
NOT_YET = set()


@pytest.fixture(scope='module')
def eng():
    engine = pkg('engine')
    e = engine.HipEngine(0)
    yield e
    e.close()


def _rel(a, b):
    return abs(a - b) / max(1.0, abs(a), abs(b))


def test_stats_records_match_direct_sums(eng):
    feats, _, truth = session({'seed': 7001, 'seconds': 400, 'n_speakers': 4, 'kwargs': {},
                               'sha256': json.load(open(os.path.join(ROOT, 'tests/golden/functions.json')))['session']['sha256']})
    eng.set_features(feats)
    sets = [[(0, 50)], [(10, 11)], [(100, 5000)], [(truth[0][0], truth[0][1]), (truth[3][0], truth[3][1])],
            [(7, 7)], [(0, feats.shape[0])]]
    got = eng.stats(sets)
    for k, ranges in enumerate(sets):
        x = np.concatenate([feats[a:b] for a, b in ranges]).astype(np.float64)
        xa = np.concatenate([x, np.ones((x.shape[0], 1))], axis=1)
        m = xa.T @ xa
        want = np.concatenate([m[r, r:] for r in range(40)])
        assert got[k, 819] == x.shape[0]
        scale = np.maximum(1.0, np.abs(want))
        assert np.max(np.abs(got[k] - want) / scale) < 1e-12, k


def test_pair_terms_against_reference_functions(eng):
    g = json.load(open(os.path.join(ROOT, 'tests/golden/functions.json')))
    feats, _, _ = session(g['session'])
    eng.set_features(feats)
    cd = pkg('change_detection')
    jobs = [([tuple(p['a'])], [tuple(p['b'])]) for p in g['pairs']]
    terms = eng.pair_terms(jobs, want_glr=True, want_kl2=True)
    worst = 0.0
    for p, t in zip(g['pairs'], terms):
        n_small = min(p['a'][1] - p['a'][0], p['b'][1] - p['b'][0])
        want_bic = float.fromhex(p['cl_bic_l1.3'])
        want_glr = float.fromhex(p['glr'])
        want_kl2 = float.fromhex(p['kl2'])
        got_bic = cd.bic_from_terms(t, g['lambda'])
        got_glr = cd.glr_from_terms(t)
        if n_small < 40:
            # rank-deficient covariance: the reference's determinant is rounding noise
            # (pinned separately: test_rank_deficient_sets_are_defined_and_reproducible)
            continue
        assert _rel(got_bic, want_bic) < 1e-9, (p, got_bic, want_bic)
        assert _rel(got_glr, want_glr) < 1e-9, (p, got_glr, want_glr)
        assert _rel(t.kl2, want_kl2) < 1e-5, (p, t.kl2, want_kl2)
        worst = max(worst, _rel(got_bic, want_bic), _rel(got_glr, want_glr))
    print('worst BIC/GLR relative error vs reference: %.3g' % worst)


def test_degenerate_inputs_follow_reference(eng):
    g = json.load(open(os.path.join(ROOT, 'tests/golden/functions.json')))
    feats, _, truth = session(g['session'])
    cd = pkg('change_detection')
    zero = np.zeros((200, 39), dtype=np.float32)
    const = np.ones((150, 39), dtype=np.float32)
    speech = feats[truth[0][0]:truth[0][0] + 300]
    buf = np.concatenate([speech, zero, zero, const])
    eng.set_features(buf)
    rng = {'speech': (0, 300), 'zero': (300, 500), 'zero2': (500, 700), 'const': (700, 850)}
    cases = {'speech_zero': ('speech', 'zero'), 'zero_zero': ('zero', 'zero2'), 'const_zero': ('const', 'zero')}
    for rec in g['degenerate']:
        a, b = cases[rec['name']]
        t = eng.pair_terms([([rng[a]], [rng[b]])], want_glr=True)[0]
        for key, got in (('bic', cd.bic_from_terms(t, 1.3)), ('glr', cd.glr_from_terms(t))):
            w = float.fromhex(rec[key])
            assert (math.isnan(w) and math.isnan(got)) or got == w, (rec['name'], key, got, w)
    # a one-frame set has a NaN covariance: the reference dies with ValueError
    with pytest.raises(ValueError):
        eng.pair_terms([([(0, 1)], [(0, 300)])])


def _same_bits(a, b):
    return (a == b) or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def test_rank_deficient_sets_are_defined_and_reproducible(eng):
    """A set with fewer than 40 frames has a rank-deficient covariance: the
    reference's LU determinant is rounding noise there (NaN for the 30-frame golden pair).
    include/spkd.h defines what the library returns: no error, the log of the
    partial-pivoting LU determinant of the fp64 covariance -- noise of its own (a NaN, -inf
    or a large negative number), bit-reproducible for identical input; KL2 is NaN because
    the library inverts where the reference takes a pseudo-inverse (documented deviation)."""
    g = json.load(open(os.path.join(ROOT, 'tests/golden/functions.json')))
    feats, _, _ = session(g['session'])
    eng.set_features(feats)
    short = [p for p in g['pairs'] if min(p['a'][1] - p['a'][0], p['b'][1] - p['b'][0]) < 40]
    assert short
    for p in short:
        job = [([tuple(p['a'])], [tuple(p['b'])])]
        t1 = eng.pair_terms(job, want_glr=True, want_kl2=True)[0]
        t2 = eng.pair_terms(job, want_glr=True, want_kl2=True)[0]
        assert all(_same_bits(x, y) for x, y in zip(t1, t2))
        n_a = p['a'][1] - p['a'][0]
        ld_short = t1.logdet1 if n_a < 40 else t1.logdet2
        assert math.isnan(ld_short) or ld_short < -300.0, ld_short     # 39 pivots, >= 9 of them ~1e-16
        assert math.isfinite(t1.logdet2 if n_a < 40 else t1.logdet1)   # the full-rank partner is untouched
        # the reference's own values for this pair are NaN (BIC, GLR) and a finite pinv-based KL2
        assert math.isnan(float.fromhex(p['cl_bic_l1.3'])) and math.isfinite(float.fromhex(p['kl2']))
        assert math.isnan(t1.kl2)
    # in the clustering kernels the same records go through the four-per-wave elimination
    # and its pivoting fallback: same definition, same reproducibility
    segs = [tuple(short[0]['a']), tuple(short[0]['b']), (1241, 1900), (125, 1241)]
    r1 = eng.cluster_hi(segs, 1, 'BIC', 1.3, 0.0, 0)
    r2 = eng.cluster_hi(segs, 1, 'BIC', 1.3, 0.0, 0)
    assert len(r1.merges) == len(r2.merges)
    assert all(_same_bits(float(x[2]), float(y[2])) and x[:2] == y[:2] for x, y in zip(r1.merges, r2.merges))


def test_sliding_window_bic_kernel_against_reference_function(eng):
    """`-m sw -d BIC` crashes in the reference (the host raises the same
    error), but spkd_sw's BIC branch is part of the ABI: checked here against the
    reference's own bic() on the windows dist_sw would cut (functions_sw.json)."""
    g = json.load(open(os.path.join(ROOT, 'tests/golden/functions_sw.json')))
    feats, _, _ = session(g['session'])
    eng.set_features(feats)
    worst = 0.0
    for w in g['windows']:
        want = np.array([float.fromhex(v) for v in w['bic']])
        got = eng.sw([tuple(w['turn'])], 'BIC', w['lambda'], w['winsize'], w['winstep'])[0]
        assert len(got) == len(want) and len(want) > 3
        err = float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))
        assert err < 1e-9, (w['turn'], err)
        worst = max(worst, err)
    print('worst two-window BIC relative error vs the reference function: %.3g' % worst)


def test_kl2_deviations_are_the_documented_ones(eng):
    """KL2 where a covariance is not positive definite: the reference's
    SVD pinv gives a finite pseudo-inverse, the library's inverse gives NaN.  With two
    digital-silence segments in an AHC problem the NaN distances make numpy-style min()
    NaN: no merge at all unless -ms forces merging, and then every merge distance is NaN."""
    synth = pkg('synth')
    feats, _, truth = synth.make_session(4242, 600, 4)
    segs = [(a, b) for a, b, _ in truth][:20]
    f = feats.copy()
    for z in (3, 11):
        f[segs[z][0]:segs[z][1]] = 0.0
    eng.set_features(f)
    t = eng.pair_terms([([segs[3]], [segs[0]])], want_kl2=True)[0]
    assert math.isnan(t.kl2)
    free = eng.cluster_hi(segs, 1, 'KL2', 1.3, 12.0, 0)
    assert free.merges == []
    # -ms 5 forces merging through the NaN minimum: the first NaN cell wins twice (each
    # digital-silence segment is folded into a speech cluster, whose covariance is positive
    # definite again), after that the loop runs on ordinary finite distances
    forced = eng.cluster_hi(segs, 1, 'KL2', 1.3, 12.0, 5)
    assert len(forced.merges) >= len(segs) - 5
    assert [math.isnan(d) for _, _, d in forced.merges[:2]] == [True, True]
    assert all(math.isfinite(d) for _, _, d in forced.merges[2:])


def test_integration_md_ctypes_stub_runs():
    """The ctypes stub INTEGRATION.md shows a maintainer of the reference (its `bic`
    with the signature of spk-clustering.py:81) is executed as written -- only the library
    path is made absolute -- and reproduces the reference's own values."""
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    m = re.search(r"```python\n(# spkd_stub\.py.*?)```", text, flags=re.S)
    assert m, 'stub code block not found in INTEGRATION.md'
    code = m.group(1)
    assert "C.CDLL('libspkd_hip.so')" in code
    code = code.replace("C.CDLL('libspkd_hip.so')", 'C.CDLL(%r)' % pkg('hipabi').LIB_PATH)
    ns = {}
    exec(compile(code, 'spkd_stub.py', 'exec'), ns)
    g = json.load(open(os.path.join(ROOT, 'tests/golden/functions.json')))
    feats, _, _ = session(g['session'])
    for p in g['pairs'][:4]:
        x, y = feats[p['a'][0]:p['a'][1]], feats[p['b'][0]:p['b'][1]]
        got = ns['bic'](x, y, lambdac=g['lambda'])
        want = float.fromhex(p['cl_bic_l1.3'])
        assert _rel(got, want) < 1e-9, (p['a'], p['b'], got, want)


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_cli_case_matches_reference(case, tmp_path, eng):
    if case['name'] in NOT_YET:
        pytest.skip('mode not on the device yet')
    status, stdout, recipe, seg = run_case(case, tmp_path, eng)
    assert status == case['status']
    assert recipe == case['output_recipe']          # byte for byte
    assert seg == case['seg_recipe']
    if case['status'] == 'ok':
        # KL2 mixes float32 means into fp64: the north-star bar of
        # 1e-5 relative applies; BIC / GLR are held to 1e-9.
        kl2 = 'KL2' in case['argv_tail']
        assert_stdout_close(stdout, case['stdout'], rel=1e-5 if kl2 else 1e-9)


def _same_merges(a, b, rel=1e-9):
    assert len(a) == len(b), (a, b)
    for (a1, b1, d1), (a2, b2, d2) in zip(a, b):
        assert (a1, b1) == (a2, b2), (a, b)
        if math.isnan(d2):
            assert math.isnan(d1)
        elif math.isinf(d2):
            assert d1 == d2
        else:
            assert abs(d1 - d2) <= rel * max(1.0, abs(d2))


@pytest.mark.parametrize('variant', [1, 2])
def test_ahc_nan_and_inf_semantics_follow_numpy(eng, variant):
    """Digital-silence segments: a zero covariance gives log det = -inf, two of
    them give a NaN distance; numpy's min() then returns NaN and the merge loop
    stops at once unless -ms forces it, in which case argmin is the first NaN
    (SURVEY.md A-5, A-7).  Compared with the literal numpy restatement."""
    from oracle.numpy_engine import NumpyEngine
    synth = pkg('synth')
    feats, _, truth = synth.make_session(77, 120, 3)
    f = feats.copy()
    segs = [(a, b) for a, b, _ in truth][:9]
    f[segs[2][0]:segs[2][1]] = 0.0           # two all-zero segments
    f[segs[6][0]:segs[6][1]] = 0.0
    ne = NumpyEngine()
    ne.set_features(f)
    eng.set_features(f)
    for max_spk in (0, 4):
        want = ne.cluster_hi(segs, variant, 'BIC', 1.3, 0.0, max_spk)
        got = eng.cluster_hi(segs, variant, 'BIC', 1.3, 0.0, max_spk)
        _same_merges(got.merges, want.merges)
    # one zero segment only: +inf distances, never merged, the rest clusters normally
    f2 = feats.copy()
    f2[segs[2][0]:segs[2][1]] = 0.0
    ne.set_features(f2)
    eng.set_features(f2)
    want = ne.cluster_hi(segs, variant, 'BIC', 1.3, 0.0, 0)
    got = eng.cluster_hi(segs, variant, 'BIC', 1.3, 0.0, 0)
    _same_merges(got.merges, want.merges)
    assert len(got.merges) >= 1


@pytest.mark.parametrize('kind', ['BIC', 'GLR', 'KL2'])
@pytest.mark.parametrize('variant', [1, 2])
def test_ahc_launch_shapes_agree(eng, variant, kind):
    """The merge loop has two launch shapes (one workgroup per problem / a chain of
    launches over all CUs, spkd.h SPKD_AHC_*): same merges, same distances, same
    summary statistics, both equal to the C oracle; with NaN / inf inputs too."""
    from oracle.c_engine import COracleEngine
    synth = pkg('synth')
    hipabi = pkg('hipabi')
    feats, _, truth = synth.make_session(4242, 600, 4)
    segs = [(a, b) for a, b, _ in truth]
    assert len(segs) > 40
    thr = {'BIC': 0.0, 'GLR': 2500.0, 'KL2': 12.0}[kind]
    orc = COracleEngine()
    for zero in ((), (3, 11)):
        f = feats.copy()
        for z in zero:
            f[segs[z][0]:segs[z][1]] = 0.0
        orc.set_features(f)
        eng.set_features(f)
        for max_spk in (0, 3):
            got = {}
            for path in (hipabi.AHC_MONO, hipabi.AHC_WIDE):
                eng.ahc_path = path
                try:
                    got[path] = eng.cluster_hi(segs, variant, kind, 1.3, thr, max_spk)
                finally:
                    eng.ahc_path = hipabi.AHC_AUTO
            a, b = got[hipabi.AHC_MONO], got[hipabi.AHC_WIDE]
            assert [(x, y) for x, y, _ in a.merges] == [(x, y) for x, y, _ in b.merges]
            for (_, _, d1), (_, _, d2) in zip(a.merges, b.merges):
                assert d1 == d2 or (math.isnan(d1) and math.isnan(d2))      # same arithmetic: bit-equal
            for u, v in ((a.max_dist, b.max_dist), (a.min_dist, b.min_dist)):
                assert u == v or (u is not None and v is not None and math.isnan(u) and math.isnan(v))
            if kind != 'KL2' or not zero:
                want = orc.cluster_hi(segs, variant, kind, 1.3, thr, max_spk)
                _same_merges(b.merges, want.merges, rel=1e-5 if kind == 'KL2' else 1e-9)


@pytest.mark.parametrize('n', [65, 257])
@pytest.mark.parametrize('variant', [1, 2])
def test_merge_loop_selection_on_a_planted_matrix(eng, variant, n):
    """The merge loop on a caller's matrix (spkd_ahc_matrix) with ties and NaNs planted where the
    row scan and the selection over the rows have their seams: n = 65 is two 64-row mask chunks,
    the last with one row, and a tail lane in the scan; n = 257 a second trip of the scan's
    256-column loop that holds one live column.  Both launch shapes must agree to the bit, and
    the first merge must be numpy's M.min() / M.argmin() (first occurrence in row-major order;
    with a NaN present the minimum is NaN and the position the first NaN: CL1:203-204)."""
    synth = pkg('synth')
    hipabi = pkg('hipabi')
    feats, _, _ = synth.make_session(4242, 150, 3)
    begins = np.arange(n, dtype=np.int64) * 60              # 60-frame slices: full-rank covariances
    assert feats.shape[0] // 60 >= n
    ctx = eng.ctx
    d_fr = ctx.dev_alloc(feats.nbytes)
    d_st = ctx.dev_alloc(n * hipabi.REC * 8)
    d_m = ctx.dev_alloc(n * n * 8)
    try:
        ctx.h2d(d_fr, feats)
        ctx.set_stats(d_fr, feats.shape[0], begins, begins + 60, np.arange(n, dtype=np.int32), n, d_st)
        ctx.distance_rows(variant, 'BIC', 1.3, d_st, n, 0, n, d_m)
        M = np.empty((n, n), dtype=np.float64)
        ctx.d2h(M, d_m)
        if variant == 1:                                    # the form spkd.h asks of the caller
            diag = np.diag(M).copy()
            up = np.triu(M, 1)
            M = up + up.T
            M[np.diag_indices(n)] = diag
        iu = np.triu_indices(n, 1)
        assert np.all(np.isfinite(M[iu]))

        def put(r, c, v):
            M[r, c] = v
            if variant == 1:
                M[c, r] = v

        # (a) the global minimum at (1, 3), and its value again in a later column of that row
        # (another lane, another of the scan's loads in flight) and in a later row (another wave
        # of the selection): the first in row-major order has to win
        r0, c0 = [int(x[np.argmin(M[iu])]) for x in iu]
        g, old = M[r0, c0], M[1, 3]
        put(r0, c0, old)
        put(1, 3, g)
        far = 3 + 65 if n > 3 + 65 else n - 1
        put(1, far, g)
        put(n - 2, n - 1, g)
        # (b) a value below every other of row 5 (but above the global minimum) at the last column
        row5 = np.delete(M[5], 5)
        v = g + 0.5 * (row5.min() - g)
        assert g < v < row5.min() and g != 0.0 and v != 0.0
        put(5, n - 1, v)

        def run(M, max_spk, threshold):
            fin = M[iu][np.isfinite(M[iu])]
            got = {}
            for path in (hipabi.AHC_MONO, hipabi.AHC_WIDE):
                ctx.h2d(d_m, np.ascontiguousarray(M))
                p = hipabi.AhcParams(variant, hipabi.KINDS['BIC'], max_spk, path, 1.3, threshold)
                got[path] = ctx.ahc_matrix(d_st, n, p, d_m, float(fin.max()), float(fin.min()))
            a, b = got[hipabi.AHC_MONO], got[hipabi.AHC_WIDE]
            nm = int(a['n_merges'][0])
            assert int(b['n_merges'][0]) == nm
            assert np.array_equal(a['a'][:nm], b['a'][:nm]) and np.array_equal(a['b'][:nm], b['b'][:nm])
            for key in ('d', 'stat_max', 'stat_min'):       # equal to the bit, or both NaN
                x, y = a[key][:nm] if key == 'd' else a[key], b[key][:nm] if key == 'd' else b[key]
                assert np.array_equal(np.isnan(x), np.isnan(y)), key
                assert np.array_equal(x[~np.isnan(x)].view(np.uint64), y[~np.isnan(y)].view(np.uint64)), key
            # the first merge against numpy on the whole matrix (both variants scan every cell:
            # variant 2's lower triangle and diagonal hold +inf, variant 1's diagonal 2^63);
            # every cluster is alive, so the compacted indices are the cell's own
            want_d, pos = M.min(), int(M.argmin())
            r, c = divmod(pos, n)
            assert (int(a['a'][0]), int(a['b'][0])) == (min(r, c), max(r, c))
            assert (np.isnan(want_d) and np.isnan(a['d'][0])) or \
                np.float64(want_d).view(np.uint64) == a['d'][:1].view(np.uint64)[0]
            return nm, (min(r, c), max(r, c))

        nm, first = run(M, 0, 0.0)
        assert first == (1, 3)
        assert nm >= 10
        # (c) NaNs: one at the last column of row 7, one at an earlier cell of that row, and one
        # in a later row at a column in front of both: the first in row-major order is (7, 20).
        # The loop stops at a NaN minimum unless max_spk forces it: three forced merges, none
        # by the threshold.
        put(7, n - 1, float('nan'))
        put(7, 20, float('nan'))
        put(9, 12, float('nan'))
        nm, first = run(M, n - 3, -1e300)
        assert first == (7, 20)
        assert nm == 3
    finally:
        for d in (d_m, d_st, d_fr):
            ctx.dev_free(d)


def test_sliding_window_and_merge_modes_on_a_longer_file(eng, tmp_path):
    """sw (GLR), m (BIC with the frozen c1, GLR) on 10 minutes against the C oracle."""
    import io
    from oracle.c_engine import COracleEngine
    synth = pkg('synth')
    cli = pkg('cli')
    feats, vad, _ = synth.make_session(606, 600, 4)
    tmp = str(tmp_path)
    os.makedirs(os.path.join(tmp, 'fea'))
    synth.write_fea(os.path.join(tmp, 'fea', 'ten.fea'), feats)
    with open(os.path.join(tmp, 'vad.recipe'), 'w') as fh:
        fh.write(synth.vad_recipe_text('ten.wav', vad))
    outs = {}
    for tag, e in (('hip', eng), ('orc', COracleEngine())):
        sw = os.path.join(tmp, tag + '.sw.recipe')
        cli.main_change_detection([os.path.join(tmp, 'vad.recipe'), os.path.join(tmp, 'fea'), '-o', sw,
                                   '-t', '3000'], engine=e, stdout=io.StringIO())
        res = [open(sw).read()]
        for dist, extra in (('BIC', ['-l', '1.3']), ('GLR', ['-t', '1500'])):
            m = os.path.join(tmp, tag + '.m.' + dist + '.recipe')
            cli.main_change_detection([sw, os.path.join(tmp, 'fea'), '-o', m, '-m', 'm', '-d', dist] + extra,
                                      engine=e, stdout=io.StringIO())
            res.append(open(m).read())
        outs[tag] = res
    assert outs['hip'] == outs['orc']
    assert outs['hip'][0].count('\n') > len(vad)


def test_non_finite_covariance_raises_like_the_reference_but_writes_nothing(eng, tmp_path):
    """A NaN frame makes a covariance non-finite: scipy.linalg.det raises ValueError in the
    reference at the offending call, i.e. AFTER the lines of earlier turns were written and
    earlier `Merging:` lines printed.  The library reports it per launch: the same
    ValueError is raised, but nothing of the file group the launch covered is written or
    printed (documented deviation; failure path only)."""
    import io
    synth = pkg('synth')
    cli = pkg('cli')
    feats, vad, _ = synth.make_session(4242, 150, 3)
    bad = feats.copy()
    a, b = vad[len(vad) // 2]
    bad[(a + b) // 2, 7] = np.nan                  # inside a turn in the middle of the file
    tmp = str(tmp_path)
    os.makedirs(os.path.join(tmp, 'fea'))
    synth.write_fea(os.path.join(tmp, 'fea', 'x.fea'), bad)
    with open(os.path.join(tmp, 'vad.recipe'), 'w') as f:
        f.write(synth.vad_recipe_text('x.wav', vad))
    out = os.path.join(tmp, 'spkc.recipe')
    said = io.StringIO()
    with pytest.raises(ValueError, match='infs or NaNs'):
        cli.main_change_detection([os.path.join(tmp, 'vad.recipe'), os.path.join(tmp, 'fea') + '/', '-o', out,
                                   '-m', 'gw', '-d', 'BIC', '-w', '1.0', '-st', '3.0', '-dws', '0.1', '-l', '1.0'],
                                  engine=eng, stdout=said)
    assert not os.path.exists(out) or open(out).read() == ''
    # clustering: a recipe of clean turns plus one that covers the NaN frame
    good = os.path.join(tmp, 'turns.recipe')
    with open(good, 'w') as f:
        for k, (s, e) in enumerate(vad):
            f.write('audio=x.wav lna=a_%d start-time=%s end-time=%s speaker=spk_turn\n' % (
                k + 1, repr(s / 125.0), repr(e / 125.0)))
    said = io.StringIO()
    with pytest.raises(ValueError, match='infs or NaNs'):
        cli.main_clustering([good, os.path.join(tmp, 'fea') + '/', '-o', os.path.join(tmp, 'out.recipe'),
                             '-m', 'hi', '-l', '1.3'], variant=1, engine=eng, stdout=said)
    assert 'Merging:' not in said.getvalue()


def test_event_capacity_is_a_first_guess_that_doubles_until_it_fits(eng):
    """spkd_gw_event_capacity_p counts the scans of a window end that only moves forward; a
    turn that re-scans (a detection resets the end, spk-change-detection.py:264-266) can need
    more, is told SPKD_EOVERFLOW, and must still produce output like the reference does
    (ADVICE r2).  Data that breaks the guess is pathological and hard to synthesise, so the
    doubling is exercised from the other side: the first guess scaled down 64 times (2 event
    slots for most turns) must end in exactly the result of the ordinary call."""
    hipabi = pkg('hipabi')
    feats, vad, _ = session({'seed': 7001, 'seconds': 400, 'n_speakers': 4, 'kwargs': {},
                             'frames': 50000, 'sha256': json.load(open(os.path.join(
                                 ROOT, 'tests/golden/functions.json')))['session']['sha256']})
    eng.set_features(feats)
    b = np.array([s for (s, e) in vad], dtype=np.int64)
    e = np.array([e_ for (s, e_) in vad], dtype=np.int64)
    p = hipabi.CdParams(hipabi.KINDS['BIC'], 0, 1.0, 0.0, 125.0, 375.0, 12.0, 125.0)
    ref = eng.ctx.gw(eng.d_frames, eng.n_frames, b, e, p)
    small = eng.ctx.gw(eng.d_frames, eng.n_frames, b, e, p, first_guess_scale=1.0 / 64)
    assert int(small['off'][-1]) > 0 and int(ref['n_win'].max()) > 2      # the scaled guess was too small
    assert np.array_equal(ref['n_win'], small['n_win'])
    assert np.array_equal(ref['final_start'], small['final_start'])
    for t in range(len(b)):
        n, o1, o2 = int(ref['n_win'][t]), int(ref['off'][t]), int(small['off'][t])
        assert np.array_equal(ref['win_det'][o1:o1 + n], small['win_det'][o2:o2 + n])
        assert np.array_equal(ref['win_maxd'][o1:o1 + n], small['win_maxd'][o2:o2 + n], equal_nan=True)
        nd = int(ref['win_det'][o1:o1 + n].sum())
        for k in ('det_start', 'det_maxi', 'det_d'):
            assert np.array_equal(ref[k][o1:o1 + nd], small[k][o2:o2 + nd])
    # capacities the kernel would have refused at the first try
    assert int(small['off'][-1]) >= int(ref['n_win'].sum())


@pytest.mark.parametrize('kind', ['BIC', 'GLR'])
def test_gw_wave_shapes_agree(eng, kind, monkeypatch):
    """k_gw runs a turn on one, two, four or eight waves (chosen by the number of turns;
    SPKD_GW_WAVES pins it): the sums, the eliminations and the decisions are the same, so every
    output array is bit-identical."""
    import torch
    hipabi = pkg('hipabi')
    feats, vad, _ = session({'seed': 7001, 'seconds': 400, 'n_speakers': 4, 'kwargs': {},
                             'frames': 50000, 'sha256': json.load(open(os.path.join(
                                 ROOT, 'tests/golden/functions.json')))['session']['sha256']})
    eng.set_features(feats)
    b = np.array([s for (s, e) in vad], dtype=np.int64)
    e = np.array([e_ for (s, e_) in vad], dtype=np.int64)
    p = hipabi.CdParams(hipabi.KINDS[kind], 0, 1.0, 0.0, 125.0, 375.0, 12.0, 125.0)
    got = {}
    for nw in (1, 2, 4, 8):
        monkeypatch.setenv('SPKD_GW_WAVES', str(nw))
        ctx = hipabi.Context(0, torch.cuda.current_stream().cuda_stream)      # (reads the switch when it is made)
        try:
            got[nw] = ctx.gw(eng.d_frames, eng.n_frames, b, e, p)
        finally:
            ctx.close()
    ref = got[4]
    n_turns = len(b)
    assert sum(int(ref['win_det'][int(ref['off'][t]):int(ref['off'][t]) + int(ref['n_win'][t])].sum())
               for t in range(n_turns)) > 5
    for nw in (1, 2, 8):
        g = got[nw]
        assert np.array_equal(ref['n_win'], g['n_win']) and np.array_equal(ref['off'], g['off'])
        assert np.array_equal(ref['final_start'], g['final_start'])
        for t in range(n_turns):                     # (slots behind a turn's last event are not written)
            n, o = int(ref['n_win'][t]), int(ref['off'][t])
            assert np.array_equal(ref['win_det'][o:o + n], g['win_det'][o:o + n]), (nw, t)
            assert np.array_equal(ref['win_maxd'][o:o + n], g['win_maxd'][o:o + n], equal_nan=True), (nw, t)
            nd = int(ref['win_det'][o:o + n].sum())
            for k in ('det_start', 'det_maxi', 'det_d'):
                assert np.array_equal(ref[k][o:o + nd], g[k][o:o + nd], equal_nan=True), (nw, t, k)


def test_pair_terms_record_cache_is_transparent(eng):
    """engine.pair_terms keeps the statistics records of the frame sets it has seen on the device
    (the host-driven modes ask for the same sets again and again): terms from cached records,
    from a cache that was just emptied, and from one so small that it starts over in the middle
    of the sequence are the same bits."""
    synth = pkg('synth')
    feats, _, truth = synth.make_session(31337, 240, 3)
    eng.set_features(feats)
    segs = [(a, b) for a, b, _ in truth][:12]
    jobs = [([segs[i]], [segs[i + 1]]) for i in range(len(segs) - 1)]
    jobs += [(segs[:k], [segs[k]]) for k in range(2, 8)]                 # growing clusters, as spk_cluster_in asks
    jobs += [(tuple(segs[:k]), (segs[k],)) for k in range(2, 8)]         # the same as tuples
    def run():
        return [eng.pair_terms([j], want_glr=True, want_kl2=True)[0] for j in jobs] + \
            eng.pair_terms(jobs, want_glr=True, want_kl2=True)
    eng._forget_records()
    cold = run()
    warm = run()
    assert len(eng._rec_slot) > 0
    cap, buf = eng._rec_cap, eng._rec_buf
    try:
        eng._rec_cap, eng._rec_buf = 8, None
        eng._forget_records()
        tiny = [eng.pair_terms([j], want_glr=True, want_kl2=True)[0] for j in jobs]
    finally:
        if eng._rec_buf is not None:
            eng.ctx.dev_free(eng._rec_buf)
        eng._rec_cap, eng._rec_buf = cap, buf
        eng._forget_records()
    def bits(t):
        return tuple(np.float64(x).tobytes() if x is not None else None
                     for x in t)
    assert [bits(t) for t in cold] == [bits(t) for t in warm]
    assert [bits(t) for t in cold[:len(jobs)]] == [bits(t) for t in tiny]


class _NoChain(object):
    """An engine without the device chain of spk_cluster_in: the drivers fall back to one call per line."""

    def __init__(self, eng):
        self._eng = eng

    def __getattr__(self, name):
        if name == 'cluster_in':
            raise AttributeError(name)
        return getattr(self._eng, name)


def _in_mode(tmp, engine, variant, extra):
    import io
    cli = pkg('cli')
    out = os.path.join(tmp, 'in.recipe')
    if os.path.exists(out):
        os.remove(out)
    said = io.StringIO()
    err = None
    try:
        cli.main_clustering([os.path.join(tmp, 'spkc.recipe'), os.path.join(tmp, 'fea') + '/', '-o', out, '-m', 'in'] + extra,
                            variant=variant, engine=engine, stdout=said)
    except ValueError as e:
        err = str(e)
    return (open(out).read() if os.path.exists(out) else None), said.getvalue(), err


@pytest.mark.parametrize('variant', [1, 2])
def test_cluster_in_device_chain_equals_the_per_line_path(eng, variant, tmp_path):
    """spk_cluster_in as one device-resident chain (spkd_cluster_in: clusters as sums of their
    members' records, the decisions on the device, prints and statistics replayed on the host)
    against the same mode driven line by line (statistics of every cluster from its frames, one
    library call per line) and against the C oracle: same recipe lines, same summary, printed
    distances to 1e-9 -- BIC, GLR and KL2 (1e-4 against the oracle), a threshold that founds a cluster per line (the distance
    buffer's first guess overflows and is grown), and a NaN frame in a late line (the chain stops
    there, the per-line path raises where the reference does)."""
    from oracle.c_engine import COracleEngine
    synth = pkg('synth')
    tmp = str(tmp_path)
    feats, _, truth = synth.make_session(515, 900, 4)
    os.makedirs(os.path.join(tmp, 'fea'))
    lines = ['audio=s.wav lna=a_%d start-time=%s end-time=%s speaker=spk_turn\n' % (k + 1, a / 125.0, b / 125.0)
             for k, (a, b, _) in enumerate(truth)]
    assert len(lines) > 70
    with open(os.path.join(tmp, 'spkc.recipe'), 'w') as fh:
        fh.writelines(lines)

    def same(a, b, rel=1e-9):
        assert a[0] == b[0] and a[2] == b[2]
        assert_stdout_close(a[1], b[1], rel)

    synth.write_fea(os.path.join(tmp, 'fea', 's.fea'), feats)
    for extra in (['-l', '1.3', '-tt'], ['-d', 'GLR', '-t', '1800', '-tt'], ['-d', 'KL2', '-t', '12', '-tt'],
                  ['-l', '1.3', '-t=-1e30']):
        chain = _in_mode(tmp, eng, variant, extra)
        slow = _in_mode(tmp, _NoChain(eng), variant, extra)
        orc = _in_mode(tmp, COracleEngine(), variant, extra)
        assert chain[2] is None and chain[0].count('\n') == len(lines)
        # (KL2: the means enter rounded to float32, like np.mean of float32 frames; the C oracle and
        # the library round sums of different orders, a last-bit flip of a float32 mean is 1e-7 of a
        # delta and, squared and weighted, up to a few 1e-5 of a distance: the lines must agree, the
        # printed distances to 1e-4; chain and per-line path share the rounding)
        kl2 = 'KL2' in extra
        same(chain, slow, 1e-7 if kl2 else 1e-9)
        same(chain, orc, 1e-4 if kl2 else 1e-9)
        if kl2:
            assert 1 < len(set(re.findall(r'speaker=(\S+)', chain[0]))) < len(lines)
    assert len(set(re.findall(r'speaker=(\S+)', chain[0]))) == len(lines)          # the last run: a cluster per line
    bad = feats.copy()
    a, b, _ = truth[60]
    bad[(a + b) // 2, 7] = np.nan
    synth.write_fea(os.path.join(tmp, 'fea', 's.fea'), bad)
    chain = _in_mode(tmp, eng, variant, ['-l', '1.3', '-tt'])
    slow = _in_mode(tmp, _NoChain(eng), variant, ['-l', '1.3', '-tt'])
    assert chain[2] is not None and 'infs or NaNs' in chain[2]
    same(chain, slow)


@pytest.mark.parametrize('kind', ['BIC', 'GLR'])
def test_tiny_problems_through_every_chain(eng, kind):
    """One to five segments: the hand-off-free merge chain (one launch per merge, a bookkeeper
    workgroup beside the partners'), the one-workgroup merge loop and the spk_cluster_in chain
    on problems smaller than a wave pass -- no merges at all, one partner, a forced merge down
    to one speaker -- against the C oracle."""
    from oracle.c_engine import COracleEngine
    synth = pkg('synth')
    hipabi = pkg('hipabi')
    feats, _, truth = synth.make_session(7117, 120, 3)
    eng.set_features(feats)
    orc = COracleEngine()
    orc.set_features(feats)
    segs_all = [(a, b) for a, b, _ in truth]
    thr = {'BIC': 0.0, 'GLR': 2500.0}[kind]
    for n in (1, 2, 3, 5):
        segs = segs_all[:n]
        for max_spk in (0, 1):
            want = orc.cluster_hi(segs, 1, kind, 1.3, thr, max_spk)
            for path in (hipabi.AHC_MONO, hipabi.AHC_WIDE):
                eng.ahc_path = path
                try:
                    got = eng.cluster_hi(segs, 1, kind, 1.3, thr, max_spk)
                finally:
                    eng.ahc_path = hipabi.AHC_AUTO
                _same_merges(got.merges, want.merges)
                if max_spk == 1 and n > 1:
                    assert len(got.merges) == n - 1
        label, dists, done = eng.cluster_in(segs, kind, 1.3, thr)
        assert done == n and len(label) == n and int(label[0]) == 0
        assert [len(d) for d in dists] == [0] + [len(set(int(x) for x in label[:s])) for s in range(1, n)]


@pytest.mark.parametrize('kind', ['BIC', 'GLR'])
def test_step_chain_shapes_agree(kind, monkeypatch):
    """The hand-off-free merge chain deals a merge's partners 3, 7 or 15 to a workgroup (by the
    problem's size: a workgroup's record loads go through one CU's address unit, so with CUs to
    spare fewer partners per workgroup are back sooner) and runs four or eight waves a workgroup:
    same merges, same distances to the bit, same statistics whatever the shape."""
    synth = pkg('synth')
    hipabi = pkg('hipabi')
    engine = pkg('engine')
    feats, _, truth = synth.make_session(4243, 600, 4)
    segs = [(a, b) for a, b, _ in truth]
    thr = {'BIC': 0.0, 'GLR': 2500.0}[kind]
    got = []
    for sp, sw in ((3, 4), (7, 4), (15, 4), (15, 8)):
        monkeypatch.setenv('SPKD_STEP_PARTNERS', str(sp))
        monkeypatch.setenv('SPKD_STEP_WAVES', str(sw))
        e = engine.HipEngine(0)                       # (the switches are read when the context is made)
        try:
            e.set_features(feats)
            e.ahc_path = hipabi.AHC_WIDE
            got.append([e.cluster_hi(segs, v, kind, 1.3, thr, ms) for v in (1, 2) for ms in (0, 3)])
        finally:
            e.close()
    assert len(got[0][0].merges) > 20
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert [(x, y) for x, y, _ in a.merges] == [(x, y) for x, y, _ in b.merges]
            assert all(d1 == d2 or (math.isnan(d1) and math.isnan(d2)) for (_, _, d1), (_, _, d2) in zip(a.merges, b.merges))
            assert (a.max_dist, a.min_dist) == (b.max_dist, b.min_dist) or (a.max_dist != a.max_dist)


def test_wide_merge_loop_refuses_a_problem_above_its_limit():
    """The hand-off-free merge chain holds at most 16 384 records a problem (a matrix position
    is packed as row << 14 | column): one problem of 16 385 is refused with SPKD_EINVAL under
    WIDE and under AUTO, which picks WIDE for a single problem.  The records are allocated in
    full, so that a check placed after the n x n matrix is built costs time but reads nothing
    out of bounds."""
    hipabi = pkg('hipabi')
    n = 16385
    ctx = hipabi.Context(0)
    try:
        d_st = ctx.dev_alloc(n * hipabi.REC * 8)
        ctx.h2d(d_st, np.zeros((n, hipabi.REC), dtype=np.float64))
        for path in (hipabi.AHC_WIDE, hipabi.AHC_AUTO):
            p = hipabi.AhcParams(1, hipabi.KINDS['BIC'], 0, path, 1.3, 0.0)
            with pytest.raises(hipabi.SpkdError) as ei:
                ctx.ahc(d_st, [0, n], p)
            assert ei.value.status == hipabi.SPKD_EINVAL
            assert 'clustering problem larger than 16384 records (wide merge loop)' in str(ei.value)
        ctx.dev_free(d_st)
    finally:
        ctx.close()
