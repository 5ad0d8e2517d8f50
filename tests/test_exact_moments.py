"""The exact helper (tests/exact_moments.py), the conditioned fixture and the formulation's
accuracy domain on the CPU.  No device is involved: these run everywhere.

  * self-checks of the exact arithmetic: planted determinants, rank deficiency, agreement with
    mpmath.det, invariance under a shift of all frames (what the raw-moment records rely on);
  * tests/golden/conditioned_exact.json is reproduced bit for bit: every entry with at most 130
    frames and every fourth of the rest;
  * section "Accuracy domain" of DESIGN.md: against exact, the C oracle (the device's
    formulation) stays within the tier the fixture stores for each group, and the reference's
    arithmetic (oracle.numpy_engine) within the north star's 1e-5 on every pair.
"""
import math

import mpmath
import numpy as np
import pytest

import conditioned_cases as cc
import exact_moments as em


def _int_matrix(seed, n, lo, hi):
    u = cc.synth._uniform(seed, 7, n * n).reshape(n, n)
    return [[int(lo + math.floor(v * (hi - lo + 1))) for v in row] for row in u]


def _matmul(a, b):
    n = len(a)
    return [[sum(a[i][k] * b[k][j] for k in range(n)) for j in range(n)] for i in range(n)]


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_bareiss_finds_a_planted_determinant(seed):
    """T = (lower, planted diagonal) x U1 x U2 with unit-triangular U: det T = prod diag, whatever
    the fill; a permutation of the rows flips the sign and forces the pivot search."""
    n = 39
    r = _int_matrix(seed, n, -9, 9)
    diag = [3 + (7 * i + seed) % 11 for i in range(n)]
    diag[5] = -diag[5]
    low = [[r[i][j] if j < i else (diag[i] if i == j else 0) for j in range(n)] for i in range(n)]
    u1 = [[r[j][i] if j > i else (1 if i == j else 0) for j in range(n)] for i in range(n)]
    u2 = [[r[i][j] if j < i else (1 if i == j else 0) for j in range(n)] for i in range(n)]
    t = _matmul(_matmul(low, u1), u2)
    want = 1
    for v in diag:
        want *= v
    assert em.bareiss_det(t) == want
    t[0], t[1] = t[1], t[0]
    assert em.bareiss_det(t) == -want
    z = [row[:] for row in t]
    z[0] = [0] * n                                   # first column stays: a zero pivot at step 0
    z[0][3] = 1
    assert em.bareiss_det(z) == em.bareiss_det([row[:] for row in z][::-1]) * (-1) ** (n * (n - 1) // 2)
    # the symmetric path on a planted SPD matrix
    g = _matmul(low, [list(c) for c in zip(*low)])
    assert em.bareiss_det(g, symmetric=True) == want * want == em.bareiss_det(g)


def test_rank_deficient_set_has_log_det_minus_infinity():
    ef = cc.exact_frames('plain', 0)
    assert em.logdet_cov(ef.moments([(0, 39)])) == mpmath.mpf('-inf')         # 39 frames: rank 38
    f = np.array(cc.buffer('corr6', 8)[:200])
    f[:, 7] = f[:, 3] * np.float32(2.0)                                        # a dimension twice
    assert em.logdet_cov(em.ExactFrames(f).moments([(0, 200)])) == mpmath.mpf('-inf')
    assert math.isfinite(float(em.logdet_cov(ef.moments([(0, 40)]))))          # 40 frames: full rank


@pytest.mark.parametrize('case', [('plain', 0, (3100, 3140)), ('corr9', 64, (3200, 3264)), ('scales', 8, (0, 300))])
def test_bareiss_agrees_with_mpmath_det(case):
    cls, m, rng = case
    mom = cc.exact_frames(cls, m).moments([rng])
    a = mom.scatter()
    exact = em.bareiss_det(a, symmetric=True)
    assert exact == em.bareiss_det(a)
    with mpmath.workprec(400 + 40 * 39):             # the matrix's entries are integers of ~100 bits
        got = mpmath.det(mpmath.matrix(a))
        assert abs(got - exact) <= abs(mpmath.mpf(exact)) * mpmath.mpf(2) ** -400


def test_exact_moments_are_the_sums():
    """The limb products against plain Python integer sums, and against the fixture's decimals."""
    ef = cc.exact_frames('corr9', 64)
    rng = [(1020, 1030), (4090, 4103)]
    mom = ef.moments(rng)
    rows = [ef.frame(t) for a, b in rng for t in range(a, b)]
    assert mom.n == len(rows) == 23
    assert mom.s == [sum(r[i] for r in rows) for i in range(cc.DIM)]
    assert mom.m == [[sum(r[i] * r[j] for r in rows) for j in range(cc.DIM)] for i in range(cc.DIM)]
    f = cc.buffer('corr9', 64)
    x = np.concatenate([f[a:b] for a, b in rng]).astype(np.float64)
    assert np.array_equal(np.array(mom.s, dtype=np.float64) / 2.0 ** mom.k, x.sum(axis=0))    # 23 terms: exact
    for rec in cc.fixture()['moments']:
        cls, m = rec['buffer'].split('/')
        mom = cc.exact_frames(cls, int(m)).moments([tuple(r) for r in rec['ranges']])
        assert (mom.n, mom.k) == (rec['n'], rec['k'])
        assert [str(v) for v in mom.s] == rec['s']
        assert [str(mom.m[i][j]) for i in range(cc.DIM) for j in range(i, cc.DIM)] == rec['m']


@pytest.mark.parametrize('cls', ['plain', 'corr9', 'quiet'])
def test_covariance_is_invariant_under_a_shift_of_all_frames(cls):
    """Shifting every frame by one constant vector changes no exact log-det, BIC, GLR or KL2
    (KL2 takes differences of means): INTEGRATION.md's advice to subtract a constant vector from
    un-centred features rests on this.  The shift is a multiple of the frames' own grid, so the
    shifted frames are exact too (they are never rounded to float32 here)."""
    ef = cc.exact_frames(cls, 0)
    ra, rb = (3100, 3141), (3141, 3200)
    m1, m2 = ef.moments([ra]), ef.moments([rb])
    shift = [((-1) ** j) * (1000003 + 17 * j) << 8 for j in range(cc.DIM)]

    def shifted(mom):
        d = cc.DIM
        s = [mom.s[i] + mom.n * shift[i] for i in range(d)]
        mm = [[mom.m[i][j] + shift[i] * mom.s[j] + shift[j] * mom.s[i] + mom.n * shift[i] * shift[j]
               for j in range(d)] for i in range(d)]
        return em.Moments(mom.n, s, mm, mom.k)

    s1, s2 = shifted(m1), shifted(m2)
    assert s1.scatter() == m1.scatter() and (s1 + s2).scatter() == (m1 + m2).scatter()
    a, b = em.pair_logdets(m1, m2), em.pair_logdets(s1, s2)
    assert all(x == y for x, y in zip(a, b))
    with mpmath.workprec(em.MP_BITS_INV):
        assert abs(em.kl2(m1, m2) - em.kl2(s1, s2)) <= abs(em.kl2(m1, m2)) * mpmath.mpf(2) ** -300
    # and the shifted moments are those of shifted frames
    rows = [[v + sh for v, sh in zip(ef.frame(t), shift)] for t in range(*ra)]
    assert s1.s == [sum(r[i] for r in rows) for i in range(cc.DIM)]
    assert s1.m[3][7] == sum(r[3] * r[7] for r in rows)


# ---------------------------------------------------------------------- the fixture
def test_fixture_names_its_cases_and_environment():
    fx = cc.fixture()
    assert set(fx['buffers']) == {cc.group_name(c, m) for c, m in cc.all_buffers()}
    assert {'numpy', 'scipy', 'mpmath'} <= set(fx['env'])
    assert len(fx['moments']) <= 12
    for cls, want in (('corr3', 1e3), ('corr6', 1e6), ('corr9', 1e9)):
        assert want / 10 <= fx['buffers'][cc.group_name(cls, 0)]['cond'] <= want * 10
    for (cls, m) in cc.all_buffers():
        e = fx['buffers'][cc.group_name(cls, m)]
        assert set(e['pairs']) == {cc.size_key(s) for s in cc.SIZES}
        assert ('matrix' in e) == ('merge' in e) == ('gw' in e) == (m in cc.PROBLEM_OFFSETS)
        assert ('sw' in e) == (m == cc.PROBLEM_OFFSETS[-1]) and e['gauss']['tier'] in cc.TIERS
        for p in e['pairs'].values():
            assert all(math.isfinite(float.fromhex(v[0])) for v in p['ld'])           # full rank
            assert ('kl2' in p) == (m == 0)
        if 'merge' in e:
            assert all(e['merge'][k]['gap'] > cc.MERGE_MIN_GAP for k in ('BIC', 'GLR'))
            assert len(e['gw']['samples']) <= cc.GW_SAMPLES


@pytest.mark.parametrize('cls', cc.CLASSES)
def test_fixture_is_reproduced_bit_for_bit(cls):
    """Every entry of at most 130 frames -- the 40 + 41 and 64 + 65 pairs, the matrix problems'
    seven record log-dets, the sliding windows (128 frames) -- and every fourth of the rest: large
    pairs, matrix distances, merge orders, growing-window samples (the smallest candidate has 187
    frames), Gaussian probe scores."""
    fx = cc.fixture()
    geo = cc.gw_geometry()
    ci = cc.CLASSES.index(cls)
    for oi, m in enumerate(cc.OFFSETS):
        e = fx['buffers'][cc.group_name(cls, m)]
        ef = cc.exact_frames(cls, m)                  # (cc.buffer checks the sha256)
        turn = (ci * len(cc.OFFSETS) + oi)
        for si, size in enumerate(cc.SIZES):
            if sum(size) <= 130 or (turn + si) % 4 == 0:
                got = cc.exact_pair(ef, size, want_kl2=(m == 0))
                want = {k: v for k, v in e['pairs'][cc.size_key(size)].items() if not k.startswith('tier')}
                assert got == want, (cls, m, size)
        if turn % 4 == 0:
            assert cc.gauss_scores_exact(ef, cls, m)['scores'] == e['gauss']['scores']
        if 'sw' in e:
            got = cc.sw_exact(ef)
            assert (got['bic'], got['glr']) == (e['sw']['bic'], e['sw']['glr'])
        if m in cc.PROBLEM_OFFSETS:
            which = (ci * len(cc.PROBLEM_OFFSETS) + cc.PROBLEM_OFFSETS.index(m)) % 4
            got = cc.exact_matrix(ef, None if which == 0 else set())
            assert got['ld'] == e['matrix']['ld']
            if which == 0:
                assert (got['bic'], got['glr']) == (e['matrix']['bic'], e['matrix']['glr'])
            elif which == 1:
                assert cc.exact_merge(ef, 'BIC') == e['merge']['BIC']
            elif which == 2:
                assert cc.exact_merge(ef, 'GLR') == e['merge']['GLR']
            else:
                assert min(g[2] + g[3] for g in geo) > 130              # (no candidate is that small)
                idx = [s['k'] for s in e['gw']['samples']]
                assert cc.exact_gw(ef, geo, idx) == e['gw']['samples']


def test_growing_window_candidates_are_geometry_alone():
    """The stationary turn under a threshold no distance reaches: the reference's loop lists the
    same candidates for BIC and GLR on unlike data, the fixture's list, whose last scans span
    the whole turn."""
    from oracle.numpy_engine import NumpyEngine
    fx = cc.fixture()
    geo = cc.gw_geometry()
    assert len(geo) == fx['gw']['n_candidates']
    ne = NumpyEngine()
    for (cls, m, kind) in (('plain', 0, 'BIC'), ('corr6', 8, 'GLR')):
        ne.set_features(cc.buffer(cls, m))
        cands = cc.gw_candidates(ne, kind)
        assert [list(c[:4]) for c in cands] == geo
        assert all(abs(c[4] - cc.GW_THRESHOLD) / cc.GW_THRESHOLD >= 1e-3 for c in cands)
    assert max(c[2] + c[3] for c in geo) == cc.GW_TURN[1] - cc.GW_TURN[0]


# ---------------------------------------------------------------------- the formulation's domain
@pytest.mark.parametrize('cls', cc.CLASSES)
def test_formulations_against_exact_on_the_cpu(cls):
    """Against exact: the C oracle (raw moments, the device's formulation) stays within each
    group's stored tier; the reference's arithmetic (np.cov, pivoted LU) within 1e-5 on every
    pair: BIC and GLR at every offset, KL2 at offset 0.  KL2 has its tier and its bar at offset 0
    only: elsewhere the reference's float32 np.mean governs its value, which is a separate
    question.  (corr9 / 0 is a replacement buffer for that reason: conditioned_cases.REPLACED.)"""
    from oracle.c_engine import COracleEngine
    from oracle.numpy_engine import NumpyEngine
    fx = cc.fixture()
    ce, ne = COracleEngine(1), NumpyEngine()
    for m in cc.OFFSETS:
        e = fx['buffers'][cc.group_name(cls, m)]
        f = cc.buffer(cls, m)
        ce.set_features(f)
        ne.set_features(f)
        c_err, n_err = cc.pairs_errors(ce, e), cc.pairs_errors(ne, e)
        for size in cc.SIZES:
            k = cc.size_key(size)
            p = e['pairs'][k]
            print('%-22s C %.2e  numpy %.2e  tier %s' % (cc.group_name(cls, m, size), cc.worst_of(c_err[k]),
                                                         cc.worst_of(n_err[k]), p['tier']))
            assert p['tier'] in cc.TIERS
            if p['tier'] != 'outside':
                assert cc.worst_of(c_err[k]) <= cc.TIER_BAR[p['tier']], (cls, m, size, c_err[k])
            if p.get('tier_kl2', 'outside') != 'outside':
                assert c_err[k]['kl2'] <= cc.TIER_BAR[p['tier_kl2']], (cls, m, size, c_err[k])
            assert max(n_err[k]['bic'], n_err[k]['glr']) <= 1.0e-5, (cls, m, size, n_err[k])
            if m == 0:
                assert n_err[k]['kl2'] <= 1.0e-5, (cls, m, size, n_err[k])
        w = cc.gauss_reference_scores_error(ce, f, cls, m, e)
        if e['gauss']['tier'] != 'outside':
            assert w <= cc.TIER_BAR[e['gauss']['tier']], (cls, m, 'gauss scores', w)
        if m in cc.PROBLEM_OFFSETS:
            worst = {'matrix': cc.matrix_errors_from_terms(ce, e), 'merge': 0.0, 'gw': 0.0}
            geo = cc.gw_geometry()
            for kind in ('BIC', 'GLR'):
                same, err = cc.merge_errors(ce, e, kind)
                worst['merge'] = max(worst['merge'], err if same else float('inf'))
                same, err = cc.gw_errors(ce, e, kind, geo)
                worst['gw'] = max(worst['gw'], err if same else float('inf'))
            if 'sw' in e:
                worst['sw'] = cc.sw_errors(ce, e['sw'])
            for name, w in worst.items():
                tier = e[name]['tier']
                print('%-22s C %.2e  tier %s' % (cc.group_name(cls, m) + '/' + name, w, tier))
                if tier != 'outside':
                    assert w <= cc.TIER_BAR[tier], (cls, m, name, w)
