"""tests/exact_mixture.py checked against brute force, tests/golden/mixture_exact.json and .npz reproduced and held
to its conditions, every case shown to reach the branch it is there for, and the float64 restatements
(tests/reseg_gmm_numpy.py, tests/link_clr_numpy.py) held to the fixture.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest
from mpmath import mp, mpf

import conditioned_cases as cc
import exact_mixture as E
import mixture_cases as mc
import reseg_gmm_numpy as G

DIM = E.DIM
TINY = mpf(10) ** -45


def _near(a, b):
    return abs(a - b) <= TINY * max(1, abs(a), abs(b))


def _frac(a):
    return [[Fraction(float(v)) for v in row] for row in np.asarray(a).tolist()]


def _start(rng, k_comp):
    m = np.zeros((k_comp, E.COMP))
    m[:, 0] = np.log(rng.dirichlet(np.ones(k_comp)))
    m[:, E.MEAN:E.IVAR] = rng.normal(0.0, 1.0, (k_comp, DIM))
    m[:, E.IVAR:E.NORM] = rng.uniform(0.5, 2.0, (k_comp, DIM))
    m[:, E.NORM] = -0.5 * (DIM * G.LN_2PI - np.log(m[:, E.IVAR:E.NORM]).sum(axis=1))
    return m


# ---------------------------------------------------------------------- the reference against brute force
def test_one_component_is_the_maximum_likelihood_gaussian():
    rng = np.random.default_rng(11)
    x = (rng.normal(0.0, 1.0, (45, DIM)) * mc.SCALES + 64.0 * mc.SCALES).astype(np.float32)
    model, total, g_k, ok, info = E.em_step(x, _start(rng, 1), 0.01)
    first, ok0, _ = E.init_model(x, 1, 0.01)
    assert ok and ok0 and g_k == [45] and info['unit'] == [True] and info['gaps'] == [0.0] * 45
    X = _frac(x)
    with mp.workdps(E.DPS + 10):
        for d in range(DIM):
            mean = sum(r[d] for r in X) / 45
            var = sum((r[d] - mean) ** 2 for r in X) / 45
            for m in (model, first):
                assert m[0][0] == 0
                assert _near(m[0][E.MEAN + d], mpf(mean.numerator) / mean.denominator)
                assert _near(1 / m[0][E.IVAR + d], mpf(var.numerator) / var.denominator)
        assert _near(model[0][E.NORM], -(DIM * mp.log(2 * mp.pi) - sum(mp.log(v) for v in model[0][E.IVAR:E.NORM])) / 2)


def test_five_frames_and_two_components_by_hand():
    """One step in fractions.Fraction with mpmath's exp, the floor active in some dimensions; then scores
    and the UBM record of the same frames."""
    rng = np.random.default_rng(12)
    x = rng.normal(0.0, 1.0, (5, DIM)).astype(np.float32)
    x[:, 4] = x[0, 4] + np.array([0.0, 0.0, 0.0, 0.0, 8.0], dtype=np.float32)          # its within-component variance is tiny
    start = _start(rng, 2)
    var_floor = 0.9
    model, total, g_k, ok, info = E.em_step(x, start, var_floor)
    assert not ok                                                           # 5 < 40 K frames; the model is formed all the same
    X, M = _frac(x), _frac(start)
    with mp.workdps(E.DPS + 10):
        fr = lambda q: mpf(q.numerator) / q.denominator                     # noqa: E731
        ls = [[fr(M[k][0]) + fr(M[k][E.NORM]) - fr(sum((X[t][d] - M[k][E.MEAN + d]) ** 2 * M[k][E.IVAR + d] for d in range(DIM))) / 2
               for k in range(2)] for t in range(5)]
        top = [max(l) for l in ls]
        es = [[mp.exp(l - m) for l in row] for row, m in zip(ls, top)]
        g = [[e / sum(row) for e in row] for row in es]
        ll = [m + mp.log(sum(row)) for row, m in zip(es, top)]
        assert _near(total, sum(ll))
        floored, moved = 0, 2
        for k in range(2):
            gk = sum(g[t][k] for t in range(5))
            assert _near(g_k[k], gk) and _near(model[k][0], mp.log(gk / 5))
            if gk < 2:                                                      # the component stays where it was
                assert [float(v) for v in model[k][1:]] == start[k, 1:].tolist() and info['ratio'][k] is None
                moved -= 1
                continue
            for d in range(DIM):
                xs = [fr(X[t][d]) for t in range(5)]
                mean = sum(g[t][k] * xs[t] for t in range(5)) / gk
                var = sum(g[t][k] * (xs[t] - mean) ** 2 for t in range(5)) / gk
                all_mean = sum(xs) / 5
                floor = mpf(var_floor) * sum((v - all_mean) ** 2 for v in xs) / 5
                floored += var < floor
                assert _near(model[k][E.MEAN + d], mean) and _near(1 / model[k][E.IVAR + d], max(var, floor))
                assert _near(info['ratio'][k][d], var / floor)
        assert floored >= 1 and moved >= 1
        sc, _ = E.scores(x, [start])
        assert all(_near(sc[t][0], ll[t]) for t in range(5))
        n, f, _ = E.ubm_record(x, start)
        for k in range(2):
            assert _near(n[k], sum(g[t][k] for t in range(5)))
            assert all(_near(f[k][d], sum(g[t][k] * fr(X[t][d]) for t in range(5))) for d in range(DIM))


def test_the_rules_of_the_contract():
    """exp flushes to 0 below the band; a component of G_k < 2 keeps what entered and one of G_k = 0 has
    ln w = -inf; a dead component takes no part; a frame that is not finite makes the speaker not ok."""
    rng = np.random.default_rng(13)
    x = rng.normal(0.0, 1.0, (90, DIM)).astype(np.float32)
    start = _start(rng, 2)
    start[1, E.MEAN:E.IVAR] = 100.0
    model, total, g_k, ok, info = E.em_step(x, start, 0.01)
    assert ok and g_k == [90, 0] and info['unit'] == [True, True] and max(g for g in info['gaps'] if g) <= -800.0
    assert model[1][0] == mpf('-inf') and [float(v) for v in model[1][1:]] == start[1, 1:].tolist()
    again, total2, g2, ok, info = E.em_step(x, E.to_float(model), 0.01)
    assert ok and g2 == [90, 0] and len(info['gaps']) == 90 and total2 > total
    assert [float(v) for v in again[1]] == [float(v) for v in model[1]]
    y = x.copy()
    y[17, 3] = np.inf
    assert E.em_step(y, start, 0.01)[3] is False and E.init_model(y, 2, 0.01)[1] is False
    assert E.init_model(x[:79], 2, 0.01)[1] is False and E.init_model(x[:80], 2, 0.01)[1] is True


# ---------------------------------------------------------------------- the fixture
def test_fixture_names_its_cases_and_frames():
    fx = mc.fixture()
    frames, spk = mc.build()
    assert fx['sha256'] == mc.sha256() and fx['seeds'] == mc.SEEDS and len(frames) <= 4200
    assert set(fx['jobs']) == {j['name'] for j in mc.jobs()}
    for name, rs in spk.items():
        assert [b for b, _ in rs] == sorted((b for b, _ in rs), reverse=True) and len(rs) >= 3, name   # descending in memory
        assert sum(e - b for b, e in rs) <= 2200
    assert spk['wnan'][0][1] == len(frames)
    assert sum(e - b for b, e in spk['floor']) == 1024 + 65
    for k, v in mc.hand_models().items():
        assert mc.hexes(v) == fx['hand'][k], k                              # the start models, bit for bit


def _without_e(entry):
    out = {k: v for k, v in entry.items() if k != 'groups'}
    out['tiers'] = {g: (v['tier'], v['vmax']) for g, v in entry.get('groups', {}).items()}
    return out


def _same_entry(got, want):
    """Bit for bit in everything the reference says; a restatement's e may differ with the BLAS that adds
    up its sums, by less than the factor 8 a group has to spare inside its tier (cc.TIER_SLACK)."""
    assert mc.same(_without_e(got), _without_e(want))
    for g, v in want.get('groups', {}).items():
        assert got['groups'][g]['e'] <= cc.TIER_SLACK * max(v['e'], mc.EPS * v['vmax']), (g, got['groups'][g], v)


@pytest.mark.parametrize('prefix', sorted({j['name'].split('/')[0] for j in mc.jobs()}))
def test_fixture_is_reproduced_bit_for_bit(prefix):
    fx = mc.fixture()
    for job in mc.jobs():
        if job['name'].split('/')[0] == prefix:
            got = mc.compute_job(fx, job)
            assert set(got) == set(fx['jobs'][job['name']])
            for spk in got:
                _same_entry(got[spk], fx['jobs'][job['name']][spk])


def test_scores_and_records_of_the_fixture_are_reproduced_bit_for_bit():
    fx = mc.fixture()
    _same_entry(mc.compute_scores(fx), fx['scores'])
    got = mc.compute_ubm(fx)
    for spk in mc.UBM_SPEAKERS:
        _same_entry(got[spk], fx['ubm'][spk])


def _entries(fx):
    for name, job in sorted(fx['jobs'].items()):
        for spk, e in sorted(job.items()):
            if e['ok']:
                yield name, spk, e


def test_fixture_meets_its_three_conditions():
    fx = mc.fixture()
    for name, spk, e in _entries(fx):
        assert mc.conditions_hold(e['G'], e['unit'], e['check']), (name, spk)
        assert e['check']['gap_min_above'] >= -700.0 and e['check']['gap_max_below'] <= -800.0
    assert fx['scores']['check']['in_band'] == 0
    for spk in mc.UBM_SPEAKERS:
        assert fx['ubm'][spk]['check']['in_band'] == 0
    assert len(mc.dump(fx)) < 100000                                         # the arrays are in mixture_exact.npz


def test_every_case_reaches_its_branch():
    fx = mc.fixture()
    jobs = fx['jobs']
    # the floor: in the initial model and in every step, in every component; at 0.5 in most dimensions
    for step in ('init', 'step1', 'step2', 'step3'):
        assert jobs['K3/' + step]['floor']['floored'] == [1, 5, 1]
        assert all(n >= 30 for n in jobs['K3h/' + step]['floor']['floored'])
    # G_k < 2: 0, 1 (exactly: sums of zeros and ones) and 3; then the dead component in training and in scoring
    st = jobs['starved/step1']
    assert [float(st[s]['G'][1]) for s in ('sa', 'sb', 'sc')] == [0.0, 1.0, 3.0]
    assert all(st[s]['unit'][1] for s in ('sa', 'sb', 'sc'))
    assert mc.ref_model(fx, 'starved/step1', 'sa')[1, 0] == -np.inf
    assert abs(mc.ref_model(fx, 'starved/step1', 'sb')[1, 0] - math.log(1.0 / 193.0)) < 1e-15
    assert st['sc']['floored'][1] == 39 and st['sb']['floored'] == [39, 0, 39]
    assert float(jobs['starved/step2']['sa']['G'][1]) == 0.0 and float(jobs['starved/step2']['sa']['L']) > float(st['sa']['L'])
    assert [m[k, 0] for m, k in zip(mc.score_models(fx)[0][:3], (0, 1, 2))] == [-np.inf] * 3
    soft = [float(g) for s in ('floor', 'o7a', 'o7b', 'o7c') for g in jobs['K7/step1'][s]['G'] if float(g) < 2.0]
    assert len(soft) >= 4 and all(g != int(g) for g in soft)                # and G_k < 2 that no one planted
    # underflow and ties: every l_k - m of the wide speakers is 0 or below the band; halves and eighths
    for s in ('wide', 'wide3'):
        c = jobs['wide/step1'][s]['check']
        assert c['gap_min_above'] == 0.0 and c['gap_max_below'] <= -800.0 and jobs['wide/step1'][s]['ok']
    assert [float(g) for g in jobs['wide/step1']['wide']['G']] == [48.0] * 6 + [48.5] * 2
    assert [float(g) for g in jobs['wide/step1']['wide3']['G']] == [48.125] * 4 + [47.125, 48.125, 48.625, 48.625]
    for s in ('wide', 'wide3'):
        m = mc.ref_model(fx, 'wide/step1', s)
        assert m[6].tobytes() == m[7].tobytes()
    assert not jobs['wide/step1']['winf']['ok'] and not jobs['wide/step1']['wnan']['ok']
    assert mc.frames_of('wide3').max() == np.float32(3.0e38)
    # slot edges that are rounded down
    for K in mc.ODD_K:
        for n in (40 * K + 1, 40 * K + K - 1) + ((1089,) if K != 3 else ()):           # (1089 = 3 * 363)
            assert any(k * n % K for k in range(1, K)), (K, n)
        assert {'o%d%s' % (K, t) for t in 'abc'} | {'floor'} <= set(jobs['K%d/init' % K]) & set(jobs['K%d/step1' % K])
    # the dead UBM component
    for s in mc.UBM_SPEAKERS:
        rec = fx['ubm'][s]['record'].reshape(8, 40)
        assert (rec[mc.UBM_DEAD] == 0.0).all() and abs(rec[:, 0].sum() - len(mc.frames_of(s))) < 1e-9


def test_restatements_are_within_the_tiers_the_fixture_gives_them():
    """reseg_gmm_numpy and link_clr_numpy against the reference, group by group: the stored e is within the
    stored tier, and the tiers are what DESIGN.md's accuracy domain of the mixtures says: 1e-9 everywhere,
    the clusters 64 sigma from the origin included."""
    fx = mc.fixture()
    worst = {}
    groups = [(n + '/' + s, e['groups']) for n, s, e in _entries(fx)]
    groups += [('scores', fx['scores']['groups'])] + [('ubm/' + s, fx['ubm'][s]['groups']) for s in mc.UBM_SPEAKERS]
    for case, gs in groups:
        for g, v in gs.items():
            assert v['tier'] == '1e-9', (case, g, v)
            key = (case.split('/')[0] if not case.split('/')[-1].startswith('off') else case.split('/')[-1], g)
            worst[key] = max(worst.get(key, 0.0), v['e'])
    for key, e in sorted(worst.items()):
        print('%-8s %-6s restatement error at most %.3g' % (key[0], key[1], e))
