"""The mixture kernels (spkd_gmm_train, spkd_gmm_loglik_seq, spkd_ubm_stats) against a 50-digit
reference where EM's rules bite, on frames unlike the generator's (run with -m gpu on an MI355X).

Cases: tests/mixture_cases.py (the variance floor in the initial model and under EM, G_k < 2 at
G_k = 1 and 0 and a dead component afterwards, exp underflow and exact ties, initial slots for
K = 3, 5, 6, 7, cluster means up to 64 sigma from the origin).  Truth: tests/golden/mixture_exact.json
and .npz, tests/exact_mixture.py at 50 digits with centred variances, reproduced on the CPU by
tests/test_exact_mixture.py.

Every device value meets two bounds (mixture_cases.assert_row):
  tier     in a group whose stored tier is 1e-9 or 1e-5 the error against the reference, in the
           suite's measure |a - b| / max(1, |a|, |b|), is within that bar;
  kernel   the group's largest |a - b| is at most MARGIN = 64 times max(e, 2^-52 |value|max), e the
           float64 restatement's largest error against the reference as the fixture stores it.
The rules are exact: ok, ln w = -inf, the 79 doubles of a component that does not move, a floored
1 / var to 2 ulp of 1 / (var_floor V_d), two tied components bit-equal, a dead UBM component's record
0, nothing written beyond a call's own rows, every speaker alone as among the others.
"""
import numpy as np
import pytest

import mixture_cases as mc
import reseg_gmm_numpy as G
from reseg_helpers import Dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    d = Dev(mc.build()[0])
    yield d
    d.close()


@pytest.fixture(scope='module')
def fx():
    return mc.fixture()


def _jobs(prefixes):
    return [j for j in mc.jobs() if j['name'].split('/')[0] in prefixes]


def _report(rows):
    assert rows
    worst = {}
    for r in rows:
        if r['quotient'] > worst.get(r['group'], (-1.0, None))[0]:
            worst[r['group']] = (r['quotient'], r['case'])
    for g, (q, case) in sorted(worst.items()):
        print('largest device error / max(e, 2^-52 scale) of %-6s %8.3f (%s)' % (g, q, case))
    for r in rows:
        mc.assert_row(r)


def test_floor_in_the_initial_model_and_under_em(dev, fx):
    """floor: K = 3, var_floor 0.01 (1, 5 and 1 floored dimensions) and 0.5 (35, 39, 35), the initial
    model and three single steps each; every floored 1 / var is 1 / (var_floor V_d) to 2 ulp."""
    rows, far = [], 0
    for job in _jobs(('K3', 'K3h')):
        new, got, _ = mc.check_job(dev, fx, job)
        rows += new
        far = max(far, mc.check_floored(fx, job, 'floor', got['floor']))
    print('floored 1 / var: at most %d ulp from 1 / (var_floor V_d)' % far)
    _report(rows)


def test_starved_components_keep_what_entered(dev, fx):
    """sa (G_1 = 0: ln w = -inf, then a step with the component dead), sb (G_1 = 1: only the weight
    moves) and sc (G_1 = 3: it moves, all floor) in one call from the hand-written model."""
    rows = []
    for job in _jobs(('starved',)):
        new, got, start = mc.check_job(dev, fx, job)
        rows += new
        if job['name'] == 'starved/step1':
            assert [float(g) for g in fx['jobs'][job['name']]['sb']['G']][1] == 1.0
            assert got['sa'][1, 0] == -np.inf and got['sa'][1, 1:].tobytes() == start['sa'][1, 1:].tobytes()
            assert np.isfinite(got['sb'][1, 0]) and got['sb'][1, 1:].tobytes() == start['sb'][1, 1:].tobytes()
            assert (got['sc'][1, G.MEAN:G.IVAR] == 500.0).all()
            assert mc.check_floored(fx, job, 'sc', got['sc']) <= 2 and mc.floored_mask(fx, job, 'sc')[1].all()
            assert mc.check_floored(fx, job, 'sb', got['sb']) <= 2
        else:
            assert got['sa'][1].tobytes() == start['sa'][1].tobytes()          # dead stays dead, bit for bit
    _report(rows)


def test_scores_under_a_dead_component(dev, fx):
    _report(mc.check_scores(dev, fx))


def test_wide_gaps_ties_and_frames_that_are_not_finite(dev, fx):
    """wide, winf, wide3, wnan in one call from CUBE: seven exps underflow to 0, the frames of the
    identical components 6 and 7 give both 1/2, a frame of 3e38 leaves ok at 1, +inf and NaN do not
    (and their neighbours have the bits they have alone: check_job)."""
    rows = []
    for job in _jobs(('wide',)):
        new, got, _ = mc.check_job(dev, fx, job)
        rows += new
        for s in ('wide', 'wide3'):
            assert got[s][6].tobytes() == got[s][7].tobytes(), s
    _report(rows)


def test_initial_slots_of_odd_component_counts(dev, fx):
    """K = 3, 5, 6, 7 on 40 K, 40 K + 1, 40 K + K - 1 and 1089 frames: the initial model and one step
    (in which K = 7 leaves components of G_k < 2 where they were)."""
    rows = []
    for job in _jobs(('K3', 'K5', 'K6', 'K7')):
        if job['name'].split('/')[1] in ('init', 'step1'):
            rows += mc.check_job(dev, fx, job)[0]
    _report(rows)


def test_cluster_means_far_from_the_origin(dev, fx):
    """off1, off8, off64: K = 2 and 4, the initial model and three single steps."""
    rows = []
    for job in _jobs(('off2', 'off4')):
        rows += mc.check_job(dev, fx, job)[0]
    _report(rows)


def test_ubm_records_with_a_dead_component(dev, fx):
    _report(mc.check_ubm(dev, fx))
