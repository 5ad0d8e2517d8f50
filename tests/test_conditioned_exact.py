"""The moment and determinant kernels against exact arithmetic, on frames unlike the generator's
(run with -m gpu on an MI355X).

Cases: tests/conditioned_cases.py (scales over 2^12, covariance cond up to 1e9, temporal
correlation, dither-like dimensions; means of 0, 1, 8 and 64 sigma; sets of 40 frames up to two
STATS_CHUNKs).  Truth: tests/golden/conditioned_exact.json, exact integer moments and fraction-free
determinants (tests/exact_moments.py), reproduced on the CPU by tests/test_exact_moments.py.

Two assertions hold for every device value (conditioned_cases.assert_row):
  tier     in a group whose stored tier is 1e-9 (the suite's bar) or 1e-5 (the north star of
           BASELINE.json) the device's error against exact is within that bar.  The tier is the
           one the C oracle -- the device's formulation, raw moments and an elimination without
           pivoting, on the CPU -- reaches with a factor 8 to spare; `outside` groups are beyond
           what the formulation can do ("Accuracy domain") and have no bar.
  kernel   in every group the device's worst error is at most max(K x the C oracle's, 1e-12):
           a kernel may not be worse than its own formulation.
"""
import pytest

import conditioned_cases as cc
from conftest import pkg

pytestmark = pytest.mark.gpu

# K: the largest device / C-oracle quotient measured over all rows above the 1e-12 floor was 15.7
# (pair_terms, corr6/1/40x41: 9.96e-10 against 6.34e-11; one MI355X, tools/conditioned_accuracy.py,
# profiles/conditioned_accuracy.json), times 4 -- the device eliminates in another order than the
# oracle, and within one group the CPU formulations scatter by about that much -- rounded up to
# a power of two.  A quotient above 64 is a kernel worse than its formulation: a finding to track
# down in the kernel, not a constant to raise.  (Why that one group is 15.7: its 40- and 41-frame
# sample covariances have cond 3e10 and 5e9, and the formulation itself scatters from 1.1e-9 to 1.0e-8
# there over 40 orders of elimination on the CPU; the C oracle's 6.3e-11 is the lucky figure, the
# device's 1.0e-9 the good end of the scatter.  DESIGN.md, "Accuracy domain".)
K_MEASURED = 15.7
K = 64


@pytest.fixture(scope='module')
def eng():
    e = pkg('engine').HipEngine(0)
    yield e
    e.close()


@pytest.fixture(scope='module')
def ce():
    from oracle.c_engine import COracleEngine
    return COracleEngine(1)


def _each(buffers, ce, engines):
    for (cls, m) in buffers:
        f = cc.buffer(cls, m)
        ce.set_features(f)
        for e in engines:
            e.set_features(f)
        yield cls, m


def _assert_rows(rows):
    assert rows
    for r in rows:
        print('%-24s %-22s tier %-7s C %.2e  device %.2e' % (r['group'], r['what'], r['tier'], r['c'], r['dev']))
    for r in rows:
        cc.assert_row(r, K)


PROBLEMS = [(c, m) for c in cc.CLASSES for m in cc.PROBLEM_OFFSETS]


def test_records_hold_the_exact_moments(eng):
    """spkd_set_stats on every pair's two sets, on multi-range sets cut at 63 / 64 / 65 and at
    1023 / 1024 / 1025 frames, and on one chunk plus one frame: the count entry is exact and every
    moment satisfies |got - exact| <= (n + 64) 2^-53 sum_t |x_ti x_tj| (derived: see
    conditioned_cases.record_check).  Beside test_stats_records_match_direct_sums, whose
    max(1, |want|) scale cannot see cancellation."""
    worst = 0.0
    sets = cc.record_sets()
    for (cls, m) in cc.all_buffers():
        f = cc.buffer(cls, m)
        eng.set_features(f)
        got = eng.stats(sets)
        ef = cc.exact_frames(cls, m)
        for k, s in enumerate(sets):
            exact_n, w = cc.record_check(got[k], ef, f, s)
            assert exact_n, (cls, m, s)
            assert w <= 1.0, (cls, m, s, w)
            worst = max(worst, w)
    print('worst |got - exact| as a fraction of the bound: %.3g' % worst)


def test_pair_terms_against_exact(eng, ce):
    """logdet1, logdet2, logdet_union, logdet_glr and the BIC / GLR assembled from them on every
    pair; KL2 and KL2P at offset 0 (28 pairs reach the pseudo-inverse mode, no more)."""
    pinv = pkg('engine').HipEngine(0, kl2_pinv=True)
    try:
        rows = []
        for cls, m in _each(cc.all_buffers(), ce, (eng, pinv)):
            rows += cc.check_pairs(cls, m, ce, eng, pinv)
    finally:
        pinv.close()
    assert len(rows) == 28 * 4 + 7 * 4 * 2
    _assert_rows(rows)


def test_distance_matrix_rows_and_sliding_window_against_exact(eng, ce):
    """The 7-record problems through spkd_distance_matrix and spkd_distance_rows (variants 1 and
    2), BIC and GLR: 21 pairs, so the last quad of the four-per-wave elimination holds one live
    matrix.  spkd_sw shares the kernels: one call per class on 64-frame windows."""
    rows = []
    for cls, m in _each(PROBLEMS, ce, (eng,)):
        rows += cc.check_matrix(cls, m, ce, eng)
    assert len([r for r in rows if r['what'] == 'sw']) == len(cc.CLASSES)
    _assert_rows(rows)


def test_growing_window_against_exact(eng, ce):
    """engine.gw(trace=True) on the stationary turns under a threshold no distance reaches: the
    candidate list (start, i, n1, n2) is the reference's (the fixture's, which
    test_exact_moments.py holds against NumpyEngine) and every sampled candidate's distance is
    checked against exact -- the P(c) - P(b) differences of running sums over an epoch that has
    grown to the whole 1 500-frame turn."""
    rows = []
    for cls, m in _each(PROBLEMS, ce, (eng,)):
        rows += cc.check_gw(cls, m, ce, eng)
    assert all(r['same'] for r in rows), [r for r in rows if not r['same']]
    _assert_rows(rows)


def test_cluster_hi_against_exact(eng, ce):
    """The 6-segment problems forced down to one speaker, AHC_MONO and AHC_WIDE, BIC and GLR: in
    tiers 1e-9 and 1e-5 the merge order is the exact greedy order, and every merge distance --
    so every merged record's sums -- is checked against exact (in `outside` groups: up to where
    the orders part)."""
    rows = []
    for cls, m in _each(PROBLEMS, ce, (eng,)):
        rows += cc.check_merge(cls, m, ce, eng)
    for r in rows:
        if r['tier'] != 'outside':
            assert r['same'], r
    _assert_rows(rows)


def test_gauss_models_and_loglik_against_exact(eng, ce):
    """Every pair's two sets (224 models): model_ok is true -- every case is full rank, and cond
    1e9 is far inside GS_PIVOT_REL = 2^-40 -- and the constant c is checked against the exact
    log-det.  One set per buffer (sizes and sides take turns): the scores of 8 probe frames
    against tests/reseg_numpy.py's definition evaluated in mpmath (stored by the maker).  The
    formulation's column is reseg_numpy in fp64 on the C oracle's record; the scores are float32
    on the device, so half an ulp of that is allowed on top."""
    rows = []
    for cls, m in _each(cc.all_buffers(), ce, (eng,)):
        rows += cc.check_gauss(cls, m, ce, eng)
    assert len(rows) == 28 * (8 + 1)
    assert all(r['ok'] for r in rows), [r for r in rows if not r['ok']]
    _assert_rows(rows)
