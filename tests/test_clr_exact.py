"""The CLR chain (spkd_clr_link) and the gallery (spkd_clr_identify, spkd_bw_accumulate) against exact
values on the records of tests/clr_cases.py, and against tests/clr_fast_numpy.py at sizes where the
kernels' loops go round more than once.

CPU: exact_clr checked by hand; tests/golden/clr_exact.json reproduced bit for bit; the float64
restatements inside their tiers; every case's own condition; clr_fast_numpy equal to the loops of
link_clr_numpy and gallery_numpy on the fixtures of test_link_clr.py and test_gallery.py; the large
cases' margins.
GPU: every value of the small groups inside its tier and within MARGIN = 64 times max(e, 2^-52 |v|max)
of the exact value; the bits of a pair the same from k_clr_matrix, k_clr_chain's recompute and
k_ident_scores; logs, labels and identities equal to the exact ones; the large sizes equal to
clr_fast_numpy's decisions."""
import functools
import time
from fractions import Fraction

import numpy as np
import pytest

import clr_cases as cc
import clr_fast_numpy as F
import exact_clr as X
import gallery_numpy as GN
import link_clr_numpy as L
import reseg_gmm_numpy as G
from reseg_helpers import Dev
from clr_cases import identify_on_device as _identify, link_on_device as _link_on_device, upload as _upload
from test_link_clr import _hand_records

TH = cc.THRESHOLD
FINITE = [n for n in cc.NAMES if n != 'zeros']


# ------------------------------------------------------------------ not GPU: the exact statement by hand
def _tiny(n, f0, mu0=0.0, iv0=1.0):
    """K = 1: a record of n frames whose f is f0 in dimension 0, and a model that is mu0, 1 / iv0 there
    and 0, 1 elsewhere."""
    rec = np.zeros((1, L.BW_COMP))
    rec[0, 0], rec[0, 1] = n, f0
    ubm = np.zeros((1, G.COMP))
    ubm[0, G.MEAN], ubm[0, G.IVAR:G.NORM] = mu0, 1.0
    ubm[0, G.IVAR] = iv0
    return rec, ubm


def test_exact_values_checked_by_hand():
    # mu = 0, var = 1, r = 2.  a: n 2, f 2; b: n 6, f 4.  m_b = 4 / 8 = 1/2, m_a = 2 / 4 = 1/2.
    #   H(a|b) = (1/2) [1/2 * 2 - 1/2 * 2 * 1/4] = 3/8,  H(b|a) = (1/6) [1/2 * 4 - 1/2 * 6 * 1/4] = 5/24
    a, ubm = _tiny(2.0, 2.0)
    b, _ = _tiny(6.0, 4.0)
    assert X.map_means(b, ubm, 2.0)[0][:2] == [Fraction(1, 2), Fraction(0)]
    assert X.half(a, b, ubm, 2.0) == Fraction(3, 8) and X.half(b, a, ubm, 2.0) == Fraction(5, 24)
    assert X.clr(a, b, ubm, 2.0) == X.clr(b, a, ubm, 2.0) == Fraction(7, 12)
    assert X.clr(a, a, ubm, 2.0) == Fraction(3, 4) and X.total(b) == 6
    # mu = 1, var = 1/2, r = 1.  a: n 1, f 3; b: n 3, f 1.  m_b = 2 / 4 = 1/2, m_a = 4 / 2 = 2.
    #   H(a|b) = [(-1/2) 3 - 1/2 (1/4 - 1)] * 2 = -9/4,  H(b|a) = (1/3) [1 * 1 - 1/2 * 3 * (4 - 1)] * 2 = -7/3
    a2, ubm2 = _tiny(1.0, 3.0, 1.0, 2.0)
    b2, _ = _tiny(3.0, 1.0, 1.0, 2.0)
    assert X.map_means(a2, ubm2, 1.0)[0][0] == 2
    assert X.half(a2, b2, ubm2, 1.0) == Fraction(-9, 4) and X.half(b2, a2, ubm2, 1.0) == Fraction(-7, 3)
    assert X.clr(a2, b2, ubm2, 1.0) == Fraction(-55, 12)
    # the restatement gives the same where float64 can: -55/12 to an ulp or two
    assert abs(L.clr(a2, b2, ubm2, 1.0) + 55.0 / 12.0) < 1e-14
    # N = 0: not finite
    z, _ = _tiny(0.0, 0.0)
    assert X.clr(a, z, ubm, 2.0) is None and not X.matrix([a, z], [1, 1], ubm, 2.0)[1]
    # the chain on [a, b, a]: (0, 2) at 3/4 before (0, 1) at 7/12.  Merged: n 4, f 4, m = 4/6.
    #   H(M|b) = (1/4) [1/2 * 4 - 1/2 * 4 * 1/4] = 3/8,  H(b|M) = (1/6) [2/3 * 4 - 1/2 * 6 * 4/9] = 2/9
    recs, ok = [a, b, a], [1, 1, 1]
    merges, smax, smin, fin, mar = X.chain(recs, ok, ubm, 2.0, 0.75)           # d > threshold is strict
    assert merges == [] and fin and (smax, smin) == (Fraction(3, 4), Fraction(7, 12)) and mar.to_th == 0
    merges, _, _, _, mar = X.chain(recs, ok, ubm, 2.0, 0.7)
    assert merges == [(0, 2, Fraction(3, 4))] and mar.to_th == Fraction(3, 4) - Fraction(0.7) and mar.ties == 0
    assert mar.to_next == Fraction(3, 4) - Fraction(7, 12)
    merges = X.chain(recs, ok, ubm, 2.0, 0.7, max_spk=1)[0]
    assert merges == [(0, 2, Fraction(3, 4)), (0, 1, Fraction(43, 72))]
    assert X.labels_from_merges(3, merges) == [1, 1, 1] and X.labels_from_merges(3, merges[:1]) == [1, 2, 1]
    # ties: [b, a, a, a] -- (1, 2), (1, 3) and (2, 3) at 3/4: the first in row-major order; b not ok: it stays
    merges, _, _, _, mar = X.chain([b, a, a, a], [0, 1, 1, 1], ubm, 2.0, 0.7)
    assert merges[0] == (1, 2, Fraction(3, 4)) and mar.ties >= 1 and X.labels_from_merges(4, merges)[0] == 1
    # the merged record: the exact sum rounded once
    x, y = np.array([0.1, 1e16, -3.0]), np.array([0.2, 1.0, 3.0])
    assert X.merged(x, y).tobytes() == X.merged_rational(x, y).tobytes() == (x + y).tobytes()


def test_exact_assignment_checked_by_hand():
    """test_gallery's hand-written matrix, as rationals."""
    mat = [[Fraction(v) for v in row] for row in ([5.0, 1.0, -3.0], [4.0, 2.0, -2.0], [-1.0, -4.0, 0.5])]
    ok = [1, 1, 1]
    ident, score, second, mar = X.assign(mat, ok, ok, [0, 3], 0.0)
    assert ident == [0, 1, 2] and score == [5, 2, Fraction(1, 2)] and second == [1, 4, -1]
    assert (mar.to_th, mar.to_next) == (Fraction(1, 2), 1)               # gallery_numpy.margins says (0.5, 1.0)
    ident, score, second, _ = X.assign(mat, ok, ok, [0, 3], 3.0)
    assert ident == [0, -1, -1] and score == [5, 4, Fraction(1, 2)] and second == [1, 2, -1]
    for got in (X.assign(mat, ok, ok, [0, 3], 0.0, False), X.assign(mat, ok, ok, [0, 1, 2, 3], 0.0)):
        assert got[0] == [0, 0, 2] and got[1] == [5, 4, Fraction(1, 2)] and got[2] == [1, 2, -1]
    tie = [[Fraction(2)] * 2] * 2
    assert X.assign(tie, ok[:2], ok[:2], [0, 2], 0.0)[0] == [0, 1] and X.assign(tie, ok[:2], ok[:2], [0, 2], 0.0, False)[0] == [0, 0]
    ident, score, second, _ = X.assign(mat, [1, 0, 1], [0, 1, 1], [0, 3], -10.0)
    assert ident == [1, -1, 2] and score[1] is None and second[1] is None and second[0] == -3
    one = X.assign([row[:1] for row in mat], ok, ok[:1], [0, 3], 0.0)
    assert one[0] == [0, -1, -1] and one[1] == [5, 4, -1] and one[2] == [None] * 3


# ------------------------------------------------------------------ not GPU: the fixture
def test_fixture_is_reproduced_bit_for_bit():
    with open(cc.FIXTURE) as f:
        stored = f.read()
    assert cc.dump(cc.make_fixture()) == stored
    assert cc.fixture()['sha256'] == cc.sha256()
    assert len(stored) < 128 * 1024


def test_restatements_are_inside_their_tiers():
    fx = cc.fixture()['groups']
    for name in FINITE:
        e = fx[name]
        print('%-8s tier %s e %.3g |v|max %.3g' % (name, e['tier'], e['e'], e['vmax']))
        assert e['tier'] == cc.tier_of(e['e']) and e['tier'] in ('1e-9', '1e-5'), name
        assert e['e'] <= cc.TIER_BAR[e['tier']] / 8.0, name
        assert e['tier'] == ('1e-5' if name == 'off1024' else '1e-9'), name
        # the restatement takes the exact decisions: the log, the identities
        assert e['restated_log_same'], name
        ubm, rec, ok, r, _ = cc.build(name)
        pr, pok, off, gal, gok = cc.gallery_of(name)
        for key, exclusive in (('exclusive', True), ('free', False)):
            got = GN.identify(pr, pok, off, gal, gok, ubm, r, TH, exclusive)
            want = e['identify'][key]
            assert got[4] and got[0].tolist() == want['ident'], (name, key)
            for g, w in ((got[1], want['score']), (got[2], want['second'])):
                assert [v is None for v in w] == np.isnan(g).tolist(), (name, key)
                fin = [i for i, v in enumerate(w) if v is not None]
                assert cc.errors(g[fin], [float(w[i]) for i in fin])[0] <= e['e'], (name, key)
    # the error grows with the square of the offset: 64 sigma costs about four digits of the sixteen
    assert fx['off8']['e'] < fx['off64']['e'] < fx['off1024']['e'] and fx['off64']['e'] < 1e-11


def test_every_case_meets_its_own_condition():
    fx = cc.fixture()['groups']
    for name in FINITE:
        assert cc.conditions_hold(fx[name]), (name, fx[name]['chain_margins'])
    for g in cc.GROUPS:
        ubm, rec, ok, r, _ = cc.build(g['name'])
        sd = np.sqrt(1.0 / ubm[:, G.IVAR:G.NORM])
        z = ubm[:, G.MEAN:G.IVAR] / sd
        off = g.get('offset', 0.0)
        assert z.min() >= off - 5.0 and z.max() <= off + 5.0, g['name']
        assert rec.shape == (g['n'], g['K'], L.BW_COMP) and g['n'] <= 40
    assert sorted(set(g['K'] for g in cc.GROUPS)) == [1, 3, 5, 7, 8]
    # an offset of 0 is test_link_clr's generator to the bit
    for got, want in zip(cc.hand_records(107, 7, 3, 8), _hand_records(107, 7, 3, 8)):
        assert got.tobytes() == want.tobytes()
    # n_c exactly 0, in one record and in all: the adapted mean is the model's, exactly
    ubm, rec, _, r, _ = cc.build('nc0one')
    assert (rec[3, 2] == 0.0).all() and (rec[:, :, 0] > 0.0).sum() == rec.shape[0] * rec.shape[1] - 1
    assert X.map_means(rec[3], ubm, r)[2] == [Fraction(v) for v in ubm[2, G.MEAN:G.IVAR].tolist()]
    ubm, rec, _, r, _ = cc.build('nc0all')
    assert (rec[:, 2] == 0.0).all() and (np.delete(rec, 2, axis=1)[:, :, 0] > 0.0).all()
    # relevance far below and far above every n_c
    assert cc.build('r1e-3')[3] * 1e4 < cc.build('r1e-3')[1][:, :, 0].min()
    assert cc.build('r1e6')[3] > 1e3 * cc.build('r1e6')[1][:, :, 0].max()
    # one record a million times heavier
    rec = cc.build('heavy')[1]
    assert L.total(rec[0]) > 2.0e5 * max(L.total(x) for x in rec[1:])
    # the planted ties are ties in exact arithmetic and bit-equal in the restatement
    ubm, rec, ok, r, _ = cc.build('ties7')
    assert ok.tolist() == [1, 1, 1, 0, 1, 1, 1] and rec[1].tobytes() == rec[4].tobytes() == rec[5].tobytes()
    tie = [L.clr(rec[a], rec[b], ubm, r) for a, b in ((1, 4), (1, 5), (4, 5))]
    assert tie[0] == tie[1] == tie[2]
    assert X.clr(rec[1], rec[4], ubm, r) == X.clr(rec[1], rec[5], ubm, r) == X.clr(rec[4], rec[5], ubm, r)
    # (1, 4) of the three is the first in row-major order; 5 is position 4 after it
    assert fx['ties7']['chain_margins']['ties'] >= 1 and [m[:2] for m in fx['ties7']['merges'][:2]] == [[1, 4], [1, 4]]
    # an ok-flagged record of zeros: N = 0, the ratio is not finite, both restatements refuse the call
    ubm, rec, ok, r, _ = cc.build('zeros')
    assert ok[2] == 1 and (rec[2] == 0.0).all() and X.total(rec[2]) == 0 and not fx['zeros']['finite']
    assert not L.clr_link(rec, ok, ubm, r, TH)[3] and not np.isfinite(L.clr(rec[0], rec[2], ubm, r))


# ------------------------------------------------------------------ not GPU: the fast restatement
def _same_margins(fast, slow_th, slow_next):
    assert abs(fast['to_threshold'] - slow_th) <= 1e-12 or fast['to_threshold'] == slow_th
    assert fast['ties'] or abs(fast['to_next'] - slow_next) <= 1e-12 or fast['to_next'] == slow_next


def test_fast_chain_is_the_loop_on_the_small_fixtures():
    """test_link_clr.test_chain_matches_the_restatement's fixtures, every variant of them."""
    K, r = 8, 16.0
    runs = 0
    for n in (1, 2, 7, 40):
        ubm, rec, _ = _hand_records(100 + n, n, 1 if n == 2 else 3 if n == 7 else 5, K)
        ok = np.ones(n, dtype=np.int32)
        variants = [(ok, TH, 0)]
        if n == 7:
            rec[5] = rec[4] = rec[1]
            ok[3] = 0
        if n == 40:
            ok2 = ok.copy()
            ok2[[0, 17, 39]] = 0
            variants += [(ok, TH, 3), (ok, 1e9, 0), (ok, -1e9, 0), (ok2, TH, 6)]
        for good, th, max_spk in variants:
            want = L.clr_link(rec, good, ubm, r, th, max_spk)
            got = F.clr_link(rec, good, ubm, r, th, max_spk)
            assert got[3] and want[3]
            assert [(a, b) for a, b, _ in got[0]] == [(a, b) for a, b, _ in want[0]], (n, th, max_spk)
            assert np.allclose([d for _, _, d in got[0]], [d for _, _, d in want[0]], rtol=0.0, atol=1e-12)
            if n == 1:
                assert np.isnan(got[1]) and np.isnan(want[1]) and got[0] == []
            else:
                assert abs(got[1] - want[1]) <= 1e-12 and abs(got[2] - want[2]) <= 1e-12
            assert (got[4]['ties'] > 0) == (n == 7)
            runs += 1
    assert runs == 8
    # the small groups as well, against the exact log and its margins
    fx = cc.fixture()['groups']
    for name in FINITE:
        ubm, rec, ok, r, _ = cc.build(name)
        got = F.clr_link(rec, ok, ubm, r, TH)
        e = fx[name]
        assert [[a, b] for a, b, _ in got[0]] == [m[:2] for m in e['merges']], name
        assert cc.errors([d for _, _, d in got[0]], [float(m[2]) for m in e['merges']])[0] <= 4.0 * cc.unit_of(e), name
        assert got[4]['ties'] == e['chain_margins']['ties'], name
        assert abs(got[4]['to_next'] - e['chain_margins']['to_next']) <= 8.0 * cc.unit_of(e), name
        assert abs(got[4]['to_threshold'] - e['chain_margins']['to_threshold']) <= 8.0 * cc.unit_of(e), name
    # a record that is not finite, a record of zeros, nothing at all
    ubm, rec, ok, r, _ = cc.build('zeros')
    assert not F.clr_link(rec, ok, ubm, r, TH)[3]
    none = F.clr_link(rec[:0], ok[:0], ubm, r, TH)
    assert none[0] == [] and np.isnan(none[1]) and np.isnan(none[2]) and none[3]


def _gallery_fixtures():
    """(probes, pok, off, gallery, gok, ubm, th, ties) of test_gallery's device tests."""
    out = []
    for K in (1, 3, 8):
        S, Gn = 37, 19
        ubm, rec, _ = _hand_records(300 + K, S + Gn, 10, K)
        pok, gok = np.ones(S, dtype=np.int32), np.ones(Gn, dtype=np.int32)
        pok[[4, 30]] = 0
        gok[[0, 11]] = 0
        off = np.cumsum([0, 1, 2, 5, 13, 16])
        for th in (TH, 1e9, -1e9):
            out.append((rec[:S], pok, off, rec[S:], gok, ubm, th, False))
        out.append((rec[:S], pok, off, rec[S + 1:S + 2], gok[1:2], ubm, TH, False))
        out.append((rec[:S], pok, off, rec[S:S], gok[:0], ubm, TH, False))
    ubm, rec, _ = _hand_records(41, 200, 90, 8)
    gok = np.ones(130, dtype=np.int32)
    gok[[64, 129]] = 0
    out.append((rec[:70], np.ones(70, dtype=np.int32), [0, 70], rec[70:], gok, ubm, TH, False))
    ubm, rec, who = _hand_records(77, 40, 4, 8)
    of = lambda p, k: np.nonzero(who == p)[0][:k]
    p0 = of(0, 2)
    gal = np.array([rec[of(1, 1)[0]], rec[of(2, 1)[0]], rec[p0[0]], rec[of(3, 1)[0]], rec[of(1, 2)[1]], rec[p0[0]]])
    probes = np.array([rec[p0[1]], rec[p0[1]], rec[of(3, 2)[1]]])
    for off in ([0, 3], [0, 1, 2, 3]):
        out.append((probes, np.ones(3, dtype=np.int32), off, gal, np.ones(6, dtype=np.int32), ubm, TH, True))
    return out


def test_fast_assignment_is_the_loop_on_the_small_fixtures():
    r = 16.0
    for probes, pok, off, gal, gok, ubm, th, ties in _gallery_fixtures():
        for exclusive in (True, False):
            want = GN.identify(probes, pok, off, gal, gok, ubm, r, th, exclusive)
            got = F.identify(probes, pok, off, gal, gok, ubm, r, th, exclusive)
            assert got[4] and want[4]
            assert np.array_equal(np.isnan(got[3]), np.isnan(want[3]))
            assert np.allclose(got[3], want[3], rtol=0.0, atol=1e-12, equal_nan=True)
            if ties:
                # the planted ties are bit-equal in the matrix product as well
                assert got[3][0, 2] == got[3][0, 5] == got[3][1, 2] == got[3][1, 5] and got[5]['ties'] >= 1
            assert got[0].tolist() == want[0].tolist(), (len(gal), th, exclusive)
            for g, w in ((got[1], want[1]), (got[2], want[2])):
                assert np.array_equal(np.isnan(g), np.isnan(w)) and np.allclose(g, w, rtol=0.0, atol=1e-12, equal_nan=True)
            if not ties and len(gal):
                _same_margins(got[5], *GN.margins(want[3], pok, gok, off, th, exclusive))
    # test_gallery's hand-written matrix
    mat = np.array([[5.0, 1.0, -3.0], [4.0, 2.0, -2.0], [-1.0, -4.0, 0.5]])
    ok = np.ones(3, dtype=np.int32)
    for args in (([0, 3], 0.0, True), ([0, 3], 3.0, True), ([0, 3], 0.0, False), ([0, 1, 2, 3], 0.0, True)):
        want, got = GN.assign(mat, ok, ok, *args), F.assign(mat, ok, ok, *args)
        assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got[:3], want))
    assert (F.assign(mat, ok, ok, [0, 3], 0.0)[3]['to_threshold'], F.assign(mat, ok, ok, [0, 3], 0.0)[3]['to_next']) == (0.5, 1.0)
    got = F.assign(mat, [1, 0, 1], [0, 1, 1], [0, 3], -10.0)
    assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got[:3], GN.assign(mat, [1, 0, 1], [0, 1, 1], [0, 3], -10.0)))
    # the small groups, against the exact identities
    fx = cc.fixture()['groups']
    for name in FINITE:
        ubm, rec, ok, r, _ = cc.build(name)
        pr, pok, off, gal, gok = cc.gallery_of(name)
        for key, exclusive in (('exclusive', True), ('free', False)):
            assert F.identify(pr, pok, off, gal, gok, ubm, r, TH, exclusive)[0].tolist() == fx[name]['identify'][key]['ident'], name


# ------------------------------------------------------------------ not GPU: the large cases
R_LARGE = 16.0
MAX_SPK_1100 = 250


@functools.lru_cache(maxsize=None)
def _large_chain(name, max_spk=0):
    """clr_fast_numpy's chain of a large case, computed once and shared."""
    ubm, rec, ok, _ = cc.large(name)
    return F.clr_link(rec, ok, ubm, R_LARGE, TH, max_spk)


def _gallery_large():
    ubm, rec, _, _ = cc.large('g1100x600')
    pok, gok = np.ones(1100, dtype=np.int32), np.ones(600, dtype=np.int32)
    pok[list(cc.NOT_OK_PROBES)] = 0
    gok[list(cc.NOT_OK_GALLERY)] = 0
    return ubm, rec[:1100], pok, rec[1100:], gok


@functools.lru_cache(maxsize=None)
def _large_identify(ragged, exclusive):
    ubm, pr, pok, gal, gok = _gallery_large()
    off = list(cc.RAGGED) if ragged else [0, 1100]
    return F.identify(pr, pok, off, gal, gok, ubm, R_LARGE, TH, exclusive)


def _slots_of(n, merges):
    """The log replayed on the initial indices: per merge (the members of a, the members of b)."""
    groups = [[i] for i in range(n)]
    out = []
    for a, b, _ in merges:
        out.append((list(groups[a]), list(groups[b])))
        groups[a].extend(groups.pop(b))
    return out


CHAINS = ['c65k3', 'c65k5', 'c130k3', 'c130k5', 'c1100', 'c4096']


def test_large_cases_keep_their_margins():
    """The condition of the large cases, on the reference alone: every decision at least MARGIN_FLOOR
    from its threshold and from the best pair of a lower value (float64's own error is 1e-14), and
    each case reaches what it is there for."""
    t0 = time.time()
    for name in CHAINS:
        for max_spk in ((0, MAX_SPK_1100) if name == 'c1100' else (0,)):
            merges, smax, smin, fin, mar = _large_chain(name, max_spk)
            print('%s max_spk %d: %d merges, margins %s' % (name, max_spk, len(merges), mar))
            assert fin and mar['to_threshold'] >= cc.MARGIN_FLOOR and mar['to_next'] >= cc.MARGIN_FLOOR, name
            assert (mar['ties'] > 0) == (name in ('c130k3', 'c130k5', 'c4096')), name
    n = 1100
    assert len(_large_chain('c1100')[0]) > 700 and len(_large_chain('c1100', MAX_SPK_1100)[0]) == n - MAX_SPK_1100
    assert _large_chain('c1100', MAX_SPK_1100)[0][-1][2] <= TH < _large_chain('c1100')[0][-1][2]
    # n = 4 096: few merges, positions above 1 023 in the log, speakers that are not ok among them
    merges = _large_chain('c4096')[0]
    ubm, rec, ok, _ = cc.large('c4096')
    assert 20 <= len(merges) <= 60 and sum(1 for a, b, _ in merges if b > 1023) >= 10 and any(a > 1023 for a, b, _ in merges)
    assert ok.sum() == 4096 - len(cc.NOT_OK_4096) and sum(1 for s in cc.NOT_OK_4096 if s >= 1024) >= 3
    labels = L.labels_from_merges(4096, merges)
    assert all((labels == labels[s]).sum() == 1 for s in cc.NOT_OK_4096)
    # the planted ties: five identical records at i, j, j + 64, i + 1 024 and beyond; of the ten bit-equal
    # pairs (i, j) is the first in row-major order, and it is what the reference merges first of them
    i, j, j64, i1024, last = cc.TIE_4096
    assert (j64, i1024) == (j + 64, i + 1024) and all(rec[s].tobytes() == rec[i].tobytes() for s in cc.TIE_4096)
    T, N = F.derive(rec[list(cc.TIE_4096)], ubm, R_LARGE)
    tie = F.square(rec[list(cc.TIE_4096)], T, N)
    assert len(set(tie[np.triu_indices(5, 1)].tolist())) == 1
    first = [m for m in _slots_of(4096, merges) if set(m[0] + m[1]) & set(cc.TIE_4096)][0]
    assert first == ([i], [j])
    for name in ('c130k3', 'c130k5'):
        i, j, j64 = cc.TIE_130
        rec = cc.large(name)[1]
        assert j64 == j + 64 and rec[i].tobytes() == rec[j].tobytes() == rec[j64].tobytes()
        first = [m for m in _slots_of(130, _large_chain(name)[0]) if set(m[0] + m[1]) & set(cc.TIE_130)][0]
        assert first == ([i], [j])
    # the gallery: three column tiles, the last one partial; identities that are not ok at a tile's edge
    assert 600 == 2 * 256 + 88 and set(cc.NOT_OK_GALLERY) == {255, 256, 599}
    sizes = np.diff(cc.RAGGED).tolist()
    assert sizes.count(1) >= 2 and 1030 in sizes and sum(sizes) == 1100
    for ragged in (False, True):
        for exclusive in (True, False):
            ident, score, second, mat, fin, mar = _large_identify(ragged, exclusive)
            known = ident[ident >= 0]
            print('gallery ragged %d exclusive %d: %d known, margins %s' % (ragged, exclusive, len(known), mar))
            assert fin and mar['to_threshold'] >= cc.MARGIN_FLOOR and mar['to_next'] >= cc.MARGIN_FLOOR and mar['ties'] == 0
            assert len(known) > 200 and (known > 512).any() and (ident[np.asarray(_gallery_large()[2]) != 0] < 0).any()
            assert not set(known.tolist()) & set(cc.NOT_OK_GALLERY)
            if exclusive and not ragged:
                assert len(set(known.tolist())) == len(known)
    # exclusive and free differ, one group and ragged groups differ: the constraint bites at this size
    assert _large_identify(False, True)[0].tolist() != _large_identify(False, False)[0].tolist()
    assert _large_identify(False, True)[0].tolist() != _large_identify(True, True)[0].tolist()
    took = time.time() - t0
    print('the large references: %.1f s' % took)
    assert took < 30.0


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def dev():
    d = Dev(np.zeros((64, G.DIM), dtype=np.float32))
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', FINITE)
def test_small_group_values_and_decisions_are_the_exact_ones(dev, name):
    """clr_cases.check_group asserts the decisions and the bit-equalities; here every value's row."""
    e = cc.fixture()['groups'][name]
    rows = cc.check_group(dev, name)
    worst = max(rows, key=lambda q: q['quotient'])
    print('%-8s K %d tier %s e %.3g: largest quotient %.3g (%s), device error %.3g' % (
        name, len(cc.build(name)[0]), e['tier'], e['e'], worst['quotient'], worst['what'], max(q['dev'] for q in rows)))
    for q in rows:
        cc.assert_row(q)


@pytest.mark.gpu
def test_an_ok_record_of_zeros_is_refused(dev):
    ubm, rec, ok, r, _ = cc.build('zeros')
    hipabi = dev.hipabi
    link = _link_on_device(dev, ubm, rec, ok, r, TH)
    assert link['status'] == hipabi.SPKD_ENONFINITE and link['n_merges'] == 0
    pr, pok, off, gal, gok = cc.gallery_of('zeros')
    got, _ = _identify(dev, ubm, pr, pok, off, gal, gok, r, TH)
    assert got['status'] == hipabi.SPKD_ENONFINITE and (got['ident'] == -1).all() and np.isnan(got['score']).all()
    # flagged not ok, it is left alone
    ok2 = ok.copy()
    ok2[2] = 0
    want = L.clr_link(rec, ok2, ubm, r, TH)
    link = _link_on_device(dev, ubm, rec, ok2, r, TH)
    assert link['status'] == 0 and list(zip(link['a'].tolist(), link['b'].tolist())) == [(a, b) for a, b, _ in want[0]]


def _bound(K):
    """What a device value may differ by from the float64 one at the large sizes: MARGIN units of the
    small group of the same generator and K."""
    return cc.MARGIN * cc.unit_of(cc.fixture()['groups']['k%d' % K])


def _check_chain(dev, name, max_spk=0):
    ubm, rec, ok, _ = cc.large(name)
    want = _large_chain(name, max_spk)
    t0 = time.time()
    got = _link_on_device(dev, ubm, rec, ok, R_LARGE, TH, max_spk)
    took = time.time() - t0
    assert got['status'] == 0 and want[3]
    assert list(zip(got['a'].tolist(), got['b'].tolist())) == [(a, b) for a, b, _ in want[0]]
    err = cc.errors(list(got['d']) + [got['stat_max'], got['stat_min']], [d for _, _, d in want[0]] + [want[1], want[2]])[0]
    print('%s max_spk %d: %d merges in %.2f s (the chain: %.1f ms), largest |d - float64| %.3g, bound %.3g' % (
        name, max_spk, got['n_merges'], took, dev.ctx.last_ms('clr_link'), err, _bound(len(ubm))))
    assert err <= _bound(len(ubm))
    n = len(rec)
    assert dev.hipabi.labels_from_merges(n, got['a'], got['b']).tolist() == L.labels_from_merges(n, want[0]).tolist()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['c65k3', 'c65k5', 'c130k3', 'c130k5'])
def test_chain_past_a_wave_of_partners_at_an_odd_k(dev, name):
    got = _check_chain(dev, name)
    if name.startswith('c130'):
        # the tie between (i, j) and (i, j + 64) -- one lane of the row scan, two turns of its loop
        i, j, _ = cc.TIE_130
        first = [m for m in _slots_of(130, list(zip(got['a'], got['b'], got['d']))) if set(m[0] + m[1]) & set(cc.TIE_130)][0]
        assert first == ([i], [j])


@pytest.mark.gpu
def test_chain_of_1100_to_the_threshold_and_to_max_spk(dev):
    assert _check_chain(dev, 'c1100')['n_merges'] > 700
    assert _check_chain(dev, 'c1100', MAX_SPK_1100)['n_merges'] == 1100 - MAX_SPK_1100


@pytest.mark.gpu
def test_chain_of_4096_logs_positions_above_1023(dev):
    got = _check_chain(dev, 'c4096')
    assert (got['b'] > 1023).sum() >= 10
    i, j = cc.TIE_4096[:2]
    first = [m for m in _slots_of(4096, list(zip(got['a'], got['b'], got['d']))) if set(m[0] + m[1]) & set(cc.TIE_4096)][0]
    assert first == ([i], [j])


@pytest.mark.gpu
@pytest.mark.parametrize('ragged', [False, True])
def test_gallery_of_1100_probes_and_600_identities(dev, ragged):
    ubm, pr, pok, gal, gok = _gallery_large()
    off = list(cc.RAGGED) if ragged else [0, 1100]
    bound = _bound(len(ubm))
    for exclusive in (True, False):
        ident, score, second, wmat, fin, _ = _large_identify(ragged, exclusive)
        got, mat = _identify(dev, ubm, pr, pok, off, gal, gok, R_LARGE, TH, exclusive)
        assert got['status'] == 0 and np.array_equal(np.isnan(mat), np.isnan(wmat))
        assert np.isnan(mat[:, list(cc.NOT_OK_GALLERY)]).all() and np.isnan(mat[list(cc.NOT_OK_PROBES)]).all()
        errs = [cc.errors(mat[~np.isnan(wmat)], wmat[~np.isnan(wmat)])[0]]
        assert got['ident'].tolist() == ident.tolist()
        for g, w in ((got['score'], score), (got['second'], second)):
            assert np.array_equal(np.isnan(g), np.isnan(w))
            errs.append(cc.errors(g[~np.isnan(w)], w[~np.isnan(w)])[0])
        print('ragged %d exclusive %d: %d known; largest |device - float64| of matrix, score, second: %s, bound %.3g; '
              'scores %.2f ms, assignment %.2f ms' % (ragged, exclusive, (got['ident'] >= 0).sum(),
                                                       ', '.join('%.3g' % v for v in errs), bound,
                                                       dev.ctx.last_ms('ident_scores'), dev.ctx.last_ms('ident_assign')))
        assert max(errs) <= bound
        # a reported score is an entry of the matrix, to the bit
        known = np.nonzero(got['ident'] >= 0)[0]
        assert np.array_equal(got['score'][known], mat[known, got['ident'][known]])


@pytest.mark.gpu
def test_a_thousand_members_into_a_kept_slot_to_the_bit(dev):
    ubm, rec, _, _ = cc.large('acc1000')
    K = len(ubm)
    src = rec[1:] * 10.0 ** np.random.default_rng(5).integers(-3, 4, (1000, K, L.BW_COMP))
    dst = np.stack([rec[0], rec[0] * 0.5, rec[0] * 3.0])
    member = np.random.default_rng(6).permutation(1000)
    set_off, slots, keep = [0, 1000, 1000], [1, 2], [1, 0]
    d_src, d_dst = _upload(dev, src), _upload(dev, dst)
    dev.ctx.bw_accumulate(d_src, len(src), K, set_off, member, slots, keep, d_dst, len(dst))
    got = np.empty_like(dst)
    dev.ctx.d2h(got, d_dst)
    want = GN.bw_accumulate(src, set_off, member, slots, keep, dst)
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(got[0], dst[0]) and (got[2] == 0.0).all() and not np.array_equal(got[1], dst[1])
    # the order matters at this length: the same members in ascending order give other bits
    assert GN.bw_accumulate(src, set_off, np.arange(1000), slots, keep, dst).tobytes() != want.tobytes()
