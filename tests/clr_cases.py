"""Records and background models for the CLR chain and the gallery, and what is asked of them -- TEST
INFRASTRUCTURE ONLY.

test_link_clr.py's and test_gallery.py's hand records put the UBM's means at N(0, 1) and every n_c at
50 .. 500: the friendliest place for clr_derive's 0.5 (m^2 - mu^2) / var and (m - mu) / var, whose dot
product with a record cancels f (m - mu) against n / 2 (m^2 - mu^2).  The groups below leave it;
tests/exact_clr.py says what comes out in exact arithmetic; tests/golden/clr_exact.json stores that
(made by tests/golden/make_golden_clr.py, reproduced and held to its conditions by the CPU tests of
tests/test_clr_exact.py, asked of the device by its GPU tests).

Every value comes from numpy.random.default_rng(seed) in the order of test_link_clr._hand_records (an
offset of 0 gives that function's arrays bit for bit); nothing comes from synth.

groups (n records, K components, the UBM's means offset by `offset` sigma in every dimension)
  k1 k3 k5 k7 k8   every K whose E = 40 K is and is not a multiple of the 16 lanes of a pair; k8 has 40
                   records (the sample whose e bounds the large chains), the others 12.
  off8 off64 off1024
                   K = 8, the UBM's means 8, 64 and 1 024 sigma from the origin: the restatement loses
                   digits with the square of the offset.
  nc0one           K = 5, component 2 of record 3 is all zero: n_c = 0, m_c = mu_c, exactly.
  nc0all           K = 5, component 2 of EVERY record is all zero: a UBM component nobody's frame chose.
  r1e-3 r1e6       K = 3, relevance far below and far above the n_c (16 everywhere else).
  heavy            K = 8, record 0 times 1e6: a long-lived identity after many spkd_bw_accumulate.
  ties7            test_link_clr's n = 7: records 1, 4 and 5 identical, speaker 3 not ok.
  zeros            K = 3, record 2 all zero but flagged ok: N = 0, the ratio is 0 / 0, SPKD_ENONFINITE.

Each group is also a gallery problem: the first half of its records are the probes, one exclusive
group, the rest are the identities.

seeds: every seed below is the first tried; none was replaced.

large sizes (large()): the same generator at n up to 4 096; the reference there is tests/clr_fast_numpy.py,
and the seeds are the first for which that reference keeps every margin >= MARGIN_FLOOR (LARGE says
which were tried before; none was).
  c65k3 c65k5 c130k3 c130k5   65 and 130 records at K = 3 and 5: more partners than the 64 groups of the
                   recompute loop, more than a wave of columns right of a row, E = 120 and 200.  In c130*
                   records TIE_130 = (i, j, j + 64) are identical: (i, j), (i, j + 64) and (j, j + 64) tie to
                   the bit, and columns j and j + 64 of row i meet in one lane of the row scan.
  c1100            300 people: about 800 merges, to the threshold and to max_spk.
  c4096            strangers but for PAIRS_4096 pairs of one person each: few merges, positions above 1 023,
                   NOT_OK_4096 not ok.  Records TIE_4096 = (i, j, j + 64, i + 1 024, one more) are identical:
                   ten pairs tie to the bit, rows i and i + 1 024 meet in one thread of the arg-max.
  g1100x600        1 100 probes and 600 identities of 900 people: three column tiles of 256, the last partial.
  acc1000          1 001 records of K = 3 for spkd_bw_accumulate.
"""
import hashlib
import json
import math
import os

import numpy as np

import exact_clr as X
import gallery_numpy as GN
import link_clr_numpy as L
import reseg_gmm_numpy as G
from conditioned_cases import TIER_BAR, tier_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'clr_exact.json')
THRESHOLD = -0.5
EPS = 2.0 ** -52
MARGIN = 64.0                # the kernel is no worse than its formulation: 64 max(e, 2^-52 |value|max)
MARGIN_FLOOR = 1.0e-9        # what every decision of a case keeps from its threshold and its runner-up

GROUPS = [
    dict(name='k1', seed=9101, n=12, people=3, K=1),
    dict(name='k3', seed=9103, n=12, people=3, K=3),
    dict(name='k5', seed=9105, n=12, people=3, K=5),
    dict(name='k7', seed=9107, n=12, people=3, K=7),
    dict(name='k8', seed=9108, n=40, people=5, K=8),
    dict(name='off8', seed=9208, n=12, people=3, K=8, offset=8.0),
    dict(name='off64', seed=9264, n=12, people=3, K=8, offset=64.0),
    dict(name='off1024', seed=9299, n=12, people=3, K=8, offset=1024.0),
    dict(name='nc0one', seed=9301, n=12, people=3, K=5, special='nc0one'),
    dict(name='nc0all', seed=9302, n=12, people=3, K=5, special='nc0all'),
    dict(name='r1e-3', seed=9401, n=12, people=3, K=3, r=1.0e-3),
    dict(name='r1e6', seed=9402, n=12, people=3, K=3, r=1.0e6),
    dict(name='heavy', seed=9501, n=12, people=3, K=8, special='heavy'),
    dict(name='ties7', seed=107, n=7, people=3, K=8, special='ties7'),
    dict(name='zeros', seed=9601, n=6, people=2, K=3, special='zeros'),
]
NAMES = [g['name'] for g in GROUPS]


def hand_records(seed, n, n_people, K, offset=0.0, who=None):
    """test_link_clr._hand_records with the model's means moved by `offset` sigma: (ubm [K, 80],
    records [n, K, 40], the person of each record).  who: the persons, in place of the drawn ones."""
    rng = np.random.default_rng(seed)
    ubm = np.zeros((K, G.COMP))
    ubm[:, 0] = np.log(1.0 / K)
    ubm[:, G.MEAN:G.IVAR] = rng.normal(0.0, 1.0, (K, G.DIM))
    ubm[:, G.IVAR:G.NORM] = 1.0 / rng.uniform(0.5, 2.0, (K, G.DIM))
    ubm[:, G.NORM] = -0.5 * (G.DIM * G.LN_2PI - np.log(ubm[:, G.IVAR:G.NORM]).sum(axis=1))
    sd = np.sqrt(1.0 / ubm[:, G.IVAR:G.NORM])
    if offset:
        ubm[:, G.MEAN:G.IVAR] += offset * sd
    shift = rng.normal(0.0, 0.3, (n_people, K, G.DIM)) * sd
    drawn = rng.integers(0, n_people, n)
    who = drawn if who is None else np.asarray(who)
    rec = np.zeros((n, K, L.BW_COMP))
    rec[:, :, 0] = rng.uniform(50.0, 500.0, (n, K))
    mean = ubm[None, :, G.MEAN:G.IVAR] + shift[who] + rng.normal(0.0, 0.03, (n, K, G.DIM)) * sd
    rec[:, :, 1:] = rec[:, :, :1] * mean
    return ubm, rec, who


_BUILT = {}


def build(name):
    """(ubm, records, ok, relevance, who) of a group; the arrays are read-only."""
    if name not in _BUILT:
        g = GROUPS[NAMES.index(name)]
        ubm, rec, who = hand_records(g['seed'], g['n'], g['people'], g['K'], g.get('offset', 0.0))
        ok = np.ones(g['n'], dtype=np.int32)
        special = g.get('special')
        if special == 'nc0one':
            rec[3, 2] = 0.0
        elif special == 'nc0all':
            rec[:, 2] = 0.0
        elif special == 'heavy':
            rec[0] *= 1.0e6
        elif special == 'ties7':
            rec[5] = rec[4] = rec[1]
            ok[3] = 0
        elif special == 'zeros':
            rec[2] = 0.0
        for a in (ubm, rec, ok, who):
            a.setflags(write=False)
        _BUILT[name] = (ubm, rec, ok, float(g.get('r', 16.0)), who)
    return _BUILT[name]


def gallery_of(name):
    """The group as a gallery problem: (probes, probe ok, group offsets, identities, their ok)."""
    _, rec, ok, _, _ = build(name)
    s = len(rec) // 2
    return rec[:s], ok[:s], [0, s], rec[s:], ok[s:]


def sha256():
    h = hashlib.sha256()
    for name in NAMES:
        ubm, rec, ok, r, _ = build(name)
        for a in (ubm, rec):
            h.update(np.ascontiguousarray(a, dtype='<f8').tobytes())
        h.update(np.ascontiguousarray(ok, dtype='<i4').tobytes())
        h.update(np.array([r], dtype='<f8').tobytes())
    return h.hexdigest()


def fmt(v):
    return None if v is None else '%.17g' % float(v)


def errors(got, want):
    """(largest |got - want|, the largest in the suite's measure |a - b| / max(1, |a|, |b|), largest |want|)."""
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    if not len(want):
        return 0.0, 0.0, 0.0
    if not np.isfinite(got).all():
        return math.inf, math.inf, float(np.abs(want).max())
    d = np.abs(got - want)
    return float(d.max()), float((d / np.maximum(1.0, np.maximum(np.abs(got), np.abs(want)))).max()), float(np.abs(want).max())


def replay(rec, ok, merges):
    """The records and ok flags after the merges of a log, in float64 (record[a] += record[b]; pop(b))."""
    recs, good = [np.array(x) for x in rec], list(ok)
    for a, b in merges:
        recs[a] = recs[a] + recs.pop(b)
        good.pop(b)
    return np.array(recs), np.array(good, dtype=np.int32)


def compute_group(name):
    """The fixture entry of a group: the exact values rounded once to float64 as 17-digit decimals, the
    exact decisions, their margins, and e, the scale and the tier of the float64 restatement."""
    ubm, rec, ok, r, _ = build(name)
    n = len(rec)
    mat, fin = X.matrix(rec, ok, ubm, r)
    out = {'finite': bool(fin)}
    if not fin:
        # the restatement agrees that the call is refused
        assert not L.clr_link(rec, ok, ubm, r, THRESHOLD)[3]
        pr, pok, off, gal, gok = gallery_of(name)
        assert not GN.identify(pr, pok, off, gal, gok, ubm, r, THRESHOLD)[4] and not X.scores(pr, pok, gal, gok, ubm, r)[1]
        return out
    pairs = sorted(mat)
    out['clr'] = [[a, b, fmt(mat[(a, b)])] for a, b in pairs]
    merges, smax, smin, cfin, mar = X.chain(rec, ok, ubm, r, THRESHOLD)
    assert cfin
    out['merges'] = [[a, b, fmt(d)] for a, b, d in merges]
    out['labels'] = X.labels_from_merges(n, merges)
    out['stat_max'], out['stat_min'] = fmt(smax), fmt(smin)
    out['chain_margins'] = mar.floats()
    # the float64 restatement on the same pairs and along the same log
    want = [float(mat[p]) for p in pairs] + [float(d) for _, _, d in merges]
    rest = [L.clr(rec[a], rec[b], ubm, r) for a, b in pairs]
    rlog = L.clr_link(rec, ok, ubm, r, THRESHOLD)
    out['restated_log_same'] = [(a, b) for a, b, _ in rlog[0]] == [(a, b) for a, b, _ in merges]
    if out['restated_log_same']:
        rest += [d for _, _, d in rlog[0]]
    else:
        want = want[:len(pairs)]
    pr, pok, off, gal, gok = gallery_of(name)
    smat, sfin = X.scores(pr, pok, gal, gok, ubm, r)
    assert sfin
    gmat = GN.scores(pr, pok, gal, gok, ubm, r)[0]
    s = len(pr)
    for i in range(s):
        for j in range(len(gal)):
            if smat[i][j] is not None:
                assert smat[i][j] == mat[(i, s + j)]                   # the same pair, the same rational
                want.append(float(smat[i][j]))
                rest.append(gmat[i, j])
    e, rel, vmax = errors(rest, want)
    assert rel <= e
    out['e'], out['vmax'], out['tier'] = e, vmax, tier_of(e)      # (e bounds the suite's measure from above)
    out['identify'] = {}
    for key, exclusive in (('exclusive', True), ('free', False)):
        ident, score, second, imar = X.assign(smat, pok, gok, off, THRESHOLD, exclusive)
        out['identify'][key] = {'ident': ident, 'score': [fmt(v) for v in score], 'second': [fmt(v) for v in second],
                                'margins': imar.floats()}
    return out


def make_fixture():
    fx = {'env': {'numpy': np.__version__,
                  'note': 'reference: tests/exact_clr.py in rationals, each value rounded once to float64; e and tiers: '
                          'tests/link_clr_numpy.py and tests/gallery_numpy.py in float64; made by '
                          'tests/golden/make_golden_clr.py'},
          'sha256': sha256(), 'threshold': THRESHOLD, 'groups': {}}
    for name in NAMES:
        fx['groups'][name] = compute_group(name)
    return fx


def dump(fx):
    return json.dumps(fx, indent=None, separators=(',', ':'), sort_keys=True) + '\n'


def save(fx):
    with open(FIXTURE, 'w') as f:
        f.write(dump(fx))


_FIXTURE = []


def fixture():
    if not _FIXTURE:
        with open(FIXTURE) as f:
            _FIXTURE.append(json.load(f))
        assert _FIXTURE[0]['sha256'] == sha256(), 'the CLR records are not reproducible here'
    return _FIXTURE[0]


def unit_of(entry):
    """What a device error is measured in: max(e, 2^-52 |value|max)."""
    return max(entry['e'], EPS * entry['vmax'])


def conditions_hold(entry):
    """The fixture's condition on a finite group: every decision of the exact chain and of the exact
    assignment keeps MARGIN_FLOOR, and twice the device's allowance, from its threshold and from the
    best pair of a lower value."""
    need = max(MARGIN_FLOOR, 2.0 * MARGIN * unit_of(entry))
    ms = [entry['chain_margins']] + [v['margins'] for v in entry['identify'].values()]
    return all(m['to_threshold'] >= need and m['to_next'] >= need for m in ms)


def device_row(case, what, entry, got, want):
    """One row of the comparison of device values with the exact ones: the device's errors, and the
    quotient error / max(e, 2^-52 |value|max) that MARGIN bounds."""
    err, rel, _ = errors(got, want)
    unit = unit_of(entry)
    return {'case': case, 'what': what, 'tier': entry['tier'], 'scale': entry['vmax'], 'e': entry['e'], 'dev': err,
            'dev_rel': rel, 'quotient': err / unit if unit > 0.0 else (0.0 if err == 0.0 else math.inf)}


def assert_row(r):
    assert r['tier'] != 'outside', r
    assert r['dev_rel'] <= TIER_BAR[r['tier']], r
    assert r['quotient'] <= MARGIN, r


# ---------------------------------------------------------------------- the large sizes
# name: (seed, n, people, K, seeds tried before it).  `people` >= n: mostly strangers.
LARGE = {
    'c65k3': (9703, 65, 12, 3, ()), 'c65k5': (9705, 65, 12, 5, ()),
    'c130k3': (9713, 130, 20, 3, ()), 'c130k5': (9715, 130, 20, 5, ()),
    'c1100': (9721, 1100, 300, 8, ()),
    'c4096': (9731, 4096, 4096, 8, ()),
    'g1100x600': (9741, 1700, 900, 8, ()),
    'acc1000': (9751, 1001, 1, 3, ()),
}
PAIRS_4096 = 40
NOT_OK_4096 = (5, 1023, 1024, 1500, 2049, 4095)
TIE_4096 = (7, 100, 164, 1031, 3000)        # i, j, j + 64, i + 1 024 and one more: five identical records
TIE_130 = (3, 20, 84)                       # i, j, j + 64
NOT_OK_GALLERY = (255, 256, 599)
NOT_OK_PROBES = (0, 63, 1024, 1099)
RAGGED = (0, 1, 1, 2, 1032, 1040, 1099, 1100)   # groups of 1, 0, 1, 1 030, 8, 59 and 1 probes


def large(name):
    """(ubm, records, ok, who) of a large case; ties planted as the module's text says."""
    if ('large', name) not in _BUILT:
        seed, n, people, K, _ = LARGE[name]
        who = None
        if name == 'c4096':
            # strangers, but for PAIRS_4096 pairs of records of one person
            who = np.arange(n)
            twin = np.random.default_rng(seed + 1).permutation(n)[:2 * PAIRS_4096]
            who[twin[1::2]] = who[twin[::2]]
        ubm, rec, who = hand_records(seed, n, people, K, who=who)
        ok = np.ones(n, dtype=np.int32)
        if name == 'c4096':
            ok[list(NOT_OK_4096)] = 0
            rec[list(TIE_4096[1:])] = rec[TIE_4096[0]]
        if name.startswith('c130'):
            rec[list(TIE_130[1:])] = rec[TIE_130[0]]
        for a in (ubm, rec, ok, who):
            a.setflags(write=False)
        _BUILT[('large', name)] = (ubm, rec, ok, who)
    return _BUILT[('large', name)]


# ---------------------------------------------------------------------- the device against the fixture
# `dev` is a reseg_helpers.Dev.
def upload(dev, arr, name=None):
    """arr on the device: in a buffer of its own (freed when dev closes) or in the context's scratch `name`."""
    arr = np.ascontiguousarray(arr, dtype=np.float64)
    nbytes = max(arr.nbytes, 16)
    p = dev.alloc(nbytes) if name is None else dev.ctx.dev_scratch('clr_cases_' + name, nbytes)
    if arr.nbytes:
        dev.ctx.h2d(p, arr)
    return p


def link_on_device(dev, ubm, rec, ok, r, th, max_spk=0):
    """spkd_clr_link on the records -> its result; the records are not modified."""
    rec = np.ascontiguousarray(rec, dtype=np.float64)
    d_ubm, d_bw = upload(dev, ubm, 'ubm'), upload(dev, rec, 'bw')
    got = dev.ctx.clr_link(d_bw, ok, d_ubm, len(ubm), r, th, max_spk)
    after = np.empty_like(rec)
    if rec.size:
        dev.ctx.d2h(after, d_bw)
    assert after.tobytes() == rec.tobytes()
    return got


def identify_on_device(dev, ubm, probes, pok, off, gal, gok, r, th, exclusive=True):
    """spkd_clr_identify on the device -> (result, matrix); a cell the call leaves alone stays -7."""
    d_ubm, d_p, d_g = upload(dev, ubm, 'ubm'), upload(dev, probes, 'probes'), upload(dev, gal, 'gallery')
    mat = np.full((len(probes), len(gal)), -7.0)
    d_mat = upload(dev, mat, 'mat')
    got = dev.ctx.clr_identify(d_p, pok, off, d_g, gok, d_ubm, len(ubm), r, th, exclusive, d_scores=d_mat)
    if mat.size:
        dev.ctx.d2h(mat, d_mat)
    return got, mat


def _floats(decimals):
    return np.array([np.nan if v is None else float(v) for v in decimals], dtype=np.float64)


def check_group(dev, name):
    """A finite group on the device against the fixture.  Asserted here: the log, the labels and the
    identities are the exact ones; a pair's bits are the same from k_ident_scores (either way round,
    whatever the tiling), from k_clr_matrix (the extremes, the first logged value, every pair alone as a
    two-speaker call under a threshold below everything) and from k_clr_chain's recompute (a second call that starts from the records
    merged on the host by a + b continues the log with the same bits).  Returned: device_row()s of every
    value against the exact one, for assert_row."""
    e = fixture()['groups'][name]
    ubm, rec, ok, r, _ = build(name)
    n = len(rec)
    rows = []
    # k_ident_scores: every ordered pair of the group's records
    got, mat = identify_on_device(dev, ubm, rec, ok, [0, n], rec, ok, r, THRESHOLD, False)
    assert got['status'] == 0
    good = np.nonzero(ok)[0]
    assert np.isnan(mat[ok == 0]).all() and np.isnan(mat[:, ok == 0]).all() and np.isfinite(mat[np.ix_(good, good)]).all()
    assert mat[np.ix_(good, good)].tobytes() == mat[np.ix_(good, good)].T.copy().tobytes()     # H(a|b) + H(b|a) = H(b|a) + H(a|b)
    pairs = [(a, b) for a, b, _ in e['clr']]
    want = [float(v) for _, _, v in e['clr']]
    rows.append(device_row(name, 'k_ident_scores', e, [mat[a, b] for a, b in pairs], want))
    # k_clr_matrix: the extremes and the first logged value are the same bits
    link = link_on_device(dev, ubm, rec, ok, r, THRESHOLD)
    upper = np.array([mat[a, b] for a, b in pairs])
    assert link['status'] == 0 and link['stat_max'] == upper.max() and link['stat_min'] == upper.min()
    rows.append(device_row(name, 'stat', e, [link['stat_max'], link['stat_min']], [float(e['stat_max']), float(e['stat_min'])]))
    # the log: the exact one; its values
    log = list(zip(link['a'].tolist(), link['b'].tolist()))
    assert log == [(a, b) for a, b, _ in e['merges']], (name, log)
    rows.append(device_row(name, 'merge d', e, link['d'], [float(d) for _, _, d in e['merges']]))
    assert dev.hipabi.labels_from_merges(n, link['a'], link['b']).tolist() == e['labels']
    assert link['d'][0] == mat[log[0]]
    for a, b in pairs:                                                  # every pair alone, as a two-speaker call
        two = link_on_device(dev, ubm, rec[[a, b]], np.ones(2, dtype=np.int32), r, -1e300)
        assert two['n_merges'] == 1 and two['d'][0] == mat[a, b] == two['stat_max'] == two['stat_min'], (name, a, b)
    # k_clr_chain's recompute against k_clr_matrix and k_ident_scores on the merged records
    for m in sorted(set([1, len(log) // 2, len(log) - 1])):
        if not 0 < m < len(log):
            continue
        rec_m, ok_m = replay(rec, ok, log[:m])
        rest = link_on_device(dev, ubm, rec_m, ok_m, r, THRESHOLD)
        assert list(zip(rest['a'].tolist(), rest['b'].tolist())) == log[m:], (name, m)
        assert rest['d'].tobytes() == link['d'][m:].tobytes(), (name, m)
        _, mat_m = identify_on_device(dev, ubm, rec_m, ok_m, [0, len(rec_m)], rec_m, ok_m, r, THRESHOLD, False)
        assert mat_m[log[m]] == link['d'][m], (name, m)
    # the gallery problem of the group: the exact identities, scores and seconds
    pr, pok, off, gal, gok = gallery_of(name)
    s = len(pr)
    for key, exclusive in (('exclusive', True), ('free', False)):
        want = e['identify'][key]
        got, smat = identify_on_device(dev, ubm, pr, pok, off, gal, gok, r, THRESHOLD, exclusive)
        assert got['status'] == 0 and got['ident'].tolist() == want['ident'], (name, key)
        assert smat.tobytes() == mat[:s, s:].copy().tobytes(), (name, key)          # the bits do not depend on the tiling
        for what in ('score', 'second'):
            w = _floats(want[what])
            assert np.array_equal(np.isnan(got[what]), np.isnan(w)), (name, key, what)
            rows.append(device_row(name, '%s %s' % (key, what), e, got[what][~np.isnan(w)], w[~np.isnan(w)]))
    return rows
