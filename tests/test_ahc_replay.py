"""The merge loop's WHOLE log against numpy's loop where ties, NaNs, infinities and signed zeros decide: the
kernels (k_ahc, the step chain) share scan_row, row_cache_after_merge, the key-ordered selection and
final_matrix_max (spkd_cluster.hpp), which promise numpy's first-occurrence / NaN semantics.  The reference is
tests/ahc_replay.py -- the literal O(n^2)-per-round loop with C oracle distances, no row cache -- recorded in
tests/golden/ahc_replay.json for the scenarios of tests/ahc_replay_cases.py.

Why the replay's decisions are the device's: the device is held to the C oracle at 1e-9 (_same_merges); in every
round of every scenario the cells equal to the minimum share an origin key (planted with one value, or computed
from duplicate records in one orientation, hence the same arithmetic on the same bits), every other cell lies
more than 1e-7 above the minimum, and a computed minimum is more than 1e-7 away from the threshold
(test_every_scenario_meets_the_safety_condition, on the CPU)."""
import json
import math
import os

import numpy as np
import pytest

import ahc_replay
import ahc_replay_cases as cases
from conftest import pkg, ROOT

gpu = pytest.mark.gpu
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'ahc_replay.json')


def _fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)


FX = _fixture()
NAMES = [s['name'] for s in FX['scenarios']]
BY_NAME = {s['name']: s for s in FX['scenarios']}


def _val(h):
    return None if h is None else (float('nan') if h == 'nan' else float.fromhex(h))


@pytest.fixture(scope='module')
def host():
    f = cases.frames()
    return f, cases.OracleDistances(f)


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize('variant', [1, 2])
def test_replay_equals_both_oracles_with_nothing_planted(host, variant):
    """Twelve records (one duplicate pair): the replay, handed the oracle's initial matrix, gives the merges of
    NumpyEngine.cluster_hi (raw frames) and of COracleEngine.ahc_raw exactly, the distances at 1e-9."""
    from oracle.numpy_engine import NumpyEngine
    f, orc = host
    s = dict(name='twelve', n=12, variant=variant, kind='BIC', lambdac=1.3, threshold=0.0, max_spk=0, planted=[],
             slices=cases.slice_table(12, [(4, 64)]))
    got = cases.run_replay(s, orc)
    assert len(got['merges']) >= 6
    ne = NumpyEngine()
    ne.set_features(f)
    segs = [tuple(r) for r in s['slices']]
    want = ne.cluster_hi(segs, variant, 'BIC', 1.3, 0.0, 0)
    raw, smax, smin = orc.eng.ahc_raw(orc.eng.stats([[r] for r in segs]), variant, 'BIC', 1.3, 0.0, 0)
    for ref, rmax, rmin in ((want.merges, want.max_dist, want.min_dist), (raw, smax, smin)):
        assert [(a, b) for a, b, _, _ in got['merges']] == [(a, b) for a, b, _ in ref]
        for (_, _, d, _), (_, _, w) in zip(got['merges'], ref):
            assert abs(d - w) <= 1e-9 * max(1.0, abs(w))
        for g, w in ((got['max_dist'], rmax), (got['min_dist'], rmin)):
            assert g == w or abs(g - w) <= 1e-9 * max(1.0, abs(w))


@pytest.mark.parametrize('name', ['planted_n65_v1', 'nans_n65_v2'])
def test_fixture_is_current(host, name):
    """The scenario as tests/ahc_replay_cases.py defines it today, replayed live, is the fixture's entry."""
    f, orc = host
    s = [x for x in cases.scenarios() if x['name'] == name][0]
    live = cases.to_fixture(s, cases.run_replay(s, orc), cases.frames_sha256(f))
    assert json.loads(json.dumps(live)) == BY_NAME[name]


def test_fixture_holds_the_scenarios_as_defined(host):
    f, _ = host
    sc = cases.scenarios()
    assert [s['name'] for s in sc] == NAMES
    sha = cases.frames_sha256(f)
    for s in sc:
        fx = BY_NAME[s['name']]
        assert fx['frames_sha256'] == sha
        assert fx['slices'] == [list(r) for r in s['slices']] and fx['planted'] == [list(p) for p in s['planted']]
        assert (fx['n'], fx['variant'], fx['kind'], fx['lambdac'], _val(fx['threshold']), fx['max_spk']) == \
            (s['n'], s['variant'], s['kind'], s['lambdac'], s['threshold'], s['max_spk'])


def test_every_scenario_meets_the_safety_condition():
    """A condition on the fixture, not a measurement: every recorded gap and threshold gap is above 1e-7 (the
    replay leaves out of a gap only cells that share the winner's origin key and its bits, zeros of either sign
    under one key, and +inf cells against a +inf minimum); every event the merge rules can meet occurs for each
    variant it applies to, one of them at a merge index >= 10 and one at n = 257 in a column >= 256."""
    assert FX['margin'] == ahc_replay.MARGIN == 1e-7
    seen = {1: {}, 2: {}}
    late = wide = False
    for fx in FX['scenarios']:
        rounds = [{'gap': _val(g), 'thr_gap': _val(t), 'nan': bool(nn)} for g, t, nn in fx['rounds']]
        assert len(rounds) == len(fx['merges']) + 1                         # every merge and the stop
        assert ahc_replay.unsafe_rounds(rounds) == [], fx['name']
        gaps = [r['gap'] for r in rounds if r['gap'] is not None]
        assert _val(fx['smallest_gap']) == (min(gaps) if gaps else None)
        for k, cnt in fx['events'].items():
            seen[fx['variant']][k] = seen[fx['variant']].get(k, 0) + cnt
            late = late or fx['where'][k][0] >= 10
            wide = wide or (fx['n'] == 257 and fx['where'][k][1] >= 256)
        if fx['variant'] == 1:
            assert _val(fx['max_dist']) > 0.0       # the reference's `note` rule is then a plain max / min
    for variant in (1, 2):
        assert [e for e in cases.REQUIRED[variant] if not seen[variant].get(e)] == []
    assert late and wide
    assert sorted({fx['n'] for fx in FX['scenarios']}) == [65, 130, 257, 577]
    assert any(fx['kind'] == 'GLR' for fx in FX['scenarios'])


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def dev():
    """One engine and the frame buffer on the device for the whole module."""
    engine = pkg('engine')
    e = engine.HipEngine(0)
    f = cases.frames()
    d_fr = e.ctx.dev_alloc(f.nbytes)
    e.ctx.h2d(d_fr, f)
    yield e.ctx, d_fr, f.shape[0]
    e.ctx.dev_free(d_fr)
    e.close()


def _records(ctx, d_fr, n_frames, slices, d_st):
    n = len(slices)
    b = np.array([r[0] for r in slices], dtype=np.int64)
    e = np.array([r[1] for r in slices], dtype=np.int64)
    ctx.set_stats(d_fr, n_frames, b, e, np.arange(n, dtype=np.int32), n, d_st)


def _bits_or_nan_equal(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return np.array_equal(np.isnan(x), np.isnan(y)) and \
        np.array_equal(x[~np.isnan(x)].view(np.uint64), y[~np.isnan(y)].view(np.uint64))


def _check_value(got, want, kind, what, plus_zero=False):
    """want from the fixture: NaN where it has NaN; a planted or fill value to the bit (zeros of either sign are
    equal, as to numpy); a computed one within _same_merges' 1e-9.  plus_zero: a zero must come as +0.0, as spkd.h
    (4) says of a zero minimum."""
    if math.isnan(want):
        assert math.isnan(got), what
    elif want == 0.0 and plus_zero:
        assert got == 0.0 and not np.signbit(got), (what, got)
    elif kind in ahc_replay.EXACT or math.isinf(want):
        assert got == want and (want == 0.0 or np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64)), \
            (what, got, want)
    else:
        assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (what, got, want)


def _check_log(r, lo, fx, what):
    nm = int(r['n_merges'][what[1]]) if isinstance(what, tuple) else int(r['n_merges'][0])
    got = list(zip(r['a'][lo:lo + nm].tolist(), r['b'][lo:lo + nm].tolist()))
    want = [(a, b) for a, b, _, _ in fx['merges']]
    first = next((k for k, (g, w) in enumerate(zip(got, want)) if g != w), None)
    assert first is None, (what, 'merge', first, got[first], want[first])
    assert nm == len(want), (what, nm, len(want))
    for k, (_, _, d, kind) in enumerate(fx['merges']):
        _check_value(float(r['d'][lo + k]), _val(d), kind, (what, 'd', k), plus_zero=True)


@gpu
@pytest.mark.parametrize('name', NAMES)
def test_ahc_matrix_log_is_the_replays(dev, name):
    """spkd_ahc_matrix under both launch shapes on the device's own initial matrix (distance_rows, mirrored for
    variant 1 as spkd.h asks) with the scenario's cells planted: n_merges and every (a, b) are the fixture's, the
    distances and stat_max / stat_min by _check_value, and MONO and WIDE agree to the bit.  A scenario whose replay
    stops on a diagonal cell must be refused as a degenerate merge."""
    hipabi = pkg('hipabi')
    ctx, d_fr, n_frames = dev
    fx = BY_NAME[name]
    n, variant, kind = fx['n'], fx['variant'], fx['kind']
    d_st = ctx.dev_alloc(n * hipabi.REC * 8)
    d_m = ctx.dev_alloc(n * n * 8)
    try:
        _records(ctx, d_fr, n_frames, fx['slices'], d_st)
        ctx.distance_rows(variant, kind, fx['lambdac'], d_st, n, 0, n, d_m)
        M = np.empty((n, n), dtype=np.float64)
        ctx.d2h(M, d_m)
        if variant == 1:
            diag = np.diag(M).copy()
            up = np.triu(M, 1)
            M = up + up.T
            M[np.diag_indices(n)] = diag
        cases.plant(M, None, fx)
        up = M[np.triu_indices(n, 1)]
        fin = up[np.isfinite(up)]
        got = {}
        for path in (hipabi.AHC_MONO, hipabi.AHC_WIDE):
            ctx.h2d(d_m, np.ascontiguousarray(M))
            p = hipabi.AhcParams(variant, hipabi.KINDS[kind], fx['max_spk'], path, fx['lambdac'], _val(fx['threshold']))
            if fx['degenerate']:
                # the replay ended on a diagonal cell (numpy's first +inf): the call reports it, under either shape
                with pytest.raises(hipabi.SpkdError, match='degenerate merge') as ei:
                    ctx.ahc_matrix(d_st, n, p, d_m, float(fin.max()), float(fin.min()))
                assert ei.value.status == hipabi.SPKD_EINVAL
                continue
            got[path] = ctx.ahc_matrix(d_st, n, p, d_m, float(fin.max()), float(fin.min()))
            assert got[path]['status'] == 0
        if fx['degenerate']:
            return
        a, b = got[hipabi.AHC_MONO], got[hipabi.AHC_WIDE]
        for tag, r in (('MONO', a), ('WIDE', b)):
            _check_log(r, 0, fx, tag)
            _check_value(float(r['stat_max'][0]), _val(fx['max_dist']), fx['max_kind'], (tag, 'stat_max'))
            _check_value(float(r['stat_min'][0]), _val(fx['min_dist']), fx['min_kind'], (tag, 'stat_min'))
        nm = len(fx['merges'])
        assert _bits_or_nan_equal(a['d'][:nm], b['d'][:nm])
        assert _bits_or_nan_equal(a['stat_max'], b['stat_max']) and _bits_or_nan_equal(a['stat_min'], b['stat_min'])
    finally:
        ctx.dev_free(d_m)
        ctx.dev_free(d_st)


@gpu
@pytest.mark.parametrize('variant', [1, 2])
def test_ahc_batch_call_logs_are_the_replays(dev, variant):
    """The three unplanted duplicate-record scenarios as the three problems of ONE spkd_ahc call per launch shape
    (offsets 65 and 195: no multiples of a wave); duplicates of different lengths merge with each other."""
    hipabi = pkg('hipabi')
    ctx, d_fr, n_frames = dev
    fxs = [BY_NAME['dups_n%d_v%d' % (n, variant)] for n in (65, 130, 257)]
    assert all(not fx['planted'] for fx in fxs)
    slices = sum((fx['slices'] for fx in fxs), [])
    seg_off = np.array([0, 65, 195, 452], dtype=np.int64)
    d_st = ctx.dev_alloc(len(slices) * hipabi.REC * 8)
    try:
        _records(ctx, d_fr, n_frames, slices, d_st)
        got = {}
        for path in (hipabi.AHC_MONO, hipabi.AHC_WIDE):
            p = hipabi.AhcParams(variant, hipabi.KINDS['BIC'], 0, path, 1.3, 0.0)
            r = got[path] = ctx.ahc(d_st, seg_off, p)
            assert r['status'] == 0
            for k, fx in enumerate(fxs):
                _check_log(r, int(seg_off[k]), fx, (path, k))
                _check_value(float(r['stat_max'][k]), _val(fx['max_dist']), fx['max_kind'], (path, k, 'stat_max'))
                _check_value(float(r['stat_min'][k]), _val(fx['min_dist']), fx['min_kind'], (path, k, 'stat_min'))
        a, b = got[hipabi.AHC_MONO], got[hipabi.AHC_WIDE]
        assert _bits_or_nan_equal(a['d'], b['d']) and _bits_or_nan_equal(a['stat_max'], b['stat_max'])
    finally:
        ctx.dev_free(d_st)
