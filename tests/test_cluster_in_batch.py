"""spk_cluster_in for a whole batch (spkd_cluster_in_batch: one workgroup per problem) against the
single-problem chain it shares its body with (spkd_cluster_in), and the `method='in'` mode of the
batch pipeline against the command line in `-m in` mode."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

from helpers import ROOT
from conftest import pkg

MAXINT = 9223372036854775808.0
KINDS = ['BIC', 'GLR', 'KL2', 'KL2P']
# the working thresholds of test_cluster_in_device_chain_equals_the_per_line_path, and one that
# founds a cluster per record
WORKING = {'BIC': 0.0, 'GLR': 1800.0, 'KL2': 12.0, 'KL2P': 12.0}
EVERY_RECORD = -1e30
# problem sizes: empty, a lone record, one step, 19 (with a cluster per record the 17th step has 16
# clusters, one workgroup pass of 4 waves x 4 clusters, and the 18th needs the second pass), and
# one long enough to join and found in turn
SIZES = [0, 1, 2, 19, 40]
NAN_PROBLEM, NAN_RECORD = 3, 15           # the 19-record problem, a late segment


# ------------------------------------------------------------------ not GPU
def test_method_key_is_validated():
    pipeline = pkg('pipeline')
    bad = dict(pipeline.DIA2_CL, method='agglomerative')
    with pytest.raises(ValueError):
        pipeline.diarize_batch(None, 0, 0, [], cl=bad)
    with pytest.raises(ValueError):
        pipeline.cluster_batch(None, 0, 0, [], [], cl=bad)
    cl_in = dict(pipeline.DIA2_CL, method='in')
    with pytest.raises(ValueError):
        pipeline.diarize_batch(None, 0, 0, [], cl=cl_in, fused=True, handoff='device')
    # 'in' takes the host hand-off by default, also where 'hi' takes the device's; 'hi' and no key are valid
    assert pipeline.diarize_batch(None, 0, 0, [], cl=cl_in, fused=True) == []
    assert pipeline.diarize_batch(None, 0, 0, [], cl=dict(pipeline.DIA2_CL, method='hi'), fused=True) == []
    assert 'method' not in pipeline.DIA2_CL


def test_entry_point_is_declared_and_exported():
    hipabi = pkg('hipabi')
    text = open(os.path.join(ROOT, 'include', 'spkd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = hipabi.load_library()
    assert re.search(r'\bspkd_cluster_in_batch\s*\(', code)
    assert 'spkd_cluster_in_batch' in hipabi.EXPORTS and hasattr(lib, 'spkd_cluster_in_batch')
    assert lib.spkd_abi_version() == 2
    # argument checks come before any device work: no context, no call
    off = np.array([0, 1], dtype=np.int64)
    st = lib.spkd_cluster_in_batch(None, None, 1, off.ctypes.data_as(C.c_void_p), 0, 1.3, 0.0, None, None, None, None,
                                   None, None)
    assert st == hipabi.SPKD_EINVAL


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def data():
    """Records of the speaker turns of two sessions, dealt to the problems of SIZES; the single
    problem results (ctx.cluster_in on a problem's records alone) are computed once per (kind,
    threshold, problem) and shared."""
    engine = pkg('engine')
    hipabi = pkg('hipabi')
    synth = pkg('synth')
    fa, _, ta = synth.make_session(515, 900, 4)
    fb, _, tb = synth.make_session(616, 400, 3)
    frames = np.concatenate([fa, fb])
    sa = [(a, b) for a, b, _ in ta]
    sb = [(a + fa.shape[0], b + fa.shape[0]) for a, b, _ in tb]
    assert len(sa) >= 42 and len(sb) >= 20
    # (0) | 1 of B | 2 of A | 19 of B | 40 of A
    segs = [[], sb[19:20], sa[40:42], sb[:19], sa[:40]]
    assert [len(s) for s in segs] == SIZES
    eng = engine.HipEngine(0)
    eng.set_features(frames)
    d = dict(eng=eng, ctx=eng.ctx, hipabi=hipabi, frames=frames, segs=segs, single={}, bufs=[])
    d['d_stats'], d['seg_off'] = _records(d, segs)
    yield d
    for p in d['bufs']:
        eng.ctx.dev_free(p)
    eng.close()


def _records(d, segs):
    flat = [[s] for prob in segs for s in prob]
    ptr = d['eng']._stats_of_sets(flat)
    d['bufs'].append(ptr)
    seg_off = np.zeros(len(segs) + 1, dtype=np.int64)
    seg_off[1:] = np.cumsum([len(s) for s in segs])
    return ptr, seg_off


def _single(d, kind, thr, p, d_stats=None, seg_off=None, keep=True):
    """ctx.cluster_in on problem p's records alone -> dict like a problem's slice of the batch result."""
    key = (kind, thr, p)
    if keep and key in d['single']:
        return d['single'][key]
    hipabi = d['hipabi']
    d_stats = d['d_stats'] if d_stats is None else d_stats
    seg_off = d['seg_off'] if seg_off is None else seg_off
    o, n = int(seg_off[p]), int(seg_off[p + 1] - seg_off[p])
    label, dists, done, nclu, st = d['ctx'].cluster_in(d_stats + o * hipabi.REC * 8, n, kind, 1.3, thr)
    mind = np.full(done, MAXINT)
    for s in range(done):
        fin = dists[s][np.isfinite(dists[s])]
        if len(fin):
            mind[s] = fin.min()
    allfin = np.concatenate([x[np.isfinite(x)] for x in dists]) if done else np.zeros(0)
    r = dict(label=np.array(label[:done]), mind=mind, n_done=done, n_clusters=nclu, status=st,
             stat_max=allfin.max() if len(allfin) else np.nan, stat_min=allfin.min() if len(allfin) else np.nan)
    if keep:
        d['single'][key] = r
    return r


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _assert_problem(got, seg_off, p, want, tag):
    o = int(seg_off[p])
    nd = int(want['n_done'])
    assert int(got['n_done'][p]) == nd, tag
    assert int(got['n_clusters'][p]) == int(want['n_clusters']), tag
    assert np.array_equal(got['label'][o:o + nd], want['label']), tag
    assert np.array_equal(_bits(got['mind'][o:o + nd]), _bits(want['mind'])), tag
    assert np.array_equal(_bits(got['stat_max'][p:p + 1]), _bits([want['stat_max']])), tag
    assert np.array_equal(_bits(got['stat_min'][p:p + 1]), _bits([want['stat_min']])), tag


@pytest.mark.gpu
@pytest.mark.parametrize('founding', ['working', 'every_record'])
@pytest.mark.parametrize('kind', KINDS)
def test_batch_equals_single_to_the_bit(data, kind, founding):
    hipabi = data['hipabi']
    thr = WORKING[kind] if founding == 'working' else EVERY_RECORD
    seg_off = data['seg_off']
    got = data['ctx'].cluster_in_batch(data['d_stats'], seg_off, kind, 1.3, thr)
    assert got['status'] == hipabi.SPKD_OK
    for p, n in enumerate(SIZES):
        want = _single(data, kind, thr, p)
        assert want['status'] == hipabi.SPKD_OK and want['n_done'] == n
        _assert_problem(got, seg_off, p, want, (kind, thr, p))
    assert int(got['n_done'][0]) == 0 and int(got['n_clusters'][0]) == 0
    assert np.isnan(got['stat_max'][0]) and np.isnan(got['stat_min'][0])
    assert got['mind'][int(seg_off[1])] == MAXINT and np.isnan(got['stat_max'][1])     # a lone record meets no cluster
    big = int(got['n_clusters'][4])
    print('%s threshold %g: clusters per problem %s' % (kind, thr, got['n_clusters'].tolist()))
    if founding == 'working':
        assert 1 < big < 40             # records joined and records founded
    else:
        assert got['n_clusters'].tolist() == SIZES          # the 19-record problem: past one pass of 16 clusters


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_problem_order_does_not_matter(data, kind):
    hipabi = data['hipabi']
    rev = data['segs'][::-1]
    d_rev, off_rev = _records(data, rev)
    for thr in (WORKING[kind], EVERY_RECORD):
        got = data['ctx'].cluster_in_batch(d_rev, off_rev, kind, 1.3, thr)
        assert got['status'] == hipabi.SPKD_OK
        for q in range(len(SIZES)):
            p = len(SIZES) - 1 - q
            _assert_problem(got, off_rev, q, _single(data, kind, thr, p), (kind, thr, p))


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_a_nonfinite_record_stays_in_its_problem(data, kind):
    """One NaN frame inside a late segment of one problem of four: an input the library reports
    (the reference's det raises on such a covariance), in that problem only."""
    hipabi = data['hipabi']
    eng = data['eng']
    segs = data['segs'][1:]                                  # the four problems with records
    a, b = segs[NAN_PROBLEM - 1][NAN_RECORD]
    bad = data['frames'].copy()
    bad[(a + b) // 2, 7] = np.nan
    thr = WORKING[kind]
    try:
        eng.set_features(bad)
        d_bad, off_bad = _records(data, segs)
        got = data['ctx'].cluster_in_batch(d_bad, off_bad, kind, 1.3, thr)
        alone = _single(data, kind, thr, NAN_PROBLEM - 1, d_bad, off_bad, keep=False)
    finally:
        eng.set_features(data['frames'])
    assert got['status'] == hipabi.SPKD_ENONFINITE and alone['status'] == hipabi.SPKD_ENONFINITE
    assert alone['n_done'] < SIZES[NAN_PROBLEM]
    assert int(got['n_done'][NAN_PROBLEM - 1]) == alone['n_done']
    for q in range(4):
        if q != NAN_PROBLEM - 1:
            want = _single(data, kind, thr, q + 1)           # the clean data's: the records are the same
            assert want['n_done'] == SIZES[q + 1]
            _assert_problem(got, off_bad, q, want, (kind, q))


@pytest.mark.gpu
def test_argument_checks_on_a_context(data):
    hipabi = data['hipabi']
    ctx = data['ctx']
    r = ctx.cluster_in_batch(data['d_stats'], [0], 'BIC', 1.3, 0.0)              # no problem at all
    assert r['status'] == hipabi.SPKD_OK and len(r['label']) == 0 and len(r['n_done']) == 0
    r = ctx.cluster_in_batch(data['d_stats'], [0, 0, 0], 'GLR', 1.3, 0.0)        # only empty problems
    assert r['status'] == hipabi.SPKD_OK and r['n_done'].tolist() == [0, 0] and r['n_clusters'].tolist() == [0, 0]
    for seg_off, kind in (([0, 3, 2], 'BIC'), ([0, 2], 7), ([0, 2], -1)):
        with pytest.raises(hipabi.SpkdError) as ei:
            ctx.cluster_in_batch(data['d_stats'], seg_off, kind, 1.3, 0.0)
        assert ei.value.status == hipabi.SPKD_EINVAL
    off = np.array([0, 2], dtype=np.int64)
    out = [np.zeros(2, dtype=np.float64) for _ in range(6)]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [C.c_void_p(data['d_stats']), 1, ptr(off), 0, 1.3, 0.0] + [ptr(a) for a in out]
    for k in (0, 2, 6, 7, 8, 9, 10, 11):
        bad = list(args)
        bad[k] = None
        assert ctx.lib.spkd_cluster_in_batch(ctx.h, *bad) == hipabi.SPKD_EINVAL, k


def _cli_in_mode(tmp, engine, variant, lines):
    """The clustering command line in -m in mode on a recipe of `lines` -> its output rows as text."""
    cli = pkg('cli')
    rin, rout = os.path.join(tmp, 'spkc.recipe'), os.path.join(tmp, 'in%d.recipe' % variant)
    with open(rin, 'w') as fh:
        fh.writelines(lines)
    if os.path.exists(rout):
        os.remove(rout)
    cli.main_clustering([rin, os.path.join(tmp, 'fea') + '/', '-o', rout, '-m', 'in', '-l', '1.3'],
                        variant=variant, engine=engine, stdout=io.StringIO())
    return re.findall(r'start-time=(\S+) end-time=(\S+) speaker=speaker_(\d+)', open(rout).read())


@pytest.mark.gpu
def test_pipeline_in_mode_equals_the_command_line(data, tmp_path):
    """diarize_batch with method='in' (fused and two-pass, variants 1 and 2) against the command
    line in -m in mode on each file's own change-detection segments, with the library and with
    the C oracle behind it."""
    from oracle.c_engine import COracleEngine
    synth = pkg('synth')
    pipeline = pkg('pipeline')
    recipe = pkg('recipe')
    engine = pkg('engine')
    s2 = recipe.py2_float_str
    sessions = [synth.make_session(31 + i, 200 + 40 * i, 3 + (i % 2)) for i in range(3)]
    frames = np.concatenate([s[0] for s in sessions])
    eng = engine.HipEngine(0)
    cli_eng = engine.HipEngine(0)
    try:
        eng.set_features(frames)
        files, off = [], 0
        for i, (feats, vad, _) in enumerate(sessions):
            v = [(float(s2(a / 125.0)), float(s2(b / 125.0))) for a, b in vad]
            files.append(pipeline.BatchFile(off, feats.shape[0], [] if i == 1 else v))       # file 1: no turn
            off += feats.shape[0]
        args = (eng.ctx, eng.d_frames, frames.shape[0], files)
        segs = pipeline.change_detect_batch(*args)
        assert len(segs[1]) == 0 and len(segs[0]) > 10 and len(segs[2]) > 10
        got = {}
        for variant in (1, 2):
            cl = dict(pipeline.DIA2_CL, method='in', variant=variant)
            tm = {}
            got[variant] = pipeline.diarize_batch(*args, cl=cl, fused=True, timings=tm)
            two_pass = pipeline.diarize_batch(*args, cl=cl, fused=False)
            for g, t in zip(got[variant], two_pass):
                assert np.array_equal(g, t)
            assert got[variant][1].shape == (0, 3)
            labels = [g[:, 2].astype(np.int64) for g in got[variant]]
            # every record but a file's first meets the clusters founded before it
            assert tm['cluster_in_pairs'] == sum(int(np.maximum.accumulate(l[:-1]).sum()) for l in labels if len(l))
            assert len(tm['cluster_prep']) == 1 and len(tm['ahc']) == 1 and 'matrix' not in tm
        res = pipeline.cluster_batch(*args, segs, cl=dict(pipeline.DIA2_CL, method='in'), want_merges=True)
        assert all(m is None for _, m in res) and len(res[1][0]) == 0
        assert np.array_equal(res[0][0], got[1][0][:, 2].astype(np.int32))
        for k in (0, 2):
            tmp = os.path.join(str(tmp_path), 'f%d' % k)
            os.makedirs(os.path.join(tmp, 'fea'))
            synth.write_fea(os.path.join(tmp, 'fea', 'x.fea'), sessions[k][0])
            lines = ['audio=x.wav lna=a_%d start-time=%s end-time=%s speaker=spk_turn\n' % (j + 1, s2(a), s2(b))
                     for j, (a, b) in enumerate(np.asarray(segs[k]).tolist())]
            for variant in (1, 2):
                rows = got[variant][k]
                for tag, e in (('hip', cli_eng), ('orc', COracleEngine())):
                    want = _cli_in_mode(tmp, e, variant, lines)
                    assert len(want) == len(rows) == len(lines), (k, variant, tag)
                    assert [int(c) for _, _, c in want] == rows[:, 2].astype(np.int64).tolist(), (k, variant, tag)
                    assert [(a, b) for a, b, _ in want] == [(s2(a), s2(b)) for a, b in rows[:, :2].tolist()], (k, variant, tag)
                assert 1 < len(set(rows[:, 2].tolist())) < len(rows)
    finally:
        eng.close()
        cli_eng.close()
