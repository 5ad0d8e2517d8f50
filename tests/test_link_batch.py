"""Linking the speakers of a batch's files: spkd_sum_stats (records -> sums of records, in member
order, to the bit), pipeline.link_batch (spk_cluster_hi over whole speakers) against the
reference's own function on three files of one meeting series (tests/golden/link_cases.json,
written by tests/golden/make_golden_link.py), and diarize_batch(..., link=...)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from helpers import ROOT
from conftest import pkg

GOLD = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'link_cases.json')))
CASE_NAMES = [c['name'] for c in GOLD['cases']]
_SERIES = {}


def _series():
    """The golden's three files: [(features, vad turns, truth)], checked against its SHA-256."""
    if not _SERIES:
        synth = pkg('synth')
        s = synth.make_series([f['seed'] for f in GOLD['files']], GOLD['seconds'], GOLD['shared_seed'],
                              GOLD['n_shared'], GOLD['n_speakers'])
        for (feats, _, _), meta in zip(s, GOLD['files']):
            assert synth.fea_sha256(feats) == meta['sha256'], 'synthetic generator is not reproducible here'
        _SERIES['s'] = s
    return _SERIES['s']


def _golden_labels():
    return [np.array([s[2] for s in f['segments']], dtype=np.int32) for f in GOLD['files']]


def _golden_seg_off():
    return np.concatenate([[0], np.cumsum([len(f['segments']) for f in GOLD['files']])]).astype(np.int64)


def _case_cl(case):
    return dict(variant=case['variant'], kind=case['kind'], lambdac=case['lambdac'], threshold=case['threshold'],
                max_spk=case['max_spk'])


def _global_ids(case):
    """The golden's final speaker (1-based, the reference's numbering) of every initial speaker."""
    ids = np.zeros(len(GOLD['speakers']), dtype=np.int64)
    for k, group in enumerate(case['partition']):
        ids[group] = k + 1
    assert ids.min() >= 1
    return ids


# ------------------------------------------------------------------ not GPU
def test_entry_point_is_declared_and_exported():
    hipabi = pkg('hipabi')
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'spkd.h')).read(), flags=re.S)
    lib = hipabi.load_library()
    assert re.search(r'\bspkd_sum_stats\s*\(', code)
    assert 'spkd_sum_stats' in hipabi.EXPORTS and hasattr(lib, 'spkd_sum_stats')
    assert lib.spkd_abi_version() == 2 and re.search(r'#define SPKD_ABI_VERSION 2\b', code)
    off = np.array([0, 1], dtype=np.int64)
    assert lib.spkd_sum_stats(None, None, 1, None, off.ctypes.data_as(C.c_void_p), 1, None) == hipabi.SPKD_EINVAL
    assert hasattr(hipabi.Context, 'sum_stats')


def test_golden_speaker_list_is_the_rule_of_link_speakers():
    """The golden was built on speakers ordered file by file and by ascending label, each with its
    segments in segment order: link_speakers gives that list from the per-file labels."""
    pipeline = pkg('pipeline')
    member, set_off, spk_file, spk_label = pipeline.link_speakers(_golden_seg_off(), _golden_labels())
    got = [member[a:b].tolist() for a, b in zip(set_off[:-1], set_off[1:])]
    assert got == [[l for _, _, l in s] for s in GOLD['speakers']]
    assert spk_file.tolist() == sorted(spk_file.tolist())
    # the recurring speakers are linked, the files' own ones kept apart, in every case without -ms
    for case in GOLD['cases']:
        assert case['min_margin'] > GOLD['margin_bar']
        if case['max_spk'] == 0:
            assert sorted(sorted(g) for g in case['partition']) == GOLD['people']


@pytest.mark.parametrize('name', CASE_NAMES)
def test_numpy_restatement_reproduces_the_reference(name):
    """tests/link_numpy.py, the merge loop from multi-segment speakers, against the reference's
    spk_cluster_hi: same merges in the same order, distances to the 1e-9 relative
    test_oracle_golden.py holds the numpy oracle to, same final partition."""
    from oracle.numpy_engine import NumpyEngine
    from link_numpy import link_hi
    case = GOLD['cases'][CASE_NAMES.index(name)]
    ne = NumpyEngine()
    ne.set_features(np.concatenate([s[0] for s in _series()]))
    merges, partition = link_hi(ne, [[(b, e) for b, e, _ in s] for s in GOLD['speakers']], case['variant'],
                                case['kind'], case['lambdac'], case['threshold'], case['max_spk'])
    assert [(a, b) for a, b, _ in merges] == [(a, b) for a, b, _ in case['merges']]
    for (_, _, d), (_, _, w) in zip(merges, case['merges']):
        w = float.fromhex(w)
        assert abs(d - w) <= 1e-9 * max(1.0, abs(d), abs(w))
    assert partition == [sorted(g) for g in case['partition']]


class _StubContext(object):
    """Records what link_batch asks of a context and answers a canned merge log."""

    def __init__(self, merges):
        self.merges, self.calls = merges, []

    def dev_scratch(self, name, nbytes):
        self.calls.append(('dev_scratch', name, nbytes))
        return 4096

    def sum_stats(self, d_src, n_src, member, set_off, d_dst):
        self.calls.append(('sum_stats', d_src, n_src, np.array(member).tolist(), np.array(set_off).tolist(), d_dst))

    def last_ms(self, which='call'):
        return 0.25

    def ahc(self, d_stats, seg_off, params):
        self.calls.append(('ahc', d_stats, np.array(seg_off).tolist(), params.variant, params.kind, params.max_spk,
                           params.path, params.lambdac, params.threshold))
        n = int(seg_off[-1])
        a, b, d = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n)
        for k, (x, y, z) in enumerate(self.merges):
            a[k], b[k], d[k] = x, y, z
        return dict(status=0, n_merges=np.array([len(self.merges)], np.int32), a=a, b=b, d=d,
                    stat_max=np.array([7.0]), stat_min=np.array([-3.0]))


def test_speaker_order_and_label_gaps_on_the_host():
    pipeline, hipabi = pkg('pipeline'), pkg('hipabi')
    assert set(pipeline.LINK_CL) == set(pipeline.DIA2_CL)
    assert pipeline.LINK_CL == dict(variant=1, kind='BIC', lambdac=1.3, threshold=0.0, max_spk=0)
    # file 0: labels 1, 3 and 5 (2 and 4 carried by no segment); file 1: no segment; file 2: label 2 alone
    labels = [np.array([3, 1, 3, 1, 5]), np.zeros(0, dtype=np.int32), np.array([2, 2])]
    seg_off = [0, 5, 5, 7]
    member, set_off, spk_file, spk_label = pipeline.link_speakers(seg_off, labels)
    assert member.tolist() == [1, 3, 0, 2, 4, 5, 6] and set_off.tolist() == [0, 2, 4, 5, 7]
    assert spk_file.tolist() == [0, 0, 0, 2] and spk_label.tolist() == [1, 3, 5, 2]
    stub = _StubContext([(0, 3, -12.5)])               # speaker (0, 1) and speaker (2, 2) are one person
    timings = {}
    maps, merges, smax, smin = pipeline.link_batch(stub, 1 << 20, seg_off, labels, timings=timings)
    assert [m.tolist() for m in maps] == [[0, 1, 0, 2, 0, 3], [], [0, 0, 1]]
    assert merges == [(0, 3, -12.5)] and (smax, smin) == (7.0, -3.0)
    assert [c[0] for c in stub.calls] == ['dev_scratch', 'sum_stats', 'ahc']
    assert stub.calls[0][2] == 4 * hipabi.REC * 8
    assert stub.calls[1][1:] == (1 << 20, 7, [1, 3, 0, 2, 4, 5, 6], [0, 2, 4, 5, 7], 4096)
    assert stub.calls[2][1:] == (4096, [0, 4], 1, hipabi.KINDS['BIC'], 0, hipabi.AHC_AUTO, 1.3, 0.0)
    assert timings['link_speakers'] == 4 and timings['link_merges'] == 1
    assert timings['link_sum'] == [0.25] and timings['link_ahc'] == [0.25]
    # no speaker at all: empty maps, and the context is not touched
    maps, merges, _, _ = pipeline.link_batch(None, 0, [0, 0, 0], [np.zeros(0, dtype=np.int32)] * 2)
    assert [m.tolist() for m in maps] == [[], []] and merges == []
    with pytest.raises(ValueError):
        pipeline.link_speakers([0, 2], [np.array([1])])
    with pytest.raises(ValueError):
        pipeline.link_speakers([0, 2], [np.array([0, 1])])


def test_link_takes_the_host_hand_off():
    pipeline = pkg('pipeline')
    for kw in (dict(handoff='device', fused=True), dict(fused=True), dict(handoff='device')):
        with pytest.raises(ValueError, match='link takes the host hand-off'):
            pipeline.diarize_batch(None, 0, 0, [], link=pipeline.LINK_CL, **kw)
    # fused without the text contract is a host hand-off, as is the two-pass form
    det = {}
    assert pipeline.diarize_batch(None, 0, 0, [], link=pipeline.LINK_CL, fused=True, text_contract=False, detail=det) == []
    assert det['link']['maps'] == [] and det['link']['merges'] == []
    assert pipeline.diarize_batch(None, 0, 0, [], link=pipeline.LINK_CL) == []


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def dev():
    """The three files resident as one frame array, their segment records (ground-truth segments,
    segment order) and BatchFiles with the generator's VAD turns."""
    engine, pipeline, hipabi = pkg('engine'), pkg('pipeline'), pkg('hipabi')
    series = _series()
    frames = np.concatenate([s[0] for s in series])
    foff = np.concatenate([[0], np.cumsum([s[0].shape[0] for s in series])])
    eng = engine.HipEngine(0)
    eng.set_features(frames)
    sets = [[(int(foff[fi] + b), int(foff[fi] + e))] for fi, f in enumerate(GOLD['files']) for b, e, _ in f['segments']]
    d_stats = eng._stats_of_sets(sets)
    files = [pipeline.BatchFile(foff[fi], s[0].shape[0], [(a / GOLD['rate'], b / GOLD['rate']) for a, b in s[1]])
             for fi, s in enumerate(series)]
    d = dict(eng=eng, ctx=eng.ctx, hipabi=hipabi, pipeline=pipeline, frames=frames, foff=foff, d_stats=d_stats,
             n_seg=len(sets), files=files)
    yield d
    eng.ctx.dev_free(d_stats)
    eng.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.gpu
def test_sum_stats_is_a_host_loop_in_member_order_to_the_bit():
    engine, hipabi, synth = pkg('engine'), pkg('hipabi'), pkg('synth')
    feats = synth.make_session(909, 16, 2)[0]
    assert feats.shape[0] == 2000
    n_src = 40
    eng = engine.HipEngine(0)
    bufs = []
    try:
        ctx = eng.ctx
        eng.set_features(feats)
        d_src = eng._stats_of_sets([[(50 * i, 50 * i + 50)] for i in range(n_src)])
        bufs.append(d_src)
        src = np.empty((n_src, hipabi.REC))
        ctx.d2h(src, d_src)
        perm = np.random.default_rng(20261018).permutation(n_src)
        sets = [[5], [39, 0], [1, 8, 15, 22, 29, 36, 3], perm[:33].tolist()]        # interleaved; [39, 0] descends
        assert [len(s) for s in sets] == [1, 2, 7, 33] and sorted(sets[3]) != sets[3]
        member = np.concatenate(sets)
        set_off = np.concatenate([[0], np.cumsum([len(s) for s in sets])])
        d_dst = ctx.dev_alloc(len(sets) * hipabi.REC * 8)
        bufs.append(d_dst)
        ctx.sum_stats(d_src, n_src, member, set_off, d_dst)
        got = np.empty((len(sets), hipabi.REC))
        ctx.d2h(got, d_dst)
        for k, s in enumerate(sets):
            want = src[s[0]].copy()
            for m in s[1:]:
                want = want + src[m]
            assert np.array_equal(_bits(got[k]), _bits(want)), k
        assert got[3, 819] == 33 * 50 and not np.array_equal(got[1], src[39])
        # the order is the caller's: the same members the other way round are another chain of additions
        ctx.sum_stats(d_src, n_src, sets[3][::-1], [0, 33], d_dst)
        back = np.empty((1, hipabi.REC))
        ctx.d2h(back, d_dst)
        want = src[sets[3][-1]].copy()
        for m in sets[3][::-1][1:]:
            want = want + src[m]
        assert np.array_equal(_bits(back[0]), _bits(want))
        assert not np.array_equal(_bits(back[0]), _bits(got[3]))
        # a set of one member is gather_stats' copy
        d_one = ctx.dev_alloc(hipabi.REC * 8)
        bufs.append(d_one)
        ctx.gather_stats(d_src, n_src, [5], d_one, 1)
        one = np.empty((1, hipabi.REC))
        ctx.d2h(one, d_one)
        assert np.array_equal(_bits(one[0]), _bits(got[0]))
        # refusals: SPKD_EINVAL before any device work, d_dst untouched
        mark = np.full((len(sets), hipabi.REC), -7.25)
        ctx.h2d(d_dst, mark)
        bad = [('set_off starts past 0', [0, 1, 2], [1, 3]), ('set_off decreases', [0, 1, 2], [0, 3, 2]),
               ('an empty set', [0, 1], [0, 1, 1, 2]), ('member below 0', [0, -1], [0, 2]),
               ('member past the records', [0, n_src], [0, 2])]
        for what, m, off in bad:
            with pytest.raises(hipabi.SpkdError) as ei:
                ctx.sum_stats(d_src, n_src, m, off, d_dst)
            assert ei.value.status == hipabi.SPKD_EINVAL, what
        with pytest.raises(hipabi.SpkdError) as ei:
            ctx.sum_stats(d_src, n_src, [0, 1], [0, 2], d_src)                      # d_dst aliases d_src
        assert ei.value.status == hipabi.SPKD_EINVAL
        m = np.array([0, 1], dtype=np.int64).ctypes.data_as(C.c_void_p)
        off = np.array([0, 2], dtype=np.int64).ctypes.data_as(C.c_void_p)
        lib, h = ctx.lib, ctx.h
        for args in ((None, n_src, m, off, 1, C.c_void_p(d_dst)), (C.c_void_p(d_src), n_src, None, off, 1, C.c_void_p(d_dst)),
                     (C.c_void_p(d_src), n_src, m, None, 1, C.c_void_p(d_dst)), (C.c_void_p(d_src), n_src, m, off, 1, None),
                     (C.c_void_p(d_src), n_src, m, off, -1, C.c_void_p(d_dst))):
            assert lib.spkd_sum_stats(h, *args) == hipabi.SPKD_EINVAL
        assert lib.spkd_sum_stats(h, C.c_void_p(d_src), n_src, m, off, 0, C.c_void_p(d_dst)) == hipabi.SPKD_OK
        after = np.empty_like(mark)
        ctx.d2h(after, d_dst)
        assert np.array_equal(after, mark)
    finally:
        for p in bufs:
            eng.ctx.dev_free(p)
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASE_NAMES)
def test_link_batch_reproduces_the_reference(dev, name):
    """Merge sequence, maps and partition identical to the reference's; merge distances within the
    relative tolerance test_hip_parity.py applies to merge distances (its _same_merges)."""
    from test_hip_parity import _same_merges
    case = GOLD['cases'][CASE_NAMES.index(name)]
    timings = {}
    maps, merges, smax, smin = dev['pipeline'].link_batch(dev['ctx'], dev['d_stats'], _golden_seg_off(), _golden_labels(),
                                                          _case_cl(case), timings)
    want = [(a, b, float.fromhex(d)) for a, b, d in case['merges']]
    for (_, _, d), (_, _, w) in zip(merges, want):
        print('%s: merge distance %r, reference %r' % (name, d, w))
    _same_merges(merges, want)
    ids = _global_ids(case)
    _, _, spk_file, spk_label = dev['pipeline'].link_speakers(_golden_seg_off(), _golden_labels())
    got = np.array([maps[f][l] for f, l in zip(spk_file, spk_label)])
    assert got.tolist() == ids.tolist()
    assert [m.tolist() for m in maps] == [[0] + ids[3 * f:3 * f + 3].tolist() for f in range(3)]
    assert timings['link_speakers'] == len(ids) and timings['link_merges'] == len(want)
    assert len(timings['link_sum']) == 1 and len(timings['link_ahc']) == 1
    assert smax >= smin


def _rows(d, **kw):
    return d['pipeline'].diarize_batch(d['ctx'], d['eng'].d_frames, d['frames'].shape[0], kw.pop('files', d['files']),
                                       rate=GOLD['rate'], **kw)


def _direct(d, cd, cl, files=None):
    """change_detect_batch + cluster_batch + link_batch, called one by one -> (labels per file, maps, merges)."""
    p, files = d['pipeline'], files or d['files']
    segs = p.change_detect_batch(d['ctx'], d['eng'].d_frames, d['frames'].shape[0], files, GOLD['rate'], cd)
    box = []
    res = p.cluster_batch(d['ctx'], d['eng'].d_frames, d['frames'].shape[0], files, segs, GOLD['rate'], cl, stats_out=box)
    labels = [lab for lab, _ in res]
    maps, merges, _, _ = p.link_batch(d['ctx'], box[0][0], box[0][1], labels, p.LINK_CL)
    return labels, maps, merges


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['gw_hi', 'gw_in', 'sw_hi'])
def test_diarize_batch_with_link_end_to_end(dev, mode):
    p = dev['pipeline']
    cd = p.SW_CD if mode == 'sw_hi' else p.DIA2_CD
    cl = dict(p.DIA2_CL, method='in') if mode == 'gw_in' else p.DIA2_CL
    plain = _rows(dev, cd=cd, cl=cl)
    det = {}
    linked = _rows(dev, cd=cd, cl=cl, link=p.LINK_CL, detail=det)
    maps = det['link']['maps']
    assert len(plain) == len(linked) == 3 and all(len(r) for r in plain)
    for f in range(3):
        assert plain[f][:, :2].tobytes() == linked[f][:, :2].tobytes()
        assert np.array_equal(linked[f][:, 2], maps[f][plain[f][:, 2].astype(np.int64)])
        assert linked[f][:, 2].min() >= 1
    # the same global ids as link_batch gives when it is handed the stage's labels directly
    labels, maps_direct, merges_direct = _direct(dev, cd, cl)
    assert [m.tolist() for m in maps_direct] == [m.tolist() for m in maps]
    assert merges_direct == det['link']['merges']
    assert [sorted(set(l.tolist())) for l in labels] == [sorted(set(r[:, 2].astype(int).tolist())) for r in plain]
    if mode == 'gw_hi':
        # ground-truth-like input: the two recurring speakers are found in every file
        shared = set(linked[0][:, 2]) & set(linked[1][:, 2]) & set(linked[2][:, 2])
        assert len(shared) >= 2
        # link=None is the call without the argument, and the rows of the stages called one by one
        again = _rows(dev, cd=cd, cl=cl, link=None)
        assert [r.tobytes() for r in again] == [r.tobytes() for r in plain]
        with pytest.raises(ValueError, match='link takes the host hand-off'):
            _rows(dev, cd=cd, cl=cl, link=p.LINK_CL, fused=True)
        with pytest.raises(ValueError, match='link takes the host hand-off'):
            _rows(dev, cd=cd, cl=cl, link=p.LINK_CL, fused=True, handoff='device')
        fused_host = _rows(dev, cd=cd, cl=cl, link=p.LINK_CL, fused=True, handoff='host')
        assert [r[:, :2].tobytes() for r in fused_host] == [r[:, :2].tobytes() for r in plain]


@pytest.mark.gpu
def test_link_edges(dev):
    p, ctx, hipabi = dev['pipeline'], dev['ctx'], dev['hipabi']
    # a file without a segment in the middle of the batch: its map is empty, the others link as a batch of two
    f0, f1, f2 = dev['files']
    hole = p.BatchFile(f1.frame_off, f1.n_frames, [])
    det, det2 = {}, {}
    rows = _rows(dev, files=[f0, hole, f2], link=p.LINK_CL, detail=det)
    rows2 = _rows(dev, files=[f0, f2], link=p.LINK_CL, detail=det2)
    assert len(rows[1]) == 0 and len(det['link']['maps'][1]) == 0
    assert rows[0].tobytes() == rows2[0].tobytes() and rows[2].tobytes() == rows2[1].tobytes()
    assert det['link']['merges'] == det2['link']['merges'] and len(det['link']['merges']) >= 2
    # one speaker in total: one record, no merge
    maps, merges, _, _ = p.link_batch(ctx, dev['d_stats'], [0, 1], [np.array([1])])
    assert [m.tolist() for m in maps] == [[0, 1]] and merges == []
    maps, merges, _, _ = p.link_batch(ctx, dev['d_stats'], [0, 0, 3, 3], [np.zeros(0, int), np.array([2, 2, 2]), np.zeros(0, int)])
    assert [m.tolist() for m in maps] == [[], [0, 0, 1], []] and merges == []
    # a record that is not finite raises what cluster_batch raises
    bad = np.empty((4, hipabi.REC))
    ctx.d2h(bad, dev['d_stats'])
    bad[2, 17] = np.nan
    d_bad = ctx.dev_alloc(bad.nbytes)
    try:
        ctx.h2d(d_bad, bad)
        with pytest.raises(ValueError, match='array must not contain infs or NaNs'):
            p.link_batch(ctx, d_bad, [0, 2, 4], [np.array([1, 2]), np.array([1, 1])])
    finally:
        ctx.dev_free(d_bad)


@pytest.mark.gpu
def test_all_zero_frames_link_as_they_cluster(dev):
    """Digital silence: the records of all-zero frames are finite (zeros and a count) and their
    covariance is zero, which spk_cluster_hi takes as numpy does (-inf log det, NaN or inf
    distances: test_hip_parity.py pins it).  link_batch over speakers of one segment each is
    spkd_ahc over those records: whatever that call does with them -- the same merges, or the
    same ValueError -- link_batch does."""
    p, ctx, hipabi = dev['pipeline'], dev['ctx'], dev['hipabi']
    eng = pkg('engine').HipEngine(0)
    try:
        f = dev['frames'][:6000].copy()
        f[1000:2000] = 0.0
        f[4000:5000] = 0.0
        eng.set_features(f)
        d_rec = eng._stats_of_sets([[(1000 * i, 1000 * i + 1000)] for i in range(6)])
        outcome = []
        for call in (lambda: eng.ctx.ahc(d_rec, [0, 6], p._ahc_params(p.LINK_CL)),
                     lambda: p.link_batch(eng.ctx, d_rec, [0, 3, 6], [np.array([1, 2, 3])] * 2)):
            try:
                r = call()
                if isinstance(r, dict):
                    nm = int(r['n_merges'][0])
                    outcome.append(('status', r['status'], list(zip(r['a'][:nm].tolist(), r['b'][:nm].tolist()))))
                else:
                    outcome.append(('status', hipabi.SPKD_OK, [(a, b) for a, b, _ in r[1]]))
            except ValueError as e:
                outcome.append(('ValueError', str(e)))
        print(outcome)
        if outcome[0][0] == 'status' and outcome[0][1] == hipabi.SPKD_ENONFINITE:
            assert outcome[1] == ('ValueError', 'array must not contain infs or NaNs')
        else:
            assert outcome[0] == outcome[1]
        eng.ctx.dev_free(d_rec)
    finally:
        eng.close()
