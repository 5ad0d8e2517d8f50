"""The speaker gallery: spkd_clr_identify (a batch's speakers against enrolled ones: the score matrix and
the open-set, one-to-one assignment), spkd_bw_accumulate (ordered sums of records), gallery.Gallery and
pipeline.link_batch / diarize_batch with link = dict(LINK_CLR, gallery=...).
PARITY: no reference counterpart; the numpy restatement is tests/gallery_numpy.py."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import gallery_numpy as GN
import link_clr_numpy as L
import reseg_gmm_numpy as G
from helpers import ROOT
from conftest import pkg
from test_reseg_batch import _Dev, _close
from test_link_clr import _hand_records, _ptr, RATE

GAP = 1e-6          # what every decision of a fixture keeps from its threshold and from its runner-up


# ------------------------------------------------------------------ not GPU
def test_entry_points_timers_and_constants_are_declared_and_exported():
    hipabi, pipeline = pkg('hipabi'), pkg('pipeline')
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'spkd.h')).read(), flags=re.S)
    lib = hipabi.load_library()
    for name in ('spkd_clr_identify', 'spkd_bw_accumulate'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in hipabi.EXPORTS and hasattr(lib, name)
    assert hasattr(hipabi.Context, 'clr_identify') and hasattr(hipabi.Context, 'bw_accumulate')
    assert lib.spkd_abi_version() == 2 and re.search(r'#define SPKD_ABI_VERSION 2\b', code)
    enum = re.search(r'enum \{\s*SPKD_T_CALL = 0,(.*?)SPKD_N_TIMERS', code, flags=re.S).group(1)
    names = ['call'] + [n.strip()[len('SPKD_T_'):].lower() for n in enum.split(',') if n.strip()]
    # behind fb_posterior; the front-end's two stay the last
    assert names[names.index('fb_posterior') + 1:] == ['ident_scores', 'ident_assign', 'bw_accumulate', 'mfcc_static', 'mfcc_post']
    assert [n for n, _ in sorted(hipabi.TIMERS.items(), key=lambda kv: kv[1])] == names
    kern = open(os.path.join(ROOT, 'speaker-diarization_amd', 'csrc', 'spkd_ident.hpp')).read()
    header = int(re.search(r'#define SPKD_GALLERY_MAX_N (\d+)', code).group(1))
    kernel = int(re.search(r'constexpr int ID_MAX_G = (\d+);', kern).group(1))
    assert header == kernel == hipabi.GALLERY_MAX_N == GN.GALLERY_MAX_N == 16384
    assert GN.MAX_N == hipabi.CLR_MAX_N == int(re.search(r'#define SPKD_CLR_MAX_N (\d+)', code).group(1))
    for text in (kern, GN.__doc__, pkg('gallery').__doc__):
        assert 'PARITY: no reference counterpart' in text
    # the score is spkd_clr.hpp's, not restated
    assert 'clr_derive(' in kern and 'clr_pair(' in kern and 'fma(' not in kern
    assert pipeline.LINK_CLR == dict(model='clr', components=8, iterations=5, var_floor=0.01, relevance=16.0,
                                     threshold=-0.5, max_spk=0, ubm_max_frames=2_000_000)
    assert pipeline.LINK_CL == dict(variant=1, kind='BIC', lambdac=1.3, threshold=0.0, max_spk=0)


def _refusals():
    """(name, call(lib, ctx handle) -> status) of every argument refusal of the two entry points."""
    dev = C.c_void_p(4096)                        # never dereferenced: the refusal comes first
    odd = C.c_void_p(4104)
    pok, gok = np.ones(4, dtype=np.int32), np.ones(3, dtype=np.int32)
    out_i, out_d = np.zeros(8, dtype=np.int32), np.zeros(8)
    keep = {}
    q = lambda v: None if v is None else _ptr(v)

    def ident(probe=dev, n=4, h_pok=pok, off=(0, 1, 4), n_groups=None, gal=dev, n_gal=3, h_gok=gok, ubm=dev, K=2, r=16.0,
              th=-0.5, excl=1, i=out_i, s=out_d, s2=out_d, scores=None):
        arr = None if off is None else np.array(off, dtype=np.int64)
        keep[len(keep)] = arr
        ng = (len(off) - 1 if off is not None else 2) if n_groups is None else n_groups
        return lambda lib, h: lib.spkd_clr_identify(h, probe, n, q(h_pok), ng, q(arr), gal, n_gal, q(h_gok), ubm, K, r, th,
                                                    excl, q(i), q(s), q(s2), scores)

    def acc(src=dev, n_src=5, K=2, off=(0, 1, 3), member=(0, 4, 2), slot=(1, 0), kp=(1, 0), dst=dev, n_dst=2, n_sets=None):
        arrs = [None if off is None else np.array(off, dtype=np.int64)] + [
            None if v is None else np.array(v, dtype=np.int32) for v in (member, slot, kp)]
        keep[len(keep)] = arrs
        ns = (len(off) - 1 if off is not None else 2) if n_sets is None else n_sets
        return lambda lib, h: lib.spkd_bw_accumulate(h, src, n_src, K, ns, q(arrs[0]), q(arrs[1]), q(arrs[2]), q(arrs[3]),
                                                     dst, n_dst)

    return [
        ('identify: null probes', ident(probe=None)), ('identify: null probe ok', ident(h_pok=None)),
        ('identify: null offsets', ident(off=None)), ('identify: null gallery', ident(gal=None)),
        ('identify: null gallery ok', ident(h_gok=None)), ('identify: null model', ident(ubm=None)),
        ('identify: null ident', ident(i=None)), ('identify: null score', ident(s=None)),
        ('identify: null second', ident(s2=None)),
        ('identify: negative probe count', ident(n=-1)), ('identify: negative gallery count', ident(n_gal=-1)),
        ('identify: negative group count', ident(n_groups=-1)), ('identify: no group', ident(n_groups=0)),
        ('identify: more probes than the limit', ident(n=4097, off=(0, 4097))),
        ('identify: more identities than the limit', ident(n_gal=16385)),
        ('identify: offsets not from 0', ident(off=(1, 2, 4))), ('identify: offsets go back', ident(off=(0, 3, 2, 4))),
        ('identify: offsets end early', ident(off=(0, 1, 3))), ('identify: offsets end late', ident(off=(0, 1, 5))),
        ('identify: no component', ident(K=0)), ('identify: a 9th component', ident(K=9)),
        ('identify: relevance 0', ident(r=0.0)), ('identify: negative relevance', ident(r=-1.0)),
        ('identify: relevance NaN', ident(r=float('nan'))), ('identify: relevance inf', ident(r=float('inf'))),
        ('identify: threshold NaN', ident(th=float('nan'))),
        ('identify: exclusive 2', ident(excl=2)), ('identify: exclusive -1', ident(excl=-1)),
        ('identify: misaligned probes', ident(probe=odd)), ('identify: misaligned gallery', ident(gal=odd)),
        ('identify: misaligned model', ident(ubm=odd)), ('identify: misaligned scores', ident(scores=odd)),
        ('sum: null source', acc(src=None)), ('sum: null offsets', acc(off=None)), ('sum: null members', acc(member=None)),
        ('sum: null slots', acc(slot=None)), ('sum: null keep', acc(kp=None)), ('sum: null destination', acc(dst=None)),
        ('sum: negative set count', acc(n_sets=-1)), ('sum: negative source count', acc(n_src=-1)),
        ('sum: negative slot count', acc(n_dst=-1)),
        ('sum: no component', acc(K=0)), ('sum: a 9th component', acc(K=9)),
        ('sum: offsets not from 0', acc(off=(1, 2, 3))), ('sum: offsets go back', acc(off=(0, 2, 1), member=(0, 4))),
        ('sum: member below 0', acc(member=(0, -1, 2))), ('sum: member past the source', acc(member=(0, 5, 2))),
        ('sum: slot below 0', acc(slot=(-1, 0))), ('sum: slot past the destination', acc(slot=(1, 2))),
        ('sum: a slot named twice', acc(slot=(1, 1))),
        ('sum: misaligned source', acc(src=odd)), ('sum: misaligned destination', acc(dst=odd)),
    ]


def test_every_refusal_is_einval_without_a_context():
    hipabi = pkg('hipabi')
    lib = hipabi.load_library()
    for name, call in _refusals():
        assert call(lib, None) == hipabi.SPKD_EINVAL, name


def test_restated_greedy_on_a_hand_written_matrix():
    """Rows 0 and 1 both prefer column 0; row 0's score is the higher."""
    mat = np.array([[5.0, 1.0, -3.0],
                    [4.0, 2.0, -2.0],
                    [-1.0, -4.0, 0.5]])
    ok = np.ones(3, dtype=np.int32)
    ident, score, second = GN.assign(mat, ok, ok, [0, 3], 0.0)
    assert ident.tolist() == [0, 1, 2] and score.tolist() == [5.0, 2.0, 0.5] and second.tolist() == [1.0, 4.0, -1.0]
    # the loser's second choice below the threshold: unknown, its score the highest of the row
    ident, score, second = GN.assign(mat, ok, ok, [0, 3], 3.0)
    assert ident.tolist() == [0, -1, -1] and score.tolist() == [5.0, 4.0, 0.5] and second.tolist() == [1.0, 2.0, -1.0]
    # without the constraint, and as groups of their own: both take column 0
    for got in (GN.assign(mat, ok, ok, [0, 3], 0.0, exclusive=False), GN.assign(mat, ok, ok, [0, 1, 2, 3], 0.0)):
        assert got[0].tolist() == [0, 0, 2] and got[1].tolist() == [5.0, 4.0, 0.5] and got[2].tolist() == [1.0, 2.0, -1.0]
    # a tie between rows: the first in row-major order; between columns: the lowest
    tie = np.array([[2.0, 2.0], [2.0, 2.0]])
    assert GN.assign(tie, ok[:2], ok[:2], [0, 2], 0.0)[0].tolist() == [0, 1]
    assert GN.assign(tie, ok[:2], ok[:2], [0, 2], 0.0, exclusive=False)[0].tolist() == [0, 0]
    # a row and a column that are not ok; one identity: no second
    ident, score, second = GN.assign(mat, [1, 0, 1], [0, 1, 1], [0, 3], -10.0)
    assert ident.tolist() == [1, -1, 2] and np.isnan(score[1]) and np.isnan(second[1]) and second[0] == -3.0
    one = GN.assign(mat[:, :1], ok, ok[:1], [0, 3], 0.0)
    assert one[0].tolist() == [0, -1, -1] and one[1].tolist() == [5.0, 4.0, -1.0] and np.isnan(one[2]).all()
    assert GN.margins(mat, ok, ok, [0, 3], 0.0) == (0.5, 1.0)
    # the ordered sum
    src = np.arange(24, dtype=np.float64).reshape(4, 2, 3) * 0.1
    dst = GN.bw_accumulate(src, [0, 2, 3], [3, 0, 1], [1, 0], [1, 0], np.ones((2, 2, 3)))
    assert np.array_equal(dst[1], (np.ones((2, 3)) + src[3]) + src[0]) and np.array_equal(dst[0], np.zeros((2, 3)) + src[1])


def test_gallery_arrays_round_trip_without_a_device(tmp_path):
    gallery, hipabi, pipeline = pkg('gallery'), pkg('hipabi'), pkg('pipeline')
    ubm, rec, _ = _hand_records(5, 3, 2, 4)
    arrays = dict(version=np.array(gallery.FORMAT_VERSION), components=np.array(4), relevance=np.array(12.0),
                  threshold=np.array(-0.25), ubm=ubm, records=rec, ok=np.array([1, 0, 1], dtype=np.int32),
                  frames=rec[:, :, 0].sum(axis=1), names=np.array(['anchor', 'spk_2', 'chair']))
    g = gallery.Gallery.from_arrays(None, arrays)
    assert (g.n, g.components, g.relevance, g.threshold, g.names) == (3, 4, 12.0, -0.25, ['anchor', 'spk_2', 'chair'])
    back = g.to_arrays()
    assert sorted(back) == sorted(arrays)
    for k in arrays:
        assert np.array_equal(back[k], arrays[k]) and back[k].shape == np.asarray(arrays[k]).shape, k
    path = str(tmp_path / 'people.npz')
    g.save(path)
    with np.load(path, allow_pickle=False) as z:                        # (nothing pickled in the file)
        assert sorted(z.files) == sorted(arrays)
    again = gallery.Gallery.load(None, path).to_arrays()
    for k in arrays:
        assert again[k].tobytes() == back[k].tobytes() and again[k].dtype == back[k].dtype, k
    # an empty gallery without a model, and its defaults
    e = gallery.Gallery(None)
    assert (e.n, e.ubm, e.components, e.relevance, e.threshold) == (0, None, 8, 16.0, pipeline.LINK_CLR['threshold'])
    e2 = gallery.Gallery.from_arrays(None, e.to_arrays())
    assert e2.n == 0 and e2.ubm is None and e2.names == []
    assert gallery.default_name(0) == 'spk_1'
    # what is refused
    bad = [dict(version=np.array(gallery.FORMAT_VERSION + 1)), dict(records=rec[:2]), dict(records=rec[:, :3]),
           dict(ok=np.ones(4, dtype=np.int32)), dict(names=np.array(['a', 'b'])), dict(ubm=ubm[:3]), dict(components=np.array(3)),
           dict(frames=np.zeros(2)), dict(ubm=np.zeros((0, hipabi.GMM_COMP)))]
    for change in bad:
        with pytest.raises(ValueError, match='gallery|link components'):
            gallery.Gallery.from_arrays(None, dict(arrays, **change))
    with pytest.raises(ValueError, match='gallery: no names'):
        gallery.Gallery.from_arrays(None, {k: v for k, v in arrays.items() if k != 'names'})
    # the model may change only while nobody is enrolled
    with pytest.raises(ValueError, match='holds identities'):
        g.set_ubm(ubm)
    with pytest.raises(ValueError, match='holds identities'):
        g.train_ubm(0, 0, [0], [], [])
    with pytest.raises(ValueError, match='no model'):
        e.identify(0, [1], [0, 1])
    with pytest.raises(ValueError, match='no model'):
        e.update(0, [1], [-1])
    with pytest.raises(ValueError, match='at most'):
        g.update(0, np.ones(hipabi.GALLERY_MAX_N, dtype=np.int32), np.full(hipabi.GALLERY_MAX_N, -1))
    assert g.n == 3


def test_refusals_of_the_pipeline_need_no_device():
    pipeline, gallery = pkg('pipeline'), pkg('gallery')
    files = [pipeline.BatchFile(0, 1000, [(0.0, 8.0)])]
    segments = [np.array([(0.0, 4.0), (4.0, 8.0)])]
    labels = [np.array([1, 2])]
    g4 = gallery.Gallery(None, dict(pipeline.LINK_CLR, components=4))
    g8 = gallery.Gallery(None, dict(pipeline.LINK_CLR, relevance=8.0))
    bad = [(dict(pipeline.LINK_CLR, gallery=g4), 'link components'), (dict(pipeline.LINK_CLR, gallery=g8), 'link relevance'),
           (dict(pipeline.LINK_CLR, gallery=object()), 'link gallery'), (dict(pipeline.LINK_CLR, gallery={}), 'link gallery'),
           (dict(pipeline.LINK_CL, gallery=g4), 'link gallery')]
    for link, match in bad:
        with pytest.raises(ValueError, match=match):
            pipeline.link_batch(None, 0, [0, 2], labels, link, d_frames=0, total_frames=1000, files=files, segments=segments)
        with pytest.raises(ValueError, match=match):
            pipeline.diarize_batch(None, 0, 0, [], link=link)
    # the keys of the link are checked as without a gallery
    with pytest.raises(ValueError, match='link threshold'):
        pipeline.diarize_batch(None, 0, 0, [], link=dict(pipeline.LINK_CLR, gallery=g4, threshold=float('nan')))
    with pytest.raises(ValueError, match='a gallery holds the records'):
        gallery.Gallery(None, pipeline.LINK_CL)
    # nothing to link: no device work, the gallery untouched
    ok = gallery.Gallery(None)
    det = {}
    assert pipeline.diarize_batch(None, 0, 0, [], link=dict(pipeline.LINK_CLR, gallery=ok), detail=det) == []
    assert det['link']['merges'] == [] and ok.n == 0 and ok.ubm is None


# ------------------------------------------------------------------ the people of three batches, restated
PEOPLE_SEEDS = dict(A=((11, 777), (12, 777)), B=((13, 777), (14, 778)), C=((16, 778), (15, 777)))


@functools.lru_cache(maxsize=None)
def _batches():
    """The sessions of batches A, B and C in ONE frame array: 60 s files of two bimodal people each, the
    people of model seed 777 being persons 0 and 1 and those of 778 persons 2 and 3.  Returns (frames,
    {batch: (first frame of each file, sessions, speakers as range lists, the person of each speaker)})."""
    synth = pkg('synth')
    models = {m: [synth._speaker_model(m, k) for k in range(4)] for m in (777, 778)}
    feats, out, at = [], {}, 0
    for name in 'ABC':
        sess = [synth.make_session(seed, 60.0, 4, models=models[m]) for seed, m in PEOPLE_SEEDS[name]]
        first, speakers, person = [], [], []
        for s, (_, m) in zip(sess, PEOPLE_SEEDS[name]):
            first.append(at)
            for p in (0, 1):
                speakers.append([(at + a, at + b) for a, b, k in s[2] if k // 2 == p])
                person.append(p + (2 if m == 778 else 0))
            feats.append(s[0])
            at += len(s[0])
        out[name] = (first, sess, speakers, person)
    return np.concatenate(feats), out


@functools.lru_cache(maxsize=None)
def _restated_flow():
    """Batch A, B and C through the restatement with one gallery, and B without enrolment between A and
    B: {name: gallery_numpy.link's result}, the gallery's records after each."""
    pipeline = pkg('pipeline')
    feats, batches = _batches()
    gal = GN.Gallery(pipeline.LINK_CLR)
    out = {}
    for name in ('A', 'B-', 'B', 'C'):
        out[name] = GN.link(feats, batches[name[0]][2], pipeline.LINK_CLR, gal, enrol=not name.endswith('-'))
        out[name]['records'] = gal.records.copy()
    return out


def test_restated_gallery_names_the_people_across_batches():
    """What the feature is for, in numpy alone: the labels are the persons' in every batch, and no decision
    sits closer than GAP to the threshold or to its runner-up."""
    _, batches = _batches()
    flow = _restated_flow()
    want = dict(A=[1, 2, 1, 2], B=[1, 2, 3, 4], C=[3, 4, 1, 2])
    th = pkg('pipeline').LINK_CLR['threshold']
    for name in ('A', 'B-', 'B', 'C'):
        r = flow[name]
        assert [p + 1 for p in batches[name[0]][3]] == want[name[0]]
        assert r['labels'].tolist() == want[name[0]], name
        assert len(r['records']) == dict(A=2, B=4, C=4)[name[0]] - (2 if name == 'B-' else 0), name
        if r['mat'].size:
            to_th, to_next = GN.margins(r['mat'], r['cluster_ok'], np.ones(r['mat'].shape[1]), [0, len(r['mat'])], th)
            print('batch %s: scores\n%s\nleast gap to the threshold %.3f, to a runner-up %.3f' % (name, r['mat'].round(3), to_th, to_next))
            assert to_th >= GAP and to_next >= GAP, name
    assert flow['A']['enrolled'] == [0, 1] and flow['B']['enrolled'] == [2, 3] and flow['C']['enrolled'] == []
    assert flow['B-']['enrolled'] == [] and flow['B-']['identity'].tolist() == [0, 1, -1, -1]
    assert flow['B-']['records'].tobytes() == flow['A']['records'].tobytes()


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def dev():
    feats, _ = _batches()
    d = _Dev(feats)
    yield d
    d.close()


def _upload(dev, arr):
    arr = np.ascontiguousarray(arr, dtype=np.float64)
    p = dev.alloc(max(arr.nbytes, 16))
    if arr.nbytes:
        dev.ctx.h2d(p, arr)
    return p


def _identify(dev, ubm, probes, pok, off, gal, gok, r, th, exclusive=True):
    """spkd_clr_identify on the device -> (result, matrix); the records are not modified."""
    d_ubm, d_p, d_g = _upload(dev, ubm), _upload(dev, probes), _upload(dev, gal)
    mat = np.full((len(probes), len(gal)), -7.0)
    d_mat = _upload(dev, mat)
    got = dev.ctx.clr_identify(d_p, pok, off, d_g, gok, d_ubm, len(ubm), r, th, exclusive, d_scores=d_mat)
    if mat.size:
        dev.ctx.d2h(mat, d_mat)
    for d_x, x in ((d_p, probes), (d_g, gal)):
        after = np.empty_like(x)
        if x.size:
            dev.ctx.d2h(after, d_x)
        assert after.tobytes() == x.tobytes()
    return got, mat


def _same(got, mat, want):
    ident, score, second, wmat, fin = want
    assert fin and got['status'] == 0
    assert np.array_equal(np.isnan(mat), np.isnan(wmat)) and _close(mat[~np.isnan(wmat)], wmat[~np.isnan(wmat)])
    assert got['ident'].tolist() == ident.tolist()
    for g, w in ((got['score'], score), (got['second'], second)):
        assert np.array_equal(np.isnan(g), np.isnan(w)) and _close(g[~np.isnan(w)], w[~np.isnan(w)])


def _decided(wmat, pok, gok, off, th, exclusive, ties=False):
    """The fixture's own condition, in numpy: no decision within GAP of the threshold or of its runner-up."""
    to_th, to_next = GN.margins(wmat, pok, gok, off, th, exclusive)
    assert to_th >= GAP and (ties or to_next >= GAP), (to_th, to_next)


@pytest.mark.gpu
@pytest.mark.parametrize('K', [1, 3, 8])
def test_scores_and_assignment_match_the_restatement(dev, K):
    S, Gn, r, th = 37, 19, 16.0, -0.5
    ubm, rec, who = _hand_records(300 + K, S + Gn, 10, K)
    probes, gal = rec[:S], rec[S:]
    off = np.cumsum([0, 1, 2, 5, 13, 16])
    assert off[-1] == S
    pok, gok = np.ones(S, dtype=np.int32), np.ones(Gn, dtype=np.int32)
    pok[[4, 30]] = 0
    gok[[0, 11]] = 0
    for exclusive in (True, False):
        want = GN.identify(probes, pok, off, gal, gok, ubm, r, th, exclusive)
        _decided(want[3], pok, gok, off, th, exclusive)
        got, mat = _identify(dev, ubm, probes, pok, off, gal, gok, r, th, exclusive)
        print('K %d exclusive %d: ident %s' % (K, exclusive, got['ident'].tolist()))
        _same(got, mat, want)
        assert (got['ident'][[4, 30]] == -1).all() and np.isnan(got['score'][[4, 30]]).all() and np.isnan(mat[4]).all()
        assert not set(got['ident'].tolist()) & {0, 11} and np.isnan(mat[:, 11]).all() and (got['ident'] >= 0).any()
        assert dev.ctx.last_ms('ident_scores') > 0.0 and dev.ctx.last_ms('ident_assign') > 0.0
        if exclusive:                                                  # distinct identities inside every group
            for a, b in zip(off[:-1], off[1:]):
                known = [i for i in got['ident'][a:b].tolist() if i >= 0]
                assert len(known) == len(set(known))
        # a threshold above and below every score
        none, _ = _identify(dev, ubm, probes, pok, off, gal, gok, r, 1e9, exclusive)
        _same(none, mat, GN.identify(probes, pok, off, gal, gok, ubm, r, 1e9, exclusive))
        assert (none['ident'] == -1).all() and _close(none['score'][pok != 0], np.nanmax(mat[pok != 0], axis=1))
        every, _ = _identify(dev, ubm, probes, pok, off, gal, gok, r, -1e9, exclusive)
        _same(every, mat, GN.identify(probes, pok, off, gal, gok, ubm, r, -1e9, exclusive))
        assert (every['ident'][pok != 0] >= 0).sum() == (int((pok != 0).sum()) if not exclusive else
                                                         sum(min(int(pok[a:b].sum()), int(gok.sum())) for a, b in zip(off[:-1], off[1:])))
        # one identity: no second; nobody enrolled: everybody unknown, no launch
        want1 = GN.identify(probes, pok, off, gal[1:2], gok[1:2], ubm, r, th, exclusive)
        _decided(want1[3], pok, gok[1:2], off, th, exclusive)
        got1, mat1 = _identify(dev, ubm, probes, pok, off, gal[1:2], gok[1:2], r, th, exclusive)
        _same(got1, mat1, want1)
        assert np.isnan(got1['second']).all() and set(got1['ident'].tolist()) <= {-1, 0}
        got0, _ = _identify(dev, ubm, probes, pok, off, gal[:0], gok[:0], r, th, exclusive)
        assert got0['status'] == 0 and (got0['ident'] == -1).all() and np.isnan(got0['score']).all() and np.isnan(got0['second']).all()


@pytest.mark.gpu
def test_more_rows_and_columns_than_a_wave_or_a_tile(dev):
    S, Gn, K, r, th = 70, 130, 8, 16.0, -0.5
    ubm, rec, _ = _hand_records(41, S + Gn, 90, K)
    probes, gal = rec[:S], rec[S:]
    pok, gok = np.ones(S, dtype=np.int32), np.ones(Gn, dtype=np.int32)
    gok[[64, 129]] = 0
    want = GN.identify(probes, pok, [0, S], gal, gok, ubm, r, th)
    _decided(want[3], pok, gok, [0, S], th, True)
    got, mat = _identify(dev, ubm, probes, pok, [0, S], gal, gok, r, th)
    _same(got, mat, want)
    known = [i for i in got['ident'].tolist() if i >= 0]
    print('%d of %d probes known' % (len(known), S))
    assert 10 < len(known) == len(set(known)) and max(known) > 64 and (got['ident'] == -1).any()


def _of(who, person, k):
    idx = np.nonzero(who == person)[0][:k]
    assert len(idx) == k
    return idx


@pytest.mark.gpu
def test_exact_ties_go_to_the_lower_index(dev):
    K, r, th = 8, 16.0, -0.5
    ubm, rec, who = _hand_records(77, 40, 4, K)
    p0 = _of(who, 0, 2)
    gal = np.array([rec[_of(who, 1, 1)[0]], rec[_of(who, 2, 1)[0]], rec[p0[0]], rec[_of(who, 3, 1)[0]], rec[_of(who, 1, 2)[1]],
                    rec[p0[0]]])                                        # identities 2 and 5: the same record
    probes = np.array([rec[p0[1]], rec[p0[1]], rec[_of(who, 3, 2)[1]]])   # probes 0 and 1: the same record
    pok, gok = np.ones(3, dtype=np.int32), np.ones(6, dtype=np.int32)
    for off, exclusive, ident in (([0, 3], True, [2, 5, 3]), ([0, 3], False, [2, 2, 3]), ([0, 1, 2, 3], True, [2, 2, 3])):
        want = GN.identify(probes, pok, off, gal, gok, ubm, r, th, exclusive)
        assert want[3][0, 2] == want[3][0, 5] == want[3][1, 2] == want[3][1, 5] > th
        _decided(want[3], pok, gok, off, th, exclusive, ties=True)
        got, mat = _identify(dev, ubm, probes, pok, off, gal, gok, r, th, exclusive)
        _same(got, mat, want)
        assert got['ident'].tolist() == ident
        assert mat[0, 2] == mat[0, 5] == mat[1, 2] == mat[1, 5]          # the bits of a pair do not depend on its place
        assert got['score'][0] == got['second'][0] == got['score'][1] == got['second'][1] == mat[0, 2]


@pytest.mark.gpu
def test_the_constraint_bites(dev):
    K, r, th = 8, 16.0, -0.5
    ubm, rec, who = _hand_records(78, 40, 4, K)
    p0 = _of(who, 0, 3)
    gal = np.array([rec[_of(who, 1, 1)[0]], rec[p0[0]], rec[_of(who, 2, 1)[0]], rec[_of(who, 3, 1)[0]]])
    probes = np.array([rec[p0[1]], rec[p0[2]]])                          # two records of the person of identity 1
    pok, gok = np.ones(2, dtype=np.int32), np.ones(4, dtype=np.int32)
    wmat = GN.scores(probes, pok, gal, gok, ubm, r)[0]
    assert (np.argmax(wmat, axis=1) == 1).all() and (wmat[:, 1] > th).all() and (np.delete(wmat, 1, axis=1) < th).all()
    win = int(np.argmax(wmat[:, 1]))
    lose = 1 - win
    runner = int(np.argmax(np.where(np.arange(4) == 1, -np.inf, wmat[lose])))
    cases = [([0, 2], th, {win: 1, lose: -1}),                           # the loser's second choice is below the threshold
             ([0, 2], -1e9, {win: 1, lose: runner}),                     # ... and above it
             ([0, 1, 2], th, {win: 1, lose: 1})]                         # groups of their own: both get the column
    for off, t, ident in cases:
        want = GN.identify(probes, pok, off, gal, gok, ubm, r, t)
        _decided(want[3], pok, gok, off, t, True)
        got, mat = _identify(dev, ubm, probes, pok, off, gal, gok, r, t)
        _same(got, mat, want)
        assert got['ident'].tolist() == [ident[0], ident[1]], (off, t)
    # the loser, unknown: its score is still the row's highest, its second the runner-up's
    got, mat = _identify(dev, ubm, probes, pok, [0, 2], gal, gok, r, th)
    assert got['score'][lose] == mat[lose, 1] and got['second'][lose] == mat[lose, runner]
    # the loser on its second choice: `second` is the column it lost
    got, mat = _identify(dev, ubm, probes, pok, [0, 2], gal, gok, r, -1e9)
    assert got['score'][lose] == mat[lose, runner] and got['second'][lose] == mat[lose, 1]


@pytest.mark.gpu
def test_a_record_that_is_not_finite_and_every_refusal_with_a_context(dev):
    hipabi, K, r, th = dev.hipabi, 8, 16.0, -0.5
    ubm, rec, _ = _hand_records(9, 16, 3, K)
    probes, gal = rec[:9], rec[9:].copy()
    pok, gok = np.ones(9, dtype=np.int32), np.ones(7, dtype=np.int32)
    gal[4, 3, 11] = np.nan
    off = [0, 4, 9]
    got, _ = _identify(dev, ubm, probes, pok, off, gal, gok, r, th)
    assert got['status'] == hipabi.SPKD_ENONFINITE and (got['ident'] == -1).all()
    assert np.isnan(got['score']).all() and np.isnan(got['second']).all()
    assert not GN.identify(probes, pok, off, gal, gok, ubm, r, th)[4]
    # the same identity flagged not ok: the rest decide as without it
    gok[4] = 0
    want = GN.identify(probes, pok, off, gal, gok, ubm, r, th)
    _decided(want[3], pok, gok, off, th, True)
    got, mat = _identify(dev, ubm, probes, pok, off, gal, gok, r, th)
    _same(got, mat, want)
    without = GN.identify(probes, pok, off, np.delete(gal, 4, axis=0), np.delete(gok, 4), ubm, r, th)
    assert [i - (i > 4) for i in got['ident'].tolist()] == without[0].tolist()
    # nothing to do, and every refusal with a context: SPKD_EINVAL
    ctx = dev.ctx
    assert ctx.lib.spkd_clr_identify(ctx.h, None, 0, None, 0, None, None, 0, None, None, K, r, th, 1, None, None, None, None) == hipabi.SPKD_OK
    assert ctx.lib.spkd_bw_accumulate(ctx.h, None, 0, K, 0, None, None, None, None, None, 0) == hipabi.SPKD_OK
    for name, call in _refusals():
        assert call(ctx.lib, ctx.h) == hipabi.SPKD_EINVAL, name


@pytest.mark.gpu
def test_ordered_sums_to_the_bit(dev):
    K = 3
    rng = np.random.default_rng(12)
    src = rng.normal(0.0, 100.0, (12, K, L.BW_COMP)) * 10.0 ** rng.integers(-6, 6, (12, K, L.BW_COMP))
    dst = rng.normal(0.0, 1.0, (5, K, L.BW_COMP))
    set_off, member = [0, 1, 3, 12], [7, 11, 0, 5, 1, 2, 3, 4, 6, 8, 9, 10]
    slots, keep = [3, 0, 4], [1, 0, 1]                                   # slot 3 and 4 are kept and added to, 0 is overwritten
    d_src, d_dst = _upload(dev, src), _upload(dev, dst)
    dev.ctx.bw_accumulate(d_src, len(src), K, set_off, member, slots, keep, d_dst, len(dst))
    assert dev.ctx.last_ms('bw_accumulate') > 0.0
    got = np.empty_like(dst)
    dev.ctx.d2h(got, d_dst)
    want = GN.bw_accumulate(src, set_off, member, slots, keep, dst)
    assert np.array_equal(got, want)
    assert np.array_equal(want[4], ((((((((dst[4] + src[5]) + src[1]) + src[2]) + src[3]) + src[4]) + src[6]) + src[8]) + src[9]) + src[10])
    assert np.array_equal(got[[1, 2]], dst[[1, 2]]) and not np.array_equal(got[3], dst[3])
    # an empty set: the slot kept, or zeroed
    dev.ctx.bw_accumulate(d_src, len(src), K, [0, 0, 0], [], [1, 2], [1, 0], d_dst, len(dst))
    dev.ctx.d2h(got, d_dst)
    assert np.array_equal(got[1], dst[1]) and (got[2] == 0.0).all() and np.array_equal(got[[0, 3, 4]], want[[0, 3, 4]])


def _pipeline_batch(dev, name):
    """The arguments of link_batch for batch `name`: truth ranges as segments, as test_link_clr.people builds them."""
    p = dev.pipeline
    first, sess, speakers, person = _batches()[1][name]
    files = [p.BatchFile(f, len(s[0]), [(a / RATE, b / RATE) for a, b in s[1]]) for f, s in zip(first, sess)]
    seg_off = np.concatenate([[0], np.cumsum([len(s[2]) for s in sess])]).astype(np.int64)
    labels = [np.array([k // 2 + 1 for _, _, k in s[2]], dtype=np.int32) for s in sess]
    segments = [np.array([((a + 0.25) / RATE, (b + 0.25) / RATE) for a, b, _ in s[2]]) for s in sess]
    return seg_off, labels, files, segments


def _link(dev, name, link, timings=None, detail=None):
    seg_off, labels, files, segments = _pipeline_batch(dev, name)
    maps = dev.pipeline.link_batch(dev.ctx, 0, seg_off, labels, link, timings, dev.eng.d_frames, len(dev.frames), files,
                                   segments, RATE, detail)[0]
    return [int(m[l]) for m in maps for l in (1, 2)]


@pytest.mark.gpu
def test_a_label_means_the_same_person_across_batches(dev, tmp_path):
    p, gallery = dev.pipeline, pkg('gallery')
    flow = _restated_flow()
    g = gallery.Gallery(dev.ctx)
    link = dict(p.LINK_CLR, gallery=g)
    try:
        # batch A: the model is trained on it and handed to the gallery; its two people are enrolled
        tm, det = {}, {}
        assert _link(dev, 'A', link, tm, det) == flow['A']['labels'].tolist() == [1, 2, 1, 2]
        assert g.n == 2 and g.names == ['spk_1', 'spk_2'] and g.ok.tolist() == [1, 1] and det['enrolled'] == [0, 1]
        assert det['identity'].tolist() == [0, 1] and np.isnan(det['score']).all()
        assert _close(g.ubm, GN.L.train_ubm(dev.frames, _batches()[1]['A'][2], p.LINK_CLR)[0])
        assert _close(g.records(), flow['A']['records']) and _close(g.N, flow['A']['records'][:, :, 0].sum(axis=1))
        assert all(len(tm[k]) == 1 for k in ('link_ubm_train', 'link_ubm_stats', 'link_clr', 'link_cluster_sum', 'link_ident', 'link_update'))
        assert tm['link_cluster_sum'][0] > 0.0 and tm['link_update'][0] > 0.0
        # batch B without enrolment: the strangers are labelled 3 and 4, the gallery stays as it is to the bit
        before = g.to_arrays()
        tm, det = {}, {}
        assert _link(dev, 'B', dict(link, enrol=False), tm, det) == flow['B-']['labels'].tolist() == [1, 2, 3, 4]
        assert det['identity'].tolist() == [0, 1, -1, -1] and det['enrolled'] == [] and 'link_ubm_train' not in tm
        after = g.to_arrays()
        assert all(after[k].tobytes() == before[k].tobytes() for k in before) and g.n == 2
        for key in ('score', 'second'):
            assert _close(det[key], flow['B-'][key])
        assert tm['link_ident'][0] > 0.0 and tm['link_update'] == [0.0]
        # batch B: the known by person, two new identities
        det = {}
        assert _link(dev, 'B', link, None, det) == flow['B']['labels'].tolist() == [1, 2, 3, 4]
        assert g.n == 4 and det['enrolled'] == [2, 3] and det['identity'].tolist() == [0, 1, 2, 3]
        assert _close(g.records(), flow['B']['records'])
        # through a file into a fresh gallery; batch C: all four by person, nobody new
        path = str(tmp_path / 'gallery.npz')
        g.save(path)
        g2 = gallery.Gallery.load(dev.ctx, path)
        try:
            saved, loaded = g.to_arrays(), g2.to_arrays()
            assert all(saved[k].tobytes() == loaded[k].tobytes() for k in saved)
            det = {}
            assert _link(dev, 'C', dict(p.LINK_CLR, gallery=g2), None, det) == flow['C']['labels'].tolist() == [3, 4, 1, 2]
            assert g2.n == 4 and det['enrolled'] == [] and det['identity'].tolist() == [2, 3, 0, 1]
            for key in ('score', 'second'):
                print('batch C %s: device %s, restated %s' % (key, det[key].tolist(), flow['C'][key].tolist()))
                assert _close(det[key], flow['C'][key])
            assert _close(g2.records(), flow['C']['records']) and g2.names == ['spk_1', 'spk_2', 'spk_3', 'spk_4']
            # the model belongs to the identities now
            with pytest.raises(ValueError, match='holds identities'):
                g2.set_ubm(g2.ubm)
            # update by hand: a name for a new identity, two probes for one identity in probe order
            rec = g2.records()
            d_p = _upload(dev, rec[[1, 0, 1]])
            got = g2.update(d_p, [1, 1, 0], [-1, 3, 2], names=['anchor', None, None])
            assert got.tolist() == [4, 3, -1] and g2.n == 5 and g2.names[4] == 'anchor' and g2.ok.tolist() == [1] * 5
            now = g2.records()
            assert np.array_equal(now[4], rec[1]) and np.array_equal(now[3], rec[3] + rec[0]) and np.array_equal(now[:3], rec[:3])
        finally:
            g2.close()
    finally:
        g.close()


@pytest.mark.gpu
def test_diarize_batch_finds_every_cluster_again(dev):
    synth, p, gallery = pkg('synth'), dev.pipeline, pkg('gallery')
    series = synth.make_series([21, 22, 23], 40.0, 555)
    d = _Dev(np.concatenate([s[0] for s in series]))
    g = gallery.Gallery(d.ctx)
    try:
        foff = np.concatenate([[0], np.cumsum([len(s[0]) for s in series])])
        files = [p.BatchFile(foff[i], len(s[0]), [(a / RATE, b / RATE) for a, b in s[1]]) for i, s in enumerate(series)]
        args = (d.ctx, d.eng.d_frames, len(d.frames), files)
        linked = p.diarize_batch(*args, rate=RATE, link=p.LINK_CLR)
        det1, det2 = {}, {}
        first = p.diarize_batch(*args, rate=RATE, link=dict(p.LINK_CLR, gallery=g), detail=det1)
        n = g.n
        second = p.diarize_batch(*args, rate=RATE, link=dict(p.LINK_CLR, gallery=g), detail=det2)
        assert n == g.n == len(det1['link']['enrolled']) > 0 and det2['link']['enrolled'] == []
        assert det1['link']['identity'].tolist() == det2['link']['identity'].tolist() == list(range(n))
        assert (det2['link']['score'] > g.threshold).all()
        for f in range(3):
            assert first[f][:, :2].tobytes() == linked[f][:, :2].tobytes() == second[f][:, :2].tobytes()
            assert second[f][:, 2].tobytes() == first[f][:, 2].tobytes() and first[f][:, 2].min() >= 1
            # an empty gallery labels the clusters in their order: the labels of the chain alone
            assert first[f][:, 2].tobytes() == linked[f][:, 2].tobytes()
        assert [m.tolist() for m in det1['link']['maps']] == [m.tolist() for m in det2['link']['maps']]
        assert det1['link']['merges'] == det2['link']['merges']
    finally:
        g.close()
        d.close()
