"""Linking speakers across files by UBM-MAP cross-likelihood ratio: spkd_ubm_stats (every speaker's
statistics under one background model), spkd_clr_link (the agglomerative chain on the device),
pipeline.link_batch / diarize_batch with LINK_CLR.
PARITY: no reference counterpart; the numpy restatement is tests/link_clr_numpy.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import link_clr_numpy as L
import reseg_gmm_numpy as G
from helpers import ROOT
from conftest import pkg
from test_reseg_batch import _Dev, _close

RATE = 125.0


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _people_fixture():
    """Three 60 s files of the same four sources, sources {0, 1} and {2, 3} being two people: two
    bimodal speakers per file, the same two in every file, in shares that differ from file to file.
    Returns (sessions, frames of the batch, file offsets, speakers as range lists in link_speakers'
    order, the person of each speaker)."""
    synth = pkg('synth')
    models = [synth._speaker_model(777, k) for k in range(4)]
    sess = [synth.make_session(seed, 60.0, 4, models=models) for seed in (11, 12, 13)]
    foff = np.concatenate([[0], np.cumsum([len(s[0]) for s in sess])])
    speakers, person = [], []
    for f, s in enumerate(sess):
        for p in (0, 1):
            speakers.append([(int(foff[f] + a), int(foff[f] + b)) for a, b, k in s[2] if k // 2 == p])
            person.append(p)
    return sess, np.concatenate([s[0] for s in sess]), foff, speakers, person


# ------------------------------------------------------------------ not GPU
def test_entry_points_timers_and_constants_are_declared_and_exported():
    hipabi = pkg('hipabi')
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'spkd.h')).read(), flags=re.S)
    lib = hipabi.load_library()
    vmap = open(os.path.join(ROOT, 'speaker-diarization_amd', 'csrc', 'libspkd_hip.map')).read()
    assert re.search(r'global:\s*spkd_\*;', vmap)
    for name in ('spkd_ubm_stats', 'spkd_clr_link'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in hipabi.EXPORTS and hasattr(lib, name)
    assert lib.spkd_abi_version() == 2 and re.search(r'#define SPKD_ABI_VERSION 2\b', code)
    enum = re.search(r'enum \{\s*SPKD_T_CALL = 0,(.*?)SPKD_N_TIMERS', code, flags=re.S).group(1)
    names = ['call'] + [n.strip()[len('SPKD_T_'):].lower() for n in enum.split(',') if n.strip()]
    # (behind the mixture timers, as those were added: the front-end's two stay the last)
    assert names[names.index('gmm_seq_loglik') + 1:][:2] == ['ubm_stats', 'clr_link']
    assert [n for n, _ in sorted(hipabi.TIMERS.items(), key=lambda kv: kv[1])] == names
    csrc = os.path.join(ROOT, 'speaker-diarization_amd', 'csrc')
    stats, chain = open(os.path.join(csrc, 'spkd_ubm_stats.hpp')).read(), open(os.path.join(csrc, 'spkd_clr.hpp')).read()
    for macro, src, const, bound, restated, want in (
            ('SPKD_BW_COMP', stats, 'BW_COMP', hipabi.BW_COMP, L.BW_COMP, 40),
            ('SPKD_CLR_MAX_N', chain, 'CL_MAX_N', hipabi.CLR_MAX_N, L.MAX_N, 4096)):
        header = int(re.search(r'#define %s (\d+)' % macro, code).group(1))
        kernel = int(re.search(r'constexpr int %s = (\d+);' % const, src).group(1))
        assert header == kernel == bound == restated == want, macro
    assert hipabi.CLR_MAX_N >= 4096
    assert hasattr(hipabi.Context, 'ubm_stats') and hasattr(hipabi.Context, 'clr_link')
    for text in (stats, chain, L.__doc__):
        assert 'PARITY: no reference counterpart' in text
    # the E-step is spkd_gmm_train.hpp's, not restated
    assert 'gt_responsibilities(' in stats and 'gt_stage_tile(' in stats and 'exp(' not in stats
    pipeline = pkg('pipeline')
    assert pipeline.LINK_CLR == dict(model='clr', components=8, iterations=5, var_floor=0.01, relevance=16.0,
                                     threshold=-0.5, max_spk=0, ubm_max_frames=2_000_000)
    assert pipeline.LINK_CL == dict(variant=1, kind='BIC', lambdac=1.3, threshold=0.0, max_spk=0)


def _refusals():
    """(name, call(lib, ctx handle) -> status) of every argument refusal of the two entry points."""
    dev = C.c_void_p(4096)                        # never dereferenced: the refusal comes first
    odd = C.c_void_p(4104)
    ok = np.ones(4, dtype=np.int32)
    out_i, out_d = np.zeros(8, dtype=np.int32), np.zeros(8)
    keep = {}

    def stats(n_frames=100, n_spk=2, off=(0, 1, 3), b=(0, 10, 50), e=(10, 50, 100), K=2, frames=dev, ubm=dev, bw=dev,
              h_ok=ok):
        arr = [None if v is None else np.array(v, dtype=np.int64) for v in (off, b, e)]
        keep[len(keep)] = arr
        p = [None if a is None else _ptr(a) for a in arr]
        return lambda lib, h: lib.spkd_ubm_stats(h, frames, n_frames, ubm, K, n_spk, p[0], p[1], p[2], bw,
                                                 None if h_ok is None else _ptr(h_ok))

    def link(bw=dev, n=4, h_ok=ok, ubm=dev, K=2, r=16.0, th=-0.5, max_spk=0, a=out_i, b=out_i, d=out_d, nm=out_i,
             smax=out_d, smin=out_d):
        q = lambda v: None if v is None else _ptr(v)
        return lambda lib, h: lib.spkd_clr_link(h, bw, n, q(h_ok), ubm, K, r, th, max_spk, q(a), q(b), q(d), q(nm),
                                                q(smax), q(smin))

    return [
        ('stats: null frames', stats(frames=None)), ('stats: null model', stats(ubm=None)),
        ('stats: null offsets', stats(off=None)), ('stats: null begin', stats(b=None)), ('stats: null end', stats(e=None)),
        ('stats: null records', stats(bw=None)), ('stats: null ok', stats(h_ok=None)),
        ('stats: negative speaker count', stats(n_spk=-1)),
        ('stats: no component', stats(K=0)), ('stats: a 9th component', stats(K=9)),
        ('stats: offsets not from 0', stats(off=(1, 2, 3))), ('stats: offsets go back', stats(off=(0, 2, 1))),
        ('stats: an empty set', stats(off=(0, 0, 3))), ('stats: an empty last set', stats(off=(0, 3, 3))),
        ('stats: begin below 0', stats(b=(-1, 10, 50))), ('stats: end past the frames', stats(e=(10, 50, 101))),
        ('stats: end before begin', stats(b=(0, 20, 50), e=(10, 19, 100))),
        ('stats: negative frame count', stats(n_frames=-1)),
        ('stats: misaligned model', stats(ubm=odd)), ('stats: misaligned records', stats(bw=odd)),
        ('link: null records', link(bw=None)), ('link: null ok', link(h_ok=None)), ('link: null model', link(ubm=None)),
        ('link: null a', link(a=None)), ('link: null b', link(b=None)), ('link: null d', link(d=None)),
        ('link: null merge count', link(nm=None)), ('link: null maximum', link(smax=None)),
        ('link: null minimum', link(smin=None)), ('link: negative count', link(n=-1)),
        ('link: more than the limit', link(n=4097)),
        ('link: no component', link(K=0)), ('link: a 9th component', link(K=9)),
        ('link: relevance 0', link(r=0.0)), ('link: negative relevance', link(r=-1.0)),
        ('link: relevance NaN', link(r=float('nan'))), ('link: relevance inf', link(r=float('inf'))),
        ('link: threshold NaN', link(th=float('nan'))), ('link: negative max_spk', link(max_spk=-1)),
        ('link: misaligned records', link(bw=odd)), ('link: misaligned model', link(ubm=odd)),
    ]


def test_every_refusal_is_einval_without_a_context():
    hipabi = pkg('hipabi')
    lib = hipabi.load_library()
    for name, call in _refusals():
        assert call(lib, None) == hipabi.SPKD_EINVAL, name


def test_ubm_ranges_cut_in_ordinal_order():
    """Hand-made ranges: speaker 0 of 10 + 0 + 20 frames, speaker 1 of 3, speaker 2 of 30 + 10; 73 in all."""
    pipeline = pkg('pipeline')
    spk = [[(0, 10), (20, 20), (30, 50)], [(100, 103)], [(60, 90), (90, 100)]]
    off = np.concatenate([[0], np.cumsum([len(r) for r in spk])])
    b, e = [x for r in spk for x, _ in r], [y for r in spk for _, y in r]
    cut = lambda cap: pipeline.ubm_ranges(off, b, e, cap).tolist()
    assert cut(1000) == e and cut(73) == e                          # a cap above the total, and at it
    # cap 40: shares floor(40 * 30 / 73) = 16, floor(40 * 3 / 73) = 1, floor(40 * 40 / 73) = 21: inside a range
    assert cut(40) == [10, 20, 36, 101, 81, 90]
    # cap 20: 8, 0 (speaker 1's share rounds to 0), 10: the later ranges are left empty
    assert cut(20) == [8, 20, 30, 100, 70, 90]
    for cap in (1000, 73, 72, 40, 20, 5):
        assert cut(cap) == [y for r in L.ubm_ranges(spk, cap) for _, y in r], cap
        assert sum(y - x for x, y in zip(b, cut(cap))) <= cap or cap >= 73


def test_refusals_of_the_pipeline_need_no_device():
    pipeline = pkg('pipeline')
    files = [pipeline.BatchFile(0, 1000, [(0.0, 8.0)])]
    segments = [np.array([(0.0, 4.0), (4.0, 8.0)])]
    labels = [np.array([1, 2])]
    nan, inf = float('nan'), float('inf')
    bad = [(dict(model='ubm'), 'link model'), (dict(components=0), 'link components'), (dict(components=9), 'link components'),
           (dict(components=2.5), 'link components'), (dict(iterations=-1), 'link iterations'),
           (dict(var_floor=-0.1), 'link var_floor'), (dict(var_floor=nan), 'link var_floor'),
           (dict(var_floor=inf), 'link var_floor'), (dict(relevance=0.0), 'link relevance'),
           (dict(relevance=-1.0), 'link relevance'), (dict(relevance=nan), 'link relevance'),
           (dict(relevance=inf), 'link relevance'), (dict(threshold=nan), 'link threshold'),
           (dict(threshold=inf), 'link threshold'), (dict(max_spk=-1), 'link max_spk'),
           (dict(ubm_max_frames=319), 'link ubm_max_frames'), (dict(components=2, ubm_max_frames=79), 'link ubm_max_frames')]
    for change, match in bad:
        link = dict(pipeline.LINK_CLR, **change)
        with pytest.raises(ValueError, match=match):
            pipeline.link_batch(None, 0, [0, 2], labels, link, d_frames=0, total_frames=1000, files=files, segments=segments)
        with pytest.raises(ValueError, match=match):
            pipeline.diarize_batch(None, 0, 0, [], link=link)
    assert pipeline._link_model(dict(pipeline.LINK_CLR, components=2, ubm_max_frames=80))[1] == 2
    assert pipeline._link_model(dict(model='clr')) == ('clr', 8, 5, 0.01, 16.0, -0.5, 0, 2_000_000)
    for missing in ('d_frames', 'total_frames', 'files', 'segments'):
        kw = dict(d_frames=0, total_frames=1000, files=files, segments=segments)
        kw[missing] = None
        with pytest.raises(ValueError, match='link model clr trains on the frames'):
            pipeline.link_batch(None, 0, [0, 2], labels, pipeline.LINK_CLR, **kw)
    with pytest.raises(ValueError, match='one per label'):
        pipeline.link_batch(None, 0, [0, 2], labels, pipeline.LINK_CLR, d_frames=0, total_frames=1000, files=files,
                            segments=[segments[0][:1]])
    with pytest.raises(ValueError, match='link takes the host hand-off'):
        pipeline.diarize_batch(None, 0, 0, [], link=pipeline.LINK_CLR, fused=True)
    # nothing to link: no device work
    det = {}
    assert pipeline.diarize_batch(None, 0, 0, [], link=pipeline.LINK_CLR, detail=det) == [] and det['link']['merges'] == []
    maps, merges, _, _ = pipeline.link_batch(None, 0, [0, 0], [np.zeros(0, dtype=np.int32)], pipeline.LINK_CLR, d_frames=0,
                                             total_frames=1000, files=files, segments=[np.zeros((0, 2))])
    assert [m.tolist() for m in maps] == [[]] and merges == []


def test_a_dictionary_wrong_in_two_ways_is_refused_for_the_same_reason_as_ever():
    """The order of the refusals, as recorded before linking got a module and one parser of its own: the
    model keys in _link_model's order, then the gallery keys, then link_batch's arrays / diarize_batch's
    hand-off; in diarize_batch the reseg, cl and cd refusals come before any of them.  Whole texts."""
    pipeline, gallery = pkg('pipeline'), pkg('gallery')
    files = [pipeline.BatchFile(0, 1000, [(0.0, 8.0)])]
    segments = [np.array([(0.0, 4.0), (4.0, 8.0)])]
    labels = [np.array([1, 2])]
    nan, held = float('nan'), gallery.Gallery(None)
    both = [
        (pipeline.LINK_CLR, dict(components=0, threshold=nan), 'link components: 1 .. 8'),
        (pipeline.LINK_CLR, dict(iterations=-1, ubm_max_frames=1), 'link iterations: an integer >= 0'),
        (pipeline.LINK_CLR, dict(model='ubm', components=0), 'link model: clr (or no model: the clustering keys of LINK_CL)'),
        (pipeline.LINK_CLR, dict(var_floor=-1.0, max_spk=-1),
         'link var_floor: a finite number >= 0 (a share of the variance of all the frames)'),
        (pipeline.LINK_CLR, dict(gallery=object(), relevance=0.0), 'link relevance: a finite number > 0'),
        (pipeline.LINK_CLR, dict(gallery=object(), max_spk=2.5), 'link max_spk: an integer >= 0'),
        (pipeline.LINK_CLR, dict(gallery=held, components=4, relevance=2.0), 'link components: the gallery has 8'),
        (pipeline.LINK_CL, dict(gallery=object(), components=0), 'link gallery: a gallery holds the records of link model clr'),
    ]
    for base, change, text in both:
        link = dict(base, **change)
        with pytest.raises(ValueError) as ei:
            pipeline.link_batch(None, 0, [0, 2], labels, link, d_frames=0, total_frames=1000, files=files, segments=segments)
        assert str(ei.value) == text, change
        with pytest.raises(ValueError) as ei:
            pipeline.diarize_batch(None, 0, 0, [], link=link)
        assert str(ei.value) == text, change
    # a bad key together with a missing array (link_batch) or the wrong hand-off (diarize_batch): the key first
    for change, text in ((dict(gallery=object()), 'link gallery: a gallery.Gallery'),
                         (dict(threshold=nan), 'link threshold: a finite number (a ratio above it merges)')):
        link = dict(pipeline.LINK_CLR, **change)
        with pytest.raises(ValueError) as ei:
            pipeline.link_batch(None, 0, [0, 2], labels, link, d_frames=None, total_frames=1000, files=files, segments=None)
        assert str(ei.value) == text, change
        with pytest.raises(ValueError) as ei:
            pipeline.diarize_batch(None, 0, 0, [], link=link, fused=True)
        assert str(ei.value) == text, change
    # diarize_batch: reseg, the clustering method and the detector are refused before a bad link dictionary
    bad = dict(pipeline.LINK_CLR, components=0)
    for kw, text in ((dict(reseg=dict(penalty=-1.0)), 'reseg penalty: a finite number >= 0 (natural-log units)'),
                     (dict(reseg=pipeline.RESEG, handoff='device'), 'reseg takes the host hand-off'),
                     (dict(cl=dict(pipeline.DIA2_CL, method='x')), 'cl method: hi or in'),
                     (dict(cd=dict(pipeline.DIA2_CD, method='x')), 'cd method: gw, sw or m'),
                     (dict(cd=pipeline.SW_CD, fused=True), 'cd method sw takes the host hand-off and is not fused')):
        with pytest.raises(ValueError) as ei:
            pipeline.diarize_batch(None, 0, 0, [], link=bad, **kw)
        assert str(ei.value) == text, kw
    # ... and a good one's hand-off before the device-mode checks and the name of the hand-off
    for base in (pipeline.LINK_CLR, pipeline.LINK_CL):
        with pytest.raises(ValueError) as ei:
            pipeline.diarize_batch(None, 0, 0, [], link=base, handoff='device', fused=False)
        assert str(ei.value) == 'link takes the host hand-off'
        with pytest.raises(ValueError) as ei:
            pipeline.diarize_batch(None, 0, 0, [], link=base, handoff='x')
        assert str(ei.value) == 'handoff: device or host'


def test_restated_clr_links_the_people_where_bic_does_not():
    """What the mode is for.  Seeds 11, 12, 13 over the sources of seed 777 (the first tried): per file
    the share of a speaker's frames from its first source runs from 0 to 1.  BIC over one Gaussian a
    speaker leaves more than two global speakers; the restated LINK_CLR finds exactly the two people,
    at its own threshold and 0.1 to either side of it."""
    from oracle.numpy_engine import NumpyEngine
    from link_numpy import link_hi
    pipeline = pkg('pipeline')
    sess, feats, foff, speakers, person = _people_fixture()
    shares = [np.mean([k % 2 == 0 for a, b, k in s[2] for _ in range(a, b) if k // 2 == p]) for s in sess for p in (0, 1)]
    print('share of the first source per speaker: %s' % ', '.join('%.2f' % v for v in shares))
    assert min(shares) < 0.05 and max(shares) > 0.95
    ne = NumpyEngine()
    ne.set_features(feats)
    cl = pipeline.LINK_CL
    _, partition = link_hi(ne, speakers, cl['variant'], cl['kind'], cl['lambdac'], cl['threshold'], cl['max_spk'])
    print('BIC: %s' % partition)
    assert len(partition) > 2
    for th in (-0.5, -0.4, -0.6):
        lab, merges, smax, smin = L.link(feats, speakers, dict(pipeline.LINK_CLR, threshold=th))[:4]
        print('CLR, threshold %.1f: labels %s, merges %s, initial ratios in [%.3f, %.3f]' % (th, lab.tolist(), merges, smin, smax))
        assert lab.tolist() == [p + 1 for p in person], th


# ------------------------------------------------------------------ GPU
N_SESSION = 7500


@pytest.fixture(scope='module')
def one():
    """One 60 s session of two speakers, then 400 frames with a NaN among them; a background model of 1
    and of 8 components trained on the session by the device, as the device left it."""
    feats = pkg('synth').make_session(909, 60.0, 2)[0]
    assert len(feats) == N_SESSION
    tail = feats[1000:1400].copy()
    tail[123, 5] = np.nan
    d = _Dev(np.concatenate([feats, tail]))
    d.ubm, d.d_ubm = {}, {}
    for K in (1, 8):
        d.d_ubm[K] = d.alloc(K * G.COMP * 8)
        ok, _ = d.ctx.gmm_train(d.eng.d_frames, len(d.frames), [0, 1], [0], [N_SESSION], K, 3, 0.01, d.d_ubm[K])
        assert ok.tolist() == [1]
        d.ubm[K] = np.empty((K, G.COMP))
        d.ctx.d2h(d.ubm[K], d.d_ubm[K])
    yield d
    d.close()


EDGES = [(5000, 1), (100, 63), (4000, 64), (200, 65), (1000, 1023), (6000, 1024), (2100, 1025)]


def _speakers():
    return [[(b, b + n)] for b, n in EDGES] + [
        [(300, 340), (50, 50), (900, 1990), (10, 17)],                # several ranges, an empty one, 1 137 frames
        [(700, 700)],                                                  # no frame
        [(N_SESSION, N_SESSION + 400)],                                # a NaN frame; the range ends at n_frames
        [(3000, 7000)]]                                                # four chunks, the last one short


def _stats(dev, spk, d_ubm, K, d_bw):
    off = np.concatenate([[0], np.cumsum([len(r) for r in spk])])
    flat = [r for rs in spk for r in rs]
    ok = dev.ctx.ubm_stats(dev.eng.d_frames, len(dev.frames), d_ubm, K, off, [b for b, _ in flat], [e for _, e in flat], d_bw)
    out = np.empty((len(spk), K, L.BW_COMP))
    dev.ctx.d2h(out, d_bw)
    return ok, out


@pytest.mark.gpu
@pytest.mark.parametrize('K', [1, 8])
def test_records_match_the_restatement(one, K):
    spk = _speakers()
    assert spk[9][0][1] == len(one.frames)
    d_bw = one.alloc(len(spk) * K * L.BW_COMP * 8)
    ok, got = _stats(one, spk, one.d_ubm[K], K, d_bw)
    assert ok.tolist() == [1] * 8 + [0, 0, 1]
    assert one.ctx.last_ms('ubm_stats') > 0.0
    for s, rs in enumerate(spk):
        want, good = L.ubm_stats(L.frames_of(one.frames, rs), one.ubm[K])
        assert good == bool(ok[s]), s
        if good:
            err = float(np.abs(got[s] - want).max())
            print('K %d speaker %d (%d frames): max abs error %.3g' % (K, s, sum(e - b for b, e in rs), err))
            assert _close(got[s], want), s
            assert _close(got[s][:, 0].sum(), sum(e - b for b, e in rs)), s      # the responsibilities of a frame add to 1
    assert (got[8] == 0.0).all()                                       # no frame: a record of zeros, not ok
    if K == 8:
        # a component whose ln w is -inf takes no part: its n and f are exactly 0
        ubm = one.ubm[K].copy()
        ubm[2, 0] = -np.inf
        d_ubm = one.alloc(ubm.nbytes)
        one.ctx.h2d(d_ubm, ubm)
        keep = [0, 3, 5, 7, 10]
        ok2, got2 = _stats(one, [spk[s] for s in keep], d_ubm, K, d_bw)
        assert ok2.tolist() == [1] * 5
        for i, s in enumerate(keep):
            want, good = L.ubm_stats(L.frames_of(one.frames, spk[s]), ubm)
            assert good and (got2[i][2] == 0.0).all() and (want[2] == 0.0).all(), s
            assert _close(got2[i], want), s


@pytest.mark.gpu
def test_records_are_reproducible_to_the_bit(one):
    K = 8
    spk = _speakers()
    n = len(spk)
    d_a, d_b = one.alloc(n * K * L.BW_COMP * 8), one.alloc(n * K * L.BW_COMP * 8)
    ok_a, a = _stats(one, spk, one.d_ubm[K], K, d_a)
    ok_b, b = _stats(one, spk, one.d_ubm[K], K, d_b)
    good = np.nonzero(ok_a)[0]
    assert ok_a.tolist() == ok_b.tolist() and a[good].tobytes() == b[good].tobytes()
    for s in (4, 7, 10):                                               # a speaker alone and among the others
        ok_s, r = _stats(one, [spk[s]], one.d_ubm[K], K, d_b)
        assert ok_s.tolist() == [1] and r.tobytes() == a[s:s + 1].tobytes()
    # nothing to do, and every refusal with a context: SPKD_EINVAL, nothing written
    hipabi, ctx = one.hipabi, one.ctx
    assert ctx.lib.spkd_ubm_stats(ctx.h, None, 0, None, K, 0, None, None, None, None, None) == hipabi.SPKD_OK
    assert ctx.lib.spkd_clr_link(ctx.h, None, 0, None, None, K, 16.0, -0.5, 0, None, None, None, None, None, None) == hipabi.SPKD_OK
    for name, call in _refusals():
        assert call(ctx.lib, ctx.h) == hipabi.SPKD_EINVAL, name
    out = np.empty_like(a)
    ctx.d2h(out, d_a)
    assert out.tobytes() == a.tobytes()


def _hand_records(seed, n, n_people, K):
    """A background model and n records by hand: person p's frames sit 0.3 a dimension off the model's
    means, so that the ratio of one person's records is near +3.5 and of two people's near -3.5."""
    rng = np.random.default_rng(seed)
    ubm = np.zeros((K, G.COMP))
    ubm[:, 0] = np.log(1.0 / K)
    ubm[:, G.MEAN:G.IVAR] = rng.normal(0.0, 1.0, (K, G.DIM))
    ubm[:, G.IVAR:G.NORM] = 1.0 / rng.uniform(0.5, 2.0, (K, G.DIM))
    ubm[:, G.NORM] = -0.5 * (G.DIM * G.LN_2PI - np.log(ubm[:, G.IVAR:G.NORM]).sum(axis=1))
    sd = np.sqrt(1.0 / ubm[:, G.IVAR:G.NORM])
    shift = rng.normal(0.0, 0.3, (n_people, K, G.DIM)) * sd
    who = rng.integers(0, n_people, n)
    rec = np.zeros((n, K, L.BW_COMP))
    rec[:, :, 0] = rng.uniform(50.0, 500.0, (n, K))
    mean = ubm[None, :, G.MEAN:G.IVAR] + shift[who] + rng.normal(0.0, 0.03, (n, K, G.DIM)) * sd
    rec[:, :, 1:] = rec[:, :, :1] * mean
    return ubm, rec, who


def _link_on_device(dev, ubm, rec, ok, r, th, max_spk=0):
    K = len(ubm)
    d_ubm, d_bw = dev.alloc(ubm.nbytes), dev.alloc(max(rec.nbytes, 16))
    dev.ctx.h2d(d_ubm, ubm)
    dev.ctx.h2d(d_bw, rec)
    got = dev.ctx.clr_link(d_bw, ok, d_ubm, K, r, th, max_spk)
    after = np.empty_like(rec)
    dev.ctx.d2h(after, d_bw)
    assert after.tobytes() == rec.tobytes()                            # d_bw is not modified
    return got


def _same_log(got, want):
    merges, smax, smin, fin = want
    assert fin and got['status'] == 0
    assert list(zip(got['a'].tolist(), got['b'].tolist())) == [(a, b) for a, b, _ in merges]
    assert _close(got['d'], [d for _, _, d in merges])
    if np.isnan(smax):
        assert np.isnan(got['stat_max']) and np.isnan(got['stat_min'])
    else:
        assert _close(got['stat_max'], smax) and _close(got['stat_min'], smin)


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 2, 7, 40])
def test_chain_matches_the_restatement(one, n):
    K, r = 8, 16.0
    ubm, rec, who = _hand_records(100 + n, n, 1 if n == 2 else 3 if n == 7 else 5, K)
    ok = np.ones(n, dtype=np.int32)
    if n == 7:
        rec[5] = rec[4] = rec[1]                                       # an exact tie among (1, 4), (1, 5), (4, 5)
        ok[3] = 0                                                      # and a speaker that is never chosen
    got = _link_on_device(one, ubm, rec, ok, r, -0.5)
    want = L.clr_link(rec, ok, ubm, r, -0.5)
    print('n %d: merges %s' % (n, [(a, b, round(d, 6)) for a, b, d in want[0]]))
    _same_log(got, want)
    assert one.ctx.last_ms('clr_link') > 0.0 or n == 1
    labels = one.hipabi.labels_from_merges(n, got['a'], got['b'])
    assert labels.tolist() == L.labels_from_merges(n, want[0]).tolist()
    if n == 1:
        assert got['n_merges'] == 0
    if n == 2:
        assert got['n_merges'] == 1 and got['a'].tolist() == [0] and got['b'].tolist() == [1]
    if n == 7:
        tie = [L.clr(rec[a], rec[b], ubm, r) for a, b in ((1, 4), (1, 5), (4, 5))]
        assert tie[0] == tie[1] == tie[2]                              # (the first pair in row-major order wins)
        assert labels[1] == labels[4] == labels[5] and (labels == labels[3]).sum() == 1
    if n == 40:
        # the threshold stop: the five people, each one cluster
        assert got['n_merges'] == 35 and len(set(zip(who.tolist(), labels.tolist()))) == 5
        # the max_spk stop: merging goes on below the threshold until three are left
        got3 = _link_on_device(one, ubm, rec, ok, r, -0.5, 3)
        _same_log(got3, L.clr_link(rec, ok, ubm, r, -0.5, 3))
        assert got3['n_merges'] == 37 and (got3['d'][35:] <= -0.5).all()
        # a threshold above every ratio: no merge; one below every ratio: one cluster
        assert _link_on_device(one, ubm, rec, ok, r, 1e9)['n_merges'] == 0
        assert _link_on_device(one, ubm, rec, ok, r, -1e9)['n_merges'] == 39
        # speakers that are not ok count as clusters of the list, positions included
        ok2 = ok.copy()
        ok2[[0, 17, 39]] = 0
        got2 = _link_on_device(one, ubm, rec, ok2, r, -0.5, 6)
        _same_log(got2, L.clr_link(rec, ok2, ubm, r, -0.5, 6))
        lab2 = one.hipabi.labels_from_merges(n, got2['a'], got2['b'])
        assert all((lab2 == lab2[s]).sum() == 1 for s in (0, 17, 39))


@pytest.mark.gpu
def test_chain_limits_and_records_that_are_not_finite(one):
    hipabi, K = one.hipabi, 8
    ubm, rec, _ = _hand_records(7, 9, 3, K)
    ok = np.ones(9, dtype=np.int32)
    # a NaN in a record whose speaker is ok: SPKD_ENONFINITE, no merge logged
    bad = rec.copy()
    bad[6, 3, 11] = np.nan
    got = _link_on_device(one, ubm, bad, ok, 16.0, -0.5)
    assert got['status'] == hipabi.SPKD_ENONFINITE and got['n_merges'] == 0
    assert not L.clr_link(bad, ok, ubm, 16.0, -0.5)[3]
    # the same speaker flagged not ok: it is left alone, the others link as without it
    ok[6] = 0
    _same_log(_link_on_device(one, ubm, bad, ok, 16.0, -0.5), L.clr_link(bad, ok, ubm, 16.0, -0.5))
    # more speakers than the limit
    with pytest.raises(hipabi.SpkdError) as ei:
        one.ctx.clr_link(one.d_ubm[K], np.ones(hipabi.CLR_MAX_N + 1, dtype=np.int32), one.d_ubm[K], K, 16.0, -0.5)
    assert ei.value.status == hipabi.SPKD_EINVAL


@pytest.fixture(scope='module')
def people():
    sess, feats, foff, speakers, person = _people_fixture()
    d = _Dev(feats)
    d.sess, d.foff, d.speakers, d.person = sess, foff, speakers, person
    d.files = [d.pipeline.BatchFile(foff[i], len(s[0]), [(a / RATE, b / RATE) for a, b in s[1]]) for i, s in enumerate(sess)]
    d.seg_off = np.concatenate([[0], np.cumsum([len(s[2]) for s in sess])]).astype(np.int64)
    d.labels = [np.array([k // 2 + 1 for _, _, k in s[2]], dtype=np.int32) for s in sess]
    # (a quarter of a frame past each bound: int(t * rate) is then the truth's frame whatever the division rounds to)
    d.segments = [np.array([((a + 0.25) / RATE, (b + 0.25) / RATE) for a, b, _ in s[2]]) for s in sess]
    yield d
    d.close()


@pytest.mark.gpu
def test_link_batch_finds_the_two_people(people):
    p, ctx = people.pipeline, people.ctx
    n = len(people.frames)
    # the restatement on the ranges the pipeline cuts from the segments' times
    _, _, seg_b, seg_e = p._segment_ranges(people.files, people.segments, RATE)
    member, set_off, spk_file, spk_label = p.link_speakers(people.seg_off, people.labels)
    speakers = [[(int(seg_b[m]), int(seg_e[m])) for m in member[a:b]] for a, b in zip(set_off[:-1], set_off[1:])]
    assert speakers == people.speakers
    want, want_merges = L.link(people.frames, speakers, p.LINK_CLR)[:2]
    timings = {}
    maps, merges, smax, smin = p.link_batch(ctx, 0, people.seg_off, people.labels, p.LINK_CLR, timings, people.eng.d_frames,
                                            n, people.files, people.segments, RATE)
    print('merges %s, initial ratios in [%.3f, %.3f]' % (merges, smin, smax))
    assert [m.tolist() for m in maps] == [[0, 1, 2]] * 3
    assert [int(maps[f][l]) for f, l in zip(spk_file, spk_label)] == want.tolist() == [q + 1 for q in people.person]
    assert [(a, b) for a, b, _ in merges] == [(a, b) for a, b, _ in want_merges]
    assert smin < -0.5 < smax
    assert all(len(timings[k]) == 1 and timings[k][0] > 0.0 for k in ('link_ubm_train', 'link_ubm_stats', 'link_clr'))
    assert timings['link_speakers'] == 6 and timings['link_merges'] == 4
    # a cap below the frames the speakers hold: the model trains on a cut, the statistics take every frame
    capped = dict(p.LINK_CLR, ubm_max_frames=6000)
    maps2 = p.link_batch(ctx, 0, people.seg_off, people.labels, capped, None, people.eng.d_frames, n, people.files,
                         people.segments, RATE)[0]
    want2 = L.link(people.frames, speakers, capped)[0]
    assert [m.tolist() for m in maps2] == [[0] + want2[2 * f:2 * f + 2].tolist() for f in range(3)]
    # no background model (fewer than 40 frames a component): every speaker keeps a label of its own
    few = [p.BatchFile(0, 200, [(0.0, 1.6)])]
    maps3, merges3, s3, _ = p.link_batch(ctx, 0, [0, 2], [np.array([1, 2])], p.LINK_CLR, None, people.eng.d_frames, n, few,
                                         [np.array([(0.0, 0.8), (0.8, 1.6)])], RATE)
    assert [m.tolist() for m in maps3] == [[0, 1, 2]] and merges3 == [] and np.isnan(s3)


@pytest.mark.gpu
def test_diarize_batch_with_clr_link_end_to_end():
    synth, p = pkg('synth'), pkg('pipeline')
    series = synth.make_series([21, 22, 23], 40.0, 555)
    d = _Dev(np.concatenate([s[0] for s in series]))
    try:
        foff = np.concatenate([[0], np.cumsum([len(s[0]) for s in series])])
        files = [p.BatchFile(foff[i], len(s[0]), [(a / RATE, b / RATE) for a, b in s[1]]) for i, s in enumerate(series)]
        args = (d.ctx, d.eng.d_frames, len(d.frames), files)
        plain = p.diarize_batch(*args, rate=RATE)
        det = {}
        linked = p.diarize_batch(*args, rate=RATE, link=p.LINK_CLR, detail=det)
        maps = det['link']['maps']
        assert len(maps) == 3 and all(len(r) for r in linked)
        for f in range(3):
            assert linked[f][:, :2].tobytes() == plain[f][:, :2].tobytes()
            assert np.array_equal(linked[f][:, 2], maps[f][plain[f][:, 2].astype(np.int64)])
            assert linked[f][:, 2].min() >= 1
        n_glob = len(set(int(g) for m in maps for g in m[1:] if g))
        assert n_glob == sum(int((m[1:] > 0).sum()) for m in maps) - len(det['link']['merges'])
        # with resegmentation as well: the resegmented rows through the same maps
        det2 = {}
        both = p.diarize_batch(*args, rate=RATE, link=p.LINK_CLR, reseg=p.RESEG, detail=det2)
        reseg = p.diarize_batch(*args, rate=RATE, reseg=p.RESEG)
        assert [m.tolist() for m in det2['link']['maps']] == [m.tolist() for m in maps]
        for f in range(3):
            assert np.array_equal(both[f][:, 2], maps[f][reseg[f][:, 2].astype(np.int64)])
        # LINK_CL and no link: what they return without the new arrays
        det3 = {}
        cl = p.diarize_batch(*args, rate=RATE, link=p.LINK_CL, detail=det3)
        segs = p.change_detect_batch(d.ctx, d.eng.d_frames, len(d.frames), files, RATE)
        box = []
        res = p.cluster_batch(d.ctx, d.eng.d_frames, len(d.frames), files, segs, RATE, stats_out=box)
        direct = p.link_batch(d.ctx, box[0][0], box[0][1], [lab for lab, _ in res])
        assert [m.tolist() for m in det3['link']['maps']] == [m.tolist() for m in direct[0]]
        assert det3['link']['merges'] == direct[1]
        for f in range(3):
            assert np.array_equal(cl[f][:, 2], direct[0][f][plain[f][:, 2].astype(np.int64)])
        assert [r.tobytes() for r in p.diarize_batch(*args, rate=RATE, link=None)] == [r.tobytes() for r in plain]
    finally:
        d.close()
