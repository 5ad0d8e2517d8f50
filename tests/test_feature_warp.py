"""Feature warping on the device ahead of linking by cross-likelihood ratio: spkd_feature_warp against its
frame-by-frame restatement (tests/warp_numpy.py) to the bit, pipeline.link_batch / diarize_batch with
LINK_CLR_WARP, the gallery's window.
PARITY: no reference counterpart; the numpy restatement is tests/warp_numpy.py."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import gallery_numpy as GN
import link_clr_numpy as L
import warp_numpy as W
from helpers import ROOT
from conftest import pkg
from reseg_helpers import Dev
from test_link_clr import _people_fixture, _same_log

RATE = 125.0
TILE = W.TILE
MAX_W = W.MAX_WINDOW


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _channel_fixture():
    """test_link_clr._people_fixture() with each file through a per-dimension channel y = a x + b of its own:
    the frozen draw of default_rng(5) (tests/golden/make_golden_feature_warp.py).  Returns (frames through
    the channels, the fixture's frames, file offsets, speakers, the person and the file of each speaker)."""
    sess, feats, foff, speakers, person = _people_fixture()
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'feature_warp_channel.npz')) as z:
        gain, offset = z['gain'], z['offset']
    assert gain.shape == offset.shape == (3, W.DIM) and (np.abs(np.log(gain)) <= 0.4).all()
    out = feats.copy()
    for f in range(3):
        out[foff[f]:foff[f + 1]] = (gain[f] * feats[foff[f]:foff[f + 1]] + offset[f]).astype(np.float32)
    return out, feats, foff, speakers, person, [s // 2 for s in range(len(speakers))]


@functools.lru_cache(maxsize=None)
def _warped_channel_frames():
    """The channel fixture's frames warped by the restatement over LINK_CLR_WARP's window, file by file."""
    feats, _, _, speakers, _, files = _channel_fixture()
    sets = [W.speech_runs([r for s, rs in enumerate(speakers) if files[s] == f for r in rs]) for f in range(3)]
    return W.warp(feats, sets, int(round(pkg('pipeline').LINK_CLR_WARP['warp_s'] * RATE)))


# ------------------------------------------------------------------ not GPU
def test_entry_point_timer_and_constants_are_declared_and_exported():
    hipabi, pipeline, linking, clr_model = pkg('hipabi'), pkg('pipeline'), pkg('linking'), pkg('clr_model')
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'spkd.h')).read(), flags=re.S)
    lib = hipabi.load_library()
    vmap = open(os.path.join(ROOT, 'speaker-diarization_amd', 'csrc', 'libspkd_hip.map')).read()
    assert re.search(r'global:\s*spkd_\*;', vmap)
    assert re.search(r'\bspkd_feature_warp\s*\(', code)
    assert 'spkd_feature_warp' in hipabi.EXPORTS and hasattr(lib, 'spkd_feature_warp')
    assert lib.spkd_abi_version() == 2 and re.search(r'#define SPKD_ABI_VERSION 2\b', code)
    enum = re.search(r'enum \{\s*SPKD_T_CALL = 0,(.*?)SPKD_N_TIMERS', code, flags=re.S).group(1)
    names = ['call'] + [n.strip()[len('SPKD_T_'):].lower() for n in enum.split(',') if n.strip()]
    assert names[names.index('energy_seeds') + 1] == 'feature_warp' and len(names) == len(set(names))
    assert [n for n, _ in sorted(hipabi.TIMERS.items(), key=lambda kv: kv[1])] == names
    kern = open(os.path.join(ROOT, 'speaker-diarization_amd', 'csrc', 'spkd_warp.hpp')).read()
    for macro, const, bound, restated, want in (('SPKD_WARP_MAX_WINDOW', 'WP_MAX_WINDOW', hipabi.WARP_MAX_WINDOW, W.MAX_WINDOW, 512),
                                                ('SPKD_WARP_TILE', 'WP_TILE', hipabi.WARP_TILE, W.TILE, None)):
        header = int(re.search(r'#define %s (\d+)' % macro, code).group(1))
        kernel = int(re.search(r'constexpr int %s = (\d+);' % const, kern).group(1))
        assert header == kernel == bound == restated and want in (None, header), macro
    assert hasattr(hipabi.Context, 'feature_warp') and callable(hipabi.warp_table) and callable(pipeline.warp_batch)
    for text in (kern, W.__doc__):
        assert 'PARITY: no reference counterpart' in text
    # the modes there were are what they were; the new one is LINK_CLR with a window and a threshold of its own
    assert pipeline.LINK_CLR == dict(model='clr', components=8, iterations=5, var_floor=0.01, relevance=16.0,
                                     threshold=-0.5, max_spk=0, ubm_max_frames=2_000_000)
    assert pipeline.LINK_CL == dict(variant=1, kind='BIC', lambdac=1.3, threshold=0.0, max_spk=0)
    assert pipeline.LINK_CLR_WARP == dict(pipeline.LINK_CLR, warp_s=3.0, threshold=-0.1)
    assert pipeline.LINK_CLR_WARP is linking.LINK_CLR_WARP is clr_model.LINK_CLR_WARP
    assert pipeline._link_model(pipeline.LINK_CLR_WARP) == pipeline._link_model(dict(pipeline.LINK_CLR, threshold=-0.1))
    assert linking._link_options(pipeline.LINK_CLR_WARP, RATE).warp == 375
    assert linking._link_options(pipeline.LINK_CLR, RATE).warp == linking._link_options(pipeline.LINK_CL, RATE).warp == 0


def _float32_neighbours(v):
    v = np.float32(v)
    return float(np.nextafter(v, np.float32(-np.inf))), float(np.nextafter(v, np.float32(np.inf)))


@pytest.mark.parametrize('n', [1, 2, 5, 375, 512])
def test_table_is_the_quantiles_rounded_to_float32(n):
    """Without scipy: every entry brackets its probability under the exact CDF 1/2 erfc(-x / sqrt 2)."""
    tab = pkg('hipabi').warp_table(n)
    assert tab.dtype == np.float32 and tab.shape == (2 * n - 1,)
    assert _bits(tab).tobytes() == _bits(W.table(n)).tobytes()             # binding and restatement: the same bits
    assert (np.diff(tab) > 0).all()
    assert all(tab[k] == -tab[2 * n - 2 - k] for k in range(2 * n - 1))
    assert tab[n - 1] == 0.0 and not np.signbit(tab[n - 1])
    cdf = lambda x: 0.5 * math.erfc(-x / math.sqrt(2.0))
    for k in range(1, 2 * n):
        below, above = _float32_neighbours(tab[k - 1])
        if k == n:
            # the middle: Phi(0) = 1/2 exactly and Phi increases strictly, so the float32 neighbours of 0 bracket it;
            # they are 1.4e-45 away, which erfc in fp64 cannot tell from 0
            assert tab[k - 1] == 0.0 and below < 0.0 < above and cdf(below) <= 0.5 <= cdf(above)
            continue
        assert cdf(below) < k / (2.0 * n) < cdf(above), (n, k)


def _refusals():
    """(name, call(lib, ctx handle) -> status) of every argument refusal of spkd_feature_warp."""
    dev = C.c_void_p(4096)                        # never dereferenced: the refusal comes first
    out = C.c_void_p(4096 + 100 * W.DIM * 4)      # right behind 100 frames, 16-byte aligned
    keep = {}

    def warp(n_frames=100, n_sets=2, off=(0, 1, 3), b=(0, 10, 50), e=(10, 50, 100), window=5, table=np.zeros(64, dtype=np.float32),
             table_len=64, table_off=(0, 0), frames=dev, d_out=out):
        arr = [None if v is None else np.array(v, dtype=np.int64) for v in (off, b, e, table_off)]
        keep[len(keep)] = arr
        p = [None if a is None else _ptr(a) for a in arr]
        tab = None if table is None else _ptr(table)
        return lambda lib, h: lib.spkd_feature_warp(h, frames, n_frames, n_sets, p[0], p[1], p[2], window, tab, table_len, p[3],
                                                    d_out)

    big = 2 ** 31
    return [
        ('null frames', warp(frames=None)), ('null offsets', warp(off=None)), ('null begin', warp(b=None)),
        ('null end', warp(e=None)), ('null table', warp(table=None)), ('null table offsets', warp(table_off=None)),
        ('null output', warp(d_out=None)),
        ('negative frame count', warp(n_frames=-1)), ('negative set count', warp(n_sets=-1)),
        ('window 0', warp(window=0)), ('window -1', warp(window=-1)), ('window past the limit', warp(window=MAX_W + 1)),
        ('offsets not from 0', warp(off=(1, 1, 3))), ('offsets go back', warp(off=(0, 2, 1), b=(0, 10), e=(10, 50))),
        ('begin below 0', warp(b=(-1, 10, 50))), ('end past the frames', warp(e=(10, 50, 101))),
        ('end before begin', warp(b=(0, 20, 50), e=(10, 19, 100))),
        ('ranges overlap inside a set', warp(b=(0, 10, 40))), ('ranges go back inside a set', warp(b=(0, 60, 20), e=(10, 70, 30))),
        ('ranges overlap across sets', warp(b=(0, 5, 50))), ('sets go back', warp(b=(50, 0, 20), e=(60, 10, 30))),
        ('a set of 2^31 frames', warp(n_frames=big + 8, n_sets=1, off=(0, 2), b=(0, 5), e=(5, big + 5), table_off=(0,),
                                      d_out=C.c_void_p(4096 + (big + 8) * W.DIM * 4))),
        ('table slice past the end', warp(table_off=(0, 56))), ('table offset below 0', warp(table_off=(-1, 0))),
        ('table offset past the end', warp(table_off=(65, 0))), ('table too short', warp(table_len=8)),
        ('negative table length', warp(table_len=-1)),
        ('misaligned frames', warp(frames=C.c_void_p(4104))), ('misaligned output', warp(d_out=C.c_void_p(4104 + 100 * W.DIM * 4))),
        ('in place', warp(d_out=dev)), ('output overlaps the frames', warp(d_out=C.c_void_p(4096 + 1600))),
        ('output overlaps from below', warp(frames=out, d_out=C.c_void_p(4096 + 1600))),
    ]


def test_every_refusal_is_einval_without_a_context():
    hipabi = pkg('hipabi')
    lib = hipabi.load_library()
    for name, call in _refusals():
        assert call(lib, None) == hipabi.SPKD_EINVAL, name


def test_refusals_of_the_dictionary_and_of_the_gallery_need_no_device(tmp_path):
    pipeline, gallery, hipabi = pkg('pipeline'), pkg('gallery'), pkg('hipabi')
    files = [pipeline.BatchFile(0, 1000, [(0.0, 8.0)])]
    segments = [np.array([(0.0, 4.0), (4.0, 8.0)])]
    labels = [np.array([1, 2])]
    nan, inf = float('nan'), float('inf')

    def both(link, rate=RATE):
        """the refusal's text, the same from link_batch and from diarize_batch"""
        with pytest.raises(ValueError) as a:
            pipeline.link_batch(None, 0, [0, 2], labels, link, d_frames=0, total_frames=1000, files=files, segments=segments,
                                rate=rate)
        with pytest.raises(ValueError) as b:
            pipeline.diarize_batch(None, 0, 0, [], rate=rate, link=link)
        assert str(a.value) == str(b.value)
        return str(a.value)

    for bad in (nan, inf, -inf, -1.0, 'x', None):
        assert both(dict(pipeline.LINK_CLR_WARP, warp_s=bad)).startswith('link warp_s: a finite number >= 0'), bad
    # the window is round(warp_s * rate) frames, refused where the rate is known: 2 .. SPKD_WARP_MAX_WINDOW
    for warp_s, rate in ((0.011, RATE), (1.5 / RATE - 1e-9, RATE), (4.11, RATE), (512.6 / RATE, RATE), (3.0, 200.0), (0.1, 10.0)):
        assert both(dict(pipeline.LINK_CLR_WARP, warp_s=warp_s), rate).startswith('link warp_s: a window of 2 .. 512 frames'), warp_s
    opts = pkg('linking')._link_options
    assert [opts(dict(pipeline.LINK_CLR_WARP, warp_s=s), r).warp for s, r in ((2.0 / RATE, RATE), (512.4 / RATE, RATE), (3.0, 100.0),
                                                                              (0, RATE), (0.0, 1e9))] == [2, 512, 300, 0, 0]
    # only model clr warps; the model keys are refused first, as ever
    assert both(dict(pipeline.LINK_CL, warp_s=3.0)) == 'link warp_s: only link model clr warps its features'
    assert both(dict(pipeline.LINK_CLR_WARP, warp_s=nan, components=0)) == 'link components: 1 .. 8'
    assert opts(dict(pipeline.LINK_CL, warp_s=0)).warp == 0
    with pytest.raises(ValueError, match='link warp_s'):
        pipeline.warp_batch(None, 0, 1000, files, segments, RATE, 0.0)
    with pytest.raises(ValueError, match='link warp_s'):
        pipeline.warp_batch(None, 0, 1000, files, segments, RATE, 5.0)
    # the gallery keeps the window its records were collected under; a link of another window is refused
    plain, warped = gallery.Gallery(None), gallery.Gallery(None, pipeline.LINK_CLR_WARP)
    slow = gallery.Gallery(None, pipeline.LINK_CLR_WARP, rate=100.0)
    assert (plain.warp, warped.warp, slow.warp, warped.threshold) == (0, 375, 300, -0.1)
    th = dict(threshold=-0.1)
    for link in (dict(pipeline.LINK_CLR_WARP, gallery=plain), dict(pipeline.LINK_CLR, gallery=warped, **th),
                 dict(pipeline.LINK_CLR_WARP, warp_s=2.0, gallery=warped), dict(pipeline.LINK_CLR_WARP, gallery=slow)):
        assert both(link).startswith('link warp_s: the gallery has a window of'), link
    # ... behind the gallery's refusals of components and relevance, which start with theirs
    assert both(dict(pipeline.LINK_CLR_WARP, components=4, gallery=plain)) == 'link components: the gallery has 8'
    assert opts(dict(pipeline.LINK_CLR_WARP, gallery=warped), RATE).warp == 375
    assert opts(dict(pipeline.LINK_CLR_WARP, gallery=slow), 100.0).warp == 300
    with pytest.raises(ValueError, match='link warp_s'):
        gallery.Gallery(None, dict(pipeline.LINK_CLR_WARP, warp_s=5.0))
    # saved and loaded: a gallery without a window has today's keys and bytes, one with a window a scalar more
    today = {'version', 'components', 'relevance', 'threshold', 'ubm', 'records', 'ok', 'frames', 'names'}
    rng = np.random.default_rng(3)
    ubm = rng.normal(0.0, 1.0, (8, hipabi.GMM_COMP))
    rec = rng.normal(0.0, 1.0, (2, 8, hipabi.BW_COMP))
    base = dict(plain.to_arrays(), ubm=ubm, records=rec, ok=np.ones(2, dtype=np.int32), frames=np.array([5.0, 6.0]),
                names=np.array(['a', 'b']))
    assert set(plain.to_arrays()) == set(base) == today
    g0 = gallery.Gallery.from_arrays(None, base)
    assert g0.warp == 0 and set(g0.to_arrays()) == today
    assert all(g0.to_arrays()[k].tobytes() == np.asarray(base[k]).tobytes() for k in today if k != 'names')
    gw = gallery.Gallery.from_arrays(None, dict(base, warp=np.array(375), threshold=np.array(-0.1)))
    arrays = gw.to_arrays()
    assert gw.warp == 375 and set(arrays) == today | {'warp'} and arrays['warp'].shape == () and int(arrays['warp']) == 375
    assert all(arrays[k].tobytes() == g0.to_arrays()[k].tobytes() for k in today - {'threshold'})
    for g, name in ((g0, 'plain.npz'), (gw, 'warped.npz')):
        path = str(tmp_path / name)
        g.save(path)
        with np.load(path, allow_pickle=False) as z:
            assert set(z.files) == set(g.to_arrays())
        again = gallery.Gallery.load(None, path)
        assert again.warp == g.warp and all(again.to_arrays()[k].tobytes() == v.tobytes() for k, v in g.to_arrays().items())
    # an old-format dictionary has no such key: no window
    assert gallery.Gallery.from_arrays(None, {k: v for k, v in arrays.items() if k != 'warp'}).warp == 0
    for bad in (np.array([375]), np.array(1), np.array(513), np.array(-3), np.array(3.5)):
        with pytest.raises(ValueError, match='gallery: warp'):
            gallery.Gallery.from_arrays(None, dict(base, warp=bad))


def test_speech_runs_sort_and_merge_a_files_segments():
    """linking.speech_runs, the one place the runs are stated, against the restatement's loop."""
    linking = pkg('linking')
    per_file = [[(40, 60), (0, 10), (10, 25), (58, 58), (50, 70), (30, 30), (80, 81)],      # out of order, touching, overlapping, empty
                [], [(200, 200)], [(100, 150), (120, 130), (149, 151)], [(90, 95)]]           # nothing; nothing but an empty one; nested
    seg_off = np.concatenate([[0], np.cumsum([len(r) for r in per_file])])
    flat = [r for rs in per_file for r in rs]
    set_off, b, e = linking.speech_runs(seg_off, [x for x, _ in flat], [y for _, y in flat])
    want = sorted([W.speech_runs(rs) for rs in per_file if W.speech_runs(rs)], key=lambda r: r[0][0])
    assert want == [[(0, 25), (40, 70), (80, 81)], [(90, 95)], [(100, 151)]]
    assert [list(zip(b[i:j].tolist(), e[i:j].tolist())) for i, j in zip(set_off[:-1], set_off[1:])] == want
    assert set_off.dtype == b.dtype == e.dtype == np.int64
    empty = linking.speech_runs([0, 0], [], [])
    assert [a.tolist() for a in empty] == [[0], [], []]


def test_restatement_on_exact_data():
    rng = np.random.default_rng(1)
    # a constant column: every window value ties with the frame's -> the middle of the table, exactly 0.0
    x = rng.normal(0.0, 1.0, (40, W.DIM)).astype(np.float32)
    x[:, 7] = 2.5
    for window in (1, 2, 9, 40, 512):
        out = W.warp_set(x, window)
        assert (out[:, 7] == 0.0).all() and not np.signbit(out[:, 7]).any(), window
    # a strictly increasing column of length n under a window of n: rank r of n -> table[2 r] = Phi^-1((r + 1/2) / n)
    for n in (1, 2, 5, 33):
        inc = np.zeros((n, W.DIM), dtype=np.float32)
        inc[:, 3] = np.cumsum(rng.uniform(0.5, 2.0, n)).astype(np.float32)
        inc[:, 4] = -inc[:, 3]
        out = W.warp_set(inc, n)
        assert _bits(out[:, 3]).tobytes() == _bits(W.table(n)[0::2]).tobytes(), n
        assert _bits(out[:, 4]).tobytes() == _bits(W.table(n)[0::2][::-1]).tobytes(), n
        assert _bits(W.warp_set(inc, 512)).tobytes() == _bits(out).tobytes()             # a window longer than the set is the set
    # the window slides and is clamped at both ends: [0, 1, 2, 3, 4, 5, 6] under 3 frames
    ramp = np.zeros((7, W.DIM), dtype=np.float32)
    ramp[:, 0] = np.arange(7)
    t3 = W.table(3)
    assert W.warp_set(ramp, 3)[:, 0].tolist() == [t3[0], t3[2], t3[2], t3[2], t3[2], t3[2], t3[4]]
    # NaN: the quiet NaN, and it counts in nobody's window; -0.0 ties with 0.0
    odd = np.zeros((4, W.DIM), dtype=np.float32)
    odd[:, 0] = [np.nan, 1.0, -0.0, 0.0]
    got = W.warp_set(odd, 4)[:, 0]
    t4 = W.table(4)
    assert _bits(got[:1])[0] == 0x7fc00000 and got[1:].tolist() == [t4[4], t4[1], t4[1]]


def test_restated_warping_links_the_people_across_channels():
    """What the mode is for.  The people of test_link_clr, each file through a channel of its own: plain LINK_CLR
    takes the channels for speakers and links the wrong people; on warped frames the chain finds exactly the
    two people at LINK_CLR_WARP's threshold and 0.1 to either side of it."""
    pipeline = pkg('pipeline')
    feats, clean, _, speakers, person, files = _channel_fixture()
    people = [p + 1 for p in person]
    assert L.link(clean, speakers, pipeline.LINK_CLR)[0].tolist() == people          # (test_link_clr's own claim)
    plain = L.link(feats, speakers, pipeline.LINK_CLR)[0].tolist()
    print('LINK_CLR through the channels: %s' % plain)
    assert plain != people and plain == [1, 2, 1, 2, 2, 1]
    warped = _warped_channel_frames()
    base = pipeline.LINK_CLR_WARP['threshold']
    for th in (base, base - 0.1, base + 0.1):
        lab, merges, smax, smin = L.link(warped, speakers, dict(pipeline.LINK_CLR_WARP, threshold=th))[:4]
        print('LINK_CLR_WARP, threshold %.1f: labels %s, merges %s, initial ratios in [%.3f, %.3f]' % (th, lab.tolist(), merges, smin, smax))
        assert lab.tolist() == people, th
    # W.link, which warps for itself, is that
    assert W.link(feats, speakers, files, pipeline.LINK_CLR_WARP)[0].tolist() == people


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def gpu():
    d = Dev(np.zeros((1, W.DIM), dtype=np.float32))
    yield d
    d.close()


SENTINEL = np.float32(-12345.5)


def _on_device(dev, frames, sets, window, one_set_a_call=False):
    """spkd_feature_warp through the binding on frames [T, 39], sets as warp_numpy.warp takes them, into a
    buffer pre-filled with SENTINEL -> what the buffer holds afterwards."""
    frames = np.ascontiguousarray(frames, dtype=np.float32)
    n = len(frames)
    d_in, d_out = dev.alloc(max(frames.nbytes, 16)), dev.alloc(max(frames.nbytes, 16))
    out = np.full_like(frames, SENTINEL)
    if n:
        dev.ctx.h2d(d_in, frames)
        dev.ctx.h2d(d_out, out)
    for group in ([[s] for s in sets] if one_set_a_call else [sets]):
        off = np.concatenate([[0], np.cumsum([len(r) for r in group])])
        flat = [r for rs in group for r in rs]
        dev.ctx.feature_warp(d_in, n, off, [b for b, _ in flat], [e for _, e in flat], window, d_out)
    if n:
        dev.ctx.d2h(out, d_out)
    for p in (d_in, d_out):
        dev.bufs.remove(p)
        dev.ctx.dev_free(p)
    return out


def _same_bits(got, want):
    bad = np.nonzero(_bits(got) != _bits(want))
    assert len(bad[0]) == 0, 'first of %d differences at frame %d, dimension %d: %r, not %r' % (
        len(bad[0]), bad[0][0], bad[1][0], got[bad[0][0], bad[1][0]], want[bad[0][0], bad[1][0]])


def _restated(frames, sets, window):
    return W.warp(frames, sets, window, np.full_like(np.asarray(frames, dtype=np.float32), SENTINEL))


@pytest.mark.gpu
@pytest.mark.parametrize('window', [2, 5, 6, 375, MAX_W])
def test_every_window_and_set_length_matches_the_restatement(gpu, window):
    """Odd and even windows, a window longer than the set, the clamp at both ends, tile borders with the halo
    to either side: one batch of one-run sets, a gap of three frames between neighbours."""
    lengths = [0, 1, window - 1, window, window + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + window // 2]
    sets, at = [], 2
    for n in lengths:
        sets.append([(at, at + n)])
        at += n + 3
    rng = np.random.default_rng(100 + window)
    frames = rng.normal(0.0, 1.0, (at, W.DIM)).astype(np.float32)
    got = _on_device(gpu, frames, sets, window)
    assert gpu.ctx.last_ms('feature_warp') > 0.0
    _same_bits(got, _restated(frames, sets, window))
    inside = np.zeros(at, dtype=bool)
    for (b, e), in sets:
        inside[b:e] = True
    assert (got[~inside] == SENTINEL).all() and np.isfinite(got[inside]).all() and (~inside).sum() == 2 + 3 * len(lengths)


@pytest.mark.gpu
def test_runs_gaps_and_set_borders(gpu):
    window = 9
    sets = [
        [(5, 105), (105, 105), (110, 111), (120, 120 + TILE - 101), (130 + TILE, 140 + TILE)],      # gaps, a run of 0 and of 1; the third
        [],                                                                                         # run ends on the tile border
        [(150 + TILE, 160 + TILE)],
        [(160 + TILE, 175 + TILE)],                                                                 # touches its neighbour
        [(200 + TILE, 200 + 3 * TILE), (210 + 3 * TILE, 210 + 3 * TILE + 7)],
    ]
    assert sum(e - b for b, e in sets[0][:4]) == TILE
    n = 230 + 3 * TILE
    rng = np.random.default_rng(7)
    frames = rng.normal(0.0, 1.0, (n, W.DIM)).astype(np.float32)
    frames[150 + TILE:160 + TILE] += 1000.0              # two neighbouring sets far apart: a window that crossed
    frames[160 + TILE:175 + TILE] -= 1000.0              # the border would rank every frame at an end
    frames[105:110] = 1e6                                # frames in no range between two runs: never seen
    want = _restated(frames, sets, window)
    got = _on_device(gpu, frames, sets, window)
    _same_bits(got, want)
    inside = np.zeros(n, dtype=bool)
    for rs in sets:
        for b, e in rs:
            inside[b:e] = True
    assert (got[~inside] == SENTINEL).all() and (~inside).sum() > 100
    # (the border would show: a set gives beside its neighbour what it gives alone)
    for b, e in ((150 + TILE, 160 + TILE), (160 + TILE, 175 + TILE)):
        _same_bits(got[b:e], W.warp_set(frames[b:e], window))
    # the same sets with 375 frames of window: every set shorter than it but the last
    _same_bits(_on_device(gpu, frames, sets, 375), _restated(frames, sets, 375))


@pytest.mark.gpu
def test_ties_signed_zeros_infinities_and_nans(gpu):
    rng = np.random.default_rng(11)
    n = 2 * TILE + 150
    frames = rng.integers(-3, 4, (n, W.DIM)).astype(np.float32)             # integer values in [-3, 3]: heavy ties
    frames[:, 5] = 1.25                                                     # a constant dimension
    frames[:, 6] = np.where(rng.integers(0, 2, n) == 0, np.float32(-0.0), np.float32(0.0))
    frames[:, 7] = rng.choice(np.array([-np.inf, -1.0, 0.0, 1.0, np.inf], dtype=np.float32), n)
    frames[:, 8] = rng.normal(0.0, 1.0, n).astype(np.float32)
    frames[rng.choice(n, 40, replace=False), 8] = np.nan                    # single NaNs
    frames[300:420, 9] = np.nan                                             # every window of 300 + 50 .. 420 - 50 is all NaN here
    frames[:, 10] = np.nan                                                  # nothing but NaN
    sets = [[(0, TILE + 40)], [(TILE + 40, n)]]
    for window in (7, 100, 375):
        want = _restated(frames, sets, window)
        got = _on_device(gpu, frames, sets, window)
        _same_bits(got, want)
        assert (got[:, 5] == 0.0).all() and (got[:, 6] == 0.0).all() and not np.signbit(got[:, 5:7]).any()
        assert (_bits(got[:, 10]) == 0x7fc00000).all() and np.isnan(got[300:420, 9]).all()
        assert np.isfinite(got[:, 7]).all() and np.isnan(got[:, 8]).sum() == 40


@pytest.mark.gpu
def test_an_increasing_map_of_a_file_changes_no_bit(gpu):
    """Integer values up to 100 in float32 and g(v) = v^3 + 5 per file, exact below 2^24."""
    rng = np.random.default_rng(13)
    n = TILE + 77
    x = rng.integers(-100, 101, (2 * n, W.DIM)).astype(np.float32)
    g = x.copy()
    g[:n] = x[:n] ** 3 + 5.0
    g[n:] = 3.0 * x[n:] - 7.0
    assert np.abs(g).max() < 2 ** 24 and (g == np.round(g)).all()
    sets = [[(0, n)], [(n, 2 * n)]]
    for window in (6, 375):
        a, b = _on_device(gpu, x, sets, window), _on_device(gpu, g, sets, window)
        assert _bits(a).tobytes() == _bits(b).tobytes(), window
        _same_bits(a, _restated(x, sets, window))


@pytest.mark.gpu
def test_two_calls_and_one_set_a_call_give_the_same_bits(gpu):
    rng = np.random.default_rng(17)
    sets = [[(0, 50), (60, 60 + TILE)], [(100 + TILE, 100 + 2 * TILE + 9)], [(150 + 2 * TILE, 151 + 2 * TILE)]]
    n = 160 + 2 * TILE
    frames = np.round(rng.normal(0.0, 2.0, (n, W.DIM))).astype(np.float32)
    first = _on_device(gpu, frames, sets, 64)
    _same_bits(first, _restated(frames, sets, 64))
    assert _bits(_on_device(gpu, frames, sets, 64)).tobytes() == _bits(first).tobytes()
    assert _bits(_on_device(gpu, frames, sets, 64, one_set_a_call=True)).tobytes() == _bits(first).tobytes()
    # nothing to do, and every refusal with a context: SPKD_EINVAL, nothing written
    hipabi, ctx = gpu.hipabi, gpu.ctx
    d_in, d_out = gpu.alloc(n * W.DIM * 4), gpu.alloc(n * W.DIM * 4)
    ctx.h2d(d_out, first)
    ctx.feature_warp(d_in, n, [0], [], [], 5, d_out)
    ctx.feature_warp(d_in, n, [0, 0, 2, 2], [7, 30], [7, 30], 5, d_out)
    for name, call in _refusals():
        assert call(ctx.lib, ctx.h) == hipabi.SPKD_EINVAL, name
    with pytest.raises(hipabi.SpkdError) as ei:
        ctx.feature_warp(d_in, n, [0, 1], [0], [10], 5, d_in)
    assert ei.value.status == hipabi.SPKD_EINVAL
    after = np.empty_like(first)
    ctx.d2h(after, d_out)
    assert _bits(after).tobytes() == _bits(first).tobytes()


class _Channels(Dev):
    """The channel fixture resident on the device, with what link_batch takes (as test_link_clr's `people`)."""

    def __init__(self):
        feats, _, foff, speakers, person, _ = _channel_fixture()
        Dev.__init__(self, feats)
        sess = _people_fixture()[0]
        self.foff, self.speakers, self.person = foff, speakers, person
        self.files = [self.pipeline.BatchFile(foff[i], len(s[0]), [(a / RATE, b / RATE) for a, b in s[1]]) for i, s in enumerate(sess)]
        self.seg_off = np.concatenate([[0], np.cumsum([len(s[2]) for s in sess])]).astype(np.int64)
        self.labels = [np.array([k // 2 + 1 for _, _, k in s[2]], dtype=np.int32) for s in sess]
        self.segments = [np.array([((a + 0.25) / RATE, (b + 0.25) / RATE) for a, b, _ in s[2]]) for s in sess]

    def link(self, link, first=0, last=3, timings=None, detail=None):
        """link_batch over the files first .. last - 1 -> (the global label of each of their speakers, merges, smax, smin)"""
        off = self.seg_off[first:last + 1] - self.seg_off[first]
        maps, merges, smax, smin = self.pipeline.link_batch(self.ctx, 0, off, self.labels[first:last], link, timings,
                                                            self.eng.d_frames, len(self.frames), self.files[first:last],
                                                            self.segments[first:last], RATE, detail)
        assert all(m.tolist()[:1] == [0] and len(m) == 3 for m in maps)
        return [int(g) for m in maps for g in m[1:]], merges, smax, smin


@pytest.fixture(scope='module')
def channels():
    d = _Channels()
    yield d
    d.close()


@pytest.mark.gpu
def test_link_batch_with_warping_finds_the_people_across_channels(channels):
    p = channels.pipeline
    people = [q + 1 for q in channels.person]
    # the stage on its own: the restatement's frames to the bit, a frame of no segment untouched
    d_out = channels.alloc(channels.frames.nbytes)
    channels.ctx.h2d(d_out, np.full_like(channels.frames, SENTINEL))
    assert p.warp_batch(channels.ctx, channels.eng.d_frames, len(channels.frames), channels.files, channels.segments, RATE,
                        p.LINK_CLR_WARP['warp_s'], d_out) == d_out
    got = np.empty_like(channels.frames)
    channels.ctx.d2h(got, d_out)
    want = _warped_channel_frames()
    inside = np.zeros(len(got), dtype=bool)
    for rs in channels.speakers:
        for b, e in rs:
            inside[b:e] = True
    _same_bits(got[inside], want[inside])
    assert (got[~inside] == SENTINEL).all()
    # the chain on them: the restatement's labels and log, the two people
    lab, merges, smax, smin = L.link(want, channels.speakers, p.LINK_CLR_WARP)[:4]
    timings = {}
    got_lab, got_merges, got_max, got_min = channels.link(p.LINK_CLR_WARP, timings=timings)
    print('merges %s, initial ratios in [%.3f, %.3f]' % (got_merges, got_min, got_max))
    assert got_lab == lab.tolist() == people
    _same_log(dict(status=0, a=np.array([a for a, _, _ in got_merges]), b=np.array([b for _, b, _ in got_merges]),
                   d=np.array([d for _, _, d in got_merges]), stat_max=got_max, stat_min=got_min), (merges, smax, smin, True))
    assert all(len(timings[k]) == 1 and timings[k][0] > 0.0 for k in ('link_warp', 'link_ubm_train', 'link_ubm_stats', 'link_clr'))
    # without warping the channels are taken for speakers, on the device as restated
    assert channels.link(p.LINK_CLR)[0] == L.link(channels.frames, channels.speakers, p.LINK_CLR)[0].tolist() != people


@pytest.mark.gpu
def test_a_gallery_keeps_the_identities_across_calls_and_channels(channels):
    p, gallery = channels.pipeline, pkg('gallery')
    want_gal = GN.Gallery(p.LINK_CLR_WARP)
    warped = _warped_channel_frames()
    want = [GN.link(warped, channels.speakers[a:b], p.LINK_CLR_WARP, want_gal)['labels'].tolist() for a, b in ((0, 4), (4, 6))]
    assert want == [[1, 2, 1, 2], [1, 2]]                                  # files 0 and 1 enrol the two people, file 2 meets them
    g = gallery.Gallery(channels.ctx, p.LINK_CLR_WARP)
    try:
        link = dict(p.LINK_CLR_WARP, gallery=g)
        det = {}
        assert channels.link(link, 0, 2, detail=det)[0] == want[0] and det['enrolled'] == [0, 1] and g.n == 2
        assert channels.link(link, 2, 3, detail=det)[0] == want[1] and det['enrolled'] == [] and g.n == 2
        assert g.warp == 375 and int(g.to_arrays()['warp']) == 375
        with pytest.raises(ValueError, match='link warp_s: the gallery'):
            channels.link(dict(p.LINK_CLR, gallery=g))
    finally:
        g.close()


@pytest.mark.gpu
def test_diarize_batch_with_and_without_warping_end_to_end():
    synth, p = pkg('synth'), pkg('pipeline')
    series = synth.make_series([21, 22, 23], 40.0, 555)
    d = Dev(np.concatenate([s[0] for s in series]))
    try:
        foff = np.concatenate([[0], np.cumsum([len(s[0]) for s in series])])
        files = [p.BatchFile(foff[i], len(s[0]), [(a / RATE, b / RATE) for a, b in s[1]]) for i, s in enumerate(series)]
        args = (d.ctx, d.eng.d_frames, len(d.frames), files)
        calls = []
        real = d.ctx.feature_warp
        d.ctx.feature_warp = lambda *a: (calls.append(a[5]), real(*a))[1]
        plain = p.diarize_batch(*args, rate=RATE)
        # LINK_CLR: no warping call, no link_warp time, the rows of a dictionary whose warp_s is 0
        tm, det = {}, {}
        linked = p.diarize_batch(*args, rate=RATE, link=p.LINK_CLR, timings=tm, detail=det)
        assert calls == [] and 'link_warp' not in tm and 'link_warped' not in d.ctx.__dict__.get('_dev_scratch', {})
        zero = p.diarize_batch(*args, rate=RATE, link=dict(p.LINK_CLR, warp_s=0.0))
        assert calls == [] and [r.tobytes() for r in zero] == [r.tobytes() for r in linked]
        for f in range(3):
            assert linked[f][:, :2].tobytes() == plain[f][:, :2].tobytes()
            assert np.array_equal(linked[f][:, 2], det['link']['maps'][f][plain[f][:, 2].astype(np.int64)])
        # LINK_CLR_WARP: one warping call of 375 frames, the same segments, the labels through its maps
        tm2, det2 = {}, {}
        warped = p.diarize_batch(*args, rate=RATE, link=p.LINK_CLR_WARP, timings=tm2, detail=det2)
        assert calls == [375] and len(tm2['link_warp']) == 1 and tm2['link_warp'][0] > 0.0
        maps = det2['link']['maps']
        assert len(maps) == 3 and all(len(r) for r in warped)
        for f in range(3):
            assert warped[f][:, :2].tobytes() == plain[f][:, :2].tobytes()
            assert np.array_equal(warped[f][:, 2], maps[f][plain[f][:, 2].astype(np.int64)])
            assert warped[f][:, 2].min() >= 1
        n_glob = len(set(int(g) for m in maps for g in m[1:] if g))
        assert n_glob == sum(int((m[1:] > 0).sum()) for m in maps) - len(det2['link']['merges'])
        # and LINK_CLR after it is what it was before it
        again = p.diarize_batch(*args, rate=RATE, link=p.LINK_CLR)
        assert calls == [375] and [r.tobytes() for r in again] == [r.tobytes() for r in linked]
    finally:
        d.close()
