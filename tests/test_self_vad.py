"""The self-trained speech / non-speech detector: spkd_frame_energy_batch and spkd_energy_seeds against
their numpy restatement (tests/self_vad_numpy.py) EXACTLY -- both are integer arithmetic -- and the stage
built on them (self_vad.decode_batch, pipeline.vad_batch / diarize_pcm_batch with pipeline.SELF_VAD,
./generate_exp.py --self-trained) on the three recordings of tests/test_mfcc_batch.py.

The accuracy condition: per recording the decoded 'p' runs are as many as the stretches the signal was
drawn with, one per stretch, and every border lies within CAP = 8 frames of the true one.  The 8 is
derived, not measured: a frame's window spans 400 / 128 = 3.1 hops and the delta chain reaches 4 frames
to either side (MFCC_POST_HALO), so the frames up to 8 from a border see both sides of it.  The numpy
restatement meets it on the CPU; the device must meet the same cap."""
import ctypes as C
import io
import json
import os
import re

import numpy as np
import pytest

import self_vad_numpy as S
from conftest import pkg
from helpers import ROOT
from test_frontend import GOLD, _cfg_text
from test_generate_exp import _write_wav
from test_mfcc_batch import TALKS, _cfg, _talk

HOP, WINDOW = 128, 400
CAP = 8
GUARD = 64                                          # int64 entries behind the energies, which the call must not touch
GUARD_PATTERN = 0x7ff8dead7ff8dead
PER_TILE = 16384 // HOP                             # frames a workgroup of k_frame_energy takes (SPKD_ENERGY_TILE / hop)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------ the inputs
# samples per file: around a hop, around a window, around a workgroup's frames; empty files first, in the
# middle and last; the odd lengths leave the files behind them at odd sample offsets
LENGTHS = [0, 1, HOP - 1, HOP, HOP + 1, WINDOW - 1, WINDOW, WINDOW + HOP - 1, 0, PER_TILE * HOP - 1, PER_TILE * HOP,
           PER_TILE * HOP + 1, (PER_TILE + 1) * HOP, 2 * PER_TILE * HOP + 5 * HOP + 77, 3001, 3000, 0]


def _energy_files():
    """Full-scale noise next to noise in [-3, 3] (a leak across a file border shows at that level); the
    last two files with samples are a constant -32768 (energy exactly 0: window sum s^2 and (sum s)^2 cancel near
    1.7e14) and -32768 / 32767 in turn (the largest value)."""
    rng = np.random.default_rng(20261020)
    files = [(rng.integers(-32768, 32768, n) if i % 2 else rng.integers(-3, 4, n)).astype(np.int16)
             for i, n in enumerate(LENGTHS)]
    files[-3][:] = -32768
    files[-2][0::2] = -32768
    files[-2][1::2] = 32767
    return files


_RESTATED = {}


def _talks():
    """The three recordings with their stretches, and the restatement's decode of them (once)."""
    if not _RESTATED:
        from oracle import mfcc_numpy as m
        cfg = _cfg(WINDOW)
        pcms, stretches = zip(*[S.talk(seconds, seed) for seconds, seed in TALKS])
        feats = [m.features(p, cfg) for p in pcms]
        energies = [S.energy_fast(p, cfg.hop, cfg.window_width) for p in pcms]
        tokens, untrained, passes = S.decode_batch(feats, energies, pkg('self_vad').SELF_VAD, float(cfg.frame_rate))
        _RESTATED.update(pcms=list(pcms), stretches=list(stretches), tokens=tokens, untrained=untrained, passes=passes,
                         counts=[len(f) for f in feats])
    return _RESTATED


def _meets_the_cap(tokens, stretches, counts, who):
    for f, (toks, st, T) in enumerate(zip(tokens, stretches, counts)):
        got, want, worst = S.border_errors(toks, st, T, HOP)
        print('%s, file %d: %d runs for %d stretches, worst border %s frames' % (who, f, len(got), len(want), worst))
        assert len(got) == len(want), (who, f, got, want)
        assert all(a < d and c < b for (a, b), (c, d) in zip(got, want)), (who, f)      # one per stretch: they overlap
        assert worst <= CAP, (who, f, worst, got, want)


# ------------------------------------------------------------------ not GPU
def test_entry_points_and_timers_are_declared_and_exported():
    hipabi = pkg('hipabi')
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'spkd.h')).read(), flags=re.S)
    lib = hipabi.load_library()
    for name in ('spkd_frame_energy_batch', 'spkd_energy_seeds'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in hipabi.EXPORTS and hasattr(lib, name), name
    assert hipabi.EXPORTS[-2:] == ['spkd_frame_energy_batch', 'spkd_energy_seeds']
    assert 'spkd_*' in open(os.path.join(ROOT, 'speaker-diarization_amd', 'csrc', 'libspkd_hip.map')).read()
    names = [n for n, _ in sorted(hipabi.TIMERS.items(), key=lambda kv: kv[1])]
    enum = re.search(r'enum \{\s*SPKD_T_CALL = 0,(.*?)SPKD_N_TIMERS', code, flags=re.S).group(1)
    assert ['call'] + [n.strip()[len('SPKD_T_'):].lower() for n in enum.split(',') if n.strip()] == names
    # behind resample, the stage in front of them; the front-end's two stay the last
    assert names[names.index('resample'):][:3] == ['resample', 'frame_energy', 'energy_seeds']
    assert names[-2:] == ['mfcc_static', 'mfcc_post'] and len(names) == len(set(names))
    assert re.search(r'#define SPKD_ENERGY_MAX_WINDOW %d\b' % hipabi.ENERGY_MAX_WINDOW, code)
    assert re.search(r'#define SPKD_ENERGY_TILE %d\b' % hipabi.ENERGY_TILE, code) and hipabi.ENERGY_TILE // HOP == PER_TILE
    assert lib.spkd_abi_version() == 2
    assert hasattr(hipabi.Context, 'frame_energy_batch') and hasattr(hipabi.Context, 'energy_seeds')
    assert pkg('pipeline').SELF_VAD is pkg('self_vad').SELF_VAD


def _refusals():
    """(name, call(lib, ctx handle) -> status) of every argument refusal of the two entry points."""
    good = np.array([0, 300, 1000], dtype=np.int64)
    dev, odd = C.c_void_p(256), C.c_void_p(257)    # never dereferenced: the refusal comes first
    keep = []

    def energy(off=good, n=2, hop=HOP, window=WINDOW, frame_off=True, d_pcm=dev, d_out=dev):
        out = np.zeros(3, dtype=np.int64)
        keep.append(out)
        return lambda lib, h: lib.spkd_frame_energy_batch(h, d_pcm, None if off is None else _ptr(off), n, hop, window,
                                                          d_out, _ptr(out) if frame_off else None)

    k = np.array([1, 1], dtype=np.int64)
    res64, res32 = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int32)
    outs = [C.c_void_p() for _ in range(3)]
    keep.extend([k, res64, res32, outs])
    long_file = np.array([0, 1 << 31], dtype=np.int64)

    def seeds(off=good, n=2, d_e=dev, kl=k, kh=k, lo=res64, hi=res64, seeded=res32, out=(0, 1, 2)):
        q = lambda v: None if v is None else _ptr(v)
        o = [C.byref(outs[i]) if i in out else None for i in range(3)]
        return lambda lib, h: lib.spkd_energy_seeds(h, d_e, q(off), n, q(kl), q(kh), q(lo), q(hi), q(seeded), *o)

    return [('energy: hop 0', energy(hop=0)), ('energy: hop above the window', energy(hop=401)),
            ('energy: window 4097', energy(window=4097)), ('energy: negative window', energy(hop=-2, window=-1)),
            ('energy: negative file count', energy(n=-1)), ('energy: null sample_off', energy(off=None)),
            ('energy: null frame_off', energy(frame_off=False)),
            ('energy: sample_off not from 0', energy(off=np.array([1, 300, 1000], dtype=np.int64))),
            ('energy: decreasing sample_off', energy(off=np.array([0, 300, 200], dtype=np.int64))),
            ('energy: null samples with a frame', energy(d_pcm=None)), ('energy: null energies with a frame', energy(d_out=None)),
            ('energy: samples at an odd address', energy(d_pcm=odd)), ('energy: misaligned energies', energy(d_out=odd)),
            ('seeds: null run_off', seeds(out=(1, 2))), ('seeds: null run_begin', seeds(out=(0, 2))),
            ('seeds: null run_end', seeds(out=(0, 1))), ('seeds: negative file count', seeds(n=-1)),
            ('seeds: null frame_off', seeds(off=None)),
            ('seeds: frame_off not from 0', seeds(off=np.array([1, 300, 1000], dtype=np.int64))),
            ('seeds: decreasing frame_off', seeds(off=np.array([0, 300, 200], dtype=np.int64))),
            ('seeds: null k_low', seeds(kl=None)), ('seeds: null k_high', seeds(kh=None)), ('seeds: null lo', seeds(lo=None)),
            ('seeds: null hi', seeds(hi=None)), ('seeds: null seeded', seeds(seeded=None)),
            ('seeds: a file of 2^31 frames', seeds(off=long_file, n=1)),
            ('seeds: null energies with a frame', seeds(d_e=None)), ('seeds: misaligned energies', seeds(d_e=odd))]


def test_every_refusal_is_einval_without_a_context():
    hipabi = pkg('hipabi')
    lib = hipabi.load_library()
    for name, call in _refusals():
        assert call(lib, None) == hipabi.SPKD_EINVAL, name


def test_the_options_are_parsed_before_any_device_work():
    sv, pipeline = pkg('self_vad'), pkg('pipeline')
    nan, inf = float('nan'), float('inf')
    o = sv._options(sv.SELF_VAD)
    assert o == (0.10, 0.10, 4, 5, 0.01, 10.0, 0.2, o.passes) and o.passes >= 1
    assert sv._options({}) == o and sv._options(dict(passes=1)).passes == 1
    assert sv._options(dict(low_share=0.5, high_share=0.5, components=8, iterations=0, var_floor=0.0, penalty=0.0,
                            min_dur_s=0.0)).components == 8
    bad = [(dict(low_share=0.0), 'low_share'), (dict(low_share=0.51), 'low_share'), (dict(low_share=nan), 'low_share'),
           (dict(low_share=-0.1), 'low_share'), (dict(high_share=0.0), 'high_share'), (dict(high_share=0.6), 'high_share'),
           (dict(high_share='a tenth'), 'high_share'), (dict(components=0), 'components'), (dict(components=9), 'components'),
           (dict(components=2.5), 'components'), (dict(components=True), 'components'), (dict(iterations=-1), 'iterations'),
           (dict(iterations=1.5), 'iterations'), (dict(var_floor=-0.01), 'var_floor'), (dict(var_floor=nan), 'var_floor'),
           (dict(var_floor=inf), 'var_floor'), (dict(penalty=-1.0), 'penalty'), (dict(penalty=nan), 'penalty'),
           (dict(penalty=inf), 'penalty'), (dict(min_dur_s=-0.1), 'min_dur_s'), (dict(min_dur_s=inf), 'min_dur_s'),
           (dict(min_dur_s=nan), 'min_dur_s'), (dict(passes=0), 'passes'), (dict(passes=2.0), 'passes'),
           (dict(passes=-1), 'passes'), (dict(passes=None), 'passes'), (dict(shares=0.1), "unknown key 'shares'")]
    cfg = _cfg(WINDOW)
    pcms = [np.zeros(4000, dtype=np.int16)]
    for change, match in bad:
        opts = dict(sv.SELF_VAD, **change)
        with pytest.raises(ValueError, match=match):
            sv._options(opts)
        with pytest.raises(ValueError, match=match):
            sv.decode_batch(None, opts, cfg, 0, [0, 4000], 0, [0, 31])
        with pytest.raises(ValueError, match=match):
            pipeline.vad_batch(None, opts, pcms, cfg=cfg)
        with pytest.raises(ValueError, match=match):
            pipeline.diarize_pcm_batch(None, opts, cfg, pcms)
        with pytest.raises(ValueError, match=match):
            pipeline.diarize_audio_batch(None, opts, cfg, [(pcms[0], 16000)])
    assert sv.seed_counts(sv.SELF_VAD, 2875) == (287, 287) and sv.seed_counts(sv.SELF_VAD, 9) == (0, 0)
    assert sv.min_frames(sv.SELF_VAD, 125) == 25 and sv.min_frames(dict(min_dur_s=0.0), 125) == 1
    assert sv.token_ranges([(0, 0), (10, 1), (30, 0)], 100, 50) == ([(100, 110), (130, 150)], [(110, 130)])


def test_the_model_path_takes_neither_new_keyword_and_the_options_need_cfg():
    pipeline = pkg('pipeline')
    model = object()                               # (anything that is no dictionary is a model: it is not looked at)
    cfg = _cfg(WINDOW)
    pcms = [np.zeros(4000, dtype=np.int16)]
    for kw in (dict(cfg=cfg), dict(features=(0, 31, [0, 31])), dict(cfg=cfg, features=(0, 31, [0, 31])), dict(cfg=None),
               dict(features=None)):
        with pytest.raises(ValueError, match='not with a VadModel'):
            pipeline.vad_batch(None, model, pcms, **kw)
    with pytest.raises(ValueError, match='cfg is required'):
        pipeline.vad_batch(None, pipeline.SELF_VAD, pcms)
    with pytest.raises(ValueError, match='cfg is required'):
        pipeline.vad_batch(None, pipeline.SELF_VAD, pcms, cfg=None, features=(0, 31, [0, 31]))
    with pytest.raises(ValueError, match='frames a second'):
        pipeline.vad_batch(None, pipeline.SELF_VAD, pcms, opt=pkg('voice_detection').VadOptions(rate=100), cfg=cfg)


def test_the_command_lines_name_the_mode():
    eg, orch = pkg('exp_generator'), pkg('orchestrator')
    out = []
    assert eg.main(['/nowhere/x.recipe', '--self-trained', '/nowhere/fconfig.cfg'], say=lambda *a: out.append(a)) == 0
    assert out == [('ERROR:', '/nowhere/x.recipe', 'does not exist.')]
    buf = io.StringIO()
    import contextlib
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        eg.main(['--help'])
    text = ' '.join(buf.getvalue().split())
    assert '--self-trained FCONFIG' in text and 'accepted and unused with --self-trained' in text
    assert orch.SELF_VAD_ARGS == ['--self-trained', '{fcfg}'] and orch.EXP_STAGE[0] == './generate_exp.py'


def test_the_restatement_states_the_two_calls():
    rng = np.random.default_rng(5)
    pcm = rng.integers(-32768, 32768, 3000).astype(np.int16)
    e = S.energy(pcm, HOP, WINDOW)
    assert e.dtype == np.int64 and len(e) == 23 and np.array_equal(e, S.energy_fast(pcm, HOP, WINDOW))
    w = pcm[22 * HOP:].astype(object)              # the last frame runs past the end: 184 samples and zeros
    assert len(w) == 184 and int(e[22]) == WINDOW * int((w * w).sum()) - int(w.sum()) ** 2
    assert not S.energy(np.full(1000, -32768, dtype=np.int16), HOP, WINDOW)[:4].any()
    assert S.runs([1, 1, 0, 1, 0, 0, 1]) == [(0, 2), (3, 4), (6, 7)] and S.runs([]) == [] and S.runs([0]) == []
    assert S.seeds_file([5, 1, 9, 1, 7], 2, 1) == (1, 9, 1, ([(1, 2), (3, 4)], [(2, 3)]))
    assert S.seeds_file([5, 1, 9, 1, 7], 3, 3) == (5, 5, 0, ([], []))
    assert S.seeds_file([5, 1, 9], 0, 1)[2] == 0 and S.seeds_file([5, 1, 9], 1, 4)[2] == 0 and S.seeds_file([], 0, 0)[2] == 0
    lo, hi, seeded, off, b, e2 = S.seeds([[1, 9, 1], [4, 4], [9, 1]], [1, 1, 1], [1, 1, 1])
    assert list(seeded) == [1, 0, 1] and list(off) == [0, 2, 3, 3, 3, 4, 5]
    assert list(b) == [0, 2, 1, 6, 5] and list(e2) == [1, 3, 2, 7, 6]


def test_the_talks_are_those_of_the_front_end_tests():
    t = _talks()
    for (seconds, seed), pcm, st in zip(TALKS, t['pcms'], t['stretches']):
        assert np.array_equal(pcm, _talk(seconds, seed)) and len(st) >= 7


def test_the_restatement_meets_the_accuracy_condition():
    t = _talks()
    assert t['untrained'] == [] and 1 <= t['passes'] <= pkg('self_vad').SELF_VAD['passes']
    _meets_the_cap(t['tokens'], t['stretches'], t['counts'], 'restatement')


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def ctx():
    c = pkg('hipabi').Context(0)
    yield c
    c.close()


def _energies(ctx, pcms, hop=HOP, window=WINDOW):
    """frame_energy_batch into a buffer with GUARD entries of a pattern behind the energies ->
    (energies int64 [sum T], the guard entries as uint64, frame_off)."""
    fe = pkg('frontend')
    d_pcm, sample_off = fe.upload_batch(ctx, pcms)
    total = int(fe.frame_offsets(sample_off, hop)[-1])
    buf = np.full(total + GUARD, GUARD_PATTERN, dtype=np.uint64)
    d_out = ctx.dev_scratch('test_self_vad_energy', buf.nbytes)
    ctx.h2d(d_out, buf)
    frame_off = ctx.frame_energy_batch(d_pcm, sample_off, hop, window, d_out)
    assert np.array_equal(frame_off, fe.frame_offsets(sample_off, hop)) and frame_off.dtype == np.int64
    ctx.d2h(buf, d_out)
    return buf[:total].view(np.int64), buf[total:], frame_off


@pytest.fixture(scope='module')
def energy_want():
    files = _energy_files()
    return files, [S.energy_fast(p, HOP, WINDOW) for p in files]


@pytest.mark.gpu
def test_energies_of_a_batch_are_exact(ctx, energy_want):
    files, want = energy_want
    assert np.array_equal(want[7], S.energy(files[7], HOP, WINDOW)) and np.array_equal(want[9], S.energy(files[9], HOP, WINDOW))
    got, guard, frame_off = _energies(ctx, files)
    assert [int(n) for n in np.diff(frame_off)] == [n // HOP for n in LENGTHS]
    for i, w in enumerate(want):
        g = got[frame_off[i]:frame_off[i + 1]]
        assert np.array_equal(g, w), 'file %d (%d samples): first differing frame %d' % (
            i, LENGTHS[i], int(np.nonzero(g != w)[0][0]))
    assert np.all(guard == GUARD_PATTERN)
    # the constant file: exactly 0 wherever the window lies inside it (the last two frames run past its end)
    assert len(want[-3]) == 23 and not want[-3][:21].any() and int(want[-3][22]) > 0
    s2 = 200 * (32768 ** 2 + 32767 ** 2)
    assert int(want[-2][0]) == WINDOW * s2 - 200 ** 2                       # -32768 / 32767 in turn: sum s = -200
    assert int(max(w.max() for w in want if len(w))) < 1 << 55
    # the loud and the quiet files do differ by what a leaked sample would carry
    assert int(want[10].max()) < 400 * 400 * 9 and int(want[9].min()) > 1 << 40


@pytest.mark.gpu
def test_a_files_energies_depend_neither_on_its_neighbours_nor_on_the_order(ctx, energy_want):
    files, want = energy_want
    for i, p in enumerate(files):
        got, guard, frame_off = _energies(ctx, [p])
        assert list(frame_off) == [0, len(p) // HOP] and np.array_equal(got, want[i]), i
        assert np.all(guard == GUARD_PATTERN)
    order = list(np.random.default_rng(4).permutation(len(files)))
    assert order != sorted(order)
    got, guard, frame_off = _energies(ctx, [files[i] for i in order])
    for slot, i in enumerate(order):
        assert np.array_equal(got[frame_off[slot]:frame_off[slot + 1]], want[i]), (slot, i)
    assert np.all(guard == GUARD_PATTERN)


@pytest.mark.gpu
def test_the_widest_window_at_full_scale_stays_exact(ctx):
    """hop = window = 4096: the header's bound.  -32768 / 32767 in turn gives the largest value a frame can
    take, 4096 * 2048 * (2^30 + 32767^2) - 2048^2, just below 2^54."""
    rng = np.random.default_rng(7)
    turn = np.empty(3 * 4096 + 5, dtype=np.int16)
    turn[0::2], turn[1::2] = -32768, 32767
    files = [turn, np.full(2 * 4096 + 4095, -32768, dtype=np.int16), rng.integers(-32768, 32768, 5 * 4096 + 1).astype(np.int16),
             np.full(4096, 32767, dtype=np.int16)]
    got, guard, frame_off = _energies(ctx, files, 4096, 4096)
    assert list(np.diff(frame_off)) == [3, 2, 5, 1]
    for i, p in enumerate(files):
        assert np.array_equal(got[frame_off[i]:frame_off[i + 1]], S.energy_fast(p, 4096, 4096)), i
    top = 4096 * 2048 * (2 ** 30 + 32767 ** 2) - 2048 ** 2
    assert [int(v) for v in got[:3]] == [top] * 3 and (1 << 53) < top < (1 << 54)
    assert not got[3:5].any() and int(got[-1]) == 0
    assert np.all(guard == GUARD_PATTERN)
    # other shapes: a hop of one sample under the widest window, and a window that is no multiple of the hop
    for hop, window, n in ((1, 4096, 16384 + 300), (100, 257, 35003), (3, 3, 16390)):
        p = rng.integers(-32768, 32768, n).astype(np.int16)
        got, guard, frame_off = _energies(ctx, [p[:7], p], hop, window)
        assert np.array_equal(got[frame_off[1]:], S.energy_fast(p, hop, window)), (hop, window)
        assert np.array_equal(got[:frame_off[1]], S.energy_fast(p[:7], hop, window)) and np.all(guard == GUARD_PATTERN)


def _seed_cases():
    """(energies per file, k_low, k_high)."""
    rng = np.random.default_rng(11)
    big = 1 << 54
    pattern = np.array([7, 7, 0, 3, 900, 900, 3, big, 5, 7, 0], dtype=np.int64)
    long_file = np.repeat(pattern, 6500)            # 71 500 frames: runs of 6 500, ties at both thresholds
    spread = rng.integers(0, big, 3000, dtype=np.int64)
    ties = np.array([5] * 4 + [1, 2, 5, 5, 9, 9, 3, 9, 5, 1] + [9] * 3, dtype=np.int64)
    files = [
        (np.zeros(0, dtype=np.int64), 0, 0),                       # no frame
        (np.array([4], dtype=np.int64), 1, 1),                     # one frame: lo == hi
        (np.array([4, 9], dtype=np.int64), 1, 1),                  # two frames, k = 1
        (np.array([4, 9], dtype=np.int64), 2, 2),                  # k equal to the frame count: lo = 9 > hi = 4
        (np.array([9, 4, 6], dtype=np.int64), 1, 1),
        (np.array([9, 4, 6], dtype=np.int64), 3, 1),               # lo the largest: lo == hi
        (np.array([9, 4, 6], dtype=np.int64), 0, 1),               # k = 0
        (np.array([9, 4, 6], dtype=np.int64), 1, 4),               # k above the frame count
        (np.full(50, 77, dtype=np.int64), 5, 5),                   # equal energies: not seeded
        (ties, 5, 4),                                              # lo = 5 and hi = 9 with ties at both; runs touch both ends
        (np.array([1, 1, 8, 8, 2, 8, 1, 1], dtype=np.int64), 4, 3),    # ends in class 0 ...
        (np.array([1, 8, 1, 8, 8], dtype=np.int64), 2, 3),         # ... and the next file begins in it: no join across the border
        (np.array([8, 8, 1], dtype=np.int64), 1, 2),               # begins in class 1 right behind a file that ends in it
        (long_file, 6500 * 2 + 10, 6500),
        (spread, 300, 300),
        (np.concatenate([spread[:1500], np.full(700, int(spread[7]), dtype=np.int64), spread[1500:]]), 1100, 1100),
        (np.zeros(0, dtype=np.int64), 1, 1),
    ]
    return [e for e, _, _ in files], [kl for _, kl, _ in files], [kh for _, _, kh in files]


@pytest.mark.gpu
def test_seeds_are_exact(ctx):
    energies, k_low, k_high = _seed_cases()
    want = S.seeds(energies, k_low, k_high)
    assert list(want[2]) == [0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 0]
    assert len(energies[13]) > 65536 and int(want[0][9]) == 5 and int(want[1][9]) == 9
    flat = np.concatenate(energies)
    frame_off = np.concatenate([[0], np.cumsum([len(e) for e in energies])]).astype(np.int64)
    d_e = ctx.dev_scratch('test_self_vad_seed_energy', flat.nbytes)
    ctx.h2d(d_e, flat)
    for _ in range(2):                                   # (the second call reuses the context's buffers)
        got = ctx.energy_seeds(d_e, frame_off, k_low, k_high)
        for name, g, w in zip(('lo', 'hi', 'seeded', 'run_off', 'run_begin', 'run_end'), got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), name
    run_off, begin, end = want[3], want[4], want[5]
    # the runs as spkd_gmm_train takes them: inside their file, ascending, apart; the two border files do not join
    for f in range(len(energies)):
        for c in (0, 1):
            b, e = begin[run_off[2 * f + c]:run_off[2 * f + c + 1]], end[run_off[2 * f + c]:run_off[2 * f + c + 1]]
            assert np.all(b < e) and np.all(b[1:] > e[:-1]) and (len(b) == 0 or (b[0] >= frame_off[f] and e[-1] <= frame_off[f + 1]))
    assert end[run_off[2 * 10 + 1] - 1] == frame_off[11] and begin[run_off[2 * 11]] == frame_off[11]
    # a batch without a frame, and no file at all
    got = ctx.energy_seeds(0, [0, 0, 0], [1, 0], [1, 0])
    assert list(got[2]) == [0, 0] and list(got[3]) == [0] * 5 and len(got[4]) == len(got[5]) == 0
    got = ctx.energy_seeds(0, [0], [], [])
    assert list(got[3]) == [0] and len(got[0]) == 0


@pytest.mark.gpu
def test_refusals_on_a_context_name_their_reason_and_leave_it_usable(ctx, energy_want):
    hipabi = pkg('hipabi')
    for name, call in _refusals():
        assert call(ctx.lib, ctx.h) == hipabi.SPKD_EINVAL, name
        assert ctx.lib.spkd_last_error(ctx.h).decode() != '', name
    with pytest.raises(hipabi.SpkdError, match='1 <= hop <= window <= 4096'):
        ctx.frame_energy_batch(256, [0, 400], 128, 64, 256)
    with pytest.raises(hipabi.SpkdError, match='one entry per file'):
        ctx.energy_seeds(256, [0, 4], [1, 1], [1])
    assert list(ctx.frame_energy_batch(0, [0, 100, 227], HOP, WINDOW, 0)) == [0, 0, 0]       # no frame: nothing launched
    files, want = energy_want
    got, guard, frame_off = _energies(ctx, files[:8])
    assert np.array_equal(got, np.concatenate(want[:8])) and np.all(guard == GUARD_PATTERN)


@pytest.fixture(scope='module')
def decoded(ctx):
    """The three recordings through self_vad.decode_batch: (cfg, pcms, tokens, last_frames, detail, timings)."""
    fe, sv = pkg('frontend'), pkg('self_vad')
    cfg = _cfg(WINDOW)
    pcms = _talks()['pcms']
    detail, timings = {}, {}
    tokens, last = _decode(ctx, cfg, pcms, detail, timings)
    return cfg, pcms, tokens, last, detail, timings


def _decode(ctx, cfg, pcms, detail=None, timings=None):
    fe, sv = pkg('frontend'), pkg('self_vad')
    d_pcm, sample_off = fe.upload_batch(ctx, pcms)
    d_frames, frame_off = fe.extract_batch(ctx, cfg, d_pcm, sample_off)
    return sv.decode_batch(ctx, sv.SELF_VAD, cfg, d_pcm, sample_off, d_frames, frame_off, timings, detail)


@pytest.mark.gpu
def test_the_device_meets_the_accuracy_condition(ctx, decoded):
    cfg, pcms, tokens, last, detail, timings = decoded
    t = _talks()
    assert last == t['counts'] == [len(p) // HOP for p in pcms]
    assert detail['vad_untrained'] == [] and 1 <= detail['vad_passes_run'] <= pkg('self_vad').SELF_VAD['passes']
    assert all(w in ('p', '<w>') for toks in tokens for _, w in toks) and all(toks[0][0] == 0 for toks in tokens)
    _meets_the_cap(tokens, t['stretches'], t['counts'], 'device')
    n = detail['vad_passes_run']
    assert len(timings['vad_energy']) == len(timings['vad_seeds']) == 1
    assert len(timings['vad_loglik']) == len(timings['vad_viterbi']) == len(timings['vad_backtrack']) == n
    assert n <= len(timings['vad_gmm_train']) <= n + 1
    # where the device and the restatement differ (their mixtures differ in rounding): written down, not asserted
    borders = lambda toks: set((at, w) for at, w in toks)
    differ = [len(borders(a) ^ borders(b)) for a, b in zip(tokens, t['tokens'])]
    print('token borders on which the device and the restatement differ, per file:', differ)
    record = dict(what='per file, the token borders (first frame, word) that only one of the device and the numpy '
                       'restatement (tests/self_vad_numpy.py) decodes, on the three recordings of tests/test_mfcc_batch.py '
                       'with pipeline.SELF_VAD; written by tests/test_self_vad.py, not asserted',
                  files=[dict(seconds=s, seed=seed, tokens_device=len(a), tokens_restatement=len(b), borders_differing=d)
                         for (s, seed), a, b, d in zip(TALKS, tokens, t['tokens'], differ)],
                  passes_run=dict(device=n, restatement=t['passes']))
    try:
        with open(os.path.join(ROOT, 'profiles', 'self_vad_accuracy.json'), 'w') as f:
            f.write(json.dumps(record, indent=1, sort_keys=True) + '\n')
    except OSError:
        pass                                        # (a read-only checkout: the figures are printed above)


@pytest.mark.gpu
def test_a_files_tokens_depend_neither_on_the_batch_nor_on_the_run(ctx, decoded):
    cfg, pcms, tokens, last, _, _ = decoded
    again, last2 = _decode(ctx, cfg, pcms)
    assert again == tokens and last2 == last
    for i, p in enumerate(pcms):
        alone, n = _decode(ctx, cfg, [p])
        assert alone == [tokens[i]] and n == [last[i]], i


@pytest.mark.gpu
def test_a_short_file_comes_back_untrained_and_leaves_its_neighbours_alone(ctx, decoded):
    cfg, pcms, tokens, last, _, _ = decoded
    short = S.talk(5.0, 77)[0]
    silent = np.zeros(30 * 16000, dtype=np.int16)   # constant audio: the thresholds meet, nothing to seed
    detail = {}
    got, n = _decode(ctx, cfg, [pcms[0], short, np.zeros(0, dtype=np.int16), pcms[1], silent], detail)
    assert got[1] == [] and got[2] == [] and got[4] == [] and detail['vad_untrained'] == [1, 2, 4]
    assert got[0] == tokens[0] and got[3] == tokens[1] and n == [last[0], 625, 0, last[1], 3750]
    pipeline = pkg('pipeline')
    vad = pipeline.vad_batch(ctx, pipeline.SELF_VAD, [short, pcms[2]], cfg=cfg)
    assert vad[0] == [] and len(vad[1]) >= 2        # no turn is guessed for the file without a model
    detail = {}
    got, n = _decode(ctx, cfg, [short], detail)
    assert got == [[]] and detail == dict(vad_untrained=[0], vad_passes_run=0)


@pytest.mark.gpu
def test_samples_to_speakers_without_a_model(ctx, decoded):
    cfg, pcms, tokens, last, _, _ = decoded
    pipeline, vd = pkg('pipeline'), pkg('voice_detection')
    timings, detail = {}, {}
    vad = pipeline.vad_batch(ctx, pipeline.SELF_VAD, pcms, cfg=cfg, timings=timings, detail=detail)
    assert detail['vad_untrained'] == [] and len(timings['mfcc_static']) == 1
    # the turns are voice-detection2.py's state machine over the decoded tokens
    for toks, n, turns in zip(tokens, last, vad):
        want = vd.turns_from_tokens(((str(t), w) for t, w in toks), 'a', vd.VadOptions(), lambda: str(n))
        want = pkg('hipabi').py2_roundtrip(np.array([(s, e) for _, s, e in want], dtype=np.float64).ravel()).reshape(-1, 2)
        assert np.array_equal(want, np.array(turns))
        assert len(turns) == len(S.speech_runs(toks, n)) >= 7
    timings, detail = {}, {}
    rows = pipeline.diarize_pcm_batch(ctx, pipeline.SELF_VAD, cfg, pcms, timings=timings, detail=detail)
    # one upload, ONE feature chain, the self-trained turns on its features
    assert len(timings['wall_upload']) == 1 and len(timings['mfcc_static']) == len(timings['mfcc_post']) == 1
    assert detail['vad_untrained'] == [] and detail['vad_passes_run'] >= 1
    d_frames, total, frame_off = pipeline.features_batch(ctx, cfg, pcms)
    assert pipeline.vad_batch(ctx, pipeline.SELF_VAD, None, cfg=cfg, uploaded=pkg('frontend').upload_batch(ctx, pcms),
                              features=(d_frames, total, frame_off)) == vad
    files = [pipeline.BatchFile(frame_off[f], frame_off[f + 1] - frame_off[f], vad[f]) for f in range(3)]
    want = pipeline.diarize_batch(ctx, d_frames, total, files, rate=float(cfg.frame_rate))
    assert len(rows) == len(want) == 3
    for got, ref, turns in zip(rows, want, vad):
        assert got.shape == ref.shape and np.all(got == ref) and len(got) >= len(turns)
        # the rows' turns are vad_batch's: every turn opens a row and closes one, and no row lies outside a turn
        near = lambda x, col: bool(np.any(np.abs(got[:, col] - x) < 1e-9))
        assert all(near(s, 0) and near(e, 1) for s, e in turns)
        assert all(any(s - 1e-9 <= a and b <= e + 1e-9 for s, e in turns) for a, b, _ in got)


@pytest.mark.gpu
def test_generate_exp_self_trained_writes_what_voice_detection_reads(ctx, decoded, tmp_path):
    cfg, pcms, tokens, last, _, _ = decoded
    eg, vd, pipeline = pkg('exp_generator'), pkg('voice_detection'), pkg('pipeline')
    wav, exp, lna = str(tmp_path / 'talk.wav'), str(tmp_path / 'exp'), str(tmp_path / 'lna')
    fcfg, recipe, out_recipe = str(tmp_path / 'fconfig.cfg'), str(tmp_path / 'in.recipe'), str(tmp_path / 'vad.recipe')
    os.mkdir(exp)
    _write_wav(wav, pcms[1])
    with open(fcfg, 'w') as f:
        f.write(_cfg_text(GOLD))
    with open(recipe, 'w') as f:
        f.write('audio=%s\n' % wav)
    said = []
    assert eg.main([recipe, '-e', exp, '-l', lna, '--self-trained', fcfg], say=lambda *a: said.append(' '.join(a))) == 0
    assert said[1] == 'Self-trained detector on the features of: ' + fcfg
    assert sorted(os.listdir(exp)) == ['talk.exp', 'talk.last_frame'] and not os.path.exists(lna)     # -l: accepted, unused
    assert open(os.path.join(exp, 'talk.last_frame')).read() == str(last[1])
    assert open(os.path.join(exp, 'talk.exp')).read() == ' '.join('%d %s' % tw for tw in tokens[1])
    vd.main([recipe, exp, '-o', out_recipe], stdout=io.StringIO())
    lines = open(out_recipe).read().splitlines()
    turns = [(float(re.search(r'start-time=(\S+)', l).group(1)), float(re.search(r'end-time=(\S+)', l).group(1))) for l in lines]
    assert turns == pipeline.vad_batch(ctx, pipeline.SELF_VAD, [pcms[1]], cfg=cfg)[0] and len(turns) >= 7
