"""Sample-rate conversion and downmix of a batch on the device (spkd_resample_batch,
frontend.resample_taps / output_offsets / read_audio / resample_batch, pipeline.diarize_audio_batch,
./to16k.py) against the numpy restatement of tests/resample_numpy.py.

The restatement and the kernel both accumulate in float64 with the taps ascending, so the int16
output is compared to the bit wherever the value before rounding lies farther than 1e-6 from a
half-integer (50 times the 2e-8 that two float64 evaluations can differ by, include/spkd.h); on the
other samples a difference of 1 is allowed, and they may be at most 1 in 10 000 of a batch.  The
identity conversion has no such exemption.  Everything else here is exact: a file of a batch
against the file alone, one order of the files against another, one grouping against another,
diarize_audio_batch against diarize_pcm_batch on the converted samples.

Border batches: the tile is T = RESAMPLE_TILE output samples, so the file lengths put n_out on
{0, 1, 2, T - 1, T, T + 1, 2 T + 3}.  A conversion that raises the rate cannot give every count
(8 kHz -> 16 kHz gives even ones only): there the file is the shortest whose n_out reaches the
target, which still puts a file's end on, just before or just behind a tile border, and the test
says which targets are met exactly."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys
import types
import wave

import numpy as np
import pytest

import resample_numpy as R
from conftest import pkg
from helpers import ROOT
from test_generate_exp import _synthetic_mixtures, load_model, write_model
from test_mfcc_batch import _cfg, _talk

RATE_OUT = 16000
TABLE_RATES = (48000, 44100, 32000, 22050, 11025, 8000, 96000, 16000)
BORDER_RATES = (48000, 44100, 8000, 11025, 16000)       # 11 025 Hz: a table above 64 KiB; 16 000 Hz: the identity
GUARD = 64                                              # int16 behind the output, which the call must not touch
GUARD_PATTERN = 0x5a3c


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _noise(rng, n, channels, loud):
    """Full-scale noise or noise in [-3, 3] (the level is what a leak across a file border carries)."""
    return (rng.integers(-32768, 32768, (n, channels)) if loud else rng.integers(-3, 4, (n, channels))).astype(np.int16)


def _shortest(target, rate):
    """The shortest file, in frames, whose n_out reaches `target`."""
    L, M, _ = R.ratio(rate, RATE_OUT)
    n = (target * M) // L
    while R.n_out(n, rate, RATE_OUT) < target:
        n += 1
    while n > 0 and R.n_out(n - 1, rate, RATE_OUT) >= target:
        n -= 1
    return n


def _border_lengths(rate):
    T = pkg('hipabi').RESAMPLE_TILE
    h = R.ratio(rate, RATE_OUT)[2]
    targets = [1, 2, T - 1, T, T + 1, 2 * T + 3]
    by_n_out = [_shortest(t, rate) for t in targets]
    by_half = [max(h - 1, 0), h, 2 * h + 1]
    # empty files first, in the middle and last
    return [0] + by_n_out[:3] + [0] + by_n_out[3:] + by_half + [0], targets


@functools.lru_cache(maxsize=None)
def _border_batch(rate):
    """The border batch of one conversion and its restatement, computed once: (audios, want, pre)."""
    rng = np.random.default_rng(20261019 + rate)
    lengths, _ = _border_lengths(rate)
    audios = [(_noise(rng, n, 1 + i % 3, i % 2 == 1), rate) for i, n in enumerate(lengths)]
    results = [R.convert(a, rate, RATE_OUT) for a, _ in audios]
    return audios, [y for y, _ in results], [p for _, p in results]


MIXED_RATES = (48000, 44100, 8000, 11025, 16000)


@functools.lru_cache(maxsize=None)
def _mixed_batch():
    """All five conversions and the three channel counts in one batch, loud beside quiet."""
    rng = np.random.default_rng(77)
    audios = []
    for i in range(11):
        rate = MIXED_RATES[i % 5]
        n = 0 if i == 6 else int(rng.integers(1500, 3000) * rate / 16000 * (3 if i % 4 == 0 else 1))
        audios.append((_noise(rng, n, 1 + i % 3, i % 2 == 0), rate))
    return audios


# ------------------------------------------------------------------ not GPU
def test_entry_point_and_timer_are_declared_and_exported():
    hipabi = pkg('hipabi')
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'spkd.h')).read(), flags=re.S)
    lib = hipabi.load_library()
    assert re.search(r'\bspkd_resample_batch\s*\(', code) and re.search(r'\}\s*spkd_resample_conv\s*;', code)
    assert 'spkd_resample_batch' in hipabi.EXPORTS and hasattr(lib, 'spkd_resample_batch')
    assert hasattr(hipabi.Context, 'resample_batch') and C.sizeof(hipabi.ResampleConv) == 24
    names = [n for n, _ in sorted(hipabi.TIMERS.items(), key=lambda kv: kv[1])]
    enum = re.search(r'enum \{\s*SPKD_T_CALL = 0,(.*?)SPKD_N_TIMERS', code, flags=re.S).group(1)
    assert ['call'] + [n.strip()[len('SPKD_T_'):].lower() for n in enum.split(',') if n.strip()] == names
    assert 'resample' in names and names[-2:] == ['mfcc_static', 'mfcc_post']
    for name in ('TILE', 'MAX_CH', 'MAX_HALF', 'MAX_TERM', 'MAX_TAPS', 'MAX_SPAN'):
        header = int(re.search(r'#define SPKD_RESAMPLE_%s (\d+)' % name, code).group(1))
        assert getattr(hipabi, 'RESAMPLE_' + name) == header, name
    assert hipabi.RESAMPLE_MAX_CH == 8 and hipabi.RESAMPLE_MAX_TAPS == 1 << 22
    # the widest span is the one of the widest designed filter: ceil(TILE down / up) + 2 half, half = 16 down / up
    assert hipabi.RESAMPLE_MAX_SPAN == hipabi.RESAMPLE_TILE * hipabi.RESAMPLE_MAX_HALF // 16 + 2 * hipabi.RESAMPLE_MAX_HALF + 1


def _refusals():
    """(name, a word of its error text, call(lib, ctx handle) -> status) of every refusal of spkd_resample_batch."""
    hipabi = pkg('hipabi')
    Conv = hipabi.ResampleConv
    good_off = np.array([0, 600, 1000], dtype=np.int64)
    good_convs = [Conv(1, 3, 48, 0), Conv(1, 1, 0, 0)]
    taps = np.zeros(96, dtype=np.float32)
    dev = C.c_void_p(256)                         # never dereferenced: the refusal comes first
    keep = []

    def call(off=good_off, n=2, channels=(2, 1), conv=(0, 1), convs=good_convs, n_conv=None, tables=True, d_in=dev,
             d_out=dev, out_off=True):
        ch = None if channels is None else np.array(channels, dtype=np.int32)
        cv = None if conv is None else np.array(conv, dtype=np.int32)
        table = None if convs is None else (Conv * max(len(convs), 1))(*convs)
        out = np.zeros(len(good_off), dtype=np.int64)
        keep.extend([ch, cv, table, out])
        nc = (0 if convs is None else len(convs)) if n_conv is None else n_conv
        return lambda lib, h: lib.spkd_resample_batch(
            h, d_in, n, None if off is None else _ptr(off), None if ch is None else _ptr(ch),
            None if cv is None else _ptr(cv), nc, table, _ptr(taps) if tables else None, d_out,
            _ptr(out) if out_off else None)

    i64 = lambda *v: np.array(v, dtype=np.int64)
    return [('negative file count', 'negative', call(n=-1)),
            ('negative conversion count', 'negative', call(n_conv=-1)),
            ('null in_off', 'null host', call(off=None)),
            ('null channels', 'null host', call(channels=None)),
            ('null conv', 'null host', call(conv=None)),
            ('null convs', 'null host', call(convs=None, n_conv=2)),
            ('null out_off', 'null host', call(out_off=False)),
            ('in_off not from 0', 'start at 0', call(off=i64(2, 600, 1000))),
            ('decreasing in_off', 'non-decreasing', call(off=i64(0, 600, 400))),
            ('span no multiple of the channels', 'multiple', call(off=i64(0, 601, 1000))),
            ('no channel', 'channel count', call(channels=(0, 1))),
            ('nine channels', 'channel count', call(off=i64(0, 900, 1000), channels=(9, 1))),
            ('conversion index -1', 'index', call(conv=(-1, 1))),
            ('conversion index behind the last', 'index', call(conv=(0, 2))),
            ('up 0', 'up and down', call(convs=[Conv(0, 3, 48, 0), Conv(1, 1, 0, 0)])),
            ('down 0', 'up and down', call(convs=[Conv(1, 0, 48, 0), Conv(1, 1, 0, 0)])),
            ('up and down share a factor', 'coprime', call(convs=[Conv(2, 6, 48, 0), Conv(1, 1, 0, 0)])),
            ('negative half_taps', 'half_taps outside', call(convs=[Conv(1, 3, -1, 0), Conv(1, 1, 0, 0)])),
            ('half_taps above the limit', 'half_taps outside',
             call(convs=[Conv(1, 3, hipabi.RESAMPLE_MAX_HALF + 1, 0), Conv(1, 1, 0, 0)])),
            ('a filter without taps', 'identity', call(convs=[Conv(1, 3, 0, 0), Conv(1, 1, 0, 0)])),
            ('an identity with taps', 'identity', call(convs=[Conv(1, 3, 48, 0), Conv(1, 1, 4, 0)])),
            ('negative taps_off', 'taps_off', call(convs=[Conv(1, 3, 48, -1), Conv(1, 1, 0, 0)])),
            ('a span beyond the LDS', 'span', call(convs=[Conv(1, 1000, 16, 0), Conv(1, 1, 0, 0)])),
            ('null tables with a filtered conversion', 'null tables', call(tables=False)),
            ('null input with a sample', 'null device', call(d_in=None)),
            ('null output with a sample', 'null device', call(d_out=None))]


def test_argument_refusals_come_before_any_device_work():
    """No context, no device: every refusal is SPKD_EINVAL.  A null context is itself refused first,
    so this shows only that no case touches a device on its way out; the GPU test below, with a
    context, is the one that tells the refusals apart."""
    hipabi = pkg('hipabi')
    lib = hipabi.load_library()
    for name, _, call in _refusals():
        assert call(lib, None) == hipabi.SPKD_EINVAL, name


@pytest.mark.parametrize('rate', TABLE_RATES)
def test_the_table_equals_the_restatement_bit_for_bit(rate):
    fe = pkg('frontend')
    table, (L, M, half) = fe.resample_taps(rate, RATE_OUT)
    want = R.taps(rate, RATE_OUT)
    assert (L, M, half) == R.ratio(rate, RATE_OUT) and L * rate == M * RATE_OUT
    assert table.dtype == np.float32 and table.shape == want.shape == (L, 2 * half)
    assert np.array_equal(table.view(np.uint32), want.view(np.uint32))
    if rate == RATE_OUT:
        assert (L, M, half) == (1, 1, 0) and table.size == 0                    # the identity conversion
    else:
        assert np.abs(table.astype(np.float64).sum(axis=1) - 1.0).max() < 1e-6  # DC gain 1 at every phase


def test_the_table_sizes_are_the_ones_the_kernel_is_laid_out_for():
    fe, hipabi = pkg('frontend'), pkg('hipabi')
    shapes = {rate: fe.resample_taps(rate, RATE_OUT)[0].shape for rate in TABLE_RATES}
    assert shapes[48000] == (1, 96) and shapes[44100] == (160, 90) and shapes[8000] == (2, 32)
    assert shapes[22050] == (320, 46) and shapes[11025] == (640, 32) and 640 * 32 * 4 > 64 * 1024
    with pytest.raises(ValueError, match='1000003 Hz -> 16000 Hz'):           # 16 000 phases x 2 002 taps
        fe.resample_taps(1000003, RATE_OUT)
    with pytest.raises(ValueError, match='positive'):
        fe.resample_taps(0, RATE_OUT)
    assert fe.resample_taps(44101, RATE_OUT)[0].size <= hipabi.RESAMPLE_MAX_TAPS      # odd rates do fit


def test_output_offsets_state_the_layout_on_the_host():
    fe = pkg('frontend')
    got = fe.output_offsets([441, 442, 0, 1], [44100] * 4, RATE_OUT)
    assert got.dtype == np.int64 and list(np.diff(got)) == [160, 161, 0, 1] and got[0] == 0
    assert list(fe.output_offsets([3, 4, 5, 7], [48000, 48000, 8000, 16000], RATE_OUT)) == [0, 1, 3, 13, 20]
    assert list(fe.output_offsets([], [], RATE_OUT)) == [0]
    rng = np.random.default_rng(3)
    for rate in TABLE_RATES:
        for n in [0, 1, 2] + [int(v) for v in rng.integers(3, 100000, 5)]:
            L, M, _ = R.ratio(rate, RATE_OUT)
            n_out = int(fe.output_offsets([n], [rate], RATE_OUT)[1])
            assert n_out == R.n_out(n, rate, RATE_OUT)
            # every output instant n M / L inside [0, n_in), and no other
            assert (n_out == 0) == (n == 0) and (n_out == 0 or (n_out - 1) * M < n * L <= n_out * M)


def _tone(rate, freq, amplitude=20000.0):
    return np.rint(amplitude * np.sin(2 * np.pi * freq * np.arange(rate) / rate)).astype(np.int16)


@pytest.mark.parametrize('rate', TABLE_RATES)
def test_the_filter_passes_the_band_and_rejects_what_would_alias(rate):
    """Design checks of the restatement on 1 s tones of amplitude 20 000, the first and last 400
    outputs left out.  Measured: pass-band gain at worst -0.002 dB (3 kHz from 8 kHz), a 1 kHz tone at
    most 1.0 from the analytic one after rounding, the stop band at worst -88.5 dB (8.8 kHz from 22.05 kHz)."""
    A, edge = 20000.0, 400
    n = np.arange(RATE_OUT)[edge:-edge]
    for freq in (1000.0, 3000.0):
        y, pre = R.convert(_tone(rate, freq), rate, RATE_OUT)
        assert len(y) == RATE_OUT
        basis = np.stack([np.sin(2 * np.pi * freq * n / RATE_OUT), np.cos(2 * np.pi * freq * n / RATE_OUT)], axis=1)
        gain = 20 * np.log10(np.hypot(*np.linalg.lstsq(basis, pre[edge:-edge], rcond=None)[0]) / A)
        print('%d Hz, tone %d Hz: gain %.5f dB' % (rate, freq, gain))
        assert abs(gain) < 0.01, (rate, freq, gain)
        if freq == 1000.0:
            worst = np.abs(y[edge:-edge] - A * np.sin(2 * np.pi * freq * n / RATE_OUT)).max()
            print('%d Hz, tone %d Hz: at most %.3f from the analytic tone' % (rate, freq, worst))
            assert worst <= 2.0, (rate, worst)
    # tones the input can hold and the output cannot: they would alias into the band
    for freq in (8800.0, 9500.0, 12000.0, 0.95 * rate / 2):
        if not 8800.0 <= freq < rate / 2:
            continue
        _, pre = R.convert(_tone(rate, freq), rate, RATE_OUT)
        level = 20 * np.log10(np.sqrt(np.mean(pre[edge:-edge] ** 2)) / (A / np.sqrt(2)))
        print('%d Hz, tone %.1f Hz: %.1f dB' % (rate, freq, level))
        assert level <= -80.0, (rate, freq, level)


@pytest.mark.parametrize('rate', BORDER_RATES)
def test_the_border_batches_are_what_they_claim(rate):
    """The lengths hit the tile borders, offsets of both parities occur, near-ties are rare in the
    restatement, and the 8 kHz batch saturates."""
    T = pkg('hipabi').RESAMPLE_TILE
    lengths, targets = _border_lengths(rate)
    audios, want, pre = _border_batch(rate)
    n_outs = [len(y) for y in want]
    L, M, h = R.ratio(rate, RATE_OUT)
    assert lengths[0] == lengths[4] == lengths[-1] == 0 and [len(a) for a, _ in audios] == lengths
    hit = [t for t in targets if t in n_outs]
    print('%d Hz: n_in %s -> n_out %s; targets met exactly: %s' % (rate, lengths, n_outs, hit))
    if L <= M:
        assert hit == targets                                       # every count can be met unless the rate rises
    for t in targets:                                               # each target met, or passed by less than L / M
        assert any(t <= n < t + -(-L // M) for n in n_outs), t
    assert {max(h - 1, 0), h, 2 * h + 1} <= set(lengths)
    assert sorted(set(a.shape[1] for a, _ in audios)) == [1, 2, 3]
    # element offsets as _convert lays the batch out behind one int16 of padding: odd ones occur on both sides, and
    # two-channel files lie on both parities (only the even ones can be read four bytes at a time)
    in_at = 1 + np.concatenate([[0], np.cumsum([a.size for a, _ in audios])])[:-1]
    out_at = 1 + np.concatenate([[0], np.cumsum(n_outs)])[:-1]
    used = [f for f, (a, _) in enumerate(audios) if a.size]
    assert (in_at[used] % 2 == 1).any() and (out_at[used] % 2 == 1).any()
    assert len(set(int(in_at[f]) % 2 for f in used if audios[f][0].shape[1] == 2)) == 2 or rate == RATE_OUT
    total = sum(n_outs)
    ties = sum(int(R.near_tie(p).sum()) for p in pre)
    # (the identity conversion is exact ties all over -- a mean of two integers -- and has no exemption)
    assert total > 4 * T and (ties <= total / 10000 or rate == RATE_OUT)
    if rate == 8000:
        beyond = sum(int((np.abs(p) > 32768).sum()) for p in pre)
        print('8 kHz: %d of %d samples saturate' % (beyond, total))
        assert beyond > 0 and any((y == 32767).any() for y in want) and any((y == -32768).any() for y in want)


def test_full_scale_noise_has_no_near_tie_in_the_restatement():
    rng = np.random.default_rng(5)
    for rate, channels in ((48000, 2), (44100, 2), (44100, 3), (8000, 1)):
        L, M, _ = R.ratio(rate, RATE_OUT)
        _, pre = R.convert(_noise(rng, -(-32000 * M // L), channels, True), rate, RATE_OUT)
        assert len(pre) >= 32000 and not R.near_tie(pre).any(), (rate, channels)


def test_host_entry_points_refuse_before_touching_the_context(tmp_path):
    fe, pipeline = pkg('frontend'), pkg('pipeline')
    cfg = _cfg(400)
    ok = np.zeros((100, 2), dtype=np.int16)
    with pytest.raises(ValueError, match='int16 samples'):
        fe.resample_batch(None, [(ok, 48000), (np.zeros((2, 5, 2), dtype=np.int16), 48000)], RATE_OUT)
    with pytest.raises(ValueError, match='int16'):
        fe.resample_batch(None, [(np.zeros(10, dtype=np.float32), 48000)], RATE_OUT)
    with pytest.raises(ValueError, match='int16 range'):
        fe.resample_batch(None, [(np.array([[0, 40000]], dtype=np.int32), 48000)], RATE_OUT)
    with pytest.raises(ValueError, match='channels'):
        fe.resample_batch(None, [(np.zeros((10, 9), dtype=np.int16), 48000)], RATE_OUT)
    with pytest.raises(ValueError, match='sample rate'):
        fe.resample_batch(None, [(ok, 0)], RATE_OUT)
    with pytest.raises(ValueError, match='sample rate'):
        fe.resample_batch(None, [(ok, 44100.0)], RATE_OUT)
    with pytest.raises(ValueError, match='pair'):
        fe.resample_batch(None, [ok], RATE_OUT)
    with pytest.raises(ValueError, match='1000003 Hz -> 16000 Hz'):
        fe.resample_batch(None, [(ok, 1000003)], RATE_OUT)
    model = lambda rate, hop: types.SimpleNamespace(cfg=types.SimpleNamespace(sample_rate=rate, hop=hop))
    with pytest.raises(ValueError, match='Hz'):
        pipeline.diarize_audio_batch(None, model(8000, cfg.hop), cfg, [(ok, 48000)])
    with pytest.raises(ValueError, match='frame'):
        pipeline.diarize_audio_batch(None, model(cfg.sample_rate, 160), cfg, [(ok, 48000)])
    with pytest.raises(ValueError, match='int16 samples'):
        pipeline.diarize_audio_batch(None, model(cfg.sample_rate, cfg.hop), cfg, [(np.zeros(10), 48000)])
    # read_audio: every channel of a 16-bit file; other widths are refused; read_wav keeps refusing stereo
    stereo = np.arange(-300, 300, dtype=np.int16).reshape(-1, 2)
    _write_wav(str(tmp_path / 's.wav'), stereo, 44100)
    got, rate = fe.read_audio(str(tmp_path / 's.wav'))
    assert rate == 44100 and got.dtype == np.int16 and np.array_equal(got, stereo)
    with pytest.raises(ValueError, match='mono'):
        fe.read_wav(str(tmp_path / 's.wav'))
    with wave.open(str(tmp_path / 'b.wav'), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(1)
        w.setframerate(8000)
        w.writeframes(bytes(100))
    with pytest.raises(ValueError, match='16-bit'):
        fe.read_audio(str(tmp_path / 'b.wav'))


def _write_wav(path, samples, rate):
    with wave.open(path, 'wb') as w:
        w.setnchannels(samples.shape[1] if samples.ndim == 2 else 1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(samples, dtype='<i2').tobytes())


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def ctx():
    c = pkg('hipabi').Context(0)
    yield c
    c.close()


def _convert(ctx, audios, lead=1):
    """spkd_resample_batch on buffers of the test's own: the raw audio behind `lead` int16 of padding
    (an odd count puts the first file on an odd element), the output at an odd element too, with
    GUARD int16 of a fixed pattern behind it that must stay -> (one int16 array per file, out_off)."""
    fe, hipabi = pkg('frontend'), pkg('hipabi')
    rates = sorted(set(rate for _, rate in audios))
    convs, tables, at = [], [], 0
    for rate in rates:
        table, (L, M, half) = fe.resample_taps(rate, RATE_OUT)
        convs.append(hipabi.ResampleConv(L, M, half, at))
        tables.append(table.ravel())
        at += table.size
    taps = np.concatenate(tables)
    raw = np.concatenate([np.zeros(lead, dtype=np.int16)] + [np.asarray(a, dtype=np.int16).ravel() for a, _ in audios])
    in_off = np.concatenate([[0], np.cumsum([np.asarray(a).size for a, _ in audios])]).astype(np.int64)
    channels = [a.shape[1] if a.ndim == 2 else 1 for a, _ in audios]
    want_off = fe.output_offsets([len(a) for a, _ in audios], [rate for _, rate in audios], RATE_OUT)
    total = int(want_off[-1])
    d_raw = ctx.dev_scratch('test_resample_raw', max(raw.nbytes, 16))
    ctx.h2d(d_raw, raw)
    buf = np.full(1 + total + GUARD, GUARD_PATTERN, dtype=np.int16)
    d_out = ctx.dev_scratch('test_resample_out', buf.nbytes)
    ctx.h2d(d_out, buf)
    out_off = ctx.resample_batch(d_raw + 2 * lead, in_off, channels, [rates.index(rate) for _, rate in audios], convs, taps,
                                 d_out + 2)
    assert out_off.dtype == np.int64 and np.array_equal(out_off, want_off)
    ctx.d2h(buf, d_out)
    assert buf[0] == GUARD_PATTERN and np.all(buf[1 + total:] == GUARD_PATTERN)      # nothing written around the output
    return [buf[1 + out_off[f]:1 + out_off[f + 1]].copy() for f in range(len(audios))], out_off


def _against_the_restatement(got, want, pre, exact):
    """The comparison rule of this module's docstring; returns the number of exempt samples that differ."""
    total = exempt = differing = 0
    for f, (g, w, p) in enumerate(zip(got, want, pre)):
        assert g.shape == w.shape, f
        tie = np.zeros(len(p), dtype=bool) if exact else R.near_tie(p)
        diff = g.astype(np.int32) - w.astype(np.int32)
        bad = (diff != 0) & ~tie
        assert not bad.any(), 'file %d (%d samples): first differing sample %d, %d for %d (%.9f before rounding)' % (
            f, len(g), int(np.argmax(bad)), g[np.argmax(bad)], w[np.argmax(bad)], p[np.argmax(bad)])
        assert np.abs(diff).max(initial=0) <= 1, f
        total, exempt, differing = total + len(g), exempt + int(tie.sum()), differing + int((diff != 0).sum())
    assert exempt <= total / 10000
    return differing


@pytest.mark.gpu
@pytest.mark.parametrize('rate', BORDER_RATES)
def test_a_border_batch_equals_the_restatement(ctx, rate):
    audios, want, pre = _border_batch(rate)
    for lead in (1, 2):                       # every file on an element of one parity, then of the other
        got, out_off = _convert(ctx, audios, lead=lead)
        differing = _against_the_restatement(got, want, pre, exact=rate == RATE_OUT)
        print('%d Hz, lead %d: %d samples, %d near-tie samples differ' % (rate, lead, int(out_off[-1]), differing))
    if rate == 8000:
        assert any((g == 32767).any() for g in got) and any((g == -32768).any() for g in got)
    assert ctx.last_ms('resample') > 0


@pytest.fixture(scope='module')
def alone(ctx):
    """Every file of the mixed batch converted on its own."""
    return [_convert(ctx, [audio])[0][0] for audio in _mixed_batch()]


@pytest.mark.gpu
def test_every_file_of_a_mixed_batch_equals_the_file_alone_to_the_bit(ctx, alone):
    audios = _mixed_batch()
    assert sorted(set(rate for _, rate in audios)) == sorted(MIXED_RATES)
    assert sorted(set(a.shape[1] for a, _ in audios)) == [1, 2, 3]
    got, out_off = _convert(ctx, audios)
    for f, (g, w) in enumerate(zip(got, alone)):
        assert np.array_equal(g, w), f
    # and the files alone are the restatement's
    results = [R.convert(a, rate, RATE_OUT) for a, rate in audios]
    filtered = [f for f, (_, rate) in enumerate(audios) if rate != RATE_OUT]
    identity = [f for f, (_, rate) in enumerate(audios) if rate == RATE_OUT]
    for files, exact in ((filtered, False), (identity, True)):        # (a mean of two integers is a tie half the time)
        _against_the_restatement([alone[f] for f in files], [results[f][0] for f in files], [results[f][1] for f in files],
                                 exact=exact)
    assert max(np.abs(a).max(initial=0) for a in alone[1::2]) <= 8 < 1000 < max(np.abs(a).max(initial=0) for a in alone[0::2])


@pytest.mark.gpu
def test_the_order_of_the_files_does_not_matter(ctx, alone):
    audios = _mixed_batch()
    order = list(np.random.default_rng(4).permutation(len(audios)))
    assert order != sorted(order)
    got, _ = _convert(ctx, [audios[i] for i in order])
    for slot, i in enumerate(order):
        assert np.array_equal(got[slot], alone[i]), (slot, i)


def _download(ctx, uploaded):
    d_pcm, sample_off = uploaded
    pcm = np.zeros(int(sample_off[-1]), dtype=np.int16)
    if pcm.size:
        ctx.d2h(pcm, d_pcm)
    return [pcm[sample_off[f]:sample_off[f + 1]].copy() for f in range(len(sample_off) - 1)]


@pytest.mark.gpu
def test_groups_of_files_give_the_bits_and_offsets_of_one_group(ctx, alone):
    fe = pkg('frontend')
    audios = _mixed_batch()
    timings = {}
    one = fe.resample_batch(ctx, audios, RATE_OUT, timings=timings)
    want = _download(ctx, one)
    assert len(timings['wall_upload']) == len(timings['resample']) == 1 and timings['resample'][0] > 0
    for f, (g, w) in enumerate(zip(want, alone)):
        assert np.array_equal(g, w), f
    calls = []
    inner = ctx.resample_batch
    ctx.resample_batch = lambda *a: calls.append(len(a[2])) or inner(*a)
    try:
        group_bytes = sum(a.nbytes for a, _ in audios) // 4
        several = fe.resample_batch(ctx, audios, RATE_OUT, group_bytes=group_bytes)
    finally:
        del ctx.resample_batch
    assert len(calls) >= 3 and sum(calls) == len(audios), calls
    assert several[0] == one[0] and np.array_equal(several[1], one[1])
    for f, (g, w) in enumerate(zip(_download(ctx, several), want)):
        assert np.array_equal(g, w), f
    # mono files given as [n] are the files given as [n, 1]
    mono = [(a[:, 0].copy(), rate) for a, rate in audios if a.shape[1] == 1]
    flat = _download(ctx, fe.resample_batch(ctx, mono, RATE_OUT))
    assert all(np.array_equal(g, alone[i]) for g, i in zip(flat, [i for i, (a, _) in enumerate(audios) if a.shape[1] == 1]))


@pytest.mark.gpu
def test_refusals_on_a_context_name_their_reason_and_leave_it_usable(ctx, alone):
    hipabi = pkg('hipabi')
    for name, word, call in _refusals():
        assert call(ctx.lib, ctx.h) == hipabi.SPKD_EINVAL, name
        assert word in ctx.lib.spkd_last_error(ctx.h).decode(), (name, ctx.lib.spkd_last_error(ctx.h).decode())
    with pytest.raises(hipabi.SpkdError, match='non-decreasing'):
        ctx.resample_batch(256, [0, 400, 300], [1, 1], [0, 0], [(1, 1, 0, 0)], [], 256)
    audios = _mixed_batch()
    got, _ = _convert(ctx, audios)
    assert all(np.array_equal(g, w) for g, w in zip(got, alone))


@pytest.mark.gpu
def test_a_batch_without_a_sample_launches_nothing(ctx):
    fe = pkg('frontend')
    table, (L, M, half) = fe.resample_taps(48000, RATE_OUT)
    convs = [(L, M, half, 0), (1, 1, 0, 0)]
    # null device pointers: a launch would have been refused (and a kernel would have faulted)
    for n in (0, 1, 3):
        out_off = ctx.resample_batch(0, [0] * (n + 1), [2, 1, 3][:n], [0, 1, 0][:n], convs, table, 0)
        assert out_off.dtype == np.int64 and list(out_off) == [0] * (n + 1)
    assert list(ctx.resample_batch(0, [0], [], [], [], [], 0)) == [0]
    d_pcm, sample_off = fe.resample_batch(ctx, [], RATE_OUT)
    assert list(sample_off) == [0]
    d_pcm, sample_off = fe.resample_batch(ctx, [(np.zeros((0, 2), dtype=np.int16), 44100), (np.zeros(0, dtype=np.int16), 16000)],
                                          RATE_OUT)
    assert list(sample_off) == [0, 0, 0]


@pytest.fixture(scope='module')
def model(tmp_path_factory):
    d = str(tmp_path_factory.mktemp('vad_model'))
    write_model(d, *_synthetic_mixtures(np.random.default_rng(11)))
    return load_model(d)


@pytest.mark.gpu
def test_recordings_to_speakers_equals_samples_to_speakers_on_the_converted_audio(ctx, model):
    fe, pipeline = pkg('frontend'), pkg('pipeline')
    cfg = _cfg(400)
    left = _talk(23.0, 114, rate=48000)
    audios = [(np.stack([left, left], axis=1), 48000), (_talk(27.0, 146, rate=44100), 44100)]
    timings = {}
    rows = pipeline.diarize_audio_batch(ctx, model, cfg, audios, timings=timings)
    assert len(timings['resample']) == len(timings['wall_upload']) == 1
    assert len(timings['mfcc_static']) == len(timings['mfcc_post']) == 2
    pcms = _download(ctx, fe.resample_batch(ctx, audios, cfg.sample_rate))
    assert [len(p) for p in pcms] == [23 * 16000, 27 * 16000]
    want = pipeline.diarize_pcm_batch(ctx, model, cfg, pcms)
    print('segments per file:', [len(r) for r in want], 'speakers per file:', [len(set(r[:, 2])) if len(r) else 0 for r in want])
    assert len(rows) == len(want) == 2 and all(len(r) >= 2 for r in want)       # the signal gives the stages work
    for got, ref in zip(rows, want):
        assert got.shape == ref.shape and np.all(got == ref)
    # 16 kHz mono goes through the identity conversion: the samples themselves
    mono = [_talk(23.0, 114), _talk(27.0, 146)]
    same = pipeline.diarize_audio_batch(ctx, model, cfg, [(p, 16000) for p in mono])
    for got, ref in zip(same, pipeline.diarize_pcm_batch(ctx, model, cfg, mono)):
        assert got.shape == ref.shape and len(ref) >= 2 and np.all(got == ref)


@pytest.mark.gpu
def test_to16k_writes_what_resample_batch_gives(ctx, tmp_path):
    fe = pkg('frontend')
    rng = np.random.default_rng(9)
    stereo = _noise(rng, 6001, 2, True)
    src, dst = str(tmp_path / 'in.wav'), str(tmp_path / 'out.wav')
    _write_wav(src, stereo, 44100)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'to16k.py'), src, '-o', dst], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with wave.open(dst, 'rb') as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, RATE_OUT)
        got = np.frombuffer(w.readframes(w.getnframes()), dtype='<i2')
    want = _download(ctx, fe.resample_batch(ctx, [fe.read_audio(src)], RATE_OUT))[0]
    assert len(got) == R.n_out(6001, 44100, RATE_OUT) and np.array_equal(got, want)
    assert np.array_equal(want, _convert(ctx, [(stereo, 44100)])[0][0])
