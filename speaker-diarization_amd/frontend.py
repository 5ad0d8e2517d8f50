"""feacat-shaped feature extraction on the MI355X: the step of
spk-diarization2.py:98-100, `feacat -c fconfig.cfg -H --raw-output x.wav > fea/x.fea`.
The reference's own configuration file is read (feaconfig.py); the arithmetic runs in
libspkd_hip.so (spkd_mfcc).  PARITY UNPINNED -- feacat itself is not available; every
choice the configuration file leaves open is listed in the test suite's numpy restatement
(mfcc_numpy.py in the checker directory) and in include/spkd.h.

`main` mirrors the one feacat command line the reference uses: -c CONFIG -H --raw-output WAV,
feature file (int32 dim + float32 frames, spk-change-detection.py:37-41) on stdout.
"""
import argparse
import math
import os
import sys
import time
import wave

import numpy as np

from . import hipabi
from .feaconfig import FeatureConfig

N_FFT, N_MEL = 512, 21


def mel_filterbank(sample_rate, n_fft=N_FFT, n_mel=N_MEL):
    """Triangular filters equally spaced on the mel scale 2595 log10(1 + f / 700), 0 .. Nyquist."""
    hz2mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)
    mel2hz = lambda m: 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    edges = mel2hz(np.linspace(hz2mel(0.0), hz2mel(sample_rate / 2.0), n_mel + 2))
    freqs = np.arange(n_fft // 2 + 1) * (sample_rate / float(n_fft))
    fb = np.zeros((n_mel, n_fft // 2 + 1))
    for m in range(n_mel):
        lo, mid, hi = edges[m], edges[m + 1], edges[m + 2]
        fb[m] = np.maximum(0.0, np.minimum((freqs - lo) / (mid - lo), (hi - freqs) / (hi - mid)))
    return fb.astype(np.float32)


def dct_matrix(n_cep, n_mel=N_MEL):
    k = np.arange(1, n_cep + 1)[:, None]
    m = np.arange(n_mel)[None, :]
    return (np.sqrt(2.0 / n_mel) * np.cos(np.pi * k * (m + 0.5) / n_mel)).astype(np.float32)


def read_wav(path):
    """16-bit mono PCM samples of a .wav file (what `ffmpeg -ar 16000 -ac 1` leaves,
    spk-diarization2.py:83-84) and its sample rate."""
    with wave.open(path, 'rb') as w:
        if w.getsampwidth() != 2 or w.getnchannels() != 1:
            raise ValueError('%s: 16-bit mono PCM expected' % path)
        return np.frombuffer(w.readframes(w.getnframes()), dtype='<i2'), w.getframerate()


def mfcc_params(cfg):
    """The spkd_mfcc_params of a feature configuration."""
    return hipabi.MfccParams(cfg.sample_rate, cfg.frame_rate, cfg.window_width, N_FFT, N_MEL, cfg.n_cep,
                             cfg.cms_left, cfg.cms_right, (hipabi.C.c_int32 * 2)(*cfg.delta_width),
                             cfg.pre_emph, (hipabi.C.c_float * 2)(*cfg.delta_norm))


def extract_device(pcm, cfg, ctx):
    """int16 samples -> (device pointer to float32 [T, 39] features, T).  The features stay on
    the device for a later stage; the caller frees the buffer (ctx.dev_free), which is None for
    T = 0."""
    pcm = np.ascontiguousarray(pcm, dtype=np.int16)
    T = len(pcm) // cfg.hop
    if T == 0:
        return None, 0
    d_pcm = ctx.dev_alloc(max(pcm.nbytes, 16))
    d_out = ctx.dev_alloc(T * cfg.dim * 4)
    try:
        ctx.h2d(d_pcm, pcm)
        n = ctx.mfcc(d_pcm, len(pcm), mfcc_params(cfg), mel_filterbank(cfg.sample_rate), dct_matrix(cfg.n_cep), cfg.mean,
                     cfg.scale, cfg.transform, d_out)
        assert n == T
    except BaseException:
        ctx.dev_free(d_out)
        raise
    finally:
        ctx.dev_free(d_pcm)
    return d_out, T


def frame_offsets(sample_off, hop):
    """The frame layout of a batch (spkd_mfcc_batch), on the host: the file of the samples
    [sample_off[f], sample_off[f+1]) has that many // hop frames, whatever its offset; returns
    their running sum, int64 [n_files + 1]."""
    off = np.asarray(sample_off, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(np.diff(off) // int(hop))]).astype(np.int64)


def upload_batch(ctx, pcms, timings=None):
    """The int16 samples of a batch of files, concatenated in a buffer the context keeps ->
    (d_pcm, sample_off int64 [n_files + 1]).  Each file is copied straight to its offset on the
    device: concatenating on the host first costs a pass over all samples that a batch of hour-long
    files does not win back (the front-end paragraph).  Both feature chains of a batch
    read this one upload (extract_batch).  A file is a one-dimensional array of integers that all
    fit int16; anything else -- two dimensions, floats, a value out of range -- is a ValueError,
    never a silent cast."""
    _t0 = time.perf_counter()
    files = []
    for i, p in enumerate(pcms):
        a = np.asarray(p)
        if a.ndim != 1 or (a.size and a.dtype.kind not in 'iu'):
            raise ValueError('file %d: one-dimensional int16 samples expected, got %s %r' % (i, a.dtype, a.shape))
        if a.size and a.dtype != np.int16 and (int(a.min()) < -32768 or int(a.max()) > 32767):
            raise ValueError('file %d: %s samples outside the int16 range' % (i, a.dtype))
        files.append(a.astype(np.int16, copy=False))
    sample_off = np.concatenate([[0], np.cumsum([len(a) for a in files])]).astype(np.int64)
    d_pcm = ctx.dev_scratch('pcm_batch', max(2 * int(sample_off[-1]), 16))
    for a, o in zip(files, sample_off):
        if a.size:
            ctx.h2d(d_pcm + 2 * int(o), a)
    if timings is not None:
        timings.setdefault('wall_upload', []).append(1e3 * (time.perf_counter() - _t0))
    return d_pcm, sample_off


def read_audio(path):
    """Every channel of a 16-bit PCM .wav file, int16 [n, channels], and its sample rate: the input
    of resample_batch (read_wav is the file `ffmpeg -ar 16000 -ac 1` left: mono only)."""
    with wave.open(path, 'rb') as w:
        if w.getsampwidth() != 2:
            raise ValueError('%s: 16-bit PCM expected, the file has %d-bit samples' % (path, 8 * w.getsampwidth()))
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype='<i2')
        return pcm.reshape(-1, w.getnchannels()), w.getframerate()


RESAMPLE_ZERO_CROSSINGS, RESAMPLE_BETA, RESAMPLE_CUTOFF = 16, 9.0, 0.92


def resample_ratio(rate_in, rate_out):
    """(L, M, half) of the conversion rate_in -> rate_out: output n lies at input instant n M / L, and
    half taps to either side of it enter (0: the identity conversion)."""
    rate_in, rate_out = int(rate_in), int(rate_out)
    if rate_in < 1 or rate_out < 1:
        raise ValueError('sample rates must be positive, got %d -> %d Hz' % (rate_in, rate_out))
    g = math.gcd(rate_in, rate_out)
    L, M = rate_out // g, rate_in // g
    half = 0 if L == M else -((-RESAMPLE_ZERO_CROSSINGS * max(L, M)) // L)      # ceil(16 / min(1, L / M))
    return L, M, half


def resample_taps(rate_in, rate_out):
    """The polyphase filter of spkd_resample_batch for rate_in -> rate_out (include/spkd.h has the
    definition): (float32 [L, 2 half] table, (L, M, half)); the identity conversion has an empty
    one.  A Kaiser-windowed sinc, beta 9, 16 zero crossings to either side, half-amplitude point at
    0.92 of the lower Nyquist frequency, every phase normalised to DC gain 1; formed in float64.
    PARITY UNPINNED: ffmpeg's resampler is not available and not restated."""
    L, M, half = resample_ratio(rate_in, rate_out)
    if half == 0:
        return np.zeros((L, 0), dtype=np.float32), (L, M, half)
    if half > hipabi.RESAMPLE_MAX_HALF or max(L, M) > hipabi.RESAMPLE_MAX_TERM or 2 * half * L > hipabi.RESAMPLE_MAX_TAPS:
        raise ValueError('%d Hz -> %d Hz: a filter of %d phases x %d taps is beyond this build (at most %d taps to '
                         'either side, %d in a table)' % (rate_in, rate_out, L, 2 * half, hipabi.RESAMPLE_MAX_HALF,
                                                          hipabi.RESAMPLE_MAX_TAPS))
    fc = RESAMPLE_CUTOFF * min(1.0, L / M)
    t = np.arange(-half + 1, half + 1, dtype=np.float64)[None, :] - np.arange(L, dtype=np.float64)[:, None] / L
    w = np.i0(RESAMPLE_BETA * np.sqrt(np.maximum(0.0, 1.0 - (t / half) ** 2))) / np.i0(RESAMPLE_BETA)
    h = fc * np.sinc(fc * t) * np.where(np.abs(t) > half, 0.0, w)
    h /= np.array([math.fsum(row) for row in h])[:, None]
    return h.astype(np.float32), (L, M, half)


def output_offsets(lengths, rates, rate_out):
    """The output layout of spkd_resample_batch, on the host: a file of lengths[f] sample frames at
    rates[f] Hz has ceil(n L / M) samples at rate_out (every output instant inside the input's
    span; the identity conversion keeps n); returns their running sum, int64 [n_files + 1]."""
    out = [0]
    for n, rate in zip(lengths, rates):
        L, M, _ = resample_ratio(rate, rate_out)
        out.append(out[-1] + -((-int(n) * L) // M))
    return np.array(out, dtype=np.int64)


RESAMPLE_GROUP_BYTES = 256 << 20


def _audio_files(audios):
    """resample_batch's input, checked: [(int16 [n, channels], rate)]."""
    files = []
    for i, item in enumerate(audios):
        try:
            samples, rate = item
        except (TypeError, ValueError):
            raise ValueError('file %d: a (samples, rate) pair expected' % i)
        a = np.asarray(samples)
        if a.ndim not in (1, 2) or (a.size and a.dtype.kind not in 'iu'):
            raise ValueError('file %d: int16 samples [n] or [n, channels] expected, got %s %r' % (i, a.dtype, a.shape))
        if a.ndim == 1:
            a = a.reshape(-1, 1)
        if not 1 <= a.shape[1] <= hipabi.RESAMPLE_MAX_CH:
            raise ValueError('file %d: 1 to %d channels expected, got %d' % (i, hipabi.RESAMPLE_MAX_CH, a.shape[1]))
        if a.size and a.dtype != np.int16 and (int(a.min()) < -32768 or int(a.max()) > 32767):
            raise ValueError('file %d: %s samples outside the int16 range' % (i, a.dtype))
        if isinstance(rate, bool) or not isinstance(rate, (int, np.integer)) or rate < 1:
            raise ValueError('file %d: a positive integer sample rate expected, got %r' % (i, rate))
        files.append((np.ascontiguousarray(a, dtype=np.int16), int(rate)))
    return files


# Delay-and-sum beamforming (include/spkd.h (6b2)): the analysis step, window and largest delay in
# seconds, and the tracking options of spkd_bf_track.  min_peak, jump_penalty and jump_cap rest on the
# synthetic scenes of tests/beamform_numpy.py and are UNMEASURED on speech, as every other default of
# this kind here is; parity with BeamformIt or any other beamformer is unpinned.  ref: the reference
# channel, -1 for the loudest, or a list with one entry per file.
BEAMFORM = dict(step_s=0.25, window_s=0.5, max_delay_s=0.01, n_best=4, min_peak=0.1, jump_penalty=0.02, jump_cap=25, ref=-1)
BEAMFORM_MAX_LAG = hipabi.BF_NFFT // 2
# The runner-up stream of a DelayStream(second=True) (include/spkd.h (6b5)): the smallest value of a runner-up candidate
# and how many samples it lies from the tracked delay at the least.  Both rest on the white-noise scenes of
# tests/beamform_numpy.py and are UNMEASURED on speech and in reverberation.
SECOND = dict(min_second=0.1, guard=3)


def beamform_geometry(rate, opts=BEAMFORM):
    """(H, W, D) of spkd_bf_geom for audio at `rate` Hz: D = ceil(max_delay_s rate), H = rint(step_s
    rate), W = min(rint(window_s rate), 8192 - D): the window and the largest lag share the fixed
    8192-point transform.  At 16 kHz the defaults give (4000, 8000, 160); at 48 kHz (12000, 7712, 480):
    there the window is shorter than the step, so a third of the audio is never looked at by the
    delay estimate (the sum still covers every sample).  ValueError if that leaves W < 1, H outside
    [1, 2^20] or D above 4096."""
    rate = int(rate)
    D = int(math.ceil(float(opts['max_delay_s']) * rate - 1e-9))
    H = int(round(float(opts['step_s']) * rate))
    if D < 0 or D > BEAMFORM_MAX_LAG:
        raise ValueError('%d Hz: a largest delay of %d samples is outside [0, %d]' % (rate, D, BEAMFORM_MAX_LAG))
    W = min(int(round(float(opts['window_s']) * rate)), hipabi.BF_NFFT - D)
    if W < 1:
        raise ValueError('%d Hz: a window of %d samples' % (rate, W))
    if not 1 <= H <= hipabi.BF_MAX_HOP:
        raise ValueError('%d Hz: a step of %d samples is outside [1, %d]' % (rate, H, hipabi.BF_MAX_HOP))
    return H, W, D


def _beamform_options(opts, n_files):
    """A beamform dictionary, checked: every key of BEAMFORM and no other -> (opts, ref int32 [n_files])."""
    if not isinstance(opts, dict) or set(opts) != set(BEAMFORM):
        raise ValueError('beamform: a dictionary with the keys of BEAMFORM expected (%s)' % ', '.join(sorted(BEAMFORM)))
    if not 1 <= int(opts['n_best']) <= hipabi.BF_NBEST:
        raise ValueError('beamform: n_best outside [1, %d]' % hipabi.BF_NBEST)
    if not float(opts['jump_penalty']) >= 0 or math.isinf(float(opts['jump_penalty'])) or int(opts['jump_cap']) < 0:
        raise ValueError('beamform: jump_penalty and jump_cap must not be negative')
    if math.isnan(float(opts['min_peak'])):
        raise ValueError('beamform: min_peak is not a number')
    ref = opts['ref']
    if isinstance(ref, (int, np.integer)):
        ref = [int(ref)] * n_files
    ref = np.array([int(r) for r in ref], dtype=np.int32)
    if ref.shape != (n_files,):
        raise ValueError('beamform: ref is one channel or one per file (%d files, %d entries)' % (n_files, ref.size))
    return opts, ref


def _beamform_plan(files, opts):
    """Geometries and reference channels of checked files -> (geoms, geom index int32, ref int32)."""
    opts, ref = _beamform_options(opts, len(files))
    rates = sorted(set(rate for _, rate in files))
    geoms = [beamform_geometry(rate, opts) for rate in rates]
    for i, ((a, _), r) in enumerate(zip(files, ref)):
        if not -1 <= r < a.shape[1]:
            raise ValueError('file %d: reference channel %d of %d channels' % (i, r, a.shape[1]))
    return geoms, np.array([rates.index(rate) for _, rate in files], dtype=np.int32), ref


def _beamform_steps(frames, channels, geom, geoms):
    """The steps of every file (spkd_bf_gcc's count): none for one channel, else one and one more for every
    whole hop the window can move inside the file -> int64 [n_files]."""
    return np.array([0 if c == 1 else (1 if n <= geoms[g][1] else (n - geoms[g][1]) // geoms[g][0] + 1)
                     for n, c, g in zip(frames, channels, geom)], dtype=np.int64)


def _beamform_group(ctx, d_raw, in_off, channels, geom, geoms, ref, opts, d_out, ms, detail=None, delays=None):
    """The three stages on one uploaded group -> out_off; ms[stage] += the stage's time.  delays: None, or
    (stream, first file): the group's delays are packed into their place of the DelayStream before the next
    group reuses the scratch (spkd_tdoa_pack; one read-back of d_ref for the reference channels)."""
    n_files = len(channels)
    C = np.asarray(channels, dtype=np.int64)
    frames = np.diff(in_off) // C
    T = _beamform_steps(frames, C, geom, geoms)
    wg_off = np.concatenate([[0], np.cumsum(T * C)]).astype(np.int64)
    total = int(wg_off[-1])
    d_ref = ctx.dev_scratch('bf_ref', max(4 * n_files, 16))
    d_lag = ctx.dev_scratch('bf_lag', max(16 * total, 16))
    d_val = ctx.dev_scratch('bf_val', max(16 * total, 16))
    d_delay = ctx.dev_scratch('bf_delay', max(4 * total, 16))
    step_off, _ = ctx.bf_gcc(d_raw, in_off, channels, geom, geoms, ref, d_ref, d_lag, d_val)
    assert np.array_equal(np.diff(step_off), T)
    some = int(in_off[-1]) > 0
    if some:
        ms['bf_gcc'] += ctx.last_ms('bf_gcc')
        ctx.bf_track(step_off, channels, d_lag, d_val, opts['n_best'], opts['min_peak'], opts['jump_penalty'], opts['jump_cap'],
                     d_delay)
        if total:
            ms['bf_track'] += ctx.last_ms('bf_track')
    out_off = ctx.bf_sum(d_raw, in_off, channels, geom, geoms, d_delay, d_out)
    if some:
        ms['bf_sum'] += ctx.last_ms('bf_sum')
    if delays is not None:
        delays[0]._pack_group(delays[1], T, C, d_ref if some else None, ref, d_delay, d_val, opts['min_peak'], ms, d_lag,
                              opts['n_best'])
    if detail is not None:
        got_ref = np.zeros(n_files, dtype=np.int32)
        delay = np.zeros(total, dtype=np.int32)
        val = np.zeros(4 * total, dtype=np.float32)
        if some:
            ctx.d2h(got_ref, d_ref)
        if some and total:
            ctx.d2h(delay, d_delay)
            ctx.d2h(val, d_val)
        for f in range(n_files):
            shape = (int(T[f]), int(C[f]))
            detail.setdefault('ref', []).append(int(got_ref[f]))
            detail.setdefault('delay', []).append(delay[wg_off[f]:wg_off[f + 1]].reshape(shape).copy())
            detail.setdefault('reliable', []).append(
                val[4 * wg_off[f]:4 * wg_off[f + 1]].reshape(shape + (4,))[:, :, 0] >= np.float32(opts['min_peak']))
    return out_off


def frame_step(t, hop, window, rate_in, rate_out, H, T):
    """The step of a file's feature frame t (file-local): the rule of csrc/spkd_tdoa.hpp (tdoa_step; include/spkd.h
    (6b3)), mirrored here in Python integers: min(T - 1, ((t hop + window // 2) rate_in) // (rate_out H))."""
    return min(int(T) - 1, ((int(t) * int(hop) + int(window) // 2) * int(rate_in)) // (int(rate_out) * int(H)))


def step_first_frame(s, hop, window, rate_in, rate_out, H):
    """The first frame of step s under frame_step without its clamp (tdoa_first_frame): the smallest t >= 0
    with (t hop + window // 2) rate_in >= s rate_out H."""
    if s <= 0:
        return 0
    q = -((-int(s) * int(rate_out) * int(H)) // int(rate_in)) - int(window) // 2
    return 0 if q <= 0 else -((-q) // int(hop))


class DelayStream(object):
    """The delays the beamformer tracked, kept on the device for a whole batch (include/spkd.h (6b3)): one
    array of packed int32, entry (f, t, c) at off_f + t C_f + c the delay of step t of file f on channel c in
    input samples, or hipabi.TDOA_NONE where the step is not reliable there -- _beamform_group's test, the
    first candidate's value >= min_peak as float32.  hop, window: the feature configuration's, in samples
    at rate_out, the rate the features are computed at: they and the per-file table (off, T, C, reference
    channel, H, input rate) take a feature frame to its step (frame_step).  resample_batch(..., beamform=b,
    delays=stream) and beamform_batch(..., delays=stream) fill it; from_arrays builds one from host arrays;
    resegment_batch(..., delays=stream) reads it.  A one-channel file has T = 0.  The buffer is a scratch
    slot of the context: a stream lives until the next one is laid out on the same context, and says so
    (ValueError) when it is used after that.
    second=True: the stream also keeps, in a scratch slot of its own under the same rule, the runner-up lag of every
    entry (include/spkd.h (6b5); spkd_tdoa_second with min_second and guard, SECOND's unless given): the other
    talker's seat while two speak at once, which overlap.overlap_batch reads (handle_second, to_host_second).
    second=False makes no call and no allocation for it."""

    def __init__(self, ctx, hop, window, rate_out=16000, second=False, min_second=None, guard=None):
        hop, window, rate_out = int(hop), int(window), int(rate_out)
        if hop < 1 or window < 0 or rate_out < 1:
            raise ValueError('DelayStream: hop >= 1, window >= 0 and rate_out >= 1, in samples and Hz')
        if not isinstance(second, (bool, np.bool_)):
            raise ValueError('DelayStream second: True or False')
        self.ctx, self.hop, self.window, self.rate_out = ctx, hop, window, rate_out
        self.second, self.d_second, self.from_beamformer = bool(second), None, False
        self.min_second = float(SECOND['min_second'] if min_second is None else min_second)
        self.guard = int(SECOND['guard'] if guard is None else guard)
        if self.second and (np.isnan(self.min_second) or self.guard < 0):
            raise ValueError('DelayStream: min_second a number and guard >= 0')
        self.d_stream, self.n_entries, self._generation = None, 0, 0
        self.files = np.zeros((0, 6), dtype=np.int64)      # off, T, C, ref, H, rate_in

    @property
    def n_files(self):
        return len(self.files)

    def _check_steps(self, C, H, rates):
        """A step is at least a feature frame long (include/spkd.h (6b3)); an input error, before any device work."""
        for f, (h, rate, c) in enumerate(zip(H, rates, C)):
            if c > 1 and int(h) * self.rate_out < self.hop * int(rate):
                raise ValueError('file %d: a step of %d samples at %d Hz is shorter than a feature frame' % (f, h, rate))

    def _check_plan(self, files, geom, geoms):
        self._check_steps([a.shape[1] for a, _ in files], [geoms[g][0] for g in geom], [rate for _, rate in files])

    def _current(self):
        """The buffer is the context's one slot: a stream laid out later on the same context took it over."""
        if self.d_stream is not None and getattr(self.ctx, '_tdoa_generation', self._generation) != self._generation:
            raise ValueError('delays: a later stream was laid out on this context, which holds one at a time')

    def _lay_out(self, ctx, T, C, ref, H, rates):
        T, C = np.asarray(T, dtype=np.int64).reshape(-1), np.asarray(C, dtype=np.int64).reshape(-1)
        self._check_steps(C, H, rates)
        off = np.concatenate([[0], np.cumsum(T * C)]).astype(np.int64)
        self.files = np.column_stack([off[:-1], T, C, np.asarray(ref, dtype=np.int64).reshape(-1),
                                      np.asarray(H, dtype=np.int64).reshape(-1),
                                      np.asarray(rates, dtype=np.int64).reshape(-1)]).astype(np.int64).reshape(-1, 6)
        self.ctx, self.n_entries = ctx, int(off[-1])
        self.d_stream = ctx.dev_scratch('tdoa_stream', max(4 * self.n_entries, 16))
        if self.second:
            self.d_second = ctx.dev_scratch('tdoa_second', max(4 * self.n_entries, 16))
        self._generation = ctx._tdoa_generation = getattr(ctx, '_tdoa_generation', 0) + 1

    def _reserve(self, ctx, files, geom, geoms):
        """The layout of a batch of checked files, before its first group: every file's steps are known from
        its length (_beamform_steps); the reference channels arrive with the groups."""
        C = np.array([a.shape[1] for a, _ in files], dtype=np.int64)
        T = _beamform_steps([len(a) for a, _ in files], C, geom, geoms)
        self._lay_out(ctx, T, C, np.full(len(files), -1), [geoms[g][0] for g in geom], [rate for _, rate in files])
        self.from_beamformer = True                        # (its runner-ups are min_second's and guard's)

    def _pack_group(self, first, T, C, d_ref, want_ref, d_delay, d_val, min_peak, ms, d_lag=None, n_best=None):
        n_files, total = len(T), int((T * C).sum())
        assert np.array_equal(self.files[first:first + n_files, 1], T) and np.array_equal(self.files[first:first + n_files, 2], C)
        at = self.d_stream + 4 * int(self.files[first, 0])
        if self.second and total:
            at2 = self.d_second + 4 * int(self.files[first, 0])
            if d_ref is None:                              # (a group without a sample has no candidates: no runner-up)
                self.ctx.h2d(at2, np.full(total, hipabi.TDOA_NONE, dtype=np.int32))
            else:
                self.ctx.tdoa_second(d_delay, d_lag, d_val, n_best, min_peak, self.min_second, self.guard, total, at2)
                ms['tdoa_second'] = ms.get('tdoa_second', 0.0) + self.ctx.last_ms('tdoa_second')
        if d_ref is None:
            # a group without a sample: the beamformer launched nothing.  Its files' one step holds what the kernels
            # define for it in any other grouping: the requested reference channel, else channel 0, at lag 0 with
            # value 1, and no other channel
            got_ref = np.where(np.asarray(want_ref) >= 0, want_ref, 0).astype(np.int32)
            entries = np.full(total, hipabi.TDOA_NONE, dtype=np.int32)
            if np.float32(1.0) >= np.float32(min_peak):
                entries[(self.files[first:first + n_files, 0] - self.files[first, 0] + got_ref)[T > 0]] = 0
            if total:
                self.ctx.h2d(at, entries)
        else:
            got_ref = np.zeros(n_files, dtype=np.int32)
            self.ctx.d2h(got_ref, d_ref)
            if total:
                self.ctx.tdoa_pack(d_delay, d_val, min_peak, total, at)
                ms['tdoa_pack'] += self.ctx.last_ms('tdoa_pack')
        self.files[first:first + n_files, 3] = got_ref

    @classmethod
    def from_arrays(cls, ctx, hop, window, files, rate_out=16000, second=None):
        """The same stream from host arrays, for known geometries and for tests: files = [(delay int32 [T, C],
        reliable bool [T, C], ref, H, rate_in)]; a delay beyond +-4096 samples on a reliable entry, a reference
        channel outside the file's, shapes that differ: ValueError.  second: None, or per file the runner-up stream as
        it lies on the device, int32 [T, C] with hipabi.TDOA_NONE for none (or None: none anywhere in the file)."""
        self = cls(ctx, hop, window, rate_out, second=second is not None)
        if second is not None and len(second) != len(files):
            raise ValueError('second: one array, or None, per file')
        packed, T, C, refs, Hs, rates = [], [], [], [], [], []
        for f, (delay, reliable, ref, H, rate_in) in enumerate(files):
            d, r = np.asarray(delay), np.asarray(reliable)
            if d.ndim != 2 or d.shape != r.shape or d.dtype.kind not in 'iu' or r.dtype != np.bool_:
                raise ValueError('file %d: delay int32 [T, C] and reliable bool [T, C] expected' % f)
            if not 1 <= d.shape[1] <= hipabi.TDOA_MAX_CH:
                raise ValueError('file %d: 1 to %d channels expected' % (f, hipabi.TDOA_MAX_CH))
            if d.shape[1] == 1 and d.shape[0]:
                raise ValueError('file %d: a one-channel file has no steps' % f)
            if d.shape[1] > 1 and not 0 <= int(ref) < d.shape[1]:
                raise ValueError('file %d: reference channel %d of %d channels' % (f, ref, d.shape[1]))
            if int(H) < 1 or int(H) > hipabi.BF_MAX_HOP or int(rate_in) < 1:
                raise ValueError('file %d: a step of 1 to %d samples and a positive rate expected' % (f, hipabi.BF_MAX_HOP))
            if r.any() and int(np.abs(d[r].astype(np.int64)).max()) > hipabi.TDOA_MAX_DELAY:
                raise ValueError('file %d: a delay beyond %d samples' % (f, hipabi.TDOA_MAX_DELAY))
            packed.append(np.where(r, d.astype(np.int64), hipabi.TDOA_NONE).astype(np.int32).ravel())
            if second is not None and second[f] is not None:
                q = np.asarray(second[f])
                if q.shape != d.shape or q.dtype.kind not in 'iu':
                    raise ValueError('file %d: second int32 [T, C] expected' % f)
                if ((q != hipabi.TDOA_NONE) & (np.abs(q.astype(np.int64)) > hipabi.TDOA_MAX_DELAY)).any():
                    raise ValueError('file %d: a runner-up beyond %d samples' % (f, hipabi.TDOA_MAX_DELAY))
            T.append(d.shape[0]), C.append(d.shape[1]), refs.append(int(ref)), Hs.append(int(H)), rates.append(int(rate_in))
        self._lay_out(ctx, T, C, refs, Hs, rates)
        if self.n_entries:
            ctx.h2d(self.d_stream, np.concatenate(packed))
            if second is not None:
                ctx.h2d(self.d_second, np.concatenate([np.full(len(p), hipabi.TDOA_NONE, dtype=np.int32) if q is None else
                                                       np.asarray(q).astype(np.int32).ravel() for p, q in zip(packed, second)]))
        return self

    def table(self, frame_off):
        """The file table of the C calls (hipabi.TDOA_FILE int64 per file): the six columns and frame_off[f], the
        file's first frame in the batch's numbering."""
        frame_off = np.asarray(frame_off, dtype=np.int64).reshape(-1)
        if len(frame_off) != self.n_files:
            raise ValueError('delays: a stream of %d files, a batch of %d' % (self.n_files, len(frame_off)))
        return np.column_stack([self.files, frame_off, np.zeros(self.n_files, dtype=np.int64)]).astype(np.int64).reshape(-1, hipabi.TDOA_FILE)

    def handle(self, frame_off):
        """What hipabi's tdoa_stats and tdoa_score take as `stream`.  ValueError when a later stream of the
        context has taken the buffer."""
        self._current()
        return self.d_stream, self.n_entries, self.table(frame_off), (self.hop, self.window, self.rate_out)

    def handle_second(self):
        """The device pointer of the runner-up stream, what hipabi's tdoa_overlap takes as d_second.  ValueError for a
        stream made without second=True, and when a later stream of the context has taken the buffers."""
        if not self.second:
            raise ValueError('delays: the stream keeps no runner-ups; make it with DelayStream(..., second=True)')
        self._current()
        return self.d_second

    def to_host_second(self):
        """Per file the runner-up stream, int32 [T, C], hipabi.TDOA_NONE where there is none."""
        d_second = self.handle_second()
        packed = np.full(self.n_entries, hipabi.TDOA_NONE, dtype=np.int32)
        if self.n_entries and d_second is not None:
            self.ctx.d2h(packed, d_second)
        return [packed[off:off + T * C].reshape(T, C).copy() for off, T, C, _, _, _ in self.files.tolist()]

    def first_frame_of(self, f, s):
        """The first frame (file-local) of step s of file f (step_first_frame with the file's table entry)."""
        _, _, _, _, H, rate_in = (int(v) for v in self.files[f])
        return step_first_frame(s, self.hop, self.window, rate_in, self.rate_out, H)

    def step_of(self, f, t):
        """The step of file f's frame t (frame_step with the file's table entry); the file has steps."""
        _, T, _, _, H, rate_in = (int(v) for v in self.files[f])
        return frame_step(t, self.hop, self.window, rate_in, self.rate_out, H, T)

    def to_host(self):
        """Per file (delay int32 [T, C], reliable bool [T, C]): delay is 0 where not reliable."""
        self._current()
        packed = np.zeros(self.n_entries, dtype=np.int32)
        if self.n_entries:
            self.ctx.d2h(packed, self.d_stream)
        out = []
        for off, T, C, _, _, _ in self.files.tolist():
            p = packed[off:off + T * C].reshape(T, C)
            ok = p != hipabi.TDOA_NONE
            out.append((np.where(ok, p, 0).astype(np.int32), ok))
        return out


def _note_beamform(timings, ms):
    if timings is not None:
        for k, v in ms.items():
            timings.setdefault(k, []).append(v)


def beamform_batch(ctx, audios, opts=BEAMFORM, timings=None, detail=None, delays=None):
    """The channels of every file aligned and summed on the device (spkd_bf_gcc, spkd_bf_track,
    spkd_bf_sum; include/spkd.h (6b2)): audios as resample_batch takes them -> (d_mono, sample_off),
    the mono int16 files at their own rates, still on the device in a buffer the context keeps, file f
    at [sample_off[f], sample_off[f+1]).  A one-channel file is copied through.  opts: a dictionary
    like BEAMFORM.  detail, if a dictionary, receives per file 'ref' (the reference channel), 'delay'
    (int32 [T, C]) and 'reliable' (bool [T, C]).  Input errors are ValueErrors before the context is
    touched.  delays: None, or a DelayStream, which is filled with the batch's delays (the files stay at
    their own rates here, so every file's rate must be the stream's rate_out)."""
    files = _audio_files(audios)
    geoms, geom, ref = _beamform_plan(files, opts)
    channels = np.array([a.shape[1] for a, _ in files], dtype=np.int32)
    if delays is not None:
        if any(rate != delays.rate_out for _, rate in files):
            raise ValueError('delays: beamform_batch does not resample, every file must be at the stream\'s %d Hz' % delays.rate_out)
        delays._check_plan(files, geom, geoms)
    in_off = np.concatenate([[0], np.cumsum([a.size for a, _ in files])]).astype(np.int64)
    sample_off = np.concatenate([[0], np.cumsum([len(a) for a, _ in files])]).astype(np.int64)
    d_raw = ctx.dev_scratch('audio_batch', max(2 * int(in_off[-1]), 16))
    d_out = ctx.dev_scratch('bf_mono', max(2 * int(sample_off[-1]), 16))
    _t0 = time.perf_counter()
    for (a, _), o in zip(files, in_off):
        if a.size:
            ctx.h2d(d_raw + 2 * int(o), a)
    wall = time.perf_counter() - _t0
    ms = dict(bf_gcc=0.0, bf_track=0.0, bf_sum=0.0)
    if delays is not None:
        ms['tdoa_pack'] = 0.0
        delays._reserve(ctx, files, geom, geoms)
    got = _beamform_group(ctx, d_raw, in_off, channels, geom, geoms, ref, opts, d_out, ms, detail,
                          None if delays is None else (delays, 0))
    assert np.array_equal(got, sample_off)
    if timings is not None:
        timings.setdefault('wall_upload', []).append(1e3 * wall)
    _note_beamform(timings, ms)
    return d_out, sample_off


def resample_batch(ctx, audios, rate_out, group_bytes=RESAMPLE_GROUP_BYTES, timings=None, beamform=None, delays=None):
    """The audio of a batch of files, audios = [(samples, rate)] with int16 samples [n] or
    [n, channels], converted to mono at rate_out on the device (spkd_resample_batch) -> (d_pcm,
    sample_off), exactly what upload_batch returns for the converted files: vad_batch(uploaded=...)
    and features_batch(uploaded=...) take it unchanged.  The raw audio goes up in groups of whole
    files of at most group_bytes (a larger file is a group of its own) into a scratch the context
    keeps, and each group is converted into its place of the 'pcm_batch' buffer, whose offsets are
    known beforehand (output_offsets): the raw scratch stays bounded, an hour of 48 kHz stereo being
    six times its 16 kHz mono.  Anything but integer samples that fit int16, one to eight channels
    and a positive integer rate is a ValueError before the context is touched.
    beamform: None, or a dictionary like BEAMFORM: each uploaded group is then aligned and summed
    (beamform_batch's three calls) into a second scratch, bounded like the first, and resampled from
    there as one-channel files, instead of being averaged by the resampler's downmix.
    delays: None, or a DelayStream (with beamform only), which is filled group by group with the delays the
    beamformer tracked: they survive the groups there, for resegment_batch(delays=...)."""
    files = _audio_files(audios)
    rate_out = int(rate_out)
    if group_bytes < 1:
        raise ValueError('group_bytes must be positive')
    if delays is not None and beamform is None:
        raise ValueError('delays: the delay stream is filled by the beamformer, which takes beamform=')
    if delays is not None and delays.rate_out != rate_out:
        raise ValueError('delays: the stream counts its frames at %d Hz, the conversion is to %d Hz' % (delays.rate_out, rate_out))
    if beamform is not None:
        geoms, geom, ref = _beamform_plan(files, beamform)
        if delays is not None:
            delays._check_plan(files, geom, geoms)
    rates = sorted(set(rate for _, rate in files))
    convs, tables, at = [], [], 0
    for rate in rates:
        h, (L, M, half) = resample_taps(rate, rate_out)
        convs.append(hipabi.ResampleConv(L, M, half, at))
        tables.append(h.ravel())
        at += h.size
    taps = np.concatenate(tables) if tables else np.zeros(0, dtype=np.float32)
    conv = np.array([rates.index(rate) for _, rate in files], dtype=np.int32)
    channels = np.array([a.shape[1] for a, _ in files], dtype=np.int32)
    sample_off = output_offsets([len(a) for a, _ in files], [rate for _, rate in files], rate_out)
    # groups of consecutive files
    groups, first, size = [], 0, 0
    for f, (a, _) in enumerate(files):
        if f > first and size + a.nbytes > group_bytes:
            groups.append((first, f))
            first, size = f, 0
        size += a.nbytes
    if len(files) > first:
        groups.append((first, len(files)))
    biggest = max([sum(files[f][0].nbytes for f in range(lo, hi)) for lo, hi in groups] + [0])
    d_pcm = ctx.dev_scratch('pcm_batch', max(2 * int(sample_off[-1]), 16))
    d_raw = ctx.dev_scratch('audio_batch', max(biggest, 16))
    wall, ms = 0.0, 0.0
    if beamform is not None:
        most = max([sum(len(files[f][0]) for f in range(lo, hi)) for lo, hi in groups] + [0])
        d_mono = ctx.dev_scratch('bf_mono', max(2 * most, 16))
        bf_ms = dict(bf_gcc=0.0, bf_track=0.0, bf_sum=0.0)
        if delays is not None:
            bf_ms['tdoa_pack'] = 0.0
            delays._reserve(ctx, files, geom, geoms)
    for lo, hi in groups:
        in_off = np.concatenate([[0], np.cumsum([files[f][0].size for f in range(lo, hi)])]).astype(np.int64)
        _t0 = time.perf_counter()
        for f, o in zip(range(lo, hi), in_off):
            if files[f][0].size:
                ctx.h2d(d_raw + 2 * int(o), files[f][0])
        wall += time.perf_counter() - _t0
        if beamform is not None:
            mono_off = _beamform_group(ctx, d_raw, in_off, channels[lo:hi], geom[lo:hi], geoms, ref[lo:hi], beamform, d_mono, bf_ms,
                                       delays=None if delays is None else (delays, lo))
            got = ctx.resample_batch(d_mono, mono_off, np.ones(hi - lo, dtype=np.int32), conv[lo:hi], convs, taps,
                                     d_pcm + 2 * int(sample_off[lo]))
        else:
            got = ctx.resample_batch(d_raw, in_off, channels[lo:hi], conv[lo:hi], convs, taps, d_pcm + 2 * int(sample_off[lo]))
        assert np.array_equal(got, sample_off[lo:hi + 1] - sample_off[lo])
        if got[-1]:
            ms += ctx.last_ms('resample')
    if timings is not None:
        timings.setdefault('wall_upload', []).append(1e3 * wall)
        timings.setdefault('resample', []).append(ms)
    if beamform is not None:
        _note_beamform(timings, bf_ms)
    return d_pcm, sample_off


def extract_batch(ctx, cfg, d_pcm, sample_off, d_out=None, timings=None):
    """Uploaded samples (upload_batch) -> (device pointer to the float32 [sum T, 39] features of
    every file, frame_off int64 [n_files + 1]) in one call (spkd_mfcc_batch).  d_out=None: a buffer
    the context keeps per window width, so the VAD chain and the diarization chain of one batch do
    not share one."""
    frame_off = frame_offsets(sample_off, cfg.hop)
    total = int(frame_off[-1])
    if d_out is None:
        d_out = ctx.dev_scratch('features_w%d' % cfg.window_width, max(total, 1) * cfg.dim * 4)
    got = ctx.mfcc_batch(d_pcm, sample_off, mfcc_params(cfg), mel_filterbank(cfg.sample_rate), dct_matrix(cfg.n_cep),
                         cfg.mean, cfg.scale, cfg.transform, d_out)
    assert np.array_equal(got, frame_off)
    if timings is not None and total:
        timings.setdefault('mfcc_static', []).append(ctx.last_ms('mfcc_static'))
        timings.setdefault('mfcc_post', []).append(ctx.last_ms('mfcc_post'))
    return d_out, got


def extract(pcm, cfg, ctx=None, device=0):
    """int16 samples -> float32 [T, 39] features (device computation, result on the host)."""
    own = ctx is None
    if own:
        ctx = hipabi.Context(device)
    try:
        d_out, T = extract_device(pcm, cfg, ctx)
        out = np.zeros((T, cfg.dim), dtype=np.float32)
        if T:
            try:
                ctx.d2h(out, d_out)
            finally:
                ctx.dev_free(d_out)
        return out
    finally:
        if own:
            ctx.close()


def main(argv=None, stdout=None):
    ap = argparse.ArgumentParser(description='feacat-shaped feature extraction (the options spk-diarization2.py uses).')
    ap.add_argument('-c', dest='config', required=True, help='feature configuration (fconfig.cfg)')
    ap.add_argument('-H', dest='header', action='store_true', help='write the int32 dimension header')
    ap.add_argument('--raw-output', dest='raw', action='store_true', help='raw float32 frames')
    ap.add_argument('wav')
    args = ap.parse_args(argv)
    cfg = FeatureConfig.load(args.config)
    pcm, rate = read_wav(args.wav)
    if rate != cfg.sample_rate:
        raise ValueError('%s is sampled at %d Hz, the configuration wants %d' % (args.wav, rate, cfg.sample_rate))
    feats = extract(pcm, cfg)
    out = stdout or sys.stdout.buffer
    if args.header:
        out.write(np.array([feats.shape[1]], dtype='<i4').tobytes())
    out.write(np.ascontiguousarray(feats, dtype='<f4').tobytes())
    return 0


def to16k_main(argv=None):
    """./to16k.py IN.wav [-o OUT.wav] [-r 16000] [--beamform]: one 16-bit PCM .wav of any rate and channel count
    -> 16-bit mono at the rate the pipeline wants, converted on the device (resample_batch).  What a
    user without ffmpeg runs in front of spk-diarization2.py for .wav input."""
    ap = argparse.ArgumentParser(description='Resample and downmix a 16-bit PCM .wav on the device (the step '
                                             '`ffmpeg -ar 16000 -ac 1` is for .wav input).')
    ap.add_argument('wav')
    ap.add_argument('-o', dest='out', default=None, help='output file (default: IN.16k.wav beside the input)')
    ap.add_argument('-r', dest='rate', type=int, default=16000, help='output sample rate')
    ap.add_argument('--beamform', action='store_true',
                    help='align the channels before summing them (delay-and-sum with the BEAMFORM defaults) '
                         'instead of averaging them')
    args = ap.parse_args(argv)
    out = args.out or os.path.splitext(args.wav)[0] + '.16k.wav'
    samples, rate = read_audio(args.wav)
    ctx = hipabi.Context(0)
    try:
        d_pcm, sample_off = resample_batch(ctx, [(samples, rate)], args.rate, beamform=BEAMFORM if args.beamform else None)
        pcm = np.zeros(int(sample_off[-1]), dtype=np.int16)
        if pcm.size:
            ctx.d2h(pcm, d_pcm)
    finally:
        ctx.close()
    with wave.open(out, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(args.rate)
        w.writeframes(pcm.astype('<i2').tobytes())
    return 0
