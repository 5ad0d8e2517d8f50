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
