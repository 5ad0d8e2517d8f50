#!/usr/bin/env python
"""Times spkd_resample_batch (k_resample) on a batch of --files x --seconds of audio at 48 kHz stereo,
44.1 kHz stereo and 8 kHz mono, converted to 16 kHz mono.  The raw audio of one file (int16 noise) is
generated once and copied to every file's place in one device buffer, so the host holds one file; each
shape gets a warm-up and then --runs calls.  Per shape: the median of the `resample` kernel timer and
its [min, median, max], the bytes the kernel has to read (the raw audio) plus the bytes it writes (the
16 kHz mono samples) and the GB/s they make of that time, the fp64 FMAs (2 half per output sample)
and their rate, and `mfcc_static` of spkd_mfcc_batch over the converted batch for scale.  device_copy
is a device-to-device copy of --copy-mib in the same process, read plus written bytes over its
synchronous wall time: the bandwidth the GB/s are a fraction of (copy_fraction).

  python tools/resample_time.py [--files 64] [--seconds 600] [--runs 5] [--out profiles/resample_time.json]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
hipabi = importlib.import_module('speaker-diarization_amd.hipabi')
fe = importlib.import_module('speaker-diarization_amd.frontend')
from mfcc_batch_time import config, spread      # noqa: E402  (fconfig.cfg's structure with stand-in arrays)

RATE_OUT = 16000
SHAPES = ((48000, 2), (44100, 2), (8000, 1))


def device_copy(ctx, mib, runs):
    """GB/s of a device-to-device copy, bytes read plus bytes written."""
    nbytes = mib << 20
    d = ctx.dev_alloc(2 * nbytes)
    try:
        ctx.copy_d2d(d + nbytes, d, nbytes)
        ms = []
        for _ in range(runs):
            t = time.perf_counter()
            ctx.copy_d2d(d + nbytes, d, nbytes)
            ms.append(1e3 * (time.perf_counter() - t))
    finally:
        ctx.dev_free(d)
    return dict(mib=mib, ms=spread(ms), gb_per_s=round(2 * nbytes / (1e6 * float(np.median(ms))), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--seconds', type=int, default=600)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--copy-mib', type=int, default=1024)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'resample_time.json'))
    a = ap.parse_args()
    ctx = hipabi.Context(0)
    rng = np.random.default_rng(16)
    cfg = config(400)
    res = dict(files=a.files, seconds=a.seconds, runs=a.runs, tile=hipabi.RESAMPLE_TILE,
               device_copy=device_copy(ctx, a.copy_mib, a.runs))
    print('device copy: %s' % json.dumps(res['device_copy']), file=sys.stderr, flush=True)
    for rate, channels in SHAPES:
        one = rng.integers(-32768, 32768, (a.seconds * rate, channels), dtype=np.int16)
        table, (L, M, half) = fe.resample_taps(rate, RATE_OUT)
        in_off = np.arange(a.files + 1, dtype=np.int64) * one.size
        sample_off = fe.output_offsets([len(one)] * a.files, [rate] * a.files, RATE_OUT)
        d_raw = ctx.dev_scratch('time_resample_raw', int(in_off[-1]) * 2)
        d_pcm = ctx.dev_scratch('pcm_batch', int(sample_off[-1]) * 2)
        for o in in_off[:-1]:
            ctx.h2d(d_raw + 2 * int(o), one)
        ms, static = [], []
        for run in range(a.runs + 1):                                # the first one warms up
            got = ctx.resample_batch(d_raw, in_off, [channels] * a.files, [0] * a.files, [(L, M, half, 0)], table, d_pcm)
            assert np.array_equal(got, sample_off)
            ms.append(ctx.last_ms('resample'))
            fe.extract_batch(ctx, cfg, d_pcm, sample_off)
            static.append(ctx.last_ms('mfcc_static'))
        ms, static = ms[1:], static[1:]
        med = float(np.median(ms))
        nbytes = 2 * int(in_off[-1]) + 2 * int(sample_off[-1])
        fmas = 2 * half * int(sample_off[-1])
        gbs = nbytes / (1e6 * med)
        row = res['%d Hz x %d' % (rate, channels)] = dict(
            up=L, down=M, half_taps=half, table_bytes=int(table.nbytes), samples_out=int(sample_off[-1]),
            resample_ms=round(med, 3), resample_ms_spread=spread(ms), bytes_read_plus_written=nbytes,
            gb_per_s=round(gbs, 1), copy_fraction=round(gbs / res['device_copy']['gb_per_s'], 3),
            fp64_fma=fmas, fp64_tflops=round(2 * fmas / (1e9 * med), 2),
            ms_per_audio_hour=round(med / (a.files * a.seconds / 3600.0), 3),
            mfcc_static_ms=round(float(np.median(static)), 3))
        print('%d Hz x %d: %s' % (rate, channels, json.dumps(row)), file=sys.stderr, flush=True)
        del one
    ctx.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
