#!/usr/bin/env python
"""Times the three beamforming calls (spkd_bf_gcc, spkd_bf_track, spkd_bf_sum) on a batch of --files x
--seconds of --channels-channel audio at 16 kHz: one file (a source at a delay of its own per channel,
over independent noise) is generated once and copied to every file's place, so the host holds one file;
a warm-up, then --runs rounds of the three calls.  Recorded: the median of each timer with its [min,
median, max], `wall_upload` (the host-to-device copies of the same audio, synchronous wall time) and
the three calls' share of it, the steps and transforms of the batch, the counted float32 flops of the
transforms (5 N log2 N each, two per step and non-reference channel) and their rate, the bytes the sum
reads and writes, and milliseconds per audio-hour.  No gate rests on these numbers.

  python tools/beamform_time.py [--files 8] [--seconds 600] [--channels 8] [--runs 5] [--out profiles/beamform_time.json]"""
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
from mfcc_batch_time import spread      # noqa: E402

RATE = 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=8)
    ap.add_argument('--seconds', type=int, default=600)
    ap.add_argument('--channels', type=int, default=8)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'beamform_time.json'))
    a = ap.parse_args()
    opts = fe.BEAMFORM
    H, W, D = geom = fe.beamform_geometry(RATE, opts)
    rng = np.random.default_rng(16)
    n, C = a.seconds * RATE, a.channels
    source = rng.integers(-6000, 6001, n + 2 * D, dtype=np.int16)
    delays = rng.integers(-(D // 2), D // 2 + 1, C)            # any two channels within D of each other
    one = np.stack([source[D - d:D - d + n] for d in delays], axis=1) + rng.integers(-1500, 1501, (n, C), dtype=np.int16)
    one = np.ascontiguousarray(one, dtype=np.int16)
    ctx = hipabi.Context(0)
    in_off = np.arange(a.files + 1, dtype=np.int64) * one.size
    T = (n - W) // H + 1 if n > W else 1
    total = a.files * T * C
    d_raw = ctx.dev_scratch('time_bf_raw', int(in_off[-1]) * 2)
    d_out = ctx.dev_scratch('time_bf_out', a.files * n * 2)
    d_ref = ctx.dev_scratch('time_bf_ref', 4 * a.files)
    d_lag, d_val = ctx.dev_scratch('time_bf_lag', 16 * total), ctx.dev_scratch('time_bf_val', 16 * total)
    d_delay = ctx.dev_scratch('time_bf_delay', 4 * total)
    upload = []
    for run in range(2):                                             # the first one warms up
        t0 = time.perf_counter()
        for o in in_off[:-1]:
            ctx.h2d(d_raw + 2 * int(o), one)
        upload.append(1e3 * (time.perf_counter() - t0))
    ms = dict(bf_gcc=[], bf_track=[], bf_sum=[])
    channels, gi = [C] * a.files, [0] * a.files
    for run in range(a.runs + 1):
        step_off, _ = ctx.bf_gcc(d_raw, in_off, channels, gi, [geom], [-1] * a.files, d_ref, d_lag, d_val)
        ms['bf_gcc'].append(ctx.last_ms('bf_gcc'))
        ctx.bf_track(step_off, channels, d_lag, d_val, opts['n_best'], opts['min_peak'], opts['jump_penalty'], opts['jump_cap'], d_delay)
        ms['bf_track'].append(ctx.last_ms('bf_track'))
        ctx.bf_sum(d_raw, in_off, channels, gi, [geom], d_delay, d_out)
        ms['bf_sum'].append(ctx.last_ms('bf_sum'))
    assert int(step_off[-1]) == a.files * T
    delay = np.zeros(total, dtype=np.int32)
    ref = np.zeros(a.files, dtype=np.int32)
    ctx.d2h(delay, d_delay)
    ctx.d2h(ref, d_ref)
    found = delay.reshape(a.files, T, C)
    right = float(np.mean(found == (delays - delays[ref[0]])[None, None, :]))
    ctx.close()
    med = {k: float(np.median(v[1:])) for k, v in ms.items()}
    hours = a.files * a.seconds / 3600.0
    transforms = 2 * a.files * T * (C - 1)
    flops = transforms * 5 * hipabi.BF_NFFT * 13
    sum_bytes = 2 * int(in_off[-1]) * 2 + 2 * a.files * n            # two reads of every channel, one write
    all_ms = sum(med.values())
    res = dict(files=a.files, seconds=a.seconds, channels=C, rate=RATE, runs=a.runs, geometry=list(geom), steps=a.files * T,
               transforms=transforms, delays_recovered=round(right, 4),
               wall_upload_ms=round(upload[1], 3), upload_gb_per_s=round(2 * int(in_off[-1]) / (1e6 * upload[1]), 2),
               bf_gcc_ms=round(med['bf_gcc'], 3), bf_gcc_ms_spread=spread(ms['bf_gcc'][1:]),
               bf_track_ms=round(med['bf_track'], 3), bf_track_ms_spread=spread(ms['bf_track'][1:]),
               bf_sum_ms=round(med['bf_sum'], 3), bf_sum_ms_spread=spread(ms['bf_sum'][1:]),
               fraction_of_upload=round(all_ms / upload[1], 3),
               transform_flops=flops, transform_tflops=round(flops / (1e9 * med['bf_gcc']), 2),
               transform_flops_per_audio_hour=int(flops / hours),
               sum_bytes_read_plus_written=sum_bytes, sum_gb_per_s=round(sum_bytes / (1e6 * med['bf_sum']), 1),
               sum_bytes_per_audio_hour=int(sum_bytes / hours),
               ms_per_audio_hour={k: round(v / hours, 3) for k, v in med.items()})
    line = json.dumps(res)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
