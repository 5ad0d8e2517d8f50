#!/usr/bin/env python
"""Times the delay stream's three kernels of the resegmentation stage (spkd_tdoa_stats, spkd_tdoa_models,
spkd_tdoa_score) on a batch of --files x --seconds with --channels microphones and --speakers speakers a file, and
on one file of --long-hours.  Frames are one file of normal deviates copied to every file's place, the speakers
take turns of five seconds, a file's VAD turns are a minute long, the stream is a DelayStream.from_arrays of
seats with a sample of jitter and a tenth of the steps unreliable.  Every figure is taken after a warm-up, over
--runs calls: [min, median, max] of the kernel timers.

The expectation stated beforehand: tdoa_score moves 8 bytes per score entry (a read and a write) and little
else, so it is compared with a device-to-device copy of the same score bytes in the same process and on the same
stream, enqueued between two events as the kernel is between its timer's two (read plus written bytes);
tdoa_stats should be a small fraction of gauss_loglik on the same batch.

  python tools/tdoa_time.py [--files 64] [--seconds 600] [--long-hours 10] [--runs 5] [--out profiles/tdoa_time.json]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
hipabi = importlib.import_module('speaker-diarization_amd.hipabi')
fe = importlib.import_module('speaker-diarization_amd.frontend')
reseg = importlib.import_module('speaker-diarization_amd.resegmentation')
from mfcc_batch_time import spread               # noqa: E402

RATE, HOP, WINDOW, FRAME_RATE, H = 16000, 128, 400, 125, 4000
TURN_S, SEG_S = 60, 5


def workload(ctx, torch, n_files, seconds, channels, speakers, runs):
    T_f = seconds * FRAME_RATE                                   # frames a file
    total = n_files * T_f
    rng = np.random.default_rng(1)
    one = rng.standard_normal((T_f, hipabi.DIM)).astype(np.float32)
    d_frames = ctx.dev_scratch('time_frames', total * hipabi.DIM * 4)
    for f in range(n_files):
        ctx.h2d(d_frames + f * one.nbytes, one)
    # speakers in turns of SEG_S; one stream file, repeated
    seg = SEG_S * FRAME_RATE
    b1 = np.arange(0, T_f, seg, dtype=np.int64)
    who1 = (np.arange(len(b1)) % speakers).astype(np.int64)
    steps = (T_f * HOP - 2 * H) // H + 1
    first = np.array([fe.step_first_frame(s, HOP, WINDOW, RATE, RATE, H) for s in range(steps)])
    seats = rng.integers(-150, 151, (speakers, channels))
    delay = seats[who1[np.minimum(first // seg, len(who1) - 1)]] + rng.integers(-1, 2, (steps, channels))
    delay[:, 0] = 0
    reliable = rng.random((steps, channels)) >= 0.1
    stream = fe.DelayStream.from_arrays(ctx, HOP, WINDOW, [(delay.astype(np.int32), reliable, 0, H, RATE)] * n_files, rate_out=RATE)
    frame0 = np.arange(n_files, dtype=np.int64) * T_f
    handle = stream.handle(frame0)
    # ranges grouped by speaker (ascending sets), turns of a minute
    rb = np.concatenate([frame0[f] + b1[who1 == k] for f in range(n_files) for k in range(speakers)])
    sets = np.repeat(np.arange(n_files * speakers), [int((who1 == k).sum()) for _ in range(n_files) for k in range(speakers)])
    n_spk = n_files * speakers
    spk_file = np.repeat(np.arange(n_files), speakers)
    re_ = np.minimum(rb + seg, (spk_file[sets] + 1) * T_f)
    tb = np.concatenate([frame0[f] + np.arange(0, T_f, TURN_S * FRAME_RATE) for f in range(n_files)])
    te = np.minimum(tb + TURN_S * FRAME_RATE, np.repeat(frame0 + T_f, len(tb) // n_files))
    owner = np.repeat(np.arange(n_files), len(tb) // n_files)
    # the acoustic side, for the comparison: records, models, scores
    d_rec = ctx.dev_scratch('time_records', n_spk * hipabi.REC * 8)
    d_mod = ctx.dev_scratch('time_models', n_spk * hipabi.GAUSS_MODEL * 8)
    scores = torch.empty(total * speakers, dtype=torch.float32, device='cuda:0')     # (torch's, so that it can copy them)
    copied = torch.empty_like(scores)
    d_scores = scores.data_ptr()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    d_tstats = ctx.dev_scratch('time_tdoa_stats', n_spk * 8 * 3 * 8)
    d_tmod = ctx.dev_scratch('time_tdoa_models', n_spk * 8 * hipabi.TDOA_MODEL * 8)
    ctx.set_stats(d_frames, total, rb, re_, sets.astype(np.int32), n_spk, d_rec)
    ok = ctx.gauss_models(d_rec, n_spk, d_mod)
    ms = dict(gauss_loglik=[], tdoa_stats=[], tdoa_models=[], tdoa_score=[], copy=[])
    live = None
    for _ in range(runs + 1):                                    # the first one warms up
        ctx.gauss_loglik(d_frames, total, d_mod, ok, tb, te, owner * speakers, np.full(len(tb), speakers), speakers, d_scores)
        ms['gauss_loglik'].append(ctx.last_ms('gauss_loglik'))
        ctx.tdoa_stats(handle, rb, re_, spk_file[sets], sets, n_spk, d_tstats)
        ms['tdoa_stats'].append(ctx.last_ms('tdoa_stats'))
        live = ctx.tdoa_models(d_tstats, spk_file, ok, handle[2], reseg.TDOA['min_frames'], reseg.TDOA['floor_s'], d_tmod)
        ms['tdoa_models'].append(ctx.last_ms('tdoa_models'))
        ctx.tdoa_score(handle, d_tmod, n_spk, live, tb, te, owner, owner * speakers, np.full(len(tb), speakers), speakers,
                       reseg.TDOA['weight'], d_scores)
        ms['tdoa_score'].append(ctx.last_ms('tdoa_score'))
        e0.record()
        copied.copy_(scores)                                     # (on the context's stream, between two events)
        e1.record()
        e1.synchronize()
        ms['copy'].append(e0.elapsed_time(e1))
    moved = 8 * total * speakers
    score_med, copy_med = float(np.median(ms['tdoa_score'][1:])), float(np.median(ms['copy'][1:]))
    return dict(files=n_files, frames=total, steps_a_file=int(steps), speakers=n_spk, ranges=len(rb), turns=len(tb),
                live_channels_of_file_0=[c for c in range(8) if (int(live[0]) >> c) & 1], acoustic_ok=int(ok.sum()),
                gauss_loglik_ms=spread(ms['gauss_loglik'][1:]), tdoa_stats_ms=spread(ms['tdoa_stats'][1:]),
                tdoa_models_ms=spread(ms['tdoa_models'][1:]), tdoa_score_ms=spread(ms['tdoa_score'][1:]),
                score_bytes_read_plus_written=moved, tdoa_score_gb_per_s=round(moved / (1e6 * score_med), 1),
                device_copy_of_the_scores_ms=spread(ms['copy'][1:]), device_copy_gb_per_s=round(moved / (1e6 * copy_med), 1),
                tdoa_score_over_copy=round(score_med / copy_med, 3),
                tdoa_stats_over_gauss_loglik=round(float(np.median(ms['tdoa_stats'][1:])) / float(np.median(ms['gauss_loglik'][1:])), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--seconds', type=int, default=600)
    ap.add_argument('--channels', type=int, default=4)
    ap.add_argument('--speakers', type=int, default=4)
    ap.add_argument('--long-hours', type=float, default=10.0)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tdoa_time.json'))
    a = ap.parse_args()
    import torch                                     # (its HIP runtime has to be the first in the process)
    torch.cuda.init()
    ctx = hipabi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    res = dict(runs=a.runs, channels=a.channels, speakers_a_file=a.speakers, hop=HOP, window=WINDOW, step=H, settings=reseg.TDOA,
               tile=hipabi.TDOA_TILE)
    res['batch'] = workload(ctx, torch, a.files, a.seconds, a.channels, a.speakers, a.runs)
    print('batch: %s' % json.dumps(res['batch']), file=sys.stderr, flush=True)
    res['long_file'] = workload(ctx, torch, 1, int(a.long_hours * 3600), a.channels, a.speakers, a.runs)
    print('long file: %s' % json.dumps(res['long_file']), file=sys.stderr, flush=True)
    ctx.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
