#!/usr/bin/env python
"""Times the two seat kernels (spkd_tdoa_cuts, per pass of seat_cut_batch, and spkd_tdoa_split) on a batch of --files x
--seconds with four microphones, on the segments change_detect_batch leaves, and puts the stage's spkd_tdoa_stats and the
one k_ahc launch of cluster_batch on the same batch beside them, for scale.  The frames are --distinct sessions of the
synthetic generator repeated over the files; a file's stream is DelayStream.from_arrays of one seat per speaker of its
session (the speaker at a step's middle frame, of the speaker before in a pause), a sample of jitter, a tenth of the
steps unreliable on a channel.  Every figure is [min, median, max] of the kernel timers over --runs repetitions of the
whole stage after one warm-up.  No target is set: nobody has measured this stage before.

  python tools/seat_time.py [--files 256] [--seconds 3600] [--distinct 4] [--runs 5] [--out profiles/seat_time.json]"""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
PKG = 'speaker-diarization_amd'
hipabi = importlib.import_module(PKG + '.hipabi')
fe = importlib.import_module(PKG + '.frontend')
pipeline = importlib.import_module(PKG + '.pipeline')
synth_device = importlib.import_module(PKG + '.synth_device')
from mfcc_batch_time import spread               # noqa: E402

RATE, HOP, WINDOW, FRAME_RATE, H, CHANNELS = 16000, 128, 400, 125.0, 4000, 4


def seated(rng, n_frames, truth, speakers):
    """(delay int32 [T, 4], reliable bool [T, 4]) of a session: tests/test_tdoa_stream.py's scene, at any length."""
    T = (n_frames * HOP - 2 * H) // H + 1
    seats = rng.integers(-200, 201, (speakers, CHANNELS))
    mid = np.array([fe.step_first_frame(s, HOP, WINDOW, RATE, RATE, H) for s in range(T)]) + 15
    starts = np.array([t[0] for t in truth])
    who = np.array([t[2] for t in truth])[np.maximum(np.searchsorted(starts, mid, side='right') - 1, 0)]
    delay = seats[who] + rng.integers(-1, 2, (T, CHANNELS))
    delay[:, 0] = 0
    return delay.astype(np.int32), rng.random((T, CHANNELS)) >= 0.1


def commit(given):
    if given:
        return given
    try:
        head = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True).stdout.strip()
        dirty = subprocess.run(['git', '-C', ROOT, 'status', '--porcelain', '-uno'], capture_output=True, text=True).stdout.strip()
        return (head + ('+changes' if dirty else '')) or 'unknown'
    except OSError:
        return 'unknown'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=256)
    ap.add_argument('--seconds', type=float, default=3600.0)
    ap.add_argument('--distinct', type=int, default=4)
    ap.add_argument('--speakers', type=int, default=4)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--commit', default='', help='what to record as the commit where the tree has no history to ask')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'seat_time.json'))
    a = ap.parse_args()
    import torch                                     # (its HIP runtime has to be the first in the process)
    torch.cuda.init()
    ctx = hipabi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(3)
    n_distinct = max(1, min(a.distinct, a.files))
    sessions = [synth_device.make_session_device(1000003 + i, a.seconds, a.speakers, device='cuda:0') for i in range(n_distinct)]
    T = int(sessions[0][0].shape[0])
    frames = torch.cat([sessions[i % n_distinct][0] for i in range(a.files)])
    files = [pipeline.BatchFile(i * T, T, [(s / FRAME_RATE, e / FRAME_RATE) for s, e in sessions[i % n_distinct][1]]) for i in range(a.files)]
    streams = [seated(rng, T, s[2], a.speakers) for s in sessions]
    delays = fe.DelayStream.from_arrays(ctx, HOP, WINDOW, [streams[i % n_distinct] + (0, H, RATE) for i in range(a.files)], rate_out=RATE)
    del sessions
    torch.cuda.synchronize()
    total, ptr = a.files * T, frames.data_ptr()
    segments = pipeline.change_detect_batch(ctx, ptr, total, files, FRAME_RATE, pipeline.DIA2_CD)
    cuts, stats, split, ahc = [], [], [], []
    detail = {}
    for _ in range(a.runs + 1):                      # the first one warms up
        t, detail = {}, {}
        pieces = pipeline.seat_cut_batch(ctx, files, segments, delays, FRAME_RATE, pipeline.SEATS, True, t, detail)
        clusters = pipeline.cluster_batch(ctx, ptr, total, files, pieces, FRAME_RATE, pipeline.DIA2_CL, t)
        labels = pipeline.seat_split_batch(ctx, files, pieces, [lab for lab, _ in clusters], delays, FRAME_RATE, pipeline.SEATS, t, detail)
        cuts.append(t['seat_cuts']), stats.append(t['seat_stats'][0]), split.append(t['seat_split'][0]), ahc.append(t['ahc'][0])
    n_pass = min(len(c) for c in cuts[1:])
    res = dict(what='kernel milliseconds of the seat stages on the segments change detection leaves: [min, median, max] over '
                    'the runs after one warm-up; tdoa_stats of the stage and the one k_ahc launch of the same batch for scale',
               commit=commit(a.commit), runs=a.runs, files=a.files, seconds=a.seconds, distinct_sessions=n_distinct, channels=CHANNELS,
               frames=total, settings=pipeline.SEATS, segments_from_change_detection=int(sum(len(s) for s in segments)),
               pieces_after_the_cuts=int(sum(len(p) for p in pieces)), cut_passes=detail['seats']['passes_run'],
               speakers_before=int(sum(len(set(np.asarray(lab).tolist())) for lab, _ in clusters)),
               speakers_after=int(sum(len(set(np.asarray(lab).tolist())) for lab in labels)),
               unplaced_segments=int(sum(detail['seats']['unplaced'])),
               tdoa_cuts_ms_per_pass=[spread([c[k] for c in cuts[1:]]) for k in range(n_pass)],
               tdoa_cuts_ms_all_passes=spread([sum(c) for c in cuts[1:]]),
               tdoa_stats_ms=spread(stats[1:]), tdoa_split_ms=spread(split[1:]), ahc_ms=spread(ahc[1:]))
    ctx.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
