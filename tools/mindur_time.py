#!/usr/bin/env python
"""Times spkd_mindur_viterbi_batch beside spkd_vad_viterbi_batch (stay = exit = 0, enter = -penalty: the
speaker loop resegmentation decodes) on the same random scores, in the same run (the
section on the minimum-duration decoder): one warm-up, the median of --runs runs, wall milliseconds
of the call and per-kernel milliseconds from spkd_last_kernel_ms, for each --min-frames value (below
and above 64 frames the kernel reads g from LDS or from its global scratch).  One JSON line.

  python tools/mindur_time.py [--seqs 512] [--frames 3000] [--cols 4] [--min-frames 16,125] [--runs 5] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hipabi = importlib.import_module('speaker-diarization_amd.hipabi')


def median_ms(fn, runs):
    fn()
    out = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seqs', type=int, default=512)
    ap.add_argument('--frames', type=int, default=3000)
    ap.add_argument('--cols', type=int, default=4)
    ap.add_argument('--min-frames', default='16,125')
    ap.add_argument('--penalty', type=float, default=50.0)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(5)
    # speakers that hold the floor for a few hundred frames, like resegmentation's scores
    who = np.repeat(rng.integers(0, a.cols, a.seqs * a.frames // 250 + 1), 250)[:a.seqs * a.frames]
    scores = rng.normal(-60.0, 4.0, (a.seqs * a.frames, a.cols))
    scores[np.arange(len(who)), who] += 6.0
    scores = scores.astype(np.float32)
    ctx = hipabi.Context(0)
    d = ctx.dev_alloc(scores.nbytes)
    ctx.h2d(d, scores)
    off = np.arange(a.seqs + 1, dtype=np.int64) * a.frames
    zero = np.zeros(a.cols)
    res = dict(seqs=a.seqs, frames=a.frames, cols=a.cols, penalty=a.penalty, runs=a.runs)
    kern = {}

    def plain():
        r = ctx.vad_viterbi_batch(d, off, a.cols, np.arange(a.cols), zero, zero, zero - a.penalty)
        for k in ('vad_viterbi', 'vad_backtrack'):
            kern.setdefault(k, []).append(ctx.last_ms(k))
        return r

    def mindur(D):
        r = ctx.mindur_viterbi_batch(d, off, a.cols, a.penalty, D)
        for k in ('mindur_viterbi', 'mindur_backtrack'):
            kern.setdefault((D, k), []).append(ctx.last_ms(k))
        return r

    row = dict(call_ms=median_ms(plain, a.runs))
    for k in ('vad_viterbi', 'vad_backtrack'):
        row[k + '_ms'] = float(np.median(kern[k][1:]))
    row['tokens'] = int(plain()[0][-1])
    res['vad_viterbi_batch'] = row
    for D in [int(v) for v in a.min_frames.split(',')]:
        row = dict(call_ms=median_ms(lambda: mindur(D), a.runs))
        for k in ('mindur_viterbi', 'mindur_backtrack'):
            row[k + '_ms'] = float(np.median(kern[(D, k)][1:]))
        row['tokens'] = int(mindur(D)[0][-1])
        res['mindur_viterbi_batch D=%d' % D] = row
    tile = hipabi.MINDUR_TILE
    res['mindur_scratch_bytes'] = int(a.seqs * ((a.frames + tile - 1) // tile * tile) * (2 + 8 + 4))
    ctx.dev_free(d)
    ctx.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
