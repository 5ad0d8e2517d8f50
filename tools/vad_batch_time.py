#!/usr/bin/env python
"""Times spkd_vad_viterbi_batch against a loop of host spkd_vad_viterbi calls on the same random
scores: one warm-up, the median of --runs runs, per-kernel milliseconds from
spkd_last_kernel_ms, the device memory of the back-pointer records, and the batch call at smaller
file counts for the break-even point.

  python tools/vad_batch_time.py [--files 64] [--frames 450000] [--runs 5]"""
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

# the decoder constants of the shipped model's word loop (transition scale 2, LM scale 10, penalty 1)
STAY = 2.0 * np.log([0.993663, 0.999217])
EXIT = 2.0 * np.log([0.00633736, 0.001])
ENTER = 10.0 * np.log(10.0) * np.array([-1.0, -1.0]) - 1.0


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
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--frames', type=int, default=450000)
    ap.add_argument('--runs', type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(5)
    scores = (-3.0 + 5.0 * rng.standard_normal((a.files * a.frames, 2))).astype(np.float32)
    ctx = hipabi.Context(0)
    d = ctx.dev_alloc(scores.nbytes)
    ctx.h2d(d, scores)
    res = dict(files=a.files, frames=a.frames, runs=a.runs)
    kern = {}

    def batch(n):
        off = np.arange(n + 1, dtype=np.int64) * a.frames
        r = ctx.vad_viterbi_batch(d, off, 2, [0, 1], STAY, EXIT, ENTER)
        for k in ('vad_viterbi', 'vad_backtrack'):
            kern.setdefault((n, k), []).append(ctx.last_ms(k))
        return r

    def host(n):
        return [hipabi.vad_viterbi(scores[i * a.frames:(i + 1) * a.frames], [0, 1], STAY, EXIT, ENTER) for i in range(n)]

    n = a.files
    while n >= 1:
        row = dict(batch_ms=median_ms(lambda: batch(n), a.runs), host_loop_ms=median_ms(lambda: host(n), a.runs))
        for k in ('vad_viterbi', 'vad_backtrack'):
            row[k + '_ms'] = float(np.median(kern[(n, k)][1:]))
        res['n=%d' % n] = row
        n //= 2
    tok_off, frames, words, sc = batch(a.files)
    h = host(a.files)
    same = all(np.array_equal(frames[tok_off[i]:tok_off[i + 1]], h[i][0]) and sc[i] == h[i][2] for i in range(a.files))
    tile = hipabi.VAD_TILE
    res.update(tokens=int(tok_off[-1]), identical_to_host=bool(same),
               back_pointer_bytes=int(a.files * ((a.frames + tile - 1) // tile * tile) * 2))
    ctx.dev_free(d)
    ctx.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
