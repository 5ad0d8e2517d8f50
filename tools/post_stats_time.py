#!/usr/bin/env python
"""Times spkd_post_stats beside spkd_set_stats over the same frames, in the same process (the
section on soft resegmentation): --seqs sequences of --frames frames, each a file of its own with --cols
speakers.  For each --cols value one warm-up and the median of --runs runs of the kernel milliseconds from
spkd_last_kernel_ms: set_stats (chunk_stats + reduce_sets, one set per sequence: every frame once) and
post_stats on dense posteriors (no weight is 0: n_cols times set_stats' FMAs) and on peaked ones (one-hot in
stretches of 250 frames, as a decoder at acoustic scale 1 leaves them: the zero weights are passed over).
ratio = post_stats / set_stats on the dense weights; the expectation is at most n_cols * 1.25.  Then the
whole RESEG_SOFT stage at passes=8 on the two-file fixture of tests/test_reseg_soft.py, per pass, from
resegment_batch's timings.  One JSON line.

  python tools/post_stats_time.py [--seqs 512] [--frames 3000] [--cols 4,16] [--runs 5] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = 'speaker-diarization_amd'
hipabi = importlib.import_module(PKG + '.hipabi')
RATE = 125.0


def kernel_ms(fn, timers, ctx, runs):
    fn()
    out = []
    for _ in range(runs):
        fn()
        out.append(sum(ctx.last_ms(t) for t in timers))
    return float(np.median(out))


def kernels(a):
    res = {}
    ctx = hipabi.Context(0)
    n = a.seqs * a.frames
    rng = np.random.default_rng(11)
    frames = rng.normal(0.0, 3.0, (n, hipabi.DIM)).astype(np.float32)
    d_frames = ctx.dev_alloc(frames.nbytes)
    ctx.h2d(d_frames, frames)
    begin = np.arange(a.seqs, dtype=np.int64) * a.frames
    end = begin + a.frames
    d_sets = ctx.dev_alloc(a.seqs * hipabi.REC * 8)
    hard = kernel_ms(lambda: ctx.set_stats(d_frames, n, begin, end, np.arange(a.seqs, dtype=np.int32), a.seqs, d_sets),
                     ('chunk_stats', 'reduce_sets'), ctx, a.runs)
    ctx.dev_free(d_sets)
    for cols in [int(v) for v in a.cols.split(',')]:
        dense = rng.random((n, cols), dtype=np.float32) + np.float32(0.01)
        dense /= dense.sum(axis=1, keepdims=True)
        who = np.repeat(rng.integers(0, cols, n // 250 + 1), 250)[:n]
        peaked = np.zeros((n, cols), dtype=np.float32)
        peaked[np.arange(n), who] = 1.0
        n_models = a.seqs * cols
        d_post, d_stats = ctx.dev_alloc(dense.nbytes), ctx.dev_alloc(n_models * hipabi.REC * 8)
        first = np.arange(a.seqs, dtype=np.int32) * cols
        count = np.full(a.seqs, cols, dtype=np.int32)
        row = dict(set_stats_ms=hard, workgroups=int(a.seqs * ((a.frames + hipabi.POST_CHUNK - 1) // hipabi.POST_CHUNK) * cols))
        row['partial_bytes'] = row['workgroups'] * hipabi.REC * 8
        for name, post in (('dense', dense), ('peaked', peaked)):
            ctx.h2d(d_post, post)
            row[name + '_post_stats_ms'] = kernel_ms(
                lambda: ctx.post_stats(d_frames, n, d_post, begin, end, first, count, cols, n_models, d_stats, masses=False),
                ('post_stats',), ctx, a.runs)
        row['ratio'] = row['dense_post_stats_ms'] / hard
        row['expected_at_most'] = 1.25 * cols
        row['peaked_ratio'] = row['peaked_post_stats_ms'] / hard
        ctx.dev_free(d_post)
        ctx.dev_free(d_stats)
        res['cols=%d' % cols] = row
    ctx.dev_free(d_frames)
    ctx.close()
    return res


def close_session(synth, seed, seconds, n_speakers, eps):
    base = [synth._speaker_model(seed, k) for k in range(n_speakers)]
    models = [(base[0][0] + eps * (m[0] - base[0][0]), base[0][1]) for m in base]
    return synth.make_session(seed, seconds, n_speakers, models=models)


def displaced(truth, vad, shift):
    segs = []
    for a, b in vad:
        inside = [t for t in truth if a <= t[0] and t[1] <= b]
        for k, (s, e, spk) in enumerate(inside):
            segs.append((s if k == 0 else s + shift, e if k == len(inside) - 1 else e + shift, spk))
    return segs


def stage():
    """RESEG_SOFT at passes=8 on the two fixtures of tests/test_reseg_soft.py as one batch, run twice: the
    timings of the second run."""
    synth, engine, pipeline = [importlib.import_module(PKG + '.' + m) for m in ('synth', 'engine', 'pipeline')]
    sess = [close_session(synth, 7002, 40.0, 2, 0.10), close_session(synth, 7006, 40.0, 3, 0.15)]
    segs = [displaced(s[2], s[1], 300) for s in sess]
    frames = np.ascontiguousarray(np.concatenate([s[0] for s in sess]), dtype=np.float32)
    eng = engine.HipEngine(0)
    eng.set_features(frames)
    foff = np.concatenate([[0], np.cumsum([len(s[0]) for s in sess])])
    files = [pipeline.BatchFile(foff[i], len(s[0]), [(a / RATE, b / RATE) for a, b in s[1]]) for i, s in enumerate(sess)]
    seg_off = np.concatenate([[0], np.cumsum([len(g) for g in segs])]).astype(np.int64)
    labels = [np.array([k + 1 for _, _, k in g], dtype=np.int32) for g in segs]
    d_stats = eng._stats_of_sets([[(int(foff[i] + a), int(foff[i] + b))] for i, g in enumerate(segs) for a, b, _ in g])
    out = {}
    for _ in range(2):
        timings, det = {}, {}
        pipeline.resegment_batch(eng.ctx, eng.d_frames, len(frames), files, d_stats, seg_off, labels, RATE,
                                 dict(pipeline.RESEG_SOFT, passes=8), False, timings, det)
        out = dict(passes_run=det['passes_run'], kernel_ms_per_pass=timings,
                   soft_mass=[m.tolist() for m in det['soft_mass']])
    eng.ctx.dev_free(d_stats)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seqs', type=int, default=512)
    ap.add_argument('--frames', type=int, default=3000)
    ap.add_argument('--cols', default='4,16')
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = dict(seqs=a.seqs, frames=a.frames, runs=a.runs, chunk=hipabi.POST_CHUNK)
    res.update(kernels(a))
    res['reseg_soft_stage'] = stage()
    line = json.dumps(res)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
