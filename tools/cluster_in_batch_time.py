#!/usr/bin/env python
"""Times spk_cluster_in over a whole batch: on bench.py's synthetic batch (--files x --seconds,
DIA2 change detection, fused records) the median over --runs, after --warmup, of
  (a) one cluster_in_batch call (BIC, lambda 1.3, threshold 0): every file's chain in one launch,
  (b) one cluster_in call per file on the same records, one after the other (with its spread),
  (c) the agglomerative clustering call (spkd_ahc) of the same step, for context.
Wall times around the calls, which return with their device work finished, and the kernel timers
of (a) and (c).  Prints one JSON line.  Run it under `timeout`."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = 'speaker-diarization_amd'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=256)
    ap.add_argument('--seconds', type=float, default=3600.0)
    ap.add_argument('--speakers', type=int, default=4)
    ap.add_argument('--runs', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    import torch
    hipabi = importlib.import_module(PKG + '.hipabi')
    pipeline = importlib.import_module(PKG + '.pipeline')
    synth_device = importlib.import_module(PKG + '.synth_device')
    rec = importlib.import_module(PKG + '.recipe')
    dev = torch.device('cuda', 0)
    parts, files, off = [], [], 0
    for i in range(args.files):
        feats, vad, _ = synth_device.make_session_device(1000003 + i, args.seconds, args.speakers, device=dev)
        v = [(float(rec.py2_float_str(s / 125.0)), float(rec.py2_float_str(e / 125.0))) for (s, e) in vad]
        files.append(pipeline.BatchFile(off, feats.shape[0], v))
        parts.append(feats)
        off += int(feats.shape[0])
    frames = torch.cat(parts)
    del parts
    torch.cuda.synchronize()
    ctx = hipabi.Context(0, torch.cuda.current_stream().cuda_stream)
    ptr, total = frames.data_ptr(), int(frames.shape[0])
    box = []
    segs = pipeline.change_detect_batch(ctx, ptr, total, files, fused=box)
    d_stats, seg_off, n, _ = pipeline.segment_stats(ctx, ptr, total, files, segs, fused=box[0])
    cl = pipeline.DIA2_CL
    ahc_p = hipabi.AhcParams(cl['variant'], hipabi.KINDS[cl['kind']], cl['max_spk'], 0, cl['lambdac'], cl['threshold'])
    P = len(seg_off) - 1

    def batch():
        t0 = time.perf_counter()
        r = ctx.cluster_in_batch(d_stats, seg_off, 'BIC', cl['lambdac'], 0.0)
        return time.perf_counter() - t0, ctx.last_ms('ahc'), ctx.last_ms('cluster_prep'), r

    def serial():
        t0 = time.perf_counter()
        labels = []
        for p in range(P):
            o, m = int(seg_off[p]), int(seg_off[p + 1] - seg_off[p])
            labels.append(ctx.cluster_in(d_stats + o * hipabi.REC * 8, m, 'BIC', cl['lambdac'], 0.0)[0])
        return time.perf_counter() - t0, labels

    def ahc():
        t0 = time.perf_counter()
        ctx.ahc(d_stats, seg_off, ahc_p)
        return time.perf_counter() - t0, ctx.last_ms('ahc'), ctx.last_ms('matrix'), ctx.last_ms('cluster_prep')

    for _ in range(args.warmup):
        rb = batch()[3]
        ls = serial()[1]
        ahc()
    # the two forms agree before they are compared
    assert rb['status'] == hipabi.SPKD_OK
    assert all(np.array_equal(rb['label'][int(seg_off[p]):int(seg_off[p + 1])], ls[p]) for p in range(P))
    a = [batch()[:3] for _ in range(args.runs)]
    b = [serial()[0] for _ in range(args.runs)]
    c = [ahc() for _ in range(args.runs)]
    ms = lambda xs: round(1e3 * float(np.median(xs)), 3)
    med = lambda xs: round(float(np.median(xs)), 3)
    npb = np.diff(seg_off)
    pairs = sum(int((np.maximum.accumulate(rb['label'][int(o):int(e) - 1]).astype(np.int64) + 1).sum())
                for o, e in zip(seg_off[:-1], seg_off[1:]) if e - o > 1)
    out = {
        'files': args.files, 'seconds': args.seconds, 'records': int(n), 'runs': args.runs,
        'records_per_file': [int(npb.min()), float(npb.mean()), int(npb.max())],
        'clusters_per_file': [int(rb['n_clusters'].min()), float(rb['n_clusters'].mean()), int(rb['n_clusters'].max())],
        'cluster_in_pairs': pairs,
        'a_batch_call_ms': ms([x[0] for x in a]), 'a_chain_kernel_ms': med([x[1] for x in a]),
        'a_prep_kernel_ms': med([x[2] for x in a]),
        'b_serial_calls_ms': ms(b), 'b_min_ms': round(1e3 * min(b), 3), 'b_max_ms': round(1e3 * max(b), 3),
        'c_ahc_call_ms': ms([x[0] for x in c]), 'c_ahc_kernel_ms': med([x[1] for x in c]),
        'c_matrix_kernel_ms': med([x[2] for x in c]), 'c_prep_kernel_ms': med([x[3] for x in c]),
        'device': torch.cuda.get_device_name(0),
    }
    print(json.dumps(out))
    ctx.close()


if __name__ == '__main__':
    main()
