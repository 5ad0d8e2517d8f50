#!/usr/bin/env python
"""Times feature warping (spkd_feature_warp) and the chain it joins (pipeline.link_batch with LINK_CLR_WARP) on
bench.py's synthetic batch (--files x --seconds): the segments are the generator's truth turns and a file's
labels its truth speakers; a file's speech is all its turns, so every frame of the batch is warped.  Reported:
  feature_warp_ms      the kernel's time (the `feature_warp` timer: HIP events around the one launch), median and
                       spread over --runs calls after a warm-up, with frames/s and the lane operations per second
                       of the count 39 x n x 4 a frame (n = min(window, frames of the file): a compare-and-add for
                       `<` and for `==` per window entry; a count from the shapes, not a measurement),
  --also LIB           the same for another build of the library (make variant NAME=plain FLAGS=-DSPKD_WARP_R=1:
                       the plain count loop, a frame a lane), the two builds called in turn in the one process,
                       after a check that they give the same bits,
  link_*_ms            the kernel times of the chain's stages from the same run: link_warp, link_ubm_train,
                       link_ubm_stats, link_clr, and the wall time of the whole link_batch.
Needs 2 x frames x 156 bytes of device memory (the frames and their warped copy).  Prints one JSON line and, with
--out, writes it there.  Run it under `timeout`."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = 'speaker-diarization_amd'


def other_build(hipabi, path, stream):
    """A context of another build of the library on the same stream."""
    ctx = hipabi.Context.__new__(hipabi.Context)
    ctx.lib = hipabi.load_library(path)
    h = C.c_void_p()
    st = ctx.lib.spkd_create_on_stream(0, C.c_void_p(int(stream)), C.byref(h))
    if st != hipabi.SPKD_OK:
        raise hipabi.SpkdError(st, 'spkd_create_on_stream failed for %s' % path)
    ctx.h = h
    return ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=256)
    ap.add_argument('--seconds', type=float, default=3600.0)
    ap.add_argument('--speakers', type=int, default=4)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--window', type=int, default=375)
    ap.add_argument('--also', default=None, help='another build of libspkd_hip.so to time in turn with the product')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    hipabi = importlib.import_module(PKG + '.hipabi')
    pipeline = importlib.import_module(PKG + '.pipeline')
    linking = importlib.import_module(PKG + '.linking')
    synth_device = importlib.import_module(PKG + '.synth_device')
    dev = torch.device('cuda', 0)
    rate = 125.0
    parts, begins, ends, labels, off, file_frames = [], [], [], [], 0, []
    for i in range(args.files):
        feats, _, truth = synth_device.make_session_device(1000003 + i, args.seconds, args.speakers, device=dev)
        begins += [off + a for a, _, _ in truth]
        ends += [off + b for _, b, _ in truth]
        labels.append(np.array([k + 1 for _, _, k in truth], dtype=np.int32))
        parts.append(feats)
        file_frames.append((off, int(feats.shape[0])))
        off += int(feats.shape[0])
    frames = torch.cat(parts)
    del parts
    total = int(frames.shape[0])
    out_a = torch.full_like(frames, -1.0)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    b, e = np.array(begins, dtype=np.int64), np.array(ends, dtype=np.int64)
    seg_off = np.concatenate([[0], np.cumsum([len(l) for l in labels])]).astype(np.int64)
    set_off, run_b, run_e = linking.speech_runs(seg_off, b, e)
    set_len = np.add.reduceat(run_e - run_b, set_off[:-1])
    warped = int(set_len.sum())
    lane_ops = int((set_len * np.minimum(set_len, args.window)).sum()) * hipabi.DIM * 4
    builds = [('product', hipabi.Context(0, stream))]
    if args.also:
        builds.append((os.path.basename(args.also), other_build(hipabi, args.also, stream)))
    # warm-up, and the builds agree to the bit before they are compared
    first = None
    for name, ctx in builds:
        ctx.feature_warp(frames.data_ptr(), total, set_off, run_b, run_e, args.window, out_a.data_ptr())
        torch.cuda.synchronize()
        got = out_a.view(torch.int32)
        digest = (int(got.sum(dtype=torch.int64).item()), int((got >> 7).sum(dtype=torch.int64).item()))
        first = first or digest
        assert digest == first, 'the builds disagree: %r, %r' % (first, digest)
        out_a.fill_(-1.0)
    ms = {name: [] for name, _ in builds}
    for _ in range(args.runs):
        for name, ctx in builds:
            ctx.feature_warp(frames.data_ptr(), total, set_off, run_b, run_e, args.window, out_a.data_ptr())
            ms[name].append(ctx.last_ms('feature_warp'))
    del out_a
    torch.cuda.empty_cache()
    med = lambda xs: round(float(np.median(xs)), 3)
    spread = lambda xs: [round(float(min(xs)), 3), round(float(max(xs)), 3)]
    out = {'files': args.files, 'seconds': args.seconds, 'speakers': args.speakers, 'frames': total, 'frames_warped': warped,
           'runs_of_speech': int(len(run_b)), 'window': args.window, 'runs': args.runs, 'lane_ops': lane_ops,
           'lane_ops_counted_as': '39 dimensions x n window entries x 4 (compare and add for <, compare and add for ==) a frame',
           'tile': hipabi.WARP_TILE, 'device': torch.cuda.get_device_name(0), 'kernel': {}}
    for name, _ in builds:
        t = med(ms[name])
        out['kernel'][name] = {'feature_warp_ms': t, 'feature_warp_min_max_ms': spread(ms[name]),
                               'frames_per_s': round(warped / (t * 1e-3)), 'lane_ops_per_s': round(lane_ops / (t * 1e-3))}
    # the chain it joins, with the product build
    ctx = builds[0][1]
    files = [pipeline.BatchFile(o, n, []) for o, n in file_frames]
    segments = [np.column_stack([(b[lo:hi] - o + 0.25) / rate, (e[lo:hi] - o + 0.25) / rate])
                for (o, _), lo, hi in zip(file_frames, seg_off[:-1], seg_off[1:])]
    link = dict(pipeline.LINK_CLR_WARP, warp_s=args.window / rate)
    keys = ('link_warp', 'link_ubm_train', 'link_ubm_stats', 'link_clr')
    chain = []
    for i in range(3):
        tm = {}
        t0 = time.perf_counter()
        maps, merges, smax, smin = pipeline.link_batch(ctx, 0, seg_off, labels, link, tm, frames.data_ptr(), total, files,
                                                       segments, rate)
        if i:
            chain.append([1e3 * (time.perf_counter() - t0)] + [tm[k][0] for k in keys])
    out['chain'] = dict({k + '_ms': med([c[1 + j] for c in chain]) for j, k in enumerate(keys)},
                        link_batch_wall_ms=med([c[0] for c in chain]), chain_runs=len(chain), speakers=tm['link_speakers'],
                        merges=len(merges), initial_ratio_max=smax, initial_ratio_min=smin)
    kernels = sum(out['chain'][k + '_ms'] for k in keys)
    out['chain']['link_warp_share_of_kernels'] = round(out['chain']['link_warp_ms'] / kernels, 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
    for _, c in builds:
        c.close()


if __name__ == '__main__':
    main()
