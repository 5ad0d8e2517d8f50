#!/usr/bin/env python
"""Times the linking of a batch's speakers (pipeline.link_batch) on bench.py's synthetic batch
(--files x --seconds): the segments are the generator's truth turns and a file's labels its
truth speakers, so the batch has --files x --speakers initial speakers.  Reported:
  (a) link_sum: the records of all speakers as sums of their segments' records (spkd_sum_stats,
      kernel time) and the GB/s of its members x 6 560 B read + sets x 6 560 B written,
  (b) the only route to the same records without it: spkd_set_stats with one multi-range set per
      speaker from the resident frames (kernel times of its two passes), every frame read again,
  (c) link_ahc: the one clustering problem over all speakers (the whole call), with its speakers
      and merges.
Medians and spreads over --runs after a warm-up of each; (a) and (b) must give the same records
(1e-12 relative: the order of the sums differs) before they are compared.  Wall times are around
calls that return with their device work finished.  Prints one JSON line.  Run it under
`timeout`.
--clr times linking by cross-likelihood ratio instead (pipeline.link_batch with LINK_CLR) on the same
batch: the kernel times of its three calls -- link_ubm_train (spkd_gmm_train on at most ubm_max_frames
frames), link_ubm_stats (spkd_ubm_stats over every frame of every speaker, with the GB/s of 156 B a
frame) and link_clr (spkd_clr_link) -- and the wall time of the whole link_batch, and writes the JSON
line into DESIGN.md in place of the "Numbers:" line of its section on the mode."""
import argparse
import importlib
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = 'speaker-diarization_amd'


NUMBERS = re.compile(r'^Numbers \(link by CLR\):.*$', flags=re.M)


def clr_mode(args, ctx, pipeline, ptr, total, file_frames, b, e, seg_off, labels, device):
    rate = 125.0
    files = [pipeline.BatchFile(o, n, []) for o, n in file_frames]
    # a quarter of a frame past each bound: the frame ranges link_batch cuts are the truth's
    segments = [np.column_stack([(b[lo:hi] - o + 0.25) / rate, (e[lo:hi] - o + 0.25) / rate])
                for (o, _), lo, hi in zip(file_frames, seg_off[:-1], seg_off[1:])]
    runs = []
    for i in range(args.runs + 1):
        tm = {}
        t0 = time.perf_counter()
        maps, merges, smax, smin = pipeline.link_batch(ctx, 0, seg_off, labels, pipeline.LINK_CLR, tm, ptr, total, files,
                                                       segments, rate)
        if i:
            runs.append((1e3 * (time.perf_counter() - t0), tm['link_ubm_train'][0], tm['link_ubm_stats'][0], tm['link_clr'][0]))
    med = lambda k: round(float(np.median([r[k] for r in runs])), 3)
    spread = lambda k: [round(float(min(r[k] for r in runs)), 3), round(float(max(r[k] for r in runs)), 3)]
    frames = int((e - b).sum())
    out = {
        'mode': 'clr', 'files': args.files, 'seconds': args.seconds, 'speakers': tm['link_speakers'], 'merges': len(merges),
        'frames_of_speakers': frames, 'runs': args.runs, 'link': pipeline.LINK_CLR,
        'link_ubm_train_ms': med(1), 'link_ubm_train_min_max_ms': spread(1),
        'link_ubm_stats_ms': med(2), 'link_ubm_stats_min_max_ms': spread(2),
        'link_clr_ms': med(3), 'link_clr_min_max_ms': spread(3),
        'link_batch_wall_ms': med(0), 'initial_ratio_max': smax, 'initial_ratio_min': smin,
        'global_speakers': int(max(int(m.max()) for m in maps)), 'device': device,
    }
    out['link_ubm_stats_gb_s'] = round(frames * 156 / (out['link_ubm_stats_ms'] * 1e-3) / 1e9, 1)
    line = json.dumps(out)
    print(line)
    path = os.path.join(ROOT, 'DESIGN.md')
    text = open(path).read()
    if NUMBERS.search(text):
        open(path, 'w').write(NUMBERS.sub(lambda m: 'Numbers (link by CLR): tools/link_time.py --clr measured ' + line, text, count=1))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=256)
    ap.add_argument('--seconds', type=float, default=3600.0)
    ap.add_argument('--speakers', type=int, default=4)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--ahc-runs', type=int, default=3)
    ap.add_argument('--clr', action='store_true')
    args = ap.parse_args()
    import torch
    hipabi = importlib.import_module(PKG + '.hipabi')
    pipeline = importlib.import_module(PKG + '.pipeline')
    synth_device = importlib.import_module(PKG + '.synth_device')
    dev = torch.device('cuda', 0)
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
    torch.cuda.synchronize()
    ctx = hipabi.Context(0, torch.cuda.current_stream().cuda_stream)
    ptr, total = frames.data_ptr(), int(frames.shape[0])
    b, e = np.array(begins, dtype=np.int64), np.array(ends, dtype=np.int64)
    n_seg = len(b)
    seg_off = np.concatenate([[0], np.cumsum([len(l) for l in labels])]).astype(np.int64)
    if args.clr:
        return clr_mode(args, ctx, pipeline, ptr, total, file_frames, b, e, seg_off, labels,
                        torch.cuda.get_device_name(0))
    # what cluster_batch leaves: one record per segment, in segment order
    d_stats = ctx.dev_alloc(n_seg * hipabi.REC * 8)
    ctx.set_stats(ptr, total, b, e, np.arange(n_seg, dtype=np.int32), n_seg, d_stats)
    member, set_off, _, _ = pipeline.link_speakers(seg_off, labels)
    n_spk = len(set_off) - 1
    d_a = ctx.dev_alloc(n_spk * hipabi.REC * 8)
    d_b = ctx.dev_alloc(n_spk * hipabi.REC * 8)
    owner = np.repeat(np.arange(n_spk, dtype=np.int32), np.diff(set_off))

    def sum_records():
        t0 = time.perf_counter()
        ctx.sum_stats(d_stats, n_seg, member, set_off, d_a)
        return time.perf_counter() - t0, ctx.last_ms('reduce_sets')

    def from_frames():
        t0 = time.perf_counter()
        ctx.set_stats(ptr, total, b[member], e[member], owner, n_spk, d_b)
        return time.perf_counter() - t0, ctx.last_ms('chunk_stats') + ctx.last_ms('reduce_sets')

    sum_records()
    from_frames()
    ra, rb = np.empty((n_spk, hipabi.REC)), np.empty((n_spk, hipabi.REC))
    ctx.d2h(ra, d_a)
    ctx.d2h(rb, d_b)
    worst = float(np.max(np.abs(ra - rb) / np.maximum(1.0, np.abs(rb))))
    assert worst < 1e-12, worst
    sa, sb = [], []
    for _ in range(args.runs):
        sa.append(sum_records())
        sb.append(from_frames())
    ahc = []
    for i in range(args.ahc_runs + 1):
        tm = {}
        t0 = time.perf_counter()
        maps, merges, _, _ = pipeline.link_batch(ctx, d_stats, seg_off, labels, timings=tm)
        if i:
            ahc.append((time.perf_counter() - t0, tm['link_ahc'][0], tm['link_sum'][0]))
    med = lambda xs: round(float(np.median(xs)), 3)
    spread = lambda xs: [round(float(min(xs)), 3), round(float(max(xs)), 3)]
    nbytes = (len(member) + n_spk) * hipabi.REC * 8
    out = {
        'files': args.files, 'seconds': args.seconds, 'segments': n_seg, 'speakers': n_spk, 'members': int(len(member)),
        'frames_of_members': int((e - b).sum()), 'runs': args.runs, 'ahc_runs': args.ahc_runs,
        'link_sum_kernel_ms': med([x[1] for x in sa]), 'link_sum_kernel_min_max_ms': spread([x[1] for x in sa]),
        'link_sum_call_ms': med([1e3 * x[0] for x in sa]), 'link_sum_bytes': nbytes,
        'set_stats_kernels_ms': med([x[1] for x in sb]), 'set_stats_kernels_min_max_ms': spread([x[1] for x in sb]),
        'set_stats_call_ms': med([1e3 * x[0] for x in sb]), 'records_worst_rel_diff': worst,
        'link_ahc_call_ms': med([x[1] for x in ahc]), 'link_ahc_min_max_ms': spread([x[1] for x in ahc]),
        'link_batch_wall_ms': med([1e3 * x[0] for x in ahc]), 'link_merges': len(merges),
        'global_speakers': int(max(int(m.max()) for m in maps)), 'device': torch.cuda.get_device_name(0),
    }
    out['link_sum_gb_s'] = round(nbytes / (out['link_sum_kernel_ms'] * 1e-3) / 1e9, 1)
    out['set_stats_over_link_sum'] = round(out['set_stats_kernels_ms'] / out['link_sum_kernel_ms'], 2)
    print(json.dumps(out))
    for p in (d_stats, d_a, d_b):
        ctx.dev_free(p)
    ctx.close()


if __name__ == '__main__':
    main()
