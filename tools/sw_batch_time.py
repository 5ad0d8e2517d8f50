#!/usr/bin/env python
"""Times sliding-window change detection over a whole batch: on bench.py's synthetic batch
(--files x --seconds, the script's defaults -m sw -d GLR -w 5.0 -st 0.5) the median and spread
over --runs, after --warmup, of
  (a) one sw_batch call: distances in bounded tiles and the positive-run pass on the device,
  (b) the same work file by file: one sw call per file, all distances back to the host, and
      ChangeDetectionRun._sw_postpass over them in Python.
The two are alternated run by run, and must write the same lines before they are compared.
Wall times around the calls, which return with their device work finished, and the kernel timer
of (a).  Prints one JSON line.  Run it under `timeout`."""
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


class _Lines(object):
    def __init__(self):
        self.lines = []

    def write(self, recline, start_frames, end_frames, lna_start, speaker):
        self.lines.append((float(start_frames), float(end_frames)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=256)
    ap.add_argument('--seconds', type=float, default=3600.0)
    ap.add_argument('--speakers', type=int, default=4)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--tile', type=int, default=0, help='windows per tile (0: the library default)')
    args = ap.parse_args()
    import torch
    hipabi = importlib.import_module(PKG + '.hipabi')
    pipeline = importlib.import_module(PKG + '.pipeline')
    cd_mod = importlib.import_module(PKG + '.change_detection')
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
    cd = pipeline.SW_CD
    owner, _, _, ls, le, tb, te = pipeline._turn_table(files, 125.0)
    p = pipeline._cd_params(cd, 125.0)
    bounds = np.searchsorted(owner, np.arange(len(files) + 1))
    opts = cd_mod.CDOptions(rate=125.0, method='sw', distance=cd['kind'], winsize_s=cd['winsize_s'],
                            winstep_s=cd['winstep_s'], threshold=cd['threshold'], lambdac=cd['lambdac'])

    def batch():
        t0 = time.perf_counter()
        r = ctx.sw_batch(ptr, total, tb, te, p, tile_windows=args.tile)
        return time.perf_counter() - t0, ctx.last_ms('sw'), r

    def serial():
        t0 = time.perf_counter()
        run = cd_mod.ChangeDetectionRun(None, opts, '')
        out = []
        for f in range(len(files)):
            lo, hi = int(bounds[f]), int(bounds[f + 1])
            st, d_off, d = ctx.sw(ptr, total, tb[lo:hi], te[lo:hi], p)
            for t in range(lo, hi):
                w = _Lines()
                run._sw_postpass(('x', 'a_1', float(ls[t]), float(le[t])), int(te[t] - tb[t]),
                                 d[int(d_off[t - lo]):int(d_off[t - lo + 1])], w)
                out.append(w.lines)
        return time.perf_counter() - t0, out, run

    for _ in range(max(args.warmup, 1)):
        rb = batch()[2]
        _, lines, run = serial()
    # the two forms agree before they are compared
    assert rb['status'] == hipabi.SPKD_OK
    for t, want in enumerate(lines):
        o, nd = int(rb['off'][t]), int(rb['n_det'][t])
        s = rb['det_start'][o:o + nd]
        assert list(zip(s.tolist(), (s + rb['det_maxi'][o:o + nd]).tolist())) == want[:-1], t
        assert float(rb['final_start'][t]) == want[-1][0], t
    assert int(rb['win_cnt'].sum()) == run.total_windows and int(rb['n_det'].sum()) == run.total_segments
    assert max(0.0, float(rb['win_max'].max())) == float(run.max_dist)
    a, b = [], []
    for _ in range(args.runs):
        a.append(batch()[:2])
        b.append(serial()[0])
    ms = lambda xs: round(1e3 * float(np.median(xs)), 3)
    spread = lambda xs: [round(1e3 * float(min(xs)), 3), round(1e3 * float(max(xs)), 3)]
    out = {
        'files': args.files, 'seconds': args.seconds, 'turns': int(len(tb)), 'windows': int(rb['d_off'][-1]),
        'detections': int(rb['n_det'].sum()), 'runs': args.runs, 'tile_windows': args.tile or 4096,
        'a_batch_call_ms': ms([x[0] for x in a]), 'a_min_max_ms': spread([x[0] for x in a]),
        'a_sw_kernels_ms': round(float(np.median([x[1] for x in a])), 3),
        'b_per_file_calls_and_host_pass_ms': ms(b), 'b_min_max_ms': spread(b),
        'device': torch.cuda.get_device_name(0),
    }
    print(json.dumps(out))
    ctx.close()


if __name__ == '__main__':
    main()
