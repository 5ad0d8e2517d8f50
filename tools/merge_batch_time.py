#!/usr/bin/env python
"""Times merge mode (`-m m`, merge_rec) over a whole batch: on bench.py's synthetic batch
(--files x --seconds) every truth turn is cut into pieces of --piece frames (the remainder stays
with the last piece), an over-segmented detector output, and the lines go through
  (a) change_detect_batch(cd=MERGE_CD ...): one spkd_merge_batch call, an ahead pass over the
      adjacent pairs and one device chain per file,
  (b) ChangeDetectionRun in merge mode, file by file on the same resident frames: one batched
      pair_terms call per file up front, then one blocking call, a D2H copy and a host decision
      for every step behind a merge -- the only path before spkd_merge_batch.
Median and spread over --runs of (a) and --serial-runs of (b), after a warm-up of each, alternated
as far as the counts allow; the two must write the same runs before they are compared.  Wall
times around calls that return with their device work finished, and the kernel timer of (a).
Prints one JSON line.  Run it under `timeout`."""
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


def pieces(truth, piece):
    out = []
    for a, b, _ in truth:
        p = a
        while b - p >= 2 * piece:
            out.append((p, p + piece))
            p += piece
        out.append((p, b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=256)
    ap.add_argument('--seconds', type=float, default=3600.0)
    ap.add_argument('--speakers', type=int, default=4)
    ap.add_argument('--piece', type=int, default=250)
    ap.add_argument('--kind', default='GLR')
    ap.add_argument('--threshold', type=float, default=2500.0)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--serial-runs', type=int, default=2)
    args = ap.parse_args()
    import torch
    hipabi = importlib.import_module(PKG + '.hipabi')
    pipeline = importlib.import_module(PKG + '.pipeline')
    cd_mod = importlib.import_module(PKG + '.change_detection')
    engine = importlib.import_module(PKG + '.engine')
    synth_device = importlib.import_module(PKG + '.synth_device')
    rec = importlib.import_module(PKG + '.recipe')
    dev = torch.device('cuda', 0)
    s2 = rec.py2_float_str
    parts, files, off = [], [], 0
    for i in range(args.files):
        feats, _, truth = synth_device.make_session_device(1000003 + i, args.seconds, args.speakers, device=dev)
        v = [(float(s2(a / 125.0)), float(s2(b / 125.0))) for (a, b) in pieces(truth, args.piece)]
        files.append(pipeline.BatchFile(off, feats.shape[0], v))
        parts.append(feats)
        off += int(feats.shape[0])
    frames = torch.cat(parts)
    del parts
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    ctx = hipabi.Context(0, stream)
    eng = engine.HipEngine(0, stream)
    ptr, total = frames.data_ptr(), int(frames.shape[0])
    cd = dict(pipeline.MERGE_CD, kind=args.kind, threshold=args.threshold)
    opts = cd_mod.CDOptions(rate=125.0, method='m', distance=cd['kind'], threshold=cd['threshold'], lambdac=cd['lambdac'])

    class Run(cd_mod.ChangeDetectionRun):
        """merge mode on a file of the resident array instead of a .fea file"""
        def _load(self, recline):
            f = files[int(recline[0])]
            self.eng.set_device_features(ptr + f.frame_off * hipabi.DIM * 4, f.n_frames)
            return f.n_frames

    def batch():
        tm = {}
        t0 = time.perf_counter()
        runs = pipeline.change_detect_batch(ctx, ptr, total, files, cd=cd, timings=tm, text_contract=False)
        return time.perf_counter() - t0, tm, runs

    def serial():
        t0 = time.perf_counter()
        out = []
        for k, f in enumerate(files):
            w = _Lines()
            Run(eng, opts, '', say=lambda *a: None).detect_changes([(str(k), 'a_%d' % (j + 1), s, e)
                                                                    for j, (s, e) in enumerate(f.vad)], w)
            out.append(w.lines)
        return time.perf_counter() - t0, out

    _, tm, runs = batch()
    _, lines = serial()
    # the two forms agree before they are compared: a run is written as (start * rate, end * rate) frames
    for k, (got, want) in enumerate(zip(runs, lines)):
        assert [(a * 125.0, b * 125.0) for a, b in np.asarray(got).tolist()] == \
            [((a / 125.0 + 0.0) * 125.0, (b / 125.0 + 0.0) * 125.0) for a, b in want], k
    a, b = [], []
    for i in range(max(args.runs, args.serial_runs)):
        if i < args.runs:
            x = batch()
            a.append((x[0], x[1]['merge'][0]))
        if i < args.serial_runs:
            b.append(serial()[0])
    ms = lambda xs: round(1e3 * float(np.median(xs)), 3)
    spread = lambda xs: [round(1e3 * float(min(xs)), 3), round(1e3 * float(max(xs)), 3)]
    out = {
        'files': args.files, 'seconds': args.seconds, 'piece_frames': args.piece, 'kind': args.kind,
        'threshold': args.threshold, 'lines': tm['merge_lines'], 'runs_written': int(sum(len(r) for r in runs)),
        'steps_behind_a_merge': tm['merge_steps_behind_a_merge'], 'runs': args.runs, 'serial_runs': args.serial_runs,
        'a_batch_call_ms': ms([x[0] for x in a]), 'a_min_max_ms': spread([x[0] for x in a]),
        'a_merge_kernels_ms': round(float(np.median([x[1] for x in a])), 3),
        'b_per_file_host_loop_ms': ms(b), 'b_min_max_ms': spread(b),
        'device': torch.cuda.get_device_name(0),
    }
    out['b_over_a'] = round(out['b_per_file_host_loop_ms'] / out['a_batch_call_ms'], 1)
    print(json.dumps(out))
    eng.close()
    ctx.close()


if __name__ == '__main__':
    main()
