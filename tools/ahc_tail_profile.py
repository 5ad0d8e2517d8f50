#!/usr/bin/env python3
"""How long every problem of the benchmark batch keeps its CU in k_ahc, and how much of the launch is
its tail: the 256 benchmark sessions once through pipeline.diarize_batch on the profiling build (make
-C speaker-diarization_amd/csrc libspkd_hip_prof.so), where thread 0 of every k_ahc workgroup stores
the wall clock at entry and at exit.  Writes N_p and t_p of every problem, the fitted exponent of t
against N, the time from the median problem's exit to the last exit, the share of CU-time idle, and the
two constants of ahc_head_rule (spkd_hip.hip) that follow.  Development tool only.

    python tools/ahc_tail_profile.py [--files 256] [--out profiles/ahc_head.json]

SPKD_AHC_HEAD=0 in the environment gives the single launches; with a head the entries of the head's
problems lie before the others', and `launch_ms` is the span of both launches."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = 'speaker-diarization_amd'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=256)
    ap.add_argument('--seconds', type=float, default=3600.0)
    ap.add_argument('--speakers', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ahc_head.json'))
    args = ap.parse_args()
    import torch
    hipabi = importlib.import_module(PKG + '.hipabi')
    lib = hipabi.load_library(os.path.join(ROOT, PKG, 'csrc', 'libspkd_hip_prof.so'))
    hipabi._lib = lib
    sd = importlib.import_module(PKG + '.synth_device')
    pipeline = importlib.import_module(PKG + '.pipeline')
    rec = importlib.import_module(PKG + '.recipe')
    sessions = [sd.make_session_device(1000003 + i, args.seconds, args.speakers, device='cuda')[:2]
                for i in range(args.files)]                       # (bench.py's batch)
    T = int(sessions[0][0].shape[0])
    frames = torch.cat([s[0] for s in sessions])
    files = [pipeline.BatchFile(i * T, T, [(float(rec.py2_float_str(s / 125.0)), float(rec.py2_float_str(e / 125.0)))
                                           for (s, e) in sessions[i][1]]) for i in range(args.files)]
    del sessions
    ctx = hipabi.Context(0, torch.cuda.current_stream().cuda_stream)
    cl = dict(pipeline.DIA2_CL, path=1)                            # one workgroup per problem
    span = (C.c_ulonglong * (2 * args.files))()
    khz = C.c_int()
    for it in range(2):                                            # (the first call sizes the scratch)
        lib.spkd_debug_ahc_span(span, args.files, C.byref(khz))    # (zeroes the clocks)
        tm = {}
        rows = pipeline.diarize_batch(ctx, frames.data_ptr(), args.files * T, files, cl=cl, timings=tm, fused=True)
    if lib.spkd_debug_ahc_span(span, args.files, C.byref(khz)) != 0:
        raise SystemExit('spkd_debug_ahc_span failed')
    n = np.array([len(r) for r in rows], dtype=np.int64)           # a row per record of the problem
    clk = np.array(list(span), dtype=np.float64).reshape(-1, 2) / float(khz.value)      # ms
    enter, leave = clk[:, 0] - clk[:, 0].min(), clk[:, 1] - clk[:, 0].min()
    t = leave - enter
    order = np.argsort(leave)
    expo, log_c = np.polyfit(np.log(n), np.log(t), 1)
    launch = float(leave.max())
    big = int(np.argmax(n))
    out = {
        'what': 'k_ahc per problem: wall clock of thread 0 at entry and exit, profiling build, benchmark batch',
        'files': args.files, 'ahc_head': tm.get('ahc_head'), 'wall_clock_khz': int(khz.value),
        'n_segments': int(n.sum()), 'n_mean': float(n.mean()), 'n_std': float(n.std()), 'n_min': int(n.min()), 'n_max': int(n.max()),
        'n_largest_12': sorted(n.tolist(), reverse=True)[:12],
        'timer_matrix_ms': tm['matrix'][-1], 'timer_ahc_ms': tm['ahc'][-1],
        'launch_ms': launch,
        'fitted_exponent_t_against_n': float(expo), 'fit_ms_at_n_mean': float(np.exp(log_c) * n.mean() ** expo),
        't_largest_problem_ms': float(t[big]), 't_mean_ms': float(t.mean()),
        'last_exit_after_second_to_last_ms': float(leave[order[-1]] - leave[order[-2]]),
        'last_exit_after_median_exit_ms': float(leave.max() - np.median(leave)),
        'last_entry_ms': float(enter.max()),
        'cu_time_idle_share': float((launch - leave).sum() / (launch * len(n))),
        # the constants of ahc_head_rule: a lone problem's milliseconds per N^2 (the largest problem's, which is
        # what ends the launch), and k_matrix's chip-milliseconds per sum of N^2
        'ahc_ms_per_n2': float(t[big] / float(n[big]) ** 2),
        'matrix_ms_per_n2': float(tm['matrix'][-1] / float((n.astype(np.float64) ** 2).sum())),
        'problems': [{'p': int(p), 'n': int(n[p]), 'enter_ms': round(float(enter[p]), 4), 't_ms': round(float(t[p]), 4)}
                     for p in range(len(n))],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != 'problems'}))


if __name__ == '__main__':
    main()
