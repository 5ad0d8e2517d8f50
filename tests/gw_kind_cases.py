"""The calls whose bits tests/test_gw_kind_instances.py pins, stated once: the test runs them on the
library under test, tools/record_gw_kind_bits.py on a library built from the commit BEFORE the
distance kind became a constant of the k_gw instances (SPKD_HIP_LIBRARY) to write
tests/golden/gw_kind_instances.npz.

The four short turns of tests/test_gw_wave_shapes_small.py (_case(): no scan at all; coarse scans,
a fine scan from a cache record and a new epoch; a fine scan from zero sums; negative to the turn
end), in fused mode, for BIC, GLR and KL2 in each of the four wave shapes: twelve kernel
instances.  The parameters are the benchmark's; the thresholds of GLR and KL2 lie between the
window maxima of the turns so that each kind meets every case (the C oracle on these turns:
GLR's coarse maxima are 508 .. 1 628 before the change of turn 1 is inside the window and 8 555
with it, 2 860 in the first window of turn 2, below 562 everywhere else; KL2's are 17 .. 136, then
564, 760 in turn 2, below 178 elsewhere) -- test_gw_kind_instances.py asserts on the FIXTURE that
they do.

run_all() -> {(kind, shape): {name: array}}.  Slots behind a turn's last event are not written by
the kernel and are left out here; float64 arrays are compared as uint64 by the test."""
import os

import numpy as np

from test_gw_wave_shapes_small import CD, DETECTIONS, EVENTS, SHAPES, _best_k, _case, _per_turn

KINDS = ('BIC', 'GLR', 'KL2')
THRESHOLD = {'BIC': CD['threshold'], 'GLR': 2000.0, 'KL2': 300.0}
N_TURNS = 4


def _pkg(name):
    import importlib
    return importlib.import_module('speaker-diarization_amd.' + name)


def _flatten(g, rec):
    """One gw result -> name -> array: per turn, what the turn wrote."""
    out = {'n_win': g['n_win'].copy(), 'final_start': g['final_start'].copy()}
    for t in range(N_TURNS):
        ev, nd = _per_turn(g, t)
        for k in EVENTS + DETECTIONS:
            out['t%d.%s' % (t, k)] = np.ascontiguousarray(ev[k]).copy()
        o = int(g['off'][t])
        out['t%d.records' % t] = rec[o:o + nd + 1].copy()      # one per detection, then the tail's
        # index of the coarse maximum of every window that ended in a detection (from the log)
        out['t%d.best_k' % t] = np.array(_best_k(g, t), dtype=np.int64)
    return out


def run_all(kinds=KINDS, shapes=SHAPES):
    import torch
    hipabi, engine = _pkg('hipabi'), _pkg('engine')
    feats, turns = _case()
    b = np.array([t[0] for t in turns], dtype=np.int64)
    e = np.array([t[1] for t in turns], dtype=np.int64)
    got = {}
    eng = engine.HipEngine(0)
    saved = os.environ.get('SPKD_GW_WAVES')
    try:
        eng.set_features(feats)
        for nw in shapes:
            os.environ['SPKD_GW_WAVES'] = str(nw)
            ctx = hipabi.Context(0, torch.cuda.current_stream().cuda_stream)   # (reads the switch when it is made)
            try:
                for kind in kinds:
                    p = hipabi.CdParams(hipabi.KINDS[kind], 1, CD['lambdac'], THRESHOLD[kind], CD['winsize'],
                                        CD['winstep'], CD['deltaws'], CD['rate'])
                    seg = {}

                    def seg_stats(n_rec):
                        seg['n'] = n_rec
                        seg['d'] = ctx.dev_scratch('fused_records', n_rec * hipabi.REC * 8)
                        return seg['d']
                    g = ctx.gw(eng.d_frames, eng.n_frames, b, e, p, log_cap=1 << 14, seg_stats=seg_stats)
                    assert g['status'] == 0, (kind, nw, g['status'])
                    rec = np.empty((seg['n'], hipabi.REC), dtype=np.float64)
                    ctx.d2h(rec, seg['d'])
                    got[(kind, nw)] = _flatten(g, rec)
            finally:
                ctx.close()
    finally:
        if saved is None:
            os.environ.pop('SPKD_GW_WAVES', None)
        else:
            os.environ['SPKD_GW_WAVES'] = saved
        eng.close()
    return got


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(x, y):
    """name -> array dicts equal to the bit; returns the first name that differs, or None."""
    if sorted(x) != sorted(y):
        return 'the set of arrays'
    for k in sorted(x):
        if x[k].shape != y[k].shape or x[k].dtype != y[k].dtype or not np.array_equal(bits(x[k]), bits(y[k])):
            return k
    return None
