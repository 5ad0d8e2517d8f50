#!/usr/bin/env python
"""The largest absolute difference between the device's GCC-PHAT correlation (spkd_bf_gcc's d_curve, a
float32 transform) and the float64 restatement (tests/beamform_numpy.py) over every element of the scenes
S1 .. S5 and the coloured S1, per scene and overall.  tests/test_beamform_batch.py takes 16 times the
overall figure as its bound, and refuses a bound above 1e-4.

  python tools/beamform_accuracy.py [--out profiles/beamform_accuracy.json]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
hipabi = importlib.import_module('speaker-diarization_amd.hipabi')
import beamform_numpy as B                      # noqa: E402


def device_curve(ctx, x, geom, ref):
    T, C = B.steps(len(x), x.shape[1], geom), x.shape[1]
    size = T * C * (2 * geom[2] + 1)
    d_raw = ctx.dev_scratch('acc_raw', max(x.nbytes, 16))
    ctx.h2d(d_raw, x)
    d_ref, d_lag, d_val = ctx.dev_scratch('acc_ref', 16), ctx.dev_scratch('acc_lag', 16 * T * C), ctx.dev_scratch('acc_val', 16 * T * C)
    d_curve = ctx.dev_scratch('acc_curve', 4 * size)
    ctx.bf_gcc(d_raw, [0, x.size], [C], [0], [geom], [ref], d_ref, d_lag, d_val, d_curve)
    out = np.zeros(size, dtype=np.float32)
    ctx.d2h(out, d_curve)
    return out.reshape(T, C, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'beamform_accuracy.json'))
    a = ap.parse_args()
    ctx = hipabi.Context(0)
    scenes = {}
    for name in B.SCENES:
        sc = B.scene(name)
        got = device_curve(ctx, sc['x'], sc['geom'], 0).astype(np.float64)
        want = B.curve(sc['x'], 0, sc['geom'], dtype=np.float64)
        scenes[name] = float(np.abs(got - want).max())
        print('%s: %d values, largest difference %.3e' % (name, got.size, scenes[name]), file=sys.stderr, flush=True)
    ctx.close()
    worst = max(scenes.values())
    res = dict(what='max |d_curve - float64 restatement| over all elements', scenes=scenes, max_abs_diff=worst,
               test_bound=16 * worst, bound_limit=1e-4)
    line = json.dumps(res)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
