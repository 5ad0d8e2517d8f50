#!/usr/bin/env python
"""Times the self-trained speech / non-speech detector on a batch of --files x --seconds of audio and on
one file of --long-hours.  The audio is one minute of the test suite's synthetic talk (stretches of two
harmonic voices over low noise, tests/self_vad_numpy.py) repeated to length, generated once and copied to
every file's place in one device buffer, so the host holds one file; every figure is taken after a
warm-up, over --runs calls.

  frame_energy    the `frame_energy` kernel timer's [min, median, max], the bytes the kernel has to read
                  (2 a sample) and write (8 a frame), the GB/s they make of the median, and that as a
                  fraction of device_copy: a device-to-device copy of --copy-mib in the same process,
                  read plus written bytes over its synchronous wall time.
  energy_seeds    the `energy_seeds` timer (both launches and the wait between them) with a tenth of the
                  frames at either end, for the batch and for the single long file (one workgroup).
  decode          the wall time of the whole self_vad.decode_batch (with the one feature chain it shares
                  with the diarization, and without it) next to exp_generator.decode_batch on the same
                  samples with the test suite's synthetic VAD model -- that call includes the second
                  feature chain (256-sample windows) a model brings -- and the self-trained call's
                  kernel timers.

  python tools/self_vad_time.py [--files 64] [--seconds 600] [--long-hours 10] [--runs 5]
                                [--out profiles/self_vad_time.json]"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
hipabi = importlib.import_module('speaker-diarization_amd.hipabi')
fe = importlib.import_module('speaker-diarization_amd.frontend')
self_vad = importlib.import_module('speaker-diarization_amd.self_vad')
exp_generator = importlib.import_module('speaker-diarization_amd.exp_generator')
from mfcc_batch_time import spread               # noqa: E402
from resample_time import device_copy            # noqa: E402
import self_vad_numpy as S                       # noqa: E402
from test_generate_exp import _synthetic_mixtures, load_model, write_model      # noqa: E402
from test_mfcc_batch import _cfg                 # noqa: E402

RATE = 16000


def place(ctx, one, n_files):
    """n_files copies of `one` in the context's sample buffer -> (d_pcm, sample_off)."""
    sample_off = np.arange(n_files + 1, dtype=np.int64) * len(one)
    d_pcm = ctx.dev_scratch('pcm_batch', 2 * int(sample_off[-1]))
    for o in sample_off[:-1]:
        ctx.h2d(d_pcm + 2 * int(o), one)
    return d_pcm, sample_off


def seed_stage(ctx, cfg, d_pcm, sample_off, runs, copy_gbs):
    """The two kernels' figures for the samples as they lie on the device."""
    frame_off = fe.frame_offsets(sample_off, cfg.hop)
    total = int(frame_off[-1])
    d_energy = ctx.dev_scratch('self_vad_energy', max(total, 1) * 8)
    k = [self_vad.seed_counts(self_vad.SELF_VAD, int(T)) for T in np.diff(frame_off)]
    e_ms, s_ms, n_runs, seeded = [], [], 0, 0
    for _ in range(runs + 1):                                        # the first one warms up
        assert np.array_equal(ctx.frame_energy_batch(d_pcm, sample_off, cfg.hop, cfg.window_width, d_energy), frame_off)
        e_ms.append(ctx.last_ms('frame_energy'))
        r = ctx.energy_seeds(d_energy, frame_off, [a for a, _ in k], [b for _, b in k])
        s_ms.append(ctx.last_ms('energy_seeds'))
        n_runs, seeded = int(r[3][-1]), int(r[2].sum())
    e_ms, s_ms = e_ms[1:], s_ms[1:]
    nbytes = 2 * int(sample_off[-1]) + 8 * total
    gbs = nbytes / (1e6 * float(np.median(e_ms)))
    return dict(samples=int(sample_off[-1]), frames=total, frame_energy_ms=spread(e_ms), bytes_read_plus_written=nbytes,
                gb_per_s=round(gbs, 1), copy_fraction=round(gbs / copy_gbs, 3), energy_seeds_ms=spread(s_ms),
                files_seeded=seeded, runs=n_runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--seconds', type=int, default=600)
    ap.add_argument('--long-hours', type=float, default=10.0)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--copy-mib', type=int, default=1024)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'self_vad_time.json'))
    a = ap.parse_args()
    cfg = _cfg(400)
    minute = S.talk(60.0, 20261020, RATE)[0]
    one = np.tile(minute, (a.seconds + 59) // 60)[:a.seconds * RATE]
    ctx = hipabi.Context(0)
    res = dict(files=a.files, seconds=a.seconds, long_hours=a.long_hours, runs=a.runs, hop=cfg.hop, window=cfg.window_width,
               tile=hipabi.ENERGY_TILE, settings=self_vad.SELF_VAD, device_copy=device_copy(ctx, a.copy_mib, a.runs))
    print('device copy: %s' % json.dumps(res['device_copy']), file=sys.stderr, flush=True)
    copy_gbs = res['device_copy']['gb_per_s']

    d_pcm, sample_off = place(ctx, one, a.files)
    res['batch'] = seed_stage(ctx, cfg, d_pcm, sample_off, a.runs, copy_gbs)
    print('batch: %s' % json.dumps(res['batch']), file=sys.stderr, flush=True)

    # the whole stage next to the model path, on the same samples
    with tempfile.TemporaryDirectory() as d:
        write_model(d, *_synthetic_mixtures(np.random.default_rng(11)))
        model = load_model(d)
    self_ms, shared_ms, model_ms, kernels, detail = [], [], [], {}, {}
    for _ in range(a.runs + 1):
        t0 = time.perf_counter()
        d_frames, frame_off = fe.extract_batch(ctx, cfg, d_pcm, sample_off)
        t1 = time.perf_counter()
        timings = {}
        tokens, _ = self_vad.decode_batch(ctx, self_vad.SELF_VAD, cfg, d_pcm, sample_off, d_frames, frame_off, timings, detail)
        t2 = time.perf_counter()
        model_tokens, _ = exp_generator.decode_batch(ctx, model, None, uploaded=(d_pcm, sample_off))
        t3 = time.perf_counter()
        self_ms.append(1e3 * (t2 - t0))
        shared_ms.append(1e3 * (t2 - t1))
        model_ms.append(1e3 * (t3 - t2))
        for key, v in timings.items():
            kernels.setdefault(key, []).append(float(np.sum(v)))
    res['decode'] = dict(
        self_trained_with_its_feature_chain_ms=spread(self_ms[1:]), self_trained_on_shared_features_ms=spread(shared_ms[1:]),
        model_path_with_its_feature_chain_ms=spread(model_ms[1:]),
        kernel_ms_summed_over_a_call={key: spread(v[1:]) for key, v in sorted(kernels.items())},
        passes_run=detail['vad_passes_run'], untrained=len(detail['vad_untrained']),
        tokens_self_trained=int(sum(len(t) for t in tokens)), tokens_model=int(sum(len(t) for t in model_tokens)))
    print('decode: %s' % json.dumps(res['decode']), file=sys.stderr, flush=True)

    long_one = np.tile(minute, int(a.long_hours * 60 + 0.5))
    d_pcm, sample_off = place(ctx, long_one, 1)
    res['long_file'] = seed_stage(ctx, cfg, d_pcm, sample_off, a.runs, copy_gbs)
    print('long file: %s' % json.dumps(res['long_file']), file=sys.stderr, flush=True)
    ctx.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
