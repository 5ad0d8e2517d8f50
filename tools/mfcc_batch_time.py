#!/usr/bin/env python
"""Times the front-end of a whole batch (frontend.upload_batch + extract_batch: every file copied to
its place in one device buffer, one spkd_mfcc_batch) against the loop it replaces, timed in the same process: per file a
blocking copy of its samples and one spkd_mfcc into its slice of the feature buffer.  spkd_mfcc is
the batch call with one file, so this loop runs the SAME kernels: the comparison measures the
batching alone, and identical_to_per_file says that a file's place in a batch does not change its
bits.  With --reference-library (a libspkd_hip.so of the same ABI built from another commit, e.g.
the one before spkd_mfcc_batch) the same loop also runs on that library's spkd_mfcc: reference_ms
then measures its kernels, and identical_to_reference compares the features with its bits.
Synthetic int16 noise, the fconfig.cfg parameters, both window widths; per shape one warm-up of
every path, then --runs runs with the paths alternated; [min, median, max] of the wall
milliseconds, the medians of the two kernel timers of the batch call, frames per second of the
batch path (the front-end paragraph).

  python tools/mfcc_batch_time.py [--shapes 256x10,64x60,16x3600] [--windows 400,256] [--runs 5]
                                  [--reference-library PATH]"""
import argparse
import importlib
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hipabi = importlib.import_module('speaker-diarization_amd.hipabi')
fe = importlib.import_module('speaker-diarization_amd.frontend')

RATE, FRAME_RATE, DIM = 16000, 125, 39


def config(window):
    """fconfig.cfg's structural parameters with stand-ins for its trained arrays."""
    rng = np.random.default_rng(39)
    return types.SimpleNamespace(sample_rate=RATE, frame_rate=FRAME_RATE, hop=RATE // FRAME_RATE, window_width=window,
                                 n_cep=12, cms_left=75, cms_right=75, delta_width=(2, 2), pre_emph=0.97,
                                 delta_norm=(1.0, 10.0), dim=DIM, mean=np.zeros(DIM), scale=0.15 + 0.05 * np.arange(DIM),
                                 transform=(np.eye(DIM) + 0.1 * rng.standard_normal((DIM, DIM))).ravel())


class Reference(object):
    """spkd_mfcc of another build of the library, bound by hand: the entry points ABI version 2 has
    had from the start."""

    def __init__(self, path):
        C = hipabi.C
        self.lib = C.CDLL(path)
        assert self.lib.spkd_abi_version() == 2
        vp, i64 = C.c_void_p, C.c_int64
        self.lib.spkd_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
        self.lib.spkd_destroy.argtypes = [vp]
        self.lib.spkd_malloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
        self.lib.spkd_memcpy_h2d.argtypes = [vp, vp, vp, C.c_size_t]
        self.lib.spkd_memcpy_d2h.argtypes = [vp, vp, vp, C.c_size_t]
        self.lib.spkd_mfcc.argtypes = [vp, vp, i64, C.POINTER(hipabi.MfccParams), vp, vp, vp, vp, vp, vp, C.POINTER(i64)]
        self.h = vp()
        self.ok(self.lib.spkd_create(0, None, C.byref(self.h)))
        self.bufs = {}

    def ok(self, status):
        if status != 0:
            raise RuntimeError('reference library: status %d' % status)

    def buffer(self, name, nbytes):
        if self.bufs.get(name, (None, 0))[1] < nbytes:           # (grow-only)
            p = hipabi.C.c_void_p()
            self.ok(self.lib.spkd_malloc(self.h, nbytes, hipabi.C.byref(p)))
            self.bufs[name] = (p.value, nbytes)
        return self.bufs[name][0]

    def loop(self, pcms, frame_off, params, tables, d_pcm, d_out):
        C = hipabi.C
        n = C.c_int64()
        for p, o in zip(pcms, frame_off):
            self.ok(self.lib.spkd_memcpy_h2d(self.h, d_pcm, p.ctypes.data_as(C.c_void_p), p.nbytes))
            self.ok(self.lib.spkd_mfcc(self.h, d_pcm, len(p), C.byref(params), *[t.ctypes.data_as(C.c_void_p) for t in tables],
                                       d_out + int(o) * DIM * 4, C.byref(n)))

    def d2h(self, arr, d_src):
        self.ok(self.lib.spkd_memcpy_d2h(self.h, arr.ctypes.data_as(hipabi.C.c_void_p), d_src, arr.nbytes))


def spread(ms):
    return [round(float(f(ms)), 3) for f in (np.min, np.median, np.max)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='256x10,64x60,16x3600', help='files x seconds, comma separated')
    ap.add_argument('--windows', default='400,256')
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--reference-library', help='a libspkd_hip.so built from another commit: its spkd_mfcc in the same loop')
    a = ap.parse_args()
    ctx = hipabi.Context(0)
    ref = Reference(a.reference_library) if a.reference_library else None
    res = dict(runs=a.runs)
    rng = np.random.default_rng(5)
    for shape in a.shapes.split(','):
        n_files, seconds = (int(v) for v in shape.split('x'))
        pcms = [rng.integers(-32768, 32768, seconds * RATE, dtype=np.int16) for _ in range(n_files)]
        for window in (int(w) for w in a.windows.split(',')):
            cfg = config(window)
            frame_off = fe.frame_offsets(np.arange(n_files + 1) * seconds * RATE, cfg.hop)
            total = int(frame_off[-1])
            d_loop_out = ctx.dev_scratch('time_loop_features', total * DIM * 4)
            d_loop_pcm = ctx.dev_scratch('time_loop_pcm', seconds * RATE * 2)
            params, melfb, dct = fe.mfcc_params(cfg), fe.mel_filterbank(RATE), fe.dct_matrix(cfg.n_cep)
            kern = dict(mfcc_static=[], mfcc_post=[])
            box = {}

            def batch():
                d_pcm, sample_off = fe.upload_batch(ctx, pcms)
                box['d_out'], got = fe.extract_batch(ctx, cfg, d_pcm, sample_off)
                for k in kern:
                    kern[k].append(ctx.last_ms(k))
                assert np.array_equal(got, frame_off)

            def loop():
                for p, o in zip(pcms, frame_off):
                    ctx.h2d(d_loop_pcm, p)
                    ctx.mfcc(d_loop_pcm, len(p), params, melfb, dct, cfg.mean, cfg.scale, cfg.transform,
                             d_loop_out + int(o) * DIM * 4)

            paths = [('batch', batch), ('loop', loop)]
            if ref:
                tables = [np.ascontiguousarray(t, dtype=np.float32) for t in (melfb, dct, cfg.mean, cfg.scale, cfg.transform)]
                d_ref_out, d_ref_pcm = ref.buffer('features', total * DIM * 4), ref.buffer('pcm', seconds * RATE * 2)
                paths.append(('reference', lambda: ref.loop(pcms, frame_off, params, tables, d_ref_pcm, d_ref_out)))
            for _, fn in paths:
                fn()
            ms = {name: [] for name, _ in paths}
            for _ in range(a.runs):
                for name, fn in paths:
                    t = time.perf_counter()
                    fn()
                    ms[name].append(1e3 * (time.perf_counter() - t))
            got, want = (np.empty((total, DIM), dtype=np.float32) for _ in range(2))
            ctx.d2h(got, box['d_out'])
            ctx.d2h(want, d_loop_out)
            hours = n_files * seconds / 3600.0
            static_ms = float(np.median(kern['mfcc_static'][1:]))
            row = res['%s w%d' % (shape, window)] = dict(
                frames=total, batch_ms=spread(ms['batch']), loop_ms=spread(ms['loop']),
                mfcc_static_ms=round(static_ms, 3), mfcc_post_ms=round(float(np.median(kern['mfcc_post'][1:])), 3),
                static_ms_per_audio_hour=round(static_ms / hours, 3),
                frames_per_s=round(total / (1e-3 * float(np.median(ms['batch'])))),
                identical_to_per_file=bool(np.array_equal(got.view(np.uint32), want.view(np.uint32))))
            if ref:
                ref.d2h(want, d_ref_out)
                row.update(reference_ms=spread(ms['reference']),
                           identical_to_reference=bool(np.array_equal(got.view(np.uint32), want.view(np.uint32))))
            del got, want
            print('%s w%d: %s' % (shape, window, json.dumps(row)), file=sys.stderr, flush=True)
    if ref:
        ref.lib.spkd_destroy(ref.h)
    ctx.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
