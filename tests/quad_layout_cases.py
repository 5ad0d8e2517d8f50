"""The calls whose bits tests/test_quad_layout_bits.py pins, stated once: the test runs them on
the library under test, tools/record_quad_bits.py on a library built from the commit before the
quad row split changed (SPKD_HIP_LIBRARY) to write tests/golden/quad_layout_bits.npz.

Which lane and slot of the quad layout holds element (i, j) is a relabelling: the chain of
operations that produces every element is the same, so every result is the same to the bit.

compute() -> dict name -> numpy array.  float64 arrays are compared as uint64 (NaNs by their bit
pattern); slots a call does not write are left out or zeroed here, never compared as they come."""
import hashlib
import importlib
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_REC = 37
SHORT = 20            # the record with 20 frames: rank-deficient, so the pivoting fallback runs
SHORT_LEN = 20
GW_WAVES = (1, 4, 8)
KINDS = ('BIC', 'GLR')
SMALL = 12            # lines of the merge_batch and of the cluster_in problem


def _pkg(name):
    return importlib.import_module('speaker-diarization_amd.' + name)


def segments():
    """37 consecutive frame ranges of 150..500 frames, one of them of 20."""
    segs, at = [], 0
    for k in range(N_REC):
        n = SHORT_LEN if k == SHORT else 150 + (k * 97) % 351
        segs.append((at, at + n))
        at += n
    return segs


def merge_log(x, n_merges, seg_off):
    """The merges a problem made, problem after problem (slots behind them are not written)."""
    return np.concatenate([x[int(o):int(o) + int(n)] for o, n in zip(seg_off[:-1], n_merges)])


PAIRS = ((SHORT, 3), (5, SHORT), (SHORT, 36), (0, 1), (7, 30), (36, 2))


def _gw_case(ctx, hipabi, eng, vad, kind):
    b = np.array([s for (s, e) in vad], dtype=np.int64)
    e = np.array([e_ for (s, e_) in vad], dtype=np.int64)
    p = hipabi.CdParams(hipabi.KINDS[kind], 0, 1.0, 0.0, 125.0, 375.0, 12.0, 125.0)
    g = ctx.gw(eng.d_frames, eng.n_frames, b, e, p)
    out = {'status': np.array([g['status']], dtype=np.int64), 'n_win': g['n_win'].copy(),
           'final_start': g['final_start'].copy()}
    cols = {k: [] for k in ('win_det', 'win_maxd', 'det_start', 'det_maxi', 'det_d')}
    for t in range(len(b)):                              # (slots behind a turn's last event are not written)
        n, o = int(g['n_win'][t]), int(g['off'][t])
        nd = int(g['win_det'][o:o + n].sum())
        for k in ('win_det', 'win_maxd'):
            cols[k].append(g[k][o:o + n])
        for k in ('det_start', 'det_maxi', 'det_d'):
            cols[k].append(g[k][o:o + nd])
    for k, v in cols.items():
        out[k] = np.concatenate(v)
    return out


def compute():
    import torch
    hipabi = _pkg('hipabi')
    engine = _pkg('engine')
    synth = _pkg('synth')
    res = {}
    eng = engine.HipEngine(0)
    ctx = eng.ctx
    owned = []

    def alloc(nbytes):
        p = ctx.dev_alloc(nbytes)
        owned.append(p)
        return p

    def records(sets):
        p = eng._stats_of_sets([[s] for s in sets])
        owned.append(p)
        return p

    try:
        # ---- records
        segs = segments()
        feats, _, _ = synth.make_session(50519, 120, 2)
        assert feats.shape[0] >= segs[-1][1]
        eng.set_features(feats)
        d_rec = records(segs)
        rec = np.empty((N_REC, hipabi.REC), dtype=np.float64)
        ctx.d2h(rec, d_rec)
        # (the records come from the statistics kernels, which know nothing of the quad layout, and
        # are most of the bytes: all of them as a digest, the counts and the short one in full)
        res['records_sha256'] = np.frombuffer(hashlib.sha256(rec.tobytes()).digest(), dtype=np.uint8)
        res['record_counts'] = rec[:, hipabi.REC - 1].copy()
        res['record_short'] = rec[SHORT].copy()
        # ---- distance_matrix (entries the call does not write stay zero)
        d_mat = alloc(N_REC * N_REC * 8)
        for kind in KINDS:
            ctx.h2d(d_mat, np.zeros((N_REC, N_REC)))
            st = ctx.distance_matrix(kind, 1.3, d_rec, N_REC, d_mat)
            m = np.empty((N_REC, N_REC), dtype=np.float64)
            ctx.d2h(m, d_mat)
            res['matrix_%s' % kind] = m
            res['matrix_%s_status' % kind] = np.array([st], dtype=np.int64)
        # ---- pair_terms
        out, st = ctx.pair_terms(d_rec, [a for a, _ in PAIRS], [b for _, b in PAIRS], hipabi.WANT_GLR)
        res['pair_terms'] = out
        res['pair_terms_status'] = np.array([st], dtype=np.int64)
        # ---- ahc: problems of 2, 9 and 37 records in one call
        d_ahc = records(segs[0:2] + segs[2:11] + segs)
        seg_off = [0, 2, 11, 11 + N_REC]
        for path in (hipabi.AHC_MONO, hipabi.AHC_WIDE):
            for variant in (1, 2):
                p = hipabi.AhcParams(variant, hipabi.KINDS['BIC'], 0, path, 1.3, 0.0)
                r = ctx.ahc(d_ahc, seg_off, p)
                tag = 'ahc_p%d_v%d_' % (path, variant)
                res[tag + 'status'] = np.array([r['status']], dtype=np.int64)
                for k in ('n_merges', 'stat_max', 'stat_min'):
                    res[tag + k] = r[k]
                for k in ('a', 'b', 'd'):
                    res[tag + k] = merge_log(r[k], r['n_merges'], seg_off)
        # ---- merge_batch and cluster_in: one small problem each
        small = [s for k, s in enumerate(segs) if k != SHORT][:SMALL]
        r = ctx.merge_batch(eng.d_frames, eng.n_frames, [0, SMALL], [s for s, _ in small], [e for _, e in small],
                            'BIC', 1.3, 0.0)
        for k in ('merged', 'dist', 'n_done', 'win_cnt', 'win_max', 'win_min', 'det_cnt', 'det_max', 'det_min'):
            res['merge_' + k] = r[k]
        res['merge_status'] = np.array([r['status']], dtype=np.int64)
        d_small = records(small)
        r = ctx.cluster_in_batch(d_small, [0, SMALL], 'BIC', 1.3, 0.0)
        for k in ('label', 'mind', 'n_done', 'n_clusters', 'stat_max', 'stat_min'):
            res['cin_' + k] = r[k]
        res['cin_status'] = np.array([r['status']], dtype=np.int64)
        # ---- gw: the 400 s / 4-speaker session, every wave shape
        meta = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'functions.json')))['session']
        feats, vad, _ = synth.make_session(7001, 400, 4)
        assert synth.fea_sha256(feats) == meta['sha256'], 'synthetic generator is not reproducible here'
        eng.set_features(feats)
        saved = os.environ.get('SPKD_GW_WAVES')
        try:
            for nw in GW_WAVES:
                os.environ['SPKD_GW_WAVES'] = str(nw)
                c2 = hipabi.Context(0, torch.cuda.current_stream().cuda_stream)   # (reads the switch when it is made)
                try:
                    for kind in KINDS:
                        for k, v in _gw_case(c2, hipabi, eng, vad, kind).items():
                            res['gw%d_%s_%s' % (nw, kind, k)] = v
                finally:
                    c2.close()
        finally:
            if saved is None:
                os.environ.pop('SPKD_GW_WAVES', None)
            else:
                os.environ['SPKD_GW_WAVES'] = saved
    finally:
        for p in owned:
            ctx.dev_free(p)
        eng.close()
    return {k: np.ascontiguousarray(v) for k, v in res.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a
