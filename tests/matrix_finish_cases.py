"""The calls whose bits tests/test_matrix_finish_bits.py pins, stated once: the test runs them on
the library under test, tools/record_matrix_finish_bits.py on a library built from the commit
before k_matrix's passes stopped finishing their distances (SPKD_HIP_LIBRARY) to write
tests/golden/matrix_finish_bits.npz.

k_matrix's passes now park the bare determinant and a dense phase takes the logs and finishes the
distances, one thread per partner.  That moves WHERE a value is computed, never how: every result
is the same to the bit.  The merge loops read that matrix (AHC_WIDE and AHC_MONO alike), so their
merge logs are pinned with it.

compute() -> dict name -> numpy array.  float64 arrays are compared as uint64 (NaNs by their bit
pattern).  Matrices of up to SMALL_N records are kept in full, larger ones as one SHA-256 per
matrix row ((N, 32) uint8), so that a mismatch names the row.  The shapes:
  * N = 2, 5, 17, 18: less than one, exactly one, and one and a bit of a round of 16 partners (four
    waves of four);  N = 257, 258, 513: a row of exactly 256 partners (one trip of the dense loop's
    256 threads), of 257, and of two full trips;
  * one ahc call with problems of 2, 3, 65, 130, 513 and 600 records: across AHC_TPB = 512 in
    k_ahc's partner-list pass and its own dense finish."""
import hashlib
import importlib

import numpy as np

SESSION = (60219, 480, 4)        # synth.make_session(seed, seconds, speakers)
POOL = 600                       # consecutive frame ranges of 60 .. 120 frames
SHORT_LEN = 20                   # a record of 20 frames: rank 19, its own log det takes the pivoting fallback
SHORT2_LEN = 15                  # with the short one: 35 frames, a union of rank 34 -- the fallback inside a PASS
MATRIX_N = (2, 5, 17, 18, 257, 258, 513)
SMALL_N = 18
KINDS = ('BIC', 'GLR')
VARIANTS = (1, 2)
AHC_SIZES = (2, 3, 65, 130, 513, 600)
AHC_SHORT_PROBLEM = 3            # the problem of 130 records holds the two short ones, late
LAMBDAC = 1.3
SW_TURN = (1000, 9000)           # frames; windows of 250 + 250 every 31
SW_SIZE, SW_STEP = 250.0, 31.0


def _pkg(name):
    return importlib.import_module('speaker-diarization_amd.' + name)


def pool():
    segs, at = [], 0
    for k in range(POOL):
        n = 60 + (k * 37) % 61
        segs.append((at, at + n))
        at += n
    return segs


def short_at(n):
    """Where the 20-frame record sits among n: a late partner of row 0 and a row of its own (with
    the 15-frame one as its partner where there is room for both)."""
    return max(n - 3, 1) if n >= 5 else n - 1


def with_short(segs):
    """The ranges with the short records in their places (each the head of the range it replaces)."""
    segs = list(segs)
    n = len(segs)
    s = short_at(n)
    segs[s] = (segs[s][0], segs[s][0] + SHORT_LEN)
    if n >= 5:
        segs[s + 1] = (segs[s + 1][0], segs[s + 1][0] + SHORT2_LEN)
    return segs


def ahc_problems():
    """The ranges of the ahc call's problems, one after the other, and seg_off."""
    p = pool()
    starts = (0, 2, 5, 70, 0, 0)
    segs, seg_off = [], [0]
    for k, (s, n) in enumerate(zip(starts, AHC_SIZES)):
        part = p[s:s + n]
        segs += with_short(part) if k == AHC_SHORT_PROBLEM else part
        seg_off.append(len(segs))
    return segs, seg_off


def row_digests(m):
    """One SHA-256 per matrix row."""
    m = np.ascontiguousarray(m)
    return np.stack([np.frombuffer(hashlib.sha256(m[r].tobytes()).digest(), dtype=np.uint8) for r in range(m.shape[0])])


def merge_log(x, n_merges, seg_off):
    """The merges a problem made, problem after problem (slots behind them are not written)."""
    return np.concatenate([x[int(o):int(o) + int(n)] for o, n in zip(seg_off[:-1], n_merges)])


def compute():
    import ctypes as C
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
        feats, _, _ = synth.make_session(*SESSION)
        segs = pool()
        assert feats.shape[0] >= max(segs[-1][1], SW_TURN[1])
        eng.set_features(feats)
        # ---- the initial matrix: every row of an N-record problem (distance_rows), both variants
        n_big = max(MATRIX_N)
        d_mat = alloc(n_big * n_big * 8)
        for n in MATRIX_N:
            case = with_short(segs[:n])
            d_rec = records(case)
            rec = np.empty((n, hipabi.REC), dtype=np.float64)
            ctx.d2h(rec, d_rec)
            res['n%d_record_counts' % n] = rec[:, hipabi.REC - 1].copy()
            for kind in KINDS:
                for variant in VARIANTS:
                    tag = 'n%d_%s_v%d_' % (n, kind, variant)
                    ctx.h2d(d_mat, np.zeros((n, n)))          # (cells a call does not write stay zero)
                    smax, smin = C.c_double(), C.c_double()
                    st = ctx.lib.spkd_distance_rows(ctx.h, variant, hipabi.KINDS[kind], LAMBDAC, C.c_void_p(d_rec), n, 0, n,
                                                    C.c_void_p(d_mat), C.byref(smax), C.byref(smin))
                    ctx.check(st, allow=(hipabi.SPKD_ENONFINITE,))
                    m = np.empty((n, n), dtype=np.float64)
                    ctx.d2h(m, d_mat)
                    res[tag + 'status'] = np.array([st], dtype=np.int64)
                    res[tag + 'stat'] = np.array([smax.value, smin.value])
                    res[tag + 'matrix'] = m if n <= SMALL_N else row_digests(m)
                    if n == SMALL_N:
                        # the merge loop of one problem on that matrix (ahc_matrix)
                        p = hipabi.AhcParams(variant, hipabi.KINDS[kind], 0, hipabi.AHC_MONO, LAMBDAC, 0.0)
                        r = ctx.ahc_matrix(d_rec, n, p, d_mat, smax.value, smin.value)
                        res[tag + 'ahcm_status'] = np.array([r['status']], dtype=np.int64)
                        for k in ('n_merges', 'stat_max', 'stat_min'):
                            res[tag + 'ahcm_' + k] = r[k]
                        for k in ('a', 'b', 'd'):
                            res[tag + 'ahcm_' + k] = r[k][:int(r['n_merges'][0])]
                # distance_matrix: the same kernel behind the entry point without a variant
                if n in (SMALL_N, 257):
                    ctx.h2d(d_mat, np.zeros((n, n)))
                    st = ctx.distance_matrix(kind, LAMBDAC, d_rec, n, d_mat)
                    m = np.empty((n, n), dtype=np.float64)
                    ctx.d2h(m, d_mat)
                    res['n%d_%s_dm_status' % (n, kind)] = np.array([st], dtype=np.int64)
                    res['n%d_%s_dm_matrix' % (n, kind)] = m if n <= SMALL_N else row_digests(m)
        # ---- ahc: six problems in one call, the merge loop in both launch shapes
        asegs, seg_off = ahc_problems()
        d_ahc = records(asegs)
        for path in (hipabi.AHC_MONO, hipabi.AHC_WIDE):
            for variant in VARIANTS:
                for max_spk in (0, 3):
                    p = hipabi.AhcParams(variant, hipabi.KINDS['BIC'], max_spk, path, LAMBDAC, 0.0)
                    r = ctx.ahc(d_ahc, seg_off, p)
                    tag = 'ahc_p%d_v%d_s%d_' % (path, variant, max_spk)
                    res[tag + 'status'] = np.array([r['status']], dtype=np.int64)
                    for k in ('n_merges', 'stat_max', 'stat_min'):
                        res[tag + k] = r[k]
                    for k in ('a', 'b', 'd'):
                        res[tag + k] = merge_log(r[k], r['n_merges'], seg_off)
        # ---- sw: every window a two-record problem of which only the left row is launched
        p = hipabi.CdParams(hipabi.KINDS['BIC'], 0, LAMBDAC, 0.0, SW_SIZE, SW_STEP, 6.0, 125.0)
        st, off, d = ctx.sw(eng.d_frames, eng.n_frames, [SW_TURN[0]], [SW_TURN[1]], p)
        res['sw_status'] = np.array([st], dtype=np.int64)
        res['sw_off'] = off
        res['sw_d'] = d
        d_d = alloc(max(d.nbytes, 16))
        ctx.h2d(d_d, d)
        r = ctx.sw_runs(d_d, off, p)
        nd = int(r['n_det'][0])
        res['sw_n_det'] = r['n_det']
        res['sw_final_start'] = r['final_start']
        for k in ('det_start', 'det_maxi', 'det_d'):
            res['sw_' + k] = r[k][:nd]               # (one turn: its events from slot 0)
    finally:
        for p in owned:
            ctx.dev_free(p)
        eng.close()
    return {k: np.ascontiguousarray(v) for k, v in res.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a
