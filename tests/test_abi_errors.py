"""Refusals of the C ABI on both sides of the point where a call opens its bracket (run with
-m gpu on an MI355X).  Each keeps its status and its message, and leaves nothing behind on
the context: a valid set_stats -> ahc and a valid gw on the same context afterwards give the
same bits as on a fresh one.

The refused arguments stay inside the buffers they name (frame counts and record counts are
claimed smaller than what is allocated), so a check that failed to refuse would still read
and write nothing out of bounds."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

SPARE_FRAMES = 100


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _gw_params(hipabi):
    return hipabi.CdParams(hipabi.KINDS['BIC'], 0, 1.0, 0.0, 125.0, 375.0, 12.0, 125.0)


def _refuse_all(ctx, hipabi, d_frames, n_frames, b, e, d_stats, n):
    """b, e: the voiced turns (gw, sw); n: records in d_stats."""
    lib, h = ctx.lib, ctx.h

    def refused(st, text):
        assert st == hipabi.SPKD_EINVAL, (st, text)
        assert text in lib.spkd_last_error(h).decode()

    # set_stats: a range past the last frame, refused in set_stats_launch after the bracket opened
    n_claimed = n_frames - SPARE_FRAMES
    rb = np.array([0], dtype=np.int64)
    re_ = np.array([n_claimed + 1], dtype=np.int64)
    rs = np.zeros(1, dtype=np.int32)
    refused(lib.spkd_set_stats(h, C.c_void_p(d_frames), n_claimed, _p(rb), _p(re_), _p(rs), 1, 1,
                               C.c_void_p(d_stats)), 'bad frame range or set id')

    # gather_stats: a source index past the records
    si = np.array([0, n - 1], dtype=np.int64)
    refused(lib.spkd_gather_stats(h, C.c_void_p(d_stats), n - 1, _p(si), None, 2, n, C.c_void_p(d_stats)),
            'gather: source index out of range')

    # gw_ex: one event slot per turn, with the capacity check on
    nt = len(b)
    P = _gw_params(hipabi)
    off = np.arange(nt + 1, dtype=np.int64)
    i32 = [np.zeros(nt, dtype=np.int32) for _ in range(2)]
    f64 = [np.zeros(nt, dtype=np.float64) for _ in range(5)]
    cnt = C.c_int64(0)
    refused(lib.spkd_gw_ex(h, C.c_void_p(d_frames), n_frames, _p(b), _p(e), nt, C.byref(P), _p(off), 1,
                           _p(i32[0]), _p(f64[0]), _p(i32[1]), _p(f64[1]), _p(f64[2]), _p(f64[3]), _p(f64[4]),
                           None, 0, C.byref(cnt)),
            'gw: event capacity too small, see spkd_gw_event_capacity_p')

    # ahc: the second of two problems is empty
    seg_off = np.array([0, n, n], dtype=np.int64)
    n_merges = np.zeros(2, dtype=np.int32)
    ma, mb = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    md = np.zeros(n, dtype=np.float64)
    smax, smin = np.zeros(2, dtype=np.float64), np.zeros(2, dtype=np.float64)
    A = hipabi.AhcParams(1, hipabi.KINDS['BIC'], 0, hipabi.AHC_AUTO, 1.3, 0.0)
    refused(lib.spkd_ahc(h, C.c_void_p(d_stats), _p(seg_off), 2, C.byref(A), _p(n_merges), _p(ma), _p(mb),
                         _p(md), _p(smax), _p(smin)), 'empty clustering problem')

    # sw: one window more than spkd_sw_window_count gives the turn
    S = hipabi.CdParams(hipabi.KINDS['BIC'], 0, 1.0, 0.0, 100.0, 50.0, 12.0, 100.0)
    w = lib.spkd_sw_window_count(int(e[0] - b[0]), S.winsize, S.winstep)
    assert w > 0
    d_off = np.array([0, w + 1], dtype=np.int64)
    dist = np.zeros(w + 1, dtype=np.float64)
    refused(lib.spkd_sw(h, C.c_void_p(d_frames), n_frames, _p(b[:1]), _p(e[:1]), 1, C.byref(S), _p(d_off),
                        _p(dist)), 'sw: offsets do not match spkd_sw_window_count')


def _valid_calls(ctx, hipabi, d_frames, n_frames, b, e, sb, se, d_stats):
    """set_stats over the speaker turns sb, se -> ahc over their records; gw over the voiced turns b, e."""
    n = len(sb)
    ctx.set_stats(d_frames, n_frames, sb, se, np.arange(n, dtype=np.int32), n, d_stats)
    stats = np.empty((n, hipabi.REC), dtype=np.float64)
    ctx.d2h(stats, d_stats)
    ahc = ctx.ahc(d_stats, [0, n], hipabi.AhcParams(1, hipabi.KINDS['BIC'], 0, hipabi.AHC_AUTO, 1.3, 0.0))
    gw = ctx.gw(d_frames, n_frames, b, e, _gw_params(hipabi))
    return stats, ahc, gw


def _same_gw(a, b, hipabi):
    assert np.array_equal(a['n_win'], b['n_win']) and np.array_equal(a['off'], b['off'])
    assert a['final_start'].tobytes() == b['final_start'].tobytes()
    for t in range(len(a['n_win'])):                  # (slots behind a turn's last event are not written)
        o, k = int(a['off'][t]), int(a['n_win'][t])
        assert a['win_det'][o:o + k].tobytes() == b['win_det'][o:o + k].tobytes(), t
        assert a['win_maxd'][o:o + k].tobytes() == b['win_maxd'][o:o + k].tobytes(), t
        nd = int(a['win_det'][o:o + k].sum())
        for key in ('det_start', 'det_maxi', 'det_d'):
            assert a[key][o:o + nd].tobytes() == b[key][o:o + nd].tobytes(), (t, key)
    assert a['log_count'] == b['log_count']
    size = a['log_count'] * C.sizeof(hipabi.CandLog)
    assert C.string_at(C.addressof(a['log']), size) == C.string_at(C.addressof(b['log']), size)


def test_refusals_leave_the_context_as_a_fresh_one():
    hipabi = pkg('hipabi')
    synth = pkg('synth')
    feats, vad, truth = synth.make_session(20261015, 120, 3)
    feats = np.ascontiguousarray(feats, dtype=np.float32)
    n_frames = feats.shape[0]
    assert n_frames > 2 * SPARE_FRAMES
    b = np.array([s for s, _ in vad], dtype=np.int64)
    e = np.array([t for _, t in vad], dtype=np.int64)
    sb = np.array([s for s, _, _ in truth], dtype=np.int64)
    se = np.array([t for _, t, _ in truth], dtype=np.int64)
    n = len(sb)
    assert n >= 8 and len(b) >= 2
    ctx = hipabi.Context(0)
    fresh = None
    try:
        d_frames = ctx.dev_alloc(feats.nbytes)
        ctx.h2d(d_frames, feats)
        d_stats = ctx.dev_alloc(n * hipabi.REC * 8)
        _refuse_all(ctx, hipabi, d_frames, n_frames, b, e, d_stats, n)
        got = _valid_calls(ctx, hipabi, d_frames, n_frames, b, e, sb, se, d_stats)
        fresh = hipabi.Context(0)
        want = _valid_calls(fresh, hipabi, d_frames, n_frames, b, e, sb, se, d_stats)
        assert got[0].tobytes() == want[0].tobytes()
        assert got[1]['status'] == want[1]['status'] == hipabi.SPKD_OK
        for key in ('n_merges', 'stat_max', 'stat_min'):
            assert got[1][key].tobytes() == want[1][key].tobytes(), key
        m = int(got[1]['n_merges'][0])
        assert m > 0
        for key in ('a', 'b', 'd'):                  # (slots behind the last merge are not written)
            assert got[1][key][:m].tobytes() == want[1][key][:m].tobytes(), key
        assert got[2]['status'] == want[2]['status'] == hipabi.SPKD_OK
        _same_gw(got[2], want[2], hipabi)
        ctx.dev_free(d_stats)
        ctx.dev_free(d_frames)
    finally:
        if fresh is not None:
            fresh.close()
        ctx.close()
