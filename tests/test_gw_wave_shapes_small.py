"""Every entry of k_gw's sweep in every wave shape, on four short turns (a few seconds of GPU).

k_gw runs a turn on one, two, four or eight waves (SPKD_GW_WAVES pins the shape; a context reads
it when it is made).  Each shape has its own instances of the three sweep functions
(spkd_cd.hpp: gw_sweep_coarse, gw_sweep_fine, gw_sweep_tail); the sums, the eliminations and the
decisions are the same in all of them, so every output is the same to the bit.  The one- and
two-wave instances lost their register-save frame (GW_SWEEP_FN); the eight-wave instances never
had one and compile to what they were: they are the reference here.

One file of two synthetic speakers, fused mode (every segment leaves its statistics record), BIC
with the benchmark's flags, the candidate log on.  The four turns:

  0  1.5 s, shorter than twice the window: no scan at all, the tail record by gw_sweep_tail;
  1  12 s with the speaker change at 5 s: coarse scans over a growing window, a fine scan that
     starts from a cache record (the coarse maximum lies far behind candidate 2), a new epoch;
  2  the speaker change 0.6 s after the turn start: the coarse maximum is candidate 1 -- the
     candidates lie 0.5 s, 0.6 s, 0.7 s ... behind the window start, so a change any later has
     two candidates in front of it -- and the fine scan starts from zero sums (base == nullptr);
  3  8 s of one speaker: the turn ends on a negative scan whose window end is the turn end, so the
     tail record comes out of LDS.

That the turns do this is asserted (on the C oracle and on the device alike), not assumed."""
import os

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

SEED, SECONDS = 41001, 150
SHAPES = (1, 2, 4, 8)
REFERENCE = 8
EVENTS = ('win_maxd', 'win_det')
DETECTIONS = ('det_start', 'det_maxi', 'det_d')
# winsize 1.0 s, winstep 3.0 s, deltaws 0.1 s at 125 frames/s, lambda 1.0, threshold 0 (pipeline.DIA2_CD)
CD = dict(lambdac=1.0, threshold=0.0, winsize=125.0, winstep=375.0, deltaws=12.0, rate=125.0)


def _case():
    """(frames, turns): the file and the four frame ranges of the docstring."""
    synth = pkg('synth')
    feats, _, truth = synth.make_session(SEED, SECONDS, 2, min_turn=9.0, max_turn=15.0, group=(8, 8))
    change = [truth[i][1] for i in range(len(truth) - 1) if truth[i][1] == truth[i + 1][0]]
    one = [t for t in truth if t[1] - t[0] >= 1050][-1]
    turns = [(truth[0][0] + 10, truth[0][0] + 10 + 187),
             (change[0] - 625, change[0] + 875),
             (change[1] - 75, change[1] - 75 + 900),
             (one[0] + 20, one[0] + 1020)]
    assert all(0 <= b < e <= feats.shape[0] for b, e in turns)
    return feats, turns


def _per_turn(g, t):
    """What turn t wrote: its event arrays (slots behind its last event are not written)."""
    n, o = int(g['n_win'][t]), int(g['off'][t])
    nd = int(g['win_det'][o:o + n].sum())
    out = {k: g[k][o:o + n] for k in EVENTS}
    out.update({k: g[k][o:o + nd] for k in DETECTIONS})
    return out, nd


def _best_k(g, t):
    """Per detection of turn t: the index of the coarse maximum of its window, from the log
    (seq = window << 32 | candidate; the first of equal maxima, as the kernel takes it)."""
    n, o = int(g['n_win'][t]), int(g['off'][t])
    by_win = {}
    for i in range(g['log_count']):
        r = g['log'][i]
        if r.turn == t and r.coarse:
            by_win.setdefault(r.seq >> 32, []).append((r.seq & 0x7fffffff, r.d))
    out = []
    for w in range(n):
        if g['win_det'][o + w]:
            cands = sorted(by_win[w])
            assert [k for k, _ in cands] == list(range(len(cands)))
            out.append(max(cands, key=lambda kd: (kd[1], -kd[0]))[0])
    return out


@pytest.fixture(scope='module')
def runs():
    """shape -> (gw result, fused records [n_ev, REC]); plus the turns and the oracle's results."""
    import torch
    from oracle.c_engine import COracleEngine
    hipabi = pkg('hipabi')
    engine = pkg('engine')
    feats, turns = _case()
    orc = COracleEngine(1)
    orc.set_features(feats)
    want = orc.gw(turns, 'BIC', CD['lambdac'], CD['threshold'], CD['winsize'], CD['winstep'], CD['deltaws'],
                  CD['rate'], trace=True)
    b = np.array([t[0] for t in turns], dtype=np.int64)
    e = np.array([t[1] for t in turns], dtype=np.int64)
    p = hipabi.CdParams(hipabi.KINDS['BIC'], 1, CD['lambdac'], CD['threshold'], CD['winsize'], CD['winstep'],
                        CD['deltaws'], CD['rate'])
    got = {}
    eng = engine.HipEngine(0)
    saved = os.environ.get('SPKD_GW_WAVES')
    try:
        eng.set_features(feats)
        for nw in SHAPES:
            os.environ['SPKD_GW_WAVES'] = str(nw)
            ctx = hipabi.Context(0, torch.cuda.current_stream().cuda_stream)   # (reads the switch when it is made)
            try:
                seg = {}

                def seg_stats(n_rec):
                    seg['n'] = n_rec
                    seg['d'] = ctx.dev_scratch('fused_records', n_rec * hipabi.REC * 8)
                    return seg['d']
                g = ctx.gw(eng.d_frames, eng.n_frames, b, e, p, log_cap=1 << 14, seg_stats=seg_stats)
                rec = np.empty((seg['n'], hipabi.REC), dtype=np.float64)
                ctx.d2h(rec, seg['d'])
                got[nw] = (g, rec)
            finally:
                ctx.close()
    finally:
        if saved is None:
            os.environ.pop('SPKD_GW_WAVES', None)
        else:
            os.environ['SPKD_GW_WAVES'] = saved
        eng.close()
    return got, turns, want


def test_the_turns_exercise_every_entry_of_the_sweep(runs):
    got, turns, want = runs
    for nw in SHAPES:
        g = got[nw][0]
        assert g['status'] == 0
        nd = [_per_turn(g, t)[1] for t in range(4)]
        assert int(g['n_win'][0]) == 0 and nd[0] == 0              # no scan: gw_sweep_tail
        assert nd[1] >= 1 and int(g['n_win'][1]) > 3               # coarse scans, a detection, a new epoch
        assert min(_best_k(g, 1)) >= 2                             # its fine scan starts from a cache record
        assert nd[2] >= 1 and _best_k(g, 2)[0] < 2                 # fine scan from zero sums
        assert nd[3] == 0 and int(g['n_win'][3]) > 3               # negative to the turn end: tail from LDS
        assert g['final_start'][3] == 0.0
    # the oracle saw the same cases
    assert [sum(1 for ev in r.events if ev[0] == 'det') for r in want] == \
        [_per_turn(got[REFERENCE][0], t)[1] for t in range(4)]


@pytest.mark.parametrize('nw', [s for s in SHAPES if s != REFERENCE])
def test_shape_equals_the_eight_wave_shape_bit_for_bit(runs, nw):
    got = runs[0]
    (ref, ref_rec), (g, rec) = got[REFERENCE], got[nw]
    assert np.array_equal(ref['off'], g['off'])
    assert np.array_equal(ref['n_win'], g['n_win'])
    assert np.array_equal(ref['final_start'].view(np.uint64), g['final_start'].view(np.uint64))
    for t in range(4):
        (a, nd), (c, nd2) = _per_turn(ref, t), _per_turn(g, t)
        assert nd == nd2
        for k in EVENTS + DETECTIONS:
            x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(c[k])
            if x.dtype == np.float64:
                x, y = x.view(np.uint64), y.view(np.uint64)
            assert np.array_equal(x, y), (nw, t, k)
        # the fused records: one per detection, then the tail's
        o = int(ref['off'][t])
        assert np.array_equal(ref_rec[o:o + nd + 1].view(np.uint64), rec[o:o + nd + 1].view(np.uint64)), (nw, t)
        # (and the tail's record is the tail's: it carries the frame count of [final start, turn end))
        b, e = runs[1][t]
        assert ref_rec[o + nd, -1] == float(e - b - int(ref['final_start'][t]))


def test_detections_equal_the_c_oracle(runs):
    """Boundaries exactly; the distance within 1e-9 relative, the bound the suite holds fp64 BIC
    values of the device to against the C oracle (test_hip_parity.py: same formula, another
    order of the eliminations' operations)."""
    got, turns, want = runs
    g = got[REFERENCE][0]
    for t, r in enumerate(want):
        mine, nd = _per_turn(g, t)
        assert int(g['n_win'][t]) == sum(1 for ev in r.events if ev[0] == 'win')
        dets = [ev for ev in r.events if ev[0] == 'det']
        assert nd == len(dets)
        assert g['final_start'][t] == r.final_start
        for j, (_, start, maxi, d) in enumerate(dets):
            assert mine['det_start'][j] == start and mine['det_maxi'][j] == maxi
            assert abs(mine['det_d'][j] - d) <= 1e-9 * max(1.0, abs(d))
