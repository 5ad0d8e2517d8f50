"""Sliding-window change detection for a whole batch (spkd_sw_batch / spkd_sw_runs): the distances
against the single-call path they share their sums with (spkd_sw), bit for bit and whatever the
tiling; the positive-run state machine on planted distances against the host restatement of the
script (ChangeDetectionRun._sw_postpass); `cd['method'] = 'sw'` of the batch pipeline against the
reference's goldens and against the command line."""
import ctypes as C
import io
import json
import math
import os
import re

import numpy as np
import pytest

from helpers import ROOT, cli, load_cases, session, synth
from conftest import pkg

NAN, INF = float('nan'), float('inf')
MAXINT_F = 9223372036854775808.0              # float(sys.maxint): where the script's minima start
KINDS = ['GLR', 'BIC', 'KL2', 'KL2P']
SIZE, STEP = 250, 31                          # -w 2.0 -st 0.25 at 125 frames / s
# windows per turn: none (one frame short of two windows), none (a turn without a frame), 1, 2, 41
TURN_LENS = [2 * SIZE - 1, 0, 2 * SIZE, 2 * SIZE + STEP, 2 * SIZE + 40 * STEP]
TURN_WINDOWS = [0, 0, 1, 2, 41]
EVENT_KEYS = ('n_det', 'det_start', 'det_maxi', 'det_d', 'final_start', 'win_cnt', 'win_max', 'win_min',
              'det_max', 'det_min')

with open(os.path.join(ROOT, 'tests', 'golden', 'kl2_pinv_cases.json')) as _f:
    _PCASES = {c['name']: c for c in json.load(_f)['cases']}
_CASES = {c['name']: c for c in load_cases()}


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------ not GPU
def test_method_key_is_validated():
    pipeline = pkg('pipeline')
    bad = dict(pipeline.SW_CD, method='sliding')
    with pytest.raises(ValueError):
        pipeline.change_detect_batch(None, 0, 0, [], cd=bad)
    with pytest.raises(ValueError):
        pipeline.diarize_batch(None, 0, 0, [], cd=bad)
    with pytest.raises(ValueError):
        pipeline.diarize_batch(None, 0, 0, [], cd=pipeline.SW_CD, fused=True)
    with pytest.raises(ValueError):
        pipeline.change_detect_batch(None, 0, 0, [], cd=pipeline.SW_CD, fused=[])
    with pytest.raises(ValueError):
        pipeline.diarize_batch(None, 0, 0, [], cd=pipeline.SW_CD, handoff='device')
    assert pipeline.change_detect_batch(None, 0, 0, [], cd=pipeline.SW_CD) == []
    assert pipeline.diarize_batch(None, 0, 0, [], cd=pipeline.SW_CD) == []
    assert pipeline.diarize_batch(None, 0, 0, [], cd=dict(pipeline.DIA2_CD, method='gw')) == []
    assert 'method' not in pipeline.DIA2_CD
    assert pipeline.SW_CD == dict(method='sw', kind='GLR', lambdac=1.3, threshold=0.0, winsize_s=5.0,
                                  winstep_s=0.5, deltaws_s=0.05)


def test_entry_points_are_declared_and_exported():
    hipabi = pkg('hipabi')
    text = open(os.path.join(ROOT, 'include', 'spkd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = hipabi.load_library()
    for name in ('spkd_sw_runs', 'spkd_sw_batch'):
        assert re.search(r'\b%s\s*\(' % name, code)
        assert name in hipabi.EXPORTS and hasattr(lib, name)
    assert lib.spkd_abi_version() == 2
    # argument checks come before any device work: no context, no call
    p = hipabi.CdParams(1, 0, 1.3, 0.0, 250.0, 31.0, 6.0, 125.0)
    off = np.array([0, 1], dtype=np.int64)
    o = off.ctypes.data_as(C.c_void_p)
    assert lib.spkd_sw_runs(None, None, o, 1, C.byref(p), o, *[None] * 10) == hipabi.SPKD_EINVAL
    assert lib.spkd_sw_batch(None, None, 500, o, o, 1, C.byref(p), o, o, 0, *[None] * 11) == hipabi.SPKD_EINVAL


def test_window_count_of_whole_frame_geometry():
    """spkd_sw_window_count: the script's loop, `s = 0; while s + 2 * size <= len: s += step`."""
    lib = pkg('hipabi').load_library()
    for size, step in ((250.0, 31.0), (1.0, 1.0), (625.0, 62.0), (2.5, 1.5)):
        for n in (0, 1, 2, 3, 499, 500, 501, 530, 531, 1250, 1311, 1312, 450000):
            w, s = 0, 0.0
            while s + 2 * size <= n:
                w, s = w + 1, s + step
            assert lib.spkd_sw_window_count(n, size, step) == w, (size, step, n)
    assert lib.spkd_sw_window_count(10, 0.5, 1.0) == -1 and lib.spkd_sw_window_count(10, 1.0, 0.5) == -1


# ------------------------------------------------------------------ GPU
def _edited(meta):
    """The frames of a kl2_pinv_cases.json session: synth.make_session, then the zeroed ranges."""
    f = session(meta)[0].copy()
    for b, e in meta['edits']['zero']:
        f[b:e] = 0.0
    assert synth.fea_sha256(f) == meta['edited_sha256']
    return f


@pytest.fixture(scope='module')
def data():
    """The 150 s session of A_cd_sw_glr and the 120 s session of P_cd_sw_kl2 as one resident batch."""
    engine, hipabi = pkg('engine'), pkg('hipabi')
    fa = session(_CASES['A_cd_sw_glr']['session'])[0]
    fp = _edited(_PCASES['P_cd_sw_kl2']['session'])
    assert fa.shape[0] == 18750 and fp.shape[0] == 15000
    frames = np.concatenate([fa, fp])
    eng = engine.HipEngine(0)
    eng.set_features(frames)
    d = dict(eng=eng, ctx=eng.ctx, hipabi=hipabi, frames=frames, fa=fa, fp=fp, cli={})
    yield d
    eng.close()


def _turns(begin0, lens, gap=7):
    b, pos = [], begin0
    for n in lens:
        b.append(pos)
        pos += n + gap
    b = np.array(b, dtype=np.int64)
    return b, b + np.array(lens, dtype=np.int64)


def _params(hipabi, kind, size, step, thr=0.0):
    return hipabi.CdParams(hipabi.KINDS[kind], 0, 1.3, thr, float(size), float(step), 6.0, 125.0)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_distances_equal_the_single_call_to_the_bit(data, kind):
    hipabi, ctx, eng = data['hipabi'], data['ctx'], data['eng']
    b, e = _turns(300, TURN_LENS)
    assert int(e[-1]) <= 18750                       # ordinary speech: every covariance is regular
    thr = {'GLR': 1800.0, 'BIC': 0.0, 'KL2': 12.0, 'KL2P': 12.0}[kind]
    p = _params(hipabi, kind, SIZE, STEP, thr)
    st, off, want = ctx.sw(eng.d_frames, eng.n_frames, b, e, p)
    assert st == hipabi.SPKD_OK and np.diff(off).tolist() == TURN_WINDOWS
    assert np.isfinite(want).all() and len(set(want.tolist())) == len(want)
    got = {}
    # 1: a seam behind every window; 3: one on the edge between the 2- and the 41-window turn
    # (windows 0 | 1 2 | 3 ..) and more inside the last; 0: the default, one tile
    for tile in (1, 3, 0):
        r = got[tile] = ctx.sw_batch(eng.d_frames, eng.n_frames, b, e, p, tile_windows=tile, want_d=True)
        assert r['status'] == hipabi.SPKD_OK
        assert np.array_equal(r['d_off'], off)
        assert np.array_equal(_bits(r['d']), _bits(want)), (kind, tile)
    for tile in (1, 3):
        for k in EVENT_KEYS:
            assert got[tile][k].tobytes() == got[0][k].tobytes(), (kind, tile, k)
    r = got[0]
    assert r['n_det'][:2].tolist() == [0, 0] and r['final_start'][:2].tolist() == [0.0, 0.0]
    assert r['win_cnt'].tolist() == TURN_WINDOWS
    print('%s: detections per turn %s' % (kind, r['n_det'].tolist()))


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_halves_longer_than_a_chunk_sum_in_chunk_order(data, kind):
    """size 1100 > STATS_CHUNK = 1024: every half is two chunks, added as k_reduce_sets adds them."""
    hipabi, ctx, eng = data['hipabi'], data['ctx'], data['eng']
    b, e = _turns(4000, [2450, 2199])
    p = _params(hipabi, kind, 1100, 100)
    st, off, want = ctx.sw(eng.d_frames, eng.n_frames, b, e, p)
    assert st == hipabi.SPKD_OK and np.diff(off).tolist() == [3, 0] and np.isfinite(want).all()
    for tile in (2, 0):
        r = ctx.sw_batch(eng.d_frames, eng.n_frames, b, e, p, tile_windows=tile, want_d=True)
        assert r['status'] == hipabi.SPKD_OK
        assert np.array_equal(_bits(r['d']), _bits(want)), (kind, tile)


class _Recorder(object):
    def __init__(self):
        self.lines = []

    def write(self, recline, start_frames, end_frames, lna_start, speaker):
        self.lines.append((float(start_frames), float(end_frames)))


def _host_runs(rows, thr):
    """_sw_postpass over every row with a recording writer, a fresh set of counters per turn."""
    cd = pkg('change_detection')
    want = []
    for row in rows:
        run = cd.ChangeDetectionRun(None, cd.CDOptions(rate=125, winsize_s=2.0, winstep_s=0.25, threshold=thr), '')
        assert run.o.winsize == SIZE and run.o.winstep == STEP
        n = 2 * SIZE + (len(row) - 1) * STEP if len(row) else 2 * SIZE - 1
        w = _Recorder()
        run._sw_postpass(('x.wav', 'a_1', 1.0, 1.0 + n / 125.0), n, row, w)
        want.append(dict(lines=w.lines, cnt=run.total_windows, wmax=float(run.max_dist), wmin=float(run.min_dist),
                         nd=run.total_segments, dmax=float(run.max_det_dist), dmin=float(run.min_det_dist)))
    return want


# threshold 5
ROWS = [
    [1.0, 2.0, 3.0, -1.0],                        # no positive at all
    [1.0, 7.0, 9.0, 8.0],                         # a series that ends with the turn
    [7.0, 9.0, 1.0, 6.0, 12.0, 11.0, 0.0],        # two series
    [1.0, NAN, 1.0],                              # a NaN-only series: best_position = -1 is written
    [1.0, NAN, NAN],                              # the same, ending with the turn
    [6.0, NAN, 9.0, 1.0],                         # NaN inside a series
    [NAN, 6.0, 1.0, NAN, 2.0],                    # NaN first: the second series writes the stale position
    [INF, 7.0, -INF, 8.0, INF, 9.0],              # +-inf are negative windows and count for nothing
    [5.0, 1.0, 5.0, 4.999],                       # d == threshold is positive
    [9.0, 9.0, 1.0, 8.0, 8.0, 8.0, 0.0],          # equal maxima: the first wins
    [7.0],                                        # a single window, positive
    [1.0],                                        # a single window, negative
    [],                                           # no window
    [6.0 + (i % 7) if i % 11 else 0.0 for i in range(150)],      # past two stages of 64
]
# threshold -2: after the first series bestd is 0, and a series at or below 0 never beats it
ROWS_NEGATIVE_THRESHOLD = [
    [3.0, -5.0, -1.0, -1.5, -5.0, 0.0, -2.0, -3.0],
    [-1.0, -1.5, -3.0, -0.5],
    [-2.5, -3.0],
]


@pytest.mark.gpu
@pytest.mark.parametrize('rows,thr', [(ROWS, 5.0), (ROWS_NEGATIVE_THRESHOLD, -2.0)], ids=['thr5', 'thr-2'])
def test_state_machine_on_planted_distances(data, rows, thr):
    hipabi, ctx = data['hipabi'], data['ctx']
    want = _host_runs(rows, thr)
    d_off = np.zeros(len(rows) + 1, dtype=np.int64)
    d_off[1:] = np.cumsum([len(r) for r in rows])
    flat = np.array([x for r in rows for x in r], dtype=np.float64)
    d_dist = ctx.dev_alloc(max(flat.nbytes, 16))
    try:
        ctx.h2d(d_dist, flat)
        got = ctx.sw_runs(d_dist, d_off, _params(hipabi, 'GLR', SIZE, STEP, thr))
    finally:
        ctx.dev_free(d_dist)
    assert got['status'] == hipabi.SPKD_OK
    assert np.diff(got['off']).tolist() == [len(r) // 2 + 1 for r in rows]
    for t, (row, w) in enumerate(zip(rows, want)):
        o, nd = int(got['off'][t]), int(got['n_det'][t])
        assert nd == w['nd'] == len(w['lines']) - 1, t
        starts = got['det_start'][o:o + nd]
        ends = starts + got['det_maxi'][o:o + nd]
        assert list(zip(starts.tolist(), ends.tolist())) == w['lines'][:-1], (t, row)
        assert float(got['final_start'][t]) == w['lines'][-1][0], t
        # det_d: what _detection_stat saw -- its maximum and minimum pin the values down with the count
        assert int(got['win_cnt'][t]) == w['cnt'], t
        for k, kw in (('win_max', 'wmax'), ('win_min', 'wmin'), ('det_max', 'dmax'), ('det_min', 'dmin')):
            assert np.array_equal(_bits(got[k][t:t + 1]), _bits([w[kw]])), (t, k, got[k][t], w[kw])
        dd = got['det_d'][o:o + nd]
        if nd:
            assert max(0.0, dd.max()) == w['dmax'] and min(MAXINT_F, dd.min()) == w['dmin'], t
    if thr == 5.0:
        assert want[3]['lines'][0] == (0.0, -1.0) and got['det_d'][int(got['off'][3])] == -1.0
        assert want[6]['lines'][1][1] == want[6]['lines'][0][1]                 # the stale position
        assert want[9]['lines'][0][1] == 0.0 + SIZE and want[9]['lines'][1][1] == 3.0 * STEP + SIZE
        assert got['n_det'][12] == 0 and got['win_min'][12] == MAXINT_F
    else:
        assert want[0]['nd'] == 3 and want[0]['lines'][1][1] == want[0]['lines'][0][1]      # the stale position
    # the event layout gives the script's lines: through gw_lines and the 12-digit round trip
    nt = len(rows)
    ls = np.full(nt, 1.0)
    n = np.array([2 * SIZE + (len(r) - 1) * STEP if len(r) else 2 * SIZE - 1 for r in rows], dtype=np.int64)
    le = 1.0 + n / 125.0
    lines = hipabi.gw_lines(got['off'][:-1], got['n_det'], got['det_start'], got['det_maxi'], got['final_start'],
                            ls, le, np.zeros(nt, dtype=np.int64), n, 125.0)
    rec = pkg('recipe')
    text = [(float(rec.py2_float_str(a / 125.0 + 1.0)), float(rec.py2_float_str(b / 125.0 + 1.0)))
            for w in want for (a, b) in w['lines']]
    assert [tuple(x) for x in lines['times'].tolist()] == text


def _vad(case):
    rec = pkg('recipe')
    return [(r[2], r[3]) for r in rec.parse_recipe(case['input_recipe'].splitlines(True))]


def _times(text):
    rec = pkg('recipe')
    return [(r[2], r[3]) for r in rec.parse_recipe(text.splitlines(True))]


def _cli_cd(data, tmp_path, which, flags):
    """cli.main_change_detection with `flags` on one session ('A' / 'P') -> (recipe text, directory)."""
    key = (which, tuple(flags))
    if key not in data['cli']:
        case = _CASES['A_cd_sw_glr'] if which == 'A' else _PCASES['P_cd_sw_kl2']
        feats = data['fa'] if which == 'A' else data['fp']
        tmp = os.path.join(str(tmp_path), '%s_%d' % (which, len(data['cli'])))
        os.makedirs(os.path.join(tmp, 'fea'))
        synth.write_fea(os.path.join(tmp, 'fea', os.path.splitext(case['audio'])[0] + '.fea'), feats)
        with open(os.path.join(tmp, 'in.recipe'), 'w') as f:
            f.write(case['input_recipe'])
        out = os.path.join(tmp, 'cd.recipe')
        eng = pkg('engine').HipEngine(0, kl2_pinv='--kl2-pinv' in flags)
        try:
            cli.main_change_detection([os.path.join(tmp, 'in.recipe'), os.path.join(tmp, 'fea') + '/', '-o', out]
                                      + list(flags), engine=eng, stdout=io.StringIO())
        finally:
            eng.close()
        data['cli'][key] = (open(out).read(), tmp)
    return data['cli'][key]


def _files(data):
    pipeline = pkg('pipeline')
    return [pipeline.BatchFile(0, 18750, _vad(_CASES['A_cd_sw_glr'])),
            pipeline.BatchFile(18750, 15000, _vad(_PCASES['P_cd_sw_kl2']))]


GOLDEN_RUNS = {
    # name: (cd, command-line flags, the golden's file, the golden, its lines)
    'A_cd_sw_glr': (dict(threshold=3000.0), ['-t', '3000'], 0, _CASES['A_cd_sw_glr'], 15),
    'P_cd_sw_kl2': (dict(kind='KL2P', winsize_s=2.0, winstep_s=0.25, threshold=25.0),
                    ['-m', 'sw', '-d', 'KL2', '-w', '2.0', '-st', '0.25', '-t', '25', '--kl2-pinv'], 1,
                    _PCASES['P_cd_sw_kl2'], 26),
    'A_cd_sw_kl2': (dict(kind='KL2', winsize_s=2.0, winstep_s=0.25, threshold=25.0),
                    ['-m', 'sw', '-d', 'KL2', '-w', '2.0', '-st', '0.25', '-t', '25'], 0, _CASES['A_cd_sw_kl2'], 16),
}


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(GOLDEN_RUNS))
def test_pipeline_equals_the_reference_goldens(data, tmp_path, name):
    pipeline = pkg('pipeline')
    over, flags, own, case, n_lines = GOLDEN_RUNS[name]
    assert list(case['argv_tail']) == [f for f in flags if f != '--kl2-pinv']
    cd = dict(pipeline.SW_CD, **over)
    tm = {}
    got = pipeline.change_detect_batch(data['ctx'], data['eng'].d_frames, 33750, _files(data), cd=cd, timings=tm)
    want = _times(case['output_recipe'])
    assert len(want) == n_lines
    assert [tuple(x) for x in np.asarray(got[own]).tolist()] == want
    other = _times(_cli_cd(data, tmp_path, 'P' if own == 0 else 'A', flags)[0])
    assert len(other) > 5
    assert [tuple(x) for x in np.asarray(got[1 - own]).tolist()] == other
    # the timings entries: the script's window loop and slices, turn by turn
    size, step = math.floor(cd['winsize_s'] * 125.0), math.floor(cd['winstep_s'] * 125.0)
    windows = frames = 0
    for f in _files(data):
        for ls, le in f.vad:
            f0 = min(int(ls * 125.0), f.n_frames)
            n = max(f0, min(int(le * 125.0), f.n_frames)) - f0
            frames += n
            start = 0
            while start + 2 * size <= n:
                windows, start = windows + 1, start + step
    assert len(tm['sw']) == 1 and tm['sw'][0] > 0.0
    assert tm['sw_windows'] == windows > 0 and tm['sw_frames'] == frames


@pytest.mark.gpu
@pytest.mark.parametrize('method', ['hi', 'in'])
def test_whole_pipeline_equals_the_command_lines(data, tmp_path, method):
    pipeline = pkg('pipeline')
    s2 = pkg('recipe').py2_float_str
    cd = dict(pipeline.SW_CD, threshold=3000.0)
    cl = dict(pipeline.DIA2_CL, method=method)
    got = pipeline.diarize_batch(data['ctx'], data['eng'].d_frames, 33750, _files(data), cd=cd, cl=cl)
    eng = pkg('engine').HipEngine(0)
    try:
        for k, which in enumerate('AP'):
            text, tmp = _cli_cd(data, tmp_path, which, ['-t', '3000'])
            out = os.path.join(tmp, 'cl_%s.recipe' % method)
            cli.main_clustering([os.path.join(tmp, 'cd.recipe'), os.path.join(tmp, 'fea') + '/', '-o', out,
                                 '-m', method, '-l', '1.3'], variant=1, engine=eng, stdout=io.StringIO())
            want = re.findall(r'start-time=(\S+) end-time=(\S+) speaker=speaker_(\d+)', open(out).read())
            assert len(want) == text.count('\n') > 5
            assert [(s2(a), s2(b), str(int(c))) for a, b, c in got[k].tolist()] == want, (method, which)
            assert len(set(c for _, _, c in want)) > 1
    finally:
        eng.close()


@pytest.mark.gpu
def test_errors(data):
    hipabi, ctx, eng = data['hipabi'], data['ctx'], data['eng']
    pipeline = pkg('pipeline')
    files = _files(data)
    # BIC under sw follows the script: it dies on the first turn with a window ...
    with pytest.raises(ValueError, match='array must not contain infs or NaNs'):
        pipeline.change_detect_batch(ctx, eng.d_frames, 33750, files, cd=dict(pipeline.SW_CD, kind='BIC'))
    # ... and writes every turn as one line when none has (windows longer than the longest turn)
    got = pipeline.change_detect_batch(ctx, eng.d_frames, 33750, files, cd=dict(pipeline.SW_CD, kind='BIC', winsize_s=30.0))
    for g, f in zip(got, files):
        assert [tuple(x) for x in np.asarray(g).tolist()] == f.vad
    b, e = _turns(300, TURN_LENS)
    p = _params(hipabi, 'GLR', SIZE, STEP)
    d_off = np.zeros(len(b) + 1, dtype=np.int64)
    d_off[1:] = np.cumsum(TURN_WINDOWS)
    ev_off = np.zeros(len(b) + 1, dtype=np.int64)
    ev_off[1:] = np.cumsum([w // 2 + 1 for w in TURN_WINDOWS])
    short = ev_off.copy()
    short[-1] -= 1                                   # the last turn one slot short of the bound
    wrong = d_off.copy()
    wrong[-1] += 1                                   # off by one window
    for kw in (dict(ev_off=short), dict(d_off=wrong), dict(tile_windows=-1)):
        with pytest.raises(hipabi.SpkdError) as ei:
            ctx.sw_batch(eng.d_frames, eng.n_frames, b, e, p, **kw)
        assert ei.value.status == hipabi.SPKD_EINVAL, kw
        assert ctx.last_ms('sw') >= 0.0
    for bad in (_params(hipabi, 'GLR', 0.5, STEP), _params(hipabi, 'GLR', SIZE, 0.5),
                hipabi.CdParams(9, 0, 1.3, 0.0, float(SIZE), float(STEP), 6.0, 125.0)):
        with pytest.raises(hipabi.SpkdError) as ei:
            ctx.sw_batch(eng.d_frames, eng.n_frames, b, e, bad, d_off=d_off, ev_off=ev_off)
        assert ei.value.status == hipabi.SPKD_EINVAL
    with pytest.raises(hipabi.SpkdError) as ei:
        ctx.sw_batch(eng.d_frames, eng.n_frames, b, e + 40000, p, d_off=d_off, ev_off=ev_off)
    assert ei.value.status == hipabi.SPKD_EINVAL
    with pytest.raises(hipabi.SpkdError) as ei:
        ctx.sw_runs(0, d_off, p, ev_off=short)
    assert ei.value.status == hipabi.SPKD_EINVAL
    assert ctx.sw_batch(eng.d_frames, eng.n_frames, b, e, p, d_off=d_off, ev_off=ev_off)['status'] == hipabi.SPKD_OK
    # one NaN frame inside a turn
    nan = data['frames'].copy()
    nan[int(b[-1]) + 700, 5] = NAN
    try:
        eng.set_features(nan)
        r = ctx.sw_batch(eng.d_frames, eng.n_frames, b, e, p)
        assert r['status'] == hipabi.SPKD_ENONFINITE
        nan[int(b[-1]) + 700, 5] = 0.0
        nan[2000, 5] = NAN                           # inside the first VAD turn of the first file
        eng.set_features(nan)
        with pytest.raises(ValueError, match='array must not contain infs or NaNs'):
            pipeline.change_detect_batch(ctx, eng.d_frames, 33750, files, cd=pipeline.SW_CD)
    finally:
        eng.set_features(data['frames'])
