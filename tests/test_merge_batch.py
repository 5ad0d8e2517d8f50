"""merge_rec (`-m m`) for a whole batch (spkd_merge_batch: an ahead pass over the adjacent pairs
of lines, then one device chain per file) against itself -- batch against alone, ahead pass
against none, problem order -- and, through pipeline.change_detect_batch(cd=MERGE_CD), against the
command line in `-m m` mode on each file's recipe alone.

Inputs: synth sessions whose truth turns are cut into pieces (the remainder stays with the last
piece), so that a turn is a run of several lines and the 2 s of silence between VAD groups are
gaps between lines.  Decisions checked on the CPU with oracle.numpy_engine behind
ChangeDetectionRun, at the thresholds used here (BIC lambda 1.3 t 0, GLR t 2500, KL2 t 150):
  make_session(31, 120, 3), pieces of 250: 50 lines, 3 gaps, 14 runs, the same decisions for all
      three distances, MM.MM.MM..MM.MMM..MMMMMM.MMMM.MMMMM..MMMMM.MMMM.M -- the chain starts with a
      merge (the frozen c1 of BIC comes from a pair that merged), ends with one, runs of up to 6
  make_session(33, 40, 2), pieces of 200: 19 lines, 6 runs
  make_session(32, 60, 1), pieces of 250: 24 lines, one gap; under BIC t 0 every step merges, so
      the one run spans the gap
Every GLR and KL2 distance of the merged chains is at least 45 % away from its threshold."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

from helpers import ROOT, assert_stdout_close
from conftest import pkg

MAXINT = 9223372036854775808.0
KINDS = ['BIC', 'GLR', 'KL2', 'KL2P']
WORKING = {'BIC': 0.0, 'GLR': 2500.0, 'KL2': 150.0, 'KL2P': 150.0}
ALL_MERGE, NONE_MERGES = 1e30, -1e30
SESSIONS = [((31, 120, 3), 250), ((33, 40, 2), 200), ((32, 60, 1), 250)]
DECISIONS_31 = 'MM.MM.MM..MM.MMM..MMMMMM.MMMM.MMMMM..MMMMM.MMMM.M'
SIZES = [0, 1, 2, 3, 19, 50]
NAN_PROBLEM, NAN_LINE = 2, 15             # of the four problems with more than one line: the 19-line one
COUNTERS = ['win_cnt', 'win_max', 'win_min', 'det_cnt', 'det_max', 'det_min']


def _pieces(truth, piece):
    out = []
    for a, b, _ in truth:
        p = a
        while b - p >= 2 * piece:
            out.append((p, p + piece))
            p += piece
        out.append((p, b))
    return out


def _sessions():
    synth = pkg('synth')
    out = []
    for args, piece in SESSIONS:
        feats, _, truth = synth.make_session(*args)
        out.append((feats, _pieces(truth, piece)))
    return out


# ------------------------------------------------------------------ not GPU
def test_the_sessions_are_the_documented_ones():
    lines = [l for _, l in _sessions()]
    assert [len(l) for l in lines] == [50, 19, 24]
    gaps = [sum(1 for (_, e), (b, _) in zip(l[:-1], l[1:]) if b > e) for l in lines]
    assert gaps[0] == 3 and gaps[2] == 1
    assert all(b >= e for l in lines for (_, e), (b, _) in zip(l[:-1], l[1:]))


def test_method_key_is_validated():
    pipeline = pkg('pipeline')
    m = pipeline.MERGE_CD
    assert (m['method'], m['kind'], m['lambdac'], m['threshold']) == ('m', 'GLR', 1.3, 0.0)
    assert pipeline.change_detect_batch(None, 0, 0, [], cd=m) == []
    assert pipeline.diarize_batch(None, 0, 0, [], cd=m) == []
    with pytest.raises(ValueError):
        pipeline.change_detect_batch(None, 0, 0, [], cd=m, fused=[])
    with pytest.raises(ValueError):
        pipeline.diarize_batch(None, 0, 0, [], cd=m, fused=True)
    with pytest.raises(ValueError):
        pipeline.diarize_batch(None, 0, 0, [], cd=m, handoff='device')
    with pytest.raises(ValueError):
        pipeline.change_detect_batch(None, 0, 0, [], cd=dict(m, method='merge'))
    # a file without a line gives no run, a file of one line dies as the script does, before any device work
    empty = pipeline.BatchFile(0, 100, [])
    assert pipeline.change_detect_batch(None, 0, 100, [empty], cd=m) == [[]]
    with pytest.raises(AttributeError, match="'function' object has no attribute 'prev'"):
        pipeline.change_detect_batch(None, 0, 100, [empty, pipeline.BatchFile(0, 100, [(0.0, 0.5)])], cd=m)
    with pytest.raises(ValueError):
        pipeline.change_detect_batch(None, 0, 100, [pipeline.BatchFile(0, 100, [(0.0, 0.5), (0.4, 0.8)])], cd=m)


def test_entry_point_is_declared_and_exported():
    hipabi = pkg('hipabi')
    text = open(os.path.join(ROOT, 'include', 'spkd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = hipabi.load_library()
    assert re.search(r'\bspkd_merge_batch\s*\(', code)
    assert 'spkd_merge_batch' in hipabi.EXPORTS and hasattr(lib, 'spkd_merge_batch')
    assert 'merge' in hipabi.TIMERS
    assert lib.spkd_abi_version() == 2
    # argument checks come before any device work: no context, no call
    off = np.array([0, 2], dtype=np.int64)
    b = np.array([0, 10], dtype=np.int64)
    e = np.array([10, 20], dtype=np.int64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    st = lib.spkd_merge_batch(None, None, 20, 1, ptr(off), ptr(b), ptr(e), 0, 1.3, 0.0, 0, *([None] * 9))
    assert st == hipabi.SPKD_EINVAL
    out = [np.zeros(2) for _ in range(9)]
    st = lib.spkd_merge_batch(None, None, 20, 1, ptr(off), ptr(b), ptr(e), 0, 1.3, 0.0, 0, *[ptr(a) for a in out])
    assert st == hipabi.SPKD_EINVAL


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def data():
    """The three sessions in one resident frame array, their lines dealt to the problems of SIZES;
    a problem's result alone (ctx.merge_batch on its lines only) is computed once per (kind,
    threshold, flags, problem) and shared."""
    engine = pkg('engine')
    hipabi = pkg('hipabi')
    sess = _sessions()
    frames = np.concatenate([f for f, _ in sess])
    starts = np.cumsum([0] + [f.shape[0] for f, _ in sess])
    l31, l33, l32 = [[(a + int(o), b + int(o)) for a, b in l] for (_, l), o in zip(sess, starts)]
    # (0) | 1 of 32 | 2 of 32 | 3 of 32, across its gap | the 19 of 33 | the 50 of 31
    gap = next(k for k in range(len(l32) - 1) if l32[k + 1][0] > l32[k][1])
    probs = [[], l32[0:1], l32[1:3], l32[gap - 1:gap + 2], l33, l31]
    assert [len(p) for p in probs] == SIZES
    eng = engine.HipEngine(0)
    eng.set_features(frames)
    d = dict(eng=eng, ctx=eng.ctx, hipabi=hipabi, frames=frames, probs=probs, alone={}, sess=sess)
    yield d
    eng.close()


def _call(d, probs, kind, thr, flags=0):
    off = np.zeros(len(probs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(p) for p in probs])
    flat = np.array([r for p in probs for r in p], dtype=np.int64).reshape(-1, 2)
    r = d['ctx'].merge_batch(d['eng'].d_frames, d['frames'].shape[0], off, flat[:, 0], flat[:, 1], kind, 1.3, thr, flags)
    r['off'] = off
    return r


def _alone(d, kind, thr, p, flags=0):
    key = (kind, thr, flags, p)
    if key not in d['alone']:
        d['alone'][key] = _call(d, [d['probs'][p]], kind, thr, flags)
    return d['alone'][key]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _assert_problem(got, q, want, tag):
    """Problem q of `got` equals the one problem of `want` to the bit."""
    o, n = int(got['off'][q]), int(got['off'][q + 1] - got['off'][q])
    assert int(want['off'][1]) == n, tag
    assert int(got['n_done'][q]) == int(want['n_done'][0]), tag
    assert np.array_equal(got['merged'][o:o + n], want['merged']), tag
    assert np.array_equal(_bits(got['dist'][o:o + n]), _bits(want['dist'])), tag
    for k in COUNTERS:
        assert np.array_equal(_bits(got[k][q:q + 1].astype(np.float64)), _bits(want[k].astype(np.float64))), (tag, k)


def _decisions(r, q=0):
    o, n = int(r['off'][q]), int(r['off'][q + 1] - r['off'][q])
    return ''.join('M' if m == 1 else '.' for m in r['merged'][o + 1:o + n])


def _behind_a_merge(r):
    """Steps whose predecessor merged: the ones the chain computes itself."""
    cnt = 0
    for q in range(len(r['off']) - 1):
        m = r['merged'][int(r['off'][q]):int(r['off'][q + 1])]
        cnt += int((m[1:-1] == 1).sum())
    return cnt


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['working', 'all_merge', 'none_merges'])
@pytest.mark.parametrize('kind', KINDS)
def test_batch_equals_alone_and_ahead_equals_no_ahead_to_the_bit(data, kind, which):
    hipabi = data['hipabi']
    thr = {'working': WORKING[kind], 'all_merge': ALL_MERGE, 'none_merges': NONE_MERGES}[which]
    got = _call(data, data['probs'], kind, thr)
    assert got['status'] == hipabi.SPKD_OK
    assert got['n_done'].tolist() == SIZES
    for p in range(len(SIZES)):
        _assert_problem(got, p, _alone(data, kind, thr, p), (kind, thr, p))
    # without the ahead pass every step computes its own terms: the same results to the bit
    slow = _call(data, data['probs'], kind, thr, hipabi.MERGE_NO_AHEAD)
    assert slow['status'] == hipabi.SPKD_OK
    for p in range(len(SIZES)):
        _assert_problem(slow, p, _alone(data, kind, thr, p), (kind, thr, p, 'no ahead'))
        _assert_problem(slow, p, _alone(data, kind, thr, p, hipabi.MERGE_NO_AHEAD), (kind, thr, p, 'no ahead, alone'))
    # empty problem, lone line: the counters stand where the script starts them
    o1 = int(got['off'][1])
    assert got['merged'][o1] == 0 and np.isnan(got['dist'][o1])
    for q in (0, 1):
        assert (got['win_cnt'][q], got['det_cnt'][q]) == (0, 0)
        assert (got['win_max'][q], got['win_min'][q], got['det_max'][q], got['det_min'][q]) == (0.0, MAXINT, 0.0, MAXINT)
    steps = sum(n - 1 for n in SIZES if n > 1)
    assert int(got['win_cnt'].sum()) == steps
    big = _decisions(got, 5)
    print('%s threshold %g: runs per problem %s, steps behind a merge %d of %d' % (
        kind, thr, [int((got['merged'][int(a):int(b)] == 0).sum()) for a, b in zip(got['off'][:-1], got['off'][1:])],
        _behind_a_merge(got), steps))
    if which == 'working':
        if kind != 'KL2P':
            assert big == DECISIONS_31
            assert _decisions(got, 4).count('.') == 5            # 19 lines, 6 runs
        assert 0 < big.count('M') < 49
    elif which == 'all_merge':
        assert int(got['det_cnt'].sum()) == steps and _behind_a_merge(got) == steps - 4
    else:
        assert int(got['det_cnt'].sum()) == 0 and _behind_a_merge(got) == 0
        assert got['det_min'].tolist() == [MAXINT] * len(SIZES)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_problem_order_does_not_matter(data, kind):
    hipabi = data['hipabi']
    for thr in (WORKING[kind], ALL_MERGE):
        got = _call(data, data['probs'][::-1], kind, thr)
        assert got['status'] == hipabi.SPKD_OK
        for q in range(len(SIZES)):
            p = len(SIZES) - 1 - q
            _assert_problem(got, q, _alone(data, kind, thr, p), (kind, thr, p))


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_a_nonfinite_line_stays_in_its_problem(data, kind):
    """One NaN frame inside a late line of one problem of four: the reference's det raises at the
    step that meets it; here that problem stops at that line and no other is touched."""
    hipabi = data['hipabi']
    eng = data['eng']
    probs = data['probs'][2:]
    a, b = probs[NAN_PROBLEM][NAN_LINE]
    bad = data['frames'].copy()
    bad[(a + b) // 2, 7] = np.nan
    thr = WORKING[kind]
    try:
        eng.set_features(bad)
        got = _call(data, probs, kind, thr)
    finally:
        eng.set_features(data['frames'])
    assert got['status'] == hipabi.SPKD_ENONFINITE
    assert int(got['n_done'][NAN_PROBLEM]) == NAN_LINE < SIZES[2 + NAN_PROBLEM]
    o = int(got['off'][NAN_PROBLEM])
    clean = _alone(data, kind, thr, 2 + NAN_PROBLEM)
    assert np.array_equal(got['merged'][o:o + NAN_LINE], clean['merged'][:NAN_LINE])
    assert np.array_equal(_bits(got['dist'][o:o + NAN_LINE]), _bits(clean['dist'][:NAN_LINE]))
    assert (got['merged'][o + NAN_LINE:o + 19] == -1).all() and np.isnan(got['dist'][o + NAN_LINE:o + 19]).all()
    for q in range(4):
        if q != NAN_PROBLEM:
            _assert_problem(got, q, _alone(data, kind, thr, 2 + q), (kind, q))


@pytest.mark.gpu
def test_argument_checks_on_a_context(data):
    hipabi = data['hipabi']
    ctx = data['ctx']
    nf = data['frames'].shape[0]
    df = data['eng'].d_frames
    r = ctx.merge_batch(df, nf, [0], [], [], 'BIC', 1.3, 0.0)                      # no problem at all
    assert r['status'] == hipabi.SPKD_OK and len(r['merged']) == 0 and len(r['n_done']) == 0
    r = ctx.merge_batch(df, nf, [0, 0, 0], [], [], 'GLR', 1.3, 0.0)                # only empty problems
    assert r['status'] == hipabi.SPKD_OK and r['n_done'].tolist() == [0, 0] and r['win_min'].tolist() == [MAXINT] * 2
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    i64 = lambda v: np.array(v, dtype=np.int64)
    good = dict(off=i64([0, 2, 3]), b=i64([0, 100, 300]), e=i64([100, 200, 400]), kind=0)
    cases = [dict(good, b=i64([0, 90, 300])),                   # overlapping lines
             dict(good, b=i64([150, 100, 300]), e=i64([250, 120, 400])),     # lines that go backwards
             dict(good, e=i64([100, 200, nf + 1])),             # a range past n_frames
             dict(good, e=i64([100, 99, 400])),                 # end < begin
             dict(good, b=i64([-1, 100, 300])),
             dict(good, off=i64([0, 3, 2])),                    # a decreasing line_off
             dict(good, kind=4), dict(good, kind=-1)]
    for k, cs in enumerate([good] + cases):
        out = [np.full(3, 77, dtype=np.int32), np.full(3, 77.0)] + [np.full(2, 77, dtype=np.int64), np.full(2, 77, dtype=np.int64),
               np.full(2, 77.0), np.full(2, 77.0), np.full(2, 77, dtype=np.int64), np.full(2, 77.0), np.full(2, 77.0)]
        st = ctx.lib.spkd_merge_batch(ctx.h, C.c_void_p(df), nf, 2, ptr(cs['off']), ptr(cs['b']), ptr(cs['e']), cs['kind'],
                                      1.3, 0.0, 0, *[ptr(a) for a in out])
        if k == 0:
            assert st == hipabi.SPKD_OK and out[2].tolist() == [2, 1]
        else:
            assert st == hipabi.SPKD_EINVAL, k
            assert all((a == 77).all() for a in out), k          # outputs untouched
    out = [np.zeros(3, dtype=np.int32), np.zeros(3)] + [np.zeros(2, dtype=np.int64) for _ in range(7)]
    args = [C.c_void_p(df), nf, 2, ptr(good['off']), ptr(good['b']), ptr(good['e']), 0, 1.3, 0.0, 0] + [ptr(a) for a in out]
    for k in (0, 3, 4, 5) + tuple(range(10, 19)):
        bad = list(args)
        bad[k] = None
        assert ctx.lib.spkd_merge_batch(ctx.h, *bad) == hipabi.SPKD_EINVAL, k


def _cli_merge(tmp, engine, lines, extra):
    """The change-detection command line in -m m mode on a recipe of `lines` -> (recipe text,
    stdout, error text or None)."""
    cli = pkg('cli')
    rin, rout = os.path.join(tmp, 'in.recipe'), os.path.join(tmp, 'out.recipe')
    with open(rin, 'w') as fh:
        fh.writelines(lines)
    if os.path.exists(rout):
        os.remove(rout)
    out = io.StringIO()
    err = None
    try:
        cli.main_change_detection([rin, os.path.join(tmp, 'fea') + '/', '-o', rout, '-m', 'm', '-tt'] + extra,
                                  engine=engine, stdout=out)
    except (ValueError, AttributeError) as e:
        err = str(e)
    return (open(rout).read() if os.path.exists(rout) else ''), out.getvalue(), err


def _cpu_oracle():
    try:
        from oracle.c_engine import COracleEngine
        return COracleEngine()
    except (ImportError, OSError):
        from oracle.numpy_engine import NumpyEngine
        return NumpyEngine()


@pytest.mark.gpu
def test_pipeline_merge_mode_equals_the_command_line(data, tmp_path):
    """change_detect_batch(cd=MERGE_CD) on the three sessions as three files of one batch (and a
    file without a line) against the command line in -m m mode on each file's recipe alone, with
    the library and with the CPU oracle behind it: the same output lines as text, the printed
    distances within the bounds of test_cluster_in_device_chain_equals_the_per_line_path (a chain
    of summed records against a per-line path)."""
    synth = pkg('synth')
    pipeline = pkg('pipeline')
    recipe = pkg('recipe')
    engine = pkg('engine')
    hipabi = data['hipabi']
    s2 = recipe.py2_float_str
    sess = data['sess']
    files, recipes, off = [], [], 0
    for i, (feats, lines) in enumerate(sess):
        v = [(float(s2(a / 125.0)), float(s2(b / 125.0))) for a, b in lines]
        files.append(pipeline.BatchFile(off, feats.shape[0], v))
        recipes.append(['audio=x.wav lna=a_%d start-time=%s end-time=%s speaker=spk_turn\n' % (j + 1, s2(a), s2(b))
                        for j, (a, b) in enumerate(v)])
        off += feats.shape[0]
        if i == 0:
            files.append(pipeline.BatchFile(off, 0, []))                   # a file without a line
    args = lambda: (data['ctx'], data['eng'].d_frames, data['frames'].shape[0], files)
    line_off, _, _, lb, le = pipeline._merge_lines(files, 125.0)
    cli_eng = engine.HipEngine(0)
    orc = _cpu_oracle()
    try:
        for i, (feats, _) in enumerate(sess):
            os.makedirs(os.path.join(str(tmp_path), 'f%d' % i, 'fea'))
            synth.write_fea(os.path.join(str(tmp_path), 'f%d' % i, 'fea', 'x.fea'), feats)
        for kind in ('BIC', 'GLR', 'KL2'):
            thr = WORKING[kind]
            cd = dict(pipeline.MERGE_CD, kind=kind, threshold=thr)
            tm = {}
            runs = pipeline.change_detect_batch(*args(), cd=cd, timings=tm)
            assert len(runs) == 4 and len(runs[1]) == 0
            raw = data['ctx'].merge_batch(args()[1], args()[2], line_off, lb, le, kind, 1.3, thr)
            raw['off'] = line_off
            assert tm['merge_lines'] == 93 and len(tm['merge']) == 1
            assert tm['merge_steps_behind_a_merge'] == _behind_a_merge(raw) > 0
            margins = []
            for i, k in enumerate((0, 2, 3)):
                tmp = os.path.join(str(tmp_path), 'f%d' % i)
                mine = [(s2(a), s2(b)) for a, b in np.asarray(runs[k]).tolist()]
                d_mine = raw['dist'][int(raw['off'][k]) + 1:int(raw['off'][k + 1])]
                margins.append(float(np.min(np.abs(d_mine - thr) / np.abs(d_mine))) if thr else float('nan'))
                texts = {}
                for tag, e in (('hip', cli_eng), ('orc', orc)):
                    text, stdout, err = _cli_merge(tmp, e, recipes[i], ['-d', kind, '-t', repr(thr)])
                    assert err is None, (kind, i, tag, err)
                    texts[tag] = stdout
                    want = re.findall(r'start-time=(\S+) end-time=(\S+)', text)
                    assert want == mine, (kind, i, tag)
                    d_cli = [float(x) for x in re.findall(r'- Distance: (\S+)', stdout)]
                    rel = (1e-7 if tag == 'hip' else 1e-4) if kind == 'KL2' else 1e-9
                    assert len(d_cli) == len(d_mine), (kind, i, tag)
                    for a, b in zip(d_mine.tolist(), d_cli):
                        assert abs(a - b) <= rel * max(1.0, abs(a), abs(b)), (kind, i, tag, a, b)
                assert_stdout_close(texts['hip'], texts['orc'], 1e-4 if kind == 'KL2' else 1e-9)
            print('%s threshold %g: runs %s, minimum margin per session %s' % (
                kind, thr, [len(r) for r in runs], ['%.3f' % m for m in margins]))
            assert [len(runs[k]) for k in (0, 2)] == [14, 6]
            if kind == 'BIC':
                # session 31: the frozen c1 comes from a pair that merged; session 32: every step merges,
                # and the one output line covers the silence between the two VAD groups
                assert _decisions(raw, 0) == DECISIONS_31
                assert len(runs[3]) == 1
                lines32 = sess[2][1]
                gap = next(k for k in range(len(lines32) - 1) if lines32[k + 1][0] > lines32[k][1])
                a, b = runs[3][0]
                assert a * 125 <= lines32[gap][1] and b * 125 >= lines32[gap + 1][0]
            else:
                assert all(m >= 0.45 for m in margins), margins
        # a NaN frame: the pipeline raises the reference's error
        bad = data['frames'].copy()
        bad[files[0].frame_off + sess[0][1][30][0] + 5, 3] = np.nan
        try:
            data['eng'].set_features(bad)
            with pytest.raises(ValueError, match='infs or NaNs'):
                pipeline.change_detect_batch(*args(), cd=dict(pipeline.MERGE_CD, threshold=WORKING['GLR']))
        finally:
            data['eng'].set_features(data['frames'])
        one = [files[0], pipeline.BatchFile(files[2].frame_off, files[2].n_frames, files[2].vad[:1])]
        with pytest.raises(AttributeError, match="'function' object has no attribute 'prev'"):
            pipeline.change_detect_batch(*args()[:3], one, cd=pipeline.MERGE_CD)
    finally:
        cli_eng.close()
