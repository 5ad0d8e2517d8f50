"""Head and rest of a batch clustering call (include/spkd.h, SPKD_AHC_HEAD): the K largest problems get their
matrices first and run their merge loops on a side stream, beside the matrices of the others.  Only the order
of the launches differs, so every output is that of SPKD_AHC_HEAD=0 to the bit, the call still returns with
its work finished whatever the status, and the scratch is reusable at once."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg

gpu = pytest.mark.gpu

UNEVEN = [1, 2, 3, 5, 9, 17, 40, 70, 130]            # one call; with K = 2 the head is the last two problems
TWENTY = [30 + (7 * i) % 31 for i in range(20)]      # 30 .. 60 records
THRESHOLD = {'BIC': 0.0, 'GLR': 2500.0, 'KL2': 12.0}
NAN_HEAD, NAN_REST = 8, 4                            # problems of UNEVEN that get a NaN frame


def _seg_off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _sets(segs, sizes):
    """Problem k: sizes[k] segments from the k-th on (problems may share segments; they never share records)."""
    out = []
    for k, n in enumerate(sizes):
        out += [[s] for s in segs[3 * k:3 * k + n]]
    return out


@pytest.fixture(scope='module')
def records():
    """The statistics records of the problems, computed once and kept on the host: 'uneven' and 'twenty' clean,
    'nan_head' / 'nan_rest' as 'uneven' with one NaN frame inside a record of problem NAN_HEAD / NAN_REST."""
    synth = pkg('synth')
    hipabi = pkg('hipabi')
    eng = pkg('engine').HipEngine(0)
    feats, _, truth = synth.make_session(4242, 2400, 4)
    segs = [(a, b) for a, b, _ in truth]
    assert len(segs) >= 3 * len(UNEVEN) + max(UNEVEN) and len(segs) >= 3 * len(TWENTY) + max(TWENTY)
    out = {}

    def host_records(f, sets):
        eng.set_features(f)
        d = eng._stats_of_sets(sets)
        try:
            h = np.empty((len(sets), hipabi.REC), dtype=np.float64)
            eng.ctx.d2h(h, d)
        finally:
            eng.ctx.dev_free(d)
        return h

    try:
        out['uneven'] = host_records(feats, _sets(segs, UNEVEN))
        out['twenty'] = host_records(feats, _sets(segs, TWENTY))
        off = _seg_off(UNEVEN)
        for name, p in (('nan_head', NAN_HEAD), ('nan_rest', NAN_REST)):
            h = out['uneven'].copy()
            seg = _sets(segs, UNEVEN)[int(off[p]) + 1][0]            # the problem's second record
            f = feats.copy()
            f[seg[0] + 2, 5] = np.nan
            bad = host_records(f, [[seg]])
            assert np.isnan(bad).any()
            h[int(off[p]) + 1] = bad[0]
            out[name] = h
    finally:
        eng.close()
    return out


def _calls(monkeypatch, head, rec, sizes, params, repeat=1):
    """A fresh context under SPKD_AHC_HEAD = head (None: unset): spkd_ahc over the records for every (variant,
    kind, max_spk) of params, `repeat` times each -> the results in call order, each with its message and K."""
    hipabi = pkg('hipabi')
    if head is None:
        monkeypatch.delenv('SPKD_AHC_HEAD', raising=False)
    else:
        monkeypatch.setenv('SPKD_AHC_HEAD', str(head))
    ctx = hipabi.Context(0)                               # (the switch is read when the context is made)
    seg_off = _seg_off(sizes)
    out = []
    try:
        d = ctx.dev_alloc(rec[0].nbytes)
        for h, (variant, kind, max_spk) in zip(rec, params):
            ctx.h2d(d, h)
            p = hipabi.AhcParams(variant, hipabi.KINDS[kind], max_spk, hipabi.AHC_MONO, 1.3, THRESHOLD[kind])
            for _ in range(repeat):
                r = ctx.ahc(d, seg_off, p)
                r['message'] = ctx.lib.spkd_last_error(ctx.h) if r['status'] else b''
                r['head'] = ctx.last_ahc_head()
                out.append(r)
        ctx.dev_free(d)
    finally:
        ctx.close()
    return out


def _same(a, b, sizes, labels=True):
    hipabi = pkg('hipabi')
    seg_off = _seg_off(sizes)
    assert a['status'] == b['status'] and a['message'] == b['message']
    assert np.array_equal(a['n_merges'], b['n_merges'])
    for k in range(len(sizes)):
        lo, hi = int(seg_off[k]), int(seg_off[k]) + int(a['n_merges'][k])
        assert np.array_equal(a['a'][lo:hi], b['a'][lo:hi]) and np.array_equal(a['b'][lo:hi], b['b'][lo:hi])
        assert a['d'][lo:hi].tobytes() == b['d'][lo:hi].tobytes(), k
    assert a['stat_max'].tobytes() == b['stat_max'].tobytes() and a['stat_min'].tobytes() == b['stat_min'].tobytes()
    if labels:
        la = hipabi.labels_from_merges_batch(seg_off, a['n_merges'], a['a'], a['b'])
        lb = hipabi.labels_from_merges_batch(seg_off, b['n_merges'], b['a'], b['b'])
        assert np.array_equal(la, lb)


@gpu
@pytest.mark.parametrize('kind', ['BIC', 'GLR', 'KL2'])
@pytest.mark.parametrize('variant', [1, 2])
def test_uneven_problems_do_not_depend_on_the_head(records, monkeypatch, variant, kind):
    """Problems of 1 .. 130 records in one call: no head, one problem, two, eight, all nine (the rest empty) and
    the rule's choice; without and with -ms."""
    params = [(variant, kind, 0), (variant, kind, 3)]
    rec = [records['uneven']] * len(params)
    want = _calls(monkeypatch, 0, rec, UNEVEN, params)
    assert all(r['status'] == 0 and r['head'] == 0 for r in want)
    assert int(want[0]['n_merges'][-1]) > 60 and int(want[1]['n_merges'][-1]) == UNEVEN[-1] - 3
    for head in (1, 2, 8, 9, None):
        got = _calls(monkeypatch, head, rec, UNEVEN, params)
        for g, w in zip(got, want):
            assert g['head'] == (0 if head is None else head)         # (nine problems: the rule leaves them alone)
            _same(g, w, UNEVEN)


@gpu
@pytest.mark.parametrize('kind,variant', [('BIC', 1), ('GLR', 2)])
def test_twenty_problems_with_more_and_fewer_head_problems_than_xcds(records, monkeypatch, kind, variant):
    params = [(variant, kind, 0), (variant, kind, 2)]
    rec = [records['twenty']] * len(params)
    want = _calls(monkeypatch, 0, rec, TWENTY, params)
    assert all(r['status'] == 0 for r in want) and int(want[0]['n_merges'].min()) > 5
    for head in (12, 3, None):
        got = _calls(monkeypatch, head, rec, TWENTY, params)
        for g, w in zip(got, want):
            assert 0 <= g['head'] <= 20 and (head is None or g['head'] == head)
            _same(g, w, TWENTY)


@gpu
@pytest.mark.parametrize('where', ['nan_head', 'nan_rest'])
def test_nan_frame_reports_as_without_a_head_and_leaves_the_context_usable(records, monkeypatch, where):
    """A NaN frame in a record of a head problem / of a rest problem: status and message of the single launches;
    the clean call behind it on the same context gives the clean result (the side stream was drained, the
    scratch is reusable)."""
    hipabi = pkg('hipabi')
    params = [(1, 'BIC', 0), (1, 'BIC', 0)]
    rec = [records[where], records['uneven']]
    want = _calls(monkeypatch, 0, rec, UNEVEN, params)
    assert want[0]['status'] == hipabi.SPKD_ENONFINITE and b'infs or NaNs' in want[0]['message']
    assert want[1]['status'] == 0
    got = _calls(monkeypatch, 2, rec, UNEVEN, params)
    assert got[0]['head'] == 2
    _same(got[0], want[0], UNEVEN, labels=False)
    _same(got[1], want[1], UNEVEN)


@gpu
def test_the_same_call_three_times_on_one_context(records, monkeypatch):
    got = _calls(monkeypatch, 2, [records['uneven']], UNEVEN, [(1, 'BIC', 0)], repeat=3)
    assert len(got) == 3 and got[0]['status'] == 0 and got[0]['head'] == 2
    _same(got[1], got[0], UNEVEN)
    _same(got[2], got[0], UNEVEN)


@gpu
def test_fused_batch_rows_do_not_depend_on_the_head(monkeypatch):
    """pipeline.diarize_batch(fused=True) over six synthetic files of 60 .. 180 s, one workgroup per file."""
    torch = pytest.importorskip('torch')
    sd = pkg('synth_device')
    pipeline = pkg('pipeline')
    recipe = pkg('recipe')
    hipabi = pkg('hipabi')
    parts, files, off = [], [], 0
    for i, secs in enumerate((60, 85, 110, 130, 155, 180)):
        feats, vad, _ = sd.make_session_device(520000 + i, secs, 3, device='cuda')
        v = [(float(recipe.py2_float_str(a / 125.0)), float(recipe.py2_float_str(b / 125.0))) for a, b in vad]
        files.append(pipeline.BatchFile(off, feats.shape[0], v))
        parts.append(feats)
        off += feats.shape[0]
    frames = torch.cat(parts)
    torch.cuda.synchronize()
    cl = dict(pipeline.DIA2_CL, path=hipabi.AHC_MONO)
    rows = {}
    for head in (0, 2):
        monkeypatch.setenv('SPKD_AHC_HEAD', str(head))
        ctx = hipabi.Context(0, torch.cuda.current_stream().cuda_stream)
        try:
            tm = {}
            rows[head] = pipeline.diarize_batch(ctx, frames.data_ptr(), off, files, cl=cl, timings=tm, fused=True)
            assert tm['ahc_head'] == head
        finally:
            ctx.close()
    assert len(rows[0]) == 6 and all(len(r) > 3 for r in rows[0])
    for a, b in zip(rows[0], rows[2]):
        assert a.tobytes() == b.tobytes()


def _rule(sizes):
    lib = pkg('hipabi').load_library()
    off = _seg_off(sizes)
    return int(lib.spkd_ahc_head_rule(off.ctypes.data_as(C.c_void_p), len(sizes)))


def test_the_rule_on_the_host():
    """Sizes like the benchmark batch's (256 problems, mean 394.7, standard deviation 12.6, its twelve largest as
    measured, one of them far out): a head of 1 .. 32 problems.  Equal sizes, and fewer than 16 problems: none."""
    top = [465, 433, 431, 426, 425, 419, 419, 419, 418, 417, 415, 414]
    body = np.clip(np.round(394.7 + 12.6 * np.linspace(-2.2, 1.5, 256 - len(top))), 366, 413).astype(int).tolist()
    k = _rule(body[:100] + top + body[100:])
    assert 1 <= k <= 32
    assert _rule([395] * 256) == 0
    assert _rule(top + [300, 300, 300]) == 0
    assert _rule([]) == 0
