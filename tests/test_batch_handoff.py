"""The batch hand-off on the device (spkd_gw_batch, spkd_ahc_fused; pipeline.diarize_batch_device)
against the host hand-off it replaces: the same lines, the same records, the same rows."""
import os
import re

import numpy as np
import pytest

from helpers import ROOT
from conftest import pkg

N_FILES = 64
NO_TURN_FILE = 63          # its VAD list is emptied
SHORT_TURN_FILE = 62       # its first turn is cut to 1.5 s: 187 frames, no window of 2 x 125 fits


@pytest.fixture(scope='module')
def batch():
    """64 distinct 1 h / 4-speaker sessions generated on the GPU, one of them without a turn
    and one with a turn too short for a window."""
    torch = pytest.importorskip('torch')
    sd = pkg('synth_device')
    pipeline = pkg('pipeline')
    recipe = pkg('recipe')
    hipabi = pkg('hipabi')
    parts, files, off = [], [], 0
    for i in range(N_FILES):
        feats, vad, _ = sd.make_session_device(910000 + i, 3600, 4, device='cuda')
        v = [(float(recipe.py2_float_str(a / 125.0)), float(recipe.py2_float_str(b / 125.0))) for a, b in vad]
        if i == NO_TURN_FILE:
            v = []
        if i == SHORT_TURN_FILE:
            v[0] = (v[0][0], v[0][0] + 1.5)
        files.append(pipeline.BatchFile(off, feats.shape[0], v))
        parts.append(feats)
        off += feats.shape[0]
    frames = torch.cat(parts)
    del parts
    torch.cuda.synchronize()
    ctx = hipabi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield dict(ctx=ctx, frames=frames, ptr=frames.data_ptr(), total=int(frames.shape[0]), files=files)
    ctx.close()


def _turn_table(files, rate=125.0):
    nturn = [len(f.vad) for f in files]
    vad = np.concatenate([f.vad_arr for f in files])
    owner = np.repeat(np.arange(len(files)), nturn)
    foff = np.array([f.frame_off for f in files], dtype=np.int64)[owner]
    fn = np.array([f.n_frames for f in files], dtype=np.int64)[owner]
    ls, le = np.ascontiguousarray(vad[:, 0]), np.ascontiguousarray(vad[:, 1])
    f0 = np.minimum((ls * rate).astype(np.int64), fn)
    f1 = np.maximum(f0, np.minimum((le * rate).astype(np.int64), fn))
    return owner, foff, fn, ls, le, foff + f0, foff + f1


def _cd_params(hipabi):
    return hipabi.CdParams(hipabi.KINDS['BIC'], 0, 1.0, 0.0, 125.0, 375.0, 12.0, 125.0)


def _host_lines(b, scale=1.0):
    """The lines of the host hand-off: the event arrays of the fused call, walked by
    count_flags and gw_lines; plus the redo set as pipeline.segment_stats finds it."""
    hipabi = pkg('hipabi')
    ctx = b['ctx']
    owner, foff, fn, ls, le, tb, te = _turn_table(b['files'])
    alloc = lambda n: ctx.dev_scratch('test_host_seg', max(n, 1) * hipabi.REC * 8)
    r = ctx.gw(b['ptr'], b['total'], tb, te, _cd_params(hipabi), tight=True, seg_stats=alloc, first_guess_scale=scale)
    assert r['status'] == hipabi.SPKD_OK
    nd = hipabi.count_flags(r['win_det'], r['off'][:-1], r['n_win'])
    lines = hipabi.gw_lines(r['off'][:-1], nd, r['det_start'], r['det_maxi'], r['final_start'], ls, le, tb, te, 125.0,
                            text_contract=True, want_frames=True)
    t = lines['turn']
    a0 = np.clip((lines['times'][:, 0] * 125.0).astype(np.int64), 0, fn[t])
    a1 = np.maximum(a0, np.clip((lines['times'][:, 1] * 125.0).astype(np.int64), 0, fn[t]))
    rb, re_ = foff[t] + a0, foff[t] + a1
    redo = np.nonzero((rb != lines['frame_b']) | (re_ != lines['frame_e']))[0]
    return r, nd, lines, redo, rb, re_, (tb, te, owner)


@pytest.mark.gpu
def test_compact_lines_equal_the_host_walk_bit_for_bit(batch):
    hipabi = pkg('hipabi')
    ctx = batch['ctx']
    owner, foff, fn, ls, le, tb, te = _turn_table(batch['files'])
    r, nd, lines, redo, rb, re_, _ = _host_lines(batch)
    # the inputs contain what they were chosen for
    n_no_det = int((nd == 0).sum())
    n_short = int(((te - tb) < 250).sum())
    n_no_turn = sum(1 for f in batch['files'] if len(f.vad) == 0)
    print('turns %d, without detection %d, too short for a window %d, files without a turn %d, lines %d'
          % (len(tb), n_no_det, n_short, n_no_turn, len(lines['turn'])))
    assert n_no_det > 0 and n_short > 0 and n_no_turn > 0
    assert int(r['n_win'][(te - tb) < 250].max()) == 0
    alloc = lambda n: ctx.dev_scratch('test_dev_seg', max(n, 1) * hipabi.REC * 8)
    g = ctx.gw_batch(batch['ptr'], batch['total'], tb, te, _cd_params(hipabi), ls, le, foff, fn, alloc, tight=True,
                     want_index=True)
    assert g['status'] == hipabi.SPKD_OK and g['n_lines'] == len(lines['turn']) == int(nd.sum()) + len(tb)
    assert np.array_equal(g['off'], r['off'])
    assert np.array_equal(g['n_win'], r['n_win'])
    assert np.array_equal(g['times'].view(np.uint64), lines['times'].view(np.uint64))
    for k in ('turn', 'index', 'frame_b', 'frame_e'):
        assert np.array_equal(g[k], lines[k]), k
    # the redo list: the lines pipeline.segment_stats would compute from the frames again
    print('redo lines %d of %d' % (len(redo), g['n_lines']))
    assert len(redo) > 0
    assert np.array_equal(g['redo_line'], redo)
    assert np.array_equal(g['redo_begin'], rb[redo]) and np.array_equal(g['redo_end'], re_[redo])


def _host_rows_and_merges(b, cl):
    pipeline = pkg('pipeline')
    ctx, files = b['ctx'], b['files']
    box, tm = [], {}
    segs = pipeline.change_detect_batch(ctx, b['ptr'], b['total'], files, fused=box)
    keep = [i for i, sg in enumerate(segs) if len(sg) > 0]
    res = pipeline.cluster_batch(ctx, b['ptr'], b['total'], [files[i] for i in keep], [segs[i] for i in keep], cl=cl,
                                 timings=tm, want_merges=True, fused=box[0])
    rows = pipeline.diarize_batch(ctx, b['ptr'], b['total'], files, cl=cl, fused=True, handoff='host')
    return rows, [m for (_, m) in res], tm


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['BIC', 'GLR'])
def test_device_handoff_gives_the_rows_and_merges_of_the_host_handoff(batch, kind):
    pipeline = pkg('pipeline')
    cl = dict(pipeline.DIA2_CL, kind=kind)
    if kind == 'GLR':
        cl['threshold'] = 1500.0                 # (-t 1500: the GLR clustering threshold of test_full_size)
    want, want_merges, tm_host = _host_rows_and_merges(batch, cl)
    detail, tm = {}, {}
    got = pipeline.diarize_batch_device(batch['ctx'], batch['ptr'], batch['total'], batch['files'], cl=cl, timings=tm,
                                        detail=detail)
    default = pipeline.diarize_batch(batch['ctx'], batch['ptr'], batch['total'], batch['files'], cl=cl, fused=True)
    assert len(got) == len(want) == N_FILES
    for i in range(N_FILES):
        assert got[i].shape == want[i].shape, i
        assert np.array_equal(got[i], want[i]), i
        assert np.array_equal(default[i], want[i]), i
    assert got[NO_TURN_FILE].shape == (0, 3)
    n_merges = sum(len(m) for m in want_merges)
    print('%s: %d rows, %d merges, %d segments recomputed' % (kind, sum(len(g) for g in got), n_merges,
                                                               tm['stats_recomputed']))
    assert n_merges > 0
    # same kernels on the same records: the merge log is bit-identical, distances included
    assert len(detail['merges']) == len(want_merges)
    for m_new, m_old in zip(detail['merges'], want_merges):
        assert [(a, b) for a, b, _ in m_new] == [(a, b) for a, b, _ in m_old]
        assert np.array_equal(np.array([d for _, _, d in m_new]).view(np.uint64),
                              np.array([d for _, _, d in m_old]).view(np.uint64))
    assert tm['stats_recomputed'] == tm_host['stats_recomputed'] > 0
    assert tm['stats_sets'] == tm_host['stats_sets'] and tm['stats_frames'] == tm_host['stats_frames']
    for k in ('matrix_pairs', 'ahc_pairs'):
        assert tm[k] == tm_host[k], k


@pytest.mark.gpu
def test_capacity_retry_ends_in_the_same_rows(batch):
    """The first guess scaled down 64 times (2 event slots for most turns): SPKD_EOVERFLOW from the
    kernel, no compaction on the dirty error word, doubled capacities until it fits."""
    pipeline = pkg('pipeline')
    hipabi = pkg('hipabi')
    want = pipeline.diarize_batch_device(batch['ctx'], batch['ptr'], batch['total'], batch['files'])
    detail = {}
    got = pipeline.diarize_batch_device(batch['ctx'], batch['ptr'], batch['total'], batch['files'], detail=detail,
                                        first_guess_scale=1.0 / 64)
    # the scaled guess was too small for the tight first try
    owner, foff, fn, ls, le, tb, te = _turn_table(batch['files'])
    first_try = (np.maximum((((te - tb).astype(np.float64) / 25.0).astype(np.int64) + 8) // 64, 2) // 4 + 8)
    assert int((detail['lines']['n_win'] > first_try).sum()) > 0
    assert int(detail['lines']['off'][-1]) > int(first_try.sum())
    for i in range(N_FILES):
        assert np.array_equal(got[i], want[i]), i


@pytest.mark.gpu
def test_a_moved_boundary_gets_the_record_of_set_stats(batch):
    """A line whose boundary the 12-digit round trip moved across a frame edge: the host hand-off
    computes its record with spkd_set_stats and gathers it into segment order; the device
    hand-off names the same line with the same frame range (its record comes from the same
    kernels inside spkd_ahc_fused), and the record differs from the fused one it replaces."""
    hipabi = pkg('hipabi')
    pipeline = pkg('pipeline')
    ctx = batch['ctx']
    tm, detail = {}, {}
    pipeline.diarize_batch_device(ctx, batch['ptr'], batch['total'], batch['files'], timings=tm, detail=detail)
    L = detail['lines']
    assert tm['stats_recomputed'] == len(L['redo_line']) > 0
    k = len(L['redo_line']) // 2
    line, rb, re_ = int(L['redo_line'][k]), int(L['redo_begin'][k]), int(L['redo_end'][k])
    assert (rb, re_) != (int(L['frame_b'][line]), int(L['frame_e'][line]))
    assert abs(rb - int(L['frame_b'][line])) <= 1 and abs(re_ - int(L['frame_e'][line])) <= 1
    # spkd_set_stats on that range
    d_one = ctx.dev_scratch('test_one_record', hipabi.REC * 8)
    ctx.set_stats(batch['ptr'], batch['total'], [rb], [re_], [0], 1, d_one)
    one = np.empty(hipabi.REC, dtype=np.float64)
    ctx.d2h(one, d_one)
    assert one[hipabi.REC - 1] == re_ - rb                      # (the record's frame count)
    # the host hand-off's record of that line, from its gathered buffer
    pipeline.diarize_batch(ctx, batch['ptr'], batch['total'], batch['files'], fused=True, handoff='host')
    n = len(L['turn'])
    d_stats = ctx.dev_scratch('segment_stats', n * hipabi.REC * 8)
    host_rec = np.empty(hipabi.REC, dtype=np.float64)
    ctx.d2h(host_rec, d_stats + line * hipabi.REC * 8)
    assert np.array_equal(host_rec.view(np.uint64), one.view(np.uint64))
    # and the fused record it replaces covers another range
    fused_rec = np.empty(hipabi.REC, dtype=np.float64)
    ctx.d2h(fused_rec, L['d_seg'] + int(L['index'][line]) * hipabi.REC * 8)
    assert fused_rec[hipabi.REC - 1] == int(L['frame_e'][line]) - int(L['frame_b'][line])
    assert not np.array_equal(fused_rec, one)


def test_new_entry_points_are_declared_and_exported():
    hipabi = pkg('hipabi')
    text = open(os.path.join(ROOT, 'include', 'spkd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    vmap = open(os.path.join(ROOT, 'speaker-diarization_amd', 'csrc', 'libspkd_hip.map')).read()
    lib = hipabi.load_library()
    for name in ('spkd_gw_batch', 'spkd_ahc_fused'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in hipabi.EXPORTS and hasattr(lib, name)
    assert re.search(r'global:\s*spkd_\*;', vmap)               # the map exports the header's prefix
    assert 'spkd_gw_lines_view' in code


def test_spkd_gw_still_refuses_null_outputs():
    """The contract of the existing entry point does not change: only the batch form does
    without the event arrays.  (Argument checks come before any device work, so a NULL
    context pointer would do; a context needs a GPU, so the refusal is looked at in the source
    order: SPKD_EINVAL for a NULL context, and for NULL outputs with a real one on the GPU.)"""
    import ctypes as C
    hipabi = pkg('hipabi')
    lib = hipabi.load_library()
    p = hipabi.CdParams(0, 0, 1.0, 0.0, 125.0, 375.0, 12.0, 125.0)
    cnt = C.c_int64(0)
    st = lib.spkd_gw(None, None, 0, None, None, 1, C.byref(p), None, None, None, None, None, None, None, None,
                     None, 0, C.byref(cnt))
    assert st == hipabi.SPKD_EINVAL


@pytest.mark.gpu
def test_spkd_gw_refuses_null_outputs_on_a_context(batch):
    import ctypes as C
    hipabi = pkg('hipabi')
    ctx = batch['ctx']
    p = _cd_params(hipabi)
    b = np.array([0], dtype=np.int64)
    e = np.array([1000], dtype=np.int64)
    off = np.array([0, 64], dtype=np.int64)
    cnt = C.c_int64(0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    st = ctx.lib.spkd_gw(ctx.h, C.c_void_p(batch['ptr']), batch['total'], ptr(b), ptr(e), 1, C.byref(p), ptr(off),
                         None, None, None, None, None, None, None, None, 0, C.byref(cnt))
    assert st == hipabi.SPKD_EINVAL
    assert b'null argument' in ctx.lib.spkd_last_error(ctx.h)
