"""Iterated resegmentation: reseg['passes'] in pipeline.resegment_batch -- the speakers trained again
on the decoded rows, the turns decoded again.  The restatement of the loop is
reseg_mindur_numpy.resegment.  PARITY: no reference counterpart."""
import numpy as np
import pytest

import reseg_mindur_numpy as M
import reseg_numpy as R
from conftest import pkg
from reseg_helpers import Dev as _Dev, StubContext as _StubContext, displaced as _displaced

RATE = 125.0


def _rows_of(vad, spk, decoded, text_contract=False):
    out = [R.rows_of_turn(frames, words, a / RATE, b / RATE, [k + 1 for k in spk], RATE, text_contract)
           for (a, b), (frames, words) in zip(vad, decoded)]
    return np.concatenate(out)


# ------------------------------------------------------------------ not GPU
def test_passes_must_be_an_integer_from_one_on():
    pipeline = pkg('pipeline')
    files = [pipeline.BatchFile(0, 1000, [(0.0, 8.0)])]
    labels = [np.array([1, 2])]
    for bad in (0, -1, 1.5, float('nan'), float('inf'), '2', None, True):
        with pytest.raises(ValueError, match='reseg passes'):
            pipeline.resegment_batch(None, 0, 1000, files, 0, [0, 2], labels, reseg=dict(penalty=50.0, passes=bad))
        with pytest.raises(ValueError, match='reseg passes'):
            pipeline.diarize_batch(None, 0, 0, [], reseg=dict(penalty=50.0, passes=bad))
    stage = pkg('resegmentation')
    assert stage._reseg_passes(dict(penalty=1.0)) == 1 and stage._reseg_passes(dict(passes=3.0)) == 3
    # model gmm with passes still wants the segments, for pass 1
    with pytest.raises(ValueError, match='it takes segments'):
        pipeline.resegment_batch(None, 0, 1000, files, 0, [0, 2], labels, reseg=dict(pipeline.RESEG_GMM, passes=2))


def test_token_ranges_are_absolute_and_end_with_the_turn():
    tok_off = np.array([0, 2, 2, 5])
    b, e, spk = pkg('resegmentation')._token_ranges(tok_off, np.array([0, 100, 0, 7, 300]), np.array([1, 0, 2, 0, 2]),
                                                    np.array([125, 1000, 1562]), np.array([375, 1000, 2250]),
                                                    np.array([0, 0, 2]))
    assert b.tolist() == [125, 225, 1562, 1569, 1862] and e.tolist() == [225, 375, 1569, 1862, 2250]
    assert spk.tolist() == [1, 0, 4, 2, 4]


def test_the_loop_on_the_host():
    """One file of three speakers (labels 1, 2, 3), two turns.  Pass 2 trains on pass 1's tokens grouped
    by speaker in turn order; speaker 3 gets no token and is dropped; pass 3 decodes what pass 2 did,
    so the loop stops there."""
    pipeline = pkg('pipeline')
    files = [pipeline.BatchFile(1000, 1000, [(1.0, 3.0), (4.0, 6.0)])]
    labels = [np.array([3, 1, 2, 1])]
    segments = [np.array([(1.0, 2.0), (2.0, 3.0), (4.0, 5.0), (5.0, 6.0)])]
    first = [[(0, 1), (100, 0)], [(0, 0), (50, 1)]]
    second = [[(0, 1), (90, 0)], [(0, 0), (50, 1)]]
    stub = _StubContext([first, second, second, first], [[1, 1, 1], [1, 1, 0]])
    timings, det = {}, {}
    rows = pipeline.resegment_batch(stub, 1 << 20, 2000, files, 1 << 21, [0, 4], labels, RATE, dict(penalty=7.0, passes=5),
                                    False, timings, det)
    names = [c[0] for c in stub.calls]
    assert names == ['sum_stats', 'gauss_models', 'loglik', 'decode'] + ['set_stats', 'gauss_models', 'loglik', 'decode'] * 2
    # pass 2: the four tokens as absolute ranges, stably sorted by speaker (0: label 1, 1: label 2)
    assert stub.calls[4][1:] == (1 << 20, 2000, [1225, 1500, 1125, 1550], [1375, 1550, 1225, 1750], [0, 0, 1, 1], 3, 4096)
    assert stub.calls[8][3] == [1215, 1500, 1125, 1550]                    # pass 3: pass 2's tokens
    assert stub.calls[5][1:] == (4096, 3, 8192)
    assert stub.calls[6][1] == [1, 1, 0] and stub.calls[2][1] == [1, 1, 1]
    assert det['passes_run'] == 3 and det['dropped'] == [(0, 3)]
    assert all(timings[k] == [0.5] * 3 for k in ('reseg_models', 'reseg_loglik', 'reseg_viterbi', 'reseg_backtrack'))
    assert rows[0].tolist() == [[1.0, 1.0 + 90 / 125.0, 2.0], [1.0 + 90 / 125.0, 3.0, 1.0],
                                [4.0, 4.0 + 50 / 125.0, 1.0], [4.0 + 50 / 125.0, 6.0, 2.0]]
    # passes=2 ends after two decodes whatever they were; passes=1 is the key's absence
    stub = _StubContext([first, second, first], [[1, 1, 1]])
    det = {}
    pipeline.resegment_batch(stub, 1 << 20, 2000, files, 1 << 21, [0, 4], labels, RATE, dict(penalty=7.0, passes=2), False,
                             None, det)
    assert det['passes_run'] == 2 and [c[0] for c in stub.calls].count('decode') == 2
    one, none = _StubContext([first], [[1, 1, 1]]), _StubContext([first], [[1, 1, 1]])
    a = pipeline.resegment_batch(one, 1 << 20, 2000, files, 1 << 21, [0, 4], labels, RATE, dict(penalty=7.0, passes=1), False)
    b = pipeline.resegment_batch(none, 1 << 20, 2000, files, 1 << 21, [0, 4], labels, RATE, dict(penalty=7.0), False)
    assert a[0].tobytes() == b[0].tobytes() and one.calls == none.calls and 'set_stats' not in [c[0] for c in one.calls]
    # model gmm: pass 2 is a fresh training on the tokens; the speaker without a token owns one empty range
    stub = _StubContext([first, first], [[1, 1, 1], [1, 1, 0]])
    det = {}
    reseg = dict(penalty=7.0, model='gmm', components=3, iterations=2, var_floor=0.05, passes=4)
    pipeline.resegment_batch(stub, 1 << 20, 2000, files, 1 << 21, [0, 4], labels, RATE, reseg, False, None, det, segments)
    assert [c[0] for c in stub.calls] == ['gmm_train', 'loglik', 'decode'] * 2
    assert stub.calls[0][1:4] == ([0, 2, 3, 4], [1250, 1625, 1500, 1125], [1375, 1750, 1625, 1250])
    assert stub.calls[3][1:] == ([0, 2, 4, 5], [1225, 1500, 1125, 1550, 0], [1375, 1550, 1225, 1750, 0], 3, 2, 0.05, 8192, False)
    assert det['passes_run'] == 2 and det['dropped'] == [(0, 3)]


def test_restated_loop_converges_on_the_displaced_input():
    """Both models, with and without a minimum duration: pass 1 puts the boundaries back, pass 2
    trains on them and decodes the same, so five passes stop after two."""
    synth, pipeline = pkg('synth'), pkg('pipeline')
    feats, vad, truth = synth.make_session(1234, 60.0, 3)
    segs = _displaced(truth, vad)
    for reseg in (pipeline.RESEG, pipeline.RESEG_GMM, pipeline.RESEG_MD):
        spk, out, oks, n = M.resegment(feats, vad, segs, dict(reseg, passes=5))
        assert n == 2 and all(oks) and out[0] == out[1]
        assert [a + f for (a, b), (fr, _) in zip(vad, out[-1]) for f in fr] == [t[0] for t in truth]


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def displaced():
    synth = pkg('synth')
    feats, vad, truth = synth.make_session(1234, 60.0, 3)
    d = _Dev(feats)
    d.vad, d.truth, d.segs = vad, truth, _displaced(truth, vad)
    d.files = [d.pipeline.BatchFile(0, len(feats), [(a / RATE, b / RATE) for a, b in vad])]
    yield d
    d.close()


def _run(d, segs, reseg, detail=None, timings=None):
    d_stats = d.records([(a, b) for a, b, _ in segs])
    labels = [np.array([k + 1 for _, _, k in segs])]
    segments = [np.array([(a / RATE, b / RATE) for a, b, _ in segs])]
    return d.pipeline.resegment_batch(d.ctx, d.eng.d_frames, len(d.frames), d.files, d_stats, [0, len(segs)], labels, RATE,
                                      reseg, False, timings, detail, segments)[0]


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['RESEG', 'RESEG_GMM', 'RESEG_MD'])
def test_passes_on_the_device_are_the_restatement(displaced, name):
    d = displaced
    base = getattr(d.pipeline, name)
    det, timings = {}, {}
    rows = _run(d, d.segs, dict(base, passes=2), det, timings)
    spk, out, oks, n = M.resegment(d.frames, d.vad, d.segs, dict(base, passes=2))
    assert n == 2 and det['passes_run'] == 2 and det['dropped'] == []
    assert rows.tobytes() == _rows_of(d.vad, spk, out[-1]).tobytes()
    assert all(len(timings[k]) == 2 for k in ('reseg_loglik', 'reseg_viterbi', 'reseg_backtrack'))
    assert len(timings['reseg_gmm_train' if name == 'RESEG_GMM' else 'reseg_models']) == 2
    # five passes stop early: the last two decodes are equal, so the rows are those of two passes
    det5 = {}
    rows5 = _run(d, d.segs, dict(base, passes=5), det5)
    assert det5['passes_run'] < 5 and det5['passes_run'] == M.resegment(d.frames, d.vad, d.segs, dict(base, passes=5))[3]
    assert rows5.tobytes() == rows.tobytes()
    # passes=1 is the key's absence, bit for bit
    det1 = {}
    assert _run(d, d.segs, dict(base, passes=1), det1).tobytes() == _run(d, d.segs, base).tobytes()
    assert det1['passes_run'] == 1


@pytest.mark.gpu
def test_a_speaker_that_loses_its_frames_is_dropped(displaced):
    """Label 4's only segment is 41 frames of speaker 1's data.  Its Gaussian is ok -- 41 frames, a
    covariance of full rank -- and so peaked on its own frames that the plain decoder gives them back
    to it even at penalty 50; with the minimum duration of RESEG_MD (125 frames > 41) pass 1 leaves it
    nothing, pass 2 cannot model it, and it is in detail['dropped'] and in no row."""
    d = displaced
    s0, e0, k0 = d.segs[0]
    planted = [(s0, s0 + 400, k0), (s0 + 400, s0 + 441, 3), (s0 + 441, e0, k0)] + d.segs[1:]
    assert s0 + 441 < e0
    reseg = dict(d.pipeline.RESEG_MD, passes=2)
    spk, out, oks, n = M.resegment(d.frames, d.vad, planted, reseg)
    assert n == 2 and oks == [True, True, True, False] and all(3 not in words for decoded in out for _, words in decoded)
    det = {}
    rows = _run(d, planted, reseg, det)
    assert det['passes_run'] == 2 and det['dropped'] == [(0, 4)]
    assert 4.0 not in rows[:, 2].tolist() and rows.tobytes() == _rows_of(d.vad, spk, out[-1]).tobytes()
    one = {}
    _run(d, planted, d.pipeline.RESEG_MD, one)
    assert one['dropped'] == [] and one['passes_run'] == 1                  # (ok in pass 1: dropped by the retraining)
