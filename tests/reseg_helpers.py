"""What the resegmentation tests (tests/test_reseg_*.py) share: the synthetic inputs, a context stub that
records what resegment_batch asks of it, and a batch resident on the device."""
import ctypes as C

import numpy as np

from conftest import pkg

RATE = 125.0


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def close_session(seed, seconds, n_speakers, eps=0.2):
    """A session of the generator whose speakers differ by eps (a fifth) of their usual distance in the mean
    only: single frames are then often closer to the wrong speaker."""
    synth = pkg('synth')
    base = [synth._speaker_model(seed, k) for k in range(n_speakers)]
    models = [(base[0][0] + eps * (m[0] - base[0][0]), base[0][1]) for m in base]
    return synth.make_session(seed, seconds, n_speakers, models=models)


def displaced(truth, vad, shift=100):
    """The truth's segments with every boundary inside a VAD turn moved by `shift` frames."""
    segs = []
    for a, b in vad:
        inside = [t for t in truth if a <= t[0] and t[1] <= b]
        for k, (s, e, spk) in enumerate(inside):
            segs.append((s if k == 0 else s + shift, e if k == len(inside) - 1 else e + shift, spk))
    return segs


def normal_scores(rng, T, W):
    """Float32 normals around -100 rounded to halves (exact ties), as test_reseg_batch's decoder test,
    with a NaN, a -inf column and frames nobody can score planted."""
    sc = (np.round(rng.normal(-100.0, 3.0, (T, W)) * 2.0) / 2.0).astype(np.float32)
    if T >= 9:
        sc[5:9] = sc[4]
    if W > 2 and rng.integers(0, 2) == 0:
        sc[:, 1] = -np.inf
    if T >= 8 and rng.integers(0, 2) == 0:
        t = int(rng.integers(0, T - 4))
        sc[t:t + int(rng.integers(1, 5))] = -np.inf
    if T >= 2 and rng.integers(0, 2) == 0:
        sc[int(rng.integers(0, T)), int(rng.integers(0, W))] = np.nan
    if W > 1 and T >= 3 and rng.integers(0, 4) == 0:
        sc[int(rng.integers(0, T)), 0] = -np.inf
    return sc


class StubContext(object):
    """Records in `calls` what resegment_batch asks of a context and answers one canned decoding per pass.
    answers: per pass the tokens [(frame, word)] of every turn, the last one for every pass beyond; ok: per
    pass the speakers' ok flags likewise (None: every speaker is ok).  The posterior calls are the test
    files' own, as are the tuples a file asserts on."""
    SCRATCH = {'reseg_speaker_stats': 4096, 'reseg_models': 8192, 'reseg_gmm': 8192, 'reseg_scores': 12288,
               'reseg_post': 16384}
    MS = {}              # last_ms by timer; 0.5 for every other

    def __init__(self, answers, ok=None):
        self.answers, self.ok, self.calls, self.n, self.scratch = answers, ok, [], 0, []

    def _ok(self, n):
        return np.ones(n, dtype=np.int32) if self.ok is None else np.array(self.ok[min(self.n, len(self.ok) - 1)], dtype=np.int32)

    def _answer(self):
        tokens = self.answers[min(self.n, len(self.answers) - 1)]
        self.n += 1
        off = np.concatenate([[0], np.cumsum([len(t) for t in tokens])]).astype(np.int64)
        flat = [x for t in tokens for x in t]
        return (off, np.array([f for f, _ in flat], dtype=np.int64), np.array([w for _, w in flat], dtype=np.int32),
                np.zeros(len(tokens)))

    @staticmethod
    def _frame_off(b, e):
        return np.concatenate([[0], np.cumsum(np.array(e) - np.array(b))]).astype(np.int64)

    def dev_scratch(self, name, nbytes):
        self.scratch.append((name, nbytes))
        return self.SCRATCH[name]

    def sum_stats(self, *a):
        self.calls.append(('sum_stats',))

    def set_stats(self, d_frames, n_frames, begins, ends, sets, n_sets, d_stats):
        self.calls.append(('set_stats', d_frames, n_frames, np.array(begins).tolist(), np.array(ends).tolist(),
                           np.array(sets).tolist(), n_sets, d_stats))

    def gauss_models(self, d_stats, n, d_models):
        self.calls.append(('gauss_models', d_stats, n, d_models))
        return self._ok(n)

    def gmm_train(self, d_frames, n_frames, set_off, b, e, n_comp, n_iter, var_floor, d_gmm, from_model=False):
        self.calls.append(('gmm_train', np.array(set_off).tolist(), np.array(b).tolist(), np.array(e).tolist(), n_comp,
                           n_iter, var_floor, d_gmm, from_model))
        ok = self._ok(len(set_off) - 1)
        return ok, np.zeros((len(ok), n_iter))

    def gauss_loglik(self, d_frames, n_frames, d_models, ok, b, e, m, k, n_cols, d_scores):
        self.calls.append(('loglik', np.array(ok).tolist()))
        return self._frame_off(b, e)

    def gmm_loglik_seq(self, d_frames, n_frames, d_gmm, n_comp, ok, b, e, m, k, n_cols, d_scores):
        self.calls.append(('loglik', np.array(ok).tolist()))
        return self._frame_off(b, e)

    def vad_viterbi_batch(self, d_scores, frame_off, n_states, word_state, stay, exit_, enter):
        self.calls.append(('decode',))
        return self._answer()

    def mindur_viterbi_batch(self, d_scores, frame_off, n_cols, penalty, min_frames):
        self.calls.append(('decode_md',))
        return self._answer()

    def last_ms(self, which='call'):
        return self.MS.get(which, 0.5)


class Dev(object):
    """A frame array resident on the device and the records of frame sets of it."""

    def __init__(self, frames):
        self.engine, self.pipeline, self.hipabi = pkg('engine'), pkg('pipeline'), pkg('hipabi')
        self.frames = np.ascontiguousarray(frames, dtype=np.float32)
        self.eng = self.engine.HipEngine(0)
        self.eng.set_features(self.frames)
        self.ctx, self.bufs = self.eng.ctx, []

    def records(self, ranges):
        d = self.eng._stats_of_sets([[r] for r in ranges])
        self.bufs.append(d)
        return d

    def alloc(self, nbytes):
        self.bufs.append(self.ctx.dev_alloc(nbytes))
        return self.bufs[-1]

    def close(self):
        for p in self.bufs:
            self.ctx.dev_free(p)
        self.eng.close()


class Batch(Dev):
    """Files as one batch resident on the device.  sess: per file (feats, vad, segments), vad the turns and
    segments the clustering stage's [(begin, end, speaker)], both in frames of the file; label = speaker + 1.
    Holds what resegment_batch takes: files, seg_off, labels, segments (seconds) and the segments' records
    d_stats; foff are the files' frame offsets."""

    def __init__(self, sess):
        Dev.__init__(self, np.concatenate([s[0] for s in sess]))
        self.sess = sess
        foff = self.foff = np.concatenate([[0], np.cumsum([len(s[0]) for s in sess])])
        self.files = [self.pipeline.BatchFile(foff[i], len(s[0]), [(a / RATE, b / RATE) for a, b in s[1]])
                      for i, s in enumerate(sess)]
        self.seg_off = np.concatenate([[0], np.cumsum([len(s[2]) for s in sess])]).astype(np.int64)
        self.labels = [np.array([k + 1 for _, _, k in s[2]], dtype=np.int32) for s in sess]
        self.segments = [np.array([(a / RATE, b / RATE) for a, b, _ in s[2]]) for s in sess]
        self.d_stats = self.records([(int(foff[i] + a), int(foff[i] + b)) for i, s in enumerate(sess) for a, b, _ in s[2]])

    def run(self, reseg, detail=None, timings=None):
        return self.pipeline.resegment_batch(self.ctx, self.eng.d_frames, len(self.frames), self.files, self.d_stats,
                                             self.seg_off, self.labels, RATE, reseg, False, timings, detail, self.segments)
