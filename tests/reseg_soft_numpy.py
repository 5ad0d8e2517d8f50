"""CPU restatement of posterior-weighted statistics (spkd_post_stats) and of soft resegmentation
(pipeline.resegment_batch, reseg['soft']) -- TEST INFRASTRUCTURE ONLY.

PARITY: no reference counterpart.  The reference stops at clustering; what the two compute is stated
in include/spkd.h (8) and here:

  post_stats      the definition of the header, literally: record m = the sum, over the frames t of the
                  sequences whose model range holds m, of w x~ x~^T with w the float32 posterior of m at
                  t and x~ = (x, 1); a weight of exactly 0 adds nothing whatever the frame holds.  In
                  the dtype asked for (np.float64, or np.longdouble as the yardstick of the device).
  post_abs        the same sum over |w x~_i x~_j|: what the a-priori bound of a sum in any order scales
                  with; and the number of terms of every record.
  resegment_soft  reseg_mindur_numpy.resegment's loop with the retraining replaced: pass p > 1 trains every
                  speaker on all frames of the turns, weighted by reseg_fb_numpy.posterior on the scores
                  of pass p - 1 at reseg['soft_scale'], gamma rounded to float32 before use as d_post is.
"""
import numpy as np

import reseg_fb_numpy as F
import reseg_mindur_numpy as M
import reseg_numpy as R

DIM, REC = R.DIM, R.REC
_IU = np.triu_indices(DIM + 1)
SOFT_SCALE = 0.1


def _rows(seqs):
    off = [0]
    for b, e, _, _ in seqs:
        off.append(off[-1] + (e - b))
    return off


def post_stats(feats, post, seqs, n_models, dtype=np.float64, absolute=False):
    """feats [n_frames, 39] float32; post [sum len, n_cols] float32 in the compact layout; seqs
    [(begin, end, first model, model count)] -> records [n_models, 820] dtype (absolute: of |w x~_i x~_j|)."""
    feats = np.asarray(feats, dtype=np.float32)
    post = np.asarray(post, dtype=np.float32)
    out = np.zeros((n_models, REC), dtype=dtype)
    off = _rows(seqs)
    with np.errstate(all='ignore'):
        for q, (b, e, m, k) in enumerate(seqs):
            if e == b or k == 0:
                continue
            x = np.concatenate([feats[b:e].astype(dtype), np.ones((e - b, 1), dtype=dtype)], axis=1)
            w = post[off[q]:off[q + 1]].astype(dtype)
            if absolute:
                x, w = np.abs(x), np.abs(w)
            for j in range(k):
                use = w[:, j] != 0                                  # (weight 0: the frame takes no part)
                xa = x[use]
                out[m + j] += ((xa * w[use, j][:, None]).T @ xa)[_IU]
    return out


def post_terms(post, seqs, n_models):
    """The number of terms w != 0 of every record."""
    post = np.asarray(post, dtype=np.float32)
    n = np.zeros(n_models, dtype=np.int64)
    off = _rows(seqs)
    for q, (b, e, m, k) in enumerate(seqs):
        for j in range(k):
            n[m + j] += int(np.count_nonzero(post[off[q]:off[q + 1], j]))
    return n


def resegment_soft(feats, turns, segs, reseg, rate=125.0):
    """Soft resegmentation of one file with Gaussian speakers: turns [(begin, end)] in frames, segs [(begin,
    end, speaker)] the input segmentation, reseg a dictionary like pipeline.RESEG_SOFT.  Returns what
    reseg_mindur_numpy.resegment returns and the masses: (speakers, per pass the decoded turns, ok per
    speaker of the last pass run, passes run, per retraining the speakers' expected frame counts)."""
    assert reseg.get('model', 'gauss') == 'gauss'
    spk = sorted(set(s[2] for s in segs))
    n = len(spk)
    scale, penalty = float(reseg.get('soft_scale', SOFT_SCALE)), float(reseg['penalty'])
    seqs = [(a, b, 0, n) for a, b in turns]
    out, oks, masses, scores = [], [], [], None
    for p in range(int(reseg.get('passes', 1))):
        if p == 0:
            recs = []
            for sp in spk:
                rec = np.zeros(REC)
                for b, e, k in segs:
                    if k == sp:
                        rec = rec + R.record_of_frames(feats[b:e])
                recs.append(rec)
        else:
            post = np.concatenate([F.posterior(sc, penalty, scale, n, np.float64)[0].astype(np.float32) for sc in scores])
            recs = list(post_stats(feats, post, seqs, n))
            masses.append(np.array([r[REC - 1] for r in recs]))
        trained = [R.model_from_record(r) for r in recs]
        models, oks = [(mu, w, c) for mu, w, c, _ in trained], [ok for _, _, _, ok in trained]
        scores, decoded = [], []
        for a, b in turns:
            sc = R.scores(feats[a:b], models, oks, n).astype(np.float32)
            frames, words, _ = M.decode(sc, reseg, rate)
            scores.append(sc)
            decoded.append((frames, words))
        out.append(decoded)
        if p > 0 and out[-1] == out[-2]:
            break
    return spk, out, oks, len(out), masses


def frame_labels(turns, decoded, spk, n_frames):
    """Per frame the decoded speaker (-1 outside the turns)."""
    lab = np.full(n_frames, -1, dtype=np.int64)
    for (a, b), (frames, words) in zip(turns, decoded):
        for f, e, w in zip(frames, list(frames[1:]) + [b - a], words):
            lab[a + f:a + e] = spk[w]
    return lab


def truth_labels(truth, n_frames):
    lab = np.full(n_frames, -1, dtype=np.int64)
    for b, e, k in truth:
        lab[b:e] = k
    return lab
