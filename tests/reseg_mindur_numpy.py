"""CPU restatement of the minimum-duration decoder (spkd_mindur_viterbi_batch) and of iterated
resegmentation (pipeline.resegment_batch, reseg['passes']) -- TEST INFRASTRUCTURE ONLY.

PARITY: no reference counterpart.  The reference stops at clustering; what the two compute is stated
in include/spkd.h (8) and here:

  viterbi      the recurrence of the header, literally, a Python float loop like reseg_numpy.viterbi:
               cleaned scores o, running sums P and counts C of -inf per word, the window
               w_t = P_t - P_{t-D} (-inf when the window holds a -inf), d_t = max(stay, fresh) with
               staying winning ties, g and b the maximum and lowest arg-max of d_t, read D frames on.
  brute_force  an independent check of the optimum: Viterbi over the expanded state space, every word
               a left-to-right chain of D states with tied emission, entered at state 1 (at `penalty`),
               left from state D only, the path ending in a state D; a sequence shorter than D frames
               is one stretch.  Best score only.
  resegment    the stage on one file with reseg['passes'] passes over reseg_numpy / reseg_gmm_numpy:
               pass 1 trains on the input segments, pass p > 1 on the tokens pass p - 1 decoded.
"""
import math

import numpy as np

import reseg_gmm_numpy as G
import reseg_numpy as R

INF = math.inf


def cleaned(sc):
    """o_t(k) as Python floats: NaN counts as -inf, a frame whose words are all -inf as 0 for each."""
    out = []
    for row in np.asarray(sc, dtype=np.float32):
        obs = [float(v) for v in row]
        obs = [-INF if o != o else o for o in obs]
        if all(o == -INF for o in obs):
            obs = [0.0] * len(obs)
        out.append(obs)
    return out


def _lowest_argmax(v):
    best, bi = v[0], 0
    for i in range(1, len(v)):
        if v[i] > best:
            best, bi = v[i], i
    return best, bi


def viterbi(sc, penalty, min_frames):
    """(token first frames, token words, path score) of sc [T, W] float32 scores."""
    sc = np.asarray(sc, dtype=np.float32)
    T, W = sc.shape
    D, p = int(min_frames), float(penalty)
    assert D >= 1
    if T == 0:
        return [], [], -INF
    o = cleaned(sc)
    P, C = [[0.0] * W], [[0] * W]                          # P[t + 1] = P_t, P[0] = P_-1
    for t in range(T):
        P.append([P[t][k] + o[t][k] if o[t][k] != -INF else P[t][k] for k in range(W)])
        C.append([C[t][k] + (1 if o[t][k] == -INF else 0) for k in range(W)])

    def window(t, k):
        return -INF if C[t + 1][k] - C[t + 1 - D][k] > 0 else P[t + 1][k] - P[t + 1 - D][k]

    if T < D:
        best, k = _lowest_argmax([-INF if C[T][k] > 0 else P[T][k] - P[0][k] for k in range(W)])
        return [0], [k], (-p) + best
    d = [[-INF] * W for _ in range(T)]
    entered = [[False] * W for _ in range(T)]
    gb = [(-INF, 0)] * T
    for t in range(D - 1, T):
        for k in range(W):
            if t == D - 1:
                d[t][k] = (-p) + window(t, k)
                continue
            g = gb[t - D][0]
            stay, fresh = d[t - 1][k] + o[t][k], (g - p) + window(t, k)
            if stay >= fresh:
                d[t][k] = stay
            else:
                d[t][k] = fresh
                entered[t][k] = True
        gb[t] = _lowest_argmax(d[t])
    score, j = _lowest_argmax(d[T - 1])
    frames, words = [], []
    t = T - 1
    while True:
        if t <= D - 1:
            frames.append(0)
            words.append(j)
            break
        if entered[t][j]:
            frames.append(t - D + 1)
            words.append(j)
            j = gb[t - D][1]
            t -= D
        else:
            t -= 1
    return frames[::-1], words[::-1], score


def brute_force(sc, penalty, min_frames):
    """The best score of any path whose stretches all last >= min_frames frames (a sequence shorter
    than that: of the single stretches), by Viterbi over (word, frames spent in it capped at D)."""
    sc = np.asarray(sc, dtype=np.float32)
    T, W = sc.shape
    D, p = int(min_frames), float(penalty)
    if T == 0:
        return -INF
    o = cleaned(sc)
    if T < D:
        return max(-p + sum(o[t][k] for t in range(T)) for k in range(W))
    v = [[-INF] * D for _ in range(W)]                     # v[k][s]: in word k, its state s + 1
    for k in range(W):
        v[k][0] = -p + o[0][k]
    for t in range(1, T):
        leave = max(v[k][D - 1] for k in range(W))
        new = [[-INF] * D for _ in range(W)]
        for k in range(W):
            for s in range(D):
                cand = []
                if s == 0:
                    cand.append(leave - p)
                if s > 0:
                    cand.append(v[k][s - 1])
                if s == D - 1:
                    cand.append(v[k][D - 1])
                new[k][s] = max(cand) + o[t][k]
        v = new
    return max(v[k][D - 1] for k in range(W))


def path_score(sc, penalty, frames, words):
    """The score of the path the tokens describe: -penalty per token, the cleaned scores of its frames."""
    o = cleaned(sc)
    ends = list(frames[1:]) + [len(o)]
    total = 0.0
    for f, e, w in zip(frames, ends, words):
        total += -float(penalty)
        for t in range(f, e):
            total += o[t][w]
    return total


def min_frames_of(reseg, rate):
    """D of a reseg dictionary: 0 when the key is absent or 0 (the plain decoder)."""
    s = float(reseg.get('min_dur_s', 0.0))
    return max(1, int(math.floor(s * rate))) if s > 0.0 else 0


def decode(sc, reseg, rate):
    D = min_frames_of(reseg, rate)
    return viterbi(sc, reseg['penalty'], D) if D else R.viterbi(sc, reseg['penalty'])


def _train(feats, ranges, reseg):
    """(model, ok) of one speaker from its frame ranges, in that order."""
    if reseg.get('model', 'gauss') == 'gmm':
        x = np.concatenate([feats[b:e] for b, e in ranges]) if ranges else feats[:0]
        if len(x) == 0:
            return None, False
        m, ok, _ = G.train(x, reseg['components'], reseg['iterations'], reseg['var_floor'])
        return m, ok
    rec = np.zeros(R.REC)
    for b, e in ranges:
        rec = rec + R.record_of_frames(feats[b:e])
    mu, w, c, ok = R.model_from_record(rec)
    return (mu, w, c), ok


def resegment(feats, turns, segs, reseg, rate=125.0):
    """Iterated resegmentation of one file: turns [(begin, end)] in frames, segs [(begin, end, speaker)]
    the input segmentation, reseg a dictionary like pipeline.RESEG_MD with 'passes'.  Returns (speakers,
    per pass the decoded turns [(token first frames, token speaker indices)], ok per speaker of the
    last pass run, passes run).  Pass p > 1 trains speaker s on the tokens of pass p - 1 that carry it,
    in turn order; a speaker whose model is not ok scores -inf; it stops early when a pass decodes what
    the pass before it decoded."""
    spk = sorted(set(s[2] for s in segs))
    scorer = G.scores if reseg.get('model', 'gauss') == 'gmm' else R.scores
    ranges = [[(b, e) for b, e, k in segs if k == sp] for sp in spk]
    out, oks = [], []
    for p in range(int(reseg.get('passes', 1))):
        if p > 0:
            ranges = [[] for _ in spk]
            for (a, b), (frames, words) in zip(turns, out[-1]):
                for f, e, w in zip(frames, list(frames[1:]) + [b - a], words):
                    ranges[w].append((a + f, a + e))
        trained = [_train(feats, r, reseg) for r in ranges]
        models, oks = [m for m, _ in trained], [ok for _, ok in trained]
        decoded = []
        for a, b in turns:
            sc = scorer(feats[a:b], models, oks, len(spk)).astype(np.float32)
            frames, words, _ = decode(sc, reseg, rate)
            decoded.append((frames, words))
        out.append(decoded)
        if p > 0 and out[-1] == out[-2]:
            break
    return spk, out, oks, len(out)
