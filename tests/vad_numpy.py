"""CPU restatement (numpy, float64) of the generate_exp.py stand-in -- TEST INFRASTRUCTURE ONLY.

PARITY UNPINNED: AaltoASR (phone_probs, the Decoder token pass) is not available, so what it
computes is restated here from the choices the stand-in makes, each listed so that a
maintainer with AaltoASR at hand can correct it:

  front-end   the model's .cfg (256-sample windows) through the same chain as fconfig.cfg,
              the window zero-padded to the 512-point transform (mfcc_numpy.py in the
              checker directory restates it for any window width).
  scores      CHOICE: the natural-log density of each state's diagonal Gaussian mixture,
              score[t][s] = logsumexp_k (ln w_sk + c_k - 1/2 sum_d (x_td - mu_kd)^2 / v_kd),
              c_k = -1/2 (D ln 2pi + sum_d ln v_kd); weights of 0 left out, a state without
              terms or with only -inf terms -inf, a NaN term NaN.
  decoder     CHOICE: an exact Viterbi over the loop of one-state words instead of the token
              pass (its beams and limits cannot act on two one-state words), with
              stay = ts ln a_jj, exit = ts ln a_j,exit, enter = lm ln(10) log10 P(j) - ins
              (ts 2, lm 10, ins 1 from generate_exp.py:221-224; the ln 10 conversion of the
              LM's log10 and the sign of the insertion penalty are choices), ties to staying,
              then to the lowest word; a NaN score -inf, a frame of only -inf scores 0.
  tokens      CHOICE: a token's frame is the first frame of its word.
The .lna layout, the shift and .last_frame are not restated: the reference's own code pins
them (tests/golden/generate_exp_cases.json).
"""
import math

import numpy as np


def gmm_loglik(x, means, variances, mixtures):
    """x [T, D] -> [T, S] float64 scores of the mixtures [(kernels, weights)] per state."""
    x = np.asarray(x, dtype=np.float64)
    means = np.asarray(means, dtype=np.float64)
    variances = np.asarray(variances, dtype=np.float64)
    D = means.shape[1]
    c = -0.5 * (D * math.log(2.0 * math.pi) + np.log(variances).sum(axis=1))
    out = np.empty((x.shape[0], len(mixtures)))
    with np.errstate(all='ignore'):
        for s, (ks, ws) in enumerate(mixtures):
            keep = [(int(k), float(w)) for k, w in zip(ks, ws) if w != 0.0]
            if not keep:
                out[:, s] = -np.inf
                continue
            terms = np.stack([math.log(w) + c[k] - 0.5 * (((x - means[k]) ** 2) / variances[k]).sum(axis=1)
                              for k, w in keep], axis=1)
            m = terms.max(axis=1)
            nan = np.isnan(terms).any(axis=1)
            safe = np.where(np.isfinite(m), m, 0.0)
            r = m + np.log(np.exp(terms - safe[:, None]).sum(axis=1))
            r = np.where(m == -np.inf, -np.inf, r)
            out[:, s] = np.where(nan, np.nan, r)
    return out


def decoder_constants(a_stay, a_exit, log10p, ts=2.0, lm=10.0, ins=1.0):
    with np.errstate(divide='ignore'):
        stay = ts * np.log(np.asarray(a_stay, dtype=np.float64))
        exit_ = ts * np.log(np.asarray(a_exit, dtype=np.float64))
    enter = lm * np.log(10.0) * np.asarray(log10p, dtype=np.float64) - ins
    return stay, exit_, enter


def viterbi(scores, word_state, stay, exit_, enter):
    """(token frames, token words, final score) of scores [T, S] (float32 values)."""
    scores = np.asarray(scores, dtype=np.float32)
    T, W = scores.shape[0], len(word_state)
    if T == 0:
        return [], [], -math.inf
    stay, exit_, enter = [[float(v) for v in a] for a in (stay, exit_, enter)]
    back = [[-1] * W for _ in range(T)]
    d = None
    for t in range(T):
        obs = [float(scores[t, word_state[j]]) for j in range(W)]
        obs = [-math.inf if o != o else o for o in obs]
        if all(o == -math.inf for o in obs):
            obs = [0.0] * W
        if t == 0:
            d = [enter[j] + obs[j] for j in range(W)]
            continue
        best, bi = d[0] + exit_[0], 0
        for i in range(1, W):
            v = d[i] + exit_[i]
            if v > best:
                best, bi = v, i
        nd = []
        for j in range(W):
            st, sw = d[j] + stay[j], best + enter[j]
            if st >= sw:
                nd.append(st + obs[j])
            else:
                nd.append(sw + obs[j])
                back[t][j] = bi
        d = nd
    j = 0
    for i in range(1, W):
        if d[i] > d[j]:
            j = i
    score = d[j]
    frames, words = [], []
    for t in range(T - 1, -1, -1):
        b = back[t][j]
        if t == 0 or b >= 0:
            frames.append(t)
            words.append(j)
        if t > 0 and b >= 0:
            j = b
    return frames[::-1], words[::-1], score


def exp_text(frames, words, names):
    return ' '.join('%d %s' % (t, names[w]) for t, w in zip(frames, words))


def model_structure(model):
    """The structural facts of a vad_model.VadModel (and its .cfg) that tests/golden/vad_model.json
    records; trained numbers only as SHA-256 of their float64 little-endian bytes."""
    import hashlib
    h = lambda *arrs: hashlib.sha256(b''.join(np.ascontiguousarray(a, dtype='<f8').tobytes()
                                             for a in arrs)).hexdigest()
    cfg = model.cfg
    return {
        'gk': {'n_kernels': int(model.n_kernels), 'dim': int(model.dim), 'covariance': 'diagonal_cov',
               'sha256': h(model.means, model.variances)},
        'mc': {'n_states': int(model.n_states), 'kernels': [[int(k) for k in ks] for ks, _ in model.mixtures],
               'zero_weights': [int((ws == 0).sum()) for _, ws in model.mixtures],
               'sha256': h(*[ws for _, ws in model.mixtures])},
        'words': list(model.words), 'word_state': [int(s) for s in model.word_state],
        'transitions_sha256': h(model.a_stay, model.a_exit), 'lm_sha256': h(model.log10p),
        'cfg': {'sample_rate': cfg.sample_rate, 'frame_rate': cfg.frame_rate, 'window_width': cfg.window_width,
                'pre_emph': cfg.pre_emph, 'n_cep': cfg.n_cep, 'cms_left': cfg.cms_left, 'cms_right': cfg.cms_right,
                'delta_width': cfg.delta_width, 'delta_norm': cfg.delta_norm, 'dim': cfg.dim,
                'arrays_sha256': h(cfg.mean, cfg.scale, cfg.transform)},
    }
