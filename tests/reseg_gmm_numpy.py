"""CPU restatement (numpy, float64) of resegmentation under mixture models -- TEST INFRASTRUCTURE ONLY.

PARITY: no reference counterpart.  The reference stops at clustering; what spkd_gmm_train and
spkd_gmm_loglik_seq compute (include/spkd.h, section 9) is stated here; the decoder and the rows are
reseg_numpy's.

  model     [K, 80] doubles, a row per component: ln w, mean[39], 1 / var[39],
            log_norm = -1/2 (39 ln 2pi + sum ln var).
  floor     var_floor * V_d, V_d the ML (biased) variance of all N frames of the speaker.
  initial   component k takes the frames with the ordinals [floor(k N / K), floor((k + 1) N / K)):
            w = count / N, their mean and ML variance, floored.
  EM step   l_k = ln w_k + log_norm_k - 1/2 sum_d (x_d - mean_kd)^2 (1 / var)_kd, m = max_k l_k,
            g_k = exp(l_k - m) / sum_j exp(l_j - m) over the components whose ln w is not -inf;
            G_k = sum g_k, A_k = sum g_k x, B_k = sum g_k x^2, L = sum (m + ln sum_j exp(l_j - m));
            w_k = G_k / N and, when G_k >= 2, mean = A / G, var = max(B / G - mean^2, floor);
            otherwise the component keeps its mean and variance.
  ok        N >= 40 K, every V_d finite and > 0, every accumulator and L finite, every value written
            finite (ln w may be -inf).
  scores    m + ln sum_j exp(l_j - m) per frame and model, -inf for a model that is not ok and for
            the columns past a sequence's models; float64 (the device rounds once to float32).
"""
import math

import numpy as np

import reseg_numpy as R

DIM = 39
COMP = 80           # SPKD_GMM_COMP
MAX_COMP = 8        # SPKD_GMM_MAX_COMP
TILE = 64           # SPKD_GMM_TILE
CHUNK_TILES = 16    # SPKD_GMM_CHUNK_TILES
MEAN, IVAR, NORM = 1, 1 + DIM, COMP - 1
MIN_PER_COMP = DIM + 1
LN_2PI = math.log(2.0 * math.pi)


def _f64(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64).reshape(-1, DIM)


def variance_floor(x, var_floor):
    """(floor [39], ok): var_floor times the ML variance of all the frames; ok when each is a finite number > 0."""
    x = _f64(x)
    with np.errstate(all='ignore'):
        n = float(len(x))
        v = (x * x).sum(axis=0) / n - (x.sum(axis=0) / n) ** 2 if len(x) else np.full(DIM, np.nan)
    return var_floor * v, bool(np.isfinite(v).all() and (v > 0.0).all())


def _m_step(g_sum, a, b, n, floor, old):
    """The model of the accumulators G [K], A [K, 39], B [K, 39]; old: the model whose components stay
    where G_k < 2 (None: mean 0, variance 1).  Returns (model, every accumulator and value finite)."""
    k_comp = len(g_sum)
    out = np.zeros((k_comp, COMP))
    fin = bool(np.isfinite(g_sum).all() and np.isfinite(a).all() and np.isfinite(b).all())
    with np.errstate(all='ignore'):
        for k in range(k_comp):
            out[k, 0] = np.log(g_sum[k] / n)
            if g_sum[k] >= 2.0:
                mean = a[k] / g_sum[k]
                var = b[k] / g_sum[k] - mean * mean
                var = np.where(var < floor, floor, var)
                out[k, MEAN:IVAR] = mean
                out[k, IVAR:NORM] = 1.0 / var
                out[k, NORM] = -0.5 * (DIM * LN_2PI + np.log(var).sum())
            elif old is None:
                out[k, IVAR:NORM] = 1.0
                out[k, NORM] = -0.5 * DIM * LN_2PI
            else:
                out[k, MEAN:] = old[k, MEAN:]
    fin = fin and bool(np.isfinite(out[:, MEAN:]).all() and (out[:, IVAR:NORM] > 0.0).all())
    return out, fin


def init_model(x, k_comp, var_floor):
    """(model [K, 80], ok) of the frames x [N, 39]: the segmental start."""
    x = _f64(x)
    n = len(x)
    floor, ok = variance_floor(x, var_floor)
    edge = [k * n // k_comp for k in range(k_comp + 1)]
    with np.errstate(all='ignore'):
        g_sum = np.array([float(edge[k + 1] - edge[k]) for k in range(k_comp)])
        a = np.array([x[edge[k]:edge[k + 1]].sum(axis=0) for k in range(k_comp)]).reshape(k_comp, DIM)
        b = np.array([(x[edge[k]:edge[k + 1]] ** 2).sum(axis=0) for k in range(k_comp)]).reshape(k_comp, DIM)
        model, fin = _m_step(g_sum, a, b, float(n), floor, None)
    return model, bool(ok and fin and n >= MIN_PER_COMP * k_comp)


def component_loglik(x, model):
    """l [N, K] of the frames under each component; nan marks a component whose ln w is -inf (it takes no part)."""
    x = _f64(x)
    out = np.full((len(x), len(model)), np.nan)
    with np.errstate(all='ignore'):
        for k, c in enumerate(model):
            if c[0] != -np.inf:
                d = x - c[MEAN:IVAR]
                out[:, k] = c[0] + c[NORM] - 0.5 * (d * d * c[IVAR:NORM]).sum(axis=1)
    return out


def _logsumexp(l, live):
    """(m + ln sum exp(l - m) [N], exp(l - m) [N, K], the sum [N]) over the live components."""
    n = len(l)
    with np.errstate(all='ignore'):
        if not live.any():
            return np.full(n, -np.inf), np.zeros_like(l), np.zeros(n)
        m = np.max(l[:, live], axis=1)
        e = np.zeros_like(l)
        e[:, live] = np.exp(l[:, live] - m[:, None])
        s = e.sum(axis=1)
        return m + np.log(s), e, s


def em_step(x, model, var_floor):
    """One EM step from `model` on the frames x -> (model, L of the model that entered, every
    accumulator and value finite).  The floor and the first ok are variance_floor's."""
    x = _f64(x)
    model = np.asarray(model, dtype=np.float64).reshape(-1, COMP)
    n = float(len(x))
    floor, _ = variance_floor(x, var_floor)
    live = model[:, 0] != -np.inf
    with np.errstate(all='ignore'):
        ll, e, s = _logsumexp(component_loglik(x, model), live)
        g = e / s[:, None]
        total = float(ll.sum())
        new, fin = _m_step(g.sum(axis=0), g.T @ x, g.T @ (x * x), n, floor, model)
    return new, total, bool(fin and np.isfinite(total))


def train(x, k_comp, n_iter, var_floor, model=None):
    """spkd_gmm_train for one speaker: (model, ok, [L per iteration]); model: the start (from_model)."""
    x = _f64(x)
    floor_ok = variance_floor(x, var_floor)[1] and len(x) >= MIN_PER_COMP * k_comp
    if model is None:
        model, ok = init_model(x, k_comp, var_floor)
    else:
        ok = bool(floor_ok and np.isfinite(x).all())
    out = []
    for _ in range(n_iter):
        model, total, fin = em_step(x, model, var_floor)
        ok = ok and fin
        out.append(total)
    return model, bool(ok), out


def scores(x, models, ok, n_cols):
    """x [T, 39] float32 -> [T, n_cols] float64 under models = [[K, 80]] (ok[k] false: -inf)."""
    x = _f64(x)
    out = np.full((len(x), n_cols), -np.inf)
    for k, (mod, good) in enumerate(zip(models, ok)):
        if good:
            mod = np.asarray(mod, dtype=np.float64).reshape(-1, COMP)
            out[:, k] = _logsumexp(component_loglik(x, mod), mod[:, 0] != -np.inf)[0]
    return out


def resegment(feats, turns, segs, reseg):
    """The stage on one file: turns [(begin, end)] in frames, segs [(begin, end, speaker)] the input
    segmentation, reseg a dictionary like pipeline.RESEG_GMM.  A speaker trains on the frames of its
    segments in segment order; every turn is scored under the speakers (ascending) and decoded by
    reseg_numpy.viterbi.  Returns (speakers, per turn (token first frames, token speaker indices),
    ok per speaker, L per speaker and iteration)."""
    spk = sorted(set(s[2] for s in segs))
    models, oks, lls = [], [], []
    for sp in spk:
        x = np.concatenate([feats[b:e] for b, e, k in segs if k == sp])
        m, ok, ll = train(x, reseg['components'], reseg['iterations'], reseg['var_floor'])
        models.append(m); oks.append(ok); lls.append(ll)
    decoded = []
    for a, b in turns:
        sc = scores(feats[a:b], models, oks, len(spk)).astype(np.float32)
        frames, words, _ = R.viterbi(sc, reseg['penalty'])
        decoded.append((frames, words))
    return spk, decoded, oks, lls
