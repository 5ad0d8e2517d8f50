"""CPU restatement of the speaker posteriors (spkd_fb_posterior_batch) -- TEST INFRASTRUCTURE ONLY.

PARITY: no reference counterpart.  The reference stops at clustering; what the call computes is
stated in include/spkd.h (8) and here:

  posterior    the recursion of the header, literally, in the dtype asked for (np.float64, or
               np.longdouble as the yardstick of the device): cleaned scores o, b = exp(scale (o - m)),
               the normalised forward a with the log-evidence, the normalised backward beta, gamma.
  confidence   per token the mean of its word's gamma over its frames.
  brute_force  an independent check: every one of the n^T paths in np.longdouble, a path's log-weight
               scale * (sum_t o_t(k_t) - penalty * (1 + switches)); logz their log-sum, gamma_t(k) the
               share of the paths that are in word k at frame t.
"""
import itertools

import numpy as np


def cleaned(sc, n, dtype):
    """o_t(k), k < n, of sc [T, W] float32 as [T, n] dtype: NaN counts as -inf, a frame whose n words are
    all -inf as 0 for each."""
    o = np.asarray(sc, dtype=np.float32)[:, :n].astype(dtype)
    o[np.isnan(o)] = -np.inf
    o[np.all(o == -np.inf, axis=1)] = 0
    return o


def posterior(sc, penalty, scale=1.0, n=None, dtype=np.float64):
    """(gamma [T, W] dtype with 0 in the columns >= n, logz) of sc [T, W] float32 scores."""
    sc = np.asarray(sc, dtype=np.float32)
    T, W = sc.shape
    n = W if n is None else int(n)
    assert 1 <= n <= W
    gamma = np.zeros((T, W), dtype=dtype)
    if T == 0:
        return gamma, dtype(-np.inf)
    scale, penalty = dtype(scale), dtype(penalty)
    o = cleaned(sc, n, dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        m = o.max(axis=1)
        b = np.exp(scale * (o - m[:, None]))
        q = np.exp(-scale * penalty)
        r = dtype(1) - q
        a = np.zeros((T, n), dtype=dtype)
        logz = -scale * penalty
        for t in range(T):
            u = b[t] if t == 0 else b[t] * (r * a[t - 1] + q)
            s = u.sum()
            a[t] = u / s
            logz = logz + (scale * m[t] + np.log(s))
        beta = np.ones(n, dtype=dtype)
        for t in range(T - 1, -1, -1):
            if t < T - 1:
                h = b[t + 1] * beta
                w = r * h + q * h.sum()
                beta = w / w.sum()
            g = a[t] * beta
            gamma[t, :n] = g / g.sum()
    return gamma, logz


def confidence(gamma, tok_frame, tok_word):
    """Per token (first frame f_i, word) of one sequence the mean of gamma_t(word) over [f_i, f_{i+1}); the
    last token runs to T."""
    T = len(gamma)
    ends = list(tok_frame[1:]) + [T]
    return np.array([gamma[int(f):int(e), int(w)].mean() for f, e, w in zip(tok_frame, ends, tok_word)],
                    dtype=gamma.dtype)


def brute_force(sc, penalty, scale=1.0, n=None):
    """(gamma [T, W], logz) in np.longdouble from all n^T paths."""
    L = np.longdouble
    sc = np.asarray(sc, dtype=np.float32)
    T, W = sc.shape
    n = W if n is None else int(n)
    gamma = np.zeros((T, W), dtype=L)
    if T == 0:
        return gamma, L(-np.inf)
    o = cleaned(sc, n, L)
    scale, penalty = L(scale), L(penalty)
    paths = list(itertools.product(range(n), repeat=T))
    lw = np.empty(len(paths), dtype=L)
    for i, p in enumerate(paths):
        switches = sum(1 for t in range(1, T) if p[t] != p[t - 1])
        total = L(0)
        for t in range(T):
            total = total + o[t, p[t]]
        lw[i] = scale * (total - penalty * L(1 + switches))
    top = lw.max()
    wgt = np.exp(lw - top)
    z = wgt.sum()
    for i, p in enumerate(paths):
        for t in range(T):
            gamma[t, p[t]] += wgt[i]
    return gamma / z, top + np.log(z)
