"""CPU restatement of the self-trained speech / non-speech detector -- TEST INFRASTRUCTURE ONLY.

PARITY: no reference counterpart (the reference loads an AaltoASR model).  What spkd_frame_energy_batch,
spkd_energy_seeds (include/spkd.h, section 6c) and self_vad.decode_batch compute is stated here:

  energy    frame t of a file covers its samples t hop .. t hop + window - 1, 0 past the file's end;
            E = window sum s^2 - (sum s)^2 in int64 numpy.
  seeds     lo = the k_low-th smallest energy by np.sort, hi = the k_high-th largest; seeded when both k
            lie in [1, T] and lo < hi; class 0 the maximal runs with E <= lo, class 1 those with E >= hi.
  decode    the loop of self_vad.py over the restatements that exist: reseg_gmm_numpy (training and
            scores), reseg_mindur_numpy (the minimum-duration decoder); oracle/mfcc_numpy.py gives the
            features.
  talk      tests/test_mfcc_batch.py's _talk with the stretches it draws.
"""
import math

import numpy as np

import reseg_gmm_numpy as G
import reseg_mindur_numpy as M

WORDS = ('<w>', 'p')


def energy(pcm, hop, window):
    """int64 [len(pcm) // hop]."""
    s = np.asarray(pcm).astype(np.int64)
    T = len(s) // hop
    padded = np.concatenate([s, np.zeros(window, dtype=np.int64)])
    out = np.zeros(T, dtype=np.int64)
    for t in range(T):
        w = padded[t * hop:t * hop + window]
        out[t] = window * int((w * w).sum()) - int(w.sum()) ** 2
    return out


def energy_fast(pcm, hop, window):
    """The same values from prefix sums (for the long files of the tests; checked against energy())."""
    s = np.asarray(pcm).astype(np.int64)
    T = len(s) // hop
    padded = np.concatenate([[0], s, np.zeros(window, dtype=np.int64)])
    c1, c2 = np.cumsum(padded), np.cumsum(padded * padded)
    at = np.arange(T, dtype=np.int64) * hop
    s1, s2 = c1[at + window] - c1[at], c2[at + window] - c2[at]
    return window * s2 - s1 * s1


def runs(flag):
    """[(begin, end)] of the maximal runs of True."""
    f = np.concatenate([[False], np.asarray(flag, dtype=bool), [False]])
    d = np.diff(f.astype(np.int8))
    return list(zip(np.nonzero(d == 1)[0].tolist(), np.nonzero(d == -1)[0].tolist()))


def seeds_file(e, k_low, k_high):
    """(lo, hi, seeded, (class 0 runs, class 1 runs)) of one file's energies; frames relative to the file."""
    e = np.asarray(e, dtype=np.int64)
    T = len(e)
    if not (1 <= k_low <= T and 1 <= k_high <= T):
        return 0, 0, 0, ([], [])
    order = np.sort(e)
    lo, hi = int(order[k_low - 1]), int(order[T - k_high])
    if not lo < hi:
        return lo, hi, 0, ([], [])
    return lo, hi, 1, (runs(e <= lo), runs(e >= hi))


def seeds(energies, k_low, k_high):
    """spkd_energy_seeds for the files' energies -> (lo, hi, seeded, run_off, run_begin, run_end), absolute frames."""
    lo, hi, seeded, off, begin, end = [], [], [], [0], [], []
    first = 0
    for e, kl, kh in zip(energies, k_low, k_high):
        a, b, s, r = seeds_file(e, int(kl), int(kh))
        lo.append(a); hi.append(b); seeded.append(s)
        for c in (0, 1):
            begin += [first + x for x, _ in r[c]]
            end += [first + y for _, y in r[c]]
            off.append(len(begin))
        first += len(e)
    i64 = lambda v: np.array(v, dtype=np.int64)
    return i64(lo), i64(hi), np.array(seeded, dtype=np.int32), i64(off), i64(begin), i64(end)


def token_ranges(tokens, n_frames):
    out = ([], [])
    for (at, word), nxt in zip(tokens, [t for t, _ in tokens[1:]] + [n_frames]):
        out[word].append((at, nxt))
    return out


def _train(feats, ranges, opts):
    """(the two models, both ok) of a file from its two classes' ranges; nothing to train a class on: not ok."""
    if not (ranges[0] and ranges[1]):
        return None, False
    out = [G.train(np.concatenate([feats[b:e] for b, e in r]), opts['components'], opts['iterations'], opts['var_floor'])
           for r in ranges]
    return [m for m, _, _ in out], all(ok for _, ok, _ in out)


def decode_batch(feats, energies, opts, rate):
    """self_vad.decode_batch on the files' features [T, 39] and energies -> (tokens [(frame, 'p' | '<w>')] per
    file, untrained files, passes run)."""
    n = len(feats)
    D = max(1, int(math.floor(opts['min_dur_s'] * rate)))
    models = {}
    for f in range(n):
        T = len(feats[f])
        kl, kh = int(math.floor(opts['low_share'] * T)), int(math.floor(opts['high_share'] * T))
        _, _, seeded, r = seeds_file(energies[f], kl, kh)
        if seeded:
            m, ok = _train(feats[f], r, opts)
            if ok:
                models[f] = m
    untrained = [f for f in range(n) if f not in models]
    tokens = [[] for _ in range(n)]
    passes_run = 0
    for p in range(opts['passes']):
        live = sorted(models)
        if not live:
            break
        passes_run += 1
        same = True
        for f in live:
            sc = G.scores(feats[f], models[f], [True, True], 2).astype(np.float32)
            frames, words, _ = M.viterbi(sc, opts['penalty'], D)
            new = list(zip([int(t) for t in frames], [int(w) for w in words]))
            same = same and new == tokens[f]
            tokens[f] = new
        if p == opts['passes'] - 1 or same:
            break
        trained = {f: _train(feats[f], token_ranges(tokens[f], len(feats[f])), opts) for f in live}
        models = {f: m for f, (m, ok) in trained.items() if ok}
    return [[(t, WORDS[w]) for t, w in toks] for toks in tokens], untrained, passes_run


def talk(seconds, seed, rate=16000):
    """test_mfcc_batch._talk, statement for statement (the same draws from the same generator), and the
    stretches it draws: (samples, [(start_s, end_s)]), a sample n being inside when start < n / rate < end."""
    rng = np.random.default_rng(seed)
    t = np.arange(int(seconds * rate)) / rate
    x = 200 * rng.standard_normal(len(t))
    at, voice = 0.7, 0
    stretches = []
    while at < seconds - 1.0:
        length = rng.uniform(1.5, 3.0)
        on = (t > at) & (t < min(at + length, seconds - 0.5))
        stretches.append((at, min(at + length, seconds - 0.5)))
        f0 = (120.0, 210.0)[voice]
        x += on * sum(2000 / h * np.sin(2 * np.pi * f0 * h * t) for h in range(1, 8))
        at += length + rng.uniform(0.8, 1.5)
        voice = 1 - voice
    return np.clip(x, -32768, 32767).astype(np.int16), stretches


def truth_runs(stretches, n_frames, hop, rate=16000):
    """Frame t is speech when sample t hop lies inside a stretch -> [(begin, end)] in frames."""
    at = np.arange(n_frames) * hop / rate
    flag = np.zeros(n_frames, dtype=bool)
    for a, b in stretches:
        flag |= (at > a) & (at < b)
    return runs(flag)


def speech_runs(tokens, n_frames):
    """The decoded 'p' runs [(begin, end)] of one file's tokens."""
    ends = [t for t, _ in tokens[1:]] + [n_frames]
    return [(t, e) for (t, w), e in zip(tokens, ends) if w == 'p']


def border_errors(tokens, stretches, n_frames, hop):
    """(decoded 'p' runs, true runs, the largest distance of a border from its true one, or None when the
    counts differ)."""
    got, want = speech_runs(tokens, n_frames), truth_runs(stretches, n_frames, hop)
    if len(got) != len(want):
        return got, want, None
    worst = max([max(abs(a - c), abs(b - d)) for (a, b), (c, d) in zip(got, want)] or [0])
    return got, want, worst
