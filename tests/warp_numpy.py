"""CPU restatement (numpy) of feature warping -- TEST INFRASTRUCTURE ONLY.

PARITY: no reference counterpart.  The reference links nothing across files; what spkd_feature_warp computes
(include/spkd.h, section 10b) and what pipeline.link_batch does with LINK_CLR_WARP is stated here, frame by
frame.  Nothing here knows of tiles.

  set       one file's speech: frame ranges [begin, end), ascending and disjoint; concatenated they are the
            compacted axis j = 0 .. L - 1.
  window    n = min(W, L); frame j sees the compacted frames [lo, lo + n), lo = clamp(j - n // 2, 0, L - n).
  counts    per dimension, v the frame's value: lt = #(window < v), eq = #(window == v), float32 compares.
  output    table_n[2 lt + eq - 1], table_n[k - 1] = float32(Phi^-1(k / (2 n))), k = 1 .. 2 n - 1.
  NaN       gives the quiet NaN 0x7fc00000 and counts in nobody's lt or eq.
"""
import statistics

import numpy as np

import link_clr_numpy as L

DIM = 39
MAX_WINDOW = 512    # SPKD_WARP_MAX_WINDOW
TILE = 384          # SPKD_WARP_TILE (the restatement does not use it: the tests place their borders by it)
QUIET_NAN = np.array([0x7fc00000], dtype=np.uint32).view(np.float32)[0]

_tables = {}


def table(n):
    """float32 [2 n - 1]: Phi^-1(k / (2 n)) for k = 1 .. 2 n - 1 -- the lower half in fp64 (k / (2 n) is
    the correctly rounded quotient there, 1 - it above the middle is not), 0 in the middle, the upper half its
    mirror image."""
    if n not in _tables:
        inv = statistics.NormalDist().inv_cdf
        low = [inv(k / (2.0 * n)) for k in range(1, n)]
        _tables[n] = np.array(low + [0.0] + [-v for v in reversed(low)], dtype=np.float64).astype(np.float32)
    return _tables[n]


def warp_set(x, window, tab=None):
    """The warped frames of one set: x [L, 39] float32 on its compacted axis -> [L, 39] float32."""
    x = np.asarray(x, dtype=np.float32).reshape(-1, DIM)
    n_frames = len(x)
    out = np.empty_like(x)
    if n_frames == 0:
        return out
    n = min(int(window), n_frames)
    tab = table(n) if tab is None else tab
    assert len(tab) == 2 * n - 1
    with np.errstate(invalid='ignore'):
        for j in range(n_frames):
            lo = min(max(j - n // 2, 0), n_frames - n)
            w, v = x[lo:lo + n], x[j]
            lt = (w < v).sum(axis=0)
            eq = (w == v).sum(axis=0)
            nan = np.isnan(v)
            assert (eq[~nan] >= 1).all()
            out[j] = np.where(nan, QUIET_NAN, tab[np.where(nan, 0, 2 * lt + eq - 1)])
    return out


def warp(frames, sets, window, out=None):
    """spkd_feature_warp: frames [T, 39]; sets: per set its [(begin, end)], ascending and disjoint over the
    whole list.  Returns out [T, 39] float32 (given, or zeros): a frame in no range keeps what it held."""
    frames = np.asarray(frames, dtype=np.float32).reshape(-1, DIM)
    out = np.zeros_like(frames) if out is None else out
    last = 0
    for runs in sets:
        for b, e in runs:
            assert last <= b <= e <= len(frames)
            last = e
        idx = np.concatenate([np.arange(b, e) for b, e in runs] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        out[idx] = warp_set(frames[idx], window)
    return out


def speech_runs(ranges):
    """A file's segment ranges [(begin, end)] as the runs of its speech: sorted, the overlapping and the
    touching ones merged, an empty one dropped."""
    runs = []
    for b, e in sorted((int(b), int(e)) for b, e in ranges if e > b):
        if runs and b <= runs[-1][1]:
            runs[-1][1] = max(runs[-1][1], e)
        else:
            runs.append([b, e])
    return [(b, e) for b, e in runs]


def link(feats, speakers, files, link):
    """pipeline.link_batch(link=LINK_CLR_WARP) on speakers given as range lists: files[s] is the file of
    speaker s; a file's speech is the ranges of its speakers.  link_clr_numpy.link's return."""
    window = int(round(link['warp_s'] * 125.0))
    sets = [speech_runs([r for s, rs in enumerate(speakers) if files[s] == f for r in rs]) for f in sorted(set(files))]
    sets = sorted([r for r in sets if r], key=lambda r: r[0][0])
    return L.link(warp(feats, sets, window), speakers, link)
