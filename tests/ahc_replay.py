"""The merge loop of spk_cluster_hi (spk-clustering.py:201-240, spk-clustering2.py:185-222) on a SUPPLIED
initial matrix, restated literally as oracle/numpy_engine.py::cluster_hi does: dm.min() and dm.argmin() over
the whole current matrix, np.delete of row and column b, row a rewritten (variant 1: column a too, and the
`note` rule for the running max / min; variant 2: max / min of the final matrix).  CPU only; it models no row
cache and costs O(n^2) per round.  TEST INFRASTRUCTURE ONLY.

Fresh distances come from a callback dist(cluster_a, cluster_s), the merged cluster first as in the reference.

Beside the log the replay keeps an ORIGIN KEY per cell:
    ('planted', value id)                      a cell the scenario planted
    ('fill', what)                             the diagonal / variant 2's lower triangle
    ('computed', canon(first), canon(second))  a computed distance, ordered as computed; canon maps a cluster to
                                               the sorted multiset of its frame ranges, so duplicate records share
                                               a key; variant 1's mirrored cell shares the key of what it copies
and records per round the winner, whether the minimum was NaN, the GAP (below) and the events of
tests/ahc_replay_cases.py.

The gap of a round is the smallest (v - min) / max(1, |min|) over the alive cells that could decide differently
on the device: cells whose origin key differs from the winner's (or that share it without sharing its bits),
except that zeros of either sign under one key are one value, and that against a +inf minimum every +inf cell
is the same value wherever it comes from (a computed +inf is the exact -inf log determinant of an all-zero
record).  The threshold gap is |min - threshold| / max(1, |min|) where the threshold
decides and the minimum was computed; None where max_spk forces the merge or the minimum is planted (exact)."""
import math

import numpy as np

MAXINT = 9223372036854775807
MARGIN = 1e-7                      # 100 times the 1e-9 the device is held to against the C oracle
EXACT = ('planted', 'fill')


class Cluster(object):
    """tree: nested tuple of frame ranges in merge order (what fixes the bits of the summed statistics);
    canon: the sorted multiset of the ranges; stats: the summed packed record (or None)."""
    __slots__ = ('tree', 'canon', 'stats')

    def __init__(self, tree, canon, stats):
        self.tree, self.canon, self.stats = tree, canon, stats

    @staticmethod
    def leaf(rng, stats=None):
        rng = (int(rng[0]), int(rng[1]))
        return Cluster(rng, (rng,), stats)

    def merged(self, other):
        st = None if self.stats is None else self.stats + other.stats       # speakers[a].extend(speakers[b])
        return Cluster((self.tree, other.tree), tuple(sorted(self.canon + other.canon)), st)


def initial_keys(clusters, variant):
    """Origin keys of the unplanted initial matrix: (s1, s2), s1 < s2, is dist(s1, s2)."""
    n = len(clusters)
    K = np.empty((n, n), dtype=object)
    for i in range(n):
        for j in range(n):
            if i == j:
                K[i, j] = ('fill', 'diag')
            elif i < j or variant == 1:
                lo, hi = min(i, j), max(i, j)
                K[i, j] = ('computed', clusters[lo].canon, clusters[hi].canon)
            else:
                K[i, j] = ('fill', 'lower')
    return K


def _bits(v):
    return np.float64(v).view(np.uint64)


def _row_entries(dm):
    """Per row: minimum over the non-NaN cells, its first column, the first NaN column (-1: none)."""
    nanm = np.isnan(dm)
    rn = np.where(nanm.any(axis=1), nanm.argmax(axis=1), -1)
    t = np.where(nanm, np.inf, dm)
    rm = t.min(axis=1)
    eq = (t == rm[:, None]) & ~nanm
    ra = np.where(eq.any(axis=1), eq.argmax(axis=1), -1)
    return rm, ra, rn


def replay(clusters, M, K, variant, threshold, max_spk, dist):
    """-> dict: merges [(a, b, d, origin kind)], max_dist, min_dist (None: never set), their origin kinds,
    degenerate (a diagonal cell won: the loop stops, as in the C oracle and on the device),
    rounds [per decision: gap, threshold gap, nan], events {name: count}, where {name: [largest merge index,
    largest slot column]}.  M, K: the initial matrix and its origin keys (both n x n, not modified)."""
    clusters = list(clusters)
    n = len(clusters)
    dm = np.array(M, dtype=np.float64)
    keys = np.array(K, dtype=object)
    written = np.full((n, n), -1, dtype=np.int64)        # merge index that wrote the cell (-1: initial)
    slot = list(range(n))                                # compacted index -> record slot
    stat = {'max': None, 'min': None, 'max_kind': None, 'min_kind': None}
    events, where = {}, {}

    def ev(name, merge, col=0):
        events[name] = events.get(name, 0) + 1
        w = where.setdefault(name, [0, 0])
        w[0], w[1] = max(w[0], merge), max(w[1], col)

    def note(d, kind):
        if d != math.inf and d != -math.inf:
            if stat['max'] is None and d > 0 or stat['max'] is not None and d > stat['max']:
                stat['max'], stat['max_kind'] = d, kind
            if stat['min'] is None and d < MAXINT or stat['min'] is not None and d < stat['min']:
                stat['min'], stat['min_kind'] = d, kind

    if variant == 1:
        for s1 in range(n):
            for s2 in range(s1 + 1, n):
                note(float(dm[s1, s2]), keys[s1, s2][0])
    merges, rounds = [], []
    degenerate = False
    pending = None                  # (slot x, slot sa) of the lowest row whose fresh NaN only the in-place rule sees
    touched = {}                    # slot -> last merge that rewrote the row or flagged its entry for a rescan
    with np.errstate(all='ignore'):
        while True:
            m = len(clusters)
            k = len(merges)
            mind = float(dm.min())
            forced = max_spk > 0 and m > max_spk
            go = mind <= threshold or forced
            index = int(dm.argmin())
            r, c = index // m, index % m
            wkey = keys[r, c]
            rec = {'nan': math.isnan(mind), 'gap': None, 'thr_gap': None}
            if not rec['nan']:
                scale = max(1.0, abs(mind))
                same = np.zeros((m, m), dtype=bool)
                near = np.argwhere(~(dm > mind + 10.0 * MARGIN * scale) & ~np.isnan(dm))
                for i, j in near:
                    kk = keys[i, j]
                    same[i, j] = kk == wkey and (_bits(dm[i, j]) == _bits(mind) or
                                                 (dm[i, j] == 0.0 and mind == 0.0))
                if mind == np.inf:
                    same |= dm == np.inf
                rest = dm[~same & ~np.isnan(dm)]
                rec['gap'] = float((rest.min() - mind) / scale) if rest.size else None
                if not forced and wkey[0] not in EXACT:
                    rec['thr_gap'] = abs(mind - threshold) / scale
            rounds.append(rec)
            if not go:
                break
            a, b = min(r, c), max(r, c)
            if a == b:                       # a diagonal cell won: the C oracle and the device stop here
                degenerate = True
                break
            merges.append((a, b, mind, wkey[0]))
            # ---- events of the selection
            if rec['nan']:
                nanm = np.isnan(dm)
                assert not nanm[:r].any() and not nanm[r, :c].any()
                ev('E6_first_nan', k, slot[c])
                if pending == (slot[r], slot[c]) and nanm[r + 1:c].any():
                    ev('E6b_fresh_nan_decides', k, slot[c])
                if c < m - 1 and nanm[r, m - 1] and keys[r, m - 1][0] == 'planted':
                    ev('E6a_last_column', k, slot[m - 1])
            else:
                tie = dm == mind
                for c2 in np.nonzero(tie[r])[0]:
                    if c2 > c and slot[c2] - slot[c] >= 64:
                        ev('E1_row_tie', k, slot[c2])
                    if c2 > c and variant == 1 and written[r, c] > written[r, c2] >= 0 and r < c:
                        ev('E4_tie_wins', k, slot[c2])
                for r2, c2 in np.argwhere(tie):
                    if r2 > r and not (variant == 1 and c2 == r) and slot[r2] // 64 != slot[r] // 64:
                        ev('E2_rows_tie', k, slot[c2])
                if k > 0 and written[r, c] == k - 1:
                    for r2, c2 in np.argwhere(tie & (written == k - 1)):
                        if (r2, c2) != (r, c) and (r2, c2) != (c, r):
                            ev('E3_fresh_tie', k, slot[c2])
                            break
                if mind == 0.0:
                    sgn = np.signbit(dm) & tie
                    if sgn.any() and (tie & ~sgn).any():
                        other = tie & (np.signbit(dm) != np.signbit(dm[r, c]))
                        tag = 'm' if np.signbit(dm[r, c]) else 'p'
                        if any(abs(slot[c2] - slot[c]) >= 64 for c2 in np.nonzero(other[r])[0]):
                            ev('E7_row_' + tag, k, slot[c])
                        if any(r2 != r and (r2, c2) != (c, r) for r2, c2 in np.argwhere(other)):
                            ev('E7_rows_' + tag, k, slot[c])
                        if k >= 1 and written[r, c] == -1 and slot[r] not in touched:
                            ev('E7_kept_in_place', k, slot[c])
            # a row all of whose off-diagonal alive cells are NaN or +inf, one of them a planted +inf
            offd = ~np.eye(m, dtype=bool)
            dull = (np.isnan(dm) | (dm == np.inf)) | ~offd
            for x in np.nonzero(dull.all(axis=1))[0]:
                if any(keys[x, j][0] == 'planted' and dm[x, j] == np.inf for j in range(m) if j != x):
                    ev('E8_inf_row', k, slot[x])
                    break
            # ---- the merge
            rm, ra, rn = _row_entries(dm)
            pending = None
            touched[slot[a]] = k
            clusters[a] = clusters[a].merged(clusters[b])
            clusters.pop(b)
            slot.pop(b)
            dm = np.delete(np.delete(dm, b, axis=0), b, axis=1)
            keys = np.delete(np.delete(keys, b, axis=0), b, axis=1)
            written = np.delete(np.delete(written, b, axis=0), b, axis=1)
            for s2 in range(len(clusters)):
                if s2 == a:
                    continue
                d = float(dist(clusters[a], clusters[s2]))
                key = ('computed', clusters[a].canon, clusters[s2].canon)
                dm[a, s2], keys[a, s2], written[a, s2] = d, key, k
                if variant == 1:
                    dm[s2, a], keys[s2, a], written[s2, a] = d, key, k
                    note(d, 'computed')
                # ---- events of a partner row's entry (x: the row's index before the merge)
                x = s2 if s2 < b else s2 + 1
                if variant == 1:
                    nan_hit = rn[x] in (a, b)
                    if ra[x] in (a, b) or nan_hit:
                        touched[slot[s2]] = k
                        if ra[x] in (a, b) and not nan_hit and not d < rm[x]:
                            ev('E5_rescan', k, slot[s2])
                    elif math.isnan(d):
                        if rn[x] >= 0 and a < rn[x]:
                            ev('E6b_fresh_nan_lower', k, slot[a])
                        if x < a and (rn[x] < 0 or a < rn[x]) and pending is None:
                            pending = (slot[s2], slot[a])
                    elif ra[x] >= 0 and d == rm[x]:
                        ev('E4_column_tie_lower' if a < ra[x] else 'E4_column_tie_higher', k, slot[a])
                else:
                    if ra[x] == b or rn[x] == b:
                        touched[slot[s2]] = k
                    if ra[x] == b:
                        ev('E5_rescan', k, slot[s2])
                    if rn[x] == b:
                        ev('E6c_first_nan_at_sb', k, slot[s2])
        if variant == 2:
            fmax, fmin = float(dm.max()), float(dm.min())
            stat['max'], stat['min'] = fmax, fmin
            for name, v in (('max', fmax), ('min', fmin)):
                if math.isnan(v):
                    stat[name + '_kind'] = 'nan'
                else:
                    i, j = np.argwhere(dm == v)[0]
                    stat[name + '_kind'] = keys[i, j][0]
            if np.isnan(dm).any():
                ev('E8_final_nan', len(merges))
    return {'merges': merges, 'max_dist': stat['max'], 'min_dist': stat['min'], 'max_kind': stat['max_kind'],
            'min_kind': stat['min_kind'], 'rounds': rounds, 'events': events, 'where': where,
            'degenerate': degenerate}


def unsafe_rounds(rounds, margin=MARGIN):
    """The decisions of a replay that do not meet the safety condition: [(round, what, value)]."""
    bad = []
    for k, r in enumerate(rounds):
        if r['gap'] is not None and not r['gap'] > margin:
            bad.append((k, 'gap', r['gap']))
        if r['thr_gap'] is not None and not r['thr_gap'] > margin:
            bad.append((k, 'threshold', r['thr_gap']))
    return bad
