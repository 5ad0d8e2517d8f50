"""Scenarios of tests/test_ahc_replay.py: planted matrices and duplicate records on which the merge loop's
tie and NaN rules decide merges past the first one, replayed by tests/ahc_replay.py (the literal loop, C oracle
distances) into tests/golden/ahc_replay.json by tests/golden/make_golden_ahc_replay.py.

Records are frame slices of one buffer: synth.make_session(*SESSION) followed by ZERO_FRAMES all-zero frames.
A duplicate is the same slice twice, at adjacent indices (P, P + 1), so that every other record is on the same
side of both and the tied cells d(x, P), d(x, P + 1) are computed in the same orientation.  Pairs have different
lengths: two equal-length pairs free to merge with each other would all score -penalty +- rounding.

Sizes: 65 = two 64-row mask chunks plus a tail lane, 130 = three chunks, 257 = a second trip of the scan's
256-column loop and of the loops over AHC_TPB threads.

Events (counted by the replay, stored in the fixture, required per variant by REQUIRED):
  E1_row_tie            the minimum twice in one row, columns >= 64 apart; the lower column wins
  E2_rows_tie           the minimum in two rows of different 64-row chunks; the first in row-major order wins
  E3_fresh_tie          both tied cells written by the previous merge: d(A', P) == d(A', P + 1)
  E4_column_tie_lower / _higher (variant 1)  the fresh value at column sa equals a partner row's standing
                        minimum at column ra, sa < ra / sa > ra (twin pairs: A2, B2 duplicate A, B; planted
                        cells fix which pair merges first, the second merged cluster duplicates the first)
  E4_tie_wins (variant 1)  the minimum twice in one row, the winning (lower) cell written by a LATER merge than the
                        other: only the in-place update of the row's entry can have put it first
  E5_rescan             a row's standing minimum sat at column sa or sb and the fresh d is not smaller (variant 2:
                        it sat at sb; the fresh d plays no part in that variant's rule)
  E6_first_nan          the minimum is NaN, the first NaN in row-major order wins
  E6a_last_column       ... with a planted NaN at the last column of the winning row
  E6b_fresh_nan_lower (variant 1)  a fresh NaN at column sa, lower than the row's standing first-NaN column
  E6b_fresh_nan_decides (variant 1)  a row x < sa took a fresh NaN at column sa by the in-place rule alone, (x, sa)
                        wins the next round, and a row between x and sa holds a NaN too (a rescanned one): without
                        the rule that row would win
  E6c_first_nan_at_sb (variant 2)  a row whose first NaN sat at column sb
  E7_row_p / _m, E7_rows_p / _m   the minimum is a zero present with both signs (threshold 0): in one row, columns
                        >= 64 apart / in different rows; the winner is +0.0 (p) / -0.0 (m)
  E7_kept_in_place      ... and the winning row's entry is the initial scan's, kept through every merge so far
  E8_inf_row            a row whose alive off-diagonal cells are all NaN but one planted +inf
  E8_final_nan (variant 2)  the final matrix still holds a NaN: the reported max / min are NaN"""
import ctypes as C
import hashlib
import math

import numpy as np

from conftest import pkg

SESSION = (4242, 150, 3)
ZERO_FRAMES = 512
SLICE = 60                         # frames of an ordinary record: a full-rank covariance
BIG_NEG = -1.0e300

REQUIRED = {
    1: ['E1_row_tie', 'E2_rows_tie', 'E3_fresh_tie', 'E4_column_tie_lower', 'E4_column_tie_higher', 'E4_tie_wins',
        'E5_rescan', 'E6_first_nan', 'E6a_last_column', 'E6b_fresh_nan_lower', 'E6b_fresh_nan_decides', 'E7_row_p',
        'E7_row_m', 'E7_rows_p', 'E7_rows_m', 'E7_kept_in_place', 'E8_inf_row'],
    2: ['E1_row_tie', 'E2_rows_tie', 'E3_fresh_tie', 'E5_rescan', 'E6_first_nan', 'E6a_last_column',
        'E6c_first_nan_at_sb', 'E7_row_p', 'E7_row_m', 'E7_rows_p', 'E7_rows_m', 'E7_kept_in_place', 'E8_inf_row',
        'E8_final_nan'],
}

VALUE = {'nan': float('nan'), 'inf': float('inf'), '+0': 0.0, '-0': -0.0}


def value_of(vid):
    """A planted value from its id: a name of VALUE or a float.hex() string.  Zeros of both signs are one value
    to numpy, so they share the origin key ('planted', 'zero')."""
    return VALUE[vid] if vid in VALUE else float.fromhex(vid)


def key_of(vid):
    return ('planted', 'zero' if vid in ('+0', '-0') else vid)


def frames():
    synth = pkg('synth')
    feats, _, _ = synth.make_session(*SESSION)
    return np.ascontiguousarray(np.concatenate([feats, np.zeros((ZERO_FRAMES, feats.shape[1]), dtype=np.float32)]))


def frames_sha256(f):
    return hashlib.sha256(np.ascontiguousarray(f).tobytes()).hexdigest()


def slice_table(n, dups=(), zeros=(), copies=(), lengths=(), covers=()):
    """n records: SLICE frames each, cut one behind the other from the session; dups: (P, length) -> records P
    and P + 1 are one slice of that length; zeros: indices that get all-zero slices; copies: (dst, src) ->
    record dst repeats the slice of record src (src < dst or not); lengths: (index, frames) of other records;
    covers: (index, first, last, margin) -> the record spans the slices of records first .. last and `margin`
    frames either side."""
    n_speech = SESSION[1] * 125
    dup_len = dict(dups)
    table, cur, z = [None] * n, 0, n_speech
    copy_of, length = dict(copies), dict(lengths)
    for i in range(n):
        if i in copy_of:
            continue
        if i in zeros:
            table[i] = (z, z + SLICE)
            z += SLICE
        elif i - 1 in dup_len:
            table[i] = table[i - 1]
        else:
            ln = dup_len.get(i, length.get(i, SLICE))
            table[i] = (cur, cur + ln)
            cur += ln
    for dst, src in copy_of.items():
        table[dst] = table[src]
    for i, first, last, margin in covers:
        table[i] = (table[first][0] - margin, table[last][1] + margin)
        assert table[i][0] >= 0 and table[last][0] == table[first][1]
    assert cur <= n_speech and z <= n_speech + ZERO_FRAMES and all(t is not None for t in table)
    return table


def _hex(v):
    return float(v).hex()


def _ladder(pairs, top, step):
    """Planted cells that merge first, in this order, each with a value of its own."""
    return [(a, b, _hex(top + step * k)) for k, (a, b) in enumerate(pairs)]


def _apart(dups):
    """A large planted cell at (P, P + 1) holds a duplicate pair apart: the two stay alive side by side, and
    every merge elsewhere writes them the tied cells d(A', P) == d(A', P + 1)."""
    return [(p, p + 1, _hex(1.0e9 + p)) for p, _ in dups]


def _base(name, n, variant, **kw):
    s = dict(name='%s_n%d_v%d' % (name, n, variant), n=n, variant=variant, kind='BIC', lambdac=1.3, threshold=0.0,
             max_spk=0, planted=[])
    s.update(kw)
    return s


DUPS = {65: [(5, 62), (20, 64), (33, 66), (47, 68), (58, 70)],
        130: [(5, 62), (20, 64), (41, 66), (63, 68), (64 + 13, 70), (101, 72), (127, 74)],
        257: [(5, 62), (40, 64), (63, 66), (99, 68), (127, 70), (160, 72), (191, 74), (230, 76), (255, 78)]}


def scenarios():
    out = []
    for variant in (1, 2):
        # ---- duplicate records, nothing planted (also the three problems of one spkd_ahc call)
        for n in (65, 130, 257):
            out.append(_base('dups', n, variant, slices=slice_table(n, DUPS[n])))
        # (GLR: a duplicate pair scores 0 whatever its length, so the pairs are held apart by planted cells)
        out.append(_base('dups_glr', 65, variant, kind='GLR', threshold=GLR_THRESHOLD,
                         slices=slice_table(65, DUPS[65]), planted=_apart(DUPS[65])))
        # ---- planted ties below every computed distance, behind a ladder of ten planted merges
        for n in (65, 130, 257):
            out.append(_planted(n, variant))
        # ---- signed zeros: lambda 0 keeps every computed distance above the threshold 0
        out.append(_zeros(130, variant))
        # ---- NaNs: max_spk forces merges through a NaN minimum
        for n in (65, 130):
            out.append(_nans(n, variant))
        # ---- past one trip of k_ahc's selection: row 520 is thread 8's second row (wave 0), row 70 is wave 1's
        out.append(_fold(variant))
    # ---- a +inf minimum: max_spk = 1 forces variant 2 on until one cluster and the all-zero record are left; numpy's
    # first +inf is then the diagonal of the first alive row, and the loop stops there as degenerate
    out.append(_base('infs', 65, 2, threshold=BIG_NEG, max_spk=1, slices=slice_table(65, zeros=(30,))))
    return out


GLR_THRESHOLD = 900.0


def _planted(n, variant):
    """Twin pairs (E4), then a ladder of ten merges, then ties within a row and across rows (E1, E2), all far
    below the computed distances; duplicate pairs for the fresh ties behind them (E3, E5)."""
    hi = n - 1
    # twins: records (t, t + 1) and (t + 10, t + 11) are (A2, B2) and (A, B): A2 repeats A, B2 repeats B
    t1, t2 = 8, 30
    copies = [(t1, t1 + 10), (t1 + 1, t1 + 11), (t2, t2 + 10), (t2 + 1, t2 + 11)]
    dups = [(p, ln) for p, ln in DUPS[n] if p not in (5, 40, 41)]
    # (the twin sets differ in length, or their merged clusters would all score -penalty +- rounding)
    # record 5 spans A and B of set 1 and 140 frames either side: its distance to the merged A + B lies below
    # the one between the two merged duplicates, so the tie of row 5 -- the standing d(A', 5) at column 18 and the
    # fresh d(A2', 5) at column 8, which only the in-place rule can put first -- wins before those two merge
    s = _base('planted', n, variant, slices=slice_table(n, dups, copies=copies, lengths=[(t2 + 11, 66)],
                                                         covers=[(5, t1 + 10, t1 + 11, 140)]))
    pl = s['planted']
    pl += _apart(dups)
    # set 1: the higher pair first, so the second merged cluster sits at the LOWER column; set 2 the other way
    pl += [(t1 + 10, t1 + 11, _hex(-3.0e5)), (t1, t1 + 1, _hex(-2.9e5))]
    pl += [(t2, t2 + 1, _hex(-2.8e5)), (t2 + 10, t2 + 11, _hex(-2.7e5))]
    for k, t in enumerate((t1, t2)):
        # the four cells between the twins: the same distance in the other orientation, and the duplicates
        for j, (a, b) in enumerate(((t, t + 10), (t + 1, t + 11), (t, t + 11), (t + 1, t + 10))):
            pl.append((a, b, _hex(1.0e5 + 10.0 * (4 * k + j))))
    lad = [(50 + 2 * k, 51 + 2 * k) for k in range(5)] + [(24, 28), (25, 29), (2, 3), (44, 46), (45, 48)]
    if n == 65:
        lad = [(50, 51), (52, 53), (54, 55), (56, 57), (60, 61), (24, 28), (25, 29), (2, 3), (44, 46), (45, 49)]
    pl += _ladder(lad, -2.0e5, 1000.0)
    if n == 65:
        # (65 columns: two cells of one row 64 apart are columns 0 and 64; variant 2 takes (4, 0) in its lower
        # triangle, variant 1 by the mirror of (0, 4))
        pl += [(0, 4, _hex(-1.0e5)) if variant == 1 else (4, 0, _hex(-1.0e5)), (4, 64, _hex(-1.0e5))]
        pl += [(1, 7, _hex(-9.0e4)), (62, 64, _hex(-9.0e4)) if variant == 1 else (64, 62, _hex(-9.0e4))]
    else:
        pl += [(4, 6, _hex(-1.0e5)), (4, hi, _hex(-1.0e5))]               # E1; n = 257: column 256
        pl += [(1, 7, _hex(-9.0e4)), (n - 3, n - 2, _hex(-9.0e4))]        # E2
    return s


def _zeros(n, variant):
    """+0.0 and -0.0 as the smallest cells behind a short ladder, threshold 0: in one row >= 64 columns apart
    and in different rows, either sign first; two rows whose lower zero column dies in the ladder, so that the
    row is rescanned, beside rows whose entry is kept in place through every merge before it wins."""
    s = _base('zeros', n, variant, lambdac=0.0, slices=slice_table(n))
    pl = s['planted']
    pl += _ladder([(50, 51), (52, 53), (54, 90), (56, 91), (60, 61), (24, 28), (25, 29), (2, 3), (44, 46), (45, 48)],
                  -200.0, 10.0)
    pl += [(10, 12, '+0'), (10, 100, '-0'),          # one row, + first
           (11, 13, '-0'), (11, 110, '+0'),          # one row, - first
           (14, 15, '+0'), (70, 75, '-0'),           # two rows (other chunks), + first
           (16, 17, '-0'), (72, 77, '+0'),           # two rows, - first
           (18, 90, '+0'), (18, 120, '-0'),          # column 90 dies in the ladder: rescanned, then -0.0 alone
           (19, 91, '-0'), (19, 121, '+0')]
    return s


def _nans(n, variant):
    """Three all-zero records (NaN among themselves, +inf to the others), planted NaNs and one row that is NaN
    throughout but for one planted +inf; max_spk forces seven merges, and NaNs are left in the final matrix."""
    za, zb, zc = 30, 31, 60
    s = _base('nans', n, variant, threshold=BIG_NEG, max_spk=n - 7,
              slices=slice_table(n, DUPS[n][:1], zeros=(2, 3, za, zb, zc)))
    pl = s['planted']
    # two more all-zero records BELOW the pair: numbers planted over all their NaNs, row 3's minimum at column za.
    # The merge of (za, zb) writes both a fresh NaN at column za; row 3 is rescanned (its minimum sat there), row 2
    # has only the in-place rule, and numpy's next winner is (2, za)
    pl += [(2, 3, _hex(8.0e4)), (2, za, _hex(8.1e4)), (2, zb, _hex(8.2e4)), (2, zc, _hex(8.3e4)),
           (3, zb, _hex(8.4e4)), (3, zc, _hex(8.5e4)), (3, za, _hex(-1.0e6))]
    hi = n - 1
    pl += [(5, 20, 'nan'), (7, 20, 'nan'), (7, 22, 'nan'), (7, hi, 'nan'), (9, 12, 'nan')]
    # the standing NaNs of row zc at za, zb give way to numbers; its first NaN is planted at column 45
    # (and its minimum at column 50, away from the merge)
    pl += [(za, zc, _hex(7.0e4)), (zb, zc, _hex(7.1e4)), (45, zc, 'nan'), (50, zc, _hex(6.0e4))]
    pl += [(n - 5, n - 4, 'nan'), (n - 3, n - 2, 'nan')]
    row = 40
    for c in range(n):
        if c != row and (variant == 1 or c > row):
            pl.append((min(row, c), max(row, c), 'inf' if c == 50 else 'nan'))
    return s


def _fold(variant):
    """n = 577, more rows than k_ahc has threads (512): a thread meets a second row, and the fold over the waves
    sees wave 0 hold row 520 beside wave 1's row 70.  Half-overlapping slices (the session has 312 whole ones);
    lambda 0 and threshold 0, so the planted cells are the merges: a tie within row 71 whose second column lies
    in the scan's third trip, then a tie between rows 70 and 520."""
    n = 577
    s = _base('fold', n, variant, lambdac=0.0, slices=[(30 * i, 30 * i + SLICE) for i in range(n)])
    s['planted'] += [(71, 101, _hex(-60.0)), (71, 570, _hex(-60.0)), (70, 100, _hex(-50.0)), (520, 530, _hex(-50.0))]
    return s


def plant(M, K, s):
    """The scenario's cells into the matrix M (and the origin keys K, if given), mirrored for variant 1."""
    for r, c, vid in s['planted']:
        cells = [(r, c), (c, r)] if s['variant'] == 1 else [(r, c)]
        for i, j in cells:
            M[i, j] = value_of(vid)
            if K is not None:
                K[i, j] = key_of(vid)


# ---- the host side: C oracle distances, memoised on the clusters' merge trees (what fixes their bits)
class OracleDistances(object):
    def __init__(self, f):
        from oracle import c_engine
        self.eng = c_engine.COracleEngine(threads=1)
        self.eng.set_features(f)
        self.cd = pkg('change_detection')
        self.res = pkg('results')
        self.memo = {}

    def leaf_stats(self, rng):
        return self.eng.stats([[rng]])[0]

    def dist(self, kind, lambdac, ca, cs):
        key = (kind, lambdac, ca.tree, cs.tree)
        if key not in self.memo:
            out = np.zeros(8, dtype=np.float64)
            a, b = np.ascontiguousarray(ca.stats), np.ascontiguousarray(cs.stats)
            self.eng.lib.orc_pair_terms(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), int(kind == 'GLR'), 0,
                                        None, None, C.c_void_p(out.ctypes.data))
            t = self.res.PairTerms(int(out[0]), int(out[1]), float(out[2]), float(out[3]), float(out[4]),
                                   float(out[5]) if kind == 'GLR' else None, None)
            with np.errstate(all='ignore'):
                d = self.cd.bic_from_terms(t, lambdac) if kind == 'BIC' else self.cd.glr_from_terms(t)
            self.memo[key] = float(d)
        return self.memo[key]


def run_replay(s, orc):
    """The scenario through the replay: the initial matrix by the oracle, the planted cells, the loop."""
    from ahc_replay import Cluster, initial_keys, replay
    n, variant = s['n'], s['variant']
    clusters = [Cluster.leaf(r, orc.leaf_stats(tuple(r))) for r in s['slices']]
    M = np.full((n, n), np.inf) if variant == 2 else np.zeros((n, n))
    if variant == 1:
        np.fill_diagonal(M, float(9223372036854775807))
    for i in range(n):
        for j in range(i + 1, n):
            M[i, j] = orc.dist(s['kind'], s['lambdac'], clusters[i], clusters[j])
            if variant == 1:
                M[j, i] = M[i, j]
    K = initial_keys(clusters, variant)
    plant(M, K, s)
    return replay(clusters, M, K, variant, s['threshold'], s['max_spk'],
                  lambda ca, cs: orc.dist(s['kind'], s['lambdac'], ca, cs))


def _num(v):
    return None if v is None else ('nan' if math.isnan(v) else float(v).hex())


def to_fixture(s, res, sha):
    """What the fixture stores of one scenario (no matrices)."""
    gaps = [r['gap'] for r in res['rounds'] if r['gap'] is not None]
    thr = [r['thr_gap'] for r in res['rounds'] if r['thr_gap'] is not None]
    return {'name': s['name'], 'n': s['n'], 'variant': s['variant'], 'kind': s['kind'], 'lambdac': s['lambdac'],
            'threshold': _num(s['threshold']), 'max_spk': s['max_spk'], 'session': list(SESSION),
            'zero_frames': ZERO_FRAMES, 'frames_sha256': sha, 'slices': [list(r) for r in s['slices']],
            'planted': [list(p) for p in s['planted']],
            'merges': [[a, b, _num(d), kind] for a, b, d, kind in res['merges']],
            'max_dist': _num(res['max_dist']), 'min_dist': _num(res['min_dist']),
            'max_kind': res['max_kind'], 'min_kind': res['min_kind'],
            'rounds': [[_num(r['gap']), _num(r['thr_gap']), int(r['nan'])] for r in res['rounds']],
            'smallest_gap': _num(min(gaps)) if gaps else None,
            'smallest_threshold_gap': _num(min(thr)) if thr else None,
            'degenerate': bool(res['degenerate']),
            'events': dict(sorted(res['events'].items())),
            'where': {k: list(v) for k, v in sorted(res['where'].items())}}
