"""CPU restatement (numpy, float64) of the speaker gallery -- TEST INFRASTRUCTURE ONLY.

PARITY: no reference counterpart.  The reference keeps nothing from one run to the next
(spk-clustering.py:289 is a TODO for more than one wav); what spkd_clr_identify and spkd_bw_accumulate
compute (include/spkd.h, section 11) and what pipeline.link_batch does with a gallery is stated here.
The score of two records is link_clr_numpy.clr.

  scores    mat[s][g] = clr(probe s, identity g) where both are ok, NaN elsewhere.
  assign    per group of probes, exclusive: among the undecided ok rows and the ok columns not yet taken
            in this group the pair of the highest score, the first in row-major order on a tie; assigned
            while the score is above the threshold, else the rows left over are unknown (-1).  Not
            exclusive: every ok row its own arg-max (the lowest column on a tie) when above the threshold.
  score     the assigned pair's; of an unknown row its highest over the ok columns.
  second    the row's highest over the ok columns other than the reported one (of an unknown row: other
            than the first that reaches `score`); NaN when there is none.
  sum       dst[slot] = (keep ? dst[slot] : 0) + src[m_0] + src[m_1] + ... in that order.
"""
import numpy as np

import link_clr_numpy as L

GALLERY_MAX_N = 16384   # SPKD_GALLERY_MAX_N
MAX_N = L.MAX_N         # SPKD_CLR_MAX_N: probes of one call


def scores(probes, probe_ok, gallery, gallery_ok, ubm, r):
    """(mat [S, G], finite): finite False when a score between an ok probe and an ok identity is not."""
    mat = np.full((len(probes), len(gallery)), np.nan)
    fin = True
    for s in range(len(probes)):
        for g in range(len(gallery)):
            if probe_ok[s] and gallery_ok[g]:
                mat[s, g] = L.clr(probes[s], gallery[g], ubm, r)
                fin = fin and bool(np.isfinite(mat[s, g]))
    return mat, fin


def _best(row, cols):
    """(value, column) of the highest of row over cols (ascending), the lowest column on a tie."""
    v, j = None, -1
    for c in cols:
        if j < 0 or row[c] > v:
            v, j = row[c], c
    return v, j


def assign(mat, probe_ok, gallery_ok, group_off, threshold, exclusive=True):
    """(ident, score, second) of every probe; see the module's text."""
    S = mat.shape[0]
    cols = [g for g in range(mat.shape[1]) if gallery_ok[g]]
    ident = np.full(S, -1, dtype=np.int32)
    for a, b in zip(group_off[:-1], group_off[1:]):
        rows = [s for s in range(int(a), int(b)) if probe_ok[s]]
        if not exclusive:
            for s in rows:
                v, j = _best(mat[s], cols)
                if j >= 0 and v > threshold:
                    ident[s] = j
            continue
        free = list(cols)
        while rows and free:
            cand = [(s,) + _best(mat[s], free) for s in rows]
            s, v, j = cand[0]
            for t in cand[1:]:
                if t[1] > v:
                    s, v, j = t
            if not v > threshold:
                break
            ident[s] = j
            rows.remove(s)
            free.remove(j)
    score, second = np.full(S, np.nan), np.full(S, np.nan)
    for s in range(S):
        if not probe_ok[s] or not cols:
            continue
        j = int(ident[s]) if ident[s] >= 0 else _best(mat[s], cols)[1]
        score[s] = mat[s, j]
        rest = [c for c in cols if c != j]
        if rest:
            second[s] = _best(mat[s], rest)[0]
    return ident, score, second


def identify(probes, probe_ok, group_off, gallery, gallery_ok, ubm, r, threshold, exclusive=True):
    """spkd_clr_identify -> (ident, score, second, mat, finite); every ident -1 when not finite."""
    mat, fin = scores(probes, probe_ok, gallery, gallery_ok, ubm, r)
    if not fin:
        S = len(probes)
        return np.full(S, -1, dtype=np.int32), np.full(S, np.nan), np.full(S, np.nan), mat, False
    return assign(mat, probe_ok, gallery_ok, group_off, threshold, exclusive) + (mat, True)


def margins(mat, probe_ok, gallery_ok, group_off, threshold, exclusive=True):
    """How far the decisions of assign are from going another way: (the least |score - threshold| over
    the scores a decision compared with the threshold, the least lead of a chosen pair over the best
    other pair it competed with -- one that shares its row or its column).  inf where there is none."""
    cols = [g for g in range(mat.shape[1]) if gallery_ok[g]]
    to_th, to_next = np.inf, np.inf
    for a, b in zip(group_off[:-1], group_off[1:]):
        rows = [s for s in range(int(a), int(b)) if probe_ok[s]]
        free = list(cols)
        if not exclusive:
            for s in rows:
                vals = sorted((mat[s, c] for c in cols), reverse=True)
                if vals:
                    to_th = min(to_th, abs(vals[0] - threshold))
                if len(vals) > 1:
                    to_next = min(to_next, vals[0] - vals[1])
            continue
        while rows and free:
            v, s, j = max((mat[s, c], -s, -c) for s in rows for c in free)
            s, j = -s, -j
            to_th = min(to_th, abs(v - threshold))
            if not v > threshold:
                break
            rivals = [mat[x, c] for x in rows for c in free if (x == s) != (c == j)]
            if rivals:
                to_next = min(to_next, v - max(rivals))
            rows.remove(s)
            free.remove(j)
    return to_th, to_next


def bw_accumulate(src, set_off, member, slots, keep, dst):
    """spkd_bw_accumulate: dst with the sets added, in member order."""
    out = np.array(dst, dtype=np.float64)
    for k, slot in enumerate(slots):
        acc = out[slot].copy() if keep[k] else np.zeros_like(out[slot])
        for m in member[int(set_off[k]):int(set_off[k + 1])]:
            acc = acc + src[m]
        out[slot] = acc
    return out


class Gallery(object):
    """gallery.Gallery on the host: the model, the records, ok and the names."""

    def __init__(self, link):
        self.link = link
        self.ubm = None
        self.records = np.zeros((0, link['components'], L.BW_COMP))
        self.ok = np.zeros(0, dtype=np.int32)
        self.names = []

    @property
    def n(self):
        return len(self.records)

    def identify(self, probes, ok, group_off, exclusive=True, threshold=None):
        th = self.link['threshold'] if threshold is None else threshold
        got = identify(probes, ok, group_off, self.records, self.ok, self.ubm, self.link['relevance'], th, exclusive)
        if not got[4]:
            raise ValueError('array must not contain infs or NaNs')
        return got[:4]

    def update(self, probes, ok, ident):
        out = np.where(np.asarray(ok) != 0, ident, -1).astype(np.int32)
        recs = [r for r in self.records]
        for s in range(len(probes)):
            if ok[s] and ident[s] >= 0:
                recs[ident[s]] = recs[ident[s]] + probes[s]
            elif ok[s]:
                out[s] = len(recs)
                recs.append(np.zeros_like(probes[s]) + probes[s])
                self.names.append('spk_%d' % len(recs))
        self.records = np.array(recs).reshape(-1, self.link['components'], L.BW_COMP)
        self.ok = np.concatenate([self.ok, np.ones(len(recs) - len(self.ok), dtype=np.int32)])
        return out


def link(feats, speakers, link, gallery, enrol=True, exclusive=True):
    """pipeline.link_batch with link = dict(LINK_CLR, gallery=...) on speakers given as range lists.
    Returns dict(labels: the global label of each speaker, merges, identity / score / second per batch
    cluster, enrolled, mat: the clusters' scores against the gallery as it was, cluster_ok)."""
    n = len(speakers)
    if gallery.ubm is None:
        ubm, ubm_ok = L.train_ubm(feats, speakers, link)
        if not ubm_ok:
            return dict(labels=np.arange(1, n + 1, dtype=np.int32), merges=[])
        gallery.ubm = ubm
    got = [L.ubm_stats(L.frames_of(feats, rs), gallery.ubm) for rs in speakers]
    recs, ok = np.array([g[0] for g in got]), np.array([g[1] for g in got], dtype=np.int32)
    merges, _, _, fin = L.clr_link(recs, ok, gallery.ubm, link['relevance'], link['threshold'], link['max_spk'])
    if not fin:
        raise ValueError('array must not contain infs or NaNs')
    glob = L.labels_from_merges(n, merges)
    n_cl = int(glob.max())
    member = np.argsort(glob, kind='stable')
    set_off = np.concatenate([[0], np.cumsum(np.bincount(glob - 1, minlength=n_cl))])
    cl = bw_accumulate(recs, set_off, member, np.arange(n_cl), np.zeros(n_cl), np.zeros((n_cl,) + recs.shape[1:]))
    cl_ok = np.array([ok[member[a:b]].min() for a, b in zip(set_off[:-1], set_off[1:])], dtype=np.int32)
    ident, score, second, mat = gallery.identify(cl, cl_ok, [0, n_cl], exclusive)
    before = gallery.n
    unknown = np.nonzero((cl_ok != 0) & (ident < 0))[0]
    label = ident.astype(np.int64) + 1
    label[unknown] = before + 1 + np.arange(len(unknown))
    bad = np.nonzero(cl_ok == 0)[0]
    label[bad] = before + len(unknown) + 1 + np.arange(len(bad))
    enrolled = []
    if enrol:
        ident = gallery.update(cl, cl_ok, ident)
        enrolled = ident[unknown].tolist()
    return dict(labels=label[glob - 1].astype(np.int32), merges=merges, identity=ident, score=score, second=second,
                enrolled=enrolled, mat=mat, cluster_ok=cl_ok)
