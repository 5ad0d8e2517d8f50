"""The merge loop of spk_cluster_hi (spk-clustering.py:178-240, spk-clustering2.py:173-222) started
from speakers of SEVERAL segments each -- what linking the speakers of a batch's files is.
oracle.numpy_engine.NumpyEngine.cluster_hi restates the same loop from one segment per speaker;
this one reuses its frame gathering and its distances (np.cov / det on raw frames) unchanged.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle.numpy_engine import MAXINT


def link_hi(engine, speakers, variant, kind, lambdac, threshold, max_spk):
    """engine: a NumpyEngine with the concatenated features set.  speakers: per speaker the list
    of its (begin, end) frame ranges.  Returns (merges [(a, b, d)], partition: per final speaker
    the sorted indices of the initial speakers in it, in the final order)."""
    speakers = [list(s) for s in speakers]
    groups = [[i] for i in range(len(speakers))]
    sp = len(speakers)
    feats = lambda k: engine._gather(speakers[k])
    dm = np.zeros((sp, sp)) if variant == 1 else np.full((sp, sp), np.inf)
    if variant == 1:
        np.fill_diagonal(dm, MAXINT)
    for s1 in range(sp):
        for s2 in range(s1 + 1, sp):
            dm[s1, s2] = engine._dist(kind, lambdac, feats(s1), feats(s2))
            if variant == 1:
                dm[s2, s1] = dm[s1, s2]
    merges = []
    with np.errstate(all='ignore'):
        while True:
            mind = float(dm.min())
            if not (mind <= threshold or (max_spk > 0 and len(speakers) > max_spk)):
                break
            index = int(dm.argmin())
            a, b = sorted((index // len(speakers), index % len(speakers)))
            merges.append((a, b, mind))
            speakers[a].extend(speakers.pop(b))
            groups[a].extend(groups.pop(b))
            dm = np.delete(np.delete(dm, b, axis=0), b, axis=1)
            for s2 in range(len(speakers)):
                if s2 != a:
                    dm[a, s2] = engine._dist(kind, lambdac, feats(a), feats(s2))
                    if variant == 1:
                        dm[s2, a] = dm[a, s2]
    return merges, [sorted(g) for g in groups]
