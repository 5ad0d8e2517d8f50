#!/usr/bin/env python3
"""Exact goldens on frames unlike the generator's (tests/conditioned_cases.py): log-dets, BIC,
GLR and KL2 from exact integer moments and fraction-free determinants (tests/exact_moments.py),
the exact greedy merge orders, the growing window's candidate geometry, and the accuracy tier of
every group as the C oracle (the device's formulation, raw moments) reaches it on the CPU.

Writes tests/golden/conditioned_exact.json.  Needs oracle/libspkd_oracle.so (make -C oracle).

    python tests/golden/make_golden_conditioned.py

Conditions enforced here (a case that misses one is replaced by giving its buffer another
stream in conditioned_cases.REPLACED, never by loosening the condition):
  * every exact covariance is full rank;
  * every growing-window candidate is at least 1e-3 relative away from the decision threshold;
  * at every exact merge step the minimum is more than 1e-6 relative below the runner-up;
  * the reference's arithmetic (oracle.numpy_engine) is within 1e-5 of exact on every pair: BIC and
    GLR at every offset, KL2 at offset 0 (elsewhere its float32 np.mean governs KL2).
"""
import json
import math
import multiprocessing
import os
import sys

import mpmath
import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conditioned_cases as cc      # noqa: E402
import exact_moments as em          # noqa: E402
from oracle.c_engine import COracleEngine       # noqa: E402
from oracle.numpy_engine import NumpyEngine     # noqa: E402

MOMENT_SETS = (('corr9', 64, ((100, 1124), (2000, 2001))),)          # one chunk and one frame, two ranges


def exact_cond(ef):
    """cond of the exact sample covariance of the whole buffer (rounded to double once)."""
    mom = ef.moments([(0, ef.shape[0])])
    a = mom.scatter()
    with mpmath.workprec(em.MP_BITS):
        sc = mpmath.mpf(mom.n * (mom.n - 1)) * mpmath.mpf(4) ** mom.k
        cov = np.array([[float(mpmath.mpf(v) / sc) for v in row] for row in a])
    w = np.linalg.eigvalsh(cov)
    return float(w[-1] / w[0])


def finite(pair):
    return math.isfinite(float.fromhex(pair[0]))


def one_buffer(arg):
    cls, m = arg
    geometry = cc.gw_geometry()
    f = cc.make_buffer(cls, m)
    ef = em.ExactFrames(f)
    ce, ne = COracleEngine(1), NumpyEngine()
    ce.set_features(f)
    ne.set_features(f)
    entry = {'sha256': cc.synth.fea_sha256(f), 'cond': exact_cond(ef), 'pairs': {}}
    for size in cc.SIZES:
        p = cc.exact_pair(ef, size, want_kl2=(m == 0))
        assert all(finite(v) for v in p['ld']), ('rank-deficient', cls, m, size)
        entry['pairs'][cc.size_key(size)] = p
    c_err, n_err = cc.pairs_errors(ce, entry), cc.pairs_errors(ne, entry)
    for size in cc.SIZES:
        k = cc.size_key(size)
        p = entry['pairs'][k]
        p['tier'] = cc.tier_of(cc.worst_of(c_err[k]))
        if m == 0:
            p['tier_kl2'] = cc.tier_of(c_err[k]['kl2'])
        assert max(n_err[k]['bic'], n_err[k]['glr']) <= 1.0e-5, ('reference misses 1e-5', cls, m, size, n_err[k])
        if m == 0:
            assert n_err[k]['kl2'] <= 1.0e-5, ('reference misses 1e-5 (KL2)', cls, m, size, n_err[k])
    entry['gauss'] = cc.gauss_scores_exact(ef, cls, m)
    entry['gauss']['tier'] = cc.tier_of(cc.gauss_reference_scores_error(ce, f, cls, m, entry))
    if m == cc.PROBLEM_OFFSETS[-1]:
        entry['sw'] = cc.sw_exact(ef)
        entry['sw']['tier'] = cc.tier_of(cc.sw_errors(ce, entry['sw']))
    if m in cc.PROBLEM_OFFSETS:
        mx = cc.exact_matrix(ef)
        assert all(finite(v) for v in mx['ld'])
        entry['matrix'] = mx
        mx['tier'] = cc.tier_of(cc.matrix_errors_from_terms(ce, entry))
        entry['merge'] = {}
        worst = 0.0
        for kind in ('BIC', 'GLR'):
            mg = cc.exact_merge(ef, kind)
            assert mg['gap'] > cc.MERGE_MIN_GAP, ('merge step too close to call', cls, m, kind, mg['gap'])
            entry['merge'][kind] = mg
            same, err = cc.merge_errors(ce, entry, kind)
            worst = max(worst, err if same else float('inf'))
        entry['merge']['tier'] = cc.tier_of(worst)
        # growing window: the reference's own candidate list is the geometry; its distances
        # choose the samples and show the distance to the threshold
        worst = 0.0
        dists = {}
        for kind in ('BIC', 'GLR'):
            cands = cc.gw_candidates(ne, kind)
            assert [list(c[:4]) for c in cands] == geometry, ('candidate list is not geometry alone', cls, m, kind)
            for c in cands:
                assert abs(c[4] - cc.GW_THRESHOLD) / max(1.0, abs(c[4]), cc.GW_THRESHOLD) >= 1.0e-3
            dists[kind] = [c[4] for c in cands]
        idx = cc.gw_sample_indices(dists['BIC'], dists['GLR'])
        assert len(idx) <= cc.GW_SAMPLES
        entry['gw'] = {'samples': cc.exact_gw(ef, geometry, idx)}
        for kind in ('BIC', 'GLR'):
            same, err = cc.gw_errors(ce, entry, kind, geometry)
            worst = max(worst, err if same else float('inf'))
        entry['gw']['tier'] = cc.tier_of(worst)
    return cc.group_name(cls, m), entry


def moment_sets():
    out = []
    for cls, m, ranges in MOMENT_SETS:
        ef = em.ExactFrames(cc.make_buffer(cls, m))
        mom = ef.moments(list(ranges))
        d = cc.DIM
        out.append({'buffer': cc.group_name(cls, m), 'ranges': [list(r) for r in ranges], 'n': mom.n, 'k': mom.k,
                    'note': 'sums of frames * 2^k (s) and of their products (m: upper triangle, row-major)',
                    's': [str(v) for v in mom.s],
                    'm': [str(mom.m[i][j]) for i in range(d) for j in range(i, d)]})
    return out


def main():
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        done = pool.map(one_buffer, list(cc.all_buffers()), chunksize=1)
    out = {'env': {'python': sys.version.split()[0], 'numpy': np.__version__, 'scipy': scipy.__version__,
                   'mpmath': mpmath.__version__,
                   'note': 'exact values: tests/exact_moments.py; tiers: oracle/spkd_oracle.c on the CPU; '
                           'generated by tests/golden/make_golden_conditioned.py'},
           'lambda': cc.LAMBDA, 'seed': cc.SEED,
           'gw': {'turn': list(cc.GW_TURN), 'params': cc.GW_PARAMS, 'threshold': cc.GW_THRESHOLD,
                  'n_candidates': len(cc.gw_geometry())},
           'buffers': dict(done), 'moments': moment_sets()}
    for cls in ('corr3', 'corr6', 'corr9'):
        want = {'corr3': 1e3, 'corr6': 1e6, 'corr9': 1e9}[cls]
        cond = out['buffers'][cc.group_name(cls, 0)]['cond']
        assert want / 10 <= cond <= want * 10, (cls, cond)
    with open(os.path.join(HERE, 'conditioned_exact.json'), 'w') as f:
        json.dump(out, f, indent=None, separators=(',', ':'), sort_keys=True)
        f.write('\n')
    tiers = {}
    for name, e in sorted(out['buffers'].items()):
        tiers[name] = [e['pairs'][cc.size_key(s)]['tier'] for s in cc.SIZES] + \
                      [e[k]['tier'] for k in ('matrix', 'merge', 'gw', 'sw', 'gauss') if k in e]
        print(name, 'cond %.3g' % e['cond'], tiers[name])


if __name__ == '__main__':
    main()
