#!/usr/bin/env python3
"""Per-group errors against exact arithmetic on the conditioned cases (tests/conditioned_cases.py,
tests/golden/conditioned_exact.json): device, C oracle (the device's formulation on the CPU) and
the reference's arithmetic (oracle.numpy_engine), in the project's measure |a - b| / max(1, |a|, |b|).

    python tools/conditioned_accuracy.py --out profiles/conditioned_accuracy.json
    python tools/conditioned_accuracy.py --no-device          # the two CPU columns alone

The rows are the ones tests/test_conditioned_exact.py asserts on; `ratio` is the largest
device / C-oracle quotient over the rows whose device error is above the floor, the figure the
test's K is derived from (K = that times 4, rounded up to a power of two).

`scatter` (CPU) says how far the formulation itself scatters on the pair group with the largest
quotient: the BIC error of the same fp64 raw-moment covariances (from the C oracle's records)
eliminated without pivoting in 40 orders of the dimensions, and by LAPACK's pivoted LU, beside
the condition numbers of the three sample covariances.
"""
import argparse
import importlib
import json
import os
import sys
import math
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import conditioned_cases as cc                  # noqa: E402
from oracle.c_engine import COracleEngine       # noqa: E402
from oracle.numpy_engine import NumpyEngine     # noqa: E402


def elimination_scatter(ce, group):
    """See the module docstring; group = 'class/offset/n1xn2'."""
    cls, m, key = group.split('/')
    size = tuple(int(v) for v in key.split('x'))
    ce.set_features(cc.buffer(cls, int(m)))
    ra, rb = cc.pair_ranges(size)
    iu = np.triu_indices(cc.DIM + 1)
    covs = []
    for rec in ce.stats([[ra], [rb], [ra, rb]]):
        mm = np.zeros((cc.DIM + 1, cc.DIM + 1))
        mm[iu] = rec
        mm = mm + np.triu(mm, 1).T
        n, s = mm[cc.DIM, cc.DIM], mm[:cc.DIM, cc.DIM]
        covs.append((mm[:cc.DIM, :cc.DIM] - np.outer(s, s) / n) / (n - 1))

    def logdet(c, perm):
        a = c[np.ix_(perm, perm)].copy()
        t = 0.0
        for j in range(cc.DIM):
            t += math.log(a[j, j])
            a[j + 1:, j + 1:] -= np.outer(a[j + 1:, j], a[j + 1:, j]) / a[j, j]
        return t

    def bic(lds):
        n1, n2 = size
        n = n1 + n2
        return (0.5 * n * lds[2] - 0.5 * n1 * lds[0] - 0.5 * n2 * lds[1]
                - cc.LAMBDA * 0.5 * (cc.DIM + 0.5 * cc.DIM * (cc.DIM + 1)) * math.log(n))

    want = float.fromhex(cc.fixture()['buffers']['%s/%s' % (cls, m)]['pairs'][key]['bic'])
    rng = np.random.RandomState(1)
    perms = [np.arange(cc.DIM), np.arange(cc.DIM)[::-1]] + [rng.permutation(cc.DIM) for _ in range(38)]
    errs = sorted(cc._rel(bic([logdet(c, p) for c in covs]), want) for p in perms)
    return {'group': group, 'cond_of_sample_covariances': [float(np.linalg.cond(c)) for c in covs],
            'bic_error_40_orders_no_pivoting': {'min': errs[0], 'median': errs[len(errs) // 2], 'max': errs[-1]},
            'bic_error_pivoted_lu': cc._rel(bic([float(np.linalg.slogdet(c)[1]) for c in covs]), want)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--no-device', action='store_true')
    ap.add_argument('--out')
    args = ap.parse_args()
    fx = cc.fixture()
    ce, ne = COracleEngine(1), NumpyEngine()
    eng = eng_pinv = None
    if not args.no_device:
        engine = importlib.import_module('speaker-diarization_amd.engine')
        eng, eng_pinv = engine.HipEngine(0), engine.HipEngine(0, kl2_pinv=True)
    rows, pairs, records = [], {}, {'worst_ratio_to_bound': 0.0, 'counts_exact': True, 'sets': 0}
    t0 = time.time()
    for (cls, m) in cc.all_buffers():
        f = cc.buffer(cls, m)
        e = fx['buffers'][cc.group_name(cls, m)]
        ce.set_features(f)
        ne.set_features(f)
        c_err, n_err = cc.pairs_errors(ce, e), cc.pairs_errors(ne, e)
        for size in cc.SIZES:
            k = cc.size_key(size)
            pairs[cc.group_name(cls, m, size)] = {
                'tier': e['pairs'][k]['tier'], 'c_oracle': cc.worst_of(c_err[k]), 'reference': cc.worst_of(n_err[k]),
                'c_oracle_kl2': c_err[k].get('kl2'), 'reference_kl2': n_err[k].get('kl2'), 'device': None}
        if eng is None:
            continue
        eng.set_features(f)
        eng_pinv.set_features(f)
        new = cc.check_pairs(cls, m, ce, eng, eng_pinv) + cc.check_gauss(cls, m, ce, eng)
        if m in cc.PROBLEM_OFFSETS:
            new += cc.check_matrix(cls, m, ce, eng) + cc.check_gw(cls, m, ce, eng) + cc.check_merge(cls, m, ce, eng)
        for r in new:
            if r['what'] == 'pair_terms':
                pairs[r['group']]['device'] = r['dev']
            elif r['what'] == 'pair_terms KL2':
                pairs[r['group']]['device_kl2'] = r['dev']
        rows += new
        sets = cc.record_sets()
        got = eng.stats(sets)
        for k, s in enumerate(sets):
            exact_n, w = cc.record_check(got[k], cc.exact_frames(cls, m), f, s)
            records['counts_exact'] = records['counts_exact'] and exact_n
            records['worst_ratio_to_bound'] = max(records['worst_ratio_to_bound'], w)
            records['sets'] += 1
    out = {'source': {'device': None if eng is None else 'one MI355X, the library as built from this tree: `device` '
                                                            'columns and every row\'s `dev`',
                      'cpu': 'c_oracle (oracle/spkd_oracle.c) and reference (oracle/numpy_engine.py) columns, every '
                             'row\'s `c`; exact values from tests/golden/conditioned_exact.json',
                      'env': fx['env']},
           'measure': '|a - b| / max(1, |a|, |b|), worst over log-dets, BIC and GLR of the group',
           'pairs': pairs, 'seconds': round(time.time() - t0, 1)}
    if eng is not None:
        ratios = [(cc.ratio_of(r), r) for r in rows]
        ratios = [(q, r) for q, r in ratios if q is not None]
        by_what = {}
        for q, r in ratios:
            key = r['what'].split(' ')[0]
            if q > by_what.get(key, (0.0, None))[0]:
                by_what[key] = (q, r['group'])
        out['rows'] = rows
        out['records'] = records
        out['floor'] = cc.FLOOR
        out['ratio'] = max([q for q, _ in ratios], default=0.0)
        out['ratio_by_entry_point'] = {k: {'ratio': v[0], 'group': v[1]} for k, v in sorted(by_what.items())}
        out['not_same'] = [r for r in rows if r.get('same') is False or r.get('ok') is False]
        top = max((t for t in ratios if t[1]['what'] == 'pair_terms'), key=lambda t: t[0], default=None)
        if top is not None:
            out['scatter'] = elimination_scatter(ce, top[1]['group'])
        eng.close()
        eng_pinv.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    summary = {k: out.get(k) for k in ('ratio', 'ratio_by_entry_point', 'records', 'seconds', 'not_same', 'scatter')}
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
