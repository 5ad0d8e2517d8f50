#!/usr/bin/env python3
"""Per-group errors of the CLR chain and the gallery against exact arithmetic on the groups of
tests/clr_cases.py (tests/golden/clr_exact.json): per group its K, the offset of the UBM's means in
sigma, the relevance, the scale of its values, e -- the float64 restatements' largest error
(tests/link_clr_numpy.py, tests/gallery_numpy.py; stored in the fixture) --, the device's largest
error over k_ident_scores, k_clr_matrix and k_clr_chain, the quotient device error / max(e, 2^-52
scale) and the tier.

    python tools/clr_accuracy.py --out profiles/clr_accuracy.json
    python tools/clr_accuracy.py --no-device          # the fixture's columns alone

The rows are the ones tests/test_clr_exact.py asserts on (quotient <= 64, the tier's bar); `offset`
gives the digits an offset of the UBM's means costs (-log10 of 2^-52 over the error), the figures
behind the accuracy domain in DESIGN.md, include/spkd.h and INTEGRATION.md.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import clr_cases as cc                          # noqa: E402


def digits_lost(err, scale):
    """How many of float64's digits an error costs at this scale."""
    return 0.0 if err <= cc.EPS * scale else round(math.log10(err / (cc.EPS * scale)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--no-device', action='store_true')
    ap.add_argument('--out')
    args = ap.parse_args()
    fx = cc.fixture()
    t0 = time.time()
    dev = None
    if not args.no_device:
        import numpy as np
        from reseg_helpers import Dev
        dev = Dev(np.zeros((64, 39), dtype=np.float32))
    groups = {}
    try:
        for g in cc.GROUPS:
            e = fx['groups'][g['name']]
            if not e['finite']:
                continue
            row = {'K': g['K'], 'n': g['n'], 'offset_sigma': g.get('offset', 0.0), 'relevance': g.get('r', 16.0),
                   'tier': e['tier'], 'scale': e['vmax'], 'e': e['e'], 'e_digits_lost': digits_lost(e['e'], e['vmax'])}
            if dev is not None:
                rows = cc.check_group(dev, g['name'])
                worst = max(rows, key=lambda q: q['quotient'])
                row.update(dev=max(q['dev'] for q in rows), dev_rel=max(q['dev_rel'] for q in rows), quotient=worst['quotient'],
                           quotient_at=worst['what'], by_kernel={q['what']: float('%.4g' % q['dev']) for q in rows})
                row['dev_digits_lost'] = digits_lost(row['dev'], e['vmax'])
            groups[g['name']] = {k: (float('%.4g' % v) if isinstance(v, float) else v) for k, v in row.items()}
    finally:
        if dev is not None:
            dev.close()
    out = {'source': {'cpu': 'K, n, offset, relevance, tier, scale and e: tests/clr_cases.py and tests/golden/clr_exact.json',
                      'env': fx['env'],
                      'device': None if dev is None else 'one MI355X, the library as built from this tree: dev, dev_rel, quotient'},
           'measure': 'e, dev: largest |a - b| of the group against the exact value rounded once; dev_rel and the tiers: '
                      '|a - b| / max(1, |a|, |b|); quotient: dev / max(e, 2^-52 scale); digits lost: log10(error / (2^-52 scale))',
           'margin': cc.MARGIN, 'groups': groups, 'seconds': round(time.time() - t0, 1)}
    out['offset'] = {k: {c: groups[k].get(c) for c in ('offset_sigma', 'e', 'e_digits_lost', 'dev', 'dev_digits_lost')}
                     for k in ('k8', 'off8', 'off64', 'off1024')}
    if dev is not None:
        top = max(groups, key=lambda k: groups[k]['quotient'])
        out['quotient'] = {'quotient': groups[top]['quotient'], 'group': top, 'at': groups[top]['quotient_at']}
        out['missed'] = [k for k, v in groups.items() if v['quotient'] > cc.MARGIN or v['dev_rel'] > float(v['tier'])]
    text = json.dumps(out, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps({k: out.get(k) for k in ('quotient', 'offset', 'missed', 'seconds')}))


if __name__ == '__main__':
    main()
