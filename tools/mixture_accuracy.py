#!/usr/bin/env python3
"""Per-group errors of the mixture kernels against the 50-digit reference on the cases of
tests/mixture_cases.py (tests/golden/mixture_exact.json and .npz): per case and output group (ln w, mean,
1 / var, log_norm, L, scores, n_c, f_c) the reference's scale, e -- the float64 restatements'
largest error (tests/reseg_gmm_numpy.py, tests/link_clr_numpy.py; stored in the fixture) --, the
device's largest error, the quotient device error / max(e, 2^-52 scale) and the tier.

    python tools/mixture_accuracy.py --out profiles/mixture_accuracy.json
    python tools/mixture_accuracy.py --no-device          # the fixture's columns alone

The rows are the ones tests/test_mixture_exact.py asserts on (quotient <= 64, the tier's bar);
`quotient` and `quotient_by_group` are the largest, `offset` the relative errors of the speakers
whose cluster means are 1, 8 and 64 sigma from the origin, the figures behind the accuracy domain
in DESIGN.md, include/spkd.h and INTEGRATION.md.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import mixture_cases as mc                      # noqa: E402


def fixture_rows(fx):
    rows = []
    for name, job in sorted(fx['jobs'].items()):
        for spk, e in sorted(job.items()):
            for g, v in sorted(e.get('groups', {}).items()):
                rows.append({'case': '%s/%s' % (name, spk), 'group': g, 'tier': v['tier'], 'scale': v['vmax'], 'e': v['e']})
    rows.append(dict(case='scores', group='scores', tier=fx['scores']['groups']['scores']['tier'],
                     scale=fx['scores']['groups']['scores']['vmax'], e=fx['scores']['groups']['scores']['e']))
    for spk in mc.UBM_SPEAKERS:
        for g, v in sorted(fx['ubm'][spk]['groups'].items()):
            rows.append({'case': 'ubm/' + spk, 'group': g, 'tier': v['tier'], 'scale': v['vmax'], 'e': v['e']})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--no-device', action='store_true')
    ap.add_argument('--out')
    args = ap.parse_args()
    fx = mc.fixture()
    t0 = time.time()
    out = {'source': {'cpu': 'case, group, tier, scale and e: tests/golden/mixture_exact.json', 'env': fx['env'],
                      'device': None if args.no_device else 'one MI355X, the library as built from this tree: dev, dev_rel, quotient'},
           'measure': 'e, dev: largest |a - b| of the group; dev_rel and the tiers: |a - b| / max(1, |a|, |b|); '
                      'quotient: dev / max(e, 2^-52 scale)'}
    if args.no_device:
        out['rows'] = fixture_rows(fx)
    else:
        from reseg_helpers import Dev
        dev = Dev(mc.build()[0])
        try:
            rows = []
            for job in mc.jobs():
                rows += mc.check_job(dev, fx, job)[0]
            rows += mc.check_scores(dev, fx) + mc.check_ubm(dev, fx)
        finally:
            dev.close()
        by_group = {}
        for r in rows:
            if r['quotient'] > by_group.get(r['group'], {'quotient': -1.0})['quotient']:
                by_group[r['group']] = {'quotient': r['quotient'], 'case': r['case']}
        top = max(rows, key=lambda r: r['quotient'])
        out.update(rows=rows, margin=mc.MARGIN, quotient={'quotient': top['quotient'], 'case': top['case'], 'group': top['group']},
                   quotient_by_group=by_group,
                   missed=[r for r in rows if r['quotient'] > mc.MARGIN or (r['tier'] != 'outside' and r['dev_rel'] > float(r['tier']))])
        off = {}
        for r in rows:
            spk = r['case'].split('/')[-1]
            if spk.startswith('off') and r['group'] != 'L':
                off.setdefault(spk, {}).setdefault(r['group'], 0.0)
                off[spk][r['group']] = max(off[spk][r['group']], r['dev_rel'])
        out['offset'] = off
    out['seconds'] = round(time.time() - t0, 1)
    # one row a line, figures to four digits: `columns` names a row's entries
    columns = [c for c in ('case', 'group', 'tier', 'scale', 'e', 'dev', 'dev_rel', 'quotient', 'ulp32') if any(c in r for r in out['rows'])]
    rows = [[(float('%.4g' % r[c]) if isinstance(r.get(c), float) else r.get(c)) for c in columns] for r in out.pop('rows')]
    head = json.dumps(dict(out, columns=columns), indent=1, sort_keys=True)
    text = head[:-2] + ',\n "rows": [\n' + ',\n'.join('  ' + json.dumps(r) for r in rows) + '\n ]\n}'
    json.loads(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps({k: out.get(k) for k in ('quotient', 'quotient_by_group', 'offset', 'missed', 'seconds')}))


if __name__ == '__main__':
    main()
