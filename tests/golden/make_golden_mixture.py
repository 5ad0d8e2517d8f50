#!/usr/bin/env python3
"""The mixture kernels' reference on frames unlike the generator's (tests/mixture_cases.py): models,
log-likelihoods, scores and UBM records at 50 digits with centred variances (tests/exact_mixture.py),
the hand-written start models bit for bit, and per output group the error e of the float64
restatements (tests/reseg_gmm_numpy.py, tests/link_clr_numpy.py) against that reference and the tier
it puts the group in.

Writes tests/golden/mixture_exact.json (ok, L, G_k, e, tiers, the hand-written models) and
tests/golden/mixture_exact.npz (the models, scores and records: the reference rounded once to float64).

    python tests/golden/make_golden_mixture.py

Conditions enforced here before anything is stored (a speaker that misses one gets another seed in
mixture_cases.SEEDS, and that file says which seed was the first tried; the condition stays):
  * every G_k is a sum of exact zeros and ones below 2, or at least 0.5 away from 2;
  * every l_k - m is >= -700 or <= -800;
  * no unfloored variance is within 1e-6 relative of its floor, except the exact zeros.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mixture_cases as mc          # noqa: E402


def main():
    fx = mc.make_fixture()
    for name, job in sorted(fx['jobs'].items()):
        for spk, e in sorted(job.items()):
            if e['ok']:
                assert mc.conditions_hold([float(g) for g in e['G']], e['unit'], e['check']), (name, spk, e['G'], e['check'])
                print('%-14s %-6s floored %-22s G %s  %s' % (name, spk, e['floored'], ' '.join('%.4g' % float(g) for g in e['G']),
                                                         ' '.join('%s %s %.1e' % (g, v['tier'], v['e']) for g, v in sorted(e['groups'].items()))))
            else:
                print('%-14s %-6s not ok' % (name, spk))
    assert not fx['scores']['check']['in_band'], fx['scores']['check']
    print('scores', fx['scores']['groups'], fx['scores']['check'])
    for spk, e in sorted(fx['ubm'].items()):
        assert not e['check']['in_band'], (spk, e['check'])
        print('ubm', spk, e['groups'], e['check'])
    mc.save(fx)
    print('%d + %d bytes' % (os.path.getsize(mc.FIXTURE), os.path.getsize(mc.FIXTURE_ARRAYS)))


if __name__ == '__main__':
    main()
