#!/usr/bin/env python3
"""The CLR chain's and the gallery's reference on records unlike the friendly ones (tests/clr_cases.py):
every pair's ratio, the merge log, the labels and the identities in exact arithmetic
(tests/exact_clr.py), each value rounded once to float64 and stored as a 17-digit decimal, and per
group the error e of the float64 restatements (tests/link_clr_numpy.py, tests/gallery_numpy.py)
against that reference with the tier it puts the group in.

Writes tests/golden/clr_exact.json.

    python tests/golden/make_golden_clr.py

Condition enforced here before anything is stored (clr_cases.conditions_hold): every decision of the
exact chain and of the exact assignment keeps 1e-9, and twice the device's allowance, from its
threshold and from the best pair of a lower value.  A group that misses it gets another seed in
clr_cases.GROUPS, and that file says which seed was the first tried; the condition stays.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import clr_cases as cc          # noqa: E402


def main():
    fx = cc.make_fixture()
    for name in cc.NAMES:
        e = fx['groups'][name]
        if not e['finite']:
            print('%-8s not finite' % name)
            continue
        assert e['tier'] != 'outside', (name, e['e'])
        assert cc.conditions_hold(e), (name, e['chain_margins'], e['identify'])
        print('%-8s tier %s e %.2e |v|max %.3g merges %d (restated log the same: %s) chain margins %s ident %s' % (
            name, e['tier'], e['e'], e['vmax'], len(e['merges']), e['restated_log_same'], e['chain_margins'],
            e['identify']['exclusive']['ident']))
    cc.save(fx)
    print('%d bytes' % os.path.getsize(cc.FIXTURE))


if __name__ == '__main__':
    main()
