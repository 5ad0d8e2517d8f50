#!/usr/bin/env python3
"""Writes tests/golden/gw_kind_instances.npz: the results tests/test_gw_kind_instances.py pins,
computed on an MI355X by a library built from the commit BEFORE k_gw was split into one instance
per distance kind (the fixture must never come from the code under test):

    git worktree add /tmp/before <commit>; make -C /tmp/before/speaker-diarization_amd/csrc
    SPKD_HIP_LIBRARY=/tmp/before/speaker-diarization_amd/csrc/libspkd_hip.so python tools/record_gw_kind_bits.py

The calls themselves are stated once, in tests/gw_kind_cases.py.  That library has one k_gw per
wave shape and its four shapes give the same bits (tests/test_gw_wave_shapes_small.py holds that
for BIC); the recorder checks it for every kind and stores one copy per kind, as KIND.name."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'gw_kind_instances.npz'))
    args = ap.parse_args()
    if not os.environ.get('SPKD_HIP_LIBRARY'):
        sys.exit('SPKD_HIP_LIBRARY must name a library built from the commit before the change')
    try:
        import torch  # noqa: F401  (its HIP runtime has to be the first in the process)
    except ImportError:
        pass
    import gw_kind_cases as cases
    got = cases.run_all()
    res = {}
    for kind in cases.KINDS:
        ref = got[(kind, cases.SHAPES[0])]
        for nw in cases.SHAPES[1:]:
            diff = cases.same(ref, got[(kind, nw)])
            if diff is not None:
                sys.exit('%s: wave shapes %d and %d of this library differ in %s' % (kind, cases.SHAPES[0], nw, diff))
        for name, arr in ref.items():
            res['%s.%s' % (kind, name)] = arr
    np.savez_compressed(args.out, **res)
    print('%s: %d arrays, %d bytes, library %s' % (args.out, len(res), os.path.getsize(args.out),
                                                   os.environ['SPKD_HIP_LIBRARY']))


if __name__ == '__main__':
    main()
