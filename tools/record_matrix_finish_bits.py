#!/usr/bin/env python3
"""Writes tests/golden/matrix_finish_bits.npz: the results tests/test_matrix_finish_bits.py pins,
computed on an MI355X by a library built from the commit BEFORE k_matrix's passes parked their
determinants for a dense finish (the fixture must never come from the code under test):

    git worktree add /tmp/before <commit>; make -C /tmp/before/speaker-diarization_amd/csrc
    SPKD_HIP_LIBRARY=/tmp/before/speaker-diarization_amd/csrc/libspkd_hip.so python tools/record_matrix_finish_bits.py

The calls themselves are stated once, in tests/matrix_finish_cases.py."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'matrix_finish_bits.npz'))
    args = ap.parse_args()
    if not os.environ.get('SPKD_HIP_LIBRARY'):
        sys.exit('SPKD_HIP_LIBRARY must name a library built from the commit before the change')
    try:
        import torch  # noqa: F401  (its HIP runtime has to be the first in the process)
    except ImportError:
        pass
    import matrix_finish_cases as cases
    res = cases.compute()
    np.savez_compressed(args.out, **res)
    print('%s: %d arrays, %d bytes, library %s' % (args.out, len(res), os.path.getsize(args.out),
                                                   os.environ['SPKD_HIP_LIBRARY']))


if __name__ == '__main__':
    main()
