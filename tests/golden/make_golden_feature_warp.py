"""Draws the channels of tests/test_feature_warp.py once: per file of test_link_clr._people_fixture() a
per-dimension gain a = exp(U(-0.4, 0.4)) and offset b = N(0, 1) * std_d (std_d over the whole batch), from
default_rng(5), per file the 39 gains first and the 39 offsets after them.  The test reads the frozen numbers
(feature_warp_channel.npz), not the generator.  Run from tests/: python golden/make_golden_feature_warp.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import conftest  # noqa: E402,F401
from test_link_clr import _people_fixture  # noqa: E402


def main():
    feats = _people_fixture()[1]
    std = feats.std(axis=0).astype(np.float64)
    rng = np.random.default_rng(5)
    gain, offset = [], []
    for _ in range(3):
        gain.append(np.exp(rng.uniform(-0.4, 0.4, 39)))
        offset.append(rng.normal(0.0, 1.0, 39) * std)
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'feature_warp_channel.npz'), gain=np.array(gain),
             offset=np.array(offset))


if __name__ == '__main__':
    main()
