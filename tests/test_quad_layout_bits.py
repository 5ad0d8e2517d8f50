"""The quad row split (spkd_quad.hpp: which lane and slot of a DPP row holds a matrix row) is a
relabelling: every element is produced by the same chain of operations in the same order
whatever the split, so everything the elimination kernels return is the same to the bit.

tests/golden/quad_layout_bits.npz was written by tools/record_quad_bits.py on a library built
from the commit BEFORE the split changed from 13/13/13 to 7/16/16 (never from the code under
test); this test runs the same calls (tests/quad_layout_cases.py) on the default library and
compares float64 arrays as uint64, NaNs by their bit pattern."""
import os

import numpy as np
import pytest

import quad_layout_cases as cases
from helpers import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'quad_layout_bits.npz')


@pytest.fixture(scope='module')
def want():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def got():
    return cases.compute()


def test_the_fixture_compares_something(want):
    """Guards against an empty comparison."""
    for nw in cases.GW_WAVES:
        for kind in cases.KINDS:
            tag = 'gw%d_%s_' % (nw, kind)
            assert int(want[tag + 'win_det'].sum()) >= 1 and len(want[tag + 'det_d']) >= 1, tag
    # the 20-frame record: there, with its frame count, and with a row and a column of distances
    assert want['record_counts'].shape == (cases.N_REC,) and want['record_counts'][cases.SHORT] == cases.SHORT_LEN
    assert want['record_short'].shape == (820,) and want['record_short'][819] == cases.SHORT_LEN
    for kind in cases.KINDS:
        m = want['matrix_' + kind]
        assert m.shape == (cases.N_REC, cases.N_REC)
        others = [k for k in range(cases.N_REC) if k != cases.SHORT]
        full = m[np.ix_(others, others)][np.triu_indices(len(others), 1)]
        assert np.isfinite(full).all() and len(np.unique(full)) == len(full)
        assert np.count_nonzero(m[cases.SHORT]) + np.count_nonzero(m[:, cases.SHORT]) >= 1
    # pair terms of the 20-frame record: its own covariance has rank 19, so twenty pivots of the
    # elimination without pivoting are rounding noise of either sign; one of them is negative (all
    # twenty positive: 2^-20) and the pivoting fallback gives the value, which is not finite or
    # the log of a determinant of noise (twenty factors of 1e-16: far below every full-rank one)
    pt = want['pair_terms']
    short_ld = [pt[k, 2 + side] for k, pr in enumerate(cases.PAIRS) for side in (0, 1) if pr[side] == cases.SHORT]
    full_ld = [pt[k, 2 + side] for k, pr in enumerate(cases.PAIRS) for side in (0, 1) if pr[side] != cases.SHORT]
    assert len(short_ld) == 3 and np.isfinite(full_ld).all()
    assert all((not np.isfinite(v)) or v < min(full_ld) - 100.0 for v in short_ld), (short_ld, full_ld)
    # the merge loops merged something
    for path in (1, 2):
        for variant in (1, 2):
            assert want['ahc_p%d_v%d_n_merges' % (path, variant)].sum() >= 3
    assert want['merge_n_done'][0] >= 2 and want['cin_n_done'][0] >= 2


def test_every_result_has_the_bits_of_the_even_split(want, got):
    assert sorted(got) == sorted(want)
    differ = []
    for k in sorted(want):
        w, g = want[k], got[k]
        if w.shape != g.shape or w.dtype != g.dtype:
            differ.append('%s: %s %s, fixture %s %s' % (k, g.dtype, g.shape, w.dtype, w.shape))
            continue
        ne = cases.bits(w) != cases.bits(g)
        if ne.any():
            at = np.argwhere(ne)[0]
            differ.append('%s: %d of %d values differ, first at %s: %r, fixture %r'
                          % (k, int(ne.sum()), ne.size, tuple(at), g[tuple(at)], w[tuple(at)]))
    assert not differ, '\n'.join(differ)
