"""k_matrix's passes keep the bare determinant and a dense phase finishes the distances, a thread
per partner.  That moves where a value is computed, never how it is: the same log, the same
finish_distance, the same operands -- so every matrix, every merge log that starts from one and
every statistic is the same to the bit.

tests/golden/matrix_finish_bits.npz was written by tools/record_matrix_finish_bits.py on a library
built from the commit BEFORE that change (never from the code under test); this test runs the same
calls (tests/matrix_finish_cases.py) on the default library and compares float64 arrays as uint64,
NaNs by their bit pattern.  Large matrices are compared as one SHA-256 per row."""
import os

import numpy as np
import pytest

import matrix_finish_cases as cases
from helpers import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'matrix_finish_bits.npz')


@pytest.fixture(scope='module')
def want():
    assert os.path.exists(GOLDEN), 'the fixture %s is missing: tools/record_matrix_finish_bits.py writes it' % GOLDEN
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def got():
    return cases.compute()


def test_the_fixture_compares_something(want):
    """Guards against an empty comparison."""
    for n in cases.MATRIX_N:
        cnt = want['n%d_record_counts' % n]
        s = cases.short_at(n)
        assert cnt.shape == (n,) and cnt[s] == cases.SHORT_LEN and cnt.min() >= cases.SHORT2_LEN
        assert ((cnt >= 60) & (cnt <= 120)).sum() >= n - 2
        for kind in cases.KINDS:
            for variant in cases.VARIANTS:
                m = want['n%d_%s_v%d_matrix' % (n, kind, variant)]
                assert m.shape == ((n, n) if n <= cases.SMALL_N else (n, 32))
                if n <= cases.SMALL_N:
                    upper = m[np.triu_indices(n, 1)]
                    finite = upper[np.isfinite(upper)]       # (a short record's own log det may be a NaN)
                    assert np.count_nonzero(upper) == len(upper) and len(finite) >= len(upper) - 2 * n
                    assert len(np.unique(finite)) == len(finite)
                    low = m[np.tril_indices(n, -1)]
                    assert np.array_equal(cases.bits(low), cases.bits(m.T[np.tril_indices(n, -1)])) if variant == 1 \
                        else np.isposinf(low).all()
                else:
                    # no two rows alike (variant 2: but for the last ones, +inf but for distances to the short records)
                    assert len(np.unique(m, axis=0)) >= n - 2
            if n > 2:
                st = want['n%d_%s_v1_stat' % (n, kind)]
                assert np.isfinite(st).all() and st[0] > st[1]
    # the merge loops merged, in every problem without the short records down to a few clusters
    sizes = np.array(cases.AHC_SIZES)
    clean = (np.arange(len(sizes)) != cases.AHC_SHORT_PROBLEM) & (sizes > 2)
    for path in (1, 2):
        for variant in cases.VARIANTS:
            nm = want['ahc_p%d_v%d_s0_n_merges' % (path, variant)]
            assert (nm[clean] >= sizes[clean] // 2).all(), nm
            nm3 = want['ahc_p%d_v%d_s3_n_merges' % (path, variant)]
            assert (nm3[clean] >= np.maximum(sizes[clean] - 3, 0)).all(), nm3
            assert len(want['ahc_p%d_v%d_s3_d' % (path, variant)]) == int(nm3.sum())
    # sliding windows: distances of both signs, so detections
    d = want['sw_d']
    assert len(d) >= 200 and np.isfinite(d).all() and (d > 0).any() and (d < 0).any() and int(want['sw_n_det'][0]) >= 1


def test_every_result_has_the_bits_of_the_finish_in_the_pass(want, got):
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
            what = 'matrix rows (SHA-256 each)' if k.endswith('_matrix') and w.dtype == np.uint8 else 'values'
            differ.append('%s: %d of %d %s differ, first at %s: %r, fixture %r'
                          % (k, int(ne.any(axis=-1).sum()) if w.dtype == np.uint8 else int(ne.sum()),
                             w.shape[0] if w.dtype == np.uint8 else ne.size, what, tuple(at), g[tuple(at)], w[tuple(at)]))
    assert not differ, '\n'.join(differ)
