"""Every k_gw instance -- a wave shape times a distance kind -- against the bits of the kernel
that took the kind as a runtime value (a few seconds of GPU).

k_gw<NW> (BIC), k_gw_glr<NW> and k_gw_kl2<NW> are wrappers of one body (spkd_cd.hpp, gw_body) with
the kind as a constant: the BIC instance carries no second rank-one term, no GLR weights and no
KL2 branch, the KL2 instance no quad item loop.  The arithmetic of a kind is the same operations
on the same operands in the same order as before, so every output is the same to the bit.
tests/test_gw_wave_shapes_small.py compares the shapes of ONE build with each other; this test
compares all twelve instances with tests/golden/gw_kind_instances.npz, recorded by
tools/record_gw_kind_bits.py from a library of the commit before the split.

The calls are stated once, in tests/gw_kind_cases.py: the four short turns of the shape test, in
fused mode.  Compared are n_win, win_maxd, win_det, det_start, det_maxi, det_d, final_start and
every segment record.  That the fixture exercises each kind -- a detection, a negative coarse
scan, a fine scan that starts from a cache record -- is asserted on the fixture itself (no GPU
needed for that)."""
import os

import numpy as np
import pytest

import gw_kind_cases as cases


@pytest.fixture(scope='module')
def golden(golden_dir):
    """kind -> name -> array of the recorded library."""
    out = {k: {} for k in cases.KINDS}
    with np.load(os.path.join(golden_dir, 'gw_kind_instances.npz')) as z:
        for key in z.files:
            kind, name = key.split('.', 1)
            out[kind][name] = z[key]
    return out


@pytest.fixture(scope='module')
def runs():
    return cases.run_all()


@pytest.mark.parametrize('kind', cases.KINDS)
def test_the_fixture_exercises_the_kind(golden, kind):
    g = golden[kind]
    assert sorted(g) == sorted(['n_win', 'final_start'] + [
        't%d.%s' % (t, k) for t in range(cases.N_TURNS)
        for k in cases.EVENTS + cases.DETECTIONS + ('records', 'best_k')])
    det = [g['t%d.win_det' % t] for t in range(cases.N_TURNS)]
    assert all(len(det[t]) == int(g['n_win'][t]) for t in range(cases.N_TURNS))
    nd = [int(d.sum()) for d in det]
    assert int(g['n_win'][0]) == 0 and nd[0] == 0                   # no scan: the tail record alone
    assert nd[1] >= 1 and nd[2] >= 1                                # detections
    assert int((det[1] == 0).sum()) >= 1 and det[1][0] == 0         # negative coarse scans before the first one
    assert nd[3] == 0 and int(g['n_win'][3]) > 3                    # negative to the turn end
    assert len(g['t1.best_k']) == nd[1] and int(g['t1.best_k'].min()) >= 2   # fine scan from a cache record
    assert len(g['t2.best_k']) == nd[2] and int(g['t2.best_k'][0]) < 2       # ... and one from zero sums
    for t in range(cases.N_TURNS):
        assert len(g['t%d.win_maxd' % t]) == int(g['n_win'][t])
        for k in cases.DETECTIONS:
            assert len(g['t%d.%s' % (t, k)]) == nd[t]
        rec = g['t%d.records' % t]
        assert rec.shape[0] == nd[t] + 1 and np.isfinite(rec).all()
        assert np.isfinite(g['t%d.win_maxd' % t]).all() and np.isfinite(g['t%d.det_d' % t]).all()
        # the tail's record is the tail's: it carries the frame count of [final start, turn end)
        b, e = cases._case()[1][t]
        assert rec[nd[t], -1] == float(e - b - int(g['final_start'][t]))
    # a detection's maximum beats the threshold, the negative windows' do not
    thr = cases.THRESHOLD[kind]
    for t in range(cases.N_TURNS):
        assert (g['t%d.det_d' % t] > thr).all()
        assert (g['t%d.win_maxd' % t][det[t] == 0] <= thr).all()


@pytest.mark.gpu
@pytest.mark.parametrize('nw', cases.SHAPES)
@pytest.mark.parametrize('kind', cases.KINDS)
def test_instance_equals_the_recorded_kernel_bit_for_bit(runs, golden, kind, nw):
    got, want = runs[(kind, nw)], golden[kind]
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        x, y = want[name], got[name]
        assert x.dtype == y.dtype and x.shape == y.shape, (kind, nw, name)
        assert np.array_equal(cases.bits(x), cases.bits(y)), (kind, nw, name)
