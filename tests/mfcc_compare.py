"""The ONE comparator of the front-end's tests -- TEST INFRASTRUCTURE ONLY.

A candidate [T, 39] against the float64 restatement oracle/mfcc_numpy.py in STAGE SPACE (mean 0,
scale 1, transform I: the columns are the mean-subtracted statics, the deltas, the delta-deltas),
per column, with a bound from the reference side alone:

    bound[c] = max( MARGIN * max_t |f32[t, c] - f64[t, c]|,  FLOOR_ULPS float32 ulps of max_t |f64[t, c]| )

over all frames of an input, f32 being mfcc_f32_numpy.py without a fault (the same chain in the
kernels' arithmetic, its tables the restatement's rounded to float32) and f64 the restatement (with its
own float64 tables, unless an input brings tables of its own).  Nothing the device computes enters
it.  Under a real scale and transform the bound goes through the linear map:
|transform| . (scale * bound).  tests/test_mfcc_reference.py shows that this comparator rejects
planted faults, and records MARGIN's history and what the device needs of it.
"""
import functools

import numpy as np

import mfcc_f32_numpy as e32

FLOOR_ULPS = 4
MARGIN = 6          # why 6, and the device's ratios under it: the docstring of tests/test_mfcc_reference.py


def column_bound(clean32, want64, margin=None):
    """The bound of every column, from the reference side only."""
    margin = MARGIN if margin is None else margin
    noise = np.abs(clean32.astype(np.float64) - want64).max(axis=0)
    floor = FLOOR_ULPS * np.spacing(np.abs(want64).max(axis=0).astype(np.float32)).astype(np.float64)
    return np.maximum(margin * noise, floor)


def ratios(got, want64, bound):
    """THE comparator: a candidate [T, n] against the float64 restatement -> per column the largest
    |got - want| over the frames, as a fraction of the column's bound.  Accepted: all <= 1."""
    assert got.shape == want64.shape and want64.shape[1] == bound.shape[0], (got.shape, want64.shape)
    assert np.all(np.isfinite(got))
    err = np.abs(np.asarray(got, dtype=np.float64) - want64).max(axis=0)
    return err / bound


def accepted(r):
    return bool(np.all(r <= 1.0))


def blocks(r):
    """The largest ratio of each column block: statics, deltas, delta-deltas."""
    return tuple(float(r[13 * b:13 * b + 13].max()) for b in range(3))


def full_chain(stage, bound, mean, scale, transform):
    """Stage values and their bound through normalization and transform (float64)."""
    mean, scale = np.asarray(mean, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    tr = np.asarray(transform, dtype=np.float64).reshape(39, 39)
    return ((stage - mean[None, :]) * scale[None, :]) @ tr.T, np.abs(tr) @ (scale * bound)


@functools.lru_cache(maxsize=8)
def _full_chain_reference(key, cfg):
    from oracle import mfcc_numpy as m
    pcm = np.frombuffer(key, dtype=np.int16)
    # both sides build the tables from the restatement (the emulation rounds them to float32, as a device
    # table is): frontend.py's builders, whose tables the device is given, stay on the candidate's side
    want = m.stage_features(pcm, cfg)
    bound = column_bound(e32.stage_features(pcm, cfg, m.mel_filterbank(cfg.sample_rate).astype(np.float32),
                                            m.dct_matrix(cfg.n_cep).astype(np.float32)), want)
    return full_chain(want, bound, cfg.mean, cfg.scale, cfg.transform)


def full_chain_bound(pcm, cfg):
    """For a test of one signal under a real configuration (a FeatureConfig): the bound on that
    signal, pushed through cfg's scale and transform, [39]."""
    return _full_chain_reference(np.ascontiguousarray(pcm, dtype=np.int16).tobytes(), cfg)[1]


def full_chain_ratios(got, pcm, cfg):
    """... and the features `got` of `pcm` under `cfg` against the float64 restatement -> ratios [39]."""
    want, bound = _full_chain_reference(np.ascontiguousarray(pcm, dtype=np.int16).tobytes(), cfg)
    return ratios(got, want, bound)
