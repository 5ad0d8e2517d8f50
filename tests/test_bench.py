"""bench.py's --dump-outputs (what the last timed step returned, as .npy files), --steps and --full."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT

bench = importlib.import_module('bench')


def test_dump_outputs_writes_float64_arrays_by_name(tmp_path):
    arrays = {'file_00000': np.arange(6, dtype=np.int64).reshape(2, 3), 'file_00001': np.zeros((0, 3))}
    names = bench.dump_outputs(str(tmp_path / 'd'), arrays)
    assert names == ['file_00000', 'file_00001']
    for k in names:
        got = np.load(str(tmp_path / 'd' / (k + '.npy')))
        assert got.dtype == np.float64 and np.array_equal(got, arrays[k])


def test_dump_outputs_over_the_cap_is_a_fixed_sample_within_it(tmp_path):
    rng = np.random.default_rng(1)
    arrays = {'file_%05d' % i: rng.standard_normal((100 + i, 3)) for i in range(50)}
    cap = 20 * (150 * 3 * 8 + 128)
    a = bench.dump_outputs(str(tmp_path / 'a'), arrays, cap=cap)
    b = bench.dump_outputs(str(tmp_path / 'b'), arrays, cap=cap)
    assert a == b and 0 < len(a) < len(arrays)
    assert sorted(os.listdir(str(tmp_path / 'a'))) == [k + '.npy' for k in a]
    assert sum(os.path.getsize(str(tmp_path / 'a' / (k + '.npy'))) for k in a) <= cap
    # one array grown: the sample of the other build is a prefix of the same order
    grown = dict(arrays, **{a[0]: np.zeros((400, 3))})
    c = bench.dump_outputs(str(tmp_path / 'c'), grown, cap=cap)
    assert set(c) <= set(a) or set(a) <= set(c)


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, 'bench.py', '--steps', '0'], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and '--steps must be at least 1' in r.stderr


# keys of the line that only --full measures (runs of their own beside the timed steps)
FULL_ONLY = ('two_batches_in_flight', 'value_incl_h2d', 'dropin_scripts_wall_s', 'host_driven_modes_1h',
             'hbm_copy_GBps', 'other_configs', 'cpu_baseline', 'cpu_baseline_stats')


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '2', '--warmup', '1'])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '2', '--warmup', '1', '--full'])
    assert bench.parse().full is True


@pytest.mark.gpu
def test_plain_run_leaves_the_extras_to_full(tmp_path):
    """A plain run carries the headline and the figures of its own timed steps; --full adds the
    comparison of file 0 with the drop-in scripts and every measurement beside the headline.
    The timed steps return the same rows either way."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('WORLD_SIZE', None)
    lines, dumps = {}, {}
    for mode, extra in (('plain', []), ('full', ['--full', '--cpu-sample-seconds', '30'])):
        d = str(tmp_path / mode)
        r = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--files', '2', '--seconds', '120',
                            '--steps', '1', '--warmup', '1', '--dump-outputs', d] + extra,
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines[mode] = json.loads(r.stdout.strip().splitlines()[-1])
        dumps[mode] = {k: np.load(os.path.join(d, k)) for k in sorted(os.listdir(d))}
    plain, full = lines['plain'], lines['full']
    for k in ('metric', 'unit', 'higher_is_better', 'dtype', 'steps', 'warmup'):
        assert plain[k] == full[k], k
    for line in (plain, full):
        assert line['value'] > 0 and line['ms_per_step'] > 0 and line['kernels'] and line['roofline']
    assert not set(FULL_ONLY) & set(plain), sorted(set(FULL_ONLY) & set(plain))
    assert set(FULL_ONLY) <= set(full), sorted(set(FULL_ONLY) - set(full))
    assert 'file0_rows' not in plain['verified'] and full['verified']['file0_rows'] > 3
    assert plain['verified']['digest'] == full['verified']['digest']
    assert sorted(dumps['plain']) == sorted(dumps['full']) == ['file_00000.npy', 'file_00001.npy']
    for k in dumps['plain']:
        assert np.array_equal(dumps['plain'][k], dumps['full'][k])


@pytest.mark.gpu
def test_dump_outputs_is_the_timed_result_and_repeats(tmp_path):
    """Two runs with the same arguments dump the same arrays, and they are the rows of the last
    timed step (the --dump-rows archive of the same run)."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('WORLD_SIZE', None)
    dumps = []
    for run in ('a', 'b'):
        d = str(tmp_path / run)
        npz = str(tmp_path / (run + '.npz'))
        r = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--files', '3', '--seconds', '120',
                            '--steps', '2', '--warmup', '1', '--no-cpu-baseline', '--no-extras',
                            '--dump-outputs', d, '--dump-rows', npz],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        assert json.loads(r.stdout.strip().splitlines()[-1])['steps'] == 2
        assert sorted(os.listdir(d)) == ['file_00000.npy', 'file_00001.npy', 'file_00002.npy']
        rows = np.load(npz)
        got = {}
        for i in range(3):
            got[i] = np.load(os.path.join(d, 'file_%05d.npy' % i))
            assert got[i].dtype == np.float64 and len(got[i]) > 3
            assert np.array_equal(got[i], rows['f%d' % i])
        dumps.append(got)
    for i in range(3):
        assert np.array_equal(dumps[0][i], dumps[1][i])
