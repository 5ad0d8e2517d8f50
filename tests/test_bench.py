"""bench.py's --dump-outputs (what the last timed step returned, as .npy files) and --steps."""
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
