"""The sweep functions of k_gw have no register-save frame (spkd_cd.hpp, GW_SWEEP_FN).

gw_sweep_coarse, gw_sweep_fine and gw_sweep_tail are `noinline` device functions of their own,
one set per wave shape.  With the default linkage of a template the compiler saves the
callee-saved half of the register file to scratch at entry and reads it back before the return:
100 / 96 / 72 stores and loads per CALL in the one-wave shape, one call per scan.  `static` and
`not_tail_called` together take the frame away; this test holds it away.

It builds the device assembly with the Makefile's own recipe (a minute or two of CPU, no GPU)
and reads nothing but the metadata the compiler prints behind each symbol: `; ScratchSize:` of
the twelve functions, `; Occupancy:` of k_gw<1>."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'speaker-diarization_amd', 'csrc')
FUNCTIONS = ('gw_sweep_coarse', 'gw_sweep_fine', 'gw_sweep_tail')
SHAPES = (1, 2, 4, 8)


def _hipcc():
    return os.environ.get('HIPCC') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc')
                                       else shutil.which('hipcc'))


@pytest.fixture(scope='module')
def metadata(tmp_path_factory):
    """symbol -> {'ScratchSize': n, 'Occupancy': n} for every function and kernel of the listing."""
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip('hipcc is not installed')
    tmp = tmp_path_factory.mktemp('gw_sweep_frame')
    # the Makefile's spkd_hip.gfx950.s recipe, the listing written into the temporary directory
    subprocess.check_call(['make', '-C', str(tmp), '-f', os.path.join(CSRC, 'Makefile'), 'HIPCC=' + hipcc,
                           'SRC=' + os.path.join(CSRC, 'spkd_hip.hip'), 'HDR=', 'spkd_hip.gfx950.s'])
    meta, sym = {}, None
    with open(os.path.join(str(tmp), 'spkd_hip.gfx950.s')) as f:
        for line in f:
            m = re.match(r'\s*\.type\s+(\S+),@function', line)
            if m:
                sym = m.group(1)
                meta[sym] = {}
                continue
            m = re.match(r'; (ScratchSize|Occupancy): (\d+)', line)
            if m and sym is not None:
                meta[sym][m.group(1)] = int(m.group(2))
    return meta


def _instances(meta, name):
    """wave shape -> metadata of spkd::name<shape> (a function with internal linkage carries an L
    in front of its mangled name)."""
    out = {}
    for sym, md in meta.items():
        m = re.match(r'_ZN4spkdL?%d%sILi(\d+)E' % (len(name), name), sym)
        if m:
            assert int(m.group(1)) not in out, sym
            out[int(m.group(1))] = md
    return out


def test_all_twelve_sweep_functions_are_found(metadata):
    found = sorted((name, nw) for name in FUNCTIONS for nw in _instances(metadata, name))
    assert found == sorted((name, nw) for name in FUNCTIONS for nw in SHAPES)


@pytest.mark.parametrize('name', FUNCTIONS)
def test_sweep_function_has_no_scratch(metadata, name):
    inst = _instances(metadata, name)
    assert sorted(inst) == list(SHAPES)
    assert {nw: md['ScratchSize'] for nw, md in inst.items()} == {nw: 0 for nw in SHAPES}


def test_one_wave_kernel_keeps_two_waves_per_simd(metadata):
    inst = _instances(metadata, 'k_gw')
    assert sorted(inst) == list(SHAPES)
    assert inst[1]['Occupancy'] == 2
