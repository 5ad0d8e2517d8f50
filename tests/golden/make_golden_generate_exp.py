#!/usr/bin/env python3
"""Golden vectors for the .lna post-processing of generate_exp.py: the reference's own
_read_lna / _write_lna / shift_dec_bord (generate_exp.py:119-142, 177-186), executed through
the in-memory py2 loader of make_golden.py.  Inputs are .lna files in phone_probs's layout
(4 count bytes, one byte 4, float32 scores frame-major) of seeded synthetic scores; outputs
are the bytes the reference leaves in the .lna and in <exppath>/<base>.last_frame.

docopt is not needed by these three functions: a stub module stands in for the import at the
top of the script (the Decoder import happens only inside validate_arguments).  The script
opens the .lna with text modes, which is binary under py2; the loaded namespace gets an
`open` that adds 'b' for .lna paths (the reference text is not changed).

    python tests/golden/make_golden_generate_exp.py   # writes tests/golden/generate_exp_cases.json
"""
import builtins
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg            # noqa: E402  (the loader; reads the reference tree at run time)


def _lna_bytes(scores):
    scores = np.ascontiguousarray(scores, dtype='<f4')
    n = scores.shape[1]
    return bytes([(n >> 24) & 255, (n >> 16) & 255, (n >> 8) & 255, n & 255, 4]) + scores.tobytes()


def cases():
    rng = np.random.default_rng(20261016)
    out = []
    ordinary = lambda T: (-60.0 + 10.0 * rng.standard_normal((T, 2))).astype(np.float32)
    for name, T in (('empty', 0), ('one_frame', 1), ('odd', 7), ('even', 10), ('long', 301)):
        out.append((name, ordinary(T)))
    x = ordinary(12)
    x[2] = [-800.0, -800.0]          # both exp underflow: 0 / 0 -> NaN
    x[3, 0] = -800.0                 # one underflows: log 0 -> -inf (or its partner's column)
    x[5, 1] = -900.0
    x[8] = [800.0, -1.0]             # overflow: inf / inf -> NaN
    x[9, 1] = 750.0
    x[10] = [88.0, 89.0]             # large but finite
    out.append(('under_overflow', x))
    y = np.array([[-745.0, -746.0], [709.0, 710.0], [-1e30, 0.0], [0.0, -np.inf]], dtype=np.float32)
    out.append(('limits', y))
    z = np.full((3, 2), np.nan, dtype=np.float32)
    z[1, 0] = -5.0
    out.append(('nan_in', z))
    return out


def main():
    sys.modules['docopt'] = types.ModuleType('docopt')
    sys.modules['docopt'].docopt = lambda *a, **k: {}
    ns = mg.load_reference('generate_exp.py', 'generate_exp')

    def lna_open(path, mode='r', *a, **k):
        if str(path).endswith('.lna') and 'b' not in mode:
            mode += 'b'
        return builtins.open(path, mode, *a, **k)

    ns['open'] = lna_open
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, scores in cases():
            lna = os.path.join(tmp, name + '.lna')
            raw = _lna_bytes(scores)
            with open(lna, 'wb') as f:
                f.write(raw)
            with np.errstate(all='ignore'):
                ns['shift_dec_bord']([lna], tmp)
            with open(lna, 'rb') as f:
                shifted = f.read()
            with open(os.path.join(tmp, name + '.last_frame')) as f:
                last = f.read()
            res.append({'name': name, 'frames': int(scores.shape[0]), 'lna_in': raw.hex(), 'lna_out': shifted.hex(),
                        'last_frame': last})
    doc = {'source': "the reference's generate_exp.py shift_dec_bord / _read_lna / _write_lna run on these inputs "
                     "(tests/golden/make_golden_generate_exp.py)", 'cases': res}
    with open(os.path.join(HERE, 'generate_exp_cases.json'), 'w') as f:
        json.dump(doc, f, indent=1)


if __name__ == '__main__':
    main()
