"""Writes tests/golden/ahc_replay.json: every scenario of tests/ahc_replay_cases.py through the literal merge
loop of tests/ahc_replay.py with C oracle distances (minutes on the CPU; oracle/libspkd_oracle.so must be built).

    python tests/golden/make_golden_ahc_replay.py [name prefix ...]     (prefixes: print only, write nothing)

Refuses to write a fixture that misses the safety condition (every gap and threshold gap above 1e-7) or an
event that tests/ahc_replay_cases.py::REQUIRED asks of a variant."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ahc_replay  # noqa: E402
import ahc_replay_cases as cases  # noqa: E402


def main(argv):
    f = cases.frames()
    sha = cases.frames_sha256(f)
    orc = cases.OracleDistances(f)
    out, seen, ok = [], {1: {}, 2: {}}, True
    for s in cases.scenarios():
        if argv and not any(s['name'].startswith(p) for p in argv):
            continue
        t0 = time.time()
        res = cases.run_replay(s, orc)
        fx = cases.to_fixture(s, res, sha)
        out.append(fx)
        bad = ahc_replay.unsafe_rounds(res['rounds'])
        ok = ok and not bad
        for k, v in res['events'].items():
            seen[s['variant']][k] = seen[s['variant']].get(k, 0) + v
        print('%-20s merges %3d  gap %-24s thr %-24s %5.1f s  %s' % (
            s['name'], len(res['merges']), fx['smallest_gap'] and float.fromhex(fx['smallest_gap']),
            fx['smallest_threshold_gap'] and float.fromhex(fx['smallest_threshold_gap']), time.time() - t0,
            'UNSAFE %r' % bad[:3] if bad else ''))
        print('    ', fx['events'], fx['where'])
    for v in (1, 2):
        missing = [e for e in cases.REQUIRED[v] if not seen[v].get(e)]
        print('variant %d: missing events %r' % (v, missing))
        ok = ok and not missing
    if argv:
        return 0
    if not ok:
        print('NOT written: the safety condition or the event table is not met')
        return 1
    with open(os.path.join(HERE, 'ahc_replay.json'), 'w') as fh:
        json.dump({'margin': ahc_replay.MARGIN, 'scenarios': out}, fh, indent=0, sort_keys=True)
        fh.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
