#!/usr/bin/env python3
"""Generate tests/golden/link_cases.json: the REFERENCE's spk_cluster_hi (both scripts) linking
the speakers of three files, executed the way make_golden.py executes the reference (read at
generation time, never copied).

The command lines never link across wavs (spk-clustering.py:289), but spk_cluster_hi takes
`speakers` entries of any length and one feature array: it is called here with the concatenated
features of the files and one multi-segment entry per per-file speaker -- file by file, within a
file by ascending label -- which is the list it would hold had every file's final `speakers`
been concatenated.

Files: synth.make_series (two speakers recur in every file, each file has one of its own);
segments and per-file labels from the generator's ground truth, so that the fixture does not
depend on a detector.  The fixture is REJECTED, and the next seeds are tried (SURVEY.md
8(c)(ix)), unless in every case without max_spk the reference links the recurring speakers and
keeps the others apart, and unless every decision of every case -- each merge against the
threshold and against the runner-up cell, and the stop -- has a margin above 1e-6 relative.
The JSON stores seeds, SHA-256 of the features, the calls' inputs and outputs; no features.
"""
import io
import json
import os
import sys

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                    # noqa: E402

synth = mg.synth
RATE = 125.0
SECONDS, N_SHARED, N_SPK = 60, 2, 3
MARGIN = 1e-6
GLR_THRESHOLD = 1500.0
CASES = [('cl1_bic', 1, 'BIC', 1.3, 0.0, 0), ('cl2_bic', 2, 'BIC', 1.3, 0.0, 0),
         ('cl1_glr', 1, 'GLR', 1.3, GLR_THRESHOLD, 0), ('cl2_glr', 2, 'GLR', 1.3, GLR_THRESHOLD, 0),
         ('cl1_bic_ms3', 1, 'BIC', 1.3, 0.0, 3), ('cl2_bic_ms3', 2, 'BIC', 1.3, 0.0, 3)]


def rel(a, b):
    return abs(a - b) / max(1.0, abs(a), abs(b))


def build_files(seeds, shared_seed):
    """-> (files meta, concatenated features, speakers: per initial speaker its absolute
    (begin, end, line) tuples, truth: per initial speaker its person)."""
    series = synth.make_series(seeds, SECONDS, shared_seed, N_SHARED, N_SPK)
    meta, speakers, person, off, line = [], [], [], 0, 0
    for fi, (feats, _, truth) in enumerate(series):
        segs = [[int(b), int(e), int(k) + 1] for (b, e, k) in truth]
        meta.append({'seed': seeds[fi], 'frames': int(feats.shape[0]), 'sha256': synth.fea_sha256(feats),
                     'segments': segs})
        for lab in sorted(set(s[2] for s in segs)):
            mine = [(i, s) for i, s in enumerate(segs) if s[2] == lab]
            speakers.append([(float(off + s[0]), float(off + s[1]), line + i) for i, s in mine])
            person.append(lab - 1 if lab <= N_SHARED else (fi, lab))
        off += feats.shape[0]
        line += len(segs)
    return meta, np.concatenate([s[0] for s in series]), speakers, person


def run_reference(script, feats, speakers, kind, lambdac, threshold, max_spk):
    """One call of the reference's spk_cluster_hi -> (merges with exact distances, partition,
    stdout text, every distance it computed in call order)."""
    ns = mg.load_reference(script, 'ref_link')
    a = mg.Args()
    a.lambdac, a.max_spk, a.dlr, a.tt = lambdac, max_spk, True, False
    out, merges, log = io.StringIO(), [], []

    def hook(*args, **kw):
        mg._py2_print(*args, file=out)
        if args and args[0] == 'Merging:':
            merges.append((int(args[1]) - 1, int(args[3]) - 1, float(args[5])))

    base = ns[kind.lower()]

    def dist(x, y):
        d = base(x, y)
        log.append(float(d))
        return d

    ns.update(args=a, threshold=threshold, rate=RATE, segpath='', lna_letter='a', lna_count=0, max_dist=0,
              min_dist=sys.maxsize, max_det_dist=0, min_det_dist=sys.maxsize, print=hook)
    n_lines = 1 + max(t[2] for s in speakers for t in s)
    recipe = [('link.wav', 'a_%d' % l, 0.0, 0.0) for l in range(n_lines)]
    outf = io.StringIO()
    with np.errstate(all='ignore'):
        ns['spk_cluster_hi'](feats, recipe, [list(s) for s in speakers], outf, dist=dist)
    final = {}
    for ln in outf.getvalue().splitlines():
        f = dict(kv.split('=', 1) for kv in ln.split(' '))
        final[int(f['lna'][2:])] = int(f['speaker'][len('speaker_'):])
    assert len(final) == n_lines
    groups = {}
    for i, s in enumerate(speakers):
        ks = set(final[t[2]] for t in s)
        assert len(ks) == 1
        groups.setdefault(ks.pop(), []).append(i)
    return merges, [groups[k] for k in sorted(groups)], out.getvalue(), log


def margins(variant, n, merges, log, threshold, max_spk):
    """Replays the reference's matrix from the distances it computed (its own order of calls) and
    returns per decision the relative margins to the threshold and to the runner-up cell."""
    it = iter(log)
    dm = np.zeros((n, n)) if variant == 1 else np.full((n, n), np.inf)
    if variant == 1:
        np.fill_diagonal(dm, sys.maxsize)
    for s1 in range(n):
        for s2 in range(s1 + 1, n):
            dm[s1, s2] = next(it)
            if variant == 1:
                dm[s2, s1] = dm[s1, s2]
    out = []
    for step in range(len(merges) + 1):
        m = dm.shape[0]
        mind, index = float(dm.min()), int(dm.argmin())
        a, b = sorted((index // m, index % m))
        cells = dm.copy()
        np.fill_diagonal(cells, np.inf)
        cells[index // m, index % m] = np.inf
        if variant == 1:
            cells[index % m, index // m] = np.inf
        runner = float(cells.min()) if m > 1 else float('inf')
        forced = max_spk > 0 and m > max_spk
        rec = {'step': step, 'threshold': None if forced or not np.isfinite(mind) or m < 2 else rel(mind, threshold),
               'runner_up': rel(runner, mind) if np.isfinite(runner) and step < len(merges) else None}
        out.append(rec)
        if step == len(merges):
            assert not (mind <= threshold or forced), 'the replay would merge where the reference stopped'
            break
        assert (a, b, mind) == merges[step], ('the replay left the reference', step, (a, b, mind), merges[step])
        dm = np.delete(np.delete(dm, b, axis=0), b, axis=1)
        for s2 in range(m - 1):
            if s2 != a:
                dm[a, s2] = next(it)
                if variant == 1:
                    dm[s2, a] = dm[a, s2]
    assert next(it, None) is None, 'distances left over'
    return out


def attempt(seeds, shared_seed):
    meta, feats, speakers, person = build_files(seeds, shared_seed)
    if any(len(set(s[2] for s in m['segments'])) != N_SPK for m in meta):
        return None, 'a file lacks a speaker'
    want = sorted(sorted(i for i, p in enumerate(person) if p == q) for q in set(person))
    cases = []
    for name, variant, kind, lambdac, threshold, max_spk in CASES:
        script = 'spk-clustering.py' if variant == 1 else 'spk-clustering2.py'
        merges, partition, stdout, log = run_reference(script, feats, speakers, kind, lambdac, threshold, max_spk)
        if max_spk == 0 and sorted(sorted(g) for g in partition) != want:
            return None, '%s: partition %r is not the people %r' % (name, partition, want)
        mar = margins(variant, len(speakers), merges, log, threshold, max_spk)
        worst = min(v for r in mar for v in (r['threshold'], r['runner_up']) if v is not None)
        if not worst > MARGIN:
            return None, '%s: a decision within %g relative' % (name, worst)
        cases.append({'name': name, 'variant': variant, 'kind': kind, 'lambdac': lambdac, 'threshold': threshold,
                      'max_spk': max_spk, 'merges': [[a, b, mg.hexf(d)] for a, b, d in merges],
                      'partition': partition, 'stdout': stdout, 'margins': mar, 'min_margin': worst})
    return {'rate': RATE, 'seconds': SECONDS, 'n_shared': N_SHARED, 'n_speakers': N_SPK, 'shared_seed': shared_seed,
            'files': meta, 'speakers': [[[int(b), int(e), l] for b, e, l in s] for s in speakers],
            'people': want, 'margin_bar': MARGIN, 'cases': cases}, 'ok'


def main():
    base = 20261018
    for k in range(64):
        seeds = [base + 10 * k + 1, base + 10 * k + 2, base + 10 * k + 3]
        data, why = attempt(seeds, base + 10 * k)
        print('seeds %r: %s' % (seeds, why))
        if data is not None:
            break
    else:
        raise SystemExit('no fixture found')
    data['env'] = {'python': sys.version.split()[0], 'numpy': np.__version__, 'scipy': scipy.__version__,
                   'note': 'generated by executing the reference functions via tests/golden/make_golden_link.py'}
    with open(os.path.join(HERE, 'link_cases.json'), 'w') as f:
        json.dump(data, f, indent=1)
    for c in data['cases']:
        print('  %-12s %d merges, %d speakers, smallest margin %.3g' % (c['name'], len(c['merges']), len(c['partition']),
                                                                        c['min_margin']))


if __name__ == '__main__':
    main()
