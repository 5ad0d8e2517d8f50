#!/usr/bin/env python
"""Times the three kernels of the speaker gallery (spkd_clr_identify's k_ident_scores and k_ident_assign,
spkd_bw_accumulate's kernel) with the context's timers: random records of --comp components, --probes
probes in groups of --group and as ONE group, against each --gallery size, and spkd_clr_link over the same
probes beside them for scale.  Per case one warm-up and the median of --runs runs: the kernels'
milliseconds from spkd_last_kernel_ms and the wall milliseconds of the call.  The records are people
--spread a dimension off a random background model, --per-person records a person in the gallery, so
that three probes in four find somebody, rows compete for columns, and one in four is a stranger.  One JSON line.

  python tools/gallery_time.py [--probes 1024] [--group 4] [--gallery 1024,16384] [--comp 8] [--runs 5] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hipabi = importlib.import_module('speaker-diarization_amd.hipabi')
DIM = hipabi.DIM


def model(rng, K):
    ubm = np.zeros((K, hipabi.GMM_COMP))
    ubm[:, 0] = np.log(1.0 / K)
    ubm[:, 1:1 + DIM] = rng.normal(0.0, 1.0, (K, DIM))
    ubm[:, 1 + DIM:1 + 2 * DIM] = 1.0 / rng.uniform(0.5, 2.0, (K, DIM))
    ubm[:, 1 + 2 * DIM] = -0.5 * (DIM * np.log(2.0 * np.pi) - np.log(ubm[:, 1 + DIM:1 + 2 * DIM]).sum(axis=1))
    return ubm


def records(rng, ubm, shift, who):
    K = len(ubm)
    sd = np.sqrt(1.0 / ubm[:, 1 + DIM:1 + 2 * DIM])
    rec = np.zeros((len(who), K, hipabi.BW_COMP))
    rec[:, :, 0] = rng.uniform(50.0, 500.0, (len(who), K))
    mean = ubm[None, :, 1:1 + DIM] + shift[who] * sd + rng.normal(0.0, 0.03, (len(who), K, DIM)) * sd
    rec[:, :, 1:] = rec[:, :, :1] * mean
    return rec


def timed(ctx, fn, timers, runs):
    """One warm-up, then the medians over `runs` calls: wall ms and each named kernel timer."""
    fn()
    wall, kern = [], {k: [] for k in timers}
    for _ in range(runs):
        t = time.perf_counter()
        out = fn()
        wall.append(1e3 * (time.perf_counter() - t))
        for k in timers:
            kern[k].append(ctx.last_ms(k))
    row = dict(call_ms=float(np.median(wall)))
    row.update({k + '_ms': float(np.median(v)) for k, v in kern.items()})
    return row, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--probes', type=int, default=1024)
    ap.add_argument('--group', type=int, default=4)
    ap.add_argument('--gallery', default='1024,16384')
    ap.add_argument('--comp', type=int, default=8)
    ap.add_argument('--per-person', type=int, default=2)
    ap.add_argument('--spread', type=float, default=0.3)
    ap.add_argument('--relevance', type=float, default=16.0)
    ap.add_argument('--threshold', type=float, default=-0.5)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    K, S = a.comp, a.probes
    res = dict(probes=S, group=a.group, components=K, runs=a.runs, relevance=a.relevance, threshold=a.threshold)
    ctx = hipabi.Context(0)
    rng = np.random.default_rng(2026)
    ubm = model(rng, K)
    d_ubm = ctx.dev_alloc(ubm.nbytes)
    ctx.h2d(d_ubm, ubm)
    sizes = [int(v) for v in a.gallery.split(',')]
    enrolled = max(max(sizes) // a.per_person, 1)
    people = enrolled + S                                              # (the last S are enrolled nowhere)
    shift = rng.normal(0.0, a.spread, (people, K, DIM))
    pok = np.ones(S, dtype=np.int32)
    groups = np.arange(0, S + 1, a.group, dtype=np.int64)
    if groups[-1] != S:
        groups = np.append(groups, S)
    for G in sizes:
        # --per-person records of each of the gallery's people; three probes in four are people of the gallery, one a stranger
        who_g = np.arange(G) % max(G // a.per_person, 1)
        who_p = rng.integers(0, max(G // a.per_person, 1), S)
        who_p[::4] = enrolled + rng.integers(0, S, len(who_p[::4]))
        gal, probes = records(rng, ubm, shift, who_g), records(rng, ubm, shift, who_p)
        d_g, d_p = ctx.dev_alloc(gal.nbytes), ctx.dev_alloc(probes.nbytes)
        ctx.h2d(d_g, gal)
        ctx.h2d(d_p, probes)
        gok = np.ones(G, dtype=np.int32)
        row = {}
        for name, off in (('groups_of_%d' % a.group, groups), ('one_group', [0, S])):
            ident = lambda: ctx.clr_identify(d_p, pok, off, d_g, gok, d_ubm, K, a.relevance, a.threshold, True)
            row[name], r = timed(ctx, ident, ('ident_scores', 'ident_assign'), a.runs)
            row[name]['known'] = int((r['ident'] >= 0).sum())
        ident = lambda: ctx.clr_identify(d_p, pok, groups, d_g, gok, d_ubm, K, a.relevance, a.threshold, False)
        row['not_exclusive'], r = timed(ctx, ident, ('ident_scores', 'ident_assign'), a.runs)
        row['not_exclusive']['known'] = int((r['ident'] >= 0).sum())
        row['matrix_bytes'] = S * G * 8
        # every probe added to an identity of its own (what Gallery.update launches for a batch of known speakers)
        slots = rng.permutation(G)[:min(S, G)]
        n = len(slots)
        acc = lambda: ctx.bw_accumulate(d_p, S, K, np.arange(n + 1), np.arange(n), slots, np.ones(n), d_g, G)
        row['accumulate_%d_sets_of_1' % n], _ = timed(ctx, acc, ('bw_accumulate',), a.runs)
        ctx.dev_free(d_g)
        ctx.dev_free(d_p)
        res['gallery=%d' % G] = row
    # for scale: the chain of spkd_clr_link over as many speakers, four records a person
    who = np.arange(S) % max(S // 4, 1)
    spk = records(rng, ubm, shift, who)
    d_s = ctx.dev_alloc(spk.nbytes)
    ctx.h2d(d_s, spk)
    link = lambda: ctx.clr_link(d_s, pok, d_ubm, K, a.relevance, a.threshold)
    res['clr_link'], r = timed(ctx, link, ('clr_link',), a.runs)
    res['clr_link']['merges'] = int(r['n_merges'])
    # and a cluster's record from its speakers: S / 4 sets of four members
    d_c = ctx.dev_alloc(spk.nbytes)
    n = max(S // 4, 1)
    acc = lambda: ctx.bw_accumulate(d_s, S, K, np.arange(0, 4 * n + 1, 4), np.argsort(who[:4 * n], kind='stable'), np.arange(n),
                                    np.zeros(n), d_c, S)
    res['accumulate_%d_sets_of_4' % n], _ = timed(ctx, acc, ('bw_accumulate',), a.runs)
    ctx.dev_free(d_s)
    ctx.dev_free(d_c)
    ctx.dev_free(d_ubm)
    ctx.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
