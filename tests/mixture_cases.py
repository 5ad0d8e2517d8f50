"""Frames unlike the generator's for the mixture kernels, and what is asked of them -- TEST INFRASTRUCTURE ONLY.

The generator's sessions (synth.make_session) leave four pieces of spkd_gmm_train.hpp and
spkd_ubm_stats.hpp idle: the variance floor, the G_k < 2 rule (and a dead component after it), exp
underflow and exact ties among the component log-likelihoods, and initial slots whose edges are rounded
down.  The speakers below reach each of them; tests/exact_mixture.py says what comes out, at 50 digits
and with centred variances; tests/golden/mixture_exact.json and .npz store that (made by
tests/golden/make_golden_mixture.py, reproduced and held to its conditions by tests/test_exact_mixture.py,
asked of the device by tests/test_mixture_exact.py).

Every frame comes from numpy.random.default_rng(seed) rounded to float32 (no frame from synth); a
speaker owns three ranges in descending memory order, so its ordinals and its memory order differ; the
last range of `wnan` ends at n_frames.  N = 1089 = 1024 + 65 is one chunk, one full tile and a tile of
one frame.

speakers
  floor            1089 frames in three stretches (the K = 3 slots) whose means are -1.5, 0, 1.5 sigma along a
                   random sign pattern.  CONST_DIMS are exactly 0.25 in stretch 1 (within-slot variance 0,
                   floored) and 0.25 +- 1 elsewhere.  Dimension SHARED_DIM is + 64 in stretch 2 only: its V is
                   so large that 0.01 V is above every slot's variance, floored in all three.  Under EM the
                   0.25s carry responsibilities that are no longer 0 or 1, so B / G - mean^2 rounds to a few
                   ulp either side of 0: floored too.  At var_floor 0.5 most dimensions floor.
  sa, sb, sc       193 frames in three clusters.  The start model is sa's trained model (the reference's
                   initial model and two steps, rounded to float64) with component 1's means moved to 500.
                   sa: no frame near it, G_1 = 0, ln w = -inf, the second step runs with it dead.
                   sb: frame 100 is 500 in every dimension, G_1 = 1: the weight moves, nothing else.
                   sc: frames 100 .. 102 are, G_1 = 3: the component moves, its variance is all floor.
  wide             385 frames around the seven distinct means of CUBE, the hand-written K = 8 model whose
                   components are 52 sigma and more apart (so every exp but the nearest's is exactly 0:
                   with the frames' own scatter, closer corners would put some l_k - m into the band
                   -800 .. -700 that the conditions keep empty) and whose components 6 and 7 are
                   identical: the frames around them get g = 1/2 each, exactly.
  wide3            the same with other noise and one frame that is 0 but for 3e38 in SHARED_DIM, where all
                   components share mean and variance: finite in double, ok stays 1, and the frame is
                   equally far from all eight (g = 1/8 each, in exact arithmetic and in float64 alike).
  winf, wnan       wide3 behind one more frame: + inf in one dimension, NaN in one dimension.  ok = 0.
  o<K>a, b, c      40 K, 40 K + 1 and 40 K + K - 1 frames of a drifting pool with per-dimension scales
                   over 2^12 (conditioned_cases' `scales`), K in 3, 5, 6, 7: slot edges that round down.
  off1, off8, off64  200 frames in two clusters with those scales, the cluster means 1, 8 and 64 sigma
                   from the origin: where the raw-moment form B / G - mean^2 loses its digits.

seeds: every speaker's seed is the first tried; none was replaced.  What was replaced is the first
construction of `floor` (stretch means drawn from N(0, 2), normal values in CONST_DIMS outside stretch
1): under component 1's floored variances its frames spread over -100 .. -3000, so 98 of them had an
l_k - m inside -800 .. -700 whatever the seed (conditions_hold()).
"""
import hashlib
import json
import math
import os

import numpy as np

import conditioned_cases as cc
import exact_mixture as E
import link_clr_numpy as LC
import reseg_gmm_numpy as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'mixture_exact.json')
FIXTURE_ARRAYS = os.path.join(ROOT, 'tests', 'golden', 'mixture_exact.npz')
DIM, COMP = G.DIM, G.COMP
CONST_DIMS = (3, 11, 20, 33)
SHARED_DIM = 38
CUBE_C = 6.0
ODD_K = (3, 5, 6, 7)
SEEDS = {'floor': 7101, 'starved': 7201, 'wide': 7301, 'wide3': 7302, 'odd': 7401, 'off1': 7501, 'off8': 7502,
         'off64': 7503}
SIZES = [('floor', 1089), ('sa', 193), ('sb', 193), ('sc', 193), ('wide', 385), ('wide3', 385), ('odd', 286),
         ('off1', 200), ('off8', 200), ('off64', 200), ('extra', 2)]
SCALES = cc.sigma('scales')                 # 2^(-9 + d mod 13)


def _normal(seed, n, sd=1.0):
    return np.random.default_rng(seed).normal(0.0, sd, (n, DIM))


def cube_signs():
    """Seven sign vectors (Walsh functions of the dimension's number), SHARED_DIM + 1 in all; row 7 = row 6."""
    s = np.array([[-1.0 if bin(k & (d + 1)).count('1') % 2 else 1.0 for d in range(DIM)] for k in range(1, 8)])
    s[:, SHARED_DIM] = 1.0
    return np.concatenate([s, s[6:7]])


def cube_model(dead=None):
    """CUBE: K = 8, weights 1/8, means CUBE_C * signs, variances 1; dead: a component whose ln w is -inf."""
    m = np.zeros((8, COMP))
    m[:, 0] = math.log(0.125)
    m[:, G.MEAN:G.IVAR] = CUBE_C * cube_signs()
    m[:, G.IVAR:G.NORM] = 1.0
    m[:, G.NORM] = -0.5 * DIM * G.LN_2PI
    if dead is not None:
        m[dead, 0] = -np.inf
    return m


def _wide(seed):
    owner = np.repeat(np.arange(7), [48, 48, 48, 48, 48, 48, 97])
    return CUBE_C * cube_signs()[owner] + _normal(seed, 385)


def _blocks():
    z = _normal(SEEDS['floor'], 1089)
    slot = np.repeat(np.arange(3), 363)
    way = np.where(_normal(SEEDS['floor'] + 1, 1)[0] < 0.0, -1.5, 1.5)
    x = z + (slot[:, None] - 1.0) * way[None, :]
    # CONST_DIMS: 0.25 +- 1 in stretches 0 and 2, so a frame of theirs is the same 75 = 1 / (2 * 0.01 * 2/3)
    # per dimension below component 1 -- a spread of it would cross the band -800 .. -700 for some frame
    x[:, CONST_DIMS] = 0.25 + np.where(z[:, CONST_DIMS] < 0.0, -1.0, 1.0)
    x[363:726, CONST_DIMS] = 0.25
    x[:, SHARED_DIM] = z[:, SHARED_DIM] + np.where(slot == 2, 64.0, 0.0)
    out = {'floor': x}
    sa = _normal(SEEDS['starved'], 193) + _normal(SEEDS['starved'] + 1, 3, 1.5)[np.repeat(np.arange(3), [64, 64, 65])]
    sa = sa.astype(np.float32)
    sb, sc = sa.copy(), sa.copy()
    sb[100], sc[100:103] = 500.0, 500.0
    out.update(sa=sa, sb=sb, sc=sc, wide=_wide(SEEDS['wide']))
    w3 = _wide(SEEDS['wide3'])
    w3[200] = 0.0
    w3[200, SHARED_DIM] = 3.0e38
    out['wide3'] = w3
    t = np.arange(286)[:, None] / 286.0
    sign = np.where(np.arange(DIM) % 2 == 0, 1.0, -1.0)
    out['odd'] = SCALES * (_normal(SEEDS['odd'], 286) + 3.0 * t * sign)
    for m in (1, 8, 64):
        side = np.where(np.arange(200) % 3 == 0, 1.5, -1.5)[:, None]
        out['off%d' % m] = SCALES * (_normal(SEEDS['off%d' % m], 200) + side * sign + m * sign)
    extra = np.zeros((2, DIM))
    extra[0, 5], extra[1, 17] = np.inf, np.nan
    out['extra'] = extra
    return {k: np.asarray(v, dtype=np.float32) for k, v in out.items()}


def _split(b, n):
    """The ordinals 0 .. n of the block at b as three ranges in descending memory order."""
    n1, n2 = n // 3 + 1, 1
    n3 = n - n1 - n2
    return [(b + n3 + n2, b + n), (b + n3, b + n3 + n2), (b, b + n3)]


_BUILT = []


def build():
    """(frames [n, 39] float32, speakers: name -> ranges)."""
    if not _BUILT:
        blocks = _blocks()
        start, b = {}, 0
        for name, n in SIZES:
            assert len(blocks[name]) == n
            start[name], b = b, b + n
        frames = np.zeros((b, DIM), dtype=np.float32)
        spk = {}
        for name, n in SIZES:
            if name in ('odd', 'extra'):
                frames[start[name]:start[name] + n] = blocks[name]
                continue
            spk[name] = _split(start[name], n)
            frames[np.concatenate([np.arange(lo, hi) for lo, hi in spk[name]])] = blocks[name]
        for K in ODD_K:
            for tag, n in zip('abc', (40 * K, 40 * K + 1, 40 * K + K - 1)):
                spk['o%d%s' % (K, tag)] = _split(start['odd'], n)
        e = start['extra']
        spk['winf'] = [(e, e + 1)] + spk['wide3']
        spk['wnan'] = [(e + 1, e + 2)] + spk['wide3']
        assert spk['wnan'][0][1] == len(frames)
        frames.setflags(write=False)
        _BUILT.append((frames, spk, start))
    return _BUILT[0][:2]


def start_of(name):
    build()
    return _BUILT[0][2][name]


def frames_of(name):
    frames, spk = build()
    return LC.frames_of(frames, spk[name])


def sha256():
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(build()[0], dtype='<f4').tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------- what is asked
def _job(name, K, vf, speakers, start=None):
    return dict(name=name, K=K, var_floor=vf, speakers=list(speakers), start=start)


def jobs():
    """The training calls, in the order they are computed: start None is the initial model (n_iter = 0),
    ('ref', job) one step from the reference's result of that job rounded to float64, ('hand', name) one
    step from a stored model."""
    out = []
    k3 = ['floor', 'o3a', 'o3b', 'o3c']
    out += [_job('K3/init', 3, 0.01, k3), _job('K3/step1', 3, 0.01, k3, ('ref', 'K3/init')),
            _job('K3/step2', 3, 0.01, ['floor'], ('ref', 'K3/step1')), _job('K3/step3', 3, 0.01, ['floor'], ('ref', 'K3/step2'))]
    out += [_job('K3h/init', 3, 0.5, ['floor'])]
    out += [_job('K3h/step%d' % i, 3, 0.5, ['floor'], ('ref', 'K3h/' + ('init' if i == 1 else 'step%d' % (i - 1))))
            for i in (1, 2, 3)]
    out += [_job('starved/step1', 3, 0.01, ['sa', 'sb', 'sc'], ('hand', 'starved')),
            _job('starved/step2', 3, 0.01, ['sa'], ('ref', 'starved/step1'))]
    out += [_job('wide/step1', 8, 0.01, ['wide', 'winf', 'wide3', 'wnan'], ('hand', 'cube'))]
    for K in (5, 6, 7):
        spk = ['o%d%s' % (K, t) for t in 'abc'] + ['floor']
        out += [_job('K%d/init' % K, K, 0.01, spk), _job('K%d/step1' % K, K, 0.01, spk, ('ref', 'K%d/init' % K))]
    off = ['off1', 'off8', 'off64']
    for K in (2, 4):
        out += [_job('off%d/init' % K, K, 0.01, off)]
        out += [_job('off%d/step%d' % (K, i), K, 0.01, off, ('ref', 'off%d/' % K + ('init' if i == 1 else 'step%d' % (i - 1))))
                for i in (1, 2, 3)]
    return out


SCORE_LENS = (1, 63, 64, 65, 0)
UBM_SPEAKERS = ('floor', 'sb', 'wide')
UBM_DEAD = 3


def score_sequences():
    """(begin, end) of the scored sequences: sb's frame at 500, frames of sa, and floor's stretch edge."""
    sb, sa, fl = start_of('sb'), start_of('sa'), start_of('floor')
    o = 100                                            # ordinal 100 of sb, in memory
    for lo, hi in build()[1]['sb']:
        if o < hi - lo:
            at = lo + o
            break
        o -= hi - lo
    begin = [at, sa + 10, sa + 100, fl + 330, sa]
    return [(b, b + n) for b, n in zip(begin, SCORE_LENS)]


def fmt(v):
    return '%.17g' % float(v)


def hexes(a):
    return ' '.join(float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel())


def unhex(s):
    return np.array([float.fromhex(v) for v in s.split()], dtype=np.float64)


def starved_model():
    """sa's trained model (the reference's initial model and two steps, each rounded to float64) with
    component 1's means at 500."""
    x = frames_of('sa')
    m = E.to_float(E.init_model(x, 3, 0.01)[0])
    for _ in range(2):
        m = E.to_float(E.em_step(x, m, 0.01)[0])
    m[1, G.MEAN:G.IVAR] = 500.0
    return m


def hand_models():
    return {'starved': starved_model(), 'cube': cube_model()}


def ubm_model(fx):
    """CUBE as the fixture stores it, component UBM_DEAD dead."""
    ubm = unhex(fx['hand']['cube']).reshape(-1, COMP)
    ubm[UBM_DEAD, 0] = -np.inf
    return ubm


def score_models(fx):
    """Four K = 3 models and their ok: sa after starved/step1 (component 1 dead) with the dead component
    first, in the middle and last, and the middle one again marked not ok."""
    mid = ref_model(fx, 'starved/step1', 'sa')
    assert mid[1, 0] == -np.inf
    return [mid[[1, 0, 2]], mid, mid[[0, 2, 1]], mid], np.array([1, 1, 1, 0], dtype=np.int32)


def ref_model(fx, job, spk):
    return fx['jobs'][job][spk]['model'].reshape(-1, COMP)


def start_model(fx, job, spk):
    """The float64 model that enters `job` for `spk` (None: the initial model is asked for)."""
    if job['start'] is None:
        return None
    kind, name = job['start']
    if kind == 'hand':
        return unhex(fx['hand'][name]).reshape(-1, COMP)
    return ref_model(fx, name, spk)


# ---------------------------------------------------------------------- errors and tiers
GROUPS = (('lnw', slice(0, 1)), ('mean', slice(G.MEAN, G.IVAR)), ('ivar', slice(G.IVAR, G.NORM)), ('norm', slice(G.NORM, COMP)))
EPS = 2.0 ** -52
MARGIN = 64.0


def errors(got, want):
    """(largest |got - want|, largest |got - want| / max(1, |got|, |want|), largest |want|) over the entries
    where want is finite; inf when got is not finite there or differs where want is infinite."""
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    fin = np.isfinite(want)
    if not (np.isfinite(got[fin]).all() and np.array_equal(got[~fin], want[~fin])):
        return math.inf, math.inf, float(np.abs(want[fin]).max()) if fin.any() else 0.0
    if not fin.any():
        return 0.0, 0.0, 0.0
    d = np.abs(got[fin] - want[fin])
    return float(d.max()), float((d / np.maximum(1.0, np.maximum(np.abs(got[fin]), np.abs(want[fin])))).max()), \
        float(np.abs(want[fin]).max())


def group_entry(restated, want):
    """What the fixture stores of a group: e, the restatement's largest error, the group's scale, its tier."""
    e, rel, vmax = errors(restated, want)
    return {'e': e, 'vmax': vmax, 'tier': cc.tier_of(rel)}


def model_groups(restated, want, l_restated=None, l_want=None):
    out = {name: group_entry(restated[:, sl], want[:, sl]) for name, sl in GROUPS}
    if l_want is not None:
        out['L'] = group_entry([l_restated], [l_want])
    return out


def device_row(case, group, entry, got, want):
    """One row of the comparison of device values with the reference: the device's errors, the bound
    MARGIN max(e, 2^-52 |value|max) and the quotient error / max(e, 2^-52 |value|max)."""
    err, rel, _ = errors(got, want)
    unit = max(entry['e'], EPS * entry['vmax'])
    return {'case': case, 'group': group, 'tier': entry['tier'], 'scale': entry['vmax'], 'e': entry['e'], 'dev': err,
            'dev_rel': rel, 'quotient': (err / unit if unit > 0.0 else (0.0 if err == 0.0 else math.inf))}


def assert_row(r):
    if r['tier'] != 'outside':
        assert r['dev_rel'] <= cc.TIER_BAR[r['tier']], r
    assert r['quotient'] <= MARGIN, r


def model_rows(case, groups, got, want, l_got=None, l_want=None):
    rows = [device_row(case, name, groups[name], got[:, sl], want[:, sl]) for name, sl in GROUPS]
    if l_want is not None:
        rows.append(device_row(case, 'L', groups['L'], [l_got], [l_want]))
    return rows


# ---------------------------------------------------------------------- the reference of a job
def compute_job(fx, job):
    """The fixture entry of a training call: per speaker ok and, when ok, the reference's model (17 digits),
    L and G_k of a step, the groups' e and tiers, and what conditions() looks at."""
    out = {}
    for spk in job['speakers']:
        x = frames_of(spk)
        start = start_model(fx, job, spk)
        if start is None:
            model, ok, info = E.init_model(x, job['K'], job['var_floor'])
            total = None
        else:
            model, total, _, ok, info = E.em_step(x, start, job['var_floor'])
        ent = {'ok': bool(ok)}
        if ok:
            want = E.to_float(model)
            if start is None:
                rest, rok = G.init_model(x, job['K'], job['var_floor'])
                l_rest = None
            else:
                rest, l_rest, rok = G.em_step(x, start, job['var_floor'])
            assert rok, (job['name'], spk)
            ent['model'] = want.ravel().copy()
            if total is not None:
                ent['L'] = fmt(total)
            ent['groups'] = model_groups(rest, want, l_rest, None if total is None else float(total))
            ent['G'] = [fmt(g) for g in info['G']]
            ent['unit'] = [bool(u) for u in info['unit']]
            ent['floored'] = [0 if r is None else sum(1 for v in r if v < 1) for r in info['ratio']]
            ent['check'] = check_of(info)
        out[spk] = ent
    return out


def check_of(info):
    """What the conditions need of an `info`: the l_k - m nearest the band's edges from outside and inside,
    and the unfloored variance / floor nearest 1 (0 when there is none but exact zeros)."""
    gaps = [g for g in info['gaps']]
    band = [g for g in gaps if -800.0 < g < -700.0]
    ratios = [float(v) for r in info['ratio'] if r is not None for v in r if v != 0]
    near = min(ratios, key=lambda v: abs(v - 1.0)) if ratios else 0.0
    return {'in_band': len(band), 'gap_min_above': min([g for g in gaps if g >= -700.0], default=0.0),
            'gap_max_below': max([g for g in gaps if g <= -800.0], default=-math.inf), 'ratio_nearest_1': near}


def conditions_hold(G_k, unit, check):
    """The three conditions of the fixture on one entry."""
    for g, u in zip(G_k, unit):
        g = float(g)
        if not ((u and g < 2.0 and g == int(g)) or abs(g - 2.0) >= 0.5):
            return False
    if check['in_band']:
        return False
    r = check['ratio_nearest_1']
    return r == 0.0 or abs(r - 1.0) > 1.0e-6


def compute_scores(fx):
    frames = build()[0]
    models, ok = score_models(fx)
    seq, rest, want, gaps = [], [], [], []
    for b, e in score_sequences():
        ref, info = E.scores(frames[b:e], models[:3])
        gaps += info['gaps']
        w = np.array([[float(v) for v in row] for row in ref]).reshape(-1, 3)
        seq.append({'scores': w.ravel().copy()})
        want.append(w)
        rest.append(G.scores(frames[b:e], models, ok, 4)[:, :3])
    return {'seq': seq, 'groups': {'scores': group_entry(np.concatenate(rest), np.concatenate(want))},
            'check': check_of({'gaps': gaps, 'ratio': []})}


def compute_ubm(fx):
    ubm = ubm_model(fx)
    out = {}
    for spk in UBM_SPEAKERS:
        x = frames_of(spk)
        n, f, info = E.ubm_record(x, ubm)
        want = np.array([[float(n[c])] + [float(v) for v in f[c]] for c in range(len(ubm))])
        rest, rok = LC.ubm_stats(x, ubm)
        assert rok
        out[spk] = {'record': want.ravel().copy(),
                    'groups': {'n': group_entry(rest[:, 0], want[:, 0]), 'f': group_entry(rest[:, 1:], want[:, 1:])},
                    'unit': [bool(u) for u in info['unit']], 'check': check_of(info)}
    return out


def make_fixture():
    import mpmath
    fx = {'env': {'numpy': np.__version__, 'mpmath': mpmath.__version__,
                  'note': 'reference: tests/exact_mixture.py at 50 digits; e and tiers: tests/reseg_gmm_numpy.py and '
                          'tests/link_clr_numpy.py in float64; made by tests/golden/make_golden_mixture.py'},
          'sha256': sha256(), 'seeds': SEEDS, 'hand': {k: hexes(v) for k, v in hand_models().items()}, 'jobs': {}}
    for job in jobs():
        fx['jobs'][job['name']] = compute_job(fx, job)
    fx['scores'] = compute_scores(fx)
    fx['ubm'] = compute_ubm(fx)
    return fx


def split(fx, path='', arrays=None):
    """(the fixture with every float64 array replaced by its key, the arrays by key): the arrays -- models,
    scores, records, each value the reference rounded once to float64 -- go to mixture_exact.npz, the rest
    (ok, L and G_k as 17-digit decimals, e, tiers, the hand-written models as hex floats) to the JSON."""
    arrays = {} if arrays is None else arrays
    if isinstance(fx, np.ndarray):
        arrays[path] = fx
        return {'npz': path}, arrays
    if isinstance(fx, dict):
        return {k: split(v, path + '|' + k if path else k, arrays)[0] for k, v in fx.items()}, arrays
    if isinstance(fx, list):
        return [split(v, '%s|%d' % (path, i), arrays)[0] for i, v in enumerate(fx)], arrays
    return fx, arrays


def join(fx, arrays):
    if isinstance(fx, dict):
        return arrays[fx['npz']] if set(fx) == {'npz'} else {k: join(v, arrays) for k, v in fx.items()}
    return [join(v, arrays) for v in fx] if isinstance(fx, list) else fx


def dump(fx):
    return json.dumps(split(fx)[0], indent=None, separators=(',', ':'), sort_keys=True) + '\n'


def save(fx):
    with open(FIXTURE, 'w') as f:
        f.write(dump(fx))
    np.savez_compressed(FIXTURE_ARRAYS, **split(fx)[1])


def same(a, b):
    """Two fixtures or parts of them: equal, arrays bit for bit."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    if isinstance(a, dict) and isinstance(b, dict):
        return set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, list) and isinstance(b, list):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


_FIXTURE = []


def fixture():
    if not _FIXTURE:
        with open(FIXTURE) as f:
            fx = json.load(f)
        with np.load(FIXTURE_ARRAYS) as z:
            _FIXTURE.append(join(fx, {k: z[k] for k in z.files}))
        assert _FIXTURE[0]['sha256'] == sha256(), 'the mixture frames are not reproducible here'
    return _FIXTURE[0]


# ---------------------------------------------------------------------- the device against the fixture
# `dev` is a reseg_helpers.Dev that holds build()'s frames; every function returns device_row()s
# (assert_row holds each to its tier and to MARGIN) after asserting the exact rules itself.
MARK = 12345.0


def _sets(names):
    spk = build()[1]
    off = np.concatenate([[0], np.cumsum([len(spk[n]) for n in names])])
    flat = [r for n in names for r in spk[n]]
    return off, [b for b, _ in flat], [e for _, e in flat]


def train(dev, fx, job, names):
    """One spkd_gmm_train call of `job` on the speakers `names`: (ok, L [n] or None, models [n, K, 80], the
    start models or None).  The buffer holds two more models' worth of marks, which stay."""
    K, n = job['K'], len(names)
    start = None
    buf = np.full((n + 2, K, COMP), MARK)
    if job['start'] is not None:
        start = np.array([start_model(fx, job, s) for s in names])
        buf[:n] = start
    d_gmm = dev.ctx.dev_scratch('mixture_cases_gmm', buf.nbytes)
    dev.ctx.h2d(d_gmm, buf)
    off, b, e = _sets(names)
    ok, ll = dev.ctx.gmm_train(dev.eng.d_frames, len(dev.frames), off, b, e, K, 0 if start is None else 1, job['var_floor'],
                               d_gmm, start is not None)
    got = np.empty_like(buf)
    dev.ctx.d2h(got, d_gmm)
    assert (got[n:] == MARK).all(), 'models beyond the call were written'
    return ok, (None if start is None else ll[:, 0]), got[:n], start


def check_job(dev, fx, job):
    """A training call against the fixture: ok per speaker, ln w = -inf exactly where the reference has it,
    a component the reference leaves where it was (G_k < 2) bit-equal to what entered in its 79 doubles,
    every value (rows), and every speaker alone with the same bits as among the others."""
    names = job['speakers']
    ref = fx['jobs'][job['name']]
    ok, ll, got, start = train(dev, fx, job, names)
    assert ok.tolist() == [int(ref[s]['ok']) for s in names], (job['name'], ok.tolist())
    rows = []
    for i, s in enumerate(names):
        if not ref[s]['ok']:
            continue
        want = ref_model(fx, job['name'], s)
        assert np.array_equal(np.isneginf(got[i][:, 0]), np.isneginf(want[:, 0])), (job['name'], s, got[i][:, 0])
        if start is not None:
            for k, g in enumerate(ref[s]['G']):
                if float(g) < 2.0:
                    assert got[i][k, 1:].tobytes() == start[i][k, 1:].tobytes(), (job['name'], s, k)
        rows += model_rows('%s/%s' % (job['name'], s), ref[s]['groups'], got[i], want,
                           None if ll is None else ll[i], float(ref[s]['L']) if 'L' in ref[s] else None)
        ok1, ll1, got1, _ = train(dev, fx, job, [s])
        assert ok1.tolist() == [1] and got1[0].tobytes() == got[i].tobytes(), (job['name'], s, 'alone')
        assert ll is None or ll1[0] == ll[i], (job['name'], s, 'alone')
    return rows, dict(zip(names, got)), (None if start is None else dict(zip(names, start)))


def device_floor(x, K, var_floor):
    """1 / (var_floor V_d) as the device forms it, in float64 and in the device's order of addition: per
    chunk of 1 024 ordinals and initial slot one chain of the frames and of their squares (both exact
    products), the chunks added per slot, the slots in order; V = sum x^2 / N - (sum x / N)^2."""
    x = G._f64(x)
    n = len(x)
    ta, tb = np.zeros(DIM), np.zeros(DIM)
    for k in range(K):
        a, b = np.zeros(DIM), np.zeros(DIM)
        for c0 in range(0, n, G.TILE * G.CHUNK_TILES):
            lo, hi = max(c0, k * n // K), min(c0 + G.TILE * G.CHUNK_TILES, (k + 1) * n // K)
            part = x[lo:hi] if hi > lo else x[:0]
            a = a + np.add.reduce(np.concatenate([np.zeros((1, DIM)), part]), axis=0)
            b = b + np.add.reduce(np.concatenate([np.zeros((1, DIM)), part * part]), axis=0)
        ta, tb = ta + a, tb + b
    mu = ta / n
    return 1.0 / (var_floor * (tb / n - mu * mu))


def ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a.view(np.int64) - b.view(np.int64))


def floored_mask(fx, job, spk):
    """The entries of 1 / var that the reference floors: [K, 39] bool."""
    want = ref_model(fx, job['name'], spk)
    floor = np.array([float(v) for v in E.variance_floor(frames_of(spk), job['var_floor'])[0]])
    mask = np.abs(want[:, G.IVAR:G.NORM] * floor - 1.0) < 1.0e-12
    moved = np.array([float(g) >= 2.0 for g in fx['jobs'][job['name']][spk]['G']])
    mask &= moved[:, None]
    assert mask.sum(axis=1).tolist() == fx['jobs'][job['name']][spk]['floored'], (job['name'], spk)
    return mask


def check_floored(fx, job, spk, got):
    """A floored 1 / var is 1 / (var_floor V_d) to 2 ulp; returns the largest distance in ulp."""
    mask = floored_mask(fx, job, spk)
    want = np.broadcast_to(device_floor(frames_of(spk), job['K'], job['var_floor']), mask.shape)
    far = ulps(got[:, G.IVAR:G.NORM][mask], want[mask])
    worst = int(far.max()) if far.size else 0
    assert worst <= 2, (job['name'], spk, worst)
    return worst


def check_scores(dev, fx):
    """spkd_gmm_loglik_seq under the models with a dead component first, in the middle and last and one
    model that is not ok, five columns: rows of the values; the float32 scores within 1 ulp of
    float32(reference) in a group of tier 1e-9; -inf for the model that is not ok and the column past the
    models; the rows beyond the total untouched."""
    models, ok = score_models(fx)
    seqs = score_sequences()
    ctx = dev.ctx
    d_gmm = ctx.dev_scratch('mixture_cases_gmm', 8 * 8 * COMP * 8)
    ctx.h2d(d_gmm, np.array(models))
    total, n_cols, pad = sum(SCORE_LENS), 5, 8
    d_scores = ctx.dev_scratch('mixture_cases_scores', (total + pad) * n_cols * 4)
    mark = np.full((total + pad, n_cols), MARK, dtype=np.float32)
    ctx.h2d(d_scores, mark)
    off = ctx.gmm_loglik_seq(dev.eng.d_frames, len(dev.frames), d_gmm, 3, ok, [b for b, _ in seqs], [e for _, e in seqs],
                             [0] * len(seqs), [4] * len(seqs), n_cols, d_scores)
    assert off.tolist() == np.concatenate([[0], np.cumsum(SCORE_LENS)]).tolist()
    got = np.empty_like(mark)
    ctx.d2h(got, d_scores)
    assert np.array_equal(got[total:], mark[total:])
    assert np.isneginf(got[:total, 3:]).all()
    want = np.concatenate([s['scores'].reshape(-1, 3) for s in fx['scores']['seq']])
    assert np.isfinite(got[:total, :3]).all()
    entry = fx['scores']['groups']['scores']
    far = np.abs(got[:total, :3].view(np.int32).astype(np.int64) - want.astype(np.float32).view(np.int32).astype(np.int64))
    if entry['tier'] == '1e-9':
        assert int(far.max()) <= 1, int(far.max())
    # the device rounds once to float32: half an ulp of that is its own, on top of the float64 formulation's e
    half = float(np.abs(np.spacing(want.astype(np.float32)).astype(np.float64)).max()) / 2.0
    err, rel, _ = errors(got[:total, :3].astype(np.float64), want.astype(np.float32).astype(np.float64))
    unit = max(entry['e'], EPS * entry['vmax'], half)
    return [{'case': 'scores', 'group': 'scores', 'tier': entry['tier'], 'scale': entry['vmax'], 'e': entry['e'], 'dev': err,
             'dev_rel': rel, 'quotient': err / unit, 'ulp32': int(far.max())}]


def check_ubm(dev, fx):
    """spkd_ubm_stats of floor, sb and wide under CUBE with component UBM_DEAD dead: the dead component's
    record exactly 0, ok, the records beyond the call untouched, every speaker alone with the same bits;
    rows of n_c and f_c (sum_c n_c = N is a row too: group `N`, e and scale from the n group)."""
    ubm = ubm_model(fx)
    ctx = dev.ctx
    d_ubm = ctx.dev_scratch('mixture_cases_gmm', 8 * 8 * COMP * 8)
    ctx.h2d(d_ubm, ubm)

    def run(names):
        n = len(names)
        buf = np.full((n + 1, 8, LC.BW_COMP), MARK)
        d_bw = ctx.dev_scratch('mixture_cases_bw', buf.nbytes)
        ctx.h2d(d_bw, buf)
        off, b, e = _sets(names)
        ok = ctx.ubm_stats(dev.eng.d_frames, len(dev.frames), d_ubm, 8, off, b, e, d_bw)
        ctx.d2h(buf, d_bw)
        assert (buf[n:] == MARK).all()
        return ok, buf[:n]

    names = list(UBM_SPEAKERS)
    ok, got = run(names)
    assert ok.tolist() == [1] * len(names)
    rows = []
    for i, s in enumerate(names):
        want = fx['ubm'][s]['record'].reshape(8, LC.BW_COMP)
        assert (want[UBM_DEAD] == 0.0).all() and (got[i][UBM_DEAD] == 0.0).all(), s
        g = fx['ubm'][s]['groups']
        rows.append(device_row('ubm/' + s, 'n', g['n'], got[i][:, 0], want[:, 0]))
        rows.append(device_row('ubm/' + s, 'f', g['f'], got[i][:, 1:], want[:, 1:]))
        n_frames = sum(e - b for b, e in build()[1][s])
        rows.append(device_row('ubm/' + s, 'N', {'e': 8 * g['n']['e'], 'vmax': float(n_frames), 'tier': g['n']['tier']},
                               [LC.total(got[i])], [float(n_frames)]))
        ok1, got1 = run([s])
        assert ok1.tolist() == [1] and got1[0].tobytes() == got[i].tobytes(), s
    return rows
