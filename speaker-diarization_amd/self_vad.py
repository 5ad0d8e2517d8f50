"""Speech / non-speech detection trained on the recording itself: what stands in for a VAD model file
(exp_generator.decode_batch with a VadModel) when there is none.  The quietest frames of a file seed
a non-speech mixture and the loudest a speech mixture, both over the diarization features the
pipeline computes anyway (fconfig.cfg's chain: no second feature chain); decoding and retraining
alternate a few times.  PARITY: no reference counterpart (the reference loads an AaltoASR model,
generate_exp.py:94-97); tests/self_vad_numpy.py restates the stage in numpy.

  seed     spkd_frame_energy_batch on the samples (the features' frame clock, cfg.hop and
           cfg.window_width), then spkd_energy_seeds with k_low = floor(low_share * T),
           k_high = floor(high_share * T) per file: the runs of frames at or below the k_low-th smallest
           energy are class 0 (non-speech), those at or above the k_high-th largest class 1 (speech).
  train    spkd_gmm_train once for the two models of every seeded file, on the features over its runs.
  decode   spkd_gmm_loglik_seq (one sequence per file, its whole frame range, two columns) and
           spkd_mindur_viterbi_batch (penalty, D = max(1, floor(min_dur_s * rate))); the tokens become
           ranges per (file, class), spkd_gmm_train runs again from a fresh start on those, `passes`
           decodes at the most; it stops early when every file decoded what the pass before decoded.
  tokens   word 1 is 'p', word 0 is '<w>': voice_detection.turns_from_tokens runs on them unchanged.

A file is UNTRAINED, yields no tokens (and hence no turns; none is guessed) and is listed in
detail['vad_untrained'] when it is not seeded (a k of 0, or the two thresholds meet: constant audio) or
a seed model is not ok (spkd_gmm_train: fewer than 40 frames a component, constant features).  With
the defaults that is any file shorter than about 13 s: 40 frames a component, four components, from a
tenth of the file at 125 frames a second.  A file whose RETRAINED models are not ok -- or that a pass
decoded into one word only, which leaves the other model nothing to train on -- keeps the tokens it
had and takes no part in later passes.

The scores, the energies and the features never come to the host; only the runs and the tokens do.

SELF_VAD: the shares follow the usual bootstrap (a tenth of the file at either end of the energy
scale).  Every other value is a setting, not a measurement: they rest on synthetic audio and are
unmeasured on speech.  passes = 5 is the one value that was moved: with 3 the numpy restatement split
one stretch of the suite's synthetic recordings in two ("Self-trained speech / non-speech")."""
import collections
import math

import numpy as np

from . import hipabi

SELF_VAD = dict(low_share=0.10, high_share=0.10, components=4, iterations=5, var_floor=0.01,
                penalty=10.0, min_dur_s=0.2, passes=5)
WORDS = ('<w>', 'p')                     # word 0 (the quiet seed's class), word 1 (the loud seed's)

_Options = collections.namedtuple('_Options', 'low_share high_share components iterations var_floor penalty min_dur_s passes')


def _number(opts, key):
    try:
        return float(opts[key])
    except (TypeError, ValueError):
        return float('nan')


def _whole(opts, key):
    v = opts[key]
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _options(opts):
    """A dictionary like SELF_VAD parsed once (absent keys take SELF_VAD's values); ValueError for an
    unknown key, a share outside (0, 0.5], components outside 1 .. GMM_MAX_COMP, negative iterations, a
    floor that is negative or not finite, a penalty or min_dur_s that is negative or not finite,
    passes that is no integer >= 1."""
    if not isinstance(opts, dict):
        raise ValueError('self vad: a dictionary like SELF_VAD')
    unknown = sorted(set(opts) - set(SELF_VAD))
    if unknown:
        raise ValueError('self vad: unknown key %s' % ', '.join(repr(k) for k in unknown))
    o = dict(SELF_VAD, **opts)
    for key in ('low_share', 'high_share'):
        v = _number(o, key)
        if not (0.0 < v <= 0.5):
            raise ValueError('self vad %s: a share of the frames in (0, 0.5]' % key)
    if not _whole(o, 'components') or not 1 <= o['components'] <= hipabi.GMM_MAX_COMP:
        raise ValueError('self vad components: an integer in 1 .. %d' % hipabi.GMM_MAX_COMP)
    if not _whole(o, 'iterations') or o['iterations'] < 0:
        raise ValueError('self vad iterations: an integer >= 0')
    v = _number(o, 'var_floor')
    if not math.isfinite(v) or v < 0.0:
        raise ValueError('self vad var_floor: a finite number >= 0')
    for key in ('penalty', 'min_dur_s'):
        v = _number(o, key)
        if not math.isfinite(v) or v < 0.0:
            raise ValueError('self vad %s: a finite number >= 0' % key)
    if not _whole(o, 'passes') or o['passes'] < 1:
        raise ValueError('self vad passes: an integer >= 1')
    return _Options(float(o['low_share']), float(o['high_share']), int(o['components']), int(o['iterations']),
                    float(o['var_floor']), float(o['penalty']), float(o['min_dur_s']), int(o['passes']))


def seed_counts(opts, n_frames):
    """(k_low, k_high) of a file of n_frames frames: floor(share * T), in Python floats."""
    o = opts if isinstance(opts, _Options) else _options(opts)
    return int(math.floor(o.low_share * n_frames)), int(math.floor(o.high_share * n_frames))


def min_frames(opts, rate):
    """The decoder's D: max(1, floor(min_dur_s * rate))."""
    o = opts if isinstance(opts, _Options) else _options(opts)
    return max(1, int(math.floor(o.min_dur_s * float(rate))))


def token_ranges(tokens, first, n_frames):
    """[(first frame, word)] of a file whose frames are [first, first + n_frames) -> per word 0, 1 the
    absolute ranges (begin, end) its tokens cover, ascending."""
    out = ([], [])
    for (at, word), nxt in zip(tokens, [t for t, _ in tokens[1:]] + [n_frames]):
        out[word].append((first + at, first + nxt))
    return out


def _train(ctx, o, d_frames, total, files, ranges, d_gmm, clock):
    """spkd_gmm_train from a fresh start for the two models of every file of `files` whose two classes both
    have a range (ranges[f] = (class 0's, class 1's)); the models of the k-th such file are 2 k and
    2 k + 1 of d_gmm.  -> {file: k} of the files whose two models are ok."""
    able = [f for f in files if ranges[f][0] and ranges[f][1]]
    if not able:
        return {}
    sets = [ranges[f][c] for f in able for c in (0, 1)]
    set_off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    begin = np.array([b for s in sets for b, _ in s], dtype=np.int64)
    end = np.array([e for s in sets for _, e in s], dtype=np.int64)
    ok, _ = ctx.gmm_train(d_frames, total, set_off, begin, end, o.components, o.iterations, o.var_floor, d_gmm)
    clock('vad_gmm_train', 'gmm_train')
    return {f: k for k, f in enumerate(able) if ok[2 * k] and ok[2 * k + 1]}


def decode_batch(ctx, opts, cfg, d_pcm, sample_off, d_frames, frame_off, timings=None, detail=None):
    """The decision part of stage 1 for a batch of files without a model: d_pcm / sample_off the samples
    as frontend.upload_batch leaves them, d_frames / frame_off their features under cfg as
    frontend.extract_batch leaves them.  Returns what exp_generator.decode_batch returns: (tokens,
    last_frames), per file [(first frame, 'p' | '<w>')] and the frame count.  detail, a dict, receives
    vad_untrained (the files without tokens) and vad_passes_run (the decodes); timings gains vad_energy,
    vad_seeds, vad_gmm_train, vad_loglik, vad_viterbi and vad_backtrack, an entry per call."""
    o = _options(opts)
    frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
    n_files = len(frame_off) - 1
    total = int(frame_off[-1])
    counts = [int(n) for n in np.diff(frame_off)]

    def clock(key, which):
        if timings is not None:
            timings.setdefault(key, []).append(ctx.last_ms(which))

    # seed
    d_energy = ctx.dev_scratch('self_vad_energy', max(total, 1) * 8)
    energy_off = ctx.frame_energy_batch(d_pcm, sample_off, cfg.hop, cfg.window_width, d_energy)
    clock('vad_energy', 'frame_energy')
    assert np.array_equal(energy_off, frame_off), 'the energies and the features run on one frame clock'
    k = [seed_counts(o, T) for T in counts]
    _, _, seeded, run_off, run_begin, run_end = ctx.energy_seeds(d_energy, frame_off, [a for a, _ in k], [b for _, b in k])
    clock('vad_seeds', 'energy_seeds')
    ranges = {}
    for f in range(n_files):
        if seeded[f]:
            ranges[f] = tuple(list(zip(run_begin[run_off[2 * f + c]:run_off[2 * f + c + 1]].tolist(),
                                       run_end[run_off[2 * f + c]:run_off[2 * f + c + 1]].tolist())) for c in (0, 1))
    # train
    d_gmm = ctx.dev_scratch('self_vad_gmm', max(2 * n_files, 1) * o.components * hipabi.GMM_COMP * 8)
    slot = _train(ctx, o, d_frames, total, sorted(ranges), ranges, d_gmm, clock)
    untrained = [f for f in range(n_files) if f not in slot]
    tokens = [[] for _ in range(n_files)]
    d_scores = ctx.dev_scratch('self_vad_scores', max(total, 1) * 2 * 4)
    D = min_frames(o, cfg.frame_rate)
    passes_run = 0
    # decode and retrain
    for p in range(o.passes):
        live = sorted(slot)
        if not live:
            break
        n_models = 2 * (max(slot.values()) + 1)
        seq_off = ctx.gmm_loglik_seq(d_frames, total, d_gmm, o.components, np.ones(n_models, dtype=np.int32),
                                     frame_off[live], frame_off[1:][live], [2 * slot[f] for f in live],
                                     [2] * len(live), 2, d_scores)
        clock('vad_loglik', 'gmm_seq_loglik')
        tok_off, tok_frame, tok_word, _ = ctx.mindur_viterbi_batch(d_scores, seq_off, 2, o.penalty, D)
        clock('vad_viterbi', 'mindur_viterbi')
        clock('vad_backtrack', 'mindur_backtrack')
        passes_run += 1
        same = True
        for q, f in enumerate(live):
            new = list(zip(tok_frame[tok_off[q]:tok_off[q + 1]].tolist(), tok_word[tok_off[q]:tok_off[q + 1]].tolist()))
            same = same and new == tokens[f]
            tokens[f] = new
        if p == o.passes - 1 or same:
            break
        ranges = {f: token_ranges(tokens[f], int(frame_off[f]), counts[f]) for f in live}
        slot = _train(ctx, o, d_frames, total, live, ranges, d_gmm, clock)
    if detail is not None:
        detail['vad_untrained'] = untrained
        detail['vad_passes_run'] = passes_run
    return [[(at, WORDS[w]) for at, w in toks] for toks in tokens], counts
