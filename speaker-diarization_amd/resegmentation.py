"""Viterbi resegmentation of a clustered batch on the device (resegment_batch): the speakers of every file
modelled from what clustering left, every VAD turn scored under them and decoded frame by frame.  A `reseg`
dictionary is parsed once (_reseg_options); the two speaker models (_GaussSpeakers, _GmmSpeakers) share
one interface, train(tokens) -> ok and score(ok) -> frame_off, and own their device buffers.  The turn
table, the segment ranges and the speaker list are those of tables (_turn_table, _segment_ranges,
link_speakers), the layer below every stage; this module imports nothing else of the package but hipabi."""
import collections

import numpy as np

from . import hipabi
from .tables import _segment_ranges, _turn_table, link_speakers

# Viterbi resegmentation (resegment_batch): the cost of a speaker switch inside a turn, in natural-log
# units.  On the synthetic generator every value from 10 to 200 decodes the same paths; real audio,
# whose frames are correlated in time, will want it tuned.
RESEG = dict(penalty=50.0)
RESEG_MAX_SPEAKERS = 16          # of one file: the decoder's word limit (spkd_vad_viterbi_batch)
# the same stage under mixture models: a diagonal-covariance GMM per speaker, trained on the device
# (spkd_gmm_train) from the frames of the speaker's segments.  Settings, not measurements: four
# components and five EM steps are what small per-speaker mixtures usually get; the floor is a share
# of the variance of all the speaker's frames.
RESEG_GMM = dict(penalty=50.0, model='gmm', components=4, iterations=5, var_floor=0.01)
# the same stage with a minimum speaker duration in the decoder (spkd_mindur_viterbi_batch): no row shorter
# than min_dur_s unless it is a whole turn.  A setting, not a measurement: 1.0 s is the detector's own
# smallest window (pipeline.DIA2_CD['winsize_s']), and neither it nor the penalty beside it has been tuned on
# anything but the synthetic generator.  Any reseg dictionary may also carry passes=N (default 1): the speakers
# are retrained on the decoded rows and the turns decoded again, up to N decodes.
RESEG_MD = dict(penalty=50.0, min_dur_s=1.0)
# the same stage with a confidence for every row (spkd_fb_posterior_batch): the mean posterior of the row's
# speaker over its frames, under the switch-penalty loop at the acoustic scale conf_scale (default 1.0).  Any
# reseg dictionary may carry confidence=True.  On the generator's independent frames scale 1 is roughly
# calibrated; speech, whose frames are correlated in time, will want a scale below 1 -- none exists here, so the
# default is unmeasured.
RESEG_CONF = dict(penalty=50.0, confidence=True)
FB_MAX_SCALED_PENALTY = 600.0    # conf_scale * penalty, soft_scale * penalty: the limit of spkd_fb_posterior_batch
# the same stage with soft retraining between the passes (spkd_post_stats): every speaker is trained again on
# all frames of its file's turns, each weighted by the speaker's posterior there at the acoustic scale
# soft_scale, instead of on the frames the decoded path gave it wholly.  Any reseg dictionary with Gaussian
# speakers may carry soft=True.  The default soft_scale of 0.1 rests on the synthetic generator and nothing
# else: there soft at 0.1 was never worse than hard and often much better, at 1 it equals hard (the posteriors
# of 39-dimensional Gaussians are almost one-hot), and at 0.05 a speaker bleeds its mass away and the file
# collapses (DESIGN.md has the table).  On speech it is unmeasured, like conf_scale and the linking thresholds.
RESEG_SOFT = dict(penalty=50.0, passes=5, soft=True)
RESEG_SOFT_SCALE = 0.1
# the same stage with the microphone array's delays as a second stream (frontend.DelayStream; include/spkd.h
# (6b3)): per speaker and channel one Gaussian over the delays of the speaker's frames, and weight times its
# log-likelihood added to every score before anything reads them.  Any reseg dictionary may carry tdoa=.  floor_s
# is the smallest standard deviation of a delay in seconds (one sample at 16 kHz), min_frames the reliable frames
# a speaker needs on a channel.  All three rest on synthetic fixtures and are UNMEASURED on speech.
TDOA = dict(weight=1.0, floor_s=1.0 / 16000.0, min_frames=40)
RESEG_TDOA = dict(penalty=50.0, tdoa=TDOA)


def _reseg_penalty(reseg):
    p = float(reseg['penalty'])
    if not np.isfinite(p) or p < 0.0:
        raise ValueError('reseg penalty: a finite number >= 0 (natural-log units)')
    return p


def _reseg_model(reseg):
    """The speaker model of a `reseg` dictionary: ('gauss',) -- also when the key is absent -- or
    ('gmm', components, iterations, var_floor), the keys RESEG_GMM names (its values where one is
    absent)."""
    m = reseg.get('model', 'gauss')
    if m == 'gauss':
        return ('gauss',)
    if m != 'gmm':
        raise ValueError('reseg model: gauss or gmm')
    k = reseg.get('components', RESEG_GMM['components'])
    it = reseg.get('iterations', RESEG_GMM['iterations'])
    fl = float(reseg.get('var_floor', RESEG_GMM['var_floor']))
    if int(k) != k or not 1 <= k <= hipabi.GMM_MAX_COMP:
        raise ValueError('reseg components: 1 .. %d' % hipabi.GMM_MAX_COMP)
    if int(it) != it or it < 0:
        raise ValueError('reseg iterations: an integer >= 0')
    if not np.isfinite(fl) or fl < 0.0:
        raise ValueError('reseg var_floor: a finite number >= 0 (a share of the variance of all the speaker\'s frames)')
    return ('gmm', int(k), int(it), fl)


def _reseg_min_frames(reseg, rate):
    """D of a `reseg` dictionary, in frames: 0 when min_dur_s is absent or 0 -- the plain decoder --
    otherwise max(1, floor(min_dur_s * rate))."""
    try:
        s = float(reseg.get('min_dur_s', 0.0))
    except (TypeError, ValueError):
        s = float('nan')
    if not np.isfinite(s) or s < 0.0:
        raise ValueError('reseg min_dur_s: a finite number >= 0 (seconds; 0: no minimum duration)')
    return max(1, int(np.floor(s * float(rate)))) if s > 0.0 else 0


def _reseg_passes(reseg):
    n = reseg.get('passes', 1)
    try:
        whole = not isinstance(n, bool) and int(n) == n
    except (TypeError, ValueError, OverflowError):
        whole = False
    if not whole or n < 1:
        raise ValueError('reseg passes: an integer >= 1')
    return int(n)


def _reseg_confidence(reseg, detail):
    """(confidence asked for, conf_scale) of a `reseg` dictionary; `detail` is where the confidences go."""
    on = reseg.get('confidence', False)
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError('reseg confidence: True or False')
    try:
        scale = float(reseg.get('conf_scale', 1.0))
    except (TypeError, ValueError):
        scale = float('nan')
    if not np.isfinite(scale) or scale <= 0.0:
        raise ValueError('reseg conf_scale: a finite number > 0 (an acoustic scale on the path log-weights)')
    if on and not scale * float(reseg['penalty']) <= FB_MAX_SCALED_PENALTY:
        raise ValueError('reseg conf_scale * penalty: at most %g' % FB_MAX_SCALED_PENALTY)
    if on and detail is None:
        raise ValueError('reseg confidence: the confidences come back in detail, which takes a dictionary')
    return bool(on), scale


def _reseg_soft(reseg, model):
    """(soft retraining asked for, soft_scale) of a `reseg` dictionary whose model is `model` (_reseg_model)."""
    on = reseg.get('soft', False)
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError('reseg soft: True or False')
    try:
        scale = float(reseg.get('soft_scale', RESEG_SOFT_SCALE))
    except (TypeError, ValueError):
        scale = float('nan')
    if not np.isfinite(scale) or scale <= 0.0:
        raise ValueError('reseg soft_scale: a finite number > 0 (an acoustic scale on the path log-weights)')
    if on and not scale * float(reseg['penalty']) <= FB_MAX_SCALED_PENALTY:
        raise ValueError('reseg soft_scale * penalty: at most %g' % FB_MAX_SCALED_PENALTY)
    if on and model[0] == 'gmm':
        raise ValueError('reseg soft: the Gaussian speakers only (weighted mixture training is not there), not model gmm')
    return bool(on), scale


def _reseg_tdoa(reseg):
    """None without reseg['tdoa'], else (weight, floor_s, min_frames): the keys of TDOA, its values where one is
    absent."""
    t = reseg.get('tdoa')
    if t is None:
        return None
    if not isinstance(t, dict) or set(t) - set(TDOA):
        raise ValueError('reseg tdoa: a dictionary with keys of TDOA (%s)' % ', '.join(sorted(TDOA)))
    try:
        weight, floor_s = float(t.get('weight', TDOA['weight'])), float(t.get('floor_s', TDOA['floor_s']))
    except (TypeError, ValueError):
        weight = floor_s = float('nan')
    if not np.isfinite(weight) or weight < 0.0:
        raise ValueError('reseg tdoa weight: a finite number >= 0')
    if not np.isfinite(floor_s) or floor_s <= 0.0:
        raise ValueError('reseg tdoa floor_s: a finite number > 0 (seconds)')
    n = t.get('min_frames', TDOA['min_frames'])
    try:
        whole = not isinstance(n, bool) and int(n) == n
    except (TypeError, ValueError, OverflowError):
        whole = False
    if not whole or n < 1 or n > 0x7fffffff:
        raise ValueError('reseg tdoa min_frames: an integer >= 1')
    return weight, floor_s, int(n)


_Options = collections.namedtuple('_Options', 'penalty model min_frames passes confidence conf_scale soft soft_scale tdoa')


def _reseg_options(reseg, rate, detail):
    """A `reseg` dictionary parsed once, each key by its validator: the first ValueError of a dictionary that
    is wrong in several ways is that of the first key in the order penalty, model, min_dur_s, passes,
    confidence, soft, tdoa.  model is _reseg_model's tuple, min_frames the decoder's D (0: the plain decoder)."""
    penalty = _reseg_penalty(reseg)
    model = _reseg_model(reseg)
    min_frames = _reseg_min_frames(reseg, rate)
    passes = _reseg_passes(reseg)
    confidence, conf_scale = _reseg_confidence(reseg, detail)
    soft, soft_scale = _reseg_soft(reseg, model)
    return _Options(penalty, model, min_frames, passes, confidence, conf_scale, soft, soft_scale, _reseg_tdoa(reseg))


def _no_confidence(detail, n_files):
    detail['confidence'] = [np.zeros(0) for _ in range(n_files)]
    detail['log_evidence'] = [np.zeros(0) for _ in range(n_files)]


def _empty_detail(detail, opts, n_files):
    """What `detail` holds when there is nothing to decode (and before the first decode): nobody dropped, no
    pass run, with confidence a list of empty arrays for both of its keys, with soft no retraining."""
    if detail is None:
        return
    detail['dropped'] = []
    detail['passes_run'] = 0
    if opts.confidence:
        _no_confidence(detail, n_files)
    if opts.soft:
        detail['soft_mass'] = []
    if opts.tdoa:
        detail['tdoa_channels'] = [[] for _ in range(n_files)]


def _token_spans(tok_off, offset, turn_begin, turn_end):
    """Token k of turn q opens at turn_begin[q] + offset[k] and ends where the next one opens, a turn's
    last token at turn_end[q].  -> (the turn of every token, begin, end)."""
    n = np.diff(tok_off)
    turn = np.repeat(np.arange(len(n)), n)
    begin = turn_begin[turn] + offset
    end = np.empty_like(begin)
    end[:-1] = begin[1:]
    last = tok_off[1:][n > 0] - 1
    end[last] = turn_end[turn[last]]
    return turn, begin, end


def _token_ranges(tok_off, tok_frame, tok_word, tb, te, first_speaker):
    """The decoded tokens as absolute frame ranges with their speakers, in turn order: token k of turn q
    is [tb[q] + f_k, tb[q] + f_{k+1}), a turn's last token ends at te[q]; its speaker is
    first_speaker[q] + word.  -> (begin, end, speaker)."""
    turn, b, e = _token_spans(tok_off, tok_frame, tb, te)
    return b, e, first_speaker[turn] + tok_word


def _reseg_rows(tok_off, tok_frame, tok_word, turn_start_s, turn_end_s, turn_labels, rate, text_contract):
    """The rows of a decoded batch of turns, in turn order: token k of a turn, opening at the
    relative frame f_k, is [turn_start_s + f_k / rate, turn_start_s + f_{k+1} / rate, label]; a turn's
    first row starts at the turn's own start (f_0 = 0) and its last row ends at the turn's own end
    as the VAD states it (the convention of spkd_gw_lines' tail line).  turn_labels[q][w]: the label
    of word w in turn q.  Returns (rows [n_tokens, 3], the turn of every row)."""
    turn, t0, t1 = _token_spans(tok_off, tok_frame / rate, turn_start_s, turn_end_s)
    times = np.column_stack([t0, t1])
    if text_contract:
        times = hipabi.py2_roundtrip(times.ravel()).reshape(-1, 2)
    return np.column_stack([times, turn_labels[turn, tok_word].astype(np.float64)]), turn


# What is the same for every speaker model of one resegment_batch call: the context and the resident frames,
# the turns to decode as absolute frame ranges [tb, te) with their file's first speaker and speaker count,
# the width of the scores (the largest speaker count), the number of speakers, and clock(key, which), which
# appends the context's last_ms(which) to timings[key].
_Turns = collections.namedtuple('_Turns', 'ctx d_frames total_frames tb te spk_first spk_count n_cols n_spk clock')


class _Speakers(object):
    """The speaker models of a batch on the device.  train(tokens) -> ok per speaker: from the clustering
    segments in pass 1 (tokens is None), from the decoded tokens of the pass before afterwards -- token k of
    turn q is the absolute range [tb_q + f_k, tb_q + f_{k+1}), a turn's last token ends with the turn, its
    speaker is the file's word-th; the ranges go in turn order, grouped by speaker by a stable sort.
    score(ok) -> frame_off: every turn's frames under its file's speakers, into d_scores.  The buffers are
    the context's scratch slots, each asked for where pass 1 first needs it: d_spk (the records), d_models,
    d_scores, and frame_off says what d_scores holds -- the scores of the last score(), which a decode, a
    soft retraining and the confidences then read."""
    loglik_timer = None

    def __init__(self, turns):
        self.turns = turns
        self.d_spk = self.d_models = self.d_scores = self.frame_off = None

    def score(self, ok):
        t = self.turns
        if self.d_scores is None:
            self.d_scores = t.ctx.dev_scratch('reseg_scores', max(int((t.te - t.tb).sum()), 1) * t.n_cols * 4)
        self.frame_off = self._loglik(ok)
        t.clock('reseg_loglik', self.loglik_timer)
        return self.frame_off


class _GaussSpeakers(_Speakers):
    """One full-covariance Gaussian per speaker (spkd_gauss_models) from its statistics record: in pass 1
    the sum of its segments' records (spkd_sum_stats of d_stats, whose n_segments records `member` and
    `set_off` group by speaker: no frame is read), afterwards the records straight from the tokens' frames
    (spkd_set_stats), or from every frame's posteriors (train_soft).  One spkd_gauss_loglik scores the turns.
    A speaker whose record cannot be modelled (fewer than 40 frames, a covariance without positive pivots)
    is not ok."""
    loglik_timer = 'gauss_loglik'

    def __init__(self, turns, d_stats, n_segments, member, set_off):
        _Speakers.__init__(self, turns)
        self.d_stats, self.n_segments, self.member, self.set_off = d_stats, n_segments, member, set_off

    def train(self, tokens):
        t = self.turns
        if tokens is None:
            self.d_spk = t.ctx.dev_scratch('reseg_speaker_stats', t.n_spk * hipabi.REC * 8)
            t.ctx.sum_stats(self.d_stats, self.n_segments, self.member, self.set_off, self.d_spk)
            self.d_models = t.ctx.dev_scratch('reseg_models', t.n_spk * hipabi.GAUSS_MODEL * 8)
        else:
            rb, re_, spk = _token_ranges(*tokens, t.tb, t.te, t.spk_first)
            order = np.argsort(spk, kind='stable')                     # (spkd_set_stats takes ascending sets)
            t.ctx.set_stats(t.d_frames, t.total_frames, rb[order], re_[order], sets=spk[order].astype(np.int32),
                            n_sets=t.n_spk, d_stats=self.d_spk)
        return self._models()

    def train_soft(self, penalty, soft_scale, detail):
        """Baum-Welch retraining (reseg['soft']): the next speakers are trained on posteriors instead of
        tokens: one spkd_fb_posterior_batch on the scores of the pass before (d_scores, frame_off: no
        tokens, every turn's speaker count, the penalty, the acoustic scale soft_scale) writes every
        frame's posteriors, one spkd_post_stats turns them and the frames into the speakers' records --
        every speaker takes every frame of its file's turns, weighted by its posterior there -- and
        spkd_gauss_models follows as in train.  Under min_dur_s the posterior is that of the plain loop,
        as for the confidences.  detail['soft_mass'] gains the float64 array [speakers] of the records'
        count entries, each speaker's expected number of frames: a speaker that is bleeding away shows
        there; without a detail dictionary nobody reads them and the records stay on the device.  A scale
        that is too small lets a speaker lose its mass and the file collapse (RESEG_SOFT above)."""
        t = self.turns
        d_post = t.ctx.dev_scratch('reseg_post', max(int(self.frame_off[-1]), 1) * t.n_cols * 4)
        t.ctx.fb_posterior_batch(self.d_scores, self.frame_off, t.n_cols, penalty, seq_n_cols=t.spk_count,
                                 scale=soft_scale, d_post=d_post)
        t.clock('reseg_soft_posterior', 'fb_posterior')
        mass = t.ctx.post_stats(t.d_frames, t.total_frames, d_post, t.tb, t.te, t.spk_first, t.spk_count, t.n_cols,
                                t.n_spk, self.d_spk, masses=detail is not None)
        t.clock('reseg_soft_stats', 'post_stats')
        if detail is not None:
            detail['soft_mass'].append(np.asarray(mass, dtype=np.float64))
        return self._models()

    def _models(self):
        ok = self.turns.ctx.gauss_models(self.d_spk, self.turns.n_spk, self.d_models)
        self.turns.clock('reseg_models', 'gauss_models')
        return ok

    def _loglik(self, ok):
        t = self.turns
        return t.ctx.gauss_loglik(t.d_frames, t.total_frames, self.d_models, ok, t.tb, t.te, t.spk_first, t.spk_count,
                                  t.n_cols, self.d_scores)


class _GmmSpeakers(_Speakers):
    """reseg['model'] = 'gmm' (RESEG_GMM): every speaker is a diagonal-covariance mixture of
    reseg['components'] Gaussians instead, trained on the device by reseg['iterations'] EM steps from
    a segmental start (spkd_gmm_train; variances floored at reseg['var_floor'] times the variance of
    all the speaker's frames) on the frame ranges of its segments, in segment order (set_off, seg_begin,
    seg_end: the ranges segment_stats summed, grouped by speaker); the segment records are not read.  After
    pass 1: spkd_gmm_train on the tokens' ranges with the same components, iterations and floor, from a
    fresh segmental start (the segments serve pass 1 only).  The turns are scored by spkd_gmm_loglik_seq
    and decoded by the same call as the Gaussian speakers'.  A speaker of fewer than 40 frames a component,
    or of constant or non-finite frames, is not ok.  detail['loglik']: per speaker (link_speakers' order)
    the log-likelihood of its frames under the model entering each iteration, of the last training."""
    loglik_timer = 'gmm_seq_loglik'

    def __init__(self, turns, model, set_off, seg_begin, seg_end, detail):
        _Speakers.__init__(self, turns)
        _, self.n_comp, self.n_iter, self.var_floor = model
        self.set_off, self.seg_begin, self.seg_end, self.detail = set_off, seg_begin, seg_end, detail

    def train(self, tokens):
        t = self.turns
        if tokens is None:
            self.d_models = t.ctx.dev_scratch('reseg_gmm', t.n_spk * self.n_comp * hipabi.GMM_COMP * 8)
            off, rb, re_ = self.set_off, self.seg_begin, self.seg_end
        else:
            # (spkd_gmm_train takes no empty set: a speaker without a token gets one empty range)
            rb, re_, spk = _token_ranges(*tokens, t.tb, t.te, t.spk_first)
            idle = np.nonzero(np.bincount(spk, minlength=t.n_spk) == 0)[0]
            rb, re_ = np.concatenate([rb, np.zeros(len(idle), np.int64)]), np.concatenate([re_, np.zeros(len(idle), np.int64)])
            spk = np.concatenate([spk, idle])
            order = np.argsort(spk, kind='stable')
            off = np.concatenate([[0], np.cumsum(np.bincount(spk, minlength=t.n_spk))]).astype(np.int64)
            rb, re_ = rb[order], re_[order]
        ok, loglik = t.ctx.gmm_train(t.d_frames, t.total_frames, off, rb, re_, self.n_comp, self.n_iter, self.var_floor,
                                     self.d_models)
        t.clock('reseg_gmm_train', 'gmm_train')
        if self.detail is not None:
            self.detail['loglik'] = loglik
        return ok

    def _loglik(self, ok):
        t = self.turns
        return t.ctx.gmm_loglik_seq(t.d_frames, t.total_frames, self.d_models, self.n_comp, ok, t.tb, t.te, t.spk_first,
                                    t.spk_count, t.n_cols, self.d_scores)


def _check_delays(delays, opts, files, rate, segments):
    """reseg['tdoa'] takes a stream of the batch's files on the batch's frame clock, and the clustering segments."""
    if delays is None:
        raise ValueError('reseg tdoa: it reads the delays the beamformer tracked, delays=<frontend.DelayStream>')
    if delays.n_files != len(files):
        raise ValueError('delays: a stream of %d files, a batch of %d' % (delays.n_files, len(files)))
    if float(delays.rate_out) != float(rate) * delays.hop:
        raise ValueError('delays: the stream steps %d samples a frame at %d Hz, the batch has %g frames a second'
                         % (delays.hop, delays.rate_out, rate))
    if segments is None:
        raise ValueError('reseg tdoa trains on the frames of the clustering segments: it takes segments, the arrays '
                         'cluster_batch took')


class _DelayModels(object):
    """The second stream of reseg['tdoa'] (RESEG_TDOA): per (speaker, channel) the exact moments of the delays of the
    speaker's frames (spkd_tdoa_stats), one Gaussian from them (spkd_tdoa_models), and weight times their
    log-likelihood added to the scores the acoustic models left (spkd_tdoa_score), which every decoder, the
    confidences and the soft retraining then read.  train(tokens, ok): in pass 1 on the clustering segments' frame
    ranges, afterwards on the decoded tokens' ranges -- also under soft=True: the soft retraining reads the fused
    scores, the delay models stay hard-trained.  A channel is used in a file only when every speaker of the file
    whose acoustic model is ok has min_frames reliable frames on it (live)."""

    def __init__(self, turns, delays, tdoa, files, owner, spk_file, set_off, seg_b, seg_e):
        self.turns, self.owner, self.spk_file = turns, owner.astype(np.int32), spk_file.astype(np.int32)
        self.weight, self.floor_s, self.min_frames = tdoa
        self.stream = delays.handle([f.frame_off for f in files])
        self.seg = (seg_b, seg_e, np.repeat(np.arange(turns.n_spk), np.diff(set_off)))
        self.d_stats = turns.ctx.dev_scratch('reseg_tdoa_stats', max(turns.n_spk, 1) * hipabi.TDOA_MAX_CH * 3 * 8)
        self.d_models = turns.ctx.dev_scratch('reseg_tdoa_models', max(turns.n_spk, 1) * hipabi.TDOA_MAX_CH * hipabi.TDOA_MODEL * 8)
        self.live = None

    def train(self, tokens, ok):
        t = self.turns
        if tokens is None:
            rb, re_, spk = self.seg
        else:
            rb, re_, spk = _token_ranges(*tokens, t.tb, t.te, t.spk_first)
            order = np.argsort(spk, kind='stable')
            rb, re_, spk = rb[order], re_[order], spk[order]
        t.ctx.tdoa_stats(self.stream, rb, re_, self.spk_file[spk], spk, t.n_spk, self.d_stats)
        t.clock('reseg_tdoa_stats', 'tdoa_stats')
        self.live = t.ctx.tdoa_models(self.d_stats, self.spk_file, ok, self.stream[2], self.min_frames, self.floor_s,
                                      self.d_models)
        t.clock('reseg_tdoa_models', 'tdoa_models')

    def score(self, speakers):
        t = self.turns
        t.ctx.tdoa_score(self.stream, self.d_models, t.n_spk, self.live, t.tb, t.te, self.owner, t.spk_first, t.spk_count,
                         t.n_cols, self.weight, speakers.d_scores)
        t.clock('reseg_tdoa_score', 'tdoa_score')

    def channels(self, n_files):
        return [[c for c in range(hipabi.TDOA_MAX_CH) if (int(self.live[f]) >> c) & 1] for f in range(n_files)]


def _decode(speakers, penalty, min_frames):
    """The best speaker sequence of every turn on the scores `speakers` holds -> (tok_off, tok_frame,
    tok_word).  One spkd_vad_viterbi_batch with the penalty taken off at every switch (stay = exit = 0,
    enter = -penalty; staying wins ties, so consecutive rows of a turn differ in speaker).  min_frames > 0
    (reseg['min_dur_s'], RESEG_MD): the turns are decoded by spkd_mindur_viterbi_batch instead, on the same
    scores, with D = max(1, floor(min_dur_s * rate)) frames: every row lasts at least D frames or is a whole
    turn.  timings: reseg_viterbi and reseg_backtrack are the kernels of the decoder that ran."""
    t = speakers.turns
    if min_frames:
        decoded = t.ctx.mindur_viterbi_batch(speakers.d_scores, speakers.frame_off, t.n_cols, penalty, min_frames)
    else:
        zero = np.zeros(t.n_cols)
        decoded = t.ctx.vad_viterbi_batch(speakers.d_scores, speakers.frame_off, t.n_cols, np.arange(t.n_cols), zero, zero,
                                          zero - penalty)
    t.clock('reseg_viterbi', 'mindur_viterbi' if min_frames else 'vad_viterbi')
    t.clock('reseg_backtrack', 'mindur_backtrack' if min_frames else 'vad_backtrack')
    return decoded[:3]


def _confidences(speakers, tokens, penalty, conf_scale):
    """reseg['confidence'] (RESEG_CONF; either model, either decoder, any passes): after the last decode one
    spkd_fb_posterior_batch runs on the last pass's scores with the final tokens, every turn's speaker
    count and the penalty, at the acoustic scale conf_scale -> (the mean posterior of every token's speaker
    over the token's frames -- a row is a token: they come back in row order -- and every turn's
    log-evidence, -inf for a turn without frames).  The posterior is that of the plain switch-penalty loop
    also under min_dur_s: the minimum duration shapes the rows, not the distribution they are weighed in."""
    t = speakers.turns
    conf, logz = t.ctx.fb_posterior_batch(speakers.d_scores, speakers.frame_off, t.n_cols, penalty, tokens=tokens,
                                          seq_n_cols=t.spk_count, scale=conf_scale)
    t.clock('reseg_posterior', 'fb_posterior')
    return conf, logz


def _speaker_segments(files, segments, seg_off, rate):
    """The frame ranges of the clustering segments the mixtures train on in pass 1 -> (begin, end), one per
    label, file by file: the ranges segment_stats summed (_segment_ranges)."""
    if segments is None:
        raise ValueError('reseg model gmm trains on the frames: it takes segments, the arrays cluster_batch took')
    if len(segments) != len(files):
        raise ValueError('one segment array per file')
    seg_off_s, _, seg_b, seg_e = _segment_ranges(files, segments, rate)
    if seg_off_s.tolist() != np.asarray(seg_off, dtype=np.int64).tolist():
        raise ValueError('segments: one per label, file by file')
    return seg_b, seg_e


def resegment_batch(ctx, d_frames, total_frames, files, d_stats, seg_off, labels, rate=125.0, reseg=RESEG,
                    text_contract=True, timings=None, detail=None, segments=None, delays=None):
    """Viterbi resegmentation of a clustered batch on the device: the closing pass of a BIC
    segmentation + agglomerative clustering system (the reference has none).  d_stats, seg_off,
    labels: the segment records, the files' offsets and the per-file labels of a cluster_batch
    (its stats_out and results).  The speakers are link_speakers' -- file by file, by ascending
    label -- their records the sums of their segments' (spkd_sum_stats), their models one
    full-covariance Gaussian each (spkd_gauss_models).  Every VAD turn (_turn_table) of a file with
    speakers is one sequence: one spkd_gauss_loglik scores all its frames under the file's speakers,
    one spkd_vad_viterbi_batch decodes the best speaker sequence with reseg['penalty'] taken off at
    every switch (_decode).  Returns per file the rows [start_s, end_s, label] that tile its turns
    (_reseg_rows; times through the 12-digit round trip with text_contract), label the file's own
    cluster label; a file with no segments or no turns gives np.zeros((0, 3)), a turn with no
    frames no rows.
    A speaker whose record cannot be modelled (fewer than 40 frames, a covariance without positive
    pivots) scores -inf and is never chosen; when that is every speaker of a turn the decoder's
    all--inf rule applies and the file's lowest label takes the turn.  detail: a dict; receives
    dropped = [(file, label)] of those speakers.  More than 16 speakers in one file, a negative or
    non-finite penalty: ValueError before any device work.  timings: reseg_models, reseg_loglik,
    reseg_viterbi, reseg_backtrack (kernel ms).
    reseg['model'] = 'gmm' (RESEG_GMM): mixture speakers (_GmmSpeakers).  segments: per file the
    (start_s, end_s) arrays cluster_batch took; d_stats is not read.  A speaker that cannot be trained is
    dropped as above.  detail['loglik'] as there.  timings: reseg_gmm_train instead of reseg_models;
    reseg_loglik is the mixture scorer's.  An unknown model, components outside 1 .. 8, negative iterations,
    a negative or non-finite floor, no segments: ValueError before any device work.
    reseg['min_dur_s'] > 0 (RESEG_MD): a minimum speaker duration in the decoder (_decode).  Absent or 0:
    the call above, unchanged.  timings: reseg_viterbi and reseg_backtrack are then that decoder's kernels.
    reseg['passes'] = N (an integer >= 1, default 1; either model, with or without min_dur_s): after
    every decode but the last the speakers are trained again, on the decoded tokens (_Speakers).  Then the
    turns are scored and decoded as in pass 1.  A speaker that holds no frame any more, or whose new model
    is not ok, scores -inf from then on; detail['dropped'] (and detail['loglik']) are those of the last
    pass run.  The loop stops early when a pass decodes exactly the tokens of the pass before it;
    detail['passes_run'] is the number of decodes done (0 when there was nothing to decode).  timings: the
    reseg lists get one entry per pass.  A min_dur_s that is negative or not finite, passes that is not an
    integer >= 1: ValueError before any device work.
    reseg['confidence'] = True (RESEG_CONF; either model, either decoder, any passes): one posterior call
    behind the last decode, at the acoustic scale reseg['conf_scale'] (default 1.0; _confidences).  The
    rows are those of the call without it, to the byte.  detail['confidence']: per file a float64
    array aligned with the file's rows, the mean posterior of the row's speaker over the row's frames;
    detail['log_evidence']: per file the log-evidence of each of its decoded turns, in turn order (-inf
    for a turn without frames).  Both are lists of empty arrays when there is nothing to decode.
    timings: reseg_posterior.  A confidence that is not a bool, a conf_scale that is not a finite number
    > 0, conf_scale * penalty above 600, confidence without a detail dictionary: ValueError before any
    device work.
    reseg['soft'] = True (RESEG_SOFT; Gaussian speakers, either decoder, any passes): Baum-Welch
    retraining (_GaussSpeakers.train_soft).  Pass 1 is unchanged.  After every decode that is neither the
    last nor a repeat of the one before, the next speakers are trained on posteriors instead of tokens, at
    the acoustic scale reseg['soft_scale'] (default 0.1).  The early stop and passes_run keep their meaning;
    confidence=True still runs its own final call at conf_scale.  detail['soft_mass']: per retraining the
    float64 array [speakers] (link_speakers' order) of each speaker's expected number of frames.  timings:
    reseg_soft_posterior and reseg_soft_stats, one entry per retraining.  The default scale comes from the
    synthetic generator only and is unmeasured on speech.  Without soft, or with soft=False, the calls and
    the rows are those described above, to the byte.  A soft that is not a bool, a soft_scale that is not a
    finite number > 0, soft_scale * penalty above 600, soft with model gmm: ValueError before any device
    work.
    reseg['tdoa'] = a dictionary like TDOA (RESEG_TDOA; either model, either decoder, any passes, confidence
    and soft), with delays=<frontend.DelayStream> of the same files on the same frame clock, and segments: in
    every pass, after the speakers are trained, the delay models are (_DelayModels: spkd_tdoa_stats,
    spkd_tdoa_models), and after the turns are scored, weight times the delay log-likelihood is added to the
    scores (spkd_tdoa_score).  The delay models train on the clustering segments' frame ranges in pass 1 and on
    the decoded tokens' ranges afterwards, under soft=True too: soft retraining reads the fused scores, the
    delay models stay hard-trained.  detail['tdoa_channels']: per file the channels used in the last pass (none
    for a one-channel file).  timings: reseg_tdoa_stats, reseg_tdoa_models, reseg_tdoa_score, one entry per
    pass.  Without tdoa the calls and the rows are those described above, to the byte; delays is then not
    looked at.  tdoa without delays, a stream of another file count or frame clock, no segments, unknown keys,
    a weight that is not finite and >= 0, a floor_s that is not finite and > 0, min_frames < 1: ValueError
    before any device work.  The defaults rest on synthetic fixtures and are unmeasured on speech."""
    rate = float(rate)
    opts = _reseg_options(reseg, rate, detail)
    if opts.tdoa:
        _check_delays(delays, opts, files, rate, segments)
    if opts.model[0] == 'gmm' or opts.tdoa:
        seg_b, seg_e = _speaker_segments(files, segments, seg_off, rate)
    member, set_off, spk_file, spk_label = link_speakers(seg_off, labels)
    n_files = len(files)
    if len(labels) != n_files:
        raise ValueError('one label array per file')
    n_spk_file = np.bincount(spk_file, minlength=n_files).astype(np.int64)
    if n_files and int(n_spk_file.max()) > RESEG_MAX_SPEAKERS:
        raise ValueError('resegmentation decodes at most %d speakers a file: file %d has %d'
                         % (RESEG_MAX_SPEAKERS, int(n_spk_file.argmax()), int(n_spk_file.max())))
    out = [np.zeros((0, 3)) for _ in files]
    _empty_detail(detail, opts, n_files)
    table = _turn_table(files, rate)
    if table is None or len(spk_file) == 0:
        return out
    owner, _, _, ls, le, tb, te = table
    keep = n_spk_file[owner] > 0
    owner, ls, le, tb, te = owner[keep], ls[keep], le[keep], tb[keep], te[keep]
    if len(owner) == 0:
        return out
    n_spk, n_cols = len(spk_file), int(n_spk_file.max())
    spk_base = np.zeros(n_files + 1, dtype=np.int64)
    spk_base[1:] = np.cumsum(n_spk_file)

    def clock(key, which):
        if timings is not None:
            timings.setdefault(key, []).append(ctx.last_ms(which))

    turns = _Turns(ctx, d_frames, total_frames, tb, te, spk_base[owner], n_spk_file[owner], n_cols, n_spk, clock)
    if opts.model[0] == 'gmm':
        speakers = _GmmSpeakers(turns, opts.model, set_off, seg_b[member], seg_e[member], detail)
    else:
        speakers = _GaussSpeakers(turns, d_stats, int(seg_off[-1]), member, set_off)
    second = _DelayModels(turns, delays, opts.tdoa, files, owner, spk_file, set_off, seg_b[member], seg_e[member]) \
        if opts.tdoa else None
    tokens = None
    for p in range(opts.passes):
        if opts.soft and tokens is not None:
            ok = speakers.train_soft(opts.penalty, opts.soft_scale, detail)
        else:
            ok = speakers.train(tokens)
        if detail is not None:
            detail['dropped'] = [(int(spk_file[s]), int(spk_label[s])) for s in np.nonzero(ok == 0)[0]]
        if second is not None:
            second.train(tokens, ok)
        speakers.score(ok)
        if second is not None:
            second.score(speakers)
            if detail is not None:
                detail['tdoa_channels'] = second.channels(n_files)
        decoded = _decode(speakers, opts.penalty, opts.min_frames)
        if detail is not None:
            detail['passes_run'] = p + 1
        same = tokens is not None and all(np.array_equal(a, b) for a, b in zip(tokens, decoded))
        tokens = decoded
        if same or len(tokens[1]) == 0:
            break
    # label of word w in a turn of file f: the file's w-th speaker (a word past the file's speakers
    # is never decoded: its column is -inf beside column 0, which wins every tie)
    file_labels = np.zeros((n_files, n_cols), dtype=np.int64)
    file_labels[spk_file, np.arange(n_spk) - spk_base[spk_file]] = spk_label
    rows, turn = _reseg_rows(*tokens, ls, le, file_labels[owner], rate, text_contract)
    bounds = np.searchsorted(owner[turn], np.arange(n_files + 1))
    if opts.confidence:
        conf, logz = _confidences(speakers, tokens, opts.penalty, opts.conf_scale)
        first_turn = np.searchsorted(owner, np.arange(n_files + 1))
        detail['confidence'] = [conf[bounds[i]:bounds[i + 1]] for i in range(n_files)]
        detail['log_evidence'] = [logz[first_turn[i]:first_turn[i + 1]] for i in range(n_files)]
    return [rows[bounds[i]:bounds[i + 1]] for i in range(n_files)]
