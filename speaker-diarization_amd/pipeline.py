"""In-memory batch pipeline: growing-window BIC change detection followed by
agglomerative clustering for MANY files in a handful of device launches, keeping
the semantics of the two-script pipeline spk-diarization2.py runs
(spk-diarization2.py:122-128), including the 12-significant-digit text contract
between the two stages: every boundary the change detector emits
is formatted like the recipe writer would and re-parsed like the clustering
script would, so segment frame ranges are the ones the file-based path gets.

All files of a batch live in one resident frame array [sum T, 39]; turns and
segments are absolute frame ranges into it.  One k_gw launch covers every turn of
every file, one k_chunk_stats/k_reduce_sets pair every segment, one
k_cluster_prep/k_matrix/k_ahc triple every file (a clustering problem each).
"""
import time

import numpy as np

from . import exp_generator, frontend, hipabi, voice_detection
from . import linking as _linking
from . import overlap as _overlap
from . import resegmentation as _resegmentation
from . import seats as _seats
from . import self_vad as _self_vad
from .recipe import py2_float_str
# the linking stage (linking.py, on clr_model.py and gallery.py): its settings and its entry point under their names here
from .linking import LINK_CL, LINK_CLR, LINK_CLR_WARP, _link_model, link_batch, ubm_ranges
# the overlap stage behind the rows (overlap.py): its settings and its entry points under their names here
from .overlap import OVERLAP, overlap_batch, second_rows
# the resegmentation stage (resegmentation.py): its settings and its entry point under their names here
from .resegmentation import (FB_MAX_SCALED_PENALTY, RESEG, RESEG_CONF, RESEG_GMM, RESEG_MAX_SPEAKERS, RESEG_MD,
                             RESEG_SOFT, RESEG_SOFT_SCALE, RESEG_TDOA, TDOA, resegment_batch)
# the seat stages behind change detection and clustering (seats.py): their settings and entry points under their names here
from .seats import SEATS, seat_cut_batch, seat_split_batch
# the self-trained speech / non-speech detector (self_vad.py): its settings under their name here
from .self_vad import SELF_VAD
# the tables every stage reads (tables.py), under their names here
from .tables import BatchFile, _ahc_params, _segment_ranges, _turn_table, link_speakers

DIA2_CD = dict(kind='BIC', lambdac=1.0, threshold=0.0, winsize_s=1.0, winstep_s=3.0, deltaws_s=0.1)
DIA2_CL = dict(variant=1, kind='BIC', lambdac=1.3, threshold=0.0, max_spk=0)
# the change-detection script's own defaults: -m sw -d GLR -w 5.0 -st 0.5 (spk-change-detection.py:499-532)
SW_CD = dict(method='sw', kind='GLR', lambdac=1.3, threshold=0.0, winsize_s=5.0, winstep_s=0.5, deltaws_s=0.05)
# the same script in merge mode, -m m: its second pass, over a detector's output (the window flags are unused there)
MERGE_CD = dict(method='m', kind='GLR', lambdac=1.3, threshold=0.0, winsize_s=5.0, winstep_s=0.5, deltaws_s=0.05)


class FusedStats(object):
    """What the fused change detector leaves for the clustering stage: per recipe line
    (same order as the concatenated per-file segment lists) the record index of its
    statistics in the device buffer and the absolute frame range those statistics
    cover."""

    def __init__(self, d_buf, n_buf, index, begin, end):
        self.d_buf, self.n_buf, self.index, self.begin, self.end = d_buf, n_buf, index, begin, end


_ABSENT = object()                      # a keyword of vad_batch that the caller did not write


def vad_batch(ctx, model, pcms, opt=None, text_contract=True, timings=None, uploaded=None, cfg=_ABSENT, features=_ABSENT,
              detail=None):
    """Speech / non-speech turns of a batch of files from their int16 samples, decided on the
    device (exp_generator.decode_batch: front-end, scores, border shift and decoding without the
    scores leaving it), then the turn state machine of voice-detection2.py over each file's tokens.
    One list of (start_s, end_s) per file, ready for BatchFile(..., vad=...).  With text_contract
    the times are the ones the change detector reads back from the recipe the file path writes
    (py2_str, 12 significant digits: spkd_py2_roundtrip).  uploaded: the samples already on the
    device (frontend.upload_batch), as decode_batch takes them.
    model: a VadModel, or a dictionary like SELF_VAD: then no model file is needed, the detector is
    trained on each recording itself (self_vad.decode_batch) over the features of cfg, the diarization
    feature configuration, which is required; features = (d_frames, total_frames, frame_off) are
    those features when the caller has them (features_batch computes them otherwise); detail, a dict,
    receives vad_untrained and vad_passes_run; opt's rate must be cfg.frame_rate (the default when
    opt is None).  A file too short or too even to train on has no turns.  With a VadModel cfg and
    features must be absent."""
    self_trained = isinstance(model, dict)
    if not self_trained and (cfg is not _ABSENT or features is not _ABSENT):
        raise ValueError('cfg and features go with a dictionary like SELF_VAD, not with a VadModel')
    if self_trained:
        cfg = None if cfg is _ABSENT else cfg
        features = None if features is _ABSENT else features
        if cfg is None:
            raise ValueError('the self-trained detector works on the features of cfg: cfg is required')
        _self_vad._options(model)                   # (its refusals come before any device work)
        opt = opt or voice_detection.VadOptions(rate=cfg.frame_rate)
        if float(opt.rate) != float(cfg.frame_rate):
            raise ValueError('the turns are counted at %g frames a second, the features at %g' % (opt.rate, cfg.frame_rate))
    opt = opt or voice_detection.VadOptions()
    _t0 = time.perf_counter()
    if self_trained:
        if uploaded is None:
            uploaded = frontend.upload_batch(ctx, pcms, timings)
        if features is None:
            features = features_batch(ctx, cfg, uploaded=uploaded, timings=timings)
        tokens, last_frames = _self_vad.decode_batch(ctx, model, cfg, uploaded[0], uploaded[1], features[0], features[2],
                                                     timings, detail)
    else:
        tokens, last_frames = exp_generator.decode_batch(ctx, model, pcms, timings, uploaded)
    _t1 = time.perf_counter()
    out = []
    for toks, last in zip(tokens, last_frames):
        turns = voice_detection.turns_from_tokens(((str(t), w) for t, w in toks), 'a', opt, lambda: str(last))
        times = np.array([(s, e) for _, s, e in turns], dtype=np.float64).reshape(-1, 2)
        if text_contract:
            times = hipabi.py2_roundtrip(times.ravel()).reshape(-1, 2)
        out.append([(float(s), float(e)) for s, e in times])
    if timings is not None:
        timings.setdefault('wall_vad_decode', []).append(1e3 * (_t1 - _t0))
        timings.setdefault('wall_vad_turns', []).append(1e3 * (time.perf_counter() - _t1))
    return out


def features_batch(ctx, cfg, pcms=None, uploaded=None, timings=None):
    """The resident frame array of a batch from its files' int16 samples (or from `uploaded`, the
    pair of a frontend.upload_batch): (d_frames, total_frames, frame_off), file f at the frames
    [frame_off[f], frame_off[f+1]).  The buffer is the context's and lives until its next batch of
    this window width."""
    if uploaded is None:
        uploaded = frontend.upload_batch(ctx, pcms, timings)
    d_frames, frame_off = frontend.extract_batch(ctx, cfg, uploaded[0], uploaded[1], timings=timings)
    return d_frames, int(frame_off[-1]), frame_off


def _one_clock(model, cfg):
    """The VAD chain and the diarization features read the same samples on one frame clock."""
    if model.cfg.sample_rate != cfg.sample_rate:
        raise ValueError('the VAD model wants %d Hz, the feature configuration %d Hz' % (model.cfg.sample_rate, cfg.sample_rate))
    if model.cfg.hop != cfg.hop:
        raise ValueError('the VAD model steps %d samples a frame, the feature configuration %d: one frame '
                         'clock for the turns and the features' % (model.cfg.hop, cfg.hop))


def diarize_pcm_batch(ctx, model, cfg, pcms, cd=DIA2_CD, cl=DIA2_CL, timings=None, uploaded=None, **kw):
    """From samples to speakers for a batch of files: one upload of the int16 samples, the VAD
    chain (vad_batch with the model's own feature configuration) and the diarization features
    (features_batch with cfg, the fconfig.cfg chain) both from it, then diarize_batch with the
    turns and the frames as they lie on the device.  uploaded: the samples already on the device
    (frontend.upload_batch or frontend.resample_batch; pcms is not read then).  kw: diarize_batch's
    text_contract, fused, handoff, link, reseg, seats, overlap, detail, delays (the frontend.DelayStream of
    reseg['tdoa'], of seats and of overlap).  Returns its rows.
    model: a dictionary like SELF_VAD instead of a VadModel needs no model file: one upload, ONE
    feature chain (cfg's), the self-trained turns on those features (vad_batch), then diarize_batch;
    detail, if given, also receives vad_untrained and vad_passes_run."""
    self_trained = isinstance(model, dict)
    if self_trained:
        _self_vad._options(model)
    else:
        _one_clock(model, cfg)
    if uploaded is None:
        uploaded = frontend.upload_batch(ctx, pcms, timings)
    if self_trained:
        d_frames, total, frame_off = features_batch(ctx, cfg, uploaded=uploaded, timings=timings)
        vad = vad_batch(ctx, model, None, text_contract=kw.get('text_contract', True), timings=timings, uploaded=uploaded,
                        cfg=cfg, features=(d_frames, total, frame_off), detail=kw.get('detail'))
    else:
        vad = vad_batch(ctx, model, None, text_contract=kw.get('text_contract', True), timings=timings, uploaded=uploaded)
        d_frames, total, frame_off = features_batch(ctx, cfg, uploaded=uploaded, timings=timings)
    files = [BatchFile(frame_off[f], frame_off[f + 1] - frame_off[f], vad[f]) for f in range(len(vad))]
    return diarize_batch(ctx, d_frames, total, files, rate=float(cfg.frame_rate), cd=cd, cl=cl, timings=timings, **kw)


# delay-and-sum beamforming in front of the resampler (frontend.BEAMFORM has the words on its defaults:
# min_peak, jump_penalty and jump_cap are unmeasured on speech)
BEAMFORM = frontend.BEAMFORM


def diarize_audio_batch(ctx, model, cfg, audios, cd=DIA2_CD, cl=DIA2_CL, timings=None, group_bytes=None, beamform=None,
                        delays=None, **kw):
    """From recordings to speakers: audios = [(samples, rate)], int16 [n] or [n, channels] at any
    rate (frontend.read_audio), resampled and downmixed to cfg.sample_rate on the device
    (frontend.resample_batch; group_bytes: its bound on the raw audio held there), then exactly
    diarize_pcm_batch from its upload on (model: a VadModel, or a dictionary like SELF_VAD).
    beamform: None (the channels are averaged), or a dictionary like BEAMFORM (they are aligned by
    GCC-PHAT delays and summed: frontend.resample_batch).  reseg=dict(..., tdoa=...) with beamform: the
    delays the beamformer tracks are kept (a frontend.DelayStream on cfg's frame clock, made here unless
    delays= hands one in) and the resegmentation stage reads them as a second stream (resegment_batch);
    tdoa without beamform is a ValueError.  seats=<a dictionary like SEATS> with beamform takes the same stream (one
    serves both) to the seat stages of diarize_batch; seats without beamform is a ValueError.  overlap=<a dictionary
    like OVERLAP> with beamform: the stream is made with second=True and the dictionary's min_second and guard, so it
    also keeps the runner-up lags (one stream serves tdoa, seats and overlap), and diarize_batch runs the overlap stage
    on its rows; overlap without beamform, or with a stream handed in that keeps no runner-ups, is a ValueError.
    Returns its rows."""
    if isinstance(model, dict):
        _self_vad._options(model)
    else:
        _one_clock(model, cfg)
    group = {} if group_bytes is None else {'group_bytes': group_bytes}
    second = {}                                      # what a stream made here is made with
    if kw.get('overlap') is not None:
        o = _overlap._overlap_options(kw['overlap'])
        if beamform is None:
            raise ValueError('overlap: the delays are the beamformer\'s, which takes beamform=')
        if delays is not None and not delays.second:
            raise ValueError('overlap: the stream keeps no runner-ups; make it with frontend.DelayStream(..., second=True)')
        second = dict(second=True, min_second=o.min_second, guard=o.guard)
    tdoa = kw.get('reseg') is not None and _resegmentation._reseg_tdoa(kw['reseg']) is not None
    if tdoa and beamform is None:
        raise ValueError('reseg tdoa: the delays are the beamformer\'s, which takes beamform=')
    if kw.get('seats') is not None:
        _seats._seat_options(kw['seats'], float(cfg.frame_rate))
        if beamform is None:
            raise ValueError('seats: the delays are the beamformer\'s, which takes beamform=')
    if (tdoa or second or kw.get('seats') is not None) and delays is None:     # one stream serves the three
        delays = frontend.DelayStream(ctx, cfg.hop, cfg.window_width, cfg.sample_rate, **second)
    if beamform is not None:
        group['beamform'] = beamform
        if delays is not None:
            group['delays'] = kw['delays'] = delays
    uploaded = frontend.resample_batch(ctx, audios, cfg.sample_rate, timings=timings, **group)
    return diarize_pcm_batch(ctx, model, cfg, None, cd=cd, cl=cl, timings=timings, uploaded=uploaded, **kw)


def _cd_params(cd, rate):
    return hipabi.CdParams(hipabi.KINDS[cd['kind']], 0, cd['lambdac'], cd['threshold'],
                           float(np.floor(cd['winsize_s'] * rate)), float(np.floor(cd['winstep_s'] * rate)),
                           float(np.floor(rate * cd['deltaws_s'])), rate)


def _method(cl):
    """The clustering mode of a `cl` dictionary: 'hi' (spk_cluster_hi, also when the key is
    absent) or 'in' (spk_cluster_in)."""
    m = cl.get('method', 'hi')
    if m not in ('hi', 'in'):
        raise ValueError('cl method: hi or in')
    return m


def _cd_method(cd):
    """The change-detection mode of a `cd` dictionary: 'gw' (dist_gw, also when the key is
    absent), 'sw' (dist_sw) or 'm' (merge_rec)."""
    m = cd.get('method', 'gw')
    if m not in ('gw', 'sw', 'm'):
        raise ValueError('cd method: gw, sw or m')
    return m


def _merge_lines(files, rate):
    """Per line of the batch, in file order, for merge mode: line_off per file, start / end
    seconds, absolute frame range -- ChangeDetectionRun._merge_ranges' truncation and clamps.
    Raises what the script's path raises for a file of one line, and ValueError for lines that
    overlap or go backwards: a merged run is then not the sum of its lines and gaps, and the
    caller takes ChangeDetectionRun."""
    cnt = [len(f.vad) for f in files]
    if 1 in cnt:
        raise AttributeError("'function' object has no attribute 'prev'")
    line_off = np.zeros(len(files) + 1, dtype=np.int64)
    line_off[1:] = np.cumsum(cnt)
    vad = np.concatenate([f.vad_arr for f in files])
    owner = np.repeat(np.arange(len(files)), cnt)
    foff = np.array([f.frame_off for f in files], dtype=np.int64)[owner]
    fn = np.array([f.n_frames for f in files], dtype=np.int64)[owner]
    ls, le = vad[:, 0], vad[:, 1]
    f0 = np.clip((ls * rate).astype(np.int64), 0, fn)
    f1 = np.clip((le * rate).astype(np.int64), 0, fn)
    inside = owner[1:] == owner[:-1]
    if bool((f1 < f0).any()) or bool((inside & (f0[1:] < f1[:-1])).any()):
        raise ValueError('merge mode in a batch takes lines in time order that do not overlap')
    return line_off, ls, le, foff + f0, foff + f1


def _merge_done(ctx, timings, line_off, r):
    """After a merge_batch call (result r), as _detector_done."""
    if timings is not None:
        timings.setdefault('merge', []).append(ctx.last_ms('merge'))
        timings['merge_lines'] = len(r['merged'])
        # a step is the chain's own work when the line before its line had joined a run
        stepped = r['merged'] >= 0
        stepped[line_off[:-1][np.diff(line_off) > 0]] = False          # (a file's first line is no step)
        timings['merge_steps_behind_a_merge'] = int((stepped[1:] & (r['merged'][:-1] == 1)).sum())
    if r['status'] == hipabi.SPKD_ENONFINITE:
        raise ValueError('array must not contain infs or NaNs')


def _sw_done(ctx, timings, tb, te, r):
    """After a sliding-window call (sw_batch result r), as _detector_done."""
    if timings is not None:
        timings.setdefault('sw', []).append(ctx.last_ms('sw'))
        timings['sw_frames'] = int((te - tb).sum())
        timings['sw_windows'] = int(r['d_off'][-1])
    if r['status'] == hipabi.SPKD_ENONFINITE:
        raise ValueError('array must not contain infs or NaNs')


def _detector_done(ctx, timings, tb, te, r):
    """After a growing-window call (gw or gw_batch result r): its timings entries, and the
    reference's error for frames that are not finite."""
    if timings is not None:
        timings.setdefault('gw', []).append(ctx.last_ms('gw'))
        timings.setdefault('gw_stream_ms', []).append(ctx.last_ms('call'))     # uploads + kernel + result copies
        timings['gw_frames'] = int((te - tb).sum())
        timings['gw_windows'] = int(r['n_win'].sum())
        timings['gw_dets'] = ctx.last_gw_items()
    if r['status'] == hipabi.SPKD_ENONFINITE:
        raise ValueError('array must not contain infs or NaNs')


def _time_stats(ctx, timings, n, begin, end):
    """The timings entries of the statistics kernels: n records, those of [begin, end) from the frames."""
    if len(begin):
        timings.setdefault('chunk_stats', []).append(ctx.last_ms('chunk_stats'))
        timings.setdefault('reduce_sets', []).append(ctx.last_ms('reduce_sets'))
    timings['stats_frames'] = int((end - begin).sum())
    timings['stats_sets'] = n
    timings['stats_recomputed'] = len(begin)


def _clustering_done(ctx, timings, seg_off, r):
    """After a clustering call (ahc or ahc_fused result r), as _detector_done."""
    if timings is not None:
        for k in ('cluster_prep', 'matrix', 'ahc'):
            timings.setdefault(k, []).append(ctx.last_ms(k))
        timings['ahc_head'] = ctx.last_ahc_head()     # (above 0: 'matrix' and 'ahc' are spans that overlap)
    if r['status'] == hipabi.SPKD_ENONFINITE:
        raise ValueError('array must not contain infs or NaNs')
    if timings is not None:
        npb = np.diff(seg_off)
        nm = r['n_merges'].astype(np.int64)
        timings['matrix_pairs'] = int((npb * (npb - 1) // 2).sum())
        # merge m of a problem with N records recomputes N - 2 - m distances
        timings['ahc_pairs'] = int((nm * (npb - 2) - nm * (nm - 1) // 2).sum())


def _cluster_in_done(ctx, timings, seg_off, r):
    """After a cluster_in_batch call (result r), as _clustering_done: the chain is the 'ahc' entry."""
    if timings is not None:
        for k in ('cluster_prep', 'ahc'):
            timings.setdefault(k, []).append(ctx.last_ms(k))
    if r['status'] == hipabi.SPKD_ENONFINITE:
        raise ValueError('array must not contain infs or NaNs')
    if timings is not None:
        # a record meets the clusters founded before it: one more than the largest label so far
        pairs = 0
        for o, e in zip(seg_off[:-1].tolist(), seg_off[1:].tolist()):
            if e - o > 1:
                pairs += int((np.maximum.accumulate(r['label'][o:e - 1]).astype(np.int64) + 1).sum())
        timings['cluster_in_pairs'] = pairs


def _problems(cnt):
    """A file without a line is not a clustering problem (spkd_ahc rejects empty ones): the
    indices of the others and their seg_off; the lines of those stay in place."""
    cnt = np.asarray(cnt, dtype=np.int64)
    kept = np.nonzero(cnt)[0]
    seg_off = np.zeros(len(kept) + 1, dtype=np.int64)
    seg_off[1:] = np.cumsum(cnt[kept])
    return kept, seg_off


def _recipe_rows(times, line_file, labels, rate):
    """Rows [start_s, end_s, speaker] in the recipe order of spk_cluster_hi's output: per file,
    sorted by (start*rate, end*rate, line).  The change detector emits a file's lines in time
    order, so the keys are almost always sorted already (a stable sort then changes nothing):
    one O(n) look instead of the sort."""
    k0, k1 = times[:, 0] * rate, times[:, 1] * rate
    in_order = (line_file[1:] != line_file[:-1]) | (k0[1:] > k0[:-1]) | ((k0[1:] == k0[:-1]) & (k1[1:] >= k1[:-1]))
    rows = np.column_stack([times, labels.astype(np.float64)])       # (a copy: the inputs may be views)
    if not bool(in_order.all()):
        rows = rows[np.lexsort((np.arange(len(rows)), k1, k0, line_file))]
    return rows


def change_detect_batch(ctx, d_frames, total_frames, files, rate=125.0, cd=DIA2_CD, timings=None,
                        text_contract=True, fused=None):
    """Returns, per file, the list of (start_s, end_s) the change-detection recipe
    would contain (already passed through the 12-digit text round trip).
    text_contract=False is the opt-in fused mode of SURVEY.md §8(f) row 4: the times go
    to the clustering stage as the doubles they are, without being printed and re-read
    (A-2) -- NOT the reference's semantics: a boundary within 1e-12 relative of a frame
    edge can land one frame away.
    fused: a list; when given, the detector also leaves the statistics record of every
    segment on the device (spkd_gw_fused) and a FusedStats is appended to the list, so that
    cluster_batch does not read the frames a second time.
    cd['method'] = 'm' (MERGE_CD): the script's merge mode (merge_rec), its second pass over a
    detector's output: every file's `vad` list is the recipe lines to merge, every file's chain in
    one call (spkd_merge_batch); the result is the (start_s, end_s) of every run as the script
    writes them.  No fused records.  A file of one line raises the script's AttributeError, a
    file whose lines overlap or go backwards ValueError (ChangeDetectionRun takes those).
    cd['method'] = 'sw': the sliding double window (dist_sw) instead of the growing one, every
    turn of every file in one call (spkd_sw_batch: distances and the positive-run pass on the
    device); no fused records.  kind 'BIC' follows the script there: it raises on
    the first turn that has a window, and writes every turn as one line when none has."""
    method = _cd_method(cd)
    if method == 'sw' and fused is not None:
        raise ValueError('the sliding window leaves no fused records: cd method sw takes fused=None')
    if method == 'm' and fused is not None:
        raise ValueError('merge mode leaves no fused records: cd method m takes fused=None')
    rate = float(rate)
    _t0 = time.perf_counter()
    if method == 'm':
        if sum(len(f.vad) for f in files) == 0:
            return [[] for _ in files]
        line_off, ls, le, lb, lend = _merge_lines(files, rate)
        _t1 = time.perf_counter()
        r = ctx.merge_batch(d_frames, total_frames, line_off, lb, lend, cd['kind'], cd['lambdac'], cd['threshold'])
        _t2 = time.perf_counter()
        _merge_done(ctx, timings, line_off, r)
        # a run: from the start of the line that founds it to the end of the last line that joined; the
        # script writes prev[2] * rate and prev[3] * rate as frames with lna_start 0 (CD:175-176, :392-394)
        first = np.nonzero(r['merged'] == 0)[0]
        last = np.append(first[1:], len(ls)) - 1
        rt = np.column_stack([(ls[first] * rate) / rate + 0.0, (le[last] * rate) / rate + 0.0])
        if text_contract:
            rt = hipabi.py2_roundtrip(rt.ravel()).reshape(-1, 2)
        bounds = np.searchsorted(first, line_off)
        out = [rt[bounds[i]:bounds[i + 1]] for i in range(len(files))]
        if timings is not None:
            _t3 = time.perf_counter()
            timings.setdefault('wall_cd_prepare', []).append(1e3 * (_t1 - _t0))
            timings.setdefault('wall_cd_call', []).append(1e3 * (_t2 - _t1))
            timings.setdefault('wall_cd_finish', []).append(1e3 * (_t3 - _t2))
        return out
    table = _turn_table(files, rate)
    if table is None:
        return [[] for _ in files]
    owner, _, _, ls, le, tb, te = table
    p = _cd_params(cd, rate)
    _t1 = time.perf_counter()
    if method == 'sw':
        if cd['kind'] == 'BIC':
            if bool((2 * p.winsize <= (te - tb)).any()):
                raise ValueError('array must not contain infs or NaNs')
            nt = len(tb)
            off = np.arange(nt + 1, dtype=np.int64)
            nd, ds, dm, fs = np.zeros(nt, dtype=np.int32), np.zeros(nt), np.zeros(nt), np.zeros(nt)
        else:
            r = ctx.sw_batch(d_frames, total_frames, tb, te, p)
            _sw_done(ctx, timings, tb, te, r)
            off, nd, ds, dm, fs = r['off'], r['n_det'], r['det_start'], r['det_maxi'], r['final_start']
        _t2 = time.perf_counter()
        lines = hipabi.gw_lines(off[:-1], nd, ds, dm, fs, ls, le, tb, te, rate, text_contract=text_contract)
        return _lines_per_file(lines, owner, len(files), timings, _t0, _t1, _t2)
    seg_buf = {}

    def seg_alloc(n_rec):
        seg_buf['n'] = n_rec
        seg_buf['p'] = ctx.dev_scratch('fused_segment_stats', max(n_rec, 1) * hipabi.REC * 8)
        return seg_buf['p']

    r = ctx.gw(d_frames, total_frames, tb, te, p, log_cap=4096, tight=True, reuse=True,
               seg_stats=seg_alloc if fused is not None else None)
    _t2 = time.perf_counter()
    _detector_done(ctx, timings, tb, te, r)
    off = r['off']
    # detections per turn = ones among the turn's n_win window flags (what lies behind them
    # in the reused buffers is not looked at)
    nd = hipabi.count_flags(r['win_det'], off[:-1], r['n_win'])
    # recipe order: per turn its detections (detection j of turn t sits at off[t] + j), then the
    # tail line; times as the script computes them, through the 12-digit text round trip
    lines = hipabi.gw_lines(off[:-1], nd, r['det_start'], r['det_maxi'], r['final_start'], ls, le, tb, te, rate,
                            text_contract=text_contract, want_frames=fused is not None)
    if fused is not None:
        # the frames each record covers: [int(start), int(start + maxi)) of the turn for a
        # detection, [int(final start), turn end) for the tail
        fused.append(FusedStats(seg_buf['p'], seg_buf['n'], lines['index'], lines['frame_b'], lines['frame_e']))
    return _lines_per_file(lines, owner, len(files), timings, _t0, _t1, _t2)


def _lines_per_file(lines, owner, n_files, timings, _t0, _t1, _t2):
    """The (start_s, end_s) lists of change_detect_batch from a gw_lines result, and the wall
    times of its three phases."""
    rt, line_turn = lines['times'], lines['turn']
    line_file = owner[line_turn]
    bounds = np.searchsorted(line_file, np.arange(n_files + 1))
    out = [rt[bounds[i]:bounds[i + 1]] for i in range(n_files)]
    if timings is not None:
        _t3 = time.perf_counter()
        timings.setdefault('wall_cd_prepare', []).append(1e3 * (_t1 - _t0))
        timings.setdefault('wall_cd_call', []).append(1e3 * (_t2 - _t1))
        timings.setdefault('wall_cd_finish', []).append(1e3 * (_t3 - _t2))
    return out


def segment_stats(ctx, d_frames, total_frames, files, segments, rate=125.0, timings=None, fused=None,
                  scratch_name='segment_stats'):
    """The statistics record of every segment (get_spk_features + the np.cov inputs,
    spk-clustering.py:46-52, 88-94) -> (device pointer to n records in segment order,
    seg_off per file, n, time stamp after the host preparation).  fused: see cluster_batch."""
    seg_off, n, b, e = _segment_ranges(files, segments, rate)
    d_stats = ctx.dev_scratch(scratch_name, max(n, 1) * hipabi.REC * 8)
    _t1 = time.perf_counter()
    if fused is None:
        ctx.set_stats(d_frames, total_frames, b, e, np.arange(n, dtype=np.int32), n, d_stats)
        redo = np.arange(n)
    else:
        same = (fused.begin == b) & (fused.end == e)
        keep = np.nonzero(same)[0]
        redo = np.nonzero(~same)[0]
        ctx.gather_stats(fused.d_buf, fused.n_buf, fused.index[keep], d_stats, n, keep)
        if len(redo):
            d_tmp = ctx.dev_scratch(scratch_name + '_redo', len(redo) * hipabi.REC * 8)
            ctx.set_stats(d_frames, total_frames, b[redo], e[redo], np.arange(len(redo), dtype=np.int32),
                          len(redo), d_tmp)
            ctx.gather_stats(d_tmp, len(redo), np.arange(len(redo)), d_stats, n, redo)
    if timings is not None:
        _time_stats(ctx, timings, n, b[redo], e[redo])
    return d_stats, seg_off, n, _t1


def cluster_batch(ctx, d_frames, total_frames, files, segments, rate=125.0, cl=DIA2_CL, timings=None,
                  want_merges=False, fused=None, stats_out=None):
    """segments: per file, array [(start_s, end_s)] as the clustering script parses
    them.  Returns per file (labels[int array, 1-based, per segment in input
    order], merges[(a, b, d)]).
    cl['method'] = 'in': spk_cluster_in instead of spk_cluster_hi, every file's chain in one
    launch (spkd_cluster_in_batch); labels are the cluster numbers in the order the clusters
    were founded, merges is None.
    fused: the FusedStats of change_detect_batch for exactly these segments: the records
    of the segments whose frame range (as computed here, from the times) equals the range
    the detector summed are gathered from its buffer; only the others -- a boundary the
    12-digit text round trip moved across a frame edge -- are computed from the frames.
    stats_out: a list; receives (d_stats, seg_off), the segment records as they stay on the device
    (the context's until its next cluster_batch) and their offsets per file of `files`: what
    link_batch takes.  Nothing is appended when no file has a segment."""
    rate = float(rate)
    method = _method(cl)
    want_merges = want_merges and method == 'hi'
    cnt = [len(s) for s in segments]
    keep = _problems(cnt)[0]
    if len(keep) < len(files):               # (the lines of the others keep their order: fused stays valid)
        out = [(np.zeros(0, dtype=np.int32), [] if want_merges else None) for _ in files]
        if len(keep):
            box = None if stats_out is None else []
            sub = cluster_batch(ctx, d_frames, total_frames, [files[i] for i in keep],
                                [segments[i] for i in keep], rate, cl, timings, want_merges, fused, box)
            for i, r in zip(keep, sub):
                out[i] = r
            if box:                              # (the records are in file order: the files left out own none)
                stats_out.append((box[0][0], np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)))
        return out
    _t0 = time.perf_counter()
    d_stats, seg_off, n, _t1 = segment_stats(ctx, d_frames, total_frames, files, segments, rate, timings, fused)
    if stats_out is not None:
        stats_out.append((d_stats, seg_off))
    _t2 = time.perf_counter()
    if method == 'in':
        r = ctx.cluster_in_batch(d_stats, seg_off, cl['kind'], cl['lambdac'], cl['threshold'])
        _t3 = time.perf_counter()
        _cluster_in_done(ctx, timings, seg_off, r)
        all_labels = r['label'] + 1
    else:
        r = ctx.ahc(d_stats, seg_off, _ahc_params(cl))
        _t3 = time.perf_counter()
        _clustering_done(ctx, timings, seg_off, r)
        all_labels = hipabi.labels_from_merges_batch(seg_off, r['n_merges'], r['a'], r['b'])
    out = []
    for fi in range(len(files)):
        o, c = int(seg_off[fi]), cnt[fi]
        merges = None
        if want_merges:
            nm = int(r['n_merges'][fi])
            merges = list(zip(r['a'][o:o + nm].tolist(), r['b'][o:o + nm].tolist(), r['d'][o:o + nm].tolist()))
        out.append((all_labels[o:o + c], merges))
    if timings is not None:
        _t4 = time.perf_counter()
        timings.setdefault('wall_cl_prepare', []).append(1e3 * (_t1 - _t0))
        timings.setdefault('wall_cl_stats_call', []).append(1e3 * (_t2 - _t1))
        timings.setdefault('wall_cl_ahc_call', []).append(1e3 * (_t3 - _t2))
        timings.setdefault('wall_cl_finish', []).append(1e3 * (_t4 - _t3))
    return out


def diarize_batch_device(ctx, d_frames, total_frames, files, rate=125.0, cd=DIA2_CD, cl=DIA2_CL, timings=None,
                         detail=None, first_guess_scale=1.0):
    """diarize_batch(fused=True) with the hand-off between the two stages on the device: the
    detector's results come back as recipe lines (spkd_gw_batch: compacted in recipe order
    behind k_gw, round trip and redo list in one native pass), and the clustering stage reads
    the fused records in place through the line -> record map the compaction left, in one call
    (spkd_ahc_fused: redo statistics, working copies, matrix, merge loop, label replay).  Same
    rows as the host hand-off: the same records go through the same kernels.
    detail: a dict; receives the gw_batch result with its host index map ('lines') and the merge
    log per file with segments ('merges', as cluster_batch's want_merges)."""
    if _cd_method(cd) != 'gw':
        raise ValueError('the device hand-off is the growing window\'s: cd method gw')
    rate = float(rate)
    _t0 = time.perf_counter()
    table = _turn_table(files, rate)
    if table is None:
        return [np.zeros((0, 3)) for _ in files]
    owner, foff, fn, ls, le, tb, te = table
    ls, le = np.ascontiguousarray(ls), np.ascontiguousarray(le)
    p = _cd_params(cd, rate)
    _t1 = time.perf_counter()
    r = ctx.gw_batch(d_frames, total_frames, tb, te, p, ls, le, foff, fn,
                     lambda n_rec: ctx.dev_scratch('fused_segment_stats', max(n_rec, 1) * hipabi.REC * 8),
                     tight=True, first_guess_scale=first_guess_scale, want_index=detail is not None)
    _t2 = time.perf_counter()
    _detector_done(ctx, timings, tb, te, r)
    line_file = owner[r['turn']]
    bounds = np.searchsorted(line_file, np.arange(len(files) + 1))
    _t3 = time.perf_counter()
    seg_off = _problems(np.diff(bounds))[1]
    ap = _ahc_params(cl)
    _t4 = time.perf_counter()
    a = ctx.ahc_fused(d_frames, total_frames, r['d_seg'], r['n_ev'], r['d_index'], seg_off, r['redo_line'],
                      r['redo_begin'], r['redo_end'], ap)
    _t5 = time.perf_counter()
    if timings is not None:
        _time_stats(ctx, timings, r['n_lines'], r['redo_begin'], r['redo_end'])
    _clustering_done(ctx, timings, seg_off, a)
    if detail is not None:
        detail['lines'] = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in r.items()}
        detail['merges'] = [list(zip(a['a'][o:o + m].tolist(), a['b'][o:o + m].tolist(), a['d'][o:o + m].tolist()))
                            for o, m in zip(seg_off[:-1].tolist(), a['n_merges'].tolist())]
    rows = _recipe_rows(r['times'], line_file, a['labels'], rate)
    out = [rows[bounds[i]:bounds[i + 1]] for i in range(len(files))]
    if timings is not None:
        _t6 = time.perf_counter()
        timings.setdefault('wall_cd_prepare', []).append(1e3 * (_t1 - _t0))
        timings.setdefault('wall_cd_call', []).append(1e3 * (_t2 - _t1))
        timings.setdefault('wall_cd_finish', []).append(1e3 * (_t3 - _t2))
        timings.setdefault('wall_cl_prepare', []).append(1e3 * (_t4 - _t3))
        timings.setdefault('wall_cl_stats_call', []).append(0.0)      # (the redo statistics are part of the one call)
        timings.setdefault('wall_cl_ahc_call', []).append(1e3 * (_t5 - _t4))
        timings.setdefault('wall_cl_finish', []).append(1e3 * (_t6 - _t5))
    return out


def diarize_batch(ctx, d_frames, total_frames, files, rate=125.0, cd=DIA2_CD, cl=DIA2_CL, timings=None,
                  text_contract=True, fused=False, handoff=None, link=None, detail=None, reseg=None, delays=None, seats=None,
                  overlap=None):
    """CD (gw/BIC) + CL (hi/BIC) for a batch; returns per file an array of rows
    [start_s, end_s, speaker] in recipe order.
    cl['method'] = 'in' clusters with spk_cluster_in (cluster_batch): host hand-off only; the
    rows stay in input order (the script writes each line as it is decided) with the times it
    writes -- the input's, but from a file's second line on under variant 1, which casts:
    int(t * rate) / rate (clustering._cluster_in_chain).
    cd['method'] = 'sw' detects with the sliding window (change_detect_batch): host hand-off
    only, not fused; either clustering method.  cd['method'] = 'm' merges the files' lines
    instead of detecting (change_detect_batch), under the same two rules.
    fused=True: the frames are read once -- the change detector leaves every segment's
    statistics record for the clustering stage (segments and labels are those of the
    two-pass form; a record differs from the two-pass one only in the order of its
    floating-point sums).
    handoff: 'device' (the default of fused=True with the text contract: diarize_batch_device)
    or 'host' (the event arrays come to the host, which builds the lines and gathers the
    records: the only form of the two-pass and text_contract=False modes).
    link: a dictionary like LINK_CL; the speakers of the files are then linked across the batch
    (link_batch) and the rows' third column holds the global speakers -- segments, times and
    order are those of link=None.  Host hand-off only.  detail: a dict; receives link_batch's
    result as detail['link'] = dict(maps, merges, stat_max, stat_min).  A dictionary like LINK_CLR
    links by cross-likelihood ratio (link_batch, model 'clr'): the frames and the clustering segments
    are passed through to it.  Such a dictionary may carry gallery=<gallery.Gallery>, enrol and
    exclusive (link_batch): the third column then holds identities of the gallery + 1, the same
    person in every batch, and detail['link'] gains identity, score, second and enrolled.  A
    dictionary like LINK_CLR_WARP feature-warps the frames first (link['warp_s'], link_batch; warp_batch
    is that stage on its own).
    reseg: a dictionary like RESEG; the rows are then those of resegment_batch on the records and
    labels clustering left: every turn decoded frame by frame under the file's speaker models, so
    the boundaries sit where the evidence changes instead of on the detector's candidate grid.
    Either clustering method, any detector; host hand-off only.  With link as well, linking runs
    on the clustering segments as without reseg and the resegmented rows' third column is mapped
    through its maps.  detail['dropped'] as resegment_batch.  reseg=None: today's rows.  A dictionary
    like RESEG_GMM decodes under mixture models trained on the clustering segments' frames
    (resegment_batch, model 'gmm'; detail['loglik'] as there).  A dictionary like RESEG_MD decodes with
    a minimum speaker duration (reseg['min_dur_s']), and reseg['passes'] retrains the speakers on the
    decoded rows and decodes again; both keys go to resegment_batch as they are
    (detail['passes_run'] as there).  A dictionary like RESEG_CONF adds a confidence to every row
    (reseg['confidence'], reseg['conf_scale']; detail['confidence'] and detail['log_evidence'] as there):
    it takes a detail dictionary.  With link the confidences stay those of the file's own speakers.
    A dictionary like RESEG_SOFT retrains the speakers between the passes on frame posteriors instead of
    decoded rows (reseg['soft'], reseg['soft_scale']; detail['soft_mass'] as there).  A dictionary like
    RESEG_TDOA adds the microphone array's delays as a second stream (reseg['tdoa'], with delays=<the
    frontend.DelayStream the beamformer filled>; detail['tdoa_channels'] as there).
    seats: a dictionary like SEATS, with delays=<the same stream>: the delays also reach the two stages that decide
    how many talkers a file has.  The segments change detection returns are cut where their delays change
    (seat_cut_batch) before clustering, and the labels clustering returns are split where an acoustic cluster sits at
    two places (seat_split_batch) before resegmentation, linking or the rows read them; linking then runs on the
    pieces' records and stays acoustic (seats do not carry from one room to another).  Host hand-off only and not
    fused (the fused records belong to the uncut segments), cl method hi only; seats without delays, a stream of
    another file count or frame clock, unknown keys or bad values: ValueError before any device work.  More than 16
    speakers in a file after a split, under reseg, is resegment_batch's ValueError.  detail['seats'] = dict(cuts,
    passes_run, split, unplaced) as the two stages leave them; timings: seat_cuts, seat_stats, seat_split.  A talker
    who moves is split; two talkers who share a seat are left to the acoustics.  seats=None: today's calls and rows.
    overlap: a dictionary like OVERLAP, with delays=<a stream made with second=True>: overlap_batch runs on the rows
    this call is about to return -- after resegmentation, seats and linking -- and finds where a second speaker of the
    file talks beside the row's own; the rows themselves are returned unchanged.  detail['overlap'] = dict(rows,
    speakers, steps, seconds, unassigned) as overlap_batch leaves it (second_rows makes recipe rows of detail['overlap']
    ['rows']); timings: overlap_stats, overlap_models, overlap_match.  Host hand-off only; overlap without such a
    stream, unknown keys or bad values: ValueError before any device work.  overlap=None: today's calls and rows."""
    method = _method(cl)
    # the hand-off this call gets: the one asked for, else the device's where it can serve (a detector that
    # passes its refusal below is neither fused nor on the device, so the rule reads the same behind it)
    device = handoff == 'device' or (handoff is None and fused and text_contract and method == 'hi')
    if reseg is not None:
        reseg_opts = _resegmentation._reseg_options(reseg, rate, detail)
        if device:
            raise ValueError('reseg takes the host hand-off')
        if reseg_opts.tdoa:
            _resegmentation._check_delays(delays, reseg_opts, files, float(rate), True)
    if seats is not None:
        _seats._seat_options(seats, rate)
        if device or fused:
            raise ValueError('seats take the host hand-off and are not fused: the fused records belong to the uncut segments')
        if method != 'hi':
            raise ValueError('seats split the clusters of cl method hi')
        _seats._check_delays(delays, files, float(rate))
        _seats._empty_detail(detail, len(files))
    if overlap is not None:
        _overlap._check_delays(delays, _overlap._overlap_options(overlap), files, float(rate))
        if device:
            raise ValueError('overlap takes the host hand-off')
    if _cd_method(cd) in ('sw', 'm'):
        if fused or handoff == 'device':
            raise ValueError('cd method %s takes the host hand-off and is not fused' % _cd_method(cd))
        handoff = 'host'
    if link is not None:
        _linking._link_options(link, rate)           # (its refusals come before any work; link_batch parses for itself)
        if device:
            raise ValueError('link takes the host hand-off')
    if handoff is None:
        handoff = 'device' if device else 'host'
    if handoff == 'device':
        if method == 'in':
            raise ValueError('the device hand-off clusters with spk_cluster_hi: method in takes the host hand-off')
        if not (fused and text_contract):
            raise ValueError('the device hand-off is the fused mode with the text contract')
        return diarize_batch_device(ctx, d_frames, total_frames, files, rate, cd, cl, timings)
    if handoff != 'host':
        raise ValueError('handoff: device or host')
    box = [] if fused else None
    segs = change_detect_batch(ctx, d_frames, total_frames, files, rate, cd, timings, text_contract, box)
    fs = box[0] if box else None
    if (fused and fs is None) or not any(len(s) for s in segs):      # no turn at all in the batch
        if link is not None and detail is not None:
            detail['link'] = dict(maps=[np.zeros(0, dtype=np.int32) for _ in files], merges=[],
                                  stat_max=float('nan'), stat_min=float('nan'))
        if reseg is not None:
            _resegmentation._empty_detail(detail, reseg_opts, len(files))
        rows = [np.zeros((0, 3)) for _ in files]
        if overlap is not None:
            overlap_batch(ctx, files, rows, delays, rate, overlap, text_contract, timings, detail)
        return rows
    if seats is not None:
        segs = seat_cut_batch(ctx, files, segs, delays, rate, seats, text_contract, timings, detail)
    rows = _cluster_and_order(ctx, d_frames, total_frames, files, segs, rate, cl, timings, fs, link, detail, reseg, text_contract,
                              delays, seats)
    if overlap is not None:
        overlap_batch(ctx, files, rows, delays, rate, overlap, text_contract, timings, detail)
    return rows


def warp_batch(ctx, d_frames, total_frames, files, segments, rate, warp_s, d_out=None):
    """Feature warping on its own (spkd_feature_warp; include/spkd.h, section 10b): the frames of every
    file's segments (one array of (start_s, end_s) per file, cut into frame ranges as the clustering
    stage cuts them), each coefficient replaced by the standard-normal quantile of its rank among the
    round(warp_s * rate) frames of the file's speech around it -- what link_batch does first under
    LINK_CLR_WARP.  Into d_out (total_frames * 39 floats, not d_frames; a frame of no segment is not
    written), or, d_out=None, into a buffer the context keeps until the next call.  Returns the device
    pointer.  A window outside [2, 512] frames, warp_s = 0: ValueError.  The kernel's time is
    ctx.last_ms('feature_warp')."""
    window = _linking.warp_window(dict(model='clr', warp_s=warp_s), rate)
    if not window:
        raise ValueError('link warp_s: warp_batch takes a window')
    if len(segments) != len(files):
        raise ValueError('one segment array per file')
    seg_off, _, seg_b, seg_e = _segment_ranges(files, segments, float(rate))
    return _linking.warp_frames(ctx, d_frames, total_frames, seg_off, seg_b, seg_e, window, d_out)


def _cluster_and_order(ctx, d_frames, total_frames, files, segs, rate, cl, timings, fs, link=None, detail=None,
                       reseg=None, text_contract=True, delays=None, seats=None):
    box = None if link is None and reseg is None else []
    res = cluster_batch(ctx, d_frames, total_frames, files, segs, rate, cl, timings, fused=fs, stats_out=box)
    cnt = [len(s) for s in segs]
    if sum(cnt) == 0:
        return [np.zeros((0, 3)) for _ in segs]
    own = [lab for (lab, _) in res]
    if seats is not None:
        own = seat_split_batch(ctx, files, segs, own, delays, rate, seats, timings, detail)
    if reseg is not None:
        rows = resegment_batch(ctx, d_frames, total_frames, files, box[0][0], box[0][1], own, rate, reseg,
                               text_contract, timings, detail, segs, delays)
    if link is not None:                             # (on the clustering segments, with or without reseg)
        more = {}
        maps, merges, smax, smin = link_batch(ctx, box[0][0], box[0][1], own, link, timings, d_frames, total_frames,
                                              files, segs, rate, more)
        if detail is not None:
            detail['link'] = dict(maps=maps, merges=merges, stat_max=smax, stat_min=smin, **more)
    if reseg is not None:
        if link is not None:
            for r, m in zip(rows, maps):
                r[:, 2] = m[r[:, 2].astype(np.int64)] if len(r) else r[:, 2]
        return rows
    allseg = np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1, 2) for s in segs])
    labels = np.concatenate(own if link is None else [m[lab] for m, lab in zip(maps, own)])
    bounds = np.zeros(len(segs) + 1, dtype=np.int64)
    bounds[1:] = np.cumsum(cnt)
    if _method(cl) == 'in':
        rows = np.column_stack([allseg, labels.astype(np.float64)])
        if cl['variant'] == 1:
            later = np.ones(len(rows), dtype=bool)
            later[bounds[:-1][np.diff(bounds) > 0]] = False
            rows[later, :2] = (rows[later, :2] * rate).astype(np.int64) / rate
    else:
        rows = _recipe_rows(allseg, np.repeat(np.arange(len(segs)), cnt), labels, rate)
    out = [rows[bounds[i]:bounds[i + 1]] for i in range(len(segs))]
    return out


def in_flight(contexts, n_jobs, job):
    """Runs job(ctx, k) for k = 0 .. n_jobs - 1 with one job in flight per context -- a host
    thread per context, each taking the next k when it is free -- and yields the results in
    order of k.  With two contexts on streams of their own the host part of one batch (recipe
    text, label replay) runs under the kernels of the next, and the tail of one launch beside
    the head of the next: + 5 - 10 % throughput on 256-hour batches (DESIGN.md par. 5).  A
    context is only ever used by its own thread; an exception in a job is re-raised here."""
    import threading
    if len(contexts) == 1 or n_jobs <= 1:
        for k in range(n_jobs):
            yield job(contexts[0], k)
        return
    results = [None] * n_jobs
    done = [threading.Event() for _ in range(n_jobs)]
    nxt = [0]
    lock = threading.Lock()
    failure = []

    def worker(ctx):
        while not failure:
            with lock:
                k = nxt[0]
                nxt[0] += 1
            if k >= n_jobs:
                return
            try:
                results[k] = job(ctx, k)
            except BaseException as e:               # surfaces on the consuming thread
                failure.append(e)
            finally:
                done[k].set()

    threads = [threading.Thread(target=worker, args=(c,)) for c in contexts]
    for th in threads:
        th.start()
    try:
        for k in range(n_jobs):
            done[k].wait()
            if failure:
                break
            r, results[k] = results[k], None
            yield r
    finally:
        if not failure:
            failure.append(None)                     # (an abandoned run: the workers stop after their current job)
        for th in threads:
            th.join()
    if failure and failure[0] is not None:
        raise failure[0]
