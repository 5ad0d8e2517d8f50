"""Seats from the microphone array's delays (include/spkd.h (6b4)), behind the two acoustic stages that decide how
many talkers a file has: seat_cut_batch cuts a change-detection segment where its delays change (spkd_tdoa_cuts),
seat_split_batch makes two speakers of an acoustic cluster whose segments sit at two places (spkd_tdoa_stats,
spkd_tdoa_split, spkd_labels_from_merges).  Both read the frontend.DelayStream the beamformer filled and work on the
exact integer delay records; both are opt-in (diarize_batch(..., seats=SEATS, delays=stream)).  A `seats` dictionary
is parsed once (_seat_options).  The layer of resegmentation: this module imports tables and hipabi only."""
import collections

import numpy as np

from . import hipabi
from .tables import _segment_ranges, link_speakers

# lambdac and threshold: the penalty's weight and the decision level of the statistic, BIC's convention (Delta > threshold:
# two seats).  min_frames and floor_s as TDOA's: the reliable frames a side needs on a channel, and the smallest standard
# deviation of a delay in seconds (one sample at 16 kHz).  min_piece_s: no piece of a cut segment is shorter, the change
# detector's own smallest window.  max_passes: calls of the cut stage, each on the pieces the one before made.  cut, split:
# the two stages.  lambdac, min_piece_s and max_passes are settings that rest on synthetic fixtures and are UNMEASURED
# on speech, like min_frames and floor_s.  Segments whose ends fall inside steps carry a few frames of the neighbour's
# seat, which the statistic reads as a change: on acoustically distinct speakers the stages over-split (DESIGN.md par. 5).
SEATS = dict(lambdac=1.0, threshold=0.0, min_frames=40, floor_s=1.0 / 16000.0, min_piece_s=1.0, max_passes=8, cut=True,
             split=True)

_Seats = collections.namedtuple('_Seats', 'lambdac threshold min_frames floor_s min_piece max_passes cut split')


def _number(seats, key):
    try:
        return float(seats.get(key, SEATS[key]))
    except (TypeError, ValueError):
        return float('nan')


def _whole(seats, key):
    n = seats.get(key, SEATS[key])
    try:
        ok = not isinstance(n, (bool, np.bool_)) and int(n) == n
    except (TypeError, ValueError, OverflowError):
        ok = False
    return int(n) if ok and 1 <= n <= 0x7fffffff else None


def _flag(seats, key):
    on = seats.get(key, SEATS[key])
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError('seats %s: True or False' % key)
    return bool(on)


def _seat_options(seats, rate):
    """A `seats` dictionary parsed once, each key by its validator, in the order of SEATS; a key that is absent takes
    SEATS' value, a key SEATS does not have is refused.  min_piece is in frames: max(1, floor(min_piece_s * rate))."""
    if not isinstance(seats, dict) or set(seats) - set(SEATS):
        raise ValueError('seats: a dictionary with keys of SEATS (%s)' % ', '.join(sorted(SEATS)))
    lambdac = _number(seats, 'lambdac')
    if not np.isfinite(lambdac):
        raise ValueError('seats lambdac: a finite number')
    threshold = _number(seats, 'threshold')
    if np.isnan(threshold):
        raise ValueError('seats threshold: a number (Delta above it means two seats)')
    min_frames = _whole(seats, 'min_frames')
    if min_frames is None:
        raise ValueError('seats min_frames: an integer >= 1')
    floor_s = _number(seats, 'floor_s')
    if not np.isfinite(floor_s) or floor_s <= 0.0:
        raise ValueError('seats floor_s: a finite number > 0 (seconds)')
    piece = _number(seats, 'min_piece_s')
    if not np.isfinite(piece) or piece < 0.0:
        raise ValueError('seats min_piece_s: a finite number >= 0 (seconds)')
    max_passes = _whole(seats, 'max_passes')
    if max_passes is None:
        raise ValueError('seats max_passes: an integer >= 1')
    cut, split = _flag(seats, 'cut'), _flag(seats, 'split')
    return _Seats(lambdac, threshold, min_frames, floor_s, max(1, int(np.floor(piece * float(rate)))), max_passes, cut, split)


def _check_delays(delays, files, rate):
    """The stages read a stream of the batch's files on the batch's frame clock (resegmentation._check_delays' rule)."""
    if delays is None:
        raise ValueError('seats: they read the delays the beamformer tracked, delays=<frontend.DelayStream>')
    if delays.n_files != len(files):
        raise ValueError('delays: a stream of %d files, a batch of %d' % (delays.n_files, len(files)))
    if float(delays.rate_out) != float(rate) * delays.hop:
        raise ValueError('delays: the stream steps %d samples a frame at %d Hz, the batch has %g frames a second'
                         % (delays.hop, delays.rate_out, rate))


def _empty_detail(detail, n_files):
    if detail is not None:
        detail['seats'] = dict(cuts=[[] for _ in range(n_files)], passes_run=0, split=[[] for _ in range(n_files)],
                               unplaced=[0] * n_files)


def _has_steps(delays):
    """Per file of the stream: more than one channel and at least one step."""
    return (delays.files[:, 2] > 1) & (delays.files[:, 1] > 0)


def cut_time(frame, rate, text_contract):
    """A time in seconds that _segment_ranges takes back to exactly `frame` (file-local): int(time * rate) == frame, and
    with text_contract the time is its own 12-digit round trip (hipabi.py2_roundtrip), so it survives the recipe.  The
    frame's own time frame / rate where that holds; a quarter or half a frame later where the division or the twelve
    digits land just below the frame."""
    frame, rate = int(frame), float(rate)
    for eps in (0.0, 0.25, 0.5):
        t = (frame + eps) / rate
        if text_contract:
            t = float(hipabi.py2_roundtrip(np.array([t]))[0])
        if int(t * rate) == frame:
            return t
    raise ValueError('frame %d has no time at %g frames a second' % (frame, rate))


def seat_cut_batch(ctx, files, segments, delays, rate=125.0, seats=SEATS, text_contract=True, timings=None, detail=None):
    """segments: per file the (start_s, end_s) of change_detect_batch.  Every segment of a file with delays goes to
    spkd_tdoa_cuts as its frame range (_segment_ranges); a segment that is cut is replaced by its two pieces, and the
    call is repeated on the pieces that are new until one cuts nothing or seats['max_passes'] calls are done.  A cut
    time is cut_time's, so the pieces' frame ranges meet at the cut frame.  Returns the segments per file, arrays [n, 2];
    a file with one channel or no steps, and any file when nothing can be cut, keeps its segments object.
    detail['seats'] gains cuts (per file the cut times, ascending) and passes_run (the calls made); timings:
    seat_cuts, kernel ms, one entry per call.  Every ValueError comes before any device work."""
    rate = float(rate)
    opts = _seat_options(seats, rate)
    _check_delays(delays, files, rate)
    if len(segments) != len(files):
        raise ValueError('one segment array per file')
    if detail is not None and 'seats' not in detail:
        _empty_detail(detail, len(files))
    active = _has_steps(delays)
    work = {f: [(float(s), float(e), True) for s, e in np.asarray(segments[f], dtype=np.float64).reshape(-1, 2)]
            for f in range(len(files)) if active[f] and len(segments[f])}
    if not work or not opts.cut:
        return list(segments)
    stream = delays.handle([f.frame_off for f in files])
    cuts = {f: [] for f in work}
    passes = 0
    while passes < opts.max_passes:
        new = [(f, i) for f in sorted(work) for i, s in enumerate(work[f]) if s[2]]
        if not new:
            break
        cur = [[(s, e) for s, e, _ in work[f]] if f in work else [] for f in range(len(files))]
        seg_off, _, b, e = _segment_ranges(files, cur, rate)
        at = np.array([seg_off[f] + i for f, i in new], dtype=np.int64)
        cut, _ = ctx.tdoa_cuts(stream, b[at], e[at], [f for f, _ in new], opts.min_piece, opts.min_frames, opts.floor_s,
                               opts.lambdac, opts.threshold)
        passes += 1
        if timings is not None:
            timings.setdefault('seat_cuts', []).append(ctx.last_ms('tdoa_cuts'))
        for f in work:
            work[f] = [(s, e, False) for s, e, _ in work[f]]
        for (f, i), frame in sorted(zip(new, cut.tolist()), reverse=True):       # (from the back: the indices before stay)
            if frame < 0:
                continue
            s, e, _ = work[f][i]
            t = cut_time(frame - files[f].frame_off, rate, text_contract)
            work[f][i:i + 1] = [(s, t, True), (t, e, True)]
            cuts[f].append(t)
        if not (cut >= 0).any():
            break
    if detail is not None:
        detail['seats']['passes_run'] = passes
        for f in work:
            detail['seats']['cuts'][f] = sorted(cuts[f])
    return [np.array([(s, e) for s, e, _ in work[f]], dtype=np.float64).reshape(-1, 2) if f in work and cuts[f] else segments[f]
            for f in range(len(files))]


def seat_split_batch(ctx, files, segments, labels, delays, rate=125.0, seats=SEATS, timings=None, detail=None):
    """segments, labels: per file what cluster_batch took and returned.  A problem is the segments of one label of one
    file (link_speakers' order: file by file, by ascending label, the segments in their order).  One spkd_tdoa_stats
    gives every segment its delay record, one spkd_tdoa_split chains every problem, spkd_labels_from_merges replays
    the logs.  A seat is a final cluster with a placed record; an unplaced segment joins the seat of its problem that
    holds the most frames, the lowest seat on a tie; a problem with no placed segment stays whole.  Returns the labels
    per file: 1 .. K ordered by (old label, first segment of the seat) in a file where a label split, the file's own
    label array, the same object, elsewhere.  detail['seats'] gains split (per file (old label, seats) of every label
    that split) and unplaced (per file the count of unplaced segments of files with delays); timings: seat_stats,
    seat_split (kernel ms).  More than 16 speakers in a file afterwards is resegment_batch's ValueError, when it
    runs.  Every ValueError here comes before any device work."""
    rate = float(rate)
    opts = _seat_options(seats, rate)
    _check_delays(delays, files, rate)
    if len(segments) != len(files) or len(labels) != len(files):
        raise ValueError('one segment array and one label array per file')
    seg_off, n, b, e = _segment_ranges(files, segments, rate)
    member, set_off, spk_file, spk_label = link_speakers(seg_off, labels)
    if detail is not None and 'seats' not in detail:
        _empty_detail(detail, len(files))
    active = _has_steps(delays)
    if n == 0 or not opts.split or not active.any():
        return list(labels)
    stream = delays.handle([f.frame_off for f in files])
    owner = np.repeat(np.arange(len(files)), np.diff(seg_off))
    d_stats = ctx.dev_scratch('seat_stats', n * hipabi.TDOA_MAX_CH * 3 * 8)
    ctx.tdoa_stats(stream, b[member], e[member], owner[member], np.arange(n), n, d_stats)
    if timings is not None:
        timings.setdefault('seat_stats', []).append(ctx.last_ms('tdoa_stats'))
    r = ctx.tdoa_split(d_stats, set_off, spk_file, stream[2], stream[3], opts.min_frames, opts.floor_s, opts.lambdac,
                       opts.threshold)
    if timings is not None:
        timings.setdefault('seat_split', []).append(ctx.last_ms('tdoa_split'))
    cluster = hipabi.labels_from_merges_batch(set_off, r['n_merges'], r['a'], r['b'])
    frames = (e - b)[member]
    out = list(labels)
    split = [[] for _ in files]
    unplaced = [0] * len(files)
    new = np.zeros(n, dtype=np.int64)                      # per segment its speaker, 0-based within its file
    base = 0
    for p in range(len(spk_file)):
        f = int(spk_file[p])
        if p and spk_file[p - 1] != f:
            base = 0
        o, k = int(set_off[p]), int(set_off[p + 1])
        placed, cl = r['placed'][o:k] != 0, cluster[o:k]
        if active[f]:
            unplaced[f] += int((~placed).sum())
        seat_of = {int(c): i for i, c in enumerate(np.unique(cl[placed]))}       # (ascending cluster: by first segment)
        if len(seat_of) < 2:
            seat = np.zeros(k - o, dtype=np.int64)
        else:
            seat = np.array([seat_of.get(int(c), -1) for c in cl], dtype=np.int64)
            held = np.bincount(seat[placed], weights=frames[o:k][placed], minlength=len(seat_of))
            seat[~placed] = int(np.argmax(held))           # (the first of equals: the lowest seat)
            split[f].append((int(spk_label[p]), len(seat_of)))
        new[member[o:k]] = base + seat
        base += max(len(seat_of), 1)
    for f in range(len(files)):
        if split[f]:
            out[f] = (new[seg_off[f]:seg_off[f + 1]] + 1).astype(np.asarray(labels[f]).dtype)
    if detail is not None:
        detail['seats']['split'] = split
        detail['seats']['unplaced'] = unplaced
    return out
