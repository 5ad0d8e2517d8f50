"""Overlapped speech from the microphone array's delays (include/spkd.h (6b5)), behind everything that decides the rows:
while two talkers at two seats speak in one step, the delay the beamformer tracked is one talker's seat and the
runner-up among the step's GCC-PHAT candidates is the other's.  overlap_batch trains one delay model per speaker of
the rows it is handed (spkd_tdoa_stats, spkd_tdoa_models), asks the device for the pair of speakers of every step
(spkd_tdoa_overlap) and cuts the rows where a pair holds: each piece names its row's speaker and a second one.  It reads
a frontend.DelayStream made with second=True; the rows themselves are not changed.  Opt-in (diarize_batch(...,
overlap=OVERLAP, delays=stream)).  An `overlap` dictionary is parsed once (_overlap_options).  The layer of seats: this
module imports tables, seats and hipabi only."""
import collections

import numpy as np

from . import hipabi
from .seats import cut_time
from .tables import _segment_ranges

# min_second, guard: the runner-up stream's (frontend.SECOND; they act where the stream is made).  gate: a lag is near a
# speaker's seat on a channel while (lag - mean)^2 / (2 var) <= gate, three standard deviations.  min_channels: the channels
# that must agree on a pair (or all the live ones, where a file has fewer).  min_steps: the shortest run of steps with one
# pair that counts.  min_frames, floor_s as TDOA's: the reliable frames a speaker needs on a channel, and the smallest
# standard deviation of a delay in seconds.  min_second, guard, gate, min_channels and min_steps rest on the white-noise
# scenes of tests/beamform_numpy.py and are UNMEASURED on speech and in reverberation.  Talkers at one seat, or at seats
# whose delays coincide on all but fewer than min_channels channels, are not seen; a second talker 10 dB down is not seen
# in the two-talker scene of tests/test_overlap.py (profiles/overlap_accuracy.json).
OVERLAP = dict(min_second=0.1, guard=3, gate=4.5, min_channels=2, min_steps=2, min_frames=40, floor_s=1.0 / 16000.0)

_Overlap = collections.namedtuple('_Overlap', 'min_second guard gate min_channels min_steps min_frames floor_s')


def _number(overlap, key):
    try:
        return float(overlap.get(key, OVERLAP[key]))
    except (TypeError, ValueError):
        return float('nan')


def _whole(overlap, key, lo, hi=0x7fffffff):
    n = overlap.get(key, OVERLAP[key])
    try:
        ok = not isinstance(n, (bool, np.bool_)) and int(n) == n
    except (TypeError, ValueError, OverflowError):
        ok = False
    return int(n) if ok and lo <= n <= hi else None


def _overlap_options(overlap):
    """An `overlap` dictionary parsed once, each key by its validator, in the order of OVERLAP; a key that is absent
    takes OVERLAP's value, a key OVERLAP does not have is refused."""
    if not isinstance(overlap, dict) or set(overlap) - set(OVERLAP):
        raise ValueError('overlap: a dictionary with keys of OVERLAP (%s)' % ', '.join(sorted(OVERLAP)))
    min_second = _number(overlap, 'min_second')
    if np.isnan(min_second):
        raise ValueError('overlap min_second: a number')
    guard = _whole(overlap, 'guard', 0)
    if guard is None:
        raise ValueError('overlap guard: an integer >= 0 (samples)')
    gate = _number(overlap, 'gate')
    if not np.isfinite(gate) or gate <= 0.0:
        raise ValueError('overlap gate: a finite number > 0')
    min_channels = _whole(overlap, 'min_channels', 1)
    if min_channels is None:
        raise ValueError('overlap min_channels: an integer >= 1')
    min_steps = _whole(overlap, 'min_steps', 1, hipabi.OVERLAP_MAX_RUN)
    if min_steps is None:
        raise ValueError('overlap min_steps: an integer in [1, %d]' % hipabi.OVERLAP_MAX_RUN)
    min_frames = _whole(overlap, 'min_frames', 1)
    if min_frames is None:
        raise ValueError('overlap min_frames: an integer >= 1')
    floor_s = _number(overlap, 'floor_s')
    if not np.isfinite(floor_s) or floor_s <= 0.0:
        raise ValueError('overlap floor_s: a finite number > 0 (seconds)')
    return _Overlap(min_second, guard, gate, min_channels, min_steps, min_frames, floor_s)


def _check_delays(delays, opts, files, rate):
    """The stage reads a stream of the batch's files on the batch's frame clock (seats._check_delays' rule) that keeps
    the runner-ups, made with the dictionary's min_second and guard where the stream knows its own."""
    if delays is None:
        raise ValueError('overlap: it reads the delays the beamformer tracked, delays=<frontend.DelayStream(..., second=True)>')
    if not getattr(delays, 'second', False):
        raise ValueError('overlap: the stream keeps no runner-ups; make it with frontend.DelayStream(..., second=True) '
                         'before the beamformer fills it (diarize_audio_batch(..., overlap=) does)')
    if delays.n_files != len(files):
        raise ValueError('delays: a stream of %d files, a batch of %d' % (delays.n_files, len(files)))
    if float(delays.rate_out) != float(rate) * delays.hop:
        raise ValueError('delays: the stream steps %d samples a frame at %d Hz, the batch has %g frames a second'
                         % (delays.hop, delays.rate_out, rate))
    if delays.from_beamformer and (delays.min_second, delays.guard) != (opts.min_second, opts.guard):
        raise ValueError('overlap: the stream kept its runner-ups with min_second %g and guard %d, the dictionary says %g and %d'
                         % (delays.min_second, delays.guard, opts.min_second, opts.guard))


def _speakers(rows):
    """Per file the distinct values of the rows' third column, ascending; more than 16 in a file: ValueError."""
    out = []
    for f, r in enumerate(rows):
        r = np.asarray(r, dtype=np.float64)
        if r.size and (r.ndim != 2 or r.shape[1] < 3):
            raise ValueError('file %d: rows [start_s, end_s, speaker] expected' % f)
        spk = np.unique(r[:, 2]) if r.size else np.zeros(0)
        if len(spk) > hipabi.OVERLAP_MAX_SPK:
            raise ValueError('file %d: %d speakers, the overlap stage takes at most %d a file' % (f, len(spk), hipabi.OVERLAP_MAX_SPK))
        out.append(spk)
    return out


def step_runs(steps):
    """int32 [T, 2] -> [(first step, last step, j, k)]: the maximal runs of consecutive steps with one pair."""
    steps = np.asarray(steps).reshape(-1, 2)
    runs, t, T = [], 0, len(steps)
    while t < T:
        u = t
        while u + 1 < T and steps[u + 1, 0] == steps[t, 0] and steps[u + 1, 1] == steps[t, 1]:
            u += 1
        if steps[t, 0] >= 0:
            runs.append((t, u, int(steps[t, 0]), int(steps[t, 1])))
        t = u + 1
    return runs


def pieces_of_file(steps, first_frame, n_frames, row_b, row_e, row_spk):
    """The host intersection for one file.  steps int32 [T, 2] (indices into the file's speakers); first_frame(s): the
    first frame of step s, file-local; the rows' frame ranges [row_b, row_e), file-local, and their speakers' indices.
    A run of steps [s0, s1] covers the frames [first_frame(s0), first_frame(s1 + 1)) clipped to [0, n_frames].
    Returns ([(begin, end, speaker index, second index)] in row order and, within a row, run order; the frames of rows
    whose speaker is neither of a run's pair)."""
    out, unassigned = [], 0
    runs = [(min(first_frame(s0), n_frames), min(first_frame(s1 + 1), n_frames), j, k) for s0, s1, j, k in step_runs(steps)]
    for b, e, p in zip(row_b, row_e, row_spk):
        for lo, hi, j, k in runs:
            x, y = max(int(b), lo), min(int(e), hi)
            if y <= x:
                continue
            if p == j or p == k:
                out.append((x, y, int(p), k if p == j else j))
            else:
                unassigned += y - x
    return out, unassigned


def overlap_batch(ctx, files, rows, delays, rate=125.0, overlap=OVERLAP, text_contract=True, timings=None, detail=None):
    """rows: per file the array [start_s, end_s, speaker, ...] a diarization returned.  The speakers of a file are the
    distinct values of the third column, ascending (at most 16); the rows' frame ranges are _segment_ranges'.  One
    spkd_tdoa_stats gives every (file, speaker) its delay record over its rows, one spkd_tdoa_models a Gaussian per
    channel (every speaker counts as ok), one spkd_tdoa_overlap the pair of every step, read back.  Each run of steps
    [s0, s1] with one pair (j, k) covers the frames [first frame of s0, first frame of s1 + 1), clipped to the file;
    intersected with a row of speaker p it gives a piece whose second speaker is the other of the pair, or, where p is
    neither, frames that are counted and dropped.  Times are seats.cut_time's.  Returns per file an array
    [start_s, end_s, speaker, second], in row order (second_rows makes recipe rows of it).  detail['overlap'] =
    dict(rows: the result, speakers: per file the ascending speakers, steps: per file int32 [T, 2] of indices into
    them or -1, seconds: per file the length of the pieces, unassigned: per file the dropped frames); timings:
    overlap_stats, overlap_models, overlap_match (kernel ms).  A stream without runner-ups, of another file count or
    frame clock, unknown keys, bad values, more than 16 speakers: ValueError before any device work."""
    rate = float(rate)
    opts = _overlap_options(overlap)
    _check_delays(delays, opts, files, rate)
    if len(rows) != len(files):
        raise ValueError('one row array per file')
    speakers = _speakers(rows)
    n_files = len(files)
    cut = [np.asarray(r, dtype=np.float64)[:, :2] if len(r) else np.zeros((0, 2)) for r in rows]
    seg_off, n, b, e = _segment_ranges(files, cut, rate)
    spk_off = np.concatenate([[0], np.cumsum([len(s) for s in speakers])]).astype(np.int64)
    T = delays.files[:, 1].astype(np.int64) if n_files else np.zeros(0, dtype=np.int64)
    step_off = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    total = int(step_off[-1])
    pair = np.full((total, 2), -1, dtype=np.int32)
    which = [np.searchsorted(speakers[f], np.asarray(rows[f], dtype=np.float64)[:, 2]) if len(rows[f]) else np.zeros(0, dtype=np.int64)
             for f in range(n_files)]
    if total and n:
        stream = delays.handle([f.frame_off for f in files])
        d_second = delays.handle_second()
        owner = np.repeat(np.arange(n_files), np.diff(seg_off))
        sets = np.concatenate([spk_off[f] + which[f] for f in range(n_files)]).astype(np.int64)
        order = np.argsort(sets, kind='stable')
        n_spk = int(spk_off[-1])
        d_stats = ctx.dev_scratch('overlap_stats', n_spk * hipabi.TDOA_MAX_CH * 3 * 8)
        d_models = ctx.dev_scratch('overlap_models', n_spk * hipabi.TDOA_MAX_CH * hipabi.TDOA_MODEL * 8)
        d_pair = ctx.dev_scratch('overlap_pair', total * 8)
        ctx.tdoa_stats(stream, b[order], e[order], owner[order], sets[order], n_spk, d_stats)
        if timings is not None:
            timings.setdefault('overlap_stats', []).append(ctx.last_ms('tdoa_stats'))
        spk_file = np.repeat(np.arange(n_files), np.diff(spk_off))
        live = ctx.tdoa_models(d_stats, spk_file, np.ones(n_spk, dtype=np.int32), stream[2], opts.min_frames, opts.floor_s, d_models)
        if timings is not None:
            timings.setdefault('overlap_models', []).append(ctx.last_ms('tdoa_models'))
        ctx.tdoa_overlap(stream, d_second, d_models, live, spk_off, opts.gate, opts.min_channels, opts.min_steps, d_pair)
        if timings is not None:
            timings.setdefault('overlap_match', []).append(ctx.last_ms('tdoa_overlap'))
        ctx.d2h(pair, d_pair)
    out, steps, seconds, unassigned = [], [], [], []
    for f in range(n_files):
        st = pair[step_off[f]:step_off[f + 1]]
        fo = int(files[f].frame_off)
        got, lost = pieces_of_file(st, lambda s, f=f: delays.first_frame_of(f, s), int(files[f].n_frames),
                                   b[seg_off[f]:seg_off[f + 1]] - fo, e[seg_off[f]:seg_off[f + 1]] - fo, which[f])
        out.append(np.array([(cut_time(x, rate, text_contract), cut_time(y, rate, text_contract), speakers[f][p], speakers[f][q])
                             for x, y, p, q in got], dtype=np.float64).reshape(-1, 4))
        steps.append(st.copy())
        seconds.append(sum(y - x for x, y, _, _ in got) / rate)
        unassigned.append(int(lost))
    if detail is not None:
        detail['overlap'] = dict(rows=out, speakers=[s.tolist() for s in speakers], steps=steps, seconds=seconds, unassigned=unassigned)
    return out


def second_rows(result):
    """overlap_batch's result -> per file rows [start_s, end_s, second]: the second speaker's lines, to append to a
    recipe beside the rows the diarization returned."""
    return [np.asarray(r, dtype=np.float64).reshape(-1, 4)[:, [0, 1, 3]] for r in result]
