"""Linking the speakers of a batch's files (link_batch): which speaker of one file is which speaker of
another, by BIC over the speakers' summed records (LINK_CL) or by cross-likelihood ratio under a universal
background model (LINK_CLR), the latter optionally on warped features (LINK_CLR_WARP) and against a gallery
of enrolled speakers.  A `link` dictionary is parsed once (_link_options); the two chains (_bic_chain,
_clr_chain) hand link_batch the same six values.
Layers: tables (the speaker list, the segment ranges) and clr_model (LINK_CLR, _link_model, ubm_ranges,
train_ubm -- the four pieces the gallery needs too, offered here under their names) lie below, gallery
stands on clr_model, this module on all three, pipeline on this one.  clr_model is a file of its own
because this module imports gallery (it refuses a link['gallery'] that is no Gallery) and gallery needs
the four: held here, they would close a cycle."""
import collections
import contextlib

import numpy as np

from . import hipabi
from .clr_model import LINK_CLR, LINK_CLR_WARP, _link_model, train_ubm, ubm_ranges, warp_window
from .gallery import Gallery
from .tables import _ahc_params, _segment_ranges, link_speakers

# linking the speakers of a batch's files (link_batch): the clustering script's own defaults
LINK_CL = dict(variant=1, kind='BIC', lambdac=1.3, threshold=0.0, max_spk=0)

_Options = collections.namedtuple('_Options', 'model gallery enrol exclusive warp')


def _link_options(link, rate=125.0):
    """A `link` dictionary parsed once: model is _link_model's tuple, whose refusals come first, in its
    order; then warp, the feature-warping window in frames at `rate` (clr_model.warp_window; 0: none);
    then the gallery keys, which only model 'clr' takes: gallery (None without one), enrol and
    exclusive (both True where absent, False without a gallery)."""
    model = _link_model(link)
    warp = warp_window(link, rate)
    gal = link.get('gallery')
    if model.name != 'clr' and gal is not None:
        raise ValueError('link gallery: a gallery holds the records of link model clr')
    if gal is None:
        return _Options(model, None, False, False, warp)
    if not isinstance(gal, Gallery):
        raise ValueError('link gallery: a gallery.Gallery')
    if gal.components != model.components:
        raise ValueError('link components: the gallery has %d' % gal.components)
    if gal.relevance != model.relevance:
        raise ValueError('link relevance: the gallery has %r' % gal.relevance)
    if gal.warp != warp:
        raise ValueError('link warp_s: the gallery has a window of %d frames, the link one of %d' % (gal.warp, warp))
    return _Options(model, gal, bool(link.get('enrol', True)), bool(link.get('exclusive', True)), warp)


@contextlib.contextmanager
def _einval_is_value_error():
    """An argument the library refuses is the caller's: ValueError with the library's text."""
    try:
        yield
    except hipabi.SpkdError as e:
        if e.status == hipabi.SPKD_EINVAL:
            raise ValueError(str(e))
        raise


def _finite(r):
    """After a chain's call (result r): the reference's error for values that are not finite."""
    if r['status'] == hipabi.SPKD_ENONFINITE:
        raise ValueError('array must not contain infs or NaNs')


def speech_runs(seg_off, begin, end):
    """The speech of every file as feature warping takes it (include/spkd.h, section 10b): a file's
    segment ranges (seg_off: the files' offsets among begin / end) sorted by their first frame, the
    overlapping and the touching ones merged into runs, an empty range dropped; the files in the order of
    their first run, so that the runs ascend over the whole list -> (set_off, run_begin, run_end), a set
    per file that has a frame.  Host-side numpy; the one place this is stated."""
    sets = []
    for f in range(len(seg_off) - 1):
        b, e = (np.asarray(a[seg_off[f]:seg_off[f + 1]], dtype=np.int64) for a in (begin, end))
        keep = e > b
        order = np.argsort(b[keep], kind='stable')
        b, e = b[keep][order], np.maximum.accumulate(e[keep][order])
        if len(b):
            first = np.concatenate([[True], b[1:] > e[:-1]])             # a range that starts past all before it
            sets.append((b[first], e[np.concatenate([first[1:], [True]])]))
    sets.sort(key=lambda be: int(be[0][0]))
    set_off = np.concatenate([[0], np.cumsum([len(b) for b, _ in sets])]).astype(np.int64)
    cat = lambda k: np.concatenate([be[k] for be in sets] + [np.zeros(0, dtype=np.int64)])
    return set_off, cat(0), cat(1)


def warp_frames(ctx, d_frames, total_frames, seg_off, begin, end, window, d_out=None):
    """The frames of the segments begin / end, warped file by file over `window` frames (speech_runs,
    spkd_feature_warp), into d_out -- None: the context's buffer 'link_warped', one more copy of the
    frames -> the device pointer.  A frame of no segment is not written."""
    if d_out is None:
        d_out = ctx.dev_scratch('link_warped', max(int(total_frames), 1) * hipabi.DIM * 4)
    set_off, run_b, run_e = speech_runs(seg_off, begin, end)
    with _einval_is_value_error():
        ctx.feature_warp(d_frames, total_frames, set_off, run_b, run_e, window, d_out)
    return d_out


def _bic_chain(ctx, link, d_stats, n_segments, member, set_off, clock):
    """The calls of link_batch without a model: the speakers' records as the sums of their segments'
    (spkd_sum_stats), one clustering problem of `link` -> (n_merges, a, b, d, stat_max, stat_min)."""
    n_spk = len(set_off) - 1
    d_spk = ctx.dev_scratch('link_speaker_stats', n_spk * hipabi.REC * 8)
    ctx.sum_stats(d_stats, n_segments, member, set_off, d_spk)
    clock('link_sum', 'reduce_sets')
    with _einval_is_value_error():
        r = ctx.ahc(d_spk, np.array([0, n_spk], dtype=np.int64), _ahc_params(link))
    clock('link_ahc', 'call')
    _finite(r)
    nm = int(r['n_merges'][0])
    return nm, r['a'][:nm], r['b'][:nm], r['d'][:nm], float(r['stat_max'][0]), float(r['stat_min'][0])


def _clr_chain(ctx, opts, set_off, rng_b, rng_e, d_frames, total_frames, clock, kept):
    """The calls of link_batch under model 'clr' -> (n_merges, a, b, d, stat_max, stat_min), or None
    when no background model could be trained.  With a gallery its model is the background model --
    trained here, as without a gallery, when it has none yet.  kept: a dict that receives the speakers'
    records (d_bw) and their flags (ok)."""
    m, gallery = opts.model, opts.gallery
    n_spk = len(set_off) - 1
    with _einval_is_value_error():
        if n_spk > hipabi.CLR_MAX_N:
            raise ValueError('clr_link: at most %d speakers' % hipabi.CLR_MAX_N)
        trained = None
        if gallery is None:
            d_ubm = ctx.dev_scratch('link_ubm', m.components * hipabi.GMM_COMP * 8)
            trained = train_ubm(ctx, d_frames, total_frames, d_ubm, m.components, set_off, rng_b, rng_e, m.iterations,
                                m.var_floor, m.ubm_max_frames)
        elif gallery.ubm is None:
            trained = gallery.train_ubm(d_frames, total_frames, set_off, rng_b, rng_e, m.iterations, m.var_floor,
                                        m.ubm_max_frames)
        if trained is not None:
            clock('link_ubm_train', 'gmm_train')
            if not trained:
                return None
        if gallery is not None:
            d_ubm = gallery.d_ubm
        d_bw = ctx.dev_scratch('link_speaker_bw', n_spk * m.components * hipabi.BW_COMP * 8)
        spk_ok = ctx.ubm_stats(d_frames, total_frames, d_ubm, m.components, set_off, rng_b, rng_e, d_bw)
        clock('link_ubm_stats', 'ubm_stats')
        kept.update(d_bw=d_bw, ok=spk_ok)
        r = ctx.clr_link(d_bw, spk_ok, d_ubm, m.components, m.relevance, m.threshold, m.max_spk)
        clock('link_clr', 'clr_link')
        _finite(r)
        return r['n_merges'], r['a'], r['b'], r['d'], r['stat_max'], r['stat_min']


def _identify_clusters(ctx, opts, kept, glob, clock, detail):
    """The gallery step of link_batch: the batch clusters of the chain (glob: the 1-based cluster of each
    speaker) get their records, are identified against the gallery as ONE group and are labelled by
    identity -> the global label of each speaker."""
    gallery = opts.gallery
    n_spk, n_cl = len(glob), int(glob.max())
    member = np.argsort(glob, kind='stable')                             # a cluster's speakers in ascending order
    set_off = np.concatenate([[0], np.cumsum(np.bincount(glob - 1, minlength=n_cl))])
    cl_ok = np.minimum.reduceat(np.asarray(kept['ok'], dtype=np.int32)[member], set_off[:-1]).astype(np.int32)
    d_cl = ctx.dev_scratch('link_cluster_bw', n_cl * gallery.record_doubles * 8)
    ctx.bw_accumulate(kept['d_bw'], n_spk, gallery.components, set_off, member, np.arange(n_cl), np.zeros(n_cl), d_cl, n_cl)
    clock('link_cluster_sum', 'bw_accumulate')
    r = gallery.identify(d_cl, cl_ok, [0, n_cl], opts.exclusive)
    clock('link_ident', *(('ident_scores', 'ident_assign') if gallery.n else ()))
    n_before = gallery.n
    ident = r['ident'].astype(np.int64)
    unknown = np.nonzero((cl_ok != 0) & (ident < 0))[0]
    label = ident + 1
    label[unknown] = n_before + 1 + np.arange(len(unknown))
    bad = np.nonzero(cl_ok == 0)[0]                                      # (no record: a label that stands for nobody)
    label[bad] = n_before + len(unknown) + 1 + np.arange(len(bad))
    enrolled = []
    if opts.enrol:
        after = gallery.update(d_cl, cl_ok, ident)
        enrolled = after[unknown].tolist()
        ident = after.astype(np.int64)
    clock('link_update', *(('bw_accumulate',) if opts.enrol and (cl_ok != 0).any() else ()))
    if detail is not None:
        detail.update(identity=ident.astype(np.int32), score=r['score'], second=r['second'], enrolled=enrolled)
    return label[glob - 1].astype(np.int32)


def link_batch(ctx, d_stats, seg_off, labels, link=LINK_CL, timings=None, d_frames=None, total_frames=None,
               files=None, segments=None, rate=125.0, detail=None):
    """Which speaker of one file is which speaker of another: spk_cluster_hi over the speakers of
    all files of a batch (spk-clustering.py:178-240 takes `speakers` of any length per entry; the
    command line never gets there, :289).  d_stats, seg_off: the segment records and the files'
    offsets as segment_stats leaves them (cluster_batch's stats_out); labels: per file the labels
    cluster_batch returned.  The speakers (link_speakers) get their records as the sums of their
    segments' records, in segment order (spkd_sum_stats: no frame is read again), and are one
    clustering problem of `link` (the keys of DIA2_CL).
    Returns (maps, merges, stat_max, stat_min): maps[f][l] is the global 1-based speaker of label
    l of file f (0 for a label no segment carries; length 0 for a file without segments), merges
    the log [(a, b, d)] over the speaker list, stat_max / stat_min as spkd_ahc states them.
    More than 16 384 speakers: ValueError.  timings: link_sum (the sum kernel, ms), link_ahc (the
    clustering call, ms), link_speakers, link_merges.
    link['model'] = 'clr' (LINK_CLR): the speakers are compared by cross-likelihood ratio under a
    universal background model instead -- one Gaussian is the wrong model of a whole speaker, whose
    frames fall into several modes in shares that differ from file to file.  This mode trains and
    scores on frames: it takes d_frames, total_frames, files, segments (the arrays cluster_batch took;
    the ranges are the ones segment_stats summed) and rate; d_stats is not read.  A speaker's frames
    are those of its segments in member order.  The background model is spkd_gmm_train's model of ONE
    speaker that owns the ranges of all speakers in speaker order (cut by ubm_ranges beyond
    link['ubm_max_frames'] frames); spkd_ubm_stats gives every speaker's record under it from all its
    frames, spkd_clr_link walks the chain.  Same return; stat_max / stat_min are the extremes of the
    initial ratios.  When no background model can be trained (too few frames, constant or non-finite
    frames) every speaker keeps a global label of its own and merges = [].  More than 4 096 speakers,
    a key out of range, a missing array: ValueError.  timings: link_ubm_train, link_ubm_stats,
    link_clr (kernel ms), link_speakers, link_merges.
    link['warp_s'] (LINK_CLR_WARP; model 'clr' only): the frames are feature-warped first, file by file
    over round(warp_s * rate) frames of the file's speech -- its segment ranges, sorted and merged into
    runs (speech_runs) -- by spkd_feature_warp; the background model, the statistics and a gallery's
    training then read the warped frames.  They are written to a buffer the context keeps
    ('link_warped'): device memory for one more copy of the frames, total_frames * 156 bytes.  A window
    outside [2, 512] frames: ValueError.  With a gallery the window must be the gallery's.  timings gain
    link_warp (kernel ms).  LINK_CLR_WARP's threshold, like LINK_CLR's, rests on a synthetic fixture.
    A link dictionary of model 'clr' may carry gallery=<gallery.Gallery>, enrol (default True) and
    exclusive (default True); the global labels then mean the same person in every batch.  The
    gallery's model is the background model: it is trained on this batch, as above, only when the
    gallery has none yet, and link['components'] and link['relevance'] must equal the gallery's
    (ValueError).  The statistics and the chain run within the batch as above.  The records of the
    resulting batch clusters are the sums of their speakers' records in ascending speaker order
    (spkd_bw_accumulate); the clusters are identified against the gallery as ONE group
    (Gallery.identify with the gallery's threshold: the chain declined to merge them, so they are
    distinct people, and under `exclusive` they get distinct identities).  The global label of a
    cluster is its identity's index + 1.  With enrol the unknown clusters are appended to the gallery
    in cluster order and the matched identities take the cluster's record (Gallery.update); without it
    the gallery is left untouched and the k-th unknown cluster is labelled gallery.n + 1 + k -- the
    label it would have got.  (A cluster without a usable record is labelled behind those; its label
    stands for nobody.)  maps, merges, stat_max and stat_min as above; detail: a dict that receives
    identity, score and second per batch cluster (Gallery.identify's, identity after enrolment) and
    enrolled, the new identities.  timings gain link_cluster_sum, link_ident (both identify kernels,
    ms) and link_update.  When no background model can be trained the fallback is the one above and
    the gallery is unchanged.  The identification threshold, like LINK_CLR's, rests on a synthetic
    fixture and not on speech."""
    opts = _link_options(link, rate)
    clr = opts.model.name == 'clr'
    if clr:
        if d_frames is None or total_frames is None or files is None or segments is None:
            raise ValueError('link model clr trains on the frames: it takes d_frames, total_frames, files and '
                             'segments, the arrays cluster_batch took')
        if len(segments) != len(files):
            raise ValueError('one segment array per file')
        seg_off_s, _, seg_b, seg_e = _segment_ranges(files, segments, float(rate))
        if seg_off_s.tolist() != np.asarray(seg_off, dtype=np.int64).tolist():
            raise ValueError('segments: one per label, file by file')
    member, set_off, spk_file, spk_label = link_speakers(seg_off, labels)
    n_spk = len(spk_file)
    maps = [np.zeros(int(np.max(l)) + 1 if len(l) else 0, dtype=np.int32) for l in labels]
    if n_spk == 0:
        return maps, [], float('nan'), float('nan')

    def clock(key, *which):
        """timings[key] gains the context's time of the calls `which`, 0.0 when none ran."""
        if timings is not None:
            timings.setdefault(key, []).append(sum((ctx.last_ms(w) for w in which), 0.0))

    kept = {}
    if clr and opts.warp:
        d_frames = warp_frames(ctx, d_frames, total_frames, seg_off_s, seg_b, seg_e, opts.warp)
        clock('link_warp', 'feature_warp')
    if clr:
        chain = _clr_chain(ctx, opts, set_off, seg_b[member], seg_e[member], d_frames, total_frames, clock, kept)
    else:
        chain = _bic_chain(ctx, link, d_stats, int(seg_off[-1]), member, set_off, clock)
    nm, a, b, d, smax, smin = chain if chain is not None else (0, [], [], [], float('nan'), float('nan'))
    if timings is not None:
        timings['link_speakers'] = n_spk
        timings['link_merges'] = nm
    glob = hipabi.labels_from_merges(n_spk, a, b)
    if opts.gallery is not None and chain is not None:
        with _einval_is_value_error():
            glob = _identify_clusters(ctx, opts, kept, glob, clock, detail)
    for f, l, g in zip(spk_file.tolist(), spk_label.tolist(), glob.tolist()):
        maps[f][l] = g
    return maps, list(zip(np.asarray(a).tolist(), np.asarray(b).tolist(), np.asarray(d).tolist())), smax, smin
