"""The settings of linking by cross-likelihood ratio and the training of its universal background model:
LINK_CLR, the parser of a `link` dictionary's model keys (_link_model), the cut of the training frames
(ubm_ranges) and the one spelling of the training call (train_ubm); LINK_CLR_WARP and the parser of the
feature-warping key (warp_window).  Both the gallery, which owns a
background model, and linking, which refuses what is not a gallery.Gallery, need these four: they live
below both (this module imports hipabi only), linking offers them under its own name, pipeline under its."""
import collections

import numpy as np

from . import hipabi

# linking by cross-likelihood ratio (linking.link_batch, model 'clr'): a universal background model of
# `components` diagonal Gaussians trained on the speakers' own frames (spkd_gmm_train: `iterations` EM
# steps, `var_floor`; at most `ubm_max_frames` frames go in), every speaker's statistics under it
# (spkd_ubm_stats), means MAP-adapted with `relevance`, and the agglomerative chain of spkd_clr_link:
# merged while the ratio is above `threshold` (higher is more alike; max_spk as in LINK_CL).  The
# threshold rests on ONE synthetic fixture (tests/test_link_clr.py), not on speech: tune it on real audio.
LINK_CLR = dict(model='clr', components=8, iterations=5, var_floor=0.01, relevance=16.0,
                threshold=-0.5, max_spk=0, ubm_max_frames=2_000_000)

# LINK_CLR on warped features (spkd_feature_warp, include/spkd.h section 10b): over `warp_s` seconds of a file's
# speech every coefficient becomes the standard-normal quantile of its rank, which takes a per-dimension gain
# and offset -- another microphone -- out of the comparison.  Warped features compress the ratios, so the mode
# has a threshold of its own: -0.1 is the middle of the window [-0.28, 0.08] in which the ONE synthetic
# fixture (tests/test_feature_warp.py: the people of tests/test_link_clr.py, each file through a channel of
# its own) is linked correctly.  It is unmeasured on speech: tune it on real audio.
LINK_CLR_WARP = dict(LINK_CLR, warp_s=3.0, threshold=-0.1)

_Bic = collections.namedtuple('_Bic', 'name')
_Clr = collections.namedtuple('_Clr', 'name components iterations var_floor relevance threshold max_spk ubm_max_frames')


def _link_model(link):
    """The model of a `link` dictionary: ('bic',) when the key is absent -- the clustering keys of
    LINK_CL -- or ('clr', components, iterations, var_floor, relevance, threshold, max_spk,
    ubm_max_frames), the keys LINK_CLR names (its values where one is absent)."""
    if 'model' not in link:
        return _Bic('bic')
    if link['model'] != 'clr':
        raise ValueError('link model: clr (or no model: the clustering keys of LINK_CL)')
    get = lambda k: link.get(k, LINK_CLR[k])
    k, it, cap, ms = get('components'), get('iterations'), get('ubm_max_frames'), get('max_spk')
    fl, r, th = float(get('var_floor')), float(get('relevance')), float(get('threshold'))
    if int(k) != k or not 1 <= k <= hipabi.GMM_MAX_COMP:
        raise ValueError('link components: 1 .. %d' % hipabi.GMM_MAX_COMP)
    if int(it) != it or it < 0:
        raise ValueError('link iterations: an integer >= 0')
    if not np.isfinite(fl) or fl < 0.0:
        raise ValueError('link var_floor: a finite number >= 0 (a share of the variance of all the frames)')
    if not np.isfinite(r) or r <= 0.0:
        raise ValueError('link relevance: a finite number > 0')
    if not np.isfinite(th):
        raise ValueError('link threshold: a finite number (a ratio above it merges)')
    if int(ms) != ms or ms < 0:
        raise ValueError('link max_spk: an integer >= 0')
    if int(cap) != cap or cap < (hipabi.DIM + 1) * k:
        raise ValueError('link ubm_max_frames: an integer >= 40 per component')
    return _Clr('clr', int(k), int(it), fl, r, th, int(ms), int(cap))


def warp_window(link, rate):
    """The feature-warping window of a `link` dictionary in frames: round(link['warp_s'] * rate), 0 where
    the key is absent or 0.  Only model 'clr' takes the key."""
    w = link.get('warp_s', 0.0)
    try:
        w = float(w)
    except (TypeError, ValueError):
        w = float('nan')
    if not np.isfinite(w) or w < 0.0:
        raise ValueError('link warp_s: a finite number >= 0 (seconds of speech; 0: no warping)')
    if w == 0.0:
        return 0
    if link.get('model') != 'clr':
        raise ValueError('link warp_s: only link model clr warps its features')
    n = int(round(w * float(rate)))
    if not 2 <= n <= hipabi.WARP_MAX_WINDOW:
        raise ValueError('link warp_s: a window of 2 .. %d frames (%r s at %r frames a second are %d)'
                         % (hipabi.WARP_MAX_WINDOW, w, rate, n))
    return n


def ubm_ranges(set_off, begin, end, cap):
    """What the speakers give to the training of the background model: the ends of their ranges, cut.
    Speaker s owns the ranges set_off[s] .. set_off[s + 1] of begin / end, its frames numbered in that
    order.  While the speakers hold at most `cap` frames every range stays whole; beyond that speaker s
    gives its first floor(cap N_s / N_total) frames -- a range past them is left empty."""
    set_off, begin, end = (np.asarray(a, dtype=np.int64) for a in (set_off, begin, end))
    length = end - begin
    owner = np.repeat(np.arange(len(set_off) - 1), np.diff(set_off))
    n = np.zeros(len(set_off) - 1, dtype=np.int64)
    np.add.at(n, owner, length)
    total = int(n.sum())
    if total <= cap:
        return end.copy()
    share = np.array([int(cap) * int(k) // total for k in n], dtype=np.int64)
    before = np.concatenate([[0], np.cumsum(length)])[:-1]              # frames in the ranges before this one
    ord0 = before - before[set_off[:-1]][owner]                         # the ordinal of the range's first frame
    return begin + np.clip(share[owner] - ord0, 0, length)


def train_ubm(ctx, d_frames, total_frames, d_ubm, components, set_off, begin, end, iterations, var_floor, cap):
    """Trains the background model into the device buffer d_ubm: spkd_gmm_train's model of ONE speaker that
    owns the ranges begin / end of all speakers in speaker order (set_off: the speakers' offsets among
    them), cut by ubm_ranges beyond `cap` frames.  Returns whether a model was obtained; the call's time is
    the context's last_ms('gmm_train')."""
    ok, _ = ctx.gmm_train(d_frames, total_frames, [0, len(begin)], begin, ubm_ranges(set_off, begin, end, cap),
                          components, iterations, var_floor, d_ubm)
    return bool(ok[0])
