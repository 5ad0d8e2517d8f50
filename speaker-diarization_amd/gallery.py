"""A gallery of enrolled speakers: the records of linking by cross-likelihood ratio (clr_model.LINK_CLR,
spkd_ubm_stats) kept on the device from one batch to the next, so that a global speaker label means
the same person in every batch and known voices can be enrolled by name.

The gallery owns the universal background model: records are comparable only under the model they
were collected under.  Identification is spkd_clr_identify (an open-set decision with a one-to-one
constraint inside a group of probes), enrolment and the growth of an identity are spkd_bw_accumulate.
PARITY: no reference counterpart (spk-clustering.py:289 is a TODO for more than one wav);
tests/gallery_numpy.py restates the flow in numpy.

The default threshold is LINK_CLR's.  Like it, it rests on ONE synthetic fixture (tests/test_gallery.py),
not on speech: tune it on real audio.

Layers: this module stands on clr_model (the CLR settings, their parser, the training of the background
model) and hipabi; linking and pipeline stand on it.
"""
import numpy as np

from . import hipabi
from .clr_model import LINK_CLR, _link_model, train_ubm, warp_window

FORMAT_VERSION = 1
_KEYS = ('version', 'components', 'relevance', 'threshold', 'ubm', 'records', 'ok', 'frames', 'names')


def default_name(index):
    return 'spk_%d' % (index + 1)


class Gallery(object):
    """State: the UBM (`ubm`, a host copy [components, GMM_COMP], and `d_ubm` on the device; None
    without a model), `components`, `relevance`, `threshold`, the records of the `n` identities in
    one device buffer `d_bw` that grows by doubling, and per identity `ok`, the frame total `N` (the
    sum of n_c over what was added to it) and `names`; `warp`, the feature-warping window in frames its
    records were collected under (link['warp_s'] at `rate`; 0: none) -- records of warped and of plain
    frames do not compare, so link_batch refuses a link of another window.  ctx=None: a gallery of host
    arrays only (to_arrays / from_arrays / save / load work, nothing that needs the device does)."""

    def __init__(self, ctx, link=None, rate=125.0):
        model = _link_model(LINK_CLR if link is None else link)
        if model.name != 'clr':
            raise ValueError('a gallery holds the records of link model clr')
        self.warp = warp_window(LINK_CLR if link is None else link, rate)
        self.components, self.iterations, self.var_floor = model.components, model.iterations, model.var_floor
        self.relevance, self.threshold, self.ubm_max_frames = model.relevance, model.threshold, model.ubm_max_frames
        self.ctx = ctx
        self.ubm, self.d_ubm = None, None
        self.d_bw, self._cap, self._host = None, 0, None
        self.n = 0
        self.ok = np.zeros(0, dtype=np.int32)
        self.N = np.zeros(0, dtype=np.float64)
        self.names = []

    # ---- the model
    @property
    def record_doubles(self):
        return self.components * hipabi.BW_COMP

    def _no_identity(self, what):
        if self.n:
            raise ValueError('%s: the gallery holds identities, whose records rest on its model' % what)

    def set_ubm(self, model):
        """The background model [components, GMM_COMP] as spkd_gmm_train leaves one; only while the
        gallery holds no identity."""
        self._no_identity('set_ubm')
        model = np.ascontiguousarray(model, dtype=np.float64)
        if model.shape != (self.components, hipabi.GMM_COMP):
            raise ValueError('set_ubm: a model of %d components of %d doubles' % (self.components, hipabi.GMM_COMP))
        self.ubm = model.copy()
        if self.ctx is not None:
            if self.d_ubm is None:
                self.d_ubm = self.ctx.dev_alloc(model.nbytes)
            self.ctx.h2d(self.d_ubm, self.ubm)

    def train_ubm(self, d_frames, total_frames, set_off, begin, end, iterations=None, var_floor=None,
                  ubm_max_frames=None):
        """Trains the model by the call link_batch makes under LINK_CLR (clr_model.train_ubm) on the
        ranges begin / end of all speakers (set_off: the speakers' offsets among them); a setting that
        is None is the gallery's own.  Only while the gallery holds no identity.  Returns False, and
        leaves the gallery without a model, when none can be trained."""
        self._no_identity('train_ubm')
        it = self.iterations if iterations is None else iterations
        fl = self.var_floor if var_floor is None else var_floor
        cap = self.ubm_max_frames if ubm_max_frames is None else ubm_max_frames
        if self.d_ubm is None:
            self.d_ubm = self.ctx.dev_alloc(self.components * hipabi.GMM_COMP * 8)
        self.ubm = None
        if not train_ubm(self.ctx, d_frames, total_frames, self.d_ubm, self.components, set_off, begin, end, it, fl, cap):
            return False
        self.ubm = np.empty((self.components, hipabi.GMM_COMP))
        self.ctx.d2h(self.ubm, self.d_ubm)
        return True

    # ---- the records
    def _reserve(self, n):
        """Room for n records on the device: the buffer doubles, what it holds moves along."""
        if n <= self._cap:
            return
        cap = max(self._cap, 16)
        while cap < n:
            cap *= 2
        cap = min(cap, hipabi.GALLERY_MAX_N)
        d_new = self.ctx.dev_alloc(cap * self.record_doubles * 8)
        if self.n:
            self.ctx.copy_d2d(d_new, self.d_bw, self.n * self.record_doubles * 8)
        if self.d_bw is not None:
            self.ctx.dev_free(self.d_bw)
        self.d_bw, self._cap = d_new, cap

    def records(self):
        """The records of the identities on the host, [n, components, BW_COMP]."""
        if self.ctx is None:
            return (self._host if self._host is not None else np.zeros((0, self.components, hipabi.BW_COMP))).copy()
        out = np.empty((self.n, self.components, hipabi.BW_COMP))
        if self.n:
            self.ctx.d2h(out, self.d_bw)
        return out

    def identify(self, d_bw, ok, group_off, exclusive=True, threshold=None):
        """The records at d_bw (one per flag of ok, collected under THIS gallery's model) against the
        identities: hipabi.Context.clr_identify with the gallery's relevance and, unless one is given,
        its threshold.  Returns dict(ident, score, second)."""
        if self.ubm is None:
            raise ValueError('identify: the gallery has no model (set_ubm, train_ubm)')
        th = self.threshold if threshold is None else float(threshold)
        r = self.ctx.clr_identify(d_bw, ok, group_off, self.d_bw, self.ok, self.d_ubm, self.components, self.relevance,
                                  th, exclusive)
        if r['status'] == hipabi.SPKD_ENONFINITE:
            raise ValueError('array must not contain infs or NaNs')
        return dict(ident=r['ident'], score=r['score'], second=r['second'])

    def update(self, d_bw, ok, ident, names=None):
        """Adds the record of each matched probe (ok, ident >= 0) to its identity, in ascending probe
        order, and appends every unknown ok probe (ident < 0) as a new identity, in probe order.
        names: per probe the name of the identity it founds (None: 'spk_<index + 1>').  Returns the
        identity of every probe, -1 for a probe that is not ok.  More than GALLERY_MAX_N identities:
        ValueError before anything is changed."""
        if self.ubm is None:
            raise ValueError('update: the gallery has no model (set_ubm, train_ubm)')
        ok = np.asarray(ok, dtype=np.int32).reshape(-1)
        ident = np.asarray(ident, dtype=np.int64).reshape(-1)
        if len(ident) != len(ok) or (names is not None and len(names) != len(ok)):
            raise ValueError('update: one flag, one identity and one name per probe')
        good = ok != 0
        if (ident[good] >= self.n).any():
            raise ValueError('update: an identity the gallery does not hold')
        new = np.nonzero(good & (ident < 0))[0]
        if self.n + len(new) > hipabi.GALLERY_MAX_N:
            raise ValueError('update: at most %d identities' % hipabi.GALLERY_MAX_N)
        out = np.where(good, ident, -1).astype(np.int32)
        out[new] = self.n + np.arange(len(new))
        if not good.any():
            return out
        # one set per identity that takes a record: its probes in ascending order
        order = np.argsort(out[good], kind='stable')
        member = np.nonzero(good)[0][order]
        slots, counts = np.unique(out[member], return_counts=True)
        set_off = np.concatenate([[0], np.cumsum(counts)])
        n_after = self.n + len(new)
        self._reserve(n_after)
        self.ctx.bw_accumulate(d_bw, len(ok), self.components, set_off, member, slots, slots < self.n, self.d_bw, n_after)
        rec = np.empty((len(ok), self.components, hipabi.BW_COMP))
        self.ctx.d2h(rec, d_bw)
        self.ok = np.concatenate([self.ok, np.ones(len(new), dtype=np.int32)])
        self.N = np.concatenate([self.N, np.zeros(len(new))])
        for s in member.tolist():
            self.N[out[s]] += rec[s, :, 0].sum()
        for s in new.tolist():
            given = None if names is None else names[s]
            self.names.append(default_name(len(self.names)) if given is None else str(given))
        self.n = n_after
        return out

    # ---- the host side
    def to_arrays(self):
        """The gallery as a dictionary of numpy arrays (what save writes).  `warp` is among them only when
        the gallery has a window: one without saves to the keys and bytes it always had."""
        warp = dict(warp=np.array(self.warp, dtype=np.int64)) if self.warp else {}
        return dict(version=np.array(FORMAT_VERSION, dtype=np.int64), components=np.array(self.components, dtype=np.int64),
                    relevance=np.array(self.relevance, dtype=np.float64), threshold=np.array(self.threshold, dtype=np.float64),
                    ubm=(np.zeros((0, hipabi.GMM_COMP)) if self.ubm is None else self.ubm.copy()),
                    records=self.records(), ok=self.ok.astype(np.int32), frames=self.N.astype(np.float64),
                    names=np.array(self.names, dtype=np.str_).reshape(len(self.names)), **warp)

    @classmethod
    def from_arrays(cls, ctx, arrays):
        """A gallery from what to_arrays gave.  Another format version, a key that is missing, shapes
        that disagree: ValueError.  No `warp` among them: a gallery without a window."""
        missing = [k for k in _KEYS if k not in arrays]
        if missing:
            raise ValueError('gallery: no %s' % ', '.join(missing))
        a = {k: np.asarray(arrays[k]) for k in _KEYS}
        if a['version'].shape != () or int(a['version']) != FORMAT_VERSION:
            raise ValueError('gallery: format version %s, not %d' % (a['version'], FORMAT_VERSION))
        if any(a[k].shape != () for k in ('components', 'relevance', 'threshold')):
            raise ValueError('gallery: components, relevance and threshold are scalars')
        g = cls(ctx, dict(LINK_CLR, components=int(a['components']), relevance=float(a['relevance']),
                          threshold=float(a['threshold'])))
        warp = np.asarray(arrays['warp']) if 'warp' in arrays else np.array(0)
        if warp.shape != () or warp.dtype.kind not in 'iu' or not (warp == 0 or 2 <= warp <= hipabi.WARP_MAX_WINDOW):
            raise ValueError('gallery: warp is a scalar, 0 or a window of 2 .. %d frames' % hipabi.WARP_MAX_WINDOW)
        g.warp = int(warp)
        k, n = g.components, len(a['ok'])
        if a['records'].shape != (n, k, hipabi.BW_COMP) or a['ok'].shape != (n,) or a['frames'].shape != (n,) or \
                a['names'].shape != (n,) or a['ubm'].shape not in ((0, hipabi.GMM_COMP), (k, hipabi.GMM_COMP)):
            raise ValueError('gallery: the shapes of ubm, records, ok, frames and names disagree')
        if n > hipabi.GALLERY_MAX_N:
            raise ValueError('gallery: at most %d identities' % hipabi.GALLERY_MAX_N)
        if n and not len(a['ubm']):
            raise ValueError('gallery: identities without a model')
        if len(a['ubm']):
            g.set_ubm(a['ubm'].astype(np.float64))
        rec = np.ascontiguousarray(a['records'], dtype=np.float64)
        if ctx is None:
            g._host = rec.copy()
        elif n:
            g._reserve(n)
            ctx.h2d(g.d_bw, rec)
        g.n = n
        g.ok = a['ok'].astype(np.int32)
        g.N = a['frames'].astype(np.float64)
        g.names = [str(x) for x in a['names'].tolist()]
        return g

    def save(self, path):
        """One .npz (no pickled object in it): the format version, the parameters, the model, the
        records, ok, the frame totals and the names."""
        with open(path, 'wb') as f:
            np.savez(f, **self.to_arrays())

    @classmethod
    def load(cls, ctx, path):
        with np.load(path, allow_pickle=False) as z:
            return cls.from_arrays(ctx, {k: z[k] for k in z.files})

    def close(self):
        """Frees the device buffers."""
        if self.ctx is not None:
            for p in (self.d_bw, self.d_ubm):
                if p is not None:
                    self.ctx.dev_free(p)
        self.d_bw, self.d_ubm, self._cap = None, None, 0
