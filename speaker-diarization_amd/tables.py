"""The tables every stage of the batch pipeline reads: a file of the batch (BatchFile), its turns and its
segments as absolute frame ranges (_turn_table, _segment_ranges), the speakers clustering left
(link_speakers) and the clustering parameters of a `cl` dictionary (_ahc_params).  The lowest layer of the
package's stages: it imports hipabi only; clr_model, gallery, resegmentation, linking and pipeline stand on
it, and pipeline offers every name here under its own."""
import numpy as np

from . import hipabi


class BatchFile(object):
    """One file of a batch: frame window in the resident array + its VAD turns
    (start / end seconds as the VAD recipe states them)."""

    def __init__(self, frame_off, n_frames, vad):
        self.frame_off = int(frame_off)
        self.n_frames = int(n_frames)
        self.vad = [(float(s), float(e)) for (s, e) in vad]
        self.vad_arr = np.array(self.vad, dtype=np.float64).reshape(-1, 2)     # (converted once, not per call)


def _turn_table(files, rate):
    """Per VAD turn of the batch, in file order: owning file, that file's offset and length in
    the resident array, start / end seconds (views), absolute frame range -- int() truncation
    and the clamp of a slice (no lower clamp: spk-change-detection.py cuts feas[start:end]).
    None when no file has a turn."""
    nturn = [len(f.vad) for f in files]
    if sum(nturn) == 0:
        return None
    vad = np.concatenate([f.vad_arr for f in files])
    owner = np.repeat(np.arange(len(files)), nturn)
    foff = np.array([f.frame_off for f in files], dtype=np.int64)[owner]
    fn = np.array([f.n_frames for f in files], dtype=np.int64)[owner]
    ls, le = vad[:, 0], vad[:, 1]
    f0 = np.minimum((ls * rate).astype(np.int64), fn)
    f1 = np.maximum(f0, np.minimum((le * rate).astype(np.int64), fn))
    return owner, foff, fn, ls, le, foff + f0, foff + f1


def _segment_ranges(files, segments, rate):
    """The absolute frame range of every segment of a batch, in segment order (get_spk_features,
    spk-clustering.py:46-52: int() truncation, the clamps of a slice) -> (seg_off per file, n,
    begin, end)."""
    cnt = [len(s) for s in segments]
    seg_off = np.zeros(len(files) + 1, dtype=np.int64)
    seg_off[1:] = np.cumsum(cnt)
    n = int(seg_off[-1])
    allseg = np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1, 2) for s in segments]) if n else np.zeros((0, 2))
    owner = np.repeat(np.arange(len(files)), cnt)
    foff = np.array([f.frame_off for f in files], dtype=np.int64)[owner]
    fn = np.array([f.n_frames for f in files], dtype=np.int64)[owner]
    a0 = np.clip((allseg[:, 0] * rate).astype(np.int64), 0, fn)
    a1 = np.maximum(a0, np.clip((allseg[:, 1] * rate).astype(np.int64), 0, fn))
    return seg_off, n, foff + a0, foff + a1


def _ahc_params(cl):
    return hipabi.AhcParams(cl['variant'], hipabi.KINDS[cl['kind']], cl['max_spk'], cl.get('path', 0),
                            cl['lambdac'], cl['threshold'])


def link_speakers(seg_off, labels):
    """The initial speakers of a batch's linking problem: the clusters of its files, file by file
    and within a file by ascending label -- the list the reference would hold had every file's
    final `speakers` been concatenated.  A label no segment carries is no speaker.  labels: per
    file the 1-based label of each of its segments (seg_off: the files' offsets among all
    segments).  Returns (member, set_off, spk_file, spk_label): speaker s owns the segments
    member[set_off[s]:set_off[s + 1]], in segment order, and is label spk_label[s] of file
    spk_file[s]."""
    seg_off = np.asarray(seg_off, dtype=np.int64)
    if len(labels) != len(seg_off) - 1:
        raise ValueError('one label array per file')
    labs = [np.asarray(l, dtype=np.int64).reshape(-1) for l in labels]
    if [len(l) for l in labs] != np.diff(seg_off).tolist():
        raise ValueError('one label per segment')
    lab = np.concatenate(labs) if labs else np.zeros(0, dtype=np.int64)
    if len(lab) == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, np.zeros(1, dtype=np.int64), z, z
    if int(lab.min()) < 1:
        raise ValueError('labels are 1-based')
    owner = np.repeat(np.arange(len(labs), dtype=np.int64), [len(l) for l in labs])
    width = int(lab.max()) + 1
    keys, spk = np.unique(owner * width + lab, return_inverse=True)
    member = np.argsort(spk, kind='stable').astype(np.int64)
    set_off = np.zeros(len(keys) + 1, dtype=np.int64)
    set_off[1:] = np.cumsum(np.bincount(spk, minlength=len(keys)))
    return member, set_off, keys // width, keys % width
