"""The grow-only pinned and scratch slots behind the C ABI's mirrored tables and result blocks, reused
across calls of different sizes (run with -m gpu on an MI355X).  On one context every call that sends a
table up or brings a block down through them runs at a small size, at a larger one (its slots grow) and
at the small one again (the images are placed in slots larger than they need); what the third run hands
back, on the host and on the device, has the bits of the same calls on a fresh context.

The sizes misalign what they can: 3 and 5 speakers, so that an int32 tail of odd length stands in front
of a double part or of the next image; sequences of 70 and 130 frames against the 64-frame tiles; 2
components, 2 EM steps; a gallery of 3 against 5 probes in 2 groups."""
import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

K_MAX = 5
N_COMP = 2
N_ITER = 2
LENS = (70, 130)


def _shape(k):
    """k speakers, each with a range of 70 and one of 130 frames (they overlap: nothing here asks them not to)."""
    b = np.array([37 * s for s in range(k)] + [200 + 41 * s for s in range(k)], dtype=np.int64)
    e = b + np.repeat(np.array(LENS, dtype=np.int64), k)
    order = np.arange(2 * k).reshape(2, k).T.ravel()              # speaker s: ranges s and k + s
    return b, e, order


def _run(ctx, hipabi, d, n_frames, k):
    """Every converted call once at size k -> {name: bytes of what came back}.  Device outputs are
    overwritten with 0xff first, so that nothing an earlier run left there can pass for a result."""
    out = {}
    b, e, order = _shape(k)
    rows = int((e - b).sum())

    def fetch(name, ptr, shape, dtype):
        a = np.empty(shape, dtype=dtype)
        ctx.d2h(a, ptr)
        out[name] = a.tobytes()
        return a

    def poison(ptr, nbytes):
        ctx.h2d(ptr, np.full(nbytes, 0xff, dtype=np.uint8))

    # sum_stats: a record per range, a speaker's record the sum of its two
    ctx.set_stats(d['frames'], n_frames, b, e, np.arange(2 * k, dtype=np.int32), 2 * k, d['range_stats'])
    poison(d['stats'], k * hipabi.REC * 8)
    ctx.sum_stats(d['range_stats'], 2 * k, order, 2 * np.arange(k + 1), d['stats'])
    fetch('sum_stats', d['stats'], (k, hipabi.REC), np.float64)

    # gauss_loglik: every range a sequence under all k models
    ok = ctx.gauss_models(d['stats'], k, d['models'])
    assert ok.all()
    seq = (b, e, np.zeros(2 * k, dtype=np.int32), np.full(2 * k, k, dtype=np.int32))
    poison(d['scores'], rows * k * 4)
    frame_off = ctx.gauss_loglik(d['frames'], n_frames, d['models'], ok, *seq, k, d['scores'])
    fetch('gauss_loglik', d['scores'], (rows, k), np.float32)

    # fb_posterior_batch with tokens: two per sequence, the second from frame 35 on
    tok_off = 2 * np.arange(2 * k + 1)
    tok_frame = np.tile(np.array([0, 35], dtype=np.int64), 2 * k)
    tok_word = np.tile(np.array([0, 1], dtype=np.int32), 2 * k)
    poison(d['post'], rows * k * 4)
    conf, logz = ctx.fb_posterior_batch(d['scores'], frame_off, k, 2.0, tokens=(tok_off, tok_frame, tok_word), d_post=d['post'])
    out['fb_posterior_batch conf'], out['fb_posterior_batch logz'] = conf.tobytes(), logz.tobytes()
    fetch('fb_posterior_batch post', d['post'], (rows, k), np.float32)

    # post_stats
    poison(d['post_stats'], k * hipabi.REC * 8)
    ctx.post_stats(d['frames'], n_frames, d['post'], *seq, k, k, d['post_stats'], masses=False)
    fetch('post_stats', d['post_stats'], (k, hipabi.REC), np.float64)

    # gmm_train, gmm_loglik_seq
    sets = (2 * np.arange(k + 1), b[order], e[order])
    poison(d['gmm'], k * N_COMP * hipabi.GMM_COMP * 8)
    gok, ll = ctx.gmm_train(d['frames'], n_frames, *sets, N_COMP, N_ITER, 0.01, d['gmm'])
    assert gok.all()
    out['gmm_train ok'], out['gmm_train loglik'] = gok.tobytes(), ll.tobytes()
    fetch('gmm_train models', d['gmm'], (k, N_COMP, hipabi.GMM_COMP), np.float64)
    poison(d['scores'], rows * k * 4)
    ctx.gmm_loglik_seq(d['frames'], n_frames, d['gmm'], N_COMP, gok, *seq, k, d['scores'])
    fetch('gmm_loglik_seq', d['scores'], (rows, k), np.float32)

    # ubm_stats, clr_link
    poison(d['bw'], k * N_COMP * hipabi.BW_COMP * 8)
    bok = ctx.ubm_stats(d['frames'], n_frames, d['ubm'], N_COMP, *sets, d['bw'])
    assert bok.all()
    out['ubm_stats ok'] = bok.tobytes()
    fetch('ubm_stats records', d['bw'], (k, N_COMP, hipabi.BW_COMP), np.float64)
    link = ctx.clr_link(d['bw'], bok, d['ubm'], N_COMP, 16.0, 0.0, max_spk=1)
    assert link['status'] == hipabi.SPKD_OK and link['n_merges'] == k - 1
    out['clr_link'] = b''.join(np.asarray(link[key]).tobytes() for key in ('a', 'b', 'd', 'stat_max', 'stat_min'))

    # clr_identify with `exclusive`: the k speakers in 2 groups against the first 8 - k enrolled ones
    n_gal = 8 - k
    poison(d['id_scores'], k * n_gal * 8)
    ident = ctx.clr_identify(d['bw'], bok, [0, 2, k], d['gallery'], np.ones(n_gal, dtype=np.int32), d['ubm'], N_COMP, 16.0,
                             -1e30, exclusive=True, d_scores=d['id_scores'])
    assert ident['status'] == hipabi.SPKD_OK and (ident['ident'] >= 0).all()
    out['clr_identify'] = b''.join(ident[key].tobytes() for key in ('ident', 'score', 'second'))
    fetch('clr_identify scores', d['id_scores'], (k, n_gal), np.float64)

    # bw_accumulate: set j is the records j and j + 1 (cyclically), into slot k - 1 - j, every other one kept
    ctx.h2d(d['acc'], np.arange(k * N_COMP * hipabi.BW_COMP, dtype=np.float64))
    member = np.stack([np.arange(k), (np.arange(k) + 1) % k], axis=1).ravel()
    ctx.bw_accumulate(d['bw'], k, N_COMP, 2 * np.arange(k + 1), member, np.arange(k)[::-1], np.arange(k) % 2, d['acc'], k)
    fetch('bw_accumulate', d['acc'], (k, N_COMP, hipabi.BW_COMP), np.float64)
    return out


def test_slots_that_grew_hand_back_what_a_fresh_context_does():
    hipabi = pkg('hipabi')
    synth = pkg('synth')
    feats, _, _ = synth.make_session(20261019, 6, 3)
    feats = np.ascontiguousarray(feats, dtype=np.float32)
    n_frames = feats.shape[0]
    b, e, _ = _shape(K_MAX)
    assert n_frames < 1000 and e.max() + 11 <= n_frames
    rows = int((e - b).sum())
    sizes = dict(frames=feats.nbytes, range_stats=2 * K_MAX * hipabi.REC * 8, stats=K_MAX * hipabi.REC * 8,
                 models=K_MAX * hipabi.GAUSS_MODEL * 8, scores=rows * K_MAX * 4, post=rows * K_MAX * 4,
                 post_stats=K_MAX * hipabi.REC * 8, gmm=K_MAX * N_COMP * hipabi.GMM_COMP * 8,
                 ubm=N_COMP * hipabi.GMM_COMP * 8, bw=K_MAX * N_COMP * hipabi.BW_COMP * 8,
                 gallery=K_MAX * N_COMP * hipabi.BW_COMP * 8, id_scores=K_MAX * K_MAX * 8,
                 acc=K_MAX * N_COMP * hipabi.BW_COMP * 8)
    ctx = hipabi.Context(0)
    fresh = None
    d = {}
    try:
        for name, nbytes in sizes.items():
            d[name] = ctx.dev_alloc(nbytes)
        ctx.h2d(d['frames'], feats)
        # the UBM over every frame, and the enrolled speakers: the larger shape's, shifted by 11 frames
        ok, _ = ctx.gmm_train(d['frames'], n_frames, [0, 1], [0], [n_frames], N_COMP, N_ITER, 0.01, d['ubm'])
        assert ok.all()
        _, _, order = _shape(K_MAX)
        assert ctx.ubm_stats(d['frames'], n_frames, d['ubm'], N_COMP, 2 * np.arange(K_MAX + 1), b[order] + 11, e[order] + 11,
                             d['gallery']).all()
        small = _run(ctx, hipabi, d, n_frames, 3)
        large = _run(ctx, hipabi, d, n_frames, K_MAX)
        again = _run(ctx, hipabi, d, n_frames, 3)
        fresh = hipabi.Context(0)
        want = _run(fresh, hipabi, d, n_frames, 3)
        assert sorted(again) == sorted(want) == sorted(large)
        for name in sorted(want):
            assert small[name] == want[name], name
            assert again[name] == want[name], name
        for ptr in d.values():
            ctx.dev_free(ptr)
    finally:
        if fresh is not None:
            fresh.close()
        ctx.close()
