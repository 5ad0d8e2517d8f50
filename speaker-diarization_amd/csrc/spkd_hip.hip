// libspkd_hip.so — C ABI (include/spkd.h) over the HIP kernels.  gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <atomic>
#include <thread>
#include <vector>

#include "../../include/spkd.h"
#include "spkd_cd.hpp"
#include "spkd_cluster.hpp"
#include "spkd_device.hpp"
#include "spkd_handoff.hpp"
#include "spkd_merge.hpp"
#include "spkd_stats.hpp"
#include "spkd_post_stats.hpp"
#include "spkd_mfcc.hpp"
#include "spkd_mfcc_batch.hpp"
#include "spkd_resample.hpp"
#include "spkd_beamform.hpp"
#include "spkd_tdoa.hpp"
#include "spkd_seat.hpp"
#include "spkd_overlap.hpp"
#include "spkd_energy.hpp"
#include "spkd_vad.hpp"
#include "spkd_vad_batch.hpp"
#include "spkd_mindur.hpp"
#include "spkd_fb.hpp"
#include "spkd_gauss.hpp"
#include "spkd_gmm_train.hpp"
#include "spkd_ubm_stats.hpp"
#include "spkd_clr.hpp"
#include "spkd_warp.hpp"
#include "spkd_ident.hpp"

using namespace spkd;

namespace {
constexpr int N_SLOTS = 88;
// Pinned host buffers, each named where it is used (stage(), TokenHandBack, the batch hand-off).  A slot belongs
// to one block of one entry point: what a call leaves there for its caller (the hand-off's results, a decoder's
// tokens) stays valid until that entry point is called again, so two calls whose results can be live together
// never share a slot; nor do the block that goes up and the block that comes down in one call.
enum { PIN_GW_TURNS = 0, PIN_GW_LINES, PIN_AHC_OUT, PIN_VAD_FILES, PIN_VAD_TOKENS, PIN_SUM_IDX, PIN_GAUSS_IDX,
       PIN_GT_TAB, PIN_GT_OUT, PIN_GT_IDX, PIN_UBM_TAB, PIN_UBM_OUT, PIN_CLR_IN, PIN_CLR_OUT, PIN_MD_SEQS, PIN_MD_TOKENS,
       PIN_FB_TAB, PIN_ID_IN, PIN_ID_OUT, PIN_ACC_TAB, PIN_POST_TAB, PIN_ES_FILES, PIN_ES_RUNS, PIN_WARP_TAB, PIN_TD_TAB, PIN_SEAT_OUT, N_PIN };
}

struct spkd_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool gw_lds_ok = false;
    int rs_lds_cap = 0;          // dynamic LDS bytes admitted for k_resample
    bool bf_lds_ok = false;      // k_bf_gcc's dynamic LDS size is admitted
    bool warp_lds_ok = false;    // k_feature_warp's dynamic LDS size is admitted
    bool bf_tw_ready = false;    // the transform's twiddles are in their scratch slot (S_BF_TW)
    int gw_waves = 0;
    unsigned long long init_keys[2] = {0ull, ~0ull};
    int step_waves = 0;          // step chain: waves per workgroup (0 = by problem size, 4, 8)
    int step_partners = 0;       // step chain: partners per workgroup (0 = by problem size, 3, 7, 15)
    int64_t last_gw_items = 0;
    // the head of a batch clustering call (ahc_impl): SPKD_AHC_HEAD (-1 = the rule decides, 0 = none, k = forced),
    // the K of the most recent call, and the side stream its merge loops run on with the two events that order
    // it against the call's stream (created by the first call that forks, destroyed with the context)
    int ahc_head = -1;
    int64_t last_ahc_head = 0;
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::string err;
    int* d_err = nullptr;
    unsigned long long* d_counter = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = 0.f;
    // per-kernel timers (HIP events on the launch stream), see spkd_last_kernel_ms
    hipEvent_t ka[SPKD_N_TIMERS] = {}, kb[SPKD_N_TIMERS] = {};
    bool kused[SPKD_N_TIMERS] = {};
    float kms[SPKD_N_TIMERS] = {};
    void* slot[N_SLOTS] = {};
    size_t slot_bytes[N_SLOTS] = {};
    // SPKD_KL2_PINV: the Jacobi slabs of spkd_device.hpp (allocated by the first call that asks
    // for the mode) and what the current call's KL2 kernels get (nullptr: the inverse)
    void* pinv_ws = nullptr;
    double* pinv_cur = nullptr;
    // grow-only pinned host memory (results of the batch hand-off land here) and the redo
    // list of the most recent spkd_gw_batch
    void* pin[N_PIN] = {};
    size_t pin_bytes[N_PIN] = {};
    std::vector<int64_t> redo_line, redo_begin, redo_end;
    // host side of the redo statistics of spkd_ahc_fused (read by copies of the call)
    std::vector<Chunk> redo_chunks;
    std::vector<int64_t> redo_setoff;
    std::vector<int32_t> redo_sets;
};

namespace {

spkd_status fail(spkd_ctx* c, spkd_status s, const std::string& msg) {
    if (c) c->err = msg;
    return s;
}

#define HIPCHK(c, call)                                                              \
    do {                                                                             \
        hipError_t e_ = (call);                                                      \
        if (e_ != hipSuccess)                                                        \
            return fail((c), SPKD_EHIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// a step that returns an spkd_status: its failure is the caller's
#define TRY(expr) do { const spkd_status s_ = (expr); if (s_ != SPKD_OK) return s_; } while (0)

// grow-only scratch buffers (no hipMalloc in the steady state)
spkd_status scratch(spkd_ctx* c, int slot, size_t bytes, void** out) {
    if (bytes == 0) bytes = 16;
    if (c->slot_bytes[slot] < bytes) {
        if (c->slot[slot]) HIPCHK(c, hipFree(c->slot[slot]));
        c->slot[slot] = nullptr;
        c->slot_bytes[slot] = 0;
        size_t want = bytes + bytes / 4;
        hipError_t e = hipMalloc(&c->slot[slot], want);
        if (e != hipSuccess) {
            want = bytes;
            e = hipMalloc(&c->slot[slot], want);
        }
        if (e != hipSuccess) return fail(c, SPKD_ENOMEM, "scratch allocation failed");
        c->slot_bytes[slot] = want;
    }
    *out = c->slot[slot];
    return SPKD_OK;
}

// grow-only pinned host buffers, like scratch(): a copy into pinned memory is one DMA
// transfer at link speed, and the pages are touched once in the life of the context
spkd_status pinned(spkd_ctx* c, int which, size_t bytes, void** out) {
    if (bytes == 0) bytes = 16;
    if (c->pin_bytes[which] < bytes) {
        if (c->pin[which]) HIPCHK(c, hipHostFree(c->pin[which]));
        c->pin[which] = nullptr;
        c->pin_bytes[which] = 0;
        const size_t want = bytes + bytes / 4;
        if (hipHostMalloc(&c->pin[which], want, hipHostMallocDefault) != hipSuccess) {
            c->pin[which] = nullptr;
            return fail(c, SPKD_ENOMEM, "pinned host allocation failed");
        }
        c->pin_bytes[which] = want;
    }
    *out = c->pin[which];
    return SPKD_OK;
}

template <class T>
spkd_status upload(spkd_ctx* c, int slot, const T* h, size_t n, T** d) {
    void* p = nullptr;
    TRY(scratch(c, slot, n * sizeof(T), &p));
    if (n) HIPCHK(c, hipMemcpyAsync(p, h, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    *d = (T*)p;
    return SPKD_OK;
}

// A buffer that holds several arrays.  Its parts are listed once, in a function that chains a
// part() for each in order and returns bytes(); that function runs twice: on a Layout without
// a base to measure, on one with the base to place the pointers.  Every part starts at a
// multiple of its type's alignment.  With a staging area, part() also copies its source there:
// the host image of a table that goes up in one copy.
constexpr size_t IMAGE_ALIGN = 16;   // of the base of every buffer and image, so a part's offset is the same in each
struct Layout {
    char* const base;
    char* const stage;
    size_t at = 0;
    explicit Layout(void* b = nullptr, void* s = nullptr) : base((char*)b), stage((char*)s) {}
    template <class T>
    Layout& part(T*& p, size_t count, const T* src = nullptr) {
        static_assert(alignof(T) <= IMAGE_ALIGN, "a base aligns every part");
        align(alignof(T));
        p = base ? (T*)(base + at) : nullptr;
        if (stage && src) std::memcpy(stage + at, src, count * sizeof(T));
        at += count * sizeof(T);
        return *this;
    }
    size_t bytes() const { return at; }
    Layout& align(size_t a) { at = (at + a - 1) / a * a; return *this; }
};

// such a buffer from scratch() or pinned(): the size is what the walk over its parts measured
template <class Parts>
spkd_status carve(spkd_ctx* c, spkd_status (*alloc)(spkd_ctx*, int, size_t, void**), int slot, Parts parts) {
    void* p = nullptr;
    TRY(alloc(c, slot, parts(Layout()), &p));
    parts(Layout(p));
    return SPKD_OK;
}

// The table upload of the older stages, which stage in pageable memory (`image`, declared before the
// Call) and so stay off Mirror's pinned slots; the walk over the parts is the same one.
template <class Parts>
spkd_status upload_parts(spkd_ctx* c, int slot, std::vector<char>& image, Parts parts) {
    image.resize(parts(Layout()));
    parts(Layout(nullptr, image.data()));
    char* d = nullptr;
    TRY(upload(c, slot, image.data(), image.size(), &d));
    parts(Layout(d));
    return SPKD_OK;
}

// The bracket of an entry point that enqueues device work, opened after its argument checks:
// whatever its status, the call returns with that work finished (include/spkd.h).  finish()
// waits for the stream, the destructor whenever finish() did not get through.  Host memory that
// a copy of the call reads or writes is declared before the Call, so that the wait comes first.
struct Call {
    spkd_ctx* const c;
    spkd_status opened;          // of the constructor: TRY(call.opened)
    int herr = 0;                // the device error word (a member: its copy may be in flight)
    bool drained = false;
    bool forked = false, joined = false;   // the side stream: used by this call, and waited for by the call's stream
    explicit Call(spkd_ctx* ctx) : c(ctx) { opened = open(); }
    ~Call() {
        if (drained) return;
        (void)hipStreamSynchronize(c->stream);
        if (forked) (void)hipStreamSynchronize(c->side);
    }
    spkd_status open() {
        HIPCHK(c, hipSetDevice(c->device));
        for (int i = 0; i < SPKD_N_TIMERS; ++i) c->kused[i] = false;
        HIPCHK(c, hipMemsetAsync(c->d_err, 0, sizeof(int), c->stream));
        HIPCHK(c, hipEventRecord(c->ev0, c->stream));
        return SPKD_OK;
    }

    // The side stream of the context, for work of this call that may run beside what the call's stream
    // does next: it starts behind everything the call's stream holds at this point (uploads, memsets and
    // kernels of the call included).  Ordering is by the two events only; the bracket's promise covers
    // the side stream from here on (join(), finish(), the destructor).
    spkd_status fork() {
        // (default priority: what it is gated on ends and its first workgroup starts within 20 us, with a
        // k_matrix launch of the call's stream ready at the same moment -- profiles/ahc_head.json)
        if (!c->side) HIPCHK(c, hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
        if (!c->ev_fork) HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        if (!c->ev_join) HIPCHK(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
        HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
        forked = true;                     // (from the first enqueue that names the side stream)
        HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
        return SPKD_OK;
    }
    // the call's stream goes on behind what the side stream holds: before the first copy of a result
    spkd_status join() {
        if (!forked || joined) return SPKD_OK;
        HIPCHK(c, hipEventRecord(c->ev_join, c->side));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
        joined = true;
        return SPKD_OK;
    }

    // records the end event, waits, folds the device error word into a status (both streams OR into
    // the one word: it is copied behind the join, and read after both have drained)
    spkd_status finish() {
        TRY(join());
        HIPCHK(c, hipEventRecord(c->ev1, c->stream));
        HIPCHK(c, hipMemcpyAsync(&herr, c->d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (forked) HIPCHK(c, hipStreamSynchronize(c->side));
        drained = true;
        HIPCHK(c, hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
        c->kms[0] = c->last_ms;
        for (int i = 1; i < SPKD_N_TIMERS; ++i)
            if (c->kused[i]) HIPCHK(c, hipEventElapsedTime(&c->kms[i], c->ka[i], c->kb[i]));
        if (herr & ERR_SWEEP) return fail(c, SPKD_EHIP, "internal error: growing-window sweep order");
        if (herr & ERR_TDOA_STEPS) return fail(c, SPKD_EHIP, "internal error: tdoa_score met a step shorter than a frame");
        if (herr & 4) return fail(c, SPKD_EOVERFLOW, "device scratch capacity exceeded");
        if (herr & ERR_DEGENERATE_MERGE) return fail(c, SPKD_EINVAL, "degenerate merge: a diagonal cell was the minimum");
        if (herr & ERR_NONFINITE) return fail(c, SPKD_ENONFINITE, "array must not contain infs or NaNs");
        return SPKD_OK;
    }
};

// A mirrored block: one listing parts(Layout, Tab&), placed as h in a pinned slot and as d on the device, and one
// copy between the two images -- up for a table of the caller's arguments, down for a block of results.  A block
// is anything with `Tab h, d; Image host, dev;` and that parts(): a table struct with its checks and its fill
// (SeqTable, RangeTable), or a Mirror around a listing written where it is used.  stage() comes before the Call and
// takes none; what enqueues takes the Call.  So a copy's host side is a pinned slot of the context, staged, and for
// a table filled, before the bracket opens: the rule over Call holds.
struct Image { char* base = nullptr; size_t bytes = 0; };   // of a placed listing: where it starts, what it covers
template <class Tab, class Parts>
struct Mirror { const Parts parts; Tab h{}, d{}; Image host, dev; };
template <class Tab, class Parts>
Mirror<Tab, Parts> mirror(Parts parts) { return {parts}; }
// One image of the block as the next region of the buffer that L walks, from a multiple of IMAGE_ALIGN to
// one: the device's inside a scratch carve of the Call, whose own parts go on behind it; the host's for stage().
enum Side { DEVICE, HOST };
template <class Block>
Layout& place(Layout& L, Block& b, Side side = DEVICE) {
    Image& im = side == HOST ? b.host : b.dev;
    im.base = L.align(IMAGE_ALIGN).base ? L.base + L.at : nullptr;
    L.at += im.bytes = b.parts(Layout(im.base), side == HOST ? b.h : b.d);
    return L.align(IMAGE_ALIGN);
}
// before the Call: the host image in pinned slot `pin`, for the caller to fill or, after finish(), to read
template <class Block>
spkd_status stage(spkd_ctx* c, int pin, Block& b) {
    return carve(c, pinned, pin, [&](Layout L) { return place(L, b, HOST).bytes(); });
}
// the one copy of a staged and placed block, `kind` its direction
template <class Block>
spkd_status copy(Call& call, const Block& b, hipMemcpyKind kind) {
    if (!b.host.base || b.host.bytes != b.dev.bytes) return fail(call.c, SPKD_EHIP, "internal error: a block is copied staged and placed");
    const bool up = kind == hipMemcpyHostToDevice;
    HIPCHK(call.c, hipMemcpyAsync(up ? b.dev.base : b.host.base, up ? b.host.base : b.dev.base, b.host.bytes, kind, call.c->stream));
    return SPKD_OK;
}
// a table in scratch slot `slot` of its own, and up
template <class Block>
spkd_status send(Call& call, int slot, Block& b) {
    TRY(carve(call.c, scratch, slot, [&](Layout L) { return place(L, b).bytes(); }));
    return copy(call, b, hipMemcpyHostToDevice);
}

// The kind of a call that takes one: SPKD_KL2_PINV runs as SPKD_KL2 with the pseudo-inverse
// workspace handed to the kernels (c->pinv_cur), every other kind with none.  Called after the
// call's bracket is open (the first use clears the workspace's lock words on the stream).
spkd_status use_kind(spkd_ctx* c, int kind, int* base) {
    c->pinv_cur = nullptr;
    *base = kind;
    if (kind != SPKD_KL2_PINV) return SPKD_OK;
    *base = SPKD_KL2;
    if (!c->pinv_ws) {
        if (hipMalloc(&c->pinv_ws, PINV_WS_BYTES) != hipSuccess) {
            c->pinv_ws = nullptr;
            return fail(c, SPKD_ENOMEM, "pinv workspace allocation failed");
        }
        HIPCHK(c, hipMemsetAsync(c->pinv_ws, 0, PINV_LOCK_BYTES, c->stream));
    }
    c->pinv_cur = (double*)c->pinv_ws;
    return SPKD_OK;
}

bool bad_kind(int kind) { return kind < 0 || kind > 3; }
bool bad_comp(int n_comp) { return n_comp < 1 || n_comp > GT_MAX_COMP; }   // (the entry points' messages say 8)

// the caller's parameters with the kind as the kernels take it: Pk is the copy, P points to it
template <class Params>
spkd_status kernel_params(spkd_ctx* c, const Params*& P, Params& Pk) {
    Pk = *P;
    TRY(use_kind(c, P->kind, &Pk.kind));
    P = &Pk;
    return SPKD_OK;
}

// times the work its scope enqueues as kernel timer idx (spkd_last_kernel_ms); closes before finish()
struct Timer {
    spkd_ctx* const c;
    const int idx;
    Timer(spkd_ctx* ctx, int i) : c(ctx), idx(i) { (void)hipEventRecord(c->ka[idx], c->stream); }
    ~Timer() { (void)hipEventRecord(c->kb[idx], c->stream); c->kused[idx] = true; }
};

enum {
    S_CHUNKS = 0, S_SETOFF, S_PARTIAL, S_IDXA, S_IDXB, S_TERMS, S_TURNS, S_SNAP, S_CAND,
    S_GW_N_WIN, S_GW_WIN_DET, S_GW_WIN_MAXD, S_GW_DET_START, S_GW_DET_MAXI, S_GW_DET_D, S_GW_FINAL_START, S_LOG,
    S_AHC_STATS, S_AHC_LD, S_AHC_AUX, S_AHC_MAT, S_AHC_MISC, S_AHC_OUT, S_AHC_OFF, S_AHC_PROB, S_AHC_PACKED, S_MFCC_TAB, S_MFCC_STATIC, S_MFCC_TW,
    S_STEP_EXM, S_STEP_PKM, S_STEP_MISC, S_GMM_TAB, S_GMM_IDX,
    S_CP_TURNS, S_CP_TIMES, S_CP_LINES, S_REDO_STATS, S_REDO_IDX, S_VAD_TAB, S_VAD_BACK, S_VAD_FILES, S_VAD_TOKENS, S_SUM_IDX, S_GAUSS_OK, S_GAUSS_IDX,
    S_GT_TAB, S_GT_WORK, S_GT_IDX, S_UBM_TAB, S_UBM_WORK, S_CLR_WORK, S_CLR_MAT,
    S_MD_TAB, S_MD_BACK, S_MD_G, S_MD_B, S_MD_SEQS, S_MD_TOKENS, S_FB_TAB, S_FB_FWD, S_FB_OUT,
    S_ID_WORK, S_ID_MAT, S_ACC_TAB, S_POST_TAB, S_POST_PARTIAL, S_RS_TAB, S_BF_TAB, S_BF_TW, S_BF_ENERGY, S_BF_BACK, S_EN_TAB, S_ES_TAB, S_ES_FILES, S_ES_RUNS, S_WARP_TAB, S_TD_TAB, S_SEAT_OUT, S_SEAT_WORK, S_SEAT_MAT, S_OVL_RAW, S_COUNT
};
static_assert(S_COUNT <= N_SLOTS, "scratch slot table too small");

}  // namespace

extern "C" {

int spkd_abi_version(void) { return SPKD_ABI_VERSION; }

static spkd_status create_ctx(int device, void* stream, bool borrow, spkd_ctx** out) {
    if (!out) return SPKD_EINVAL;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return SPKD_EHIP;
    spkd_ctx* c = new spkd_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete c; return SPKD_EHIP; }
    if (borrow) {
        c->stream = (hipStream_t)stream;           // NULL = the legacy default stream itself
    } else {
        // a BLOCKING stream: ordered after (and before) work on the legacy default stream,
        // which is where torch's default stream puts the producers of d_frames
        if (hipStreamCreateWithFlags(&c->stream, hipStreamDefault) != hipSuccess) { delete c; return SPKD_EHIP; }
        c->own_stream = true;
    }
    if (hipMalloc(&c->d_err, sizeof(int)) != hipSuccess ||
        hipMalloc(&c->d_counter, 2 * sizeof(unsigned long long)) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
        spkd_destroy(c);
        return SPKD_EHIP;
    }
    for (int i = 0; i < SPKD_N_TIMERS; ++i)
        if (hipEventCreate(&c->ka[i]) != hipSuccess || hipEventCreate(&c->kb[i]) != hipSuccess) {
            spkd_destroy(c);
            return SPKD_EHIP;
        }
    // k_gw carves its LDS dynamically: the size must fit the device and be admitted
    // for the kernel, or every later launch fails -- checked once, reported by spkd_gw
    // (twelve kernels: a wave shape times a distance kind)
    int lds_max = 0;
    const struct { const void* fn; int bytes; } gw_kernels[] = {
#define SPKD_GW_SHAPE(NW_)                                                                                  \
        {(const void*)k_gw<NW_>, Gw<NW_>::LDS_BYTES}, {(const void*)k_gw_glr<NW_>, Gw<NW_>::LDS_BYTES},     \
        {(const void*)k_gw_kl2<NW_>, Gw<NW_>::LDS_BYTES}
        SPKD_GW_SHAPE(8), SPKD_GW_SHAPE(4), SPKD_GW_SHAPE(2), SPKD_GW_SHAPE(1)
#undef SPKD_GW_SHAPE
    };
    c->gw_lds_ok = hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess &&
                   Gw<4>::LDS_BYTES <= lds_max;
    for (const auto& k : gw_kernels)
        c->gw_lds_ok = c->gw_lds_ok &&
                       hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.bytes) == hipSuccess;
    // k_resample carves a tile's span and table dynamically, up to the whole LDS where the device admits it
    c->rs_lds_cap = 64 * 1024;
    if (lds_max > c->rs_lds_cap) {
        const int want = lds_max < RS_LDS_MAX ? lds_max : RS_LDS_MAX;
        if (hipFuncSetAttribute((const void*)k_resample, hipFuncAttributeMaxDynamicSharedMemorySize, want) == hipSuccess)
            c->rs_lds_cap = want;
    }
    c->bf_lds_ok = BF_LDS_BYTES <= lds_max &&
                   hipFuncSetAttribute((const void*)k_bf_gcc, hipFuncAttributeMaxDynamicSharedMemorySize, BF_LDS_BYTES) == hipSuccess;
    c->warp_lds_ok = (int)WP_LDS_MAX <= lds_max &&
                     hipFuncSetAttribute((const void*)k_feature_warp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)WP_LDS_MAX) == hipSuccess;
    // waves per turn of the growing-window kernel: 0 = by the number of turns (gw_impl)
    if (const char* e = getenv("SPKD_GW_WAVES")) c->gw_waves = atoi(e);
    if (const char* e = getenv("SPKD_STEP_WAVES")) { const int v = atoi(e); c->step_waves = (v == 4 || v == 8) ? v : 0; }
    if (const char* e = getenv("SPKD_STEP_PARTNERS")) { const int v = atoi(e); c->step_partners = (v == 3 || v == 7 || v == 15) ? v : 0; }
    // problems of a batch clustering call whose merge loops start under the others' matrices: -1 = by the
    // rule (ahc_head_rule), 0 = none, k = the k largest (results do not depend on it)
    if (const char* e = getenv("SPKD_AHC_HEAD")) { const int v = atoi(e); c->ahc_head = v >= 0 ? v : -1; }
    *out = c;
    return SPKD_OK;
}

spkd_status spkd_create(int device, void* stream, spkd_ctx** out) {
    return create_ctx(device, stream, stream != nullptr, out);
}

spkd_status spkd_create_on_stream(int device, void* stream, spkd_ctx** out) {
    return create_ctx(device, stream, true, out);
}

void spkd_destroy(spkd_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->side) {
        (void)hipStreamSynchronize(c->side);
        (void)hipStreamDestroy(c->side);
    }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    for (int i = 0; i < N_SLOTS; ++i)
        if (c->slot[i]) (void)hipFree(c->slot[i]);
    if (c->d_err) (void)hipFree(c->d_err);
    if (c->pinv_ws) (void)hipFree(c->pinv_ws);
    for (int i = 0; i < N_PIN; ++i)
        if (c->pin[i]) (void)hipHostFree(c->pin[i]);
    if (c->d_counter) (void)hipFree(c->d_counter);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (int i = 0; i < SPKD_N_TIMERS; ++i) {
        if (c->ka[i]) (void)hipEventDestroy(c->ka[i]);
        if (c->kb[i]) (void)hipEventDestroy(c->kb[i]);
    }
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* spkd_last_error(const spkd_ctx* c) { return c ? c->err.c_str() : "null context"; }

spkd_status spkd_sync(spkd_ctx* c) {
    if (!c) return SPKD_EINVAL;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SPKD_OK;
}

spkd_status spkd_malloc(spkd_ctx* c, size_t bytes, void** d_ptr) {
    if (!c || !d_ptr) return SPKD_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    hipError_t e = hipMalloc(d_ptr, bytes ? bytes : 16);
    if (e != hipSuccess) return fail(c, SPKD_ENOMEM, hipGetErrorString(e));
    return SPKD_OK;
}

spkd_status spkd_free(spkd_ctx* c, void* d_ptr) {
    if (!c) return SPKD_EINVAL;
    HIPCHK(c, hipFree(d_ptr));
    return SPKD_OK;
}

spkd_status spkd_memcpy_h2d(spkd_ctx* c, void* d_dst, const void* h_src, size_t bytes) {
    if (!c) return SPKD_EINVAL;
    HIPCHK(c, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SPKD_OK;
}

spkd_status spkd_memcpy_d2h(spkd_ctx* c, void* h_dst, const void* d_src, size_t bytes) {
    if (!c) return SPKD_EINVAL;
    HIPCHK(c, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SPKD_OK;
}

spkd_status spkd_memcpy_d2d(spkd_ctx* c, void* d_dst, const void* d_src, size_t bytes) {
    if (!c) return SPKD_EINVAL;
    HIPCHK(c, hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SPKD_OK;
}

spkd_status spkd_last_gw_items(spkd_ctx* c, int64_t* items) {
    if (!c || !items) return SPKD_EINVAL;
    *items = c->last_gw_items;
    return SPKD_OK;
}

spkd_status spkd_last_kernel_ms(spkd_ctx* c, int which, float* ms) {
    if (!c || !ms || which < 0 || which >= SPKD_N_TIMERS) return SPKD_EINVAL;
    *ms = c->kms[which];
    return SPKD_OK;
}

// ------------------------------------------------------------------ (1) stats
namespace {
// the launches of spkd_set_stats, without the call bracket (spkd_sw uses them too)
spkd_status set_stats_launch(spkd_ctx* c, const float* d_frames, int64_t n_frames,
                             const int64_t* h_begin, const int64_t* h_end, const int32_t* h_set,
                             int64_t n_ranges, int64_t n_sets, double* d_stats,
                             std::vector<Chunk>& chunks, std::vector<int64_t>& set_off) {
    chunks.clear();
    set_off.assign((size_t)n_sets + 1, 0);
    int32_t prev = 0;
    for (int64_t r = 0; r < n_ranges; ++r) {
        const int64_t b = h_begin[r], e = h_end[r];
        const int32_t s = h_set[r];
        if (b < 0 || e < b || e > n_frames || s < prev || s >= n_sets)
            return fail(c, SPKD_EINVAL, "bad frame range or set id");
        prev = s;
        for (int64_t t = b; t < e; t += STATS_CHUNK) {
            Chunk ch;
            ch.begin = t;
            ch.len = (int32_t)std::min<int64_t>(STATS_CHUNK, e - t);
            ch.set = s;
            chunks.push_back(ch);
            set_off[(size_t)s + 1]++;
        }
    }
    for (int64_t s = 0; s < n_sets; ++s) set_off[(size_t)s + 1] += set_off[(size_t)s];
    Chunk* d_chunks = nullptr;
    int64_t* d_setoff = nullptr;
    void* d_partial = nullptr;
    TRY(upload(c, S_CHUNKS, chunks.data(), chunks.size(), &d_chunks));
    TRY(upload(c, S_SETOFF, set_off.data(), set_off.size(), &d_setoff));
    TRY(scratch(c, S_PARTIAL, chunks.size() * REC * sizeof(double), &d_partial));
    if (!chunks.empty()) {
        Timer t(c, SPKD_T_CHUNK_STATS);
        hipLaunchKernelGGL(k_chunk_stats, dim3((unsigned)chunks.size()), dim3(STATS_TPB), 0, c->stream,
                           d_frames, d_chunks, (double*)d_partial);
    }
    Timer t(c, SPKD_T_REDUCE_SETS);                  // (to the end: nothing else is enqueued)
    hipLaunchKernelGGL(k_reduce_sets, dim3((unsigned)n_sets), dim3(STATS_TPB), 0, c->stream,
                       (const double*)d_partial, d_setoff, d_stats);
    HIPCHK(c, hipGetLastError());
    return SPKD_OK;
}
}  // namespace

spkd_status spkd_set_stats(spkd_ctx* c, const float* d_frames, int64_t n_frames,
                           const int64_t* h_begin, const int64_t* h_end, const int32_t* h_set,
                           int64_t n_ranges, int64_t n_sets, double* d_stats) {
    if (!c || !d_stats || n_sets < 0 || n_ranges < 0) return SPKD_EINVAL;
    if (n_sets == 0) return SPKD_OK;
    if (n_ranges > 0 && (!h_begin || !h_end || !h_set || !d_frames)) return fail(c, SPKD_EINVAL, "null range arrays");
    std::vector<Chunk> chunks;
    std::vector<int64_t> set_off;
    Call call(c);
    TRY(call.opened);
    TRY(set_stats_launch(c, d_frames, n_frames, h_begin, h_end, h_set, n_ranges, n_sets, d_stats, chunks, set_off));
    return call.finish();
}

// ------------------------------------------------------------------ (2) pair terms
spkd_status spkd_pair_terms(spkd_ctx* c, const double* d_stats, const int32_t* h_a, const int32_t* h_b,
                            int64_t n_pairs, int flags, double* h_terms) {
    if (!c || n_pairs < 0) return SPKD_EINVAL;
    if (n_pairs == 0) return SPKD_OK;
    if (!d_stats || !h_a || !h_b || !h_terms) return fail(c, SPKD_EINVAL, "null argument");
    if ((flags & SPKD_WANT_KL2) && (flags & SPKD_WANT_KL2_PINV))
        return fail(c, SPKD_EINVAL, "pair_terms: SPKD_WANT_KL2 and SPKD_WANT_KL2_PINV exclude each other");
    Call call(c);
    TRY(call.opened);
    int kind_unused;
    TRY(use_kind(c, (flags & SPKD_WANT_KL2_PINV) ? (int)SPKD_KL2_PINV : (int)SPKD_KL2, &kind_unused));
    if (flags & SPKD_WANT_KL2_PINV) flags = (flags & ~SPKD_WANT_KL2_PINV) | SPKD_WANT_KL2;
    int32_t *d_a = nullptr, *d_b = nullptr;
    void* d_terms = nullptr;
    TRY(upload(c, S_IDXA, h_a, (size_t)n_pairs, &d_a));
    TRY(upload(c, S_IDXB, h_b, (size_t)n_pairs, &d_b));
    TRY(scratch(c, S_TERMS, (size_t)n_pairs * 8 * sizeof(double), &d_terms));
    const unsigned blocks = (unsigned)((n_pairs + PT2_WAVES - 1) / PT2_WAVES);
    {
        Timer t(c, SPKD_T_PAIR_TERMS);
        hipLaunchKernelGGL(k_pair_terms, dim3(blocks), dim3(PT2_WAVES * WAVE), 0, c->stream,
                           d_stats, d_a, d_b, n_pairs, flags, (double*)d_terms, c->d_err, c->pinv_cur);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_terms, d_terms, (size_t)n_pairs * 8 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return call.finish();
}

// ------------------------------------------------------------------ clustering internals
namespace {
// What ahc_prepare leaves: the device buffers of the problems, and the host images of its two
// uploads -- declared by the caller before its Call, since copies of the call read them.
struct AhcPrep {
    double* ex;
    double* pk;          // packed working copies (the pair passes load these)
    double* ld;
    double* aux;
    double* mat;
    int64_t* seg_off;
    int64_t* mat_off;
    unsigned long long* smax;
    unsigned long long* smin;
    int64_t n_total = 0;
    int64_t grid_rows = 0;           // k_matrix's grid
    std::vector<char> offs;          // seg_off | mat_off
    std::vector<char> prob_of;       // record -> its problem | k_matrix's launch order (| the head's: below)
    // Head and rest (ahc_impl sets head_k before ahc_prepare; 0: one launch over all problems, none of this).
    // The head is the head_k largest problems, ties by index.  ahc_prepare then leaves the rest's k_matrix to its
    // caller (matrix_launch): grid_rows and d_sched are the rest's, grid_head and d_sched_head the head's, and
    // k_ahc's two launches take their problems from d_block_head (head_k of them) and d_block_rest.
    int64_t head_k = 0;
    int64_t grid_head = 0;
    int64_t n_max_head = 0, n_max_rest = 0;     // the largest problem of either launch (k_ahc's dynamic LDS)
    int32_t *d_prob = nullptr, *d_sched = nullptr, *d_sched_head = nullptr, *d_block_head = nullptr, *d_block_rest = nullptr;
    int variant = 1, kind = 0;
    double lambdac = 0.0;
};

// k_matrix's launch order over a subset of the problems (`order`: largest first), in the form the
// kernel takes: block b computes the matrix row of record sched[b] (-1: nothing).  Workgroups go to
// the eight XCDs round-robin by block index and every XCD has an L2 of its own, so the rows of one
// problem -- they all read that problem's records as partners -- are given to ONE XCD: its working
// set is then a problem or two (2.5 MB each at N = 390) instead of a slice of all of them.  Whole
// problems are dealt to the least-loaded XCD, largest first; with fewer problems than XCDs the rows
// are dealt round-robin instead.  by_xcd (optional): the problems in the order in which a launch of one
// block per problem meets the same dealing (block b on XCD b mod 8, as far as the lists are even).
constexpr int N_XCD = 8;
void deal_to_xcds(const int64_t* h_seg_off, const std::vector<int64_t>& order, std::vector<int32_t>& sched,
                  std::vector<int32_t>* by_xcd = nullptr) {
    const int X = N_XCD;
    std::vector<std::vector<int32_t>> lists(X), probs(X);
    if ((int64_t)order.size() >= X) {
        double load[X] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int64_t p : order) {
            int x = 0;
            for (int i = 1; i < X; ++i) if (load[i] < load[x]) x = i;
            const double n = (double)(h_seg_off[p + 1] - h_seg_off[p]);
            load[x] += n * n;
            probs[x].push_back((int32_t)p);
            for (int64_t r = h_seg_off[p]; r < h_seg_off[p + 1]; ++r) lists[x].push_back((int32_t)r);
        }
    } else {
        std::vector<int64_t> asc(order);                 // (the rows in record order; a problem per XCD)
        std::sort(asc.begin(), asc.end());
        int64_t i = 0;
        for (size_t k = 0; k < order.size(); ++k) {
            probs[k].push_back((int32_t)order[k]);
            for (int64_t r = h_seg_off[asc[k]]; r < h_seg_off[asc[k] + 1]; ++r) lists[(size_t)(i++ % X)].push_back((int32_t)r);
        }
    }
    size_t longest = 0;
    for (auto& l : lists) longest = std::max(longest, l.size());
    sched.assign(longest * X, -1);
    for (int x = 0; x < X; ++x)
        for (size_t i = 0; i < lists[x].size(); ++i) sched[i * X + x] = lists[x][i];
    if (by_xcd) {
        by_xcd->clear();
        for (size_t i = 0; by_xcd->size() < order.size(); ++i)
            for (int x = 0; x < X; ++x) if (i < probs[x].size()) by_xcd->push_back(probs[x][i]);
    }
}

unsigned long long host_dkey(double v) {                      // dkey() of spkd_cluster.hpp, on the host
    unsigned long long b;
    std::memcpy(&b, &v, sizeof b);
    b = (b << 1) ? b : 0ull;                                  // (zeros of either sign: one key)
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// What the initial matrix is: computed here in full (the default), only the rows
// [row_begin, row_end) of a single problem (spkd_distance_rows: a rank's block of a matrix
// tiled over several GPUs), or given by the caller (spkd_ahc_matrix: the gathered blocks).
struct MatrixPlan {
    const double* d_init = nullptr;
    double init_max = NAN, init_min = NAN;            // variant 1: max / min over the distances behind d_init
    int64_t row_begin = -1, row_end = -1;
    // the batch hand-off (spkd_ahc_fused): record r of the problems is d_stats[d_map[r]] of n_src
    // records, except the redo lines, whose records are computed from the frames first
    int64_t* d_map = nullptr;
    int64_t n_src = 0;
    const float* d_frames = nullptr;
    int64_t n_frames = 0;
    const int64_t *redo_line = nullptr, *redo_begin = nullptr, *redo_end = nullptr;
    int64_t n_redo = 0;
};

// the records in the quad layout the clustering kernels load from
void to_quadrec(spkd_ctx* c, const double* d_stats, int64_t n, double* ex) {
    hipLaunchKernelGGL(k_to_quadrec, dim3((unsigned)n), dim3(256), 0, c->stream, d_stats, n, ex);
}

// log dets / KL2 vectors of n records.  KL2: one wave per record; BIC / GLR: four records per wave
void cluster_prep(spkd_ctx* c, const double* ex, int64_t n, int kind, double* ld, double* aux) {
    const int64_t per_block = kind == SPKD_KL2 ? PT_WAVES : 4 * PT_WAVES;
    const unsigned blocks = (unsigned)((n + per_block - 1) / per_block);
    hipLaunchKernelGGL(k_cluster_prep, dim3(blocks), dim3(PT_WAVES * WAVE), 0, c->stream, ex, n, kind, ld, aux, c->d_err,
                       c->pinv_cur);
}

// one k_matrix launch over the rows of a schedule that ahc_prepare uploaded, on the call's stream
void matrix_launch(spkd_ctx* c, const AhcPrep& B, const int32_t* d_sched, int64_t grid) {
    if (grid <= 0) return;
    auto kmat = B.kind == SPKD_GLR ? k_matrix<true> : k_matrix<false>;   // GLR has a second rank-one term
    hipLaunchKernelGGL(kmat, dim3((unsigned)grid), dim3(MX_WAVES * WAVE), 0, c->stream,
                       (const double*)B.ex, (const double*)B.pk, (const int64_t*)B.seg_off, (const int32_t*)B.d_prob,
                       d_sched, B.variant, B.kind, B.lambdac,
                       (const double*)B.ld, (const double*)B.aux, B.mat, (const int64_t*)B.mat_off,
                       B.smax, B.smin, c->d_err);
}

// How many of the largest problems of a batch start their merge loops under the others' matrices
// (ahc_impl).  k_ahc gives a problem one CU, so its launch ends with its largest problem; with the K
// largest as the head, the stage ends at about
//     max( M_head + t(largest head problem),
//          M_head + M_rest * CUs / (CUs - K) + t(largest rest problem) )
// where t(N) = AHC_MS_PER_N2 * N^2 is a lone problem's merge loop and M = MATRIX_MS_PER_N2 * (sum of N^2)
// a k_matrix launch on the whole chip, of which the rest's has K CUs less.  n: the sizes, largest first.
// Returns the K in 0 .. 32 that minimises this (the smallest of equals); 0 when that saves less than 1 %
// of the stage with K = 0, and for fewer than 16 problems.  Only whole rounds of the chip's 32 shader
// engines are candidates, which leaves K = 32: a k_ahc workgroup takes a CU, and the workgroups of a
// launch are dealt in order to the eight XCDs and there to the four engines of eight CUs each, whatever
// those hold already.  A workgroup of the rest whose engine is full -- a head problem on one of its CUs --
// waits for that problem's exit, and the ones behind it on that XCD wait with it, while CUs elsewhere
// idle.  Measured (profiles/ahc_head.json): K = 8 leaves 24 of the rest's workgroups waiting up to 18 ms
// and the step 10 ms SLOWER than K = 0, K = 16 sixteen (+ 7 ms), K = 24 eight; with K = 32 every engine
// holds one head problem, seven of the rest's fit beside it, none waits, and the step is 6.7 ms faster.
// The two constants are the benchmark batch's, measured with single launches (tools/ahc_tail_profile.py,
// SPKD_AHC_HEAD=0), both in one session: profiles/matrix_dense_finish.json (k_matrix with its dense
// finish; before it 6.00e-7 and 2.095e-4, profiles/ahc_head.json).
constexpr int AHC_HEAD_ROUND = 32;             // XCDs x shader engines per XCD
constexpr double AHC_MS_PER_N2 = 2.122e-4;
constexpr double MATRIX_MS_PER_N2 = 5.58e-7;
constexpr int AHC_HEAD_MAX = 32;
constexpr int AHC_RULE_CUS = 256;              // of the MI355X
int64_t ahc_head_rule(const std::vector<int64_t>& n, int cus) {
    const int64_t n_prob = (int64_t)n.size();
    if (n_prob < 16) return 0;
    auto t = [](int64_t N) { return AHC_MS_PER_N2 * (double)N * (double)N; };
    double sum_all = 0.0;
    for (int64_t N : n) sum_all += (double)N * (double)N;
    const double stage0 = MATRIX_MS_PER_N2 * sum_all + t(n[0]);
    double best = stage0, sum_head = 0.0;
    int64_t best_k = 0;
    for (int64_t k = 1; k <= std::min<int64_t>(AHC_HEAD_MAX, n_prob) && k < cus; ++k) {
        sum_head += (double)n[(size_t)k - 1] * (double)n[(size_t)k - 1];
        const double m_head = MATRIX_MS_PER_N2 * sum_head, m_rest = MATRIX_MS_PER_N2 * (sum_all - sum_head);
        const double rest = k < n_prob ? m_rest * cus / (double)(cus - k) + t(n[(size_t)k]) : 0.0;
        const double stage = m_head + std::max(t(n[0]), rest);
        if (k % AHC_HEAD_ROUND == 0 && stage < best) { best = stage; best_k = k; }
    }
    return stage0 - best < 0.01 * stage0 ? 0 : best_k;
}

spkd_status ahc_prepare(spkd_ctx* c, const double* d_stats, const int64_t* h_seg_off, int64_t n_prob,
                        int variant, int kind, double lambdac, AhcPrep& B, const MatrixPlan& plan = MatrixPlan()) {
    const int64_t n_total = B.n_total = h_seg_off[n_prob];
    const size_t np = (size_t)n_prob;
    std::vector<int64_t> mat_off(np + 1);
    int64_t cells = 0;
    for (int64_t p = 0; p < n_prob; ++p) {
        const int64_t n = h_seg_off[p + 1] - h_seg_off[p];
        if (n < 0) return fail(c, SPKD_EINVAL, "seg_off must be non-decreasing");
        mat_off[(size_t)p] = cells;
        cells += n * n;
    }
    mat_off[np] = cells;
    std::vector<int32_t> prob((size_t)n_total, 0);   // record -> its problem
    for (int64_t p = 0; p < n_prob; ++p)
        for (int64_t r = h_seg_off[p]; r < h_seg_off[p + 1]; ++r) prob[(size_t)r] = (int32_t)p;
    // k_matrix's launch order (deal_to_xcds), in the same upload; with a head, a schedule of its own for
    // either launch, and the problems of k_ahc's two launches behind them
    {
        std::vector<int32_t> sched, sched_head, block_head, block_rest;
        if (plan.row_begin >= 0) {
            // a block of rows of the one problem: dealt round-robin (every XCD holds the records)
            const int64_t rows = plan.row_end - plan.row_begin;
            sched.assign((size_t)((rows + N_XCD - 1) / N_XCD * N_XCD), -1);
            for (int64_t i = 0; i < rows; ++i) sched[(size_t)i] = (int32_t)(plan.row_begin + i);
        } else {
            std::vector<int64_t> order((size_t)n_prob);
            for (int64_t p = 0; p < n_prob; ++p) order[(size_t)p] = p;
            std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
                return h_seg_off[a + 1] - h_seg_off[a] > h_seg_off[b + 1] - h_seg_off[b];
            });
            const std::vector<int64_t> head(order.begin(), order.begin() + B.head_k), rest(order.begin() + B.head_k, order.end());
            deal_to_xcds(h_seg_off, rest, sched);
            if (B.head_k > 0) {
                deal_to_xcds(h_seg_off, head, sched_head, &block_head);
                // (the rest's merge loops in the order of the problems, as the single launch has them)
                std::vector<char> in_head((size_t)n_prob, 0);
                for (int64_t p : head) in_head[(size_t)p] = 1;
                for (int64_t p = 0; p < n_prob; ++p) if (!in_head[(size_t)p]) block_rest.push_back((int32_t)p);
                B.n_max_head = h_seg_off[head[0] + 1] - h_seg_off[head[0]];
                B.n_max_rest = rest.empty() ? 0 : h_seg_off[rest[0] + 1] - h_seg_off[rest[0]];
            }
        }
        B.grid_rows = (int64_t)sched.size();
        B.grid_head = (int64_t)sched_head.size();
        TRY(upload_parts(c, S_AHC_OFF, B.offs, [&](Layout L) {
            return L.part(B.seg_off, np + 1, h_seg_off).part(B.mat_off, np + 1, mat_off.data()).bytes();
        }));
        TRY(upload_parts(c, S_AHC_PROB, B.prob_of, [&](Layout L) {
            return L.part(B.d_prob, prob.size(), prob.data()).part(B.d_sched, sched.size(), sched.data())
                .part(B.d_sched_head, sched_head.size(), sched_head.data()).part(B.d_block_head, block_head.size(), block_head.data())
                .part(B.d_block_rest, block_rest.size(), block_rest.data()).bytes();
        }));
    }
    B.variant = variant; B.kind = kind; B.lambdac = lambdac;
    const size_t nt = (size_t)n_total;
    TRY(carve(c, scratch, S_AHC_LD, [&](Layout L) { return L.part(B.ld, nt).bytes(); }));
    TRY(carve(c, scratch, S_AHC_AUX, [&](Layout L) { return L.part(B.aux, nt * AUX).bytes(); }));
    TRY(carve(c, scratch, S_AHC_MAT, [&](Layout L) { return L.part(B.mat, (size_t)cells).bytes(); }));
    TRY(carve(c, scratch, S_AHC_MISC, [&](Layout L) { return L.part(B.smax, np).part(B.smin, np).bytes(); }));
    HIPCHK(c, hipMemsetAsync(B.smax, 0x00, (size_t)n_prob * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(B.smin, 0xff, (size_t)n_prob * sizeof(unsigned long long), c->stream));
    if (plan.d_init && n_prob == 1) {
        // (the keys live in the context: the copies are asynchronous)
        c->init_keys[0] = plan.init_max == plan.init_max ? host_dkey(plan.init_max) : 0ull;
        c->init_keys[1] = plan.init_min == plan.init_min ? host_dkey(plan.init_min) : ~0ull;
        HIPCHK(c, hipMemcpyAsync(B.smax, &c->init_keys[0], sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(B.smin, &c->init_keys[1], sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
    }
    // a private working copy of the records (clusters are merged in place), expanded to the
    // quad layout the clustering kernels load from
    TRY(carve(c, scratch, S_AHC_STATS, [&](Layout L) { return L.part(B.ex, nt * QREC).bytes(); }));
    TRY(carve(c, scratch, S_AHC_PACKED, [&](Layout L) { return L.part(B.pk, nt * REC).bytes(); }));
    if (n_total > 0) {
        if (plan.d_map) {
            void* d_redo = nullptr;
            if (plan.n_redo > 0) {
                int64_t* d_rl = nullptr;
                TRY(scratch(c, S_REDO_STATS, (size_t)plan.n_redo * REC * sizeof(double), &d_redo));
                TRY(upload(c, S_REDO_IDX, plan.redo_line, (size_t)plan.n_redo, &d_rl));
                c->redo_sets.resize((size_t)plan.n_redo);
                for (int64_t k = 0; k < plan.n_redo; ++k) c->redo_sets[(size_t)k] = (int32_t)k;
                TRY(set_stats_launch(c, plan.d_frames, plan.n_frames, plan.redo_begin, plan.redo_end, c->redo_sets.data(),
                                     plan.n_redo, plan.n_redo, (double*)d_redo, c->redo_chunks, c->redo_setoff));
                hipLaunchKernelGGL(k_patch_map, dim3((unsigned)((plan.n_redo + 255) / 256)), dim3(256), 0, c->stream,
                                   (const int64_t*)d_rl, plan.n_redo, plan.d_map);
            }
            hipLaunchKernelGGL(k_records_from_map, dim3((unsigned)n_total), dim3(256), 0, c->stream, d_stats, plan.n_src,
                               (const int64_t*)plan.d_map, (const double*)d_redo, plan.n_redo, n_total, B.ex, B.pk, c->d_err);
        } else {
            to_quadrec(c, d_stats, n_total, B.ex);
            HIPCHK(c, hipMemcpyAsync(B.pk, d_stats, (size_t)n_total * REC * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        }
        {
            Timer t(c, SPKD_T_CLUSTER_PREP);
            cluster_prep(c, B.ex, n_total, kind, B.ld, B.aux);
        }
        if (plan.d_init) {
            HIPCHK(c, hipMemcpyAsync(B.mat, plan.d_init, (size_t)cells * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        } else if (B.head_k > 0) {
            // the head's rows; the rest's are the caller's, behind the fork (SPKD_T_MATRIX spans both launches)
            (void)hipEventRecord(c->ka[SPKD_T_MATRIX], c->stream);
            matrix_launch(c, B, B.d_sched_head, B.grid_head);
        } else if (B.grid_rows > 0) {
            Timer t(c, SPKD_T_MATRIX);
            matrix_launch(c, B, B.d_sched, B.grid_rows);
        }
    }
    HIPCHK(c, hipGetLastError());
    return SPKD_OK;
}

double key_to_double(unsigned long long k, bool is_max) {
    if (is_max ? (k == 0ull) : (k == ~0ull)) return std::nan("");
    unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}
}  // namespace

spkd_status spkd_distance_matrix(spkd_ctx* c, int kind, double lambdac, const double* d_stats,
                                 int64_t n, double* d_matrix) {
    if (!c || n < 0 || bad_kind(kind)) return SPKD_EINVAL;
    if (n == 0) return SPKD_OK;
    if (!d_stats || !d_matrix) return fail(c, SPKD_EINVAL, "null argument");
    const int64_t seg_off[2] = {0, n};
    AhcPrep B;
    Call call(c);
    TRY(call.opened);
    TRY(use_kind(c, kind, &kind));
    TRY(ahc_prepare(c, d_stats, seg_off, 1, 1, kind, lambdac, B));
    HIPCHK(c, hipMemcpyAsync(d_matrix, B.mat, (size_t)n * n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return call.finish();
}

spkd_status spkd_cluster_in(spkd_ctx* c, const double* d_stats, int64_t n, int kind, double lambdac, double threshold,
                            int32_t* h_label, double* h_dist, int64_t dist_cap, int64_t* h_dist_off,
                            int64_t* h_n_done, int64_t* h_n_clusters) {
    if (!c || n < 0 || dist_cap < 0 || bad_kind(kind)) return SPKD_EINVAL;
    if (h_n_done) *h_n_done = 0;
    if (h_n_clusters) *h_n_clusters = 0;
    if (n == 0) return SPKD_OK;
    if (!d_stats || !h_label || !h_dist_off || !h_n_done || !h_n_clusters || (dist_cap > 0 && !h_dist))
        return fail(c, SPKD_EINVAL, "null argument");
    long long done2[2] = {0, 0};
    Call call(c);
    TRY(call.opened);
    TRY(use_kind(c, kind, &kind));
    void *p_ex = nullptr, *p_ld = nullptr, *p_aux = nullptr, *p_cex = nullptr, *p_cpk = nullptr, *p_dist = nullptr;
    const size_t nn = (size_t)n;
    TRY(scratch(c, S_AHC_STATS, nn * QREC * sizeof(double), &p_ex));
    TRY(scratch(c, S_AHC_LD, nn * sizeof(double), &p_ld));
    TRY(scratch(c, S_AHC_AUX, nn * AUX * sizeof(double), &p_aux));
    TRY(scratch(c, S_STEP_EXM, nn * QREC * sizeof(double), &p_cex));
    TRY(scratch(c, S_STEP_PKM, nn * REC * sizeof(double), &p_cpk));
    double *clu_ld, *tmp, *clu_aux;
    long long *d_off, *d_done;
    int32_t* d_label;
    // cluster log dets | determinants of a step | cluster KL2 vectors | dist_off | done | labels
    TRY(carve(c, scratch, S_STEP_MISC, [&](Layout L) {
        return L.part(clu_ld, nn).part(tmp, nn).part(clu_aux, nn * AUX).part(d_off, nn + 1).part(d_done, 2)
            .part(d_label, nn).bytes();
    }));
    TRY(scratch(c, S_AHC_MAT, (size_t)std::max<int64_t>(dist_cap, 1) * sizeof(double), &p_dist));
    HIPCHK(c, hipMemsetAsync(d_done, 0, 2 * sizeof(long long), c->stream));
    to_quadrec(c, d_stats, n, (double*)p_ex);
    // the records' own log dets (also for KL2: they are what flags a covariance with infs or NaNs,
    // which the reference's pinv refuses like its det)
    {
        Timer t(c, SPKD_T_CLUSTER_PREP);
        cluster_prep(c, (const double*)p_ex, n, kind == SPKD_KL2 ? (int)SPKD_BIC : kind, (double*)p_ld, (double*)p_aux);
    }
    if (kind == SPKD_KL2) {
        void* p_ld2 = nullptr;                           // (the KL2 pass of the same kernel rewrites ld with zeros)
        TRY(scratch(c, S_AHC_OUT, nn * sizeof(double), &p_ld2));
        cluster_prep(c, (const double*)p_ex, n, SPKD_KL2, (double*)p_ld2, (double*)p_aux);
    }
    auto kin = kind == SPKD_GLR ? k_cluster_in<true> : k_cluster_in<false>;
    {
        Timer t(c, SPKD_T_AHC);
        hipLaunchKernelGGL(kin, dim3(1), dim3(CIN_TPB), 0, c->stream,
                           (const double*)p_ex, d_stats, (const double*)p_ld, (const double*)p_aux, (long long)n, kind, lambdac, threshold,
                           (double*)p_cex, (double*)p_cpk, clu_ld, clu_aux, tmp, d_label, (double*)p_dist, (long long)dist_cap,
                           d_off, d_done, c->d_err, c->pinv_cur);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(done2, d_done, sizeof done2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_label, d_label, nn * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_dist_off, d_off, (nn + 1) * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    if (dist_cap > 0)
        HIPCHK(c, hipMemcpyAsync(h_dist, p_dist, (size_t)dist_cap * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    const spkd_status st = call.finish();
    *h_n_done = done2[0];
    *h_n_clusters = done2[1];
    return st;
}

spkd_status spkd_cluster_in_batch(spkd_ctx* c, const double* d_stats, int64_t n_prob, const int64_t* h_seg_off, int kind,
                                  double lambdac, double threshold, int32_t* h_label, double* h_mind,
                                  int64_t* h_n_done, int64_t* h_n_clusters, double* h_stat_max, double* h_stat_min) {
    if (!c || n_prob < 0 || bad_kind(kind)) return SPKD_EINVAL;
    if (n_prob == 0) return SPKD_OK;
    if (!h_seg_off || !h_n_done || !h_n_clusters || !h_stat_max || !h_stat_min) return fail(c, SPKD_EINVAL, "null argument");
    if (h_seg_off[0] != 0) return fail(c, SPKD_EINVAL, "seg_off must start at 0");
    int64_t longest = 0;
    for (int64_t p = 0; p < n_prob; ++p) {
        if (h_seg_off[p + 1] < h_seg_off[p]) return fail(c, SPKD_EINVAL, "seg_off must be non-decreasing");
        longest = std::max(longest, h_seg_off[p + 1] - h_seg_off[p]);
    }
    if (longest > 65536) return fail(c, SPKD_EINVAL, "cluster_in_batch: a problem of more than 65 536 records");
    const int64_t n = h_seg_off[n_prob];
    if (n > 0 && (!d_stats || !h_label || !h_mind)) return fail(c, SPKD_EINVAL, "null argument");
    const size_t nn = (size_t)n, np = (size_t)n_prob;
    std::vector<long long> done2(2 * np, 0);
    std::vector<char> offs;
    Call call(c);
    TRY(call.opened);
    TRY(use_kind(c, kind, &kind));
    int64_t* d_segoff = nullptr;
    TRY(upload_parts(c, S_AHC_OFF, offs, [&](Layout L) { return L.part(d_segoff, np + 1, h_seg_off).bytes(); }));
    double *ex, *ld, *aux, *clu_ex, *clu_pk;
    TRY(carve(c, scratch, S_AHC_STATS, [&](Layout L) { return L.part(ex, nn * QREC).bytes(); }));
    TRY(carve(c, scratch, S_AHC_LD, [&](Layout L) { return L.part(ld, nn).bytes(); }));
    TRY(carve(c, scratch, S_AHC_AUX, [&](Layout L) { return L.part(aux, nn * AUX).bytes(); }));
    TRY(carve(c, scratch, S_STEP_EXM, [&](Layout L) { return L.part(clu_ex, nn * QREC).bytes(); }));
    TRY(carve(c, scratch, S_STEP_PKM, [&](Layout L) { return L.part(clu_pk, nn * REC).bytes(); }));
    double *clu_ld, *tmp, *clu_aux, *dists, *d_mind, *d_smax, *d_smin;
    long long* d_done;
    int32_t* d_label;
    int* d_perr;
    // cluster log dets | determinants and distances of a step | cluster KL2 vectors | mind | per problem: done,
    // clusters, max, min | labels | the problems' error words
    TRY(carve(c, scratch, S_STEP_MISC, [&](Layout L) {
        return L.part(clu_ld, nn).part(tmp, nn).part(dists, nn).part(clu_aux, nn * AUX).part(d_mind, nn)
            .part(d_smax, np).part(d_smin, np).part(d_done, 2 * np).part(d_label, nn).part(d_perr, np).bytes();
    }));
    HIPCHK(c, hipMemsetAsync(d_perr, 0, np * sizeof(int), c->stream));
    if (n > 0) {
        to_quadrec(c, d_stats, n, ex);
        // (the records' own log dets also for KL2, and its vectors in a second pass: see spkd_cluster_in)
        auto prep = [&](int k, double* out_ld) {
            const int64_t per_block = k == SPKD_KL2 ? PT_WAVES : 4 * PT_WAVES;
            hipLaunchKernelGGL(k_cluster_prep_batch, dim3((unsigned)n_prob, (unsigned)((longest + per_block - 1) / per_block)),
                               dim3(PT_WAVES * WAVE), 0, c->stream, (const double*)ex, (const int64_t*)d_segoff, k, out_ld, aux,
                               d_perr, c->pinv_cur);
        };
        {
            Timer t(c, SPKD_T_CLUSTER_PREP);
            prep(kind == SPKD_KL2 ? (int)SPKD_BIC : kind, ld);
        }
        if (kind == SPKD_KL2) {
            void* p_ld2 = nullptr;
            TRY(scratch(c, S_AHC_OUT, nn * sizeof(double), &p_ld2));
            prep(SPKD_KL2, (double*)p_ld2);
        }
    }
    auto kin = kind == SPKD_GLR ? k_cluster_in_batch<true> : k_cluster_in_batch<false>;
    {
        Timer t(c, SPKD_T_AHC);
        hipLaunchKernelGGL(kin, dim3((unsigned)n_prob), dim3(CIN_TPB), 0, c->stream,
                           (const double*)ex, d_stats, (const double*)ld, (const double*)aux, (const int64_t*)d_segoff, kind,
                           lambdac, threshold, clu_ex, clu_pk, clu_ld, clu_aux, tmp, dists, d_label, d_mind, d_done,
                           d_smax, d_smin, d_perr, c->d_err, c->pinv_cur);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(done2.data(), d_done, 2 * np * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_stat_max, d_smax, np * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_stat_min, d_smin, np * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (n > 0) {
        HIPCHK(c, hipMemcpyAsync(h_label, d_label, nn * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(h_mind, d_mind, nn * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    const spkd_status st = call.finish();
    if (st != SPKD_OK && st != SPKD_ENONFINITE) return st;
    for (size_t p = 0; p < np; ++p) {
        h_n_done[p] = done2[2 * p];
        h_n_clusters[p] = done2[2 * p + 1];
    }
    return st;
}

spkd_status spkd_distance_rows(spkd_ctx* c, int variant, int kind, double lambdac, const double* d_stats,
                               int64_t n, int64_t row_begin, int64_t row_end, double* d_rows,
                               double* h_stat_max, double* h_stat_min) {
    if (!c || n < 0 || bad_kind(kind) || (variant != 1 && variant != 2)) return SPKD_EINVAL;
    if (row_begin < 0 || row_end < row_begin || row_end > n) return fail(c, SPKD_EINVAL, "distance_rows: bad row block");
    if (h_stat_max) *h_stat_max = std::nan("");
    if (h_stat_min) *h_stat_min = std::nan("");
    if (n == 0 || row_end == row_begin) return SPKD_OK;
    if (!d_stats || !d_rows) return fail(c, SPKD_EINVAL, "null argument");
    const int64_t seg_off[2] = {0, n};
    AhcPrep B;
    MatrixPlan plan;
    plan.row_begin = row_begin;
    plan.row_end = row_end;
    unsigned long long keys[2] = {0ull, ~0ull};
    Call call(c);
    TRY(call.opened);
    TRY(use_kind(c, kind, &kind));
    TRY(ahc_prepare(c, d_stats, seg_off, 1, variant, kind, lambdac, B, plan));
    HIPCHK(c, hipMemcpyAsync(d_rows, B.mat + row_begin * n, (size_t)(row_end - row_begin) * n * sizeof(double),
                             hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(&keys[0], B.smax, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&keys[1], B.smin, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    const spkd_status st = call.finish();
    if (h_stat_max) *h_stat_max = key_to_double(keys[0], true);
    if (h_stat_min) *h_stat_min = key_to_double(keys[1], false);
    return st;
}

// ------------------------------------------------------------------ (4) AHC
namespace {
spkd_status ahc_impl(spkd_ctx* c, const double* d_stats, const int64_t* h_seg_off, int64_t n_prob,
                     const spkd_ahc_params* P, const MatrixPlan& plan, int32_t* h_n_merges, int32_t* h_merge_a,
                     int32_t* h_merge_b, double* h_merge_d, double* h_stat_max, double* h_stat_min) {
    if (!c || !P || n_prob < 0) return SPKD_EINVAL;
    if (n_prob == 0) return SPKD_OK;
    if (!d_stats || !h_seg_off || !h_n_merges || !h_merge_a || !h_merge_b || !h_merge_d ||
        !h_stat_max || !h_stat_min)
        return fail(c, SPKD_EINVAL, "null argument");
    if ((P->variant != 1 && P->variant != 2) || bad_kind(P->kind))
        return fail(c, SPKD_EINVAL, "bad variant / kind");
    for (int64_t p = 0; p < n_prob; ++p)
        if (h_seg_off[p + 1] - h_seg_off[p] < 1) return fail(c, SPKD_EINVAL, "empty clustering problem");
    int64_t n_max = 0;
    for (int64_t p = 0; p < n_prob; ++p) n_max = std::max<int64_t>(n_max, h_seg_off[p + 1] - h_seg_off[p]);
    if (n_max > AHC_MAX_N) return fail(c, SPKD_EINVAL, "clustering problem larger than 65536 records");
    // one workgroup per problem fills the chip only when there are many problems;
    // with few, the merge loop runs as a chain of launches over all CUs instead
    int path = P->path;
    if (path != SPKD_AHC_MONO && path != SPKD_AHC_WIDE) path = n_prob <= 64 ? SPKD_AHC_WIDE : SPKD_AHC_MONO;
    const size_t lds = (size_t)(n_max + 4) * sizeof(int32_t);
    if (path == SPKD_AHC_MONO && lds > 150 * 1024) path = SPKD_AHC_WIDE;
    // (checked before the n x n matrix is built)
    if (path == SPKD_AHC_WIDE && n_max > STEP_MAX_N)
        return fail(c, SPKD_EINVAL, "clustering problem larger than 16384 records (wide merge loop)");
    AhcPrep B;
    // Head and rest.  One workgroup per problem leaves the CUs of the smaller problems idle until the largest
    // is through; a problem's merge loop needs only its own matrix.  So the matrices of the few largest
    // problems are computed first, their merge loops start at once on the side stream, and the other
    // matrices are computed beside them (k_matrix is bound by fp64 issue, k_ahc waits for memory).  Only
    // the order of the launches changes: every problem runs the same code on the same data.
    c->last_ahc_head = 0;
    // (the pseudo-inverse's waves share one workspace under lock words: that mode stays on one stream)
    if (path == SPKD_AHC_MONO && !plan.d_init && plan.row_begin < 0 && P->kind != SPKD_KL2_PINV) {
        B.head_k = c->ahc_head >= 0 ? std::min<int64_t>(c->ahc_head, n_prob) : spkd_ahc_head_rule(h_seg_off, n_prob);
        c->last_ahc_head = B.head_k;
    }
    std::vector<unsigned long long> kmax((size_t)n_prob), kmin((size_t)n_prob);
    std::vector<double> fmax((size_t)n_prob), fmin((size_t)n_prob);
    Call call(c);
    TRY(call.opened);
    spkd_ahc_params Pk;
    TRY(kernel_params(c, P, Pk));
    // ahc_prepare expands the records into a private working copy (merged in place)
    TRY(ahc_prepare(c, d_stats, h_seg_off, n_prob, P->variant, P->kind, P->lambdac, B, plan));
    const int64_t n_total = B.n_total;
    const size_t nt = (size_t)n_total, np = (size_t)n_prob;
    // outputs + per-slot scratch
    double *d_merge_d, *d_tmp, *d_rmin, *d_fmax, *d_fmin;
    int32_t *d_a, *d_b, *d_alive, *d_rcache, *d_n;
    TRY(carve(c, scratch, S_AHC_OUT, [&](Layout L) {            // (rcache: arg col, NaN col, dirty of every record)
        return L.part(d_merge_d, nt).part(d_tmp, nt).part(d_rmin, nt).part(d_fmax, np).part(d_fmin, np)
            .part(d_a, nt).part(d_b, nt).part(d_alive, nt).part(d_rcache, 3 * nt).part(d_n, np).bytes();
    }));
    if (path == SPKD_AHC_MONO) {
        auto kahc = P->kind == SPKD_GLR ? k_ahc<true> : k_ahc<false>;
        if (lds > 48 * 1024)
            (void)hipFuncSetAttribute((const void*)kahc, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        // one launch over `grid` problems (`blocks`: which; nullptr: all, in order), its LDS by the largest of them
        auto merge_loops = [&](hipStream_t on, int64_t grid, const int32_t* blocks, int64_t largest) {
            hipLaunchKernelGGL(kahc, dim3((unsigned)grid), dim3(AHC_TPB), (size_t)(largest + 4) * sizeof(int32_t), on,
                               B.ex, B.pk, (const int64_t*)B.seg_off, P->variant, P->kind, P->max_spk, P->lambdac,
                               P->threshold, B.ld, B.aux, B.mat, (const int64_t*)B.mat_off, d_alive, d_tmp,
                               d_rmin, d_rcache, d_n, d_a, d_b, d_merge_d, B.smax, B.smin, d_fmax, d_fmin, c->d_err,
                               c->pinv_cur, blocks);
        };
        if (B.head_k > 0) {
            // The fork is behind the head's k_matrix, and so behind every upload, memset and preparation
            // kernel of the call: all that the head reads is ordered.  SPKD_T_AHC runs from the head's start
            // on the side stream to the join on the call's stream, which is behind both launches.
            TRY(call.fork());
            (void)hipEventRecord(c->ka[SPKD_T_AHC], c->side);
            merge_loops(c->side, B.head_k, B.d_block_head, B.n_max_head);
            matrix_launch(c, B, B.d_sched, B.grid_rows);
            (void)hipEventRecord(c->kb[SPKD_T_MATRIX], c->stream);
            c->kused[SPKD_T_MATRIX] = true;
            if (n_prob > B.head_k) merge_loops(c->stream, n_prob - B.head_k, B.d_block_rest, B.n_max_rest);
            HIPCHK(c, hipGetLastError());
            TRY(call.join());
            (void)hipEventRecord(c->kb[SPKD_T_AHC], c->stream);
            c->kused[SPKD_T_AHC] = true;
        } else {
            Timer t(c, SPKD_T_AHC);
            merge_loops(c->stream, n_prob, nullptr, n_max);
        }
    } else {
        // the step chain: one launch per merge, every workgroup selects for itself (spkd_cluster.hpp)
        StepArrays Q;
        void *pe = nullptr, *pp = nullptr;
        TRY(carve(c, scratch, S_STEP_MISC, [&](Layout L) {
            return L.part(Q.sel2, 2 * nt).part(Q.cnt, nt).part(Q.sw, nt).part(Q.state2, 2 * np).part(Q.death, nt).bytes();
        }));
        TRY(scratch(c, S_STEP_EXM, nt * QREC * sizeof(double), &pe));
        TRY(scratch(c, S_STEP_PKM, nt * REC * sizeof(double), &pp));
        Q.ex = B.ex; Q.pk = B.pk; Q.exm = (double*)pe; Q.pkm = (double*)pp;
        Q.n_total = n_total;
        Q.n_prob = (int32_t)n_prob;
        // eight waves per workgroup once a thread of four would meet more than ~4 clusters in the
        // selection (SPKD_STEP_WAVES = 4 | 8 overrides; results do not depend on it)
        const int step_waves = c->step_waves ? c->step_waves : (n_max > STEP_WIDE_FROM ? 8 : 4);
        // partners per workgroup: seven (two of the four waves pass) while that leaves every workgroup a CU
        // of its own, else fifteen (SPKD_STEP_PARTNERS = 7 | 15 overrides; four-wave workgroups only)
        // partners of a merge per workgroup -- 3, 7 or 15: one, two or four of a workgroup's waves
        // eliminate -- chosen PER ROUND from the partners that are left, so that every workgroup
        // has a CU to itself while the chip has CUs to spare (a workgroup's record loads go through
        // one CU's address unit); SPKD_STEP_PARTNERS = 3 | 7 | 15 pins it
        const bool glr_k = P->kind == SPKD_GLR;
        using StepKernel = decltype(&k_ahc_step<false, 4, 3>);
        StepKernel kvar[3];                              // [0] 3, [1] 7, [2] 15 partners
        if (step_waves == 8) {
            kvar[0] = glr_k ? k_ahc_step<true, 8, 3> : k_ahc_step<false, 8, 3>;
            kvar[1] = glr_k ? k_ahc_step<true, 8, 7> : k_ahc_step<false, 8, 7>;
            kvar[2] = glr_k ? k_ahc_step<true, 8, STEP_PARTNERS> : k_ahc_step<false, 8, STEP_PARTNERS>;
        } else {
            kvar[0] = glr_k ? k_ahc_step<true, 4, 3> : k_ahc_step<false, 4, 3>;
            kvar[1] = glr_k ? k_ahc_step<true, 4, 7> : k_ahc_step<false, 4, 7>;
            kvar[2] = glr_k ? k_ahc_step<true, 4, STEP_PARTNERS> : k_ahc_step<false, 4, STEP_PARTNERS>;
        }
        auto sp_of_round = [&](int64_t partners) -> int {
            if (c->step_partners) return c->step_partners;
            const int64_t free_cus = 255;                // (the bookkeeper takes one)
            if (partners * n_prob <= 3 * free_cus) return 3;
            if (partners * n_prob <= 7 * free_cus) return 7;
            return STEP_PARTNERS;
        };
        const size_t nch_max = (size_t)((n_max + WAVE - 1) / WAVE);
        const size_t step_lds = ((size_t)2 * n_max + nch_max + 2) * sizeof(int32_t) + nch_max * sizeof(unsigned long long);
        if (step_lds + 20 * 1024 > 48 * 1024)
            for (int v = 0; v < 3; ++v)
                (void)hipFuncSetAttribute((const void*)kvar[v], hipFuncAttributeMaxDynamicSharedMemorySize, (int)step_lds);
        Timer t(c, SPKD_T_AHC);
        const unsigned row_blocks = (unsigned)((n_max + AHC_WAVES - 1) / AHC_WAVES);
        hipLaunchKernelGGL(k_step_init, dim3(row_blocks, (unsigned)n_prob), dim3(AHC_TPB), 0, c->stream,
                           (const int64_t*)B.seg_off, (const double*)B.mat, (const int64_t*)B.mat_off, Q);
        for (int64_t it = 1; it < n_max; ++it) {
            const int64_t partners = n_max - it - 1;
            // (+ 1: the bookkeeper workgroup of every problem)
            const int step_sp = sp_of_round(partners);
            StepKernel kstep = kvar[step_sp == 3 ? 0 : (step_sp == 7 ? 1 : 2)];
            const unsigned blocks = (unsigned)std::max<int64_t>(1, (partners + step_sp - 1) / step_sp) + 1;
            hipLaunchKernelGGL(kstep, dim3(blocks, (unsigned)n_prob), dim3(step_waves * WAVE), step_lds, c->stream,
                               (int)it, (const int64_t*)B.seg_off, P->variant, P->kind, P->max_spk, P->lambdac,
                               P->threshold, B.ld, B.aux, B.mat, (const int64_t*)B.mat_off, Q, d_a, d_b, d_merge_d,
                               B.smax, B.smin, c->d_err, c->pinv_cur);
        }
        hipLaunchKernelGGL(k_step_final, dim3((unsigned)n_prob), dim3(AHC_TPB), 0, c->stream,
                           (int)(n_max - 1), (const int64_t*)B.seg_off, (const double*)B.mat, (const int64_t*)B.mat_off,
                           Q, d_n, d_fmax, d_fmin);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_n_merges, d_n, (size_t)n_prob * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_merge_a, d_a, (size_t)n_total * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_merge_b, d_b, (size_t)n_total * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_merge_d, d_merge_d, (size_t)n_total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(kmax.data(), B.smax, (size_t)n_prob * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(kmin.data(), B.smin, (size_t)n_prob * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(fmax.data(), d_fmax, (size_t)n_prob * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(fmin.data(), d_fmin, (size_t)n_prob * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    const spkd_status st = call.finish();
    for (int64_t p = 0; p < n_prob; ++p) {
        if (P->variant == 1) {
            h_stat_max[p] = key_to_double(kmax[(size_t)p], true);
            h_stat_min[p] = key_to_double(kmin[(size_t)p], false);
        } else {
            h_stat_max[p] = fmax[(size_t)p];
            h_stat_min[p] = fmin[(size_t)p];
        }
    }
    return st;
}
}  // namespace

spkd_status spkd_ahc(spkd_ctx* c, const double* d_stats, const int64_t* h_seg_off, int64_t n_prob,
                     const spkd_ahc_params* P, int32_t* h_n_merges, int32_t* h_merge_a,
                     int32_t* h_merge_b, double* h_merge_d, double* h_stat_max, double* h_stat_min) {
    return ahc_impl(c, d_stats, h_seg_off, n_prob, P, MatrixPlan(), h_n_merges, h_merge_a, h_merge_b, h_merge_d,
                    h_stat_max, h_stat_min);
}

spkd_status spkd_ahc_matrix(spkd_ctx* c, const double* d_stats, int64_t n, const spkd_ahc_params* P,
                            const double* d_matrix, double stat_max_in, double stat_min_in,
                            int32_t* h_n_merges, int32_t* h_merge_a, int32_t* h_merge_b, double* h_merge_d,
                            double* h_stat_max, double* h_stat_min) {
    if (!c || n < 1) return SPKD_EINVAL;
    if (!d_matrix) return fail(c, SPKD_EINVAL, "ahc_matrix: null matrix");
    const int64_t seg_off[2] = {0, n};
    MatrixPlan plan;
    plan.d_init = d_matrix;
    plan.init_max = stat_max_in;
    plan.init_min = stat_min_in;
    return ahc_impl(c, d_stats, seg_off, 1, P, plan, h_n_merges, h_merge_a, h_merge_b, h_merge_d, h_stat_max, h_stat_min);
}

spkd_status spkd_last_ahc_head(spkd_ctx* c, int64_t* k) {
    if (!c || !k) return SPKD_EINVAL;
    *k = c->last_ahc_head;
    return SPKD_OK;
}

int64_t spkd_ahc_head_rule(const int64_t* h_seg_off, int64_t n_prob) {
    if (!h_seg_off || n_prob < 0) return -1;
    std::vector<int64_t> sizes((size_t)n_prob);
    for (int64_t p = 0; p < n_prob; ++p) sizes[(size_t)p] = h_seg_off[p + 1] - h_seg_off[p];
    std::sort(sizes.begin(), sizes.end(), std::greater<int64_t>());
    return ahc_head_rule(sizes, AHC_RULE_CUS);
}

// ------------------------------------------------------------------ (3) change detection
// A first guess, not a bound (include/spkd.h): scans of a window end that only moves forward.
int64_t spkd_gw_event_capacity(int64_t turn_len, double rate) {
    if (turn_len < 0 || !(rate >= 10.0)) return -1;
    // an outer iteration that detects advances `start` by >= 0.4*rate, one that does not grows
    // `end` by >= 0.5*rate (while winstep >= 0.2*rate; spkd_gw_event_capacity_p covers every winstep)
    return (int64_t)((double)turn_len / (0.2 * rate)) + 8;
}

int64_t spkd_gw_event_capacity_p(int64_t turn_len, const spkd_cd_params* P) {
    if (turn_len < 0 || !P || !(P->rate >= 10.0) || !(P->winstep >= 1.0)) return -1;
    // an outer iteration that detects advances `start` by maxi >= minfeas - istep = 0.4*rate;
    // one that does not grows `end` by ws, and ws is clamped to winstep from the second
    // growth of an epoch on (CD:273-284): at least min(0.5*rate, winstep) frames.  What this
    // leaves out: a detection resets `end` to start + 2*winsize (CD:264-266), the next epoch
    // regrows over frames the last one had already covered -- turns that re-scan a lot need
    // more, are told SPKD_EOVERFLOW by the kernel, and are repeated with more by the caller.
    const double step = std::min(0.2 * P->rate, std::min(0.5 * P->rate, P->winstep));
    return (int64_t)((double)turn_len / step) + 8;
}

int64_t spkd_sw_window_count(int64_t turn_len, double winsize, double winstep) {
    if (!(winstep >= 1.0) || !(winsize >= 1.0)) return -1;
    // whole frames (what the scripts' floor() gives): the sums of the loop below are exact
    if (winsize == std::floor(winsize) && winstep == std::floor(winstep) && winsize < 1e15 && winstep < 1e15 &&
        turn_len < (int64_t)1e15) {
        const int64_t size2 = 2 * (int64_t)winsize;
        return turn_len < size2 ? 0 : (turn_len - size2) / (int64_t)winstep + 1;
    }
    int64_t w = 0;
    for (double s = 0; s + 2 * winsize <= (double)turn_len; s += winstep) ++w;
    return w;
}

namespace {
spkd_status build_turns(spkd_ctx* c, int64_t n_frames, const int64_t* hb, const int64_t* he, int64_t n_turns,
                        const spkd_cd_params* P, const int64_t* h_off, bool gw, std::vector<TurnDesc>& turns,
                        int64_t& n_cand) {
    n_cand = 0;
    turns.resize((size_t)n_turns);
    for (int64_t t = 0; t < n_turns; ++t) {
        if (hb[t] < 0 || he[t] < hb[t] || he[t] > n_frames) return fail(c, SPKD_EINVAL, "bad turn range");
        TurnDesc& T = turns[(size_t)t];
        T.begin = hb[t];
        T.len = he[t] - hb[t];
        T.cand_off = n_cand;
        T.cand_cap = gw ? (int64_t)((double)T.len / (P->rate / 10)) + (int64_t)(2 * (P->rate / 10)) + 16 : 0;
        n_cand += T.cand_cap;
        T.ev_off = h_off[t];
        T.ev_cap = h_off[t + 1] - h_off[t];
        T.id = t;
        if (T.ev_cap < 0) return fail(c, SPKD_EINVAL, "offsets must be non-decreasing");
    }
    // longest turns first: a turn is a serial chain on one workgroup, so this is the
    // classic LPT order that keeps the tail of the launch short
    if (gw) std::stable_sort(turns.begin(), turns.end(), [](const TurnDesc& a, const TurnDesc& b) { return a.len > b.len; });
    return SPKD_OK;
}

// what spkd_gw_batch adds to the growing-window call
struct GwBatch {
    const double *turn_start_s, *turn_end_s;
    const int64_t *file_off, *file_len;
    int want_index;
    spkd_gw_lines_view* view;
    // device side (gw_batch_upload)
    double *d_ls = nullptr, *d_le = nullptr;
    int64_t* d_line_off = nullptr;
    int32_t *d_n_det = nullptr, *d_pos = nullptr;
    // host side, pinned
    int64_t* h_head = nullptr;                       // [0] lines, [1] the device error word
    int32_t* h_n_win = nullptr;
    int64_t n_lines = 0;
    bool have_lines = false;
};

// before k_gw is enqueued: the turn times go up while nothing waits for them
spkd_status gw_batch_upload(spkd_ctx* c, GwBatch& G, int64_t n_turns) {
    const size_t nt = (size_t)n_turns;
    TRY(carve(c, scratch, S_CP_TURNS, [&](Layout L) {
        return L.part(G.d_ls, nt).part(G.d_le, nt).part(G.d_line_off, nt + 1).part(G.d_n_det, nt).part(G.d_pos, nt).bytes();
    }));
    HIPCHK(c, hipMemcpyAsync(G.d_ls, G.turn_start_s, nt * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(G.d_le, G.turn_end_s, nt * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return carve(c, pinned, PIN_GW_TURNS, [&](Layout L) { return L.part(G.h_head, 2).part(G.h_n_win, nt).bytes(); });
}

// the event arrays of a growing-window call on the device, by the names k_gw gives them
struct GwEvents {
    int32_t* n_win = nullptr;
    double* win_maxd = nullptr;
    int32_t* win_det = nullptr;
    double *det_start = nullptr, *det_maxi = nullptr, *det_d = nullptr, *final_start = nullptr;
};

// the lines of a batch, on the device and in pinned host memory alike
struct LineArrays {
    int64_t* frame;                                  // frame_b | frame_e
    int64_t* index;
    int32_t* turn;
    Layout& parts(Layout& L, size_t n) { return L.part(frame, 2 * n).part(index, n).part(turn, n); }
};

// behind k_gw, inside its call bracket: count, scan, learn the number of lines, write and fetch them
spkd_status gw_batch_compact(spkd_ctx* c, GwBatch& G, const TurnDesc* d_turns, int64_t n_turns, const GwEvents& ev,
                             double rate) {
    const unsigned blocks = (unsigned)((n_turns + CP_TPB - 1) / CP_TPB);
    hipLaunchKernelGGL(k_cp_count, dim3(blocks), dim3(CP_TPB), 0, c->stream, d_turns, n_turns, (const int32_t*)ev.n_win,
                       (const int32_t*)ev.win_det, (const int*)c->d_err, G.d_n_det, G.d_pos);
    hipLaunchKernelGGL(k_cp_scan, dim3(1), dim3(CP_SCAN_TPB), 0, c->stream, (const int32_t*)G.d_n_det, n_turns,
                       (const int*)c->d_err, G.d_line_off);
    HIPCHK(c, hipGetLastError());
    G.h_head[0] = 0;
    G.h_head[1] = 0;
    HIPCHK(c, hipMemcpyAsync(&G.h_head[0], G.d_line_off + n_turns, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&G.h_head[1], c->d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(G.h_n_win, ev.n_win, (size_t)n_turns * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (G.h_head[1] != 0) return SPKD_OK;            // (the call's finish() turns the word into its status)
    const int64_t n = G.h_head[0];
    if (n < n_turns) return fail(c, SPKD_EHIP, "internal error: fewer lines than turns");
    const size_t nn = (size_t)n;
    void* d_t = nullptr;
    LineArrays D, H;
    double* h_times;
    TRY(scratch(c, S_CP_TIMES, nn * 2 * sizeof(double), &d_t));
    TRY(carve(c, scratch, S_CP_LINES, [&](Layout L) { return D.parts(L, nn).bytes(); }));
    TRY(carve(c, pinned, PIN_GW_LINES, [&](Layout L) { return H.parts(L.part(h_times, 2 * nn), nn).bytes(); }));
    hipLaunchKernelGGL(k_cp_lines, dim3(blocks), dim3(CP_TPB), 0, c->stream, d_turns, n_turns,
                       (const int32_t*)G.d_n_det, (const int32_t*)G.d_pos, (const int64_t*)G.d_line_off, n,
                       (const double*)ev.det_start, (const double*)ev.det_maxi, (const double*)ev.final_start,
                       (const double*)G.d_ls, (const double*)G.d_le, rate,
                       (const int*)c->d_err, (double*)d_t, D.frame, D.frame + nn, D.index, D.turn);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_times, d_t, nn * 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(H.frame, D.frame, nn * 2 * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(H.turn, D.turn, nn * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (G.want_index)
        HIPCHK(c, hipMemcpyAsync(H.index, D.index, nn * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    spkd_gw_lines_view& V = *G.view;
    V.n_lines = n;
    V.n_win = G.h_n_win;
    V.times = h_times;
    V.turn = H.turn;
    V.frame_b = H.frame;
    V.frame_e = H.frame + nn;
    V.index = G.want_index ? H.index : nullptr;
    V.d_index = D.index;
    G.n_lines = n;
    G.have_lines = true;
    return SPKD_OK;
}

// after the call has drained: the 12-digit round trip of the times in place, and in the same
// pass the lines whose frame range -- as the clustering script cuts it from the round-tripped
// times -- is not the one the fused record covers
spkd_status gw_batch_finish(spkd_ctx* c, GwBatch& G, int64_t n_turns, double rate) {
    spkd_gw_lines_view& V = *G.view;
    double* times = const_cast<double*>(V.times);
    spkd_py2_roundtrip(times, 2 * V.n_lines);
    c->redo_line.clear();
    c->redo_begin.clear();
    c->redo_end.clear();
    for (int64_t i = 0; i < V.n_lines; ++i) {
        const int64_t t = V.turn[i];
        if (t < 0 || t >= n_turns) return fail(c, SPKD_EHIP, "internal error: line of no turn");
        const int64_t fn = G.file_len[t];
        int64_t a0 = (int64_t)(times[2 * i] * rate), a1 = (int64_t)(times[2 * i + 1] * rate);
        a0 = a0 < 0 ? 0 : (a0 > fn ? fn : a0);
        a1 = a1 < 0 ? 0 : (a1 > fn ? fn : a1);
        if (a1 < a0) a1 = a0;
        const int64_t b = G.file_off[t] + a0, e = G.file_off[t] + a1;
        if (b != V.frame_b[i] || e != V.frame_e[i]) {
            c->redo_line.push_back(i);
            c->redo_begin.push_back(b);
            c->redo_end.push_back(e);
        }
    }
    V.n_redo = (int64_t)c->redo_line.size();
    V.redo_line = c->redo_line.data();
    V.redo_begin = c->redo_begin.data();
    V.redo_end = c->redo_end.data();
    return SPKD_OK;
}

// what a growing-window call reads ...
struct GwIn {
    const float* d_frames = nullptr;
    int64_t n_frames = 0, n_turns = 0;
    const int64_t *hb = nullptr, *he = nullptr, *h_ev_off = nullptr;
    const spkd_cd_params* P = nullptr;
    int check_capacity = 0;
    double* d_seg_stats = nullptr;                   // the fused forms: a record per event slot
};
// ... and where it leaves the event arrays and the candidate log on the host (the batch form
// copies none of them)
struct GwOut {
    int32_t *h_n_win = nullptr, *h_win_det = nullptr;
    double *h_win_maxd = nullptr, *h_det_start = nullptr, *h_det_maxi = nullptr, *h_det_d = nullptr,
           *h_final_start = nullptr;
    spkd_cand_log* h_log = nullptr;
    int64_t log_cap = 0;
    int64_t* h_log_count = nullptr;
};

// Every event array once, in the order k_gw takes them and the results are copied: its scratch
// slot, its element size, whether it holds a value per turn or per event slot, and where its
// pointer is in GwEvents and in GwOut.
struct GwEventArray { int slot; size_t elem; bool per_turn; size_t dev, host; };
#define SPKD_EV(SLOT, T, per_turn, name) {SLOT, sizeof(T), per_turn, offsetof(GwEvents, name), offsetof(GwOut, h_##name)}
const GwEventArray GW_EVENT_ARRAYS[] = {
    SPKD_EV(S_GW_N_WIN, int32_t, true, n_win),
    SPKD_EV(S_GW_WIN_MAXD, double, false, win_maxd),
    SPKD_EV(S_GW_WIN_DET, int32_t, false, win_det),
    SPKD_EV(S_GW_DET_START, double, false, det_start),
    SPKD_EV(S_GW_DET_MAXI, double, false, det_maxi),
    SPKD_EV(S_GW_DET_D, double, false, det_d),
    SPKD_EV(S_GW_FINAL_START, double, true, final_start),
};
#undef SPKD_EV
// (the pointer members have different types: read and written as bytes)
void* get_pointer(const void* s, size_t off) { void* p; std::memcpy(&p, (const char*)s + off, sizeof p); return p; }
void set_pointer(void* s, size_t off, void* p) { std::memcpy((char*)s + off, &p, sizeof p); }

// from this many turns on, a wave per turn (2 048 wave slots on the chip at two waves per SIMD)
constexpr int64_t GW_WAVE_PER_TURN_FROM = 4096;
constexpr int64_t GW_EIGHT_WAVES_UP_TO = 256;           // a workgroup per CU: eight waves per turn
spkd_status gw_impl(spkd_ctx* c, const GwIn& in, const GwOut& out, GwBatch* batch = nullptr) {
    const int64_t n_turns = in.n_turns, log_cap = out.log_cap;
    const spkd_cd_params* P = in.P;
    if (!c || !P || n_turns < 0) return SPKD_EINVAL;
    if (out.h_log_count) *out.h_log_count = 0;
    if (n_turns == 0) return SPKD_OK;
    if (!in.d_frames || !in.hb || !in.he || !in.h_ev_off) return fail(c, SPKD_EINVAL, "null argument");
    for (const GwEventArray& a : GW_EVENT_ARRAYS)
        if (!batch && !get_pointer(&out, a.host)) return fail(c, SPKD_EINVAL, "null argument");
    if (bad_kind(P->kind)) return fail(c, SPKD_EINVAL, "gw: bad kind");
    if (!(P->rate >= 10.0) || !(P->winsize >= 1.0) || !(P->winstep >= 1.0))
        return fail(c, SPKD_EINVAL, "gw: rate >= 10, winsize >= 1 frame and winstep >= 1 frame required");
    if (log_cap < 0 || (log_cap > 0 && !out.h_log)) return fail(c, SPKD_EINVAL, "gw: log capacity without a log buffer");
    if (!c->gw_lds_ok) return fail(c, SPKD_EHIP, "gw: the kernel's dynamic LDS size was not admitted on this device");
    std::vector<TurnDesc> turns;
    int64_t n_cand;
    TRY(build_turns(c, in.n_frames, in.hb, in.he, n_turns, P, in.h_ev_off, true, turns, n_cand));
    for (int64_t t = 0; in.check_capacity && t < n_turns; ++t)
        if (turns[(size_t)t].ev_cap < spkd_gw_event_capacity_p(turns[(size_t)t].len, P))
            return fail(c, SPKD_EINVAL, "gw: event capacity too small, see spkd_gw_event_capacity_p");
    unsigned long long cnt2[2] = {0ull, 0ull};
    Call call(c);
    TRY(call.opened);
    spkd_cd_params Pk;
    TRY(kernel_params(c, P, Pk));
    const int64_t n_ev = in.h_ev_off[n_turns];
    TurnDesc* d_turns = nullptr;
    void *d_snap = nullptr, *d_cand = nullptr, *d_log = nullptr;
    GwEvents ev;
    TRY(upload(c, S_TURNS, turns.data(), turns.size(), &d_turns));
    // one packed record (running moment sums at the split point) per candidate slot
    TRY(scratch(c, S_SNAP, (size_t)n_cand * REC * sizeof(double), &d_snap));
    TRY(scratch(c, S_CAND, (size_t)n_cand * 4 * sizeof(double), &d_cand));
    auto ev_bytes = [&](const GwEventArray& a) { return (size_t)(a.per_turn ? n_turns : n_ev) * a.elem; };
    // every pointer the kernel dereferences (a null one would be a GPU memory fault, not a status)
    bool missing = false;
    for (const GwEventArray& a : GW_EVENT_ARRAYS) {
        void* p = nullptr;
        TRY(scratch(c, a.slot, ev_bytes(a), &p));
        set_pointer(&ev, a.dev, p);
        missing = missing || !p;
    }
    TRY(scratch(c, S_LOG, (size_t)std::max<int64_t>(log_cap, 1) * sizeof(spkd_cand_log), &d_log));
    if (missing || !d_turns || !d_snap || !d_cand || !d_log || !c->d_counter || !c->d_err)
        return fail(c, SPKD_EHIP, "gw: a device scratch buffer is missing");
    HIPCHK(c, hipMemsetAsync(c->d_counter, 0, 2 * sizeof(unsigned long long), c->stream));   // [0] log entries, [1] determinants
    if (batch) TRY(gw_batch_upload(c, *batch, n_turns));
    // A turn is a serial chain of scans.  With few turns a workgroup of four waves shares a
    // turn's matrices (latency); with thousands, ONE WAVE per turn keeps every wave of the
    // chip busy with its own chain (throughput): no wave waits at a barrier for the serial
    // phases of its turn, the SIMD's other wave belongs to another turn.  The variants give
    // bit-identical results (same sums, same eliminations, same decisions).
    int nw = c->gw_waves;
    if (nw != 1 && nw != 2 && nw != 4 && nw != 8)
        nw = n_turns >= GW_WAVE_PER_TURN_FROM ? 1 : (n_turns <= GW_EIGHT_WAVES_UP_TO ? 8 : 4);
    // the kernel instance of the call's kind (kernel_params: SPKD_KL2_PINV runs as SPKD_KL2);
    // BIC is k_gw itself
#define SPKD_GW_LAUNCH(NW_)                                                                                     \
    hipLaunchKernelGGL((P->kind == SPKD_GLR ? k_gw_glr<NW_> : P->kind == SPKD_KL2 ? k_gw_kl2<NW_> : k_gw<NW_>), \
                       dim3((unsigned)n_turns), dim3(Gw<NW_>::TPB), Gw<NW_>::LDS_BYTES, c->stream,             \
                       in.d_frames, (const TurnDesc*)d_turns, *P, (double*)d_snap, (double*)d_cand,            \
                       ev.n_win, ev.win_maxd, ev.win_det, ev.det_start, ev.det_maxi, ev.det_d, ev.final_start,  \
                       in.d_seg_stats, (spkd_cand_log*)d_log, (long long)log_cap, c->d_counter, c->d_err,      \
                       c->pinv_cur)
    {
        Timer t(c, SPKD_T_GW);
        if (nw == 1) SPKD_GW_LAUNCH(1); else if (nw == 2) SPKD_GW_LAUNCH(2);
        else if (nw == 8) SPKD_GW_LAUNCH(8); else SPKD_GW_LAUNCH(4);
    }
#undef SPKD_GW_LAUNCH
    HIPCHK(c, hipGetLastError());
    unsigned long long& cnt = cnt2[0];
    if (batch) {
        TRY(gw_batch_compact(c, *batch, d_turns, n_turns, ev, P->rate));
        HIPCHK(c, hipMemcpyAsync(cnt2, c->d_counter, sizeof cnt2, hipMemcpyDeviceToHost, c->stream));
        const spkd_status st = call.finish();
        c->last_gw_items = (int64_t)cnt2[1];
        if (st != SPKD_OK) return st;
        if (!batch->have_lines) return fail(c, SPKD_EHIP, "internal error: no lines from a clean call");
        return gw_batch_finish(c, *batch, n_turns, P->rate);
    }
    for (const GwEventArray& a : GW_EVENT_ARRAYS)
        HIPCHK(c, hipMemcpyAsync(get_pointer(&out, a.host), get_pointer(&ev, a.dev), ev_bytes(a), hipMemcpyDeviceToHost,
                                 c->stream));
    HIPCHK(c, hipMemcpyAsync(cnt2, c->d_counter, sizeof cnt2, hipMemcpyDeviceToHost, c->stream));
    const spkd_status st = call.finish();
    c->last_gw_items = (int64_t)cnt2[1];
    if (out.h_log_count) *out.h_log_count = (int64_t)cnt;
    if (out.h_log && log_cap > 0 && cnt > 0) {
        const size_t ncopy = (size_t)std::min<int64_t>((int64_t)cnt, log_cap);
        HIPCHK(c, hipMemcpy(out.h_log, d_log, ncopy * sizeof(spkd_cand_log), hipMemcpyDeviceToHost));
    }
    if (st == SPKD_OK && (int64_t)cnt > log_cap && out.h_log)
        return fail(c, SPKD_EOVERFLOW, "candidate log too small");
    return st;
}

// the growing-window call of the three entry points that copy the event arrays to the host
// (d_seg_stats: nullptr unless fused)
spkd_status gw_to_host(spkd_ctx* c, const float* d_frames, int64_t n_frames, const int64_t* hb,
                       const int64_t* he, int64_t n_turns, const spkd_cd_params* P, const int64_t* h_ev_off,
                       int check_capacity, int32_t* h_n_win, double* h_win_maxd, int32_t* h_win_det,
                       double* h_det_start, double* h_det_maxi, double* h_det_d, double* h_final_start,
                       double* d_seg_stats, spkd_cand_log* h_log, int64_t log_cap, int64_t* h_log_count) {
    GwIn in;
    in.d_frames = d_frames; in.n_frames = n_frames; in.hb = hb; in.he = he; in.n_turns = n_turns;
    in.P = P; in.h_ev_off = h_ev_off; in.check_capacity = check_capacity; in.d_seg_stats = d_seg_stats;
    GwOut out;
    out.h_n_win = h_n_win; out.h_win_maxd = h_win_maxd; out.h_win_det = h_win_det; out.h_det_start = h_det_start;
    out.h_det_maxi = h_det_maxi; out.h_det_d = h_det_d; out.h_final_start = h_final_start;
    out.h_log = h_log; out.log_cap = log_cap; out.h_log_count = h_log_count;
    return gw_impl(c, in, out);
}
}  // namespace

spkd_status spkd_gw(spkd_ctx* c, const float* d_frames, int64_t n_frames, const int64_t* hb,
                    const int64_t* he, int64_t n_turns, const spkd_cd_params* P, const int64_t* h_ev_off,
                    int32_t* h_n_win, double* h_win_maxd, int32_t* h_win_det, double* h_det_start,
                    double* h_det_maxi, double* h_det_d, double* h_final_start, spkd_cand_log* h_log,
                    int64_t log_cap, int64_t* h_log_count) {
    return gw_to_host(c, d_frames, n_frames, hb, he, n_turns, P, h_ev_off, 1, h_n_win, h_win_maxd, h_win_det,
                      h_det_start, h_det_maxi, h_det_d, h_final_start, nullptr, h_log, log_cap, h_log_count);
}

spkd_status spkd_gw_ex(spkd_ctx* c, const float* d_frames, int64_t n_frames, const int64_t* hb,
                       const int64_t* he, int64_t n_turns, const spkd_cd_params* P, const int64_t* h_ev_off,
                       int check_capacity, int32_t* h_n_win, double* h_win_maxd, int32_t* h_win_det,
                       double* h_det_start, double* h_det_maxi, double* h_det_d, double* h_final_start,
                       spkd_cand_log* h_log, int64_t log_cap, int64_t* h_log_count) {
    return gw_to_host(c, d_frames, n_frames, hb, he, n_turns, P, h_ev_off, check_capacity, h_n_win, h_win_maxd,
                      h_win_det, h_det_start, h_det_maxi, h_det_d, h_final_start, nullptr, h_log, log_cap, h_log_count);
}

spkd_status spkd_gw_fused(spkd_ctx* c, const float* d_frames, int64_t n_frames, const int64_t* hb,
                          const int64_t* he, int64_t n_turns, const spkd_cd_params* P, const int64_t* h_ev_off,
                          int check_capacity, int32_t* h_n_win, double* h_win_maxd, int32_t* h_win_det,
                          double* h_det_start, double* h_det_maxi, double* h_det_d, double* h_final_start,
                          double* d_seg_stats, spkd_cand_log* h_log, int64_t log_cap, int64_t* h_log_count) {
    if (c && !d_seg_stats) return fail(c, SPKD_EINVAL, "gw_fused: null statistics buffer");
    return gw_to_host(c, d_frames, n_frames, hb, he, n_turns, P, h_ev_off, check_capacity, h_n_win, h_win_maxd,
                      h_win_det, h_det_start, h_det_maxi, h_det_d, h_final_start, d_seg_stats, h_log, log_cap,
                      h_log_count);
}

spkd_status spkd_gw_batch(spkd_ctx* c, const float* d_frames, int64_t n_frames, const int64_t* hb,
                          const int64_t* he, int64_t n_turns, const spkd_cd_params* P, const int64_t* h_ev_off,
                          const double* h_turn_start_s, const double* h_turn_end_s, const int64_t* h_turn_file_off,
                          const int64_t* h_turn_file_len, double* d_seg_stats, int want_index,
                          spkd_gw_lines_view* view) {
    if (!c || !view) return SPKD_EINVAL;
    std::memset(view, 0, sizeof *view);
    if (!d_seg_stats) return fail(c, SPKD_EINVAL, "gw_batch: null statistics buffer");
    if (n_turns > 0 && (!h_turn_start_s || !h_turn_end_s || !h_turn_file_off || !h_turn_file_len))
        return fail(c, SPKD_EINVAL, "gw_batch: null turn arrays");
    GwBatch G;
    G.turn_start_s = h_turn_start_s;
    G.turn_end_s = h_turn_end_s;
    G.file_off = h_turn_file_off;
    G.file_len = h_turn_file_len;
    G.want_index = want_index;
    G.view = view;
    GwIn in;
    in.d_frames = d_frames; in.n_frames = n_frames; in.hb = hb; in.he = he; in.n_turns = n_turns;
    in.P = P; in.h_ev_off = h_ev_off; in.d_seg_stats = d_seg_stats;
    const spkd_status st = gw_impl(c, in, GwOut(), &G);
    if (st != SPKD_OK) std::memset(view, 0, sizeof *view);
    return st;
}

spkd_status spkd_ahc_fused(spkd_ctx* c, const float* d_frames, int64_t n_frames, const double* d_records,
                           int64_t n_records, int64_t* d_line_index, const int64_t* h_seg_off, int64_t n_prob,
                           const int64_t* h_redo_line, const int64_t* h_redo_begin, const int64_t* h_redo_end,
                           int64_t n_redo, const spkd_ahc_params* P, const int32_t** h_n_merges,
                           const int32_t** h_merge_a, const int32_t** h_merge_b, const double** h_merge_d,
                           const int32_t** h_labels) {
    if (!c || !P || n_prob < 0 || n_redo < 0) return SPKD_EINVAL;
    if (!h_n_merges || !h_merge_a || !h_merge_b || !h_merge_d || !h_labels)
        return fail(c, SPKD_EINVAL, "ahc_fused: null output");
    *h_n_merges = *h_merge_a = *h_merge_b = *h_labels = nullptr;
    *h_merge_d = nullptr;
    if (n_prob == 0) return SPKD_OK;
    if (!d_records || !d_line_index || !h_seg_off || n_records < 1 || h_seg_off[0] != 0)
        return fail(c, SPKD_EINVAL, "ahc_fused: null argument or first offset not 0");
    for (int64_t p = 0; p < n_prob; ++p)
        if (h_seg_off[p + 1] < h_seg_off[p]) return fail(c, SPKD_EINVAL, "seg_off must be non-decreasing");
    const int64_t n_total = h_seg_off[n_prob];
    if (n_redo > 0 && (!h_redo_line || !h_redo_begin || !h_redo_end || !d_frames))
        return fail(c, SPKD_EINVAL, "ahc_fused: null redo arrays");
    for (int64_t k = 0; k < n_redo; ++k)
        if (h_redo_line[k] < 0 || h_redo_line[k] >= n_total || (k > 0 && h_redo_line[k] <= h_redo_line[k - 1]))
            return fail(c, SPKD_EINVAL, "ahc_fused: redo lines must be ascending line indices");
    const size_t nt = (size_t)n_total, np = (size_t)n_prob;
    double *md, *smax, *smin;
    int32_t *ma, *mb, *lab, *nm;
    // merge_d | stat_max | stat_min | merge_a | merge_b | labels | n_merges
    TRY(carve(c, pinned, PIN_AHC_OUT, [&](Layout L) {
        return L.part(md, nt).part(smax, np).part(smin, np).part(ma, nt).part(mb, nt).part(lab, nt).part(nm, np).bytes();
    }));
    MatrixPlan plan;
    plan.d_map = d_line_index;
    plan.n_src = n_records;
    plan.d_frames = d_frames;
    plan.n_frames = n_frames;
    plan.redo_line = h_redo_line;
    plan.redo_begin = h_redo_begin;
    plan.redo_end = h_redo_end;
    plan.n_redo = n_redo;
    TRY(ahc_impl(c, d_records, h_seg_off, n_prob, P, plan, nm, ma, mb, md, smax, smin));
    if (spkd_labels_from_merges_batch(n_prob, h_seg_off, nm, ma, mb, lab) != SPKD_OK)
        return fail(c, SPKD_EHIP, "internal error: merge log does not replay");
    *h_n_merges = nm;
    *h_merge_a = ma;
    *h_merge_b = mb;
    *h_merge_d = md;
    *h_labels = lab;
    return SPKD_OK;
}

spkd_status spkd_gather_stats(spkd_ctx* c, const double* d_src, int64_t n_src, const int64_t* h_src_index,
                              const int64_t* h_dst_index, int64_t n, int64_t n_dst, double* d_dst) {
    if (!c || n < 0) return SPKD_EINVAL;
    if (n == 0) return SPKD_OK;
    if (!d_src || !h_src_index || !d_dst) return fail(c, SPKD_EINVAL, "null argument");
    for (int64_t i = 0; i < n; ++i) {
        if (h_src_index[i] < 0 || h_src_index[i] >= n_src) return fail(c, SPKD_EINVAL, "gather: source index out of range");
        const int64_t d = h_dst_index ? h_dst_index[i] : i;
        if (d < 0 || d >= n_dst) return fail(c, SPKD_EINVAL, "gather: destination index out of range");
    }
    Call call(c);
    TRY(call.opened);
    int64_t *d_si = nullptr, *d_di = nullptr;
    TRY(upload(c, S_IDXA, h_src_index, (size_t)n, &d_si));
    if (h_dst_index) TRY(upload(c, S_IDXB, h_dst_index, (size_t)n, &d_di));
    hipLaunchKernelGGL(k_gather_records, dim3((unsigned)n), dim3(256), 0, c->stream, d_src,
                       (const int64_t*)d_si, (const int64_t*)d_di, n, d_dst);
    HIPCHK(c, hipGetLastError());
    return call.finish();
}

spkd_status spkd_sum_stats(spkd_ctx* c, const double* d_src, int64_t n_src, const int64_t* h_member,
                           const int64_t* h_set_off, int64_t n_sets, double* d_dst) {
    if (!c || n_sets < 0) return SPKD_EINVAL;
    if (n_sets == 0) return SPKD_OK;
    if (!d_src || !h_member || !h_set_off || !d_dst) return fail(c, SPKD_EINVAL, "null argument");
    if (n_sets > 0x7fffffff) return fail(c, SPKD_EINVAL, "sum_stats: too many sets");
    if (h_set_off[0] != 0) return fail(c, SPKD_EINVAL, "set_off must start at 0");
    for (int64_t s = 0; s < n_sets; ++s)
        if (h_set_off[s + 1] <= h_set_off[s])
            return fail(c, SPKD_EINVAL, h_set_off[s + 1] < h_set_off[s] ? "set_off must be non-decreasing" : "sum_stats: an empty set");
    const int64_t n_mem = h_set_off[n_sets];
    for (int64_t i = 0; i < n_mem; ++i)
        if (h_member[i] < 0 || h_member[i] >= n_src) return fail(c, SPKD_EINVAL, "sum_stats: member out of range");
    const uintptr_t s0 = (uintptr_t)d_src, s1 = s0 + (uintptr_t)n_src * REC * sizeof(double);
    const uintptr_t t0 = (uintptr_t)d_dst, t1 = t0 + (uintptr_t)n_sets * REC * sizeof(double);
    if (s0 % 16 || t0 % 16) return fail(c, SPKD_EINVAL, "sum_stats: record buffers must be 16-byte aligned");
    if (s0 < t1 && t0 < s1) return fail(c, SPKD_EINVAL, "sum_stats: the destination overlaps the source");
    const size_t ns = (size_t)n_sets, nm = (size_t)n_mem;
    struct Tab { int64_t *off, *member; };
    auto tab = mirror<Tab>([&](Layout L, Tab& t) { return L.part(t.off, ns + 1).part(t.member, nm).bytes(); });
    TRY(stage(c, PIN_SUM_IDX, tab));
    std::memcpy(tab.h.off, h_set_off, (ns + 1) * sizeof(int64_t));
    std::memcpy(tab.h.member, h_member, nm * sizeof(int64_t));
    Call call(c);
    TRY(call.opened);
    TRY(send(call, S_SUM_IDX, tab));
    {
        Timer t(c, SPKD_T_REDUCE_SETS);
        hipLaunchKernelGGL(k_sum_records, dim3((unsigned)n_sets), dim3(SUM_TPB), 0, c->stream, d_src,
                           (const int64_t*)tab.d.member, (const int64_t*)tab.d.off, d_dst);
    }
    HIPCHK(c, hipGetLastError());
    return call.finish();
}

// Sliding window (dist_sw, spk-change-detection.py:304-312): window w of a turn compares the
// frames [a, a + size) with [a + size, a + 2 size), a = int(w * step).  Every window is a pair
// distance between two frame sets, which is what the clustering kernels compute: the two
// statistics records of every window come from the frames (k_chunk_stats / k_reduce_sets: a
// window re-reads 2 size / step times the frames of its step, from L2 -- 9 M frame reads for
// a 1 h turn at the default 5 s / 0.5 s, under a millisecond), their log dets / KL2 vectors
// from k_cluster_prep (four records per wave) and the pooled (BIC) or within (GLR) term from
// k_matrix, every window a two-record "problem": the quad elimination and its pivoting
// fallback serve this mode too, no sliding-window kernel of its own.
spkd_status spkd_sw(spkd_ctx* c, const float* d_frames, int64_t n_frames, const int64_t* hb,
                    const int64_t* he, int64_t n_turns, const spkd_cd_params* P, const int64_t* h_d_off,
                    double* h_d) {
    if (!c || !P || n_turns < 0) return SPKD_EINVAL;
    if (n_turns == 0) return SPKD_OK;
    if (!d_frames || !hb || !he || !h_d_off || !h_d) return fail(c, SPKD_EINVAL, "null argument");
    if (bad_kind(P->kind)) return fail(c, SPKD_EINVAL, "bad kind");
    if (!(P->winsize >= 1.0) || !(P->winstep >= 1.0)) return fail(c, SPKD_EINVAL, "sw: window and step must be >= 1 frame");
    const int64_t n_d = h_d_off[n_turns];
    std::vector<int64_t> rb, re;
    std::vector<int32_t> rs;
    rb.reserve((size_t)(2 * n_d)); re.reserve((size_t)(2 * n_d)); rs.reserve((size_t)(2 * n_d));
    const int64_t wsz = (int64_t)P->winsize;
    for (int64_t t = 0; t < n_turns; ++t) {
        if (hb[t] < 0 || he[t] < hb[t] || he[t] > n_frames) return fail(c, SPKD_EINVAL, "bad turn range");
        const int64_t len = he[t] - hb[t];
        const int64_t W = spkd_sw_window_count(len, P->winsize, P->winstep);
        if (h_d_off[t + 1] - h_d_off[t] != W) return fail(c, SPKD_EINVAL, "sw: offsets do not match spkd_sw_window_count");
        for (int64_t w = 0; w < W; ++w) {
            const int64_t a = hb[t] + (int64_t)((double)w * P->winstep);
            const int32_t s0 = (int32_t)(2 * (h_d_off[t] + w));
            rb.push_back(a); re.push_back(a + wsz); rs.push_back(s0);
            rb.push_back(a + wsz); re.push_back(a + 2 * wsz); rs.push_back(s0 + 1);
        }
    }
    if (n_d == 0) return SPKD_OK;
    if (2 * n_d > 0x7fffffffLL) return fail(c, SPKD_EINVAL, "sw: too many windows in one call");
    std::vector<Chunk> chunks;
    std::vector<int64_t> set_off;
    AhcPrep B;
    Call call(c);
    TRY(call.opened);
    spkd_cd_params Pk;
    TRY(kernel_params(c, P, Pk));
    void *d_rec = nullptr, *d_out = nullptr;
    // (borrowed from the growing-window call: the two never share a call)
    TRY(scratch(c, S_SNAP, (size_t)(2 * n_d) * REC * sizeof(double), &d_rec));
    TRY(scratch(c, S_GW_WIN_MAXD, (size_t)n_d * sizeof(double), &d_out));
    {
        Timer t(c, SPKD_T_SW);
        TRY(set_stats_launch(c, d_frames, n_frames, rb.data(), re.data(), rs.data(), 2 * n_d, 2 * n_d, (double*)d_rec,
                             chunks, set_off));
        std::vector<int64_t> seg_off((size_t)n_d + 1);
        for (int64_t w = 0; w <= n_d; ++w) seg_off[(size_t)w] = 2 * w;
        TRY(ahc_prepare(c, (const double*)d_rec, seg_off.data(), n_d, 1, P->kind, P->lambdac, B));
        hipLaunchKernelGGL(k_take_pair_distance, dim3((unsigned)((n_d + 255) / 256)), dim3(256), 0, c->stream,
                           (const double*)B.mat, n_d, (double*)d_out);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_d, d_out, (size_t)n_d * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return call.finish();
}

// ---- sliding window for a whole batch (spkd_sw_batch, spkd_sw_runs)
namespace {
// windows per tile when the caller leaves the choice to the library: per window the tile holds two
// packed and two quad records, their log dets and KL2 vectors and a 2 x 2 matrix, 45.8 KB
constexpr int64_t SW_TILE_WINDOWS = 4096;

// where the positive-run pass leaves its results on the host
struct SwRunsOut {
    int32_t* n_det;
    double *det_start, *det_maxi, *det_d, *final_start;
    int64_t* win_cnt;
    double *win_max, *win_min, *det_max, *det_min;
    bool complete() const {
        return n_det && det_start && det_maxi && det_d && final_start && win_cnt && win_max && win_min && det_max && det_min;
    }
};

// the checks of the two calls on the per-turn offsets: windows from 0 and non-decreasing, event
// slots per turn at least the bound windows / 2 + 1
spkd_status sw_check_offsets(spkd_ctx* c, const int64_t* h_d_off, const int64_t* h_ev_off, int64_t n_turns) {
    if (h_d_off[0] != 0 || h_ev_off[0] < 0) return fail(c, SPKD_EINVAL, "sw: offsets must start at 0");
    for (int64_t t = 0; t < n_turns; ++t) {
        const int64_t W = h_d_off[t + 1] - h_d_off[t];
        if (W < 0) return fail(c, SPKD_EINVAL, "sw: offsets must be non-decreasing");
        if (h_ev_off[t + 1] - h_ev_off[t] < W / 2 + 1)
            return fail(c, SPKD_EINVAL, "sw: event capacity below windows / 2 + 1");
    }
    return SPKD_OK;
}

// the per-turn tables of the two calls on the device; begin / end only with frames
struct SwTurns {
    int64_t *begin = nullptr, *end = nullptr, *d_off = nullptr, *ev_off = nullptr;
    std::vector<char> image;
};

spkd_status sw_upload_turns(spkd_ctx* c, SwTurns& T, const int64_t* hb, const int64_t* he, const int64_t* h_d_off,
                            const int64_t* h_ev_off, int64_t n_turns) {
    const size_t nt = (size_t)n_turns;
    return upload_parts(c, S_TURNS, T.image, [&](Layout L) {
        if (hb) L.part(T.begin, nt, hb).part(T.end, nt, he);
        return L.part(T.d_off, nt + 1, h_d_off).part(T.ev_off, nt + 1, h_ev_off).bytes();
    });
}

// k_sw_runs over d_dist and the copies of its results, inside the caller's bracket
spkd_status sw_runs_enqueue(spkd_ctx* c, const double* d_dist, const SwTurns& T, int64_t n_turns, int64_t n_ev,
                            const spkd_cd_params* P, const SwRunsOut& out) {
    const size_t nt = (size_t)n_turns, ne = (size_t)n_ev;
    int32_t* n_det;
    double *det_start, *det_maxi, *det_d, *final_start;
    SwTurnStats st;
    TRY(carve(c, scratch, S_GW_DET_START, [&](Layout L) {
        return L.part(det_start, ne).part(det_maxi, ne).part(det_d, ne).part(final_start, nt).part(st.win_max, nt)
            .part(st.win_min, nt).part(st.det_max, nt).part(st.det_min, nt).part(st.win_cnt, nt).part(n_det, nt).bytes();
    }));
    hipLaunchKernelGGL(k_sw_runs, dim3((unsigned)n_turns), dim3(WAVE), 0, c->stream, d_dist, (const int64_t*)T.d_off,
                       (const int64_t*)T.ev_off, n_turns, P->winsize, P->winstep, P->threshold, n_det, det_start,
                       det_maxi, det_d, final_start, st, c->d_err);
    HIPCHK(c, hipGetLastError());
    auto back = [&](void* h, const void* d, size_t bytes) {
        return bytes ? hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    };
    HIPCHK(c, back(out.n_det, n_det, nt * sizeof(int32_t)));
    HIPCHK(c, back(out.det_start, det_start, ne * sizeof(double)));
    HIPCHK(c, back(out.det_maxi, det_maxi, ne * sizeof(double)));
    HIPCHK(c, back(out.det_d, det_d, ne * sizeof(double)));
    HIPCHK(c, back(out.final_start, final_start, nt * sizeof(double)));
    HIPCHK(c, back(out.win_cnt, st.win_cnt, nt * sizeof(int64_t)));
    HIPCHK(c, back(out.win_max, st.win_max, nt * sizeof(double)));
    HIPCHK(c, back(out.win_min, st.win_min, nt * sizeof(double)));
    HIPCHK(c, back(out.det_max, st.det_max, nt * sizeof(double)));
    HIPCHK(c, back(out.det_min, st.det_min, nt * sizeof(double)));
    return SPKD_OK;
}
}  // namespace

spkd_status spkd_sw_runs(spkd_ctx* c, const double* d_dist, const int64_t* h_d_off, int64_t n_turns,
                         const spkd_cd_params* P, const int64_t* h_ev_off, int32_t* h_n_det, double* h_det_start,
                         double* h_det_maxi, double* h_det_d, double* h_final_start, int64_t* h_win_cnt,
                         double* h_win_max, double* h_win_min, double* h_det_max, double* h_det_min) {
    if (!c || !P || n_turns < 0) return SPKD_EINVAL;
    if (n_turns == 0) return SPKD_OK;
    const SwRunsOut out = {h_n_det, h_det_start, h_det_maxi, h_det_d, h_final_start,
                           h_win_cnt, h_win_max, h_win_min, h_det_max, h_det_min};
    if (!h_d_off || !h_ev_off || !out.complete()) return fail(c, SPKD_EINVAL, "null argument");
    if (!(P->winsize >= 1.0) || !(P->winstep >= 1.0)) return fail(c, SPKD_EINVAL, "sw: window and step must be >= 1 frame");
    TRY(sw_check_offsets(c, h_d_off, h_ev_off, n_turns));
    if (h_d_off[n_turns] > 0 && !d_dist) return fail(c, SPKD_EINVAL, "null argument");
    SwTurns T;
    Call call(c);
    TRY(call.opened);
    TRY(sw_upload_turns(c, T, nullptr, nullptr, h_d_off, h_ev_off, n_turns));
    {
        Timer t(c, SPKD_T_SW);
        TRY(sw_runs_enqueue(c, d_dist, T, n_turns, h_ev_off[n_turns], P, out));
    }
    return call.finish();
}

// One call for every turn of every file.  The windows, counted flat over the turns, are taken in
// tiles of tile_windows: per tile k_sw_window_stats writes the two records of every window,
// k_cluster_prep and k_matrix turn them into distances exactly as spkd_sw does (every window a
// two-record problem; only the row of its left record is launched, the right one's would write
// nothing but a diagonal cell), and the distances land in the tile's slice of d_dist.  The
// scratch of the records and working copies is the tile's; the tables that say "window p owns
// records 2 p, 2 p + 1 and cells 4 p .." are the same for every tile and go up once.  Then
// k_sw_runs walks d_dist per turn.
spkd_status spkd_sw_batch(spkd_ctx* c, const float* d_frames, int64_t n_frames, const int64_t* hb,
                          const int64_t* he, int64_t n_turns, const spkd_cd_params* P, const int64_t* h_d_off,
                          const int64_t* h_ev_off, int64_t tile_windows, int32_t* h_n_det, double* h_det_start,
                          double* h_det_maxi, double* h_det_d, double* h_final_start, int64_t* h_win_cnt,
                          double* h_win_max, double* h_win_min, double* h_det_max, double* h_det_min, double* h_d) {
    if (!c || !P || n_turns < 0) return SPKD_EINVAL;
    if (n_turns == 0) return SPKD_OK;
    const SwRunsOut out = {h_n_det, h_det_start, h_det_maxi, h_det_d, h_final_start,
                           h_win_cnt, h_win_max, h_win_min, h_det_max, h_det_min};
    if (!d_frames || !hb || !he || !h_d_off || !h_ev_off || !out.complete()) return fail(c, SPKD_EINVAL, "null argument");
    if (bad_kind(P->kind)) return fail(c, SPKD_EINVAL, "bad kind");
    if (!(P->winsize >= 1.0) || !(P->winstep >= 1.0)) return fail(c, SPKD_EINVAL, "sw: window and step must be >= 1 frame");
    if (tile_windows < 0) return fail(c, SPKD_EINVAL, "sw_batch: negative tile_windows");
    const int64_t wsz = (int64_t)P->winsize;
    for (int64_t t = 0; t < n_turns; ++t) {
        if (hb[t] < 0 || he[t] < hb[t] || he[t] > n_frames) return fail(c, SPKD_EINVAL, "bad turn range");
        const int64_t W = spkd_sw_window_count(he[t] - hb[t], P->winsize, P->winstep);
        if (h_d_off[t + 1] - h_d_off[t] != W) return fail(c, SPKD_EINVAL, "sw: offsets do not match spkd_sw_window_count");
        // (the count walks s += step, the geometry multiplies: the last window must still end inside the turn)
        if (W > 0 && hb[t] + (int64_t)((double)(W - 1) * P->winstep) + 2 * wsz > he[t])
            return fail(c, SPKD_EINVAL, "sw: a window ends behind its turn");
    }
    TRY(sw_check_offsets(c, h_d_off, h_ev_off, n_turns));
    const int64_t n_d = h_d_off[n_turns];
    const int64_t tile = std::min(tile_windows ? tile_windows : SW_TILE_WINDOWS, std::min<int64_t>(n_d, 0x3fffffff));
    const size_t nw = (size_t)tile;
    // the tile's tables: window p is the problem of records 2 p, 2 p + 1 with cells 4 p ..; block b computes the
    // row of record 2 b
    std::vector<int64_t> seg_off(nw + 1), mat_off(nw + 1);
    std::vector<int32_t> prob(2 * nw), sched(nw);
    for (size_t p = 0; p <= nw; ++p) { seg_off[p] = 2 * (int64_t)p; mat_off[p] = 4 * (int64_t)p; }
    for (size_t p = 0; p < nw; ++p) { prob[2 * p] = prob[2 * p + 1] = (int32_t)p; sched[p] = (int32_t)(2 * p); }
    std::vector<char> offs, prob_of;
    SwTurns T;
    Call call(c);
    TRY(call.opened);
    spkd_cd_params Pk;
    TRY(kernel_params(c, P, Pk));
    TRY(sw_upload_turns(c, T, hb, he, h_d_off, h_ev_off, n_turns));
    void* d_dist = nullptr;
    TRY(scratch(c, S_GW_WIN_MAXD, (size_t)n_d * sizeof(double), &d_dist));
    {
        Timer timer(c, SPKD_T_SW);
        if (n_d > 0) {
            int64_t *d_segoff, *d_matoff;
            int32_t *d_prob, *d_sched;
            double *rec, *ex, *ld, *aux, *mat;
            unsigned long long *smax, *smin;
            TRY(upload_parts(c, S_AHC_OFF, offs, [&](Layout L) {
                return L.part(d_segoff, nw + 1, seg_off.data()).part(d_matoff, nw + 1, mat_off.data()).bytes();
            }));
            TRY(upload_parts(c, S_AHC_PROB, prob_of, [&](Layout L) {
                return L.part(d_prob, 2 * nw, prob.data()).part(d_sched, nw, sched.data()).bytes();
            }));
            // (the records are borrowed from the growing-window call, as in spkd_sw; nothing merges
            // here, so they serve as the packed working copies too)
            TRY(carve(c, scratch, S_SNAP, [&](Layout L) { return L.part(rec, 2 * nw * REC).bytes(); }));
            TRY(carve(c, scratch, S_AHC_STATS, [&](Layout L) { return L.part(ex, 2 * nw * QREC).bytes(); }));
            TRY(carve(c, scratch, S_AHC_LD, [&](Layout L) { return L.part(ld, 2 * nw).bytes(); }));
            TRY(carve(c, scratch, S_AHC_AUX, [&](Layout L) { return L.part(aux, 2 * nw * AUX).bytes(); }));
            TRY(carve(c, scratch, S_AHC_MAT, [&](Layout L) { return L.part(mat, 4 * nw).bytes(); }));
            TRY(carve(c, scratch, S_AHC_MISC, [&](Layout L) { return L.part(smax, nw).part(smin, nw).bytes(); }));
            HIPCHK(c, hipMemsetAsync(smax, 0x00, nw * sizeof(unsigned long long), c->stream));
            HIPCHK(c, hipMemsetAsync(smin, 0xff, nw * sizeof(unsigned long long), c->stream));
            auto kmat = P->kind == SPKD_GLR ? k_matrix<true> : k_matrix<false>;
            for (int64_t w0 = 0; w0 < n_d; w0 += tile) {
                const int64_t n = std::min(tile, n_d - w0);
                hipLaunchKernelGGL(k_sw_window_stats, dim3((unsigned)n), dim3(STATS_TPB), 0, c->stream, d_frames,
                                   (const int64_t*)T.begin, (const int64_t*)T.end, (const int64_t*)T.d_off, n_turns, w0,
                                   P->winstep, wsz, rec, c->d_err);
                to_quadrec(c, rec, 2 * n, ex);
                cluster_prep(c, ex, 2 * n, P->kind, ld, aux);
                hipLaunchKernelGGL(kmat, dim3((unsigned)n), dim3(MX_WAVES * WAVE), 0, c->stream, (const double*)ex,
                                   (const double*)rec, (const int64_t*)d_segoff, (const int32_t*)d_prob,
                                   (const int32_t*)d_sched, 1, P->kind, P->lambdac, (const double*)ld, (const double*)aux,
                                   mat, (const int64_t*)d_matoff, smax, smin, c->d_err);
                hipLaunchKernelGGL(k_take_pair_distance, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                                   (const double*)mat, n, (double*)d_dist + w0);
                HIPCHK(c, hipGetLastError());
            }
        }
        TRY(sw_runs_enqueue(c, (const double*)d_dist, T, n_turns, h_ev_off[n_turns], P, out));
    }
    if (h_d && n_d > 0)
        HIPCHK(c, hipMemcpyAsync(h_d, d_dist, (size_t)n_d * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return call.finish();
}

// ---- neighbour merge for a whole batch (spkd_merge_batch)
// One record per line and per non-empty gap between two lines of a problem, in one statistics
// pass (each frame is read once); the lines' records first, so that every per-line array is
// indexed like the caller's.  Then flags, the lines' own terms, the ahead pass and the chain
// (spkd_merge.hpp).  The problems' error words are the chain's: k_cluster_prep_batch and the
// ahead pass, which also touch lines no step reaches, get words of their own that nobody reads.
spkd_status spkd_merge_batch(spkd_ctx* c, const float* d_frames, int64_t n_frames, int64_t n_prob,
                             const int64_t* h_line_off, const int64_t* hb, const int64_t* he, int kind, double lambdac,
                             double threshold, int flags, int32_t* h_merged, double* h_dist, int64_t* h_n_done,
                             int64_t* h_win_cnt, double* h_win_max, double* h_win_min, int64_t* h_det_cnt,
                             double* h_det_max, double* h_det_min) {
    if (!c || n_prob < 0 || bad_kind(kind)) return SPKD_EINVAL;
    if (n_prob == 0) return SPKD_OK;
    if (!h_line_off || !h_n_done || !h_win_cnt || !h_win_max || !h_win_min || !h_det_cnt || !h_det_max || !h_det_min)
        return fail(c, SPKD_EINVAL, "null argument");
    if (h_line_off[0] != 0) return fail(c, SPKD_EINVAL, "line_off must start at 0");
    int64_t longest = 0;
    for (int64_t p = 0; p < n_prob; ++p) {
        if (h_line_off[p + 1] < h_line_off[p]) return fail(c, SPKD_EINVAL, "line_off must be non-decreasing");
        longest = std::max(longest, h_line_off[p + 1] - h_line_off[p]);
    }
    if (longest > 65536) return fail(c, SPKD_EINVAL, "merge_batch: a problem of more than 65 536 lines");
    const int64_t n = h_line_off[n_prob];
    if (n > 0x3fffffff) return fail(c, SPKD_EINVAL, "merge_batch: too many lines");
    if (n > 0 && (!d_frames || !hb || !he || !h_merged || !h_dist)) return fail(c, SPKD_EINVAL, "null argument");
    // ranges of the statistics pass: line k is set k, the gaps follow in line order
    std::vector<int64_t> rb(hb, hb + n), re(he, he + n);
    std::vector<int32_t> rs((size_t)n), gap_rec((size_t)n, -1);
    for (int64_t p = 0; p < n_prob; ++p)
        for (int64_t k = h_line_off[p]; k < h_line_off[p + 1]; ++k) {
            if (hb[k] < 0 || he[k] < hb[k] || he[k] > n_frames) return fail(c, SPKD_EINVAL, "bad line range");
            rs[(size_t)k] = (int32_t)k;
            if (k == h_line_off[p]) continue;
            if (hb[k] < he[k - 1]) return fail(c, SPKD_EINVAL, "merge_batch: lines of a problem overlap or go backwards");
            if (hb[k] > he[k - 1]) {
                gap_rec[(size_t)k - 1] = (int32_t)rs.size();
                rs.push_back((int32_t)rs.size());
                rb.push_back(he[k - 1]);
                re.push_back(hb[k]);
            }
        }
    const int64_t n_rec = (int64_t)rs.size();
    const size_t nn = (size_t)n, nr = (size_t)n_rec, np = (size_t)n_prob;
    std::vector<Chunk> chunks;
    std::vector<int64_t> set_off;
    std::vector<char> tables;
    Call call(c);
    TRY(call.opened);
    TRY(use_kind(c, kind, &kind));
    int64_t* d_lineoff = nullptr;
    int32_t* d_gaprec = nullptr;
    TRY(upload_parts(c, S_AHC_OFF, tables, [&](Layout L) {
        return L.part(d_lineoff, np + 1, h_line_off).part(d_gaprec, nn, gap_rec.data()).bytes();
    }));
    double *pk, *ex, *ld, *aux;
    TRY(carve(c, scratch, S_AHC_PACKED, [&](Layout L) { return L.part(pk, nr * REC).bytes(); }));
    TRY(carve(c, scratch, S_AHC_STATS, [&](Layout L) { return L.part(ex, nr * QREC).bytes(); }));
    TRY(carve(c, scratch, S_AHC_LD, [&](Layout L) { return L.part(ld, nn).bytes(); }));
    TRY(carve(c, scratch, S_AHC_AUX, [&](Layout L) { return L.part(aux, nn * AUX).bytes(); }));
    double *ahead, *d_dist;
    MergeStats st;
    long long* d_done;
    int32_t *d_merged, *d_flags;
    int *d_perr, *d_perr_unread;
    // determinants of the ahead pass | distances | per problem: the four extremes, lines done, the two counts |
    // merged | flags of all records | the problems' error words, and the words nobody reads
    TRY(carve(c, scratch, S_STEP_MISC, [&](Layout L) {
        return L.part(ahead, nn).part(d_dist, nn).part(st.win_max, np).part(st.win_min, np).part(st.det_max, np)
            .part(st.det_min, np).part(d_done, np).part(st.win_cnt, np).part(st.det_cnt, np).part(d_merged, nn)
            .part(d_flags, nr).part(d_perr, np).part(d_perr_unread, np).bytes();
    }));
    HIPCHK(c, hipMemsetAsync(d_perr, 0, 2 * np * sizeof(int), c->stream));
    const bool want_ahead = n > 0 && kind != SPKD_KL2 && !(flags & SPKD_MERGE_NO_AHEAD);
    if (n > 0) {
        TRY(set_stats_launch(c, d_frames, n_frames, rb.data(), re.data(), rs.data(), n_rec, n_rec, pk, chunks, set_off));
        to_quadrec(c, pk, n_rec, ex);
        hipLaunchKernelGGL(k_merge_flags, dim3((unsigned)n_rec), dim3(WAVE), 0, c->stream, (const double*)pk, n_rec, n,
                           d_flags);
        {
            Timer t(c, SPKD_T_CLUSTER_PREP);
            const int64_t per_block = kind == SPKD_KL2 ? PT_WAVES : 4 * PT_WAVES;
            hipLaunchKernelGGL(k_cluster_prep_batch, dim3((unsigned)n_prob, (unsigned)((longest + per_block - 1) / per_block)),
                               dim3(PT_WAVES * WAVE), 0, c->stream, (const double*)ex, (const int64_t*)d_lineoff, kind, ld, aux,
                               d_perr_unread, c->pinv_cur);
        }
        HIPCHK(c, hipGetLastError());
    }
    {
        Timer t(c, SPKD_T_MERGE);
        if (want_ahead) {
            auto kahead = kind == SPKD_GLR ? k_merge_ahead<true> : k_merge_ahead<false>;
            hipLaunchKernelGGL(kahead, dim3((unsigned)((n + MRG_AHEAD_WAVES - 1) / MRG_AHEAD_WAVES)),
                               dim3(MRG_AHEAD_WAVES * WAVE), 0, c->stream, (const double*)ex, (const double*)pk,
                               (const int64_t*)d_lineoff, n_prob, n, kind, ahead, d_perr_unread);
        }
        auto kchain = kind == SPKD_GLR ? k_merge_chain_batch<true> : k_merge_chain_batch<false>;
        hipLaunchKernelGGL(kchain, dim3((unsigned)n_prob), dim3(WAVE), 0, c->stream, (const double*)ex, (const double*)pk,
                           (const double*)ld, (const double*)aux, (const int64_t*)d_lineoff, (const int32_t*)d_gaprec,
                           (const int32_t*)d_flags, want_ahead ? (const double*)ahead : (const double*)nullptr, kind, lambdac,
                           threshold, d_merged, d_dist, d_done, st, d_perr, c->d_err, c->pinv_cur);
    }
    HIPCHK(c, hipGetLastError());
    auto back = [&](void* h, const void* d, size_t bytes) {
        return bytes ? hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    };
    static_assert(sizeof(long long) == sizeof(int64_t), "counters are copied as they are");
    HIPCHK(c, back(h_merged, d_merged, nn * sizeof(int32_t)));
    HIPCHK(c, back(h_dist, d_dist, nn * sizeof(double)));
    HIPCHK(c, back(h_n_done, d_done, np * sizeof(int64_t)));
    HIPCHK(c, back(h_win_cnt, st.win_cnt, np * sizeof(int64_t)));
    HIPCHK(c, back(h_win_max, st.win_max, np * sizeof(double)));
    HIPCHK(c, back(h_win_min, st.win_min, np * sizeof(double)));
    HIPCHK(c, back(h_det_cnt, st.det_cnt, np * sizeof(int64_t)));
    HIPCHK(c, back(h_det_max, st.det_max, np * sizeof(double)));
    HIPCHK(c, back(h_det_min, st.det_min, np * sizeof(double)));
    return call.finish();
}

// ------------------------------------------------------------------ (6) front-end
namespace {
// what spkd_mfcc and spkd_mfcc_batch refuse alike; out: the hop and k_mfcc_post's LDS bytes
spkd_status mfcc_check(spkd_ctx* c, const spkd_mfcc_params* P, const float* h_melfb, const float* h_dct,
                       const float* h_mean, const float* h_scale, const float* h_transform, int* hop, size_t* lds) {
    if (!P || !h_melfb || !h_dct || !h_mean || !h_scale || !h_transform) return fail(c, SPKD_EINVAL, "mfcc: null argument");
    if ((P->window_width != MF_WIN && P->window_width != MF_WIN_VAD) || P->n_fft != MF_NFFT || P->n_mel != MF_MEL ||
        P->n_cep != MF_CEP || P->frame_rate <= 0 || P->sample_rate <= 0 || P->sample_rate % P->frame_rate != 0)
        return fail(c, SPKD_EINVAL, "mfcc: this build does 400- or 256-sample windows, a 512-point transform, 21 mel bins, 12 cepstra");
    if (P->cms_left < 0 || P->cms_right < 0 || P->delta_width[0] < 1 || P->delta_width[0] > 2 || P->delta_width[1] < 1 ||
        P->delta_width[1] > 2 || !(P->delta_norm[0] > 0.f) || !(P->delta_norm[1] > 0.f))
        return fail(c, SPKD_EINVAL, "mfcc: unsupported mean-subtraction window or delta parameters");
    *hop = P->sample_rate / P->frame_rate;
    if (*hop < 1) return fail(c, SPKD_EINVAL, "mfcc: frame rate above the sample rate");
    // left + right <= MP_CMS_MAX is what mp_lds_floats fits into MP_LDS_MAX (compared so that no sum overflows)
    if (P->cms_left > MP_CMS_MAX || P->cms_right > MP_CMS_MAX - P->cms_left)
        return fail(c, SPKD_EINVAL, "mfcc: mean-subtraction window too wide for the LDS tile");
    *lds = (size_t)mp_lds_floats(P->cms_left + P->cms_right) * sizeof(float);
    return SPKD_OK;
}
static_assert(MP_FR == SPKD_MFCC_POST_TILE && MP_HALO == SPKD_MFCC_POST_HALO && MP_LDS_MAX == SPKD_MFCC_POST_LDS &&
              MP_CMS_MAX == SPKD_MFCC_CMS_MAX && MF_STATIC == 13, "the header states the post stage's tile and limit");

extern "C++" {
template <int WIN>
void mfcc_static_launch(spkd_ctx* c, unsigned tiles, const int16_t* d_pcm, const int64_t* d_soff, const int64_t* d_foff,
                        const int64_t* d_tiles, int64_t n_files, int hop, float pre_emph, float2* d_tw, void* d_ham,
                        const float* d_fb, const float* d_dct, float* d_static) {
    hipLaunchKernelGGL(k_mfcc_tables<WIN>, dim3(1), dim3(MF_NFFT), 0, c->stream, d_tw, (double*)d_ham);
    Timer t(c, SPKD_T_MFCC_STATIC);
    hipLaunchKernelGGL(k_mfcc_static<WIN>, dim3(tiles), dim3(MF_STATIC_TPB), 0, c->stream, d_pcm, (const long long*)d_soff,
                       (const long long*)d_foff, (const long long*)d_tiles, (long long)n_files, hop, pre_emph,
                       (const float2*)d_tw, (const double*)d_ham, d_fb, d_dct, d_static);
}
}  // extern "C++"
}  // namespace

spkd_status spkd_mfcc_batch(spkd_ctx* c, const int16_t* d_pcm, int64_t n_files, const int64_t* h_sample_off,
                            const spkd_mfcc_params* P, const float* h_melfb, const float* h_dct, const float* h_mean,
                            const float* h_scale, const float* h_transform, float* d_features, int64_t* h_frame_off) {
    if (!c) return SPKD_EINVAL;
    int hop = 0;
    size_t lds = 0;
    TRY(mfcc_check(c, P, h_melfb, h_dct, h_mean, h_scale, h_transform, &hop, &lds));
    if (n_files < 0 || !h_sample_off || !h_frame_off)
        return fail(c, SPKD_EINVAL, "mfcc_batch: null sample_off / frame_off or a negative file count");
    if (h_sample_off[0] != 0) return fail(c, SPKD_EINVAL, "mfcc_batch: sample_off must start at 0");
    for (int64_t f = 0; f < n_files; ++f)
        if (h_sample_off[f + 1] < h_sample_off[f]) return fail(c, SPKD_EINVAL, "mfcc_batch: sample_off must be non-decreasing");
    // the frame layout, and per stage the running count of tiles: a tile lies in one file
    const size_t n1 = (size_t)n_files + 1;
    std::vector<int64_t> static_tiles(n1, 0), post_tiles(n1, 0);
    h_frame_off[0] = 0;
    for (int64_t f = 0; f < n_files; ++f) {
        const int64_t T = (h_sample_off[f + 1] - h_sample_off[f]) / hop;
        h_frame_off[f + 1] = h_frame_off[f] + T;
        static_tiles[(size_t)f + 1] = static_tiles[(size_t)f] + (T + MF_FR - 1) / MF_FR;
        post_tiles[(size_t)f + 1] = post_tiles[(size_t)f] + (T + MP_FR - 1) / MP_FR;
    }
    const int64_t total = h_frame_off[n_files];
    if (total == 0) return SPKD_OK;
    if (!d_pcm || !d_features) return fail(c, SPKD_EINVAL, "mfcc: null device buffer");
    if (static_tiles[(size_t)n_files] > 0x7fffffffLL) return fail(c, SPKD_EINVAL, "mfcc_batch: too many frames in one call");
    float *d_fb, *d_dct, *d_mean, *d_scale, *d_tr;
    int64_t *d_soff, *d_foff, *d_stiles, *d_ptiles;
    float2* d_tw;
    double* d_ham;                                   // (k_mfcc_tables fills these two; the table's pad entries are never used)
    std::vector<char> tab;
    Call call(c);
    TRY(call.opened);
    void* d_static = nullptr;
    TRY(upload_parts(c, S_MFCC_TAB, tab, [&](Layout L) {
        return L.part(d_fb, MF_MEL * MF_BINS, h_melfb).part(d_dct, MF_CEP * MF_MEL, h_dct).part(d_mean, MF_DIM, h_mean)
            .part(d_scale, MF_DIM, h_scale).part(d_tr, MF_DIM * MF_DIM, h_transform).part(d_soff, n1, h_sample_off)
            .part(d_foff, n1, (const int64_t*)h_frame_off).part(d_stiles, n1, (const int64_t*)static_tiles.data())
            .part(d_ptiles, n1, (const int64_t*)post_tiles.data()).bytes();
    }));
    TRY(carve(c, scratch, S_MFCC_TW, [&](Layout L) { return L.part(d_tw, MF_TW_LEN).part(d_ham, MF_WIN).bytes(); }));
    TRY(scratch(c, S_MFCC_STATIC, (size_t)total * MF_STATIC * sizeof(float), &d_static));
    const unsigned tiles = (unsigned)static_tiles[(size_t)n_files];
    if (P->window_width == MF_WIN)
        mfcc_static_launch<MF_WIN>(c, tiles, d_pcm, d_soff, d_foff, d_stiles, n_files, hop, P->pre_emph, d_tw, d_ham, d_fb,
                                   d_dct, (float*)d_static);
    else
        mfcc_static_launch<MF_WIN_VAD>(c, tiles, d_pcm, d_soff, d_foff, d_stiles, n_files, hop, P->pre_emph, d_tw, d_ham,
                                       d_fb, d_dct, (float*)d_static);
    {
        Timer t(c, SPKD_T_MFCC_POST);
        hipLaunchKernelGGL(k_mfcc_post, dim3((unsigned)post_tiles[(size_t)n_files]), dim3(MF_TPB), lds, c->stream,
                           (const float*)d_static, (const long long*)d_foff, (const long long*)d_ptiles, (long long)n_files,
                           P->cms_left, P->cms_right, P->delta_width[0], P->delta_norm[0], P->delta_width[1],
                           P->delta_norm[1], d_mean, d_scale, d_tr, d_features);
    }
    if (hipGetLastError() != hipSuccess) return fail(c, SPKD_EHIP, "mfcc: kernel launch failed");
    return call.finish();
}

// the batch of one file
spkd_status spkd_mfcc(spkd_ctx* c, const int16_t* d_pcm, int64_t n_samples, const spkd_mfcc_params* P,
                      const float* h_melfb, const float* h_dct, const float* h_mean, const float* h_scale,
                      const float* h_transform, float* d_features, int64_t* h_n_frames) {
    if (!c || !P || !h_n_frames) return SPKD_EINVAL;
    *h_n_frames = 0;
    if (n_samples < 0) return fail(c, SPKD_EINVAL, "mfcc: null argument");
    const int64_t sample_off[2] = {0, n_samples};
    int64_t frame_off[2] = {0, 0};
    const spkd_status st = spkd_mfcc_batch(c, d_pcm, 1, sample_off, P, h_melfb, h_dct, h_mean, h_scale, h_transform,
                                           d_features, frame_off);
    *h_n_frames = frame_off[1];
    return st;
}

// ------------------------------------------------------------------ (6b) sample-rate conversion and downmix
static_assert(RS_TILE == SPKD_RESAMPLE_TILE && RS_MAX_CH == SPKD_RESAMPLE_MAX_CH && RS_MAX_HALF == SPKD_RESAMPLE_MAX_HALF &&
              RS_MAX_TAPS == SPKD_RESAMPLE_MAX_TAPS && RS_MAX_TERM == SPKD_RESAMPLE_MAX_TERM && RS_MAX_SPAN == SPKD_RESAMPLE_MAX_SPAN,
              "the header states the resampler's tile and limits");

spkd_status spkd_resample_batch(spkd_ctx* c, const int16_t* d_in, int64_t n_files, const int64_t* h_in_off,
                                const int32_t* h_channels, const int32_t* h_conv, int32_t n_conv,
                                const spkd_resample_conv* h_convs, const float* h_taps, int16_t* d_out, int64_t* h_out_off) {
    if (!c) return SPKD_EINVAL;
    if (n_files < 0 || n_conv < 0) return fail(c, SPKD_EINVAL, "resample_batch: negative file or conversion count");
    if (!h_in_off || !h_out_off || (n_files > 0 && (!h_channels || !h_conv)) || (n_conv > 0 && !h_convs))
        return fail(c, SPKD_EINVAL, "resample_batch: null host array");
    if (h_in_off[0] != 0) return fail(c, SPKD_EINVAL, "resample_batch: in_off must start at 0");
    for (int64_t f = 0; f < n_files; ++f)
        if (h_in_off[f + 1] < h_in_off[f]) return fail(c, SPKD_EINVAL, "resample_batch: in_off must be non-decreasing");
    for (int64_t f = 0; f < n_files; ++f) {
        if (h_channels[f] < 1 || h_channels[f] > RS_MAX_CH)
            return fail(c, SPKD_EINVAL, "resample_batch: channel count outside [1, 8]");
        if ((h_in_off[f + 1] - h_in_off[f]) % h_channels[f] != 0)
            return fail(c, SPKD_EINVAL, "resample_batch: a file's span is not a multiple of its channel count");
        if (h_conv[f] < 0 || h_conv[f] >= n_conv) return fail(c, SPKD_EINVAL, "resample_batch: conversion index out of range");
    }
    std::vector<RsConv> convs((size_t)n_conv);
    int64_t n_taps = 0;                              // floats of h_taps the conversions reach
    for (int32_t k = 0; k < n_conv; ++k) {
        const spkd_resample_conv& v = h_convs[k];
        if (v.up < 1 || v.down < 1 || v.up > RS_MAX_TERM || v.down > RS_MAX_TERM)
            return fail(c, SPKD_EINVAL, "resample_batch: up and down must lie in [1, 2^20]");
        int a = v.up, b = v.down;
        while (b) { const int t = a % b; a = b; b = t; }
        if (a != 1) return fail(c, SPKD_EINVAL, "resample_batch: up and down must be coprime");
        if (v.half_taps < 0 || v.half_taps > RS_MAX_HALF) return fail(c, SPKD_EINVAL, "resample_batch: half_taps outside [0, 256]");
        if ((v.half_taps == 0) != (v.up == 1 && v.down == 1))
            return fail(c, SPKD_EINVAL, "resample_batch: half_taps is 0 for the identity conversion (up == down == 1) and for no other");
        if (v.taps_off < 0) return fail(c, SPKD_EINVAL, "resample_batch: negative taps_off");
        const int64_t table = (int64_t)v.up * 2 * v.half_taps;
        if (table > RS_MAX_TAPS) return fail(c, SPKD_EINVAL, "resample_batch: a table of more than 2^22 taps");
        if (rs_span(v.up, v.down, v.half_taps) > RS_MAX_SPAN)
            return fail(c, SPKD_EINVAL, "resample_batch: a tile's input span exceeds the LDS (down / up too large for half_taps)");
        if (v.half_taps > 0 && !h_taps) return fail(c, SPKD_EINVAL, "resample_batch: null tables with a filtered conversion");
        if (v.half_taps > 0) n_taps = std::max(n_taps, v.taps_off + table);
        convs[(size_t)k] = RsConv{v.up, v.down, v.half_taps, 0, (long long)v.taps_off};
    }
    // the output layout, and the running count of tiles: a tile lies in one file
    const size_t n1 = (size_t)n_files + 1;
    std::vector<int64_t> tiles(n1, 0);
    h_out_off[0] = 0;
    size_t lds = 0;
    for (int64_t f = 0; f < n_files; ++f) {
        RsConv& v = convs[(size_t)h_conv[f]];
        const int64_t n_in = (h_in_off[f + 1] - h_in_off[f]) / h_channels[f];
        const int64_t n_out = (n_in * v.up + v.down - 1) / v.down;
        h_out_off[f + 1] = h_out_off[f] + n_out;
        tiles[(size_t)f + 1] = tiles[(size_t)f] + (n_out + RS_TILE - 1) / RS_TILE;
        if (n_out == 0 || v.half == 0) continue;
        // the table goes to LDS beside the span where the device admits both
        const size_t span = (size_t)rs_span_bytes(v.up, v.down, v.half), both = span + (size_t)rs_table_bytes(v.up, v.half);
        v.in_lds = both <= (size_t)c->rs_lds_cap;
        lds = std::max(lds, v.in_lds ? both : span);
    }
    if (h_out_off[n_files] == 0) return SPKD_OK;
    if (!d_in || !d_out) return fail(c, SPKD_EINVAL, "resample_batch: null device buffer");
    if (tiles[(size_t)n_files] > 0x7fffffffLL) return fail(c, SPKD_EINVAL, "resample_batch: too many samples in one call");
    if (lds > (size_t)c->rs_lds_cap)
        return fail(c, SPKD_EHIP, "resample_batch: the kernel's dynamic LDS size was not admitted on this device");
    int64_t *d_ioff, *d_ooff, *d_tiles;
    int32_t *d_ch, *d_conv;
    RsConv* d_convs;
    float* d_taps;
    std::vector<char> tab;
    Call call(c);
    TRY(call.opened);
    TRY(upload_parts(c, S_RS_TAB, tab, [&](Layout L) {
        return L.part(d_ioff, n1, h_in_off).part(d_ooff, n1, (const int64_t*)h_out_off).part(d_tiles, n1, (const int64_t*)tiles.data())
            .part(d_ch, (size_t)n_files, h_channels).part(d_conv, (size_t)n_files, h_conv)
            .part(d_convs, (size_t)n_conv, (const RsConv*)convs.data()).part(d_taps, (size_t)n_taps, h_taps).bytes();
    }));
    {
        Timer t(c, SPKD_T_RESAMPLE);
        hipLaunchKernelGGL(k_resample, dim3((unsigned)tiles[(size_t)n_files]), dim3(RS_TPB), lds, c->stream, d_in,
                           (const long long*)d_ioff, (const long long*)d_ooff, (const long long*)d_tiles, (long long)n_files,
                           (const int*)d_ch, (const int*)d_conv, (const RsConv*)d_convs, (const float*)d_taps, d_out);
    }
    if (hipGetLastError() != hipSuccess) return fail(c, SPKD_EHIP, "resample_batch: kernel launch failed");
    return call.finish();
}

// ------------------------------------------------------------------ (6b2) delay-and-sum beamforming
static_assert(BF_N == SPKD_BF_NFFT && BF_NBEST == SPKD_BF_NBEST && BF_MAX_HOP == SPKD_BF_MAX_HOP && BF_MAX_CH == SPKD_RESAMPLE_MAX_CH &&
              sizeof(BfGeom) == sizeof(spkd_bf_geom), "the header states the beamformer's transform length and limits");

namespace {
// The files and geometries of a beamforming call, checked (the resampler's conventions), and what the
// three stages derive from them: per file the steps T, and the running sums of T (step_off), T C (wg_off:
// workgroups of k_bf_gcc, entries of d_delay, a quarter of the candidates) and C (lane_off).
struct BfBatch {
    std::vector<int64_t> steps, wg, lanes;
    int64_t samples = 0;
};
spkd_status bf_check_files(spkd_ctx* c, const char* what, int64_t n_files, const int64_t* h_in_off, const int32_t* h_channels) {
    const std::string w(what);
    if (n_files < 0) return fail(c, SPKD_EINVAL, w + ": negative file count");
    if (!h_in_off || (n_files > 0 && !h_channels)) return fail(c, SPKD_EINVAL, w + ": null host array");
    if (h_in_off[0] != 0) return fail(c, SPKD_EINVAL, w + ": in_off must start at 0");
    for (int64_t f = 0; f < n_files; ++f)
        if (h_in_off[f + 1] < h_in_off[f]) return fail(c, SPKD_EINVAL, w + ": in_off must be non-decreasing");
    for (int64_t f = 0; f < n_files; ++f) {
        if (h_channels[f] < 1 || h_channels[f] > BF_MAX_CH) return fail(c, SPKD_EINVAL, w + ": channel count outside [1, 8]");
        if ((h_in_off[f + 1] - h_in_off[f]) % h_channels[f] != 0)
            return fail(c, SPKD_EINVAL, w + ": a file's span is not a multiple of its channel count");
    }
    return SPKD_OK;
}
spkd_status bf_batch(spkd_ctx* c, const char* what, int64_t n_files, const int64_t* h_in_off, const int32_t* h_channels,
                     const int32_t* h_geom, int32_t n_geom, const spkd_bf_geom* h_geoms, BfBatch& B) {
    const std::string w(what);
    if (n_geom < 0) return fail(c, SPKD_EINVAL, w + ": negative geometry count");
    TRY(bf_check_files(c, what, n_files, h_in_off, h_channels));
    if ((n_files > 0 && !h_geom) || (n_geom > 0 && !h_geoms)) return fail(c, SPKD_EINVAL, w + ": null host array");
    for (int64_t f = 0; f < n_files; ++f)
        if (h_geom[f] < 0 || h_geom[f] >= n_geom) return fail(c, SPKD_EINVAL, w + ": geometry index out of range");
    for (int32_t k = 0; k < n_geom; ++k) {
        const spkd_bf_geom& g = h_geoms[k];
        if (g.hop < 1 || g.hop > BF_MAX_HOP) return fail(c, SPKD_EINVAL, w + ": hop outside [1, 2^20]");
        if (g.window < 1) return fail(c, SPKD_EINVAL, w + ": window below 1");
        if (g.max_lag < 0) return fail(c, SPKD_EINVAL, w + ": negative max_lag");
        if ((int64_t)g.window + g.max_lag > BF_N) return fail(c, SPKD_EINVAL, w + ": window + max_lag exceeds the transform length 8192");
    }
    const size_t n1 = (size_t)n_files + 1;
    B.steps.assign(n1, 0);
    B.wg.assign(n1, 0);
    B.lanes.assign(n1, 0);
    for (int64_t f = 0; f < n_files; ++f) {
        const spkd_bf_geom& g = h_geoms[h_geom[f]];
        const int C = h_channels[f];
        const int64_t T = bf_steps((h_in_off[f + 1] - h_in_off[f]) / C, C, g.hop, g.window);
        B.steps[(size_t)f + 1] = B.steps[(size_t)f] + T;
        B.wg[(size_t)f + 1] = B.wg[(size_t)f] + T * C;
        B.lanes[(size_t)f + 1] = B.lanes[(size_t)f] + C;
    }
    B.samples = h_in_off[n_files];
    return SPKD_OK;
}
}  // namespace

spkd_status spkd_bf_gcc(spkd_ctx* c, const int16_t* d_in, int64_t n_files, const int64_t* h_in_off, const int32_t* h_channels,
                        const int32_t* h_geom, int32_t n_geom, const spkd_bf_geom* h_geoms, const int32_t* h_ref,
                        int32_t* d_ref, int32_t* d_lag, float* d_val, float* d_curve, int64_t* h_step_off, int64_t* h_curve_off) {
    if (!c) return SPKD_EINVAL;
    BfBatch B;
    TRY(bf_batch(c, "bf_gcc", n_files, h_in_off, h_channels, h_geom, n_geom, h_geoms, B));
    if (!h_step_off || (n_files > 0 && !h_ref) || (d_curve && !h_curve_off)) return fail(c, SPKD_EINVAL, "bf_gcc: null host array");
    for (int64_t f = 0; f < n_files; ++f)
        if (h_ref[f] < -1 || h_ref[f] >= h_channels[f])
            return fail(c, SPKD_EINVAL, "bf_gcc: reference channel outside [-1, channels)");
    const size_t n1 = (size_t)n_files + 1;
    std::vector<int64_t> en_tiles(n1, 0), curve_off(n1, 0);
    for (int64_t f = 0; f < n_files; ++f) {
        const int64_t n = (h_in_off[f + 1] - h_in_off[f]) / h_channels[f];
        en_tiles[(size_t)f + 1] = en_tiles[(size_t)f] + (n + BF_EN_TILE - 1) / BF_EN_TILE;
        curve_off[(size_t)f + 1] = curve_off[(size_t)f] +
            (B.wg[(size_t)f + 1] - B.wg[(size_t)f]) * (2 * (int64_t)h_geoms[h_geom[f]].max_lag + 1);
    }
    std::copy(B.steps.begin(), B.steps.end(), h_step_off);
    if (h_curve_off) std::copy(curve_off.begin(), curve_off.end(), h_curve_off);
    if (B.samples == 0) return SPKD_OK;
    if (!d_in || !d_ref || !d_lag || !d_val) return fail(c, SPKD_EINVAL, "bf_gcc: null device buffer");
    if (B.wg[(size_t)n_files] > 0x7fffffffLL || en_tiles[(size_t)n_files] > 0x7fffffffLL)
        return fail(c, SPKD_EINVAL, "bf_gcc: too many steps in one call");
    if (!c->bf_lds_ok) return fail(c, SPKD_EHIP, "bf_gcc: the kernel's dynamic LDS size was not admitted on this device");
    int64_t *d_ioff, *d_wg, *d_tiles, *d_coff;
    int32_t *d_ch, *d_geom, *d_want;
    BfGeom* d_geoms;
    std::vector<char> tab;
    Call call(c);
    TRY(call.opened);
    TRY(upload_parts(c, S_BF_TAB, tab, [&](Layout L) {
        return L.part(d_ioff, n1, h_in_off).part(d_wg, n1, (const int64_t*)B.wg.data()).part(d_tiles, n1, (const int64_t*)en_tiles.data())
            .part(d_coff, n1, (const int64_t*)curve_off.data()).part(d_ch, (size_t)n_files, h_channels).part(d_geom, (size_t)n_files, h_geom)
            .part(d_want, (size_t)n_files, h_ref).part(d_geoms, (size_t)n_geom, (const BfGeom*)h_geoms).bytes();
    }));
    void *d_tw = nullptr, *d_energy = nullptr;
    TRY(scratch(c, S_BF_TW, (size_t)(BF_N / 2) * sizeof(float2), &d_tw));
    TRY(scratch(c, S_BF_ENERGY, (size_t)n_files * BF_MAX_CH * sizeof(unsigned long long), &d_energy));
    HIPCHK(c, hipMemsetAsync(d_energy, 0, (size_t)n_files * BF_MAX_CH * sizeof(unsigned long long), c->stream));
    {
        Timer t(c, SPKD_T_BF_GCC);
        if (!c->bf_tw_ready) hipLaunchKernelGGL(k_bf_twiddle, dim3(BF_N / 2 / 256), dim3(256), 0, c->stream, (float2*)d_tw);
        c->bf_tw_ready = true;
        if (en_tiles[(size_t)n_files] > 0)
            hipLaunchKernelGGL(k_bf_energy, dim3((unsigned)en_tiles[(size_t)n_files]), dim3(BF_EN_TPB), 0, c->stream, d_in,
                               (const long long*)d_ioff, (const long long*)d_tiles, (long long)n_files, (const int*)d_ch,
                               (unsigned long long*)d_energy);
        hipLaunchKernelGGL(k_bf_ref, dim3((unsigned)((n_files + 255) / 256)), dim3(256), 0, c->stream,
                           (const unsigned long long*)d_energy, (const int*)d_ch, (const int*)d_want, (long long)n_files, d_ref);
        if (B.wg[(size_t)n_files] > 0)
            hipLaunchKernelGGL(k_bf_gcc, dim3((unsigned)B.wg[(size_t)n_files]), dim3(BF_TPB), BF_LDS_BYTES, c->stream, d_in,
                               (const long long*)d_ioff, (const long long*)d_wg, (long long)n_files, (const int*)d_ch,
                               (const int*)d_geom, (const BfGeom*)d_geoms, (const int*)d_ref, (const float2*)d_tw, d_lag, d_val,
                               d_curve, (const long long*)d_coff);
    }
    if (hipGetLastError() != hipSuccess) return fail(c, SPKD_EHIP, "bf_gcc: kernel launch failed");
    return call.finish();
}

spkd_status spkd_bf_track(spkd_ctx* c, int64_t n_files, const int64_t* h_step_off, const int32_t* h_channels,
                          const int32_t* d_lag, const float* d_val, int32_t n_best, float min_peak, double jump_penalty,
                          int32_t jump_cap, int32_t* d_delay) {
    if (!c) return SPKD_EINVAL;
    if (n_files < 0) return fail(c, SPKD_EINVAL, "bf_track: negative file count");
    if (!h_step_off || (n_files > 0 && !h_channels)) return fail(c, SPKD_EINVAL, "bf_track: null host array");
    if (h_step_off[0] != 0) return fail(c, SPKD_EINVAL, "bf_track: step_off must start at 0");
    for (int64_t f = 0; f < n_files; ++f) {
        if (h_step_off[f + 1] < h_step_off[f]) return fail(c, SPKD_EINVAL, "bf_track: step_off must be non-decreasing");
        if (h_channels[f] < 1 || h_channels[f] > BF_MAX_CH) return fail(c, SPKD_EINVAL, "bf_track: channel count outside [1, 8]");
    }
    if (n_best < 1 || n_best > BF_NBEST) return fail(c, SPKD_EINVAL, "bf_track: n_best outside [1, 4]");
    if (!(min_peak == min_peak)) return fail(c, SPKD_EINVAL, "bf_track: min_peak is not a number");
    if (!(jump_penalty >= 0.0) || std::isinf(jump_penalty)) return fail(c, SPKD_EINVAL, "bf_track: jump_penalty must be finite and not negative");
    if (jump_cap < 0) return fail(c, SPKD_EINVAL, "bf_track: negative jump_cap");
    const size_t n1 = (size_t)n_files + 1;
    std::vector<int64_t> wg(n1, 0), lanes(n1, 0);
    for (int64_t f = 0; f < n_files; ++f) {
        wg[(size_t)f + 1] = wg[(size_t)f] + (h_step_off[f + 1] - h_step_off[f]) * h_channels[f];
        lanes[(size_t)f + 1] = lanes[(size_t)f] + h_channels[f];
    }
    if (wg[(size_t)n_files] == 0) return SPKD_OK;
    if (!d_lag || !d_val || !d_delay) return fail(c, SPKD_EINVAL, "bf_track: null device buffer");
    if (wg[(size_t)n_files] > 0x7fffffffLL) return fail(c, SPKD_EINVAL, "bf_track: too many steps in one call");
    int64_t *d_wg, *d_lanes;
    int32_t* d_ch;
    std::vector<char> tab;
    Call call(c);
    TRY(call.opened);
    TRY(upload_parts(c, S_BF_TAB, tab, [&](Layout L) {
        return L.part(d_wg, n1, (const int64_t*)wg.data()).part(d_lanes, n1, (const int64_t*)lanes.data())
            .part(d_ch, (size_t)n_files, h_channels).bytes();
    }));
    void* d_back = nullptr;
    TRY(scratch(c, S_BF_BACK, (size_t)wg[(size_t)n_files], &d_back));
    {
        Timer t(c, SPKD_T_BF_TRACK);
        hipLaunchKernelGGL(k_bf_track, dim3((unsigned)((lanes[(size_t)n_files] + 63) / 64)), dim3(64), 0, c->stream,
                           (const long long*)d_wg, (const long long*)d_lanes, (long long)n_files, (const int*)d_ch, d_lag, d_val,
                           (int)n_best, min_peak, jump_penalty, (int)jump_cap, (unsigned char*)d_back, d_delay);
    }
    if (hipGetLastError() != hipSuccess) return fail(c, SPKD_EHIP, "bf_track: kernel launch failed");
    return call.finish();
}

spkd_status spkd_bf_sum(spkd_ctx* c, const int16_t* d_in, int64_t n_files, const int64_t* h_in_off, const int32_t* h_channels,
                        const int32_t* h_geom, int32_t n_geom, const spkd_bf_geom* h_geoms, const int32_t* d_delay,
                        int16_t* d_out, int64_t* h_out_off) {
    if (!c) return SPKD_EINVAL;
    BfBatch B;
    TRY(bf_batch(c, "bf_sum", n_files, h_in_off, h_channels, h_geom, n_geom, h_geoms, B));
    if (!h_out_off) return fail(c, SPKD_EINVAL, "bf_sum: null host array");
    const size_t n1 = (size_t)n_files + 1;
    std::vector<int64_t> tiles(n1, 0);
    h_out_off[0] = 0;
    for (int64_t f = 0; f < n_files; ++f) {
        const int64_t n = (h_in_off[f + 1] - h_in_off[f]) / h_channels[f];
        h_out_off[f + 1] = h_out_off[f] + n;
        tiles[(size_t)f + 1] = tiles[(size_t)f] + (n + BF_SUM_TILE - 1) / BF_SUM_TILE;
    }
    if (B.samples == 0) return SPKD_OK;
    if (!d_in || !d_out || (B.wg[(size_t)n_files] > 0 && !d_delay)) return fail(c, SPKD_EINVAL, "bf_sum: null device buffer");
    if (tiles[(size_t)n_files] > 0x7fffffffLL) return fail(c, SPKD_EINVAL, "bf_sum: too many samples in one call");
    int64_t *d_ioff, *d_ooff, *d_tiles, *d_wg;
    int32_t *d_ch, *d_geom;
    BfGeom* d_geoms;
    std::vector<char> tab;
    Call call(c);
    TRY(call.opened);
    TRY(upload_parts(c, S_BF_TAB, tab, [&](Layout L) {
        return L.part(d_ioff, n1, h_in_off).part(d_ooff, n1, (const int64_t*)h_out_off).part(d_tiles, n1, (const int64_t*)tiles.data())
            .part(d_wg, n1, (const int64_t*)B.wg.data()).part(d_ch, (size_t)n_files, h_channels).part(d_geom, (size_t)n_files, h_geom)
            .part(d_geoms, (size_t)n_geom, (const BfGeom*)h_geoms).bytes();
    }));
    {
        Timer t(c, SPKD_T_BF_SUM);
        hipLaunchKernelGGL(k_bf_sum, dim3((unsigned)tiles[(size_t)n_files]), dim3(BF_SUM_TPB), 0, c->stream, d_in,
                           (const long long*)d_ioff, (const long long*)d_ooff, (const long long*)d_tiles, (const long long*)d_wg,
                           (long long)n_files, (const int*)d_ch, (const int*)d_geom, (const BfGeom*)d_geoms, d_delay, d_out);
    }
    if (hipGetLastError() != hipSuccess) return fail(c, SPKD_EHIP, "bf_sum: kernel launch failed");
    return call.finish();
}

// ------------------------------------------------------------------ (6b3) the delay stream
static_assert(TD_NONE == SPKD_TDOA_NONE && TD_MAX_CH == SPKD_TDOA_MAX_CH && TD_MAX_DELAY == SPKD_TDOA_MAX_DELAY &&
              TD_FILE == SPKD_TDOA_FILE && TD_MODEL == SPKD_TDOA_MODEL && TD_TPB == SPKD_TDOA_TILE,
              "the header states the stream's layouts and the kernels' tile");

namespace {
// the clock and the per-file table of the three calls that read the stream (`name` opens the messages)
spkd_status tdoa_files(spkd_ctx* c, const std::string& name, const int64_t* h_files, int64_t n_files, int64_t n_entries,
                       int32_t hop, int32_t window, int32_t rate_out, TdoaClock* K) {
    if (n_files < 0 || n_files > 0x7fffffff || n_entries < 0) return fail(c, SPKD_EINVAL, name + ": bad count");
    if (n_files > 0 && !h_files) return fail(c, SPKD_EINVAL, name + ": null file table");
    if (hop < 1 || window < 0 || rate_out < 1) return fail(c, SPKD_EINVAL, name + ": hop >= 1, window >= 0 and rate_out >= 1 required");
    *K = TdoaClock{hop, window, rate_out};
    for (int64_t f = 0; f < n_files; ++f) {
        const int64_t* F = h_files + f * TD_FILE;
        const int64_t off = F[TDF_OFF], T = F[TDF_T], C = F[TDF_C], ref = F[TDF_REF], H = F[TDF_H], rate = F[TDF_RATE];
        if (C < 1 || C > TD_MAX_CH) return fail(c, SPKD_EINVAL, name + ": 1 to 8 channels a file");
        if (off < 0 || off > n_entries || T < 0 || T > (n_entries - off) / C)
            return fail(c, SPKD_EINVAL, name + ": a file's entries lie outside the stream");
        if (C > 1 && (ref < 0 || ref >= C)) return fail(c, SPKD_EINVAL, name + ": reference channel out of range");
        if (H < 1 || H > SPKD_BF_MAX_HOP || rate < 1 || rate > 0x7fffffff)
            return fail(c, SPKD_EINVAL, name + ": step or input rate out of range");
        if (F[TDF_FRAME0] < 0) return fail(c, SPKD_EINVAL, name + ": negative first frame");
        if (C > 1 && H * rate_out < (int64_t)hop * rate) return fail(c, SPKD_EINVAL, name + ": a step shorter than a frame");
        if (T > tdoa_step_limit(*K, H)) return fail(c, SPKD_EINVAL, name + ": too many steps for 64-bit sample positions");
    }
    return SPKD_OK;
}

// a frame range [b, e) of the batch in file f: inside the rule's 64-bit bound
spkd_status tdoa_range(spkd_ctx* c, const std::string& name, const int64_t* h_files, int64_t n_files, const TdoaClock& K,
                       int64_t f, int64_t b, int64_t e) {
    if (f < 0 || f >= n_files) return fail(c, SPKD_EINVAL, name + ": file index out of range");
    const int64_t* F = h_files + f * TD_FILE;
    if (b < F[TDF_FRAME0] || e < b) return fail(c, SPKD_EINVAL, name + ": bad frame range");
    if (e - F[TDF_FRAME0] > tdoa_frame_limit(K, F[TDF_RATE]))
        return fail(c, SPKD_EINVAL, name + ": frame beyond 64-bit sample positions");
    return SPKD_OK;
}
}  // namespace

spkd_status spkd_tdoa_pack(spkd_ctx* c, const int32_t* d_delay, const float* d_val, float min_peak, int64_t n, int32_t* d_out) {
    if (!c || n < 0) return SPKD_EINVAL;
    if (min_peak != min_peak) return fail(c, SPKD_EINVAL, "tdoa_pack: min_peak is not a number");
    if (n == 0) return SPKD_OK;
    if (!d_delay || !d_val || !d_out) return fail(c, SPKD_EINVAL, "tdoa_pack: null device buffer");
    if ((uintptr_t)d_delay % 4 || (uintptr_t)d_val % 4 || (uintptr_t)d_out % 4) return fail(c, SPKD_EINVAL, "tdoa_pack: misaligned buffer");
    const int64_t blocks = (n + TD_TPB - 1) / TD_TPB;
    if (blocks > 0x7fffffff) return fail(c, SPKD_EINVAL, "tdoa_pack: too many entries in one call");
    Call call(c);
    TRY(call.opened);
    {
        Timer tm(c, SPKD_T_TDOA_PACK);
        hipLaunchKernelGGL(k_tdoa_pack, dim3((unsigned)blocks), dim3(TD_TPB), 0, c->stream, d_delay, d_val, min_peak, (long long)n, d_out);
    }
    HIPCHK(c, hipGetLastError());
    return call.finish();
}

spkd_status spkd_tdoa_stats(spkd_ctx* c, const int32_t* d_stream, int64_t n_entries, const int64_t* h_files, int64_t n_files,
                            int32_t hop, int32_t window, int32_t rate_out, const int64_t* h_begin, const int64_t* h_end,
                            const int32_t* h_file, const int32_t* h_set, int64_t n_ranges, int64_t n_sets, int64_t* d_stats) {
    if (!c || n_ranges < 0 || n_sets < 0) return SPKD_EINVAL;
    TdoaClock K;
    TRY(tdoa_files(c, "tdoa_stats", h_files, n_files, n_entries, hop, window, rate_out, &K));
    if (n_sets > 0x7fffffff) return fail(c, SPKD_EINVAL, "tdoa_stats: too many sets");
    if (n_ranges > 0 && (!h_begin || !h_end || !h_file || !h_set)) return fail(c, SPKD_EINVAL, "tdoa_stats: null range arrays");
    if (n_sets == 0 && n_ranges == 0) return SPKD_OK;
    if (!d_stats || (uintptr_t)d_stats % 8) return fail(c, SPKD_EINVAL, "tdoa_stats: null or misaligned statistics");
    int64_t n_items = 0, frames = 0;
    for (int64_t r = 0; r < n_ranges; ++r) {
        if (h_set[r] < 0 || h_set[r] >= n_sets || (r > 0 && h_set[r] < h_set[r - 1]))
            return fail(c, SPKD_EINVAL, "tdoa_stats: set indices ascending and inside [0, n_sets)");
        TRY(tdoa_range(c, "tdoa_stats", h_files, n_files, K, h_file[r], h_begin[r], h_end[r]));
        if (r > 0 && h_set[r] != h_set[r - 1]) frames = 0;
        frames += h_end[r] - h_begin[r];
        if (frames > 0x7fffffffLL) return fail(c, SPKD_EINVAL, "tdoa_stats: a set of 2^31 frames or more");
        const int64_t* F = h_files + (int64_t)h_file[r] * TD_FILE;
        if (h_end[r] == h_begin[r] || F[TDF_C] < 2 || F[TDF_T] < 1) continue;
        const int64_t s0 = tdoa_step(h_begin[r] - F[TDF_FRAME0], K, F[TDF_H], F[TDF_RATE], F[TDF_T]);
        const int64_t s1 = tdoa_step(h_end[r] - 1 - F[TDF_FRAME0], K, F[TDF_H], F[TDF_RATE], F[TDF_T]);
        n_items += (s1 - s0) / TD_TPB + 1;
    }
    if (n_items > 0x7fffffff) return fail(c, SPKD_EINVAL, "tdoa_stats: too many steps in one call");
    if (n_items > 0 && (!d_stream || (uintptr_t)d_stream % 4)) return fail(c, SPKD_EINVAL, "tdoa_stats: null or misaligned stream");
    const size_t ni = (size_t)n_items, nf = (size_t)n_files;
    struct Tab { long long* files; TdoaItem* item; };
    auto t = mirror<Tab>([&](Layout L, Tab& p) { return L.part(p.files, nf * TD_FILE).part(p.item, ni).bytes(); });
    if (ni) {
        TRY(stage(c, PIN_TD_TAB, t));
        std::memcpy(t.h.files, h_files, nf * TD_FILE * sizeof(int64_t));
        TdoaItem* it = t.h.item;
        for (int64_t r = 0; r < n_ranges; ++r) {
            const int64_t* F = h_files + (int64_t)h_file[r] * TD_FILE;
            if (h_end[r] == h_begin[r] || F[TDF_C] < 2 || F[TDF_T] < 1) continue;
            const int64_t b = h_begin[r] - F[TDF_FRAME0], e = h_end[r] - F[TDF_FRAME0];
            const int64_t s0 = tdoa_step(b, K, F[TDF_H], F[TDF_RATE], F[TDF_T]);
            const int64_t s1 = tdoa_step(e - 1, K, F[TDF_H], F[TDF_RATE], F[TDF_T]);
            for (int64_t s = s0; s <= s1; s += TD_TPB, ++it) {
                it->b = b, it->e = e;
                it->file = h_file[r], it->set = h_set[r];
                it->step0 = (int)s;
                it->n_steps = (int)std::min<int64_t>(TD_TPB, s1 - s + 1);
            }
        }
    }
    Call call(c);
    TRY(call.opened);
    HIPCHK(c, hipMemsetAsync(d_stats, 0, (size_t)n_sets * TD_MAX_CH * TD_MOM * sizeof(int64_t), c->stream));
    if (ni) {
        TRY(send(call, S_TD_TAB, t));
        Timer tm(c, SPKD_T_TDOA_STATS);
        hipLaunchKernelGGL(k_tdoa_stats, dim3((unsigned)ni), dim3(TD_TPB), 0, c->stream, d_stream, (const long long*)t.d.files, K,
                           (const TdoaItem*)t.d.item, (unsigned long long*)d_stats);
    }
    HIPCHK(c, hipGetLastError());
    return call.finish();
}

spkd_status spkd_tdoa_models(spkd_ctx* c, const int64_t* d_stats, int64_t n_speakers, const int32_t* h_spk_file,
                             const int32_t* h_ok, const int64_t* h_files, int64_t n_files, int32_t min_frames, double floor_s,
                             double* d_models, int32_t* h_live) {
    if (!c || n_speakers < 0 || n_files < 0) return SPKD_EINVAL;
    if (n_speakers > 0x7fffffff || n_files > 0x7fffffff) return fail(c, SPKD_EINVAL, "tdoa_models: bad count");
    if (min_frames < 1) return fail(c, SPKD_EINVAL, "tdoa_models: min_frames >= 1");
    if (!(floor_s > 0.0) || !(floor_s < INFINITY)) return fail(c, SPKD_EINVAL, "tdoa_models: floor_s a finite number > 0");
    if (n_files == 0 && n_speakers == 0) return SPKD_OK;
    if (!h_files || !h_live || (n_speakers > 0 && (!h_spk_file || !h_ok || !d_stats || !d_models)))
        return fail(c, SPKD_EINVAL, "tdoa_models: null argument");
    if ((uintptr_t)d_stats % 8 || (uintptr_t)d_models % 8) return fail(c, SPKD_EINVAL, "tdoa_models: misaligned buffer");
    for (int64_t f = 0; f < n_files; ++f) {
        const int64_t* F = h_files + f * TD_FILE;
        if (F[TDF_C] < 1 || F[TDF_C] > TD_MAX_CH || (F[TDF_C] > 1 && (F[TDF_REF] < 0 || F[TDF_REF] >= F[TDF_C])) ||
            F[TDF_RATE] < 1 || F[TDF_RATE] > 0x7fffffff)
            return fail(c, SPKD_EINVAL, "tdoa_models: channels, reference channel or input rate of a file out of range");
    }
    for (int64_t s = 0; s < n_speakers; ++s)
        if (h_spk_file[s] < 0 || h_spk_file[s] >= n_files || (s > 0 && h_spk_file[s] < h_spk_file[s - 1]))
            return fail(c, SPKD_EINVAL, "tdoa_models: the speakers' files ascending and inside [0, n_files)");
    if (n_files == 0) return SPKD_OK;
    const size_t nf = (size_t)n_files, ns = (size_t)n_speakers;
    struct Tab { long long *files, *spk_off; int *ok, *live; };
    auto t = mirror<Tab>([&](Layout L, Tab& p) {
        return L.part(p.files, nf * TD_FILE).part(p.spk_off, nf + 1).part(p.ok, ns).part(p.live, nf).bytes();
    });
    TRY(stage(c, PIN_TD_TAB, t));
    std::memcpy(t.h.files, h_files, nf * TD_FILE * sizeof(int64_t));
    if (ns) std::memcpy(t.h.ok, h_ok, ns * sizeof(int32_t));
    std::memset(t.h.live, 0, nf * sizeof(int32_t));
    {
        size_t s = 0;
        for (size_t f = 0; f < nf; ++f) {
            t.h.spk_off[f] = (long long)s;
            while (s < ns && (size_t)h_spk_file[s] == f) ++s;
        }
        t.h.spk_off[nf] = (long long)ns;
    }
    Call call(c);
    TRY(call.opened);
    TRY(send(call, S_TD_TAB, t));
    {
        Timer tm(c, SPKD_T_TDOA_MODELS);
        hipLaunchKernelGGL(k_tdoa_models, dim3((unsigned)nf), dim3(WAVE), 0, c->stream, (const long long*)d_stats,
                           (const long long*)t.d.files, (const long long*)t.d.spk_off, (const int*)t.d.ok, (int)min_frames, floor_s,
                           d_models, t.d.live);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_live, t.d.live, nf * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    return call.finish();
}

spkd_status spkd_tdoa_score(spkd_ctx* c, const int32_t* d_stream, int64_t n_entries, const int64_t* h_files, int64_t n_files,
                            int32_t hop, int32_t window, int32_t rate_out, const double* d_models, int64_t n_models,
                            const int32_t* h_live, int64_t n_seq, const int64_t* h_seq_begin, const int64_t* h_seq_end,
                            const int32_t* h_seq_file, const int32_t* h_seq_model, const int32_t* h_seq_n_models, int32_t n_cols,
                            double weight, float* d_scores) {
    if (!c || n_seq < 0) return SPKD_EINVAL;
    TdoaClock K;
    TRY(tdoa_files(c, "tdoa_score", h_files, n_files, n_entries, hop, window, rate_out, &K));
    if (n_cols < 1 || n_cols > GS_MAX_COLS) return fail(c, SPKD_EINVAL, "tdoa_score: 1 <= n_cols <= 16");
    if (!(weight >= 0.0) || !(weight < INFINITY)) return fail(c, SPKD_EINVAL, "tdoa_score: weight a finite number >= 0");
    if (n_models < 0 || n_models > 0x7fffffff || n_seq > 0x7fffffff) return fail(c, SPKD_EINVAL, "tdoa_score: bad count");
    if (n_seq == 0) return SPKD_OK;
    if (!h_live || !h_seq_begin || !h_seq_end || !h_seq_file || !h_seq_model || !h_seq_n_models)
        return fail(c, SPKD_EINVAL, "tdoa_score: null argument");
    for (int64_t f = 0; f < n_files; ++f) {
        const int64_t* F = h_files + f * TD_FILE;
        const int32_t valid = F[TDF_C] > 1 ? (((1 << F[TDF_C]) - 1) & ~(1 << F[TDF_REF])) : 0;
        if (h_live[f] & ~valid) return fail(c, SPKD_EINVAL, "tdoa_score: a live channel the file does not have");
    }
    int64_t n_tiles = 0;
    for (int64_t q = 0; q < n_seq; ++q) {
        const int64_t b = h_seq_begin[q], e = h_seq_end[q], m = h_seq_model[q], k = h_seq_n_models[q];
        TRY(tdoa_range(c, "tdoa_score", h_files, n_files, K, h_seq_file[q], b, e));
        if (k < 0 || k > n_cols) return fail(c, SPKD_EINVAL, "tdoa_score: 0 <= models of a sequence <= n_cols");
        if (m < 0 || m + k > n_models) return fail(c, SPKD_EINVAL, "tdoa_score: model index out of range");
        const int64_t* F = h_files + (int64_t)h_seq_file[q] * TD_FILE;
        if (k > 0 && F[TDF_T] > 0 && h_live[h_seq_file[q]]) n_tiles += (e - b + TD_TPB - 1) / TD_TPB;
    }
    if (n_tiles == 0) return SPKD_OK;
    if (n_tiles > 0x7fffffff) return fail(c, SPKD_EINVAL, "tdoa_score: too many frames in one call");
    if (!d_stream || !d_models || !d_scores) return fail(c, SPKD_EINVAL, "tdoa_score: null device buffer");
    if ((uintptr_t)d_stream % 4 || (uintptr_t)d_models % 8 || (uintptr_t)d_scores % 4)
        return fail(c, SPKD_EINVAL, "tdoa_score: misaligned buffer");
    const size_t ns = (size_t)n_seq, nf = (size_t)n_files, nt = (size_t)n_tiles;
    struct Tab { long long *begin, *end, *row, *tile, *files; int *file, *model, *n_models, *tile_seq, *live; };
    auto t = mirror<Tab>([&](Layout L, Tab& p) {
        return L.part(p.begin, ns).part(p.end, ns).part(p.row, ns).part(p.tile, ns).part(p.files, nf * TD_FILE).part(p.file, ns)
            .part(p.model, ns).part(p.n_models, ns).part(p.tile_seq, nt).part(p.live, nf).bytes();
    });
    TRY(stage(c, PIN_TD_TAB, t));
    std::memcpy(t.h.begin, h_seq_begin, ns * sizeof(int64_t));
    std::memcpy(t.h.end, h_seq_end, ns * sizeof(int64_t));
    std::memcpy(t.h.files, h_files, nf * TD_FILE * sizeof(int64_t));
    std::memcpy(t.h.file, h_seq_file, ns * sizeof(int32_t));
    std::memcpy(t.h.model, h_seq_model, ns * sizeof(int32_t));
    std::memcpy(t.h.n_models, h_seq_n_models, ns * sizeof(int32_t));
    std::memcpy(t.h.live, h_live, nf * sizeof(int32_t));
    long long row = 0, tile = 0;
    for (size_t q = 0; q < ns; ++q) {
        t.h.row[q] = row;
        t.h.tile[q] = tile;
        const long long len = t.h.end[q] - t.h.begin[q];
        const int64_t* F = h_files + (int64_t)h_seq_file[q] * TD_FILE;
        const long long k = (h_seq_n_models[q] > 0 && F[TDF_T] > 0 && h_live[h_seq_file[q]]) ? (len + TD_TPB - 1) / TD_TPB : 0;
        for (long long i = 0; i < k; ++i) t.h.tile_seq[tile + i] = (int)q;
        row += len;
        tile += k;
    }
    Call call(c);
    TRY(call.opened);
    TRY(send(call, S_TD_TAB, t));
    {
        Timer tm(c, SPKD_T_TDOA_SCORE);
        const TdoaSeqs S{t.d.begin, t.d.end, t.d.row, t.d.tile, t.d.file, t.d.model, t.d.n_models, t.d.tile_seq, t.d.live};
        hipLaunchKernelGGL(k_tdoa_score, dim3((unsigned)nt), dim3(TD_TPB), 0, c->stream, d_stream, (const long long*)t.d.files, K,
                           d_models, S, (int)n_cols, weight, d_scores, c->d_err);
    }
    HIPCHK(c, hipGetLastError());
    return call.finish();
}

// ------------------------------------------------------------------ (6b4) seats from the delay stream
static_assert(SEAT_MAX_N == SPKD_SEAT_MAX_N, "the header states the chain's limit");

namespace {
// the four settings of the statistic (`name` opens the messages)
spkd_status seat_settings(spkd_ctx* c, const std::string& name, int32_t min_frames, double floor_s, double lambdac, double threshold) {
    if (min_frames < 1) return fail(c, SPKD_EINVAL, name + ": min_frames >= 1");
    if (!(floor_s > 0.0) || !(floor_s < INFINITY)) return fail(c, SPKD_EINVAL, name + ": floor_s a finite number > 0");
    if (!std::isfinite(lambdac)) return fail(c, SPKD_EINVAL, name + ": lambdac a finite number");
    if (std::isnan(threshold)) return fail(c, SPKD_EINVAL, name + ": threshold is NaN");
    return SPKD_OK;
}
}  // namespace

spkd_status spkd_tdoa_cuts(spkd_ctx* c, const int32_t* d_stream, int64_t n_entries, const int64_t* h_files, int64_t n_files,
                           int32_t hop, int32_t window, int32_t rate_out, const int64_t* h_begin, const int64_t* h_end,
                           const int32_t* h_file, int64_t n_ranges, int64_t min_piece, int32_t min_frames, double floor_s,
                           double lambdac, double threshold, int64_t* h_cut, double* h_delta) {
    if (!c || n_ranges < 0) return SPKD_EINVAL;
    TdoaClock K;
    TRY(tdoa_files(c, "tdoa_cuts", h_files, n_files, n_entries, hop, window, rate_out, &K));
    if (min_piece < 1) return fail(c, SPKD_EINVAL, "tdoa_cuts: min_piece >= 1");
    TRY(seat_settings(c, "tdoa_cuts", min_frames, floor_s, lambdac, threshold));
    if (n_ranges > 0x7fffffff) return fail(c, SPKD_EINVAL, "tdoa_cuts: too many ranges in one call");
    if (n_ranges == 0) return SPKD_OK;
    if (!h_begin || !h_end || !h_file || !h_cut || !h_delta) return fail(c, SPKD_EINVAL, "tdoa_cuts: null range arrays");
    bool steps = false;
    for (int64_t r = 0; r < n_ranges; ++r) {
        TRY(tdoa_range(c, "tdoa_cuts", h_files, n_files, K, h_file[r], h_begin[r], h_end[r]));
        if (h_end[r] - h_begin[r] > 0x7fffffffLL) return fail(c, SPKD_EINVAL, "tdoa_cuts: a range of 2^31 frames or more");
        const int64_t* F = h_files + (int64_t)h_file[r] * TD_FILE;
        steps = steps || (h_end[r] > h_begin[r] && F[TDF_C] > 1 && F[TDF_T] > 0);
    }
    if (steps && (!d_stream || (uintptr_t)d_stream % 4)) return fail(c, SPKD_EINVAL, "tdoa_cuts: null or misaligned stream");
    const size_t nr = (size_t)n_ranges, nf = (size_t)n_files;
    struct Tab { long long *files, *begin, *end; int* file; };
    auto t = mirror<Tab>([&](Layout L, Tab& p) { return L.part(p.files, nf * TD_FILE).part(p.begin, nr).part(p.end, nr).part(p.file, nr).bytes(); });
    struct Out { long long* cut; double* delta; };
    auto out = mirror<Out>([&](Layout L, Out& o) { return L.part(o.cut, nr).part(o.delta, nr).bytes(); });
    TRY(stage(c, PIN_TD_TAB, t));
    TRY(stage(c, PIN_SEAT_OUT, out));
    std::memcpy(t.h.files, h_files, nf * TD_FILE * sizeof(int64_t));
    std::memcpy(t.h.begin, h_begin, nr * sizeof(int64_t));
    std::memcpy(t.h.end, h_end, nr * sizeof(int64_t));
    std::memcpy(t.h.file, h_file, nr * sizeof(int32_t));
    Call call(c);
    TRY(call.opened);
    TRY(send(call, S_TD_TAB, t));
    TRY(carve(c, scratch, S_SEAT_OUT, [&](Layout L) { return place(L, out).bytes(); }));
    {
        Timer tm(c, SPKD_T_TDOA_CUTS);
        hipLaunchKernelGGL(k_tdoa_cuts, dim3((unsigned)nr), dim3(SEAT_TPB), 0, c->stream, d_stream, (const long long*)t.d.files, K,
                           (const long long*)t.d.begin, (const long long*)t.d.end, (const int*)t.d.file, (long long)min_piece,
                           (int)min_frames, floor_s, lambdac, threshold, out.d.cut, out.d.delta);
    }
    HIPCHK(c, hipGetLastError());
    TRY(copy(call, out, hipMemcpyDeviceToHost));
    TRY(call.finish());
    std::memcpy(h_cut, out.h.cut, nr * sizeof(int64_t));
    std::memcpy(h_delta, out.h.delta, nr * sizeof(double));
    return SPKD_OK;
}

spkd_status spkd_tdoa_split(spkd_ctx* c, const int64_t* d_stats, int64_t n_problems, const int64_t* h_off,
                            const int32_t* h_prob_file, const int64_t* h_files, int64_t n_files, int32_t hop, int32_t window,
                            int32_t rate_out, int32_t min_frames, double floor_s, double lambdac, double threshold,
                            int32_t* h_merge_a, int32_t* h_merge_b, double* h_merge_d, int32_t* h_n_merges, int32_t* h_placed) {
    if (!c || n_problems < 0) return SPKD_EINVAL;
    TdoaClock K;
    TRY(tdoa_files(c, "tdoa_split", h_files, n_files, INT64_MAX, hop, window, rate_out, &K));
    TRY(seat_settings(c, "tdoa_split", min_frames, floor_s, lambdac, threshold));
    if (n_problems > 0x7fffffff) return fail(c, SPKD_EINVAL, "tdoa_split: too many problems in one call");
    if (n_problems == 0) return SPKD_OK;
    if (!h_off || !h_prob_file || !h_n_merges) return fail(c, SPKD_EINVAL, "tdoa_split: null problem arrays");
    if (h_off[0] != 0) return fail(c, SPKD_EINVAL, "tdoa_split: the offsets must start at 0");
    size_t cells = 0;
    for (int64_t p = 0; p < n_problems; ++p) {
        const int64_t n = h_off[p + 1] - h_off[p];
        if (n < 0) return fail(c, SPKD_EINVAL, "tdoa_split: the offsets must be non-decreasing");
        if (n > SEAT_MAX_N) return fail(c, SPKD_EINVAL, "tdoa_split: at most 4096 records a problem");
        if (h_prob_file[p] < 0 || h_prob_file[p] >= n_files) return fail(c, SPKD_EINVAL, "tdoa_split: file index out of range");
        cells += n > 1 ? (size_t)n * (size_t)n : 0;
    }
    const int64_t n_rec = h_off[n_problems];
    if (n_rec > 0x7fffffff) return fail(c, SPKD_EINVAL, "tdoa_split: too many records in one call");
    const size_t np = (size_t)n_problems, ns = (size_t)n_rec, nf = (size_t)n_files;
    if (ns == 0) {
        std::memset(h_n_merges, 0, np * sizeof(int32_t));
        return SPKD_OK;
    }
    if (!h_merge_a || !h_merge_b || !h_merge_d || !h_placed) return fail(c, SPKD_EINVAL, "tdoa_split: null result arrays");
    if (!d_stats || (uintptr_t)d_stats % 8) return fail(c, SPKD_EINVAL, "tdoa_split: null or misaligned statistics");
    struct Tab { long long *files, *off, *mat_off; int* file; };
    auto t = mirror<Tab>([&](Layout L, Tab& p) { return L.part(p.files, nf * TD_FILE).part(p.off, np + 1).part(p.mat_off, np).part(p.file, np).bytes(); });
    struct Out { double* d; int32_t *a, *b, *nm, *placed; };
    auto out = mirror<Out>([&](Layout L, Out& o) { return L.part(o.d, ns).part(o.a, ns).part(o.b, ns).part(o.nm, np).part(o.placed, ns).bytes(); });
    TRY(stage(c, PIN_TD_TAB, t));
    TRY(stage(c, PIN_SEAT_OUT, out));
    std::memcpy(t.h.files, h_files, nf * TD_FILE * sizeof(int64_t));
    std::memcpy(t.h.off, h_off, (np + 1) * sizeof(int64_t));
    std::memcpy(t.h.file, h_prob_file, np * sizeof(int32_t));
    {
        long long at = 0;
        for (size_t p = 0; p < np; ++p) {
            const long long n = h_off[p + 1] - h_off[p];
            t.h.mat_off[p] = at;
            at += n > 1 ? n * n : 0;
        }
    }
    Call call(c);
    TRY(call.opened);
    TRY(send(call, S_TD_TAB, t));
    long long* d_w = nullptr;
    void* d_mat = nullptr;
    TRY(carve(c, scratch, S_SEAT_WORK, [&](Layout L) { return place(L, out).part(d_w, ns * SEAT_REC).bytes(); }));
    TRY(scratch(c, S_SEAT_MAT, cells * sizeof(double), &d_mat));
    {
        Timer tm(c, SPKD_T_TDOA_SPLIT);
        hipLaunchKernelGGL(k_tdoa_split, dim3((unsigned)np), dim3(SEAT_CHAIN_TPB), 0, c->stream, (const long long*)d_stats,
                           (const long long*)t.d.files, K, (const long long*)t.d.off, (const int*)t.d.file,
                           (const long long*)t.d.mat_off, (int)min_frames, floor_s, lambdac, threshold, d_w, (double*)d_mat,
                           (int*)out.d.a, (int*)out.d.b, out.d.d, (int*)out.d.nm, (int*)out.d.placed);
    }
    HIPCHK(c, hipGetLastError());
    TRY(copy(call, out, hipMemcpyDeviceToHost));
    TRY(call.finish());
    std::memcpy(h_n_merges, out.h.nm, np * sizeof(int32_t));
    std::memcpy(h_placed, out.h.placed, ns * sizeof(int32_t));
    for (size_t p = 0; p < np; ++p) {                                    // (what lies behind a problem's log is not defined)
        const size_t o = (size_t)h_off[p], k = (size_t)out.h.nm[p];
        std::memcpy(h_merge_a + o, out.h.a + o, k * sizeof(int32_t));
        std::memcpy(h_merge_b + o, out.h.b + o, k * sizeof(int32_t));
        std::memcpy(h_merge_d + o, out.h.d + o, k * sizeof(double));
    }
    return SPKD_OK;
}

// ------------------------------------------------------------------ (6b5) overlapped speech from the delay stream
static_assert(OVL_MAX_SPK == SPKD_OVERLAP_MAX_SPK && OVL_MAX_RUN == SPKD_OVERLAP_MAX_RUN && OVL_TPB == SPKD_TDOA_TILE,
              "the header states the overlap kernels' limits and tile");

spkd_status spkd_tdoa_second(spkd_ctx* c, const int32_t* d_delay, const int32_t* d_lag, const float* d_val, int32_t n_best,
                             float min_peak, float min_second, int32_t guard, int64_t n, int32_t* d_out) {
    if (!c || n < 0) return SPKD_EINVAL;
    if (n_best < 1 || n_best > BF_NBEST) return fail(c, SPKD_EINVAL, "tdoa_second: n_best outside [1, 4]");
    if (guard < 0) return fail(c, SPKD_EINVAL, "tdoa_second: guard >= 0");
    if (min_peak != min_peak) return fail(c, SPKD_EINVAL, "tdoa_second: min_peak is not a number");
    if (min_second != min_second) return fail(c, SPKD_EINVAL, "tdoa_second: min_second is not a number");
    if (n == 0) return SPKD_OK;
    if (!d_delay || !d_lag || !d_val || !d_out) return fail(c, SPKD_EINVAL, "tdoa_second: null device buffer");
    if ((uintptr_t)d_delay % 4 || (uintptr_t)d_lag % 4 || (uintptr_t)d_val % 4 || (uintptr_t)d_out % 4)
        return fail(c, SPKD_EINVAL, "tdoa_second: misaligned buffer");
    const int64_t blocks = (n + TD_TPB - 1) / TD_TPB;
    if (blocks > 0x7fffffff) return fail(c, SPKD_EINVAL, "tdoa_second: too many entries in one call");
    Call call(c);
    TRY(call.opened);
    {
        Timer tm(c, SPKD_T_TDOA_SECOND);
        hipLaunchKernelGGL(k_tdoa_second, dim3((unsigned)blocks), dim3(TD_TPB), 0, c->stream, d_delay, d_lag, d_val, (int)n_best,
                           min_peak, min_second, (int)guard, (long long)n, d_out);
    }
    HIPCHK(c, hipGetLastError());
    return call.finish();
}

spkd_status spkd_tdoa_overlap(spkd_ctx* c, const int32_t* d_stream, int64_t n_entries, const int64_t* h_files, int64_t n_files,
                              int32_t hop, int32_t window, int32_t rate_out, const int32_t* d_second, const double* d_models,
                              const int32_t* h_live, const int64_t* h_spk_off, double gate, int32_t min_channels,
                              int32_t min_steps, int32_t* d_pair) {
    if (!c) return SPKD_EINVAL;
    TdoaClock K;
    TRY(tdoa_files(c, "tdoa_overlap", h_files, n_files, n_entries, hop, window, rate_out, &K));
    if (!(gate > 0.0) || !(gate < INFINITY)) return fail(c, SPKD_EINVAL, "tdoa_overlap: gate a finite number > 0");
    if (min_channels < 1) return fail(c, SPKD_EINVAL, "tdoa_overlap: min_channels >= 1");
    if (min_steps < 1 || min_steps > OVL_MAX_RUN) return fail(c, SPKD_EINVAL, "tdoa_overlap: min_steps outside [1, 64]");
    if (n_files == 0) return SPKD_OK;
    if (!h_live || !h_spk_off) return fail(c, SPKD_EINVAL, "tdoa_overlap: null arrays");
    if (h_spk_off[0] != 0) return fail(c, SPKD_EINVAL, "tdoa_overlap: the speaker offsets must start at 0");
    int64_t total = 0, n_tiles = 0;
    for (int64_t f = 0; f < n_files; ++f) {
        const int64_t* F = h_files + f * TD_FILE;
        const int64_t k = h_spk_off[f + 1] - h_spk_off[f];
        if (k < 0) return fail(c, SPKD_EINVAL, "tdoa_overlap: the speaker offsets must be non-decreasing");
        if (k > OVL_MAX_SPK) return fail(c, SPKD_EINVAL, "tdoa_overlap: at most 16 speakers a file");
        const int32_t valid = F[TDF_C] > 1 ? (((1 << F[TDF_C]) - 1) & ~(1 << F[TDF_REF])) : 0;
        if (h_live[f] & ~valid) return fail(c, SPKD_EINVAL, "tdoa_overlap: a live channel the file does not have");
        if (F[TDF_T] > 0x7fffffff) return fail(c, SPKD_EINVAL, "tdoa_overlap: too many steps in a file");
        total += F[TDF_T];
        n_tiles += (F[TDF_T] + OVL_TPB - 1) / OVL_TPB;
    }
    if (total == 0) return SPKD_OK;
    if (n_tiles > 0x7fffffff || h_spk_off[n_files] > 0x7fffffff) return fail(c, SPKD_EINVAL, "tdoa_overlap: too many steps or speakers in one call");
    if (!d_stream || !d_second || !d_pair || (h_spk_off[n_files] > 0 && !d_models)) return fail(c, SPKD_EINVAL, "tdoa_overlap: null device buffer");
    if ((uintptr_t)d_stream % 4 || (uintptr_t)d_second % 4 || (uintptr_t)d_pair % 4 || (uintptr_t)d_models % 8)
        return fail(c, SPKD_EINVAL, "tdoa_overlap: misaligned buffer");
    const size_t nf = (size_t)n_files, nt = (size_t)n_tiles;
    struct Tab { long long *files, *spk_off, *step_off; int* live; OvlTile* tile; };
    auto t = mirror<Tab>([&](Layout L, Tab& p) {
        return L.part(p.files, nf * TD_FILE).part(p.spk_off, nf + 1).part(p.step_off, nf).part(p.live, nf).part(p.tile, nt).bytes();
    });
    TRY(stage(c, PIN_TD_TAB, t));
    std::memcpy(t.h.files, h_files, nf * TD_FILE * sizeof(int64_t));
    std::memcpy(t.h.spk_off, h_spk_off, (nf + 1) * sizeof(int64_t));
    std::memcpy(t.h.live, h_live, nf * sizeof(int32_t));
    {
        long long at = 0;
        OvlTile* tl = t.h.tile;
        for (size_t f = 0; f < nf; ++f) {
            const int64_t T = h_files[f * TD_FILE + TDF_T];
            t.h.step_off[f] = at;
            for (int64_t s = 0; s < T; s += OVL_TPB, ++tl) tl->file = (int)f, tl->step0 = (int)s;
            at += T;
        }
    }
    Call call(c);
    TRY(call.opened);
    TRY(send(call, S_TD_TAB, t));
    void* d_raw = nullptr;
    TRY(scratch(c, S_OVL_RAW, (size_t)total * sizeof(int32_t), &d_raw));
    {
        Timer tm(c, SPKD_T_TDOA_OVERLAP);
        const OvlFiles S{t.d.files, t.d.spk_off, t.d.step_off, t.d.live};
        hipLaunchKernelGGL(k_ovl_match, dim3((unsigned)nt), dim3(OVL_TPB), 0, c->stream, d_stream, d_second, S,
                           (const OvlTile*)t.d.tile, d_models, gate, (int)min_channels, (int32_t*)d_raw);
        hipLaunchKernelGGL(k_ovl_runs, dim3((unsigned)nt), dim3(OVL_TPB), 0, c->stream, (const int32_t*)d_raw, S,
                           (const OvlTile*)t.d.tile, (int)min_steps, d_pair);
    }
    HIPCHK(c, hipGetLastError());
    return call.finish();
}

// ------------------------------------------------------------------ (6c) frame energies and their seeds
static_assert(EN_TILE == SPKD_ENERGY_TILE && EN_MAX_WINDOW == SPKD_ENERGY_MAX_WINDOW,
              "the header states the energy kernel's tile and limit");

namespace {
// the offsets of a batch: n + 1 entries from 0 on that never decrease
spkd_status energy_check_offsets(spkd_ctx* c, int64_t n_files, const int64_t* off, const char* what) {
    if (n_files < 0 || !off) return fail(c, SPKD_EINVAL, std::string(what) + ": null offsets or a negative file count");
    if (off[0] != 0) return fail(c, SPKD_EINVAL, std::string(what) + ": the offsets must start at 0");
    for (int64_t f = 0; f < n_files; ++f)
        if (off[f + 1] < off[f]) return fail(c, SPKD_EINVAL, std::string(what) + ": the offsets must be non-decreasing");
    return SPKD_OK;
}
}  // namespace

spkd_status spkd_frame_energy_batch(spkd_ctx* c, const int16_t* d_pcm, const int64_t* h_sample_off, int64_t n_files,
                                    int32_t hop, int32_t window, int64_t* d_energy, int64_t* h_frame_off) {
    if (hop < 1 || window < hop || window > EN_MAX_WINDOW)
        return fail(c, SPKD_EINVAL, "frame_energy_batch: 1 <= hop <= window <= 4096");
    TRY(energy_check_offsets(c, n_files, h_sample_off, "frame_energy_batch"));
    if (!h_frame_off) return fail(c, SPKD_EINVAL, "frame_energy_batch: null frame_off");
    if (!c) return SPKD_EINVAL;
    // the frame layout (spkd_mfcc_batch's), and the running count of tiles: a tile lies in one file
    const size_t n1 = (size_t)n_files + 1;
    const int64_t per_tile = en_tile_frames(hop);
    std::vector<int64_t> tiles(n1, 0);
    h_frame_off[0] = 0;
    for (int64_t f = 0; f < n_files; ++f) {
        const int64_t T = (h_sample_off[f + 1] - h_sample_off[f]) / hop;
        h_frame_off[f + 1] = h_frame_off[f] + T;
        tiles[(size_t)f + 1] = tiles[(size_t)f] + (T + per_tile - 1) / per_tile;
    }
    if (h_frame_off[n_files] == 0) return SPKD_OK;
    if (!d_pcm || !d_energy) return fail(c, SPKD_EINVAL, "frame_energy_batch: null device buffer");
    if ((uintptr_t)d_pcm % 2 || (uintptr_t)d_energy % 8)
        return fail(c, SPKD_EINVAL, "frame_energy_batch: samples 2-byte and energies 8-byte aligned");
    if (tiles[(size_t)n_files] > 0x7fffffffLL) return fail(c, SPKD_EINVAL, "frame_energy_batch: too many samples in one call");
    int64_t *d_soff, *d_foff, *d_tiles;
    std::vector<char> tab;
    Call call(c);
    TRY(call.opened);
    TRY(upload_parts(c, S_EN_TAB, tab, [&](Layout L) {
        return L.part(d_soff, n1, h_sample_off).part(d_foff, n1, (const int64_t*)h_frame_off)
            .part(d_tiles, n1, (const int64_t*)tiles.data()).bytes();
    }));
    {
        Timer t(c, SPKD_T_FRAME_ENERGY);
        hipLaunchKernelGGL(k_frame_energy, dim3((unsigned)tiles[(size_t)n_files]), dim3(EN_TPB), 0, c->stream, d_pcm,
                           (const long long*)d_soff, (const long long*)d_foff, (const long long*)d_tiles, (long long)n_files,
                           (int)hop, (int)window, (long long*)d_energy);
    }
    if (hipGetLastError() != hipSuccess) return fail(c, SPKD_EHIP, "frame_energy_batch: kernel launch failed");
    return call.finish();
}

spkd_status spkd_energy_seeds(spkd_ctx* c, const int64_t* d_energy, const int64_t* h_frame_off, int64_t n_files,
                              const int64_t* h_k_low, const int64_t* h_k_high, int64_t* h_lo, int64_t* h_hi,
                              int32_t* h_seeded, const int64_t** h_run_off, const int64_t** h_run_begin,
                              const int64_t** h_run_end) {
    if (!h_run_off || !h_run_begin || !h_run_end) return fail(c, SPKD_EINVAL, "energy_seeds: null output");
    *h_run_off = nullptr;
    *h_run_begin = nullptr;
    *h_run_end = nullptr;
    TRY(energy_check_offsets(c, n_files, h_frame_off, "energy_seeds"));
    if (n_files > 0 && (!h_k_low || !h_k_high || !h_lo || !h_hi || !h_seeded))
        return fail(c, SPKD_EINVAL, "energy_seeds: null argument");
    if (n_files > 0x3fffffff) return fail(c, SPKD_EINVAL, "energy_seeds: too many files in one call");
    for (int64_t f = 0; f < n_files; ++f)
        if (h_frame_off[f + 1] - h_frame_off[f] > 0x7fffffffLL)
            return fail(c, SPKD_EINVAL, "energy_seeds: a file of more than 2^31 - 1 frames");
    if (h_frame_off[n_files] > 0 && !d_energy) return fail(c, SPKD_EINVAL, "energy_seeds: null device buffer");
    if ((uintptr_t)d_energy % 8) return fail(c, SPKD_EINVAL, "energy_seeds: energies 8-byte aligned");
    if (!c) return SPKD_EINVAL;
    const size_t nf = (size_t)n_files;
    // pinned, the context's until its next spkd_energy_seeds: the offsets of the runs and, in front of
    // them, what the selection left per file
    int64_t* run_off = nullptr;
    EsFile* h_files = nullptr;
    TRY(carve(c, pinned, PIN_ES_FILES, [&](Layout L) { return L.part(run_off, 2 * nf + 1).part(h_files, nf).bytes(); }));
    run_off[0] = 0;
    *h_run_off = run_off;
    if (n_files == 0) return SPKD_OK;
    int64_t *d_foff, *d_klow, *d_khigh, *d_run_off, *d_begin = nullptr, *d_end = nullptr, *h_begin = nullptr, *h_end = nullptr;
    EsFile* d_files = nullptr;
    std::vector<char> tab;
    Call call(c);
    TRY(call.opened);
    TRY(upload_parts(c, S_ES_TAB, tab, [&](Layout L) {
        return L.part(d_foff, nf + 1, h_frame_off).part(d_klow, nf, h_k_low).part(d_khigh, nf, h_k_high).bytes();
    }));
    TRY(carve(c, scratch, S_ES_FILES, [&](Layout L) { return L.part(d_run_off, 2 * nf + 1).part(d_files, nf).bytes(); }));
    {
        // both kernels and, between them, the wait for the counts that place the runs (as a decoder's backtrack)
        Timer t(c, SPKD_T_ENERGY_SEEDS);
        hipLaunchKernelGGL(k_energy_select, dim3((unsigned)n_files), dim3(ES_TPB), 0, c->stream, (const long long*)d_energy,
                           (const long long*)d_foff, (const long long*)d_klow, (const long long*)d_khigh, d_files);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(h_files, d_files, nf * sizeof(EsFile), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (size_t f = 0; f < nf; ++f) {
            run_off[2 * f + 1] = run_off[2 * f] + h_files[f].n_runs[0];
            run_off[2 * f + 2] = run_off[2 * f + 1] + h_files[f].n_runs[1];
        }
        const size_t n_runs = (size_t)run_off[2 * nf];
        TRY(carve(c, scratch, S_ES_RUNS, [&](Layout L) { return L.part(d_begin, n_runs).part(d_end, n_runs).bytes(); }));
        TRY(carve(c, pinned, PIN_ES_RUNS, [&](Layout L) { return L.part(h_begin, n_runs).part(h_end, n_runs).bytes(); }));
        if (n_runs) {
            HIPCHK(c, hipMemcpyAsync(d_run_off, run_off, (2 * nf + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(k_energy_runs, dim3((unsigned)n_files), dim3(ES_TPB), 0, c->stream, (const long long*)d_energy,
                               (const long long*)d_foff, (const EsFile*)d_files, (const long long*)d_run_off,
                               (long long*)d_begin, (long long*)d_end);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(h_begin, d_begin, n_runs * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(h_end, d_end, n_runs * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        }
    }
    for (size_t f = 0; f < nf; ++f) {
        h_lo[f] = h_files[f].lo;
        h_hi[f] = h_files[f].hi;
        h_seeded[f] = h_files[f].seeded;
    }
    *h_run_begin = h_begin;
    *h_run_end = h_end;
    return call.finish();
}

// ------------------------------------------------------------------ (7) speech / non-speech scoring
spkd_status spkd_gmm_loglik(spkd_ctx* c, const float* d_features, int64_t n_frames, const spkd_gmm_params* P,
                            float* d_scores) {
    if (!c || !P) return SPKD_EINVAL;
    const int K = P->n_kernels, S = P->n_states;
    if (P->dim != GM_DIM || K < 1 || K > GM_MAX_K || S < 1 || S > GM_MAX_S || n_frames < 0)
        return fail(c, SPKD_EINVAL, "gmm_loglik: dim must be 39, 1 <= kernels <= 256, 1 <= states <= 16");
    if (!P->mean || !P->inv_var || !P->log_norm || !P->state_off || !P->kernel || !P->log_weight)
        return fail(c, SPKD_EINVAL, "gmm_loglik: null model array");
    if (P->state_off[0] != 0) return fail(c, SPKD_EINVAL, "gmm_loglik: state_off[0] must be 0");
    for (int s = 0; s < S; ++s)
        if (P->state_off[s + 1] < P->state_off[s] || P->state_off[s + 1] - P->state_off[s] > K)
            return fail(c, SPKD_EINVAL, "gmm_loglik: state_off must be non-decreasing, at most 256 kernels a state");
    const int nnz = P->state_off[S];
    for (int j = 0; j < nnz; ++j) {
        const float lw = P->log_weight[j];
        if (P->kernel[j] < 0 || P->kernel[j] >= K || std::isnan(lw) || lw == INFINITY)
            return fail(c, SPKD_EINVAL, "gmm_loglik: kernel index out of range or log weight NaN / +inf");
    }
    for (int64_t i = 0; i < (int64_t)K * GM_DIM; ++i)
        if (!std::isfinite(P->mean[i]) || !std::isfinite(P->inv_var[i]) || !(P->inv_var[i] > 0.f))
            return fail(c, SPKD_EINVAL, "gmm_loglik: means must be finite, inverse variances finite and positive");
    for (int k = 0; k < K; ++k)
        if (!std::isfinite(P->log_norm[k])) return fail(c, SPKD_EINVAL, "gmm_loglik: non-finite normalising constant");
    if (n_frames == 0) return SPKD_OK;
    if (!d_features || !d_scores) return fail(c, SPKD_EINVAL, "gmm_loglik: null device buffer");
    const int64_t n_blocks = (n_frames + GM_TPB - 1) / GM_TPB;
    if (n_blocks > 0x7fffffffLL) return fail(c, SPKD_EINVAL, "gmm_loglik: too many frames in one call");
    float *d_mean, *d_iv, *d_c, *d_lw;
    int32_t *d_state_off, *d_kernel;
    std::vector<char> tab, idx;
    Call call(c);
    TRY(call.opened);
    TRY(upload_parts(c, S_GMM_TAB, tab, [&](Layout L) {
        return L.part(d_mean, (size_t)K * GM_DIM, P->mean).part(d_iv, (size_t)K * GM_DIM, P->inv_var)
            .part(d_c, (size_t)K, P->log_norm).part(d_lw, (size_t)nnz, P->log_weight).bytes();
    }));
    TRY(upload_parts(c, S_GMM_IDX, idx, [&](Layout L) {
        return L.part(d_state_off, (size_t)S + 1, P->state_off).part(d_kernel, (size_t)nnz, P->kernel).bytes();
    }));
    hipLaunchKernelGGL(k_gmm_loglik, dim3((unsigned)n_blocks), dim3(GM_TPB), 0, c->stream, d_features,
                       (long long)n_frames, d_mean, d_iv, d_c, (const int*)d_state_off, (const int*)d_kernel, d_lw,
                       S, d_scores);
    if (hipGetLastError() != hipSuccess) return fail(c, SPKD_EHIP, "gmm_loglik: kernel launch failed");
    return call.finish();
}

// ------------------------------------------------------------------ (7b) the decision part for a batch
namespace {
static_assert(VB_TILE == SPKD_VAD_TILE, "the header states the kernels' tile");
static_assert(LG_MAX == GM_MAX_S, "one limit for states and words, and for the lanes of a group");

spkd_status vad_check_offsets(spkd_ctx* c, int64_t n_files, const int64_t* h_frame_off) {
    if (n_files < 0 || !h_frame_off) return fail(c, SPKD_EINVAL, "vad batch: null frame_off or a negative file count");
    if (h_frame_off[0] != 0) return fail(c, SPKD_EINVAL, "vad batch: frame_off must start at 0");
    for (int64_t f = 0; f < n_files; ++f)
        if (h_frame_off[f + 1] < h_frame_off[f]) return fail(c, SPKD_EINVAL, "vad batch: frame_off must be non-decreasing");
    if (h_frame_off[n_files] > (int64_t)0x7fffffff * VB_SHIFT_TPB)
        return fail(c, SPKD_EINVAL, "vad batch: too many frames in one call");
    return SPKD_OK;
}
}  // namespace

spkd_status spkd_vad_shift_batch(spkd_ctx* c, const float* d_scores, int64_t n_files, const int64_t* h_frame_off,
                                 int32_t n_states, double shift, float* d_out) {
    if (!c) return SPKD_EINVAL;
    if (n_states < 2 || n_states > GM_MAX_S)
        return fail(c, SPKD_EINVAL, "vad_shift_batch: 2 <= states <= 16 (the shift scales row 1)");
    TRY(vad_check_offsets(c, n_files, h_frame_off));
    const int64_t total = h_frame_off[n_files];
    if (total == 0) return SPKD_OK;
    if (!d_scores || !d_out) return fail(c, SPKD_EINVAL, "vad_shift_batch: null device buffer");
    std::vector<char> tab;
    Call call(c);
    TRY(call.opened);
    int64_t* d_off = nullptr;
    TRY(upload_parts(c, S_VAD_TAB, tab, [&](Layout L) { return L.part(d_off, (size_t)n_files + 1, h_frame_off).bytes(); }));
    {
        Timer t(c, SPKD_T_VAD_SHIFT);
        hipLaunchKernelGGL(k_vad_shift, dim3((unsigned)((total + VB_SHIFT_TPB - 1) / VB_SHIFT_TPB)), dim3(VB_SHIFT_TPB), 0,
                           c->stream, d_scores, (const long long*)d_off, (long long)n_files, (int)n_states, shift, d_out);
    }
    HIPCHK(c, hipGetLastError());
    return call.finish();
}

namespace {
struct VadTables {
    int64_t *frame_off, *back_off;
    int32_t* word_state;
    double *stay, *exit, *enter;
};
struct DecodedSeqs {             // what a decoder leaves per sequence, device or pinned host
    int64_t *tok_off, *count;
    double* score;
    int32_t* final_word;
};

extern "C++" {
// The lane-group frame of spkd_lanegroup.hpp, host side.  G: the power of two >= n_words (1 .. LG_MAX),
// the lanes that share a sequence; it sizes the records and the scratch as well as the launch.
int group_width(int n_words) {
    int G = 1;
    while (G < n_words) G *= 2;
    return G;
}
// f(std::integral_constant<int, G>()) for that G
template <class F>
void with_group(int n_words, F f) {
    switch (group_width(n_words)) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 4: return f(std::integral_constant<int, 4>());
    case 8: return f(std::integral_constant<int, 8>());
    case 16: return f(std::integral_constant<int, 16>());
    default: std::abort();       // (no caller passes n_words > LG_MAX: a launch sized for another G would write out of bounds)
    }
}
// one wave a workgroup, WAVE / G sequences a wave
dim3 group_grid(int64_t n_seq, int G) { return dim3((unsigned)((n_seq + WAVE / G - 1) / (WAVE / G))); }

// How a decoder (spkd_vad_viterbi_batch, spkd_mindur_viterbi_batch) hands its tokens back: per file the
// count, the score and the final word on the device and in pinned memory, the tokens compact behind
// them.  Each call has pinned and scratch slots of its own, so neither ends the other's results.
struct TokenHandBack {
    const int64_t **const tok_off, **const tok_frame;
    const int32_t** const tok_word;
    const double** const score;
    const int pin_files, pin_tokens, s_files, s_tokens;
    size_t nf = 0;
    DecodedSeqs h{}, d{};           // pinned: the results of the call; the device's

    size_t parts(Layout L, DecodedSeqs& f) const {
        return L.part(f.tok_off, nf + 1).part(f.count, nf).part(f.score, nf).part(f.final_word, nf).bytes();
    }
    // before any other check: false for a null output, else the four outputs nulled
    bool clear() const {
        if (!tok_off || !tok_frame || !tok_word || !score) return false;
        *tok_off = nullptr;
        *tok_frame = nullptr;
        *tok_word = nullptr;
        *score = nullptr;
        return true;
    }
    // after the argument checks, before the Call: what a call without files returns as well
    spkd_status open(spkd_ctx* c, int64_t n_files) {
        nf = (size_t)n_files;
        TRY(carve(c, pinned, pin_files, [&](Layout L) { return parts(L, h); }));
        h.tok_off[0] = 0;
        *tok_off = h.tok_off;
        *score = h.score;
        return SPKD_OK;
    }
    // inside the Call, before the decoder's kernel: where it leaves each file's final word and score
    spkd_status place(spkd_ctx* c) {
        return carve(c, scratch, s_files, [&](Layout L) { return parts(L, d); });
    }
    // Both passes of the backtrack as kernel timer `timer`: count(d) leaves every file's token count,
    // which the host needs to place the tokens (hence the wait inside the call); write(d, tok_frame,
    // tok_word) writes them from tok_off on.
    template <class Count, class Write>
    spkd_status hand_back(spkd_ctx* c, int timer, Count count, Write write) {
        int64_t *d_tok_frame = nullptr, *h_frames = nullptr;
        int32_t *d_tok_word = nullptr, *h_words = nullptr;
        {
            Timer tm(c, timer);
            count(d);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(h.count, d.count, nf * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(h.score, d.score, nf * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            for (size_t f = 0; f < nf; ++f) h.tok_off[f + 1] = h.tok_off[f] + h.count[f];
            const size_t n_tok = (size_t)h.tok_off[nf];
            TRY(carve(c, scratch, s_tokens, [&](Layout L) { return L.part(d_tok_frame, n_tok).part(d_tok_word, n_tok).bytes(); }));
            TRY(carve(c, pinned, pin_tokens, [&](Layout L) { return L.part(h_frames, n_tok).part(h_words, n_tok).bytes(); }));
            HIPCHK(c, hipMemcpyAsync(d.tok_off, h.tok_off, (nf + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
            write(d, d_tok_frame, d_tok_word);
            HIPCHK(c, hipGetLastError());
            if (n_tok) {
                HIPCHK(c, hipMemcpyAsync(h_frames, d_tok_frame, n_tok * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipMemcpyAsync(h_words, d_tok_word, n_tok * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            }
        }
        *tok_frame = h_frames;
        *tok_word = h_words;
        return SPKD_OK;
    }
};

// where each file's per-frame records start: every file from a multiple of the tile on
std::vector<int64_t> tiled_offsets(const int64_t* h_frame_off, size_t nf, int64_t tile) {
    std::vector<int64_t> off(nf + 1, 0);
    for (size_t f = 0; f < nf; ++f) off[f + 1] = off[f] + (h_frame_off[f + 1] - h_frame_off[f] + tile - 1) / tile * tile;
    return off;
}

template <int G>
void vad_decode_launch(spkd_ctx* c, const float* d_scores, const VadTables& t, int64_t n_files, int S, int W, void* back,
                       const DecodedSeqs& d) {
    typedef typename VbRecord<G>::type Rec;
    hipLaunchKernelGGL(k_vad_viterbi<G>, group_grid(n_files, G), dim3(WAVE), 0, c->stream, d_scores,
                       (const long long*)t.frame_off, (const long long*)t.back_off, (long long)n_files, S, W,
                       (const int*)t.word_state, (const double*)t.stay, (const double*)t.exit, (const double*)t.enter,
                       (Rec*)back, (int*)d.final_word, d.score);
}

template <class Rec, bool WRITE>
void vad_backtrack_launch(spkd_ctx* c, const void* back, const VadTables& t, int64_t n_files, int G, const DecodedSeqs& d,
                          int64_t* tok_frame, int32_t* tok_word) {
    hipLaunchKernelGGL((k_vad_backtrack<Rec, WRITE>), dim3((unsigned)((n_files + WAVE - 1) / WAVE)), dim3(WAVE), 0,
                       c->stream, (const Rec*)back, (const long long*)t.frame_off, (const long long*)t.back_off,
                       (long long)n_files, G, (const int*)d.final_word, (long long*)d.count, (const long long*)d.tok_off,
                       (long long*)tok_frame, (int*)tok_word);
}
}  // extern "C++"
}  // namespace

spkd_status spkd_vad_viterbi_batch(spkd_ctx* c, const float* d_scores, int64_t n_files, const int64_t* h_frame_off,
                                   int32_t n_states, int32_t n_words, const int32_t* h_word_state, const double* h_stay,
                                   const double* h_exit, const double* h_enter, const int64_t** h_tok_off,
                                   const int64_t** h_tok_frame, const int32_t** h_tok_word, const double** h_score) {
    if (!c) return SPKD_EINVAL;
    TokenHandBack r{h_tok_off, h_tok_frame, h_tok_word, h_score, PIN_VAD_FILES, PIN_VAD_TOKENS, S_VAD_FILES, S_VAD_TOKENS};
    if (!r.clear()) return fail(c, SPKD_EINVAL, "vad_viterbi_batch: null output");
    if (n_states < 1 || n_states > GM_MAX_S || n_words < 1 || n_words > GM_MAX_S)
        return fail(c, SPKD_EINVAL, "vad_viterbi_batch: 1 <= states, words <= 16");
    if (!h_word_state || !h_stay || !h_exit || !h_enter) return fail(c, SPKD_EINVAL, "vad_viterbi_batch: null argument");
    for (int32_t j = 0; j < n_words; ++j)
        if (h_word_state[j] < 0 || h_word_state[j] >= n_states)
            return fail(c, SPKD_EINVAL, "vad_viterbi_batch: word state out of range");
    TRY(vad_check_offsets(c, n_files, h_frame_off));
    if (h_frame_off[n_files] > 0 && !d_scores) return fail(c, SPKD_EINVAL, "vad_viterbi_batch: null device buffer");
    const size_t nf = (size_t)n_files, W = (size_t)n_words;
    const std::vector<int64_t> back_off = tiled_offsets(h_frame_off, nf, VB_TILE);
    const int G = group_width(n_words);
    const size_t rec_bytes = G == 16 ? sizeof(VbRecord<16>::type) : sizeof(VbRecord<1>::type);
    TRY(r.open(c, n_files));
    if (n_files == 0) return SPKD_OK;
    std::vector<char> tab;
    Call call(c);
    TRY(call.opened);
    VadTables t;
    TRY(upload_parts(c, S_VAD_TAB, tab, [&](Layout L) {
        return L.part(t.frame_off, nf + 1, h_frame_off).part(t.back_off, nf + 1, back_off.data())
            .part(t.stay, W, h_stay).part(t.exit, W, h_exit).part(t.enter, W, h_enter).part(t.word_state, W, h_word_state)
            .bytes();
    }));
    TRY(r.place(c));
    void* back = nullptr;
    TRY(scratch(c, S_VAD_BACK, (size_t)back_off[nf] * rec_bytes, &back));
    {
        Timer tm(c, SPKD_T_VAD_VITERBI);
        with_group(n_words, [&](auto g) {
            vad_decode_launch<decltype(g)::value>(c, d_scores, t, n_files, n_states, n_words, back, r.d);
        });
    }
    HIPCHK(c, hipGetLastError());
    TRY(r.hand_back(c, SPKD_T_VAD_BACKTRACK,
        [&](const DecodedSeqs& d) {
            if (G == 16) vad_backtrack_launch<VbRecord<16>::type, false>(c, back, t, n_files, G, d, nullptr, nullptr);
            else vad_backtrack_launch<VbRecord<1>::type, false>(c, back, t, n_files, G, d, nullptr, nullptr);
        },
        [&](const DecodedSeqs& d, int64_t* tok_frame, int32_t* tok_word) {
            if (G == 16) vad_backtrack_launch<VbRecord<16>::type, true>(c, back, t, n_files, G, d, tok_frame, tok_word);
            else vad_backtrack_launch<VbRecord<1>::type, true>(c, back, t, n_files, G, d, tok_frame, tok_word);
        }));
    return call.finish();
}

// ------------------------------------------------------------------ (8) the speaker loop with a minimum duration
static_assert(MD_TILE == SPKD_MINDUR_TILE, "the header states the kernels' tile");

namespace {
struct MdTables { int64_t *frame_off, *rec_off; };
struct MdWork {                  // per frame, each sequence from a multiple of MD_TILE on
    uint16_t* rec;
    double* g;
    int32_t* b;
};

extern "C++" {
template <int G>
void mindur_decode_launch(spkd_ctx* c, const float* d_scores, const MdTables& t, int64_t n_seq, int W, double penalty,
                          int64_t D, const MdWork& w, const DecodedSeqs& d) {
    const dim3 grid = group_grid(n_seq, G);
    if (D < MD_RING)
        hipLaunchKernelGGL((k_mindur_viterbi<G, true>), grid, dim3(WAVE), 0, c->stream, d_scores, (const long long*)t.frame_off,
                           (const long long*)t.rec_off, (long long)n_seq, W, W, penalty, (long long)D, w.rec, w.g, (int*)w.b,
                           (int*)d.final_word, d.score);
    else
        hipLaunchKernelGGL((k_mindur_viterbi<G, false>), grid, dim3(WAVE), 0, c->stream, d_scores, (const long long*)t.frame_off,
                           (const long long*)t.rec_off, (long long)n_seq, W, W, penalty, (long long)D, w.rec, w.g, (int*)w.b,
                           (int*)d.final_word, d.score);
}

template <bool WRITE>
void mindur_backtrack_launch(spkd_ctx* c, const MdTables& t, int64_t n_seq, int64_t D, const MdWork& w, const DecodedSeqs& d,
                             int64_t* tok_frame, int32_t* tok_word) {
    hipLaunchKernelGGL((k_mindur_backtrack<WRITE>), dim3((unsigned)((n_seq + WAVE - 1) / WAVE)), dim3(WAVE), 0, c->stream,
                       (const uint16_t*)w.rec, (const int*)w.b, (const long long*)t.frame_off, (const long long*)t.rec_off,
                       (long long)n_seq, (long long)D, (const int*)d.final_word, (long long*)d.count, (const long long*)d.tok_off,
                       (long long*)tok_frame, (int*)tok_word);
}
}  // extern "C++"
}  // namespace

spkd_status spkd_mindur_viterbi_batch(spkd_ctx* c, const float* d_scores, int64_t n_seq, const int64_t* h_frame_off,
                                      int32_t n_cols, double penalty, int32_t min_frames, const int64_t** h_tok_off,
                                      const int64_t** h_tok_frame, const int32_t** h_tok_word, const double** h_score) {
    if (!c) return SPKD_EINVAL;
    TokenHandBack r{h_tok_off, h_tok_frame, h_tok_word, h_score, PIN_MD_SEQS, PIN_MD_TOKENS, S_MD_SEQS, S_MD_TOKENS};
    if (!r.clear()) return fail(c, SPKD_EINVAL, "mindur_viterbi_batch: null output");
    if (n_cols < 1 || n_cols > GM_MAX_S) return fail(c, SPKD_EINVAL, "mindur_viterbi_batch: 1 <= n_cols <= 16");
    if (!std::isfinite(penalty) || penalty < 0.0) return fail(c, SPKD_EINVAL, "mindur_viterbi_batch: a finite penalty >= 0");
    if (min_frames < 1) return fail(c, SPKD_EINVAL, "mindur_viterbi_batch: min_frames >= 1");
    TRY(vad_check_offsets(c, n_seq, h_frame_off));
    if (h_frame_off[n_seq] > 0 && !d_scores) return fail(c, SPKD_EINVAL, "mindur_viterbi_batch: null device buffer");
    const size_t nf = (size_t)n_seq;
    const std::vector<int64_t> rec_off = tiled_offsets(h_frame_off, nf, MD_TILE);
    TRY(r.open(c, n_seq));
    if (n_seq == 0) return SPKD_OK;
    std::vector<char> tab;
    Call call(c);
    TRY(call.opened);
    MdTables t;
    TRY(upload_parts(c, S_MD_TAB, tab, [&](Layout L) {
        return L.part(t.frame_off, nf + 1, h_frame_off).part(t.rec_off, nf + 1, rec_off.data()).bytes();
    }));
    TRY(r.place(c));
    MdWork w;
    void* p = nullptr;
    const size_t n_rec = (size_t)rec_off[nf];
    TRY(scratch(c, S_MD_BACK, n_rec * sizeof(uint16_t), &p));
    w.rec = (uint16_t*)p;
    TRY(scratch(c, S_MD_G, n_rec * sizeof(double), &p));
    w.g = (double*)p;
    TRY(scratch(c, S_MD_B, n_rec * sizeof(int32_t), &p));
    w.b = (int32_t*)p;
    {
        Timer tm(c, SPKD_T_MINDUR_VITERBI);
        with_group(n_cols, [&](auto g) {
            mindur_decode_launch<decltype(g)::value>(c, d_scores, t, n_seq, n_cols, penalty, min_frames, w, r.d);
        });
    }
    HIPCHK(c, hipGetLastError());
    TRY(r.hand_back(c, SPKD_T_MINDUR_BACKTRACK,
        [&](const DecodedSeqs& d) { mindur_backtrack_launch<false>(c, t, n_seq, min_frames, w, d, nullptr, nullptr); },
        [&](const DecodedSeqs& d, int64_t* tok_frame, int32_t* tok_word) {
            mindur_backtrack_launch<true>(c, t, n_seq, min_frames, w, d, tok_frame, tok_word);
        }));
    return call.finish();
}

// ------------------------------------------------------------------ (8) the speaker loop's posteriors
static_assert(FB_TILE == SPKD_FB_TILE, "the header states the kernel's tile");

namespace {
// The index and token table of spkd_fb_posterior_batch, as the kernel takes it: per sequence its first
// frame, its first tile of stored forward vectors, its first token and its word count; per token its
// first frame and word.
struct FbTab { long long *frame_off, *tile_off, *tok_off, *tok_frame; int *seq_n, *tok_word; };

extern "C++" {
template <int G>
void fb_launch(spkd_ctx* c, const float* d_scores, const FbTab& t, bool tokens, int64_t n_seq, int S, double penalty,
               double scale, double* fwd, float* d_post, double* d_conf, double* d_logz) {
    hipLaunchKernelGGL(k_fb_posterior<G>, group_grid(n_seq, G), dim3(WAVE), 0, c->stream, d_scores,
                       (const long long*)t.frame_off, (const long long*)t.tile_off, (const int*)t.seq_n,
                       (long long)n_seq, S, penalty, scale, tokens ? (const long long*)t.tok_off : nullptr,
                       (const long long*)t.tok_frame, (const int*)t.tok_word, fwd, d_post, d_conf, d_logz);
}
}  // extern "C++"
}  // namespace

spkd_status spkd_fb_posterior_batch(spkd_ctx* c, const float* d_scores, int64_t n_seq, const int64_t* h_frame_off,
                                    int32_t n_cols, double penalty, double scale, const int32_t* h_seq_n_cols,
                                    const int64_t* h_tok_off, const int64_t* h_tok_frame, const int32_t* h_tok_word,
                                    float* d_post, double* h_conf, double* h_logz) {
    if (n_cols < 1 || n_cols > GM_MAX_S) return fail(c, SPKD_EINVAL, "fb_posterior_batch: 1 <= n_cols <= 16");
    if (!std::isfinite(penalty) || penalty < 0.0) return fail(c, SPKD_EINVAL, "fb_posterior_batch: a finite penalty >= 0");
    if (!std::isfinite(scale) || scale <= 0.0 || !(scale * penalty <= 600.0))
        return fail(c, SPKD_EINVAL, "fb_posterior_batch: a finite scale > 0 with scale * penalty <= 600");
    TRY(vad_check_offsets(c, n_seq, h_frame_off));
    const bool tokens = h_tok_off || h_tok_frame || h_tok_word;
    if (tokens && !(h_tok_off && h_tok_frame && h_tok_word))
        return fail(c, SPKD_EINVAL, "fb_posterior_batch: the token table takes all three arrays");
    if (n_seq > 0 && !h_logz) return fail(c, SPKD_EINVAL, "fb_posterior_batch: null output");
    for (int64_t q = 0; q < n_seq && h_seq_n_cols; ++q)
        if (h_seq_n_cols[q] < 1 || h_seq_n_cols[q] > n_cols)
            return fail(c, SPKD_EINVAL, "fb_posterior_batch: 1 <= columns of a sequence <= n_cols");
    int64_t n_tok = 0;
    if (tokens) {
        if (h_tok_off[0] != 0) return fail(c, SPKD_EINVAL, "fb_posterior_batch: tok_off must start at 0");
        for (int64_t q = 0; q < n_seq; ++q) {
            const int64_t lo = h_tok_off[q], hi = h_tok_off[q + 1], T = h_frame_off[q + 1] - h_frame_off[q];
            if (hi < lo) return fail(c, SPKD_EINVAL, "fb_posterior_batch: tok_off must be non-decreasing");
            if (T == 0 && hi > lo) return fail(c, SPKD_EINVAL, "fb_posterior_batch: tokens on a sequence without frames");
            if (T > 0 && (hi == lo || h_tok_frame[lo] != 0))
                return fail(c, SPKD_EINVAL, "fb_posterior_batch: a sequence's tokens start at frame 0");
            for (int64_t i = lo; i < hi; ++i) {
                if (i > lo && h_tok_frame[i] <= h_tok_frame[i - 1])
                    return fail(c, SPKD_EINVAL, "fb_posterior_batch: a sequence's tokens ascend strictly");
                if (h_tok_frame[i] >= T) return fail(c, SPKD_EINVAL, "fb_posterior_batch: a token at or behind the last frame");
                if (h_tok_word[i] < 0 || h_tok_word[i] >= n_cols)
                    return fail(c, SPKD_EINVAL, "fb_posterior_batch: word out of range");
            }
        }
        n_tok = h_tok_off[n_seq];
        if (n_tok > 0 && !h_conf) return fail(c, SPKD_EINVAL, "fb_posterior_batch: null output");
    }
    if (!c) return SPKD_EINVAL;
    if (n_seq == 0) return SPKD_OK;
    if (h_frame_off[n_seq] == 0) {
        for (int64_t q = 0; q < n_seq; ++q) h_logz[q] = -INFINITY;
        return SPKD_OK;
    }
    if (!d_scores) return fail(c, SPKD_EINVAL, "fb_posterior_batch: null device buffer");
    if (n_seq > 0x7fffffff) return fail(c, SPKD_EINVAL, "fb_posterior_batch: too many sequences in one call");
    const size_t ns = (size_t)n_seq, ntok = (size_t)n_tok;
    auto t = mirror<FbTab>([&](Layout L, FbTab& p) {
        return L.part(p.frame_off, ns + 1).part(p.tile_off, ns + 1).part(p.tok_off, ns + 1).part(p.tok_frame, ntok)
            .part(p.seq_n, ns).part(p.tok_word, ntok).bytes();
    });
    TRY(stage(c, PIN_FB_TAB, t));
    std::memcpy(t.h.frame_off, h_frame_off, (ns + 1) * sizeof(int64_t));
    t.h.tile_off[0] = 0;
    for (size_t q = 0; q < ns; ++q) {
        t.h.tile_off[q + 1] = t.h.tile_off[q] + (h_frame_off[q + 1] - h_frame_off[q] + FB_TILE - 1) / FB_TILE;
        t.h.seq_n[q] = h_seq_n_cols ? h_seq_n_cols[q] : n_cols;
        t.h.tok_off[q + 1] = tokens ? h_tok_off[q + 1] : 0;
    }
    t.h.tok_off[0] = 0;
    if (n_tok) {
        std::memcpy(t.h.tok_frame, h_tok_frame, ntok * sizeof(int64_t));
        std::memcpy(t.h.tok_word, h_tok_word, ntok * sizeof(int32_t));
    }
    const int G = group_width(n_cols);
    Call call(c);
    TRY(call.opened);
    TRY(send(call, S_FB_TAB, t));
    void* p = nullptr;
    TRY(scratch(c, S_FB_FWD, (size_t)t.h.tile_off[ns] * (size_t)G * sizeof(double), &p));
    double* fwd = (double*)p;
    double *d_conf = nullptr, *d_logz = nullptr;
    TRY(carve(c, scratch, S_FB_OUT, [&](Layout L) { return L.part(d_logz, ns).part(d_conf, ntok).bytes(); }));
    {
        Timer tm(c, SPKD_T_FB_POSTERIOR);
        with_group(n_cols, [&](auto g) {
            fb_launch<decltype(g)::value>(c, d_scores, t.d, tokens, n_seq, n_cols, penalty, scale, fwd, d_post, d_conf, d_logz);
        });
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_logz, d_logz, ns * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (n_tok) HIPCHK(c, hipMemcpyAsync(h_conf, d_conf, ntok * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return call.finish();
}

// ------------------------------------------------------------------ (8) speaker models and their scores
static_assert(GS_TILE == SPKD_GAUSS_TILE && GS_MODEL == SPKD_GAUSS_MODEL, "the header states the kernels' tile and model");

spkd_status spkd_gauss_models(spkd_ctx* c, const double* d_stats, int64_t n, double* d_models, int32_t* h_ok) {
    if (!c || n < 0) return SPKD_EINVAL;
    if (n == 0) return SPKD_OK;
    if (!d_stats || !d_models || !h_ok) return fail(c, SPKD_EINVAL, "null argument");
    if (n > 0x7fffffff) return fail(c, SPKD_EINVAL, "gauss_models: too many records");
    if ((uintptr_t)d_stats % 16 || (uintptr_t)d_models % 16)
        return fail(c, SPKD_EINVAL, "gauss_models: record and model buffers must be 16-byte aligned");
    Call call(c);
    TRY(call.opened);
    void* d_ok = nullptr;
    TRY(scratch(c, S_GAUSS_OK, (size_t)n * sizeof(int32_t), &d_ok));
    {
        Timer t(c, SPKD_T_GAUSS_MODELS);
        hipLaunchKernelGGL(k_gauss_models, dim3((unsigned)n), dim3(WAVE), 0, c->stream, d_stats, d_models, (int*)d_ok);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_ok, d_ok, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    return call.finish();
}

namespace {
// what spkd_gauss_loglik, spkd_gmm_loglik_seq and spkd_post_stats ask of each sequence (`name` opens the messages)
spkd_status check_seq(spkd_ctx* c, const char* name, int64_t b, int64_t e, int64_t n_frames, int64_t m, int64_t k,
                      int32_t n_cols, int64_t n_models) {
    if (b < 0 || e < b || e > n_frames) return fail(c, SPKD_EINVAL, std::string(name) + ": sequence outside [0, n_frames]");
    if (k < 0 || k > n_cols) return fail(c, SPKD_EINVAL, std::string(name) + ": 0 <= models of a sequence <= n_cols");
    if (m < 0 || m + k > n_models) return fail(c, SPKD_EINVAL, std::string(name) + ": model index out of range");
    return SPKD_OK;
}

// The sequence table of spkd_gauss_loglik and spkd_gmm_loglik_seq, as the kernels take it: per sequence its
// frames [begin, end), its first row of the scores, its first tile, its first model and its model count;
// per model ok; per tile its sequence.  A mirrored block: build() stages and fills it, send() sends it.
struct SeqTable {
    struct Tab { long long *begin, *end, *row, *tile; int *model, *n_models, *ok, *tile_seq; } h{}, d{};
    Image host, dev;
    size_t ns = 0, nm = 0, nt = 0;  // sequences, models, tiles (0: no frame, nothing to do)

    size_t parts(Layout L, Tab& t) const {
        return L.part(t.begin, ns).part(t.end, ns).part(t.row, ns).part(t.tile, ns).part(t.model, ns).part(t.n_models, ns)
            .part(t.ok, nm).part(t.tile_seq, nt).bytes();
    }
    // the checks that the two calls share (`name` opens their messages), the tiles counted, the image filled
    spkd_status build(spkd_ctx* c, const std::string& name, int64_t tile_frames, int pin_slot, const float* d_frames,
                      int64_t n_frames, const double* d_models, int64_t n_models, const int32_t* h_model_ok, int64_t n_seq,
                      const int64_t* h_seq_begin, const int64_t* h_seq_end, const int32_t* h_seq_model,
                      const int32_t* h_seq_n_models, int32_t n_cols, const float* d_scores) {
        if (n_cols < 1 || n_cols > GS_MAX_COLS) return fail(c, SPKD_EINVAL, name + ": 1 <= n_cols <= 16");
        if (n_frames < 0 || n_models < 0 || n_models > 0x7fffffff || n_seq > 0x7fffffff)
            return fail(c, SPKD_EINVAL, name + ": bad count");
        if ((uintptr_t)d_models % 16 || (uintptr_t)d_frames % 4 || (uintptr_t)d_scores % 4)
            return fail(c, SPKD_EINVAL, name + ": misaligned buffer (models: 16 bytes)");
        int64_t n_tiles = 0;
        for (int64_t q = 0; q < n_seq; ++q) {
            const int64_t b = h_seq_begin[q], e = h_seq_end[q];
            TRY(check_seq(c, name.c_str(), b, e, n_frames, h_seq_model[q], h_seq_n_models[q], n_cols, n_models));
            n_tiles += (e - b + tile_frames - 1) / tile_frames;
        }
        if (n_tiles == 0) return SPKD_OK;
        if (n_tiles > 0x7fffffff) return fail(c, SPKD_EINVAL, name + ": too many frames in one call");
        ns = (size_t)n_seq, nm = (size_t)n_models, nt = (size_t)n_tiles;
        TRY(stage(c, pin_slot, *this));
        std::memcpy(h.begin, h_seq_begin, ns * sizeof(int64_t));
        std::memcpy(h.end, h_seq_end, ns * sizeof(int64_t));
        std::memcpy(h.model, h_seq_model, ns * sizeof(int32_t));
        std::memcpy(h.n_models, h_seq_n_models, ns * sizeof(int32_t));
        std::memcpy(h.ok, h_model_ok, nm * sizeof(int32_t));
        long long row = 0, tile = 0;
        for (size_t q = 0; q < ns; ++q) {
            h.row[q] = row;
            h.tile[q] = tile;
            const long long len = h.end[q] - h.begin[q], k = (len + tile_frames - 1) / tile_frames;
            for (long long i = 0; i < k; ++i) h.tile_seq[tile + i] = (int)q;
            row += len;
            tile += k;
        }
        return SPKD_OK;
    }
};
static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int) == sizeof(int32_t), "the tables take the caller's arrays as they are");
}  // namespace

spkd_status spkd_gauss_loglik(spkd_ctx* c, const float* d_frames, int64_t n_frames, const double* d_models,
                              int64_t n_models, const int32_t* h_model_ok, int64_t n_seq, const int64_t* h_seq_begin,
                              const int64_t* h_seq_end, const int32_t* h_seq_model, const int32_t* h_seq_n_models,
                              int32_t n_cols, float* d_scores) {
    if (!c || n_seq < 0) return SPKD_EINVAL;
    if (n_seq == 0) return SPKD_OK;
    if (!d_frames || !d_models || !h_model_ok || !h_seq_begin || !h_seq_end || !h_seq_model || !h_seq_n_models || !d_scores)
        return fail(c, SPKD_EINVAL, "null argument");
    SeqTable t;
    TRY(t.build(c, "gauss_loglik", GS_TILE, PIN_GAUSS_IDX, d_frames, n_frames, d_models, n_models, h_model_ok, n_seq,
                h_seq_begin, h_seq_end, h_seq_model, h_seq_n_models, n_cols, d_scores));
    if (!t.nt) return SPKD_OK;
    Call call(c);
    TRY(call.opened);
    TRY(send(call, S_GAUSS_IDX, t));
    {
        Timer tm(c, SPKD_T_GAUSS_LOGLIK);
        hipLaunchKernelGGL(k_gauss_loglik, dim3((unsigned)t.nt), dim3(WAVE), 0, c->stream, d_frames, d_models, t.d.ok,
                           t.d.begin, t.d.end, t.d.row, t.d.tile, t.d.model, t.d.n_models, t.d.tile_seq, (int)n_cols,
                           d_scores);
    }
    HIPCHK(c, hipGetLastError());
    return call.finish();
}

// ------------------------------------------------------------------ (8) speakers from posteriors
static_assert(STATS_CHUNK == SPKD_POST_CHUNK, "the header states the kernel's chunk");

spkd_status spkd_post_stats(spkd_ctx* c, const float* d_frames, int64_t n_frames, const float* d_post, int64_t n_seq,
                            const int64_t* h_seq_begin, const int64_t* h_seq_end, const int32_t* h_seq_model,
                            const int32_t* h_seq_n_models, int32_t n_cols, int64_t n_models, double* d_stats) {
    if (!c) return SPKD_EINVAL;
    if (n_cols < 1 || n_cols > GS_MAX_COLS) return fail(c, SPKD_EINVAL, "post_stats: 1 <= n_cols <= 16");
    if (n_frames < 0 || n_seq < 0 || n_models < 0 || n_models > 0x7fffffff || n_seq > 0x7fffffff)
        return fail(c, SPKD_EINVAL, "post_stats: bad count");
    if (!d_stats || (n_seq > 0 && (!d_frames || !d_post || !h_seq_begin || !h_seq_end || !h_seq_model || !h_seq_n_models)))
        return fail(c, SPKD_EINVAL, "post_stats: null argument");
    if ((uintptr_t)d_stats % 16 || (uintptr_t)d_frames % 4 || (uintptr_t)d_post % 4)
        return fail(c, SPKD_EINVAL, "post_stats: misaligned buffer (records: 16 bytes)");
    // per model the range that covers it (first model, count; count 0: none yet) and its workgroups
    std::vector<int32_t> cover((size_t)n_models * 2, 0);
    std::vector<int64_t> count((size_t)n_models, 0);
    int64_t n_items = 0;
    for (int64_t q = 0; q < n_seq; ++q) {
        const int64_t b = h_seq_begin[q], e = h_seq_end[q], m = h_seq_model[q], k = h_seq_n_models[q];
        TRY(check_seq(c, "post_stats", b, e, n_frames, m, k, n_cols, n_models));
        const int64_t chunks = (e - b + STATS_CHUNK - 1) / STATS_CHUNK;
        for (int64_t j = m; j < m + k; ++j) {
            int32_t* cv = &cover[(size_t)j * 2];
            if (cv[1] == 0) cv[0] = (int32_t)m, cv[1] = (int32_t)k;
            else if (cv[0] != m || cv[1] != k)
                return fail(c, SPKD_EINVAL, "post_stats: the model ranges of two sequences are identical or disjoint");
            count[(size_t)j] += chunks;
        }
        n_items += chunks * k;
    }
    if (n_items > 0x7fffffff) return fail(c, SPKD_EINVAL, "post_stats: too many frames in one call");
    if (n_models == 0) return SPKD_OK;
    // the work table, as the kernels take it: per workgroup of k_post_chunk_stats its chunk, column and
    // partial record; per model the first of its partial records (k_reduce_sets' sets)
    const size_t ni = (size_t)n_items, nm = (size_t)n_models;
    struct Tab { PostItem* item; long long* model_off; };
    auto t = mirror<Tab>([&](Layout L, Tab& p) { return L.part(p.item, ni).part(p.model_off, nm + 1).bytes(); });
    TRY(stage(c, PIN_POST_TAB, t));
    t.h.model_off[0] = 0;
    for (size_t j = 0; j < nm; ++j) t.h.model_off[j + 1] = t.h.model_off[j] + count[j];
    // a model's partial records: consecutive, in the order (sequence of the call, chunk); `count` turns cursor
    for (size_t j = 0; j < nm; ++j) count[j] = t.h.model_off[j];
    PostItem* it = t.h.item;
    int64_t row = 0;
    for (int64_t q = 0; q < n_seq; ++q) {
        const int64_t b = h_seq_begin[q], e = h_seq_end[q];
        const int32_t m = h_seq_model[q], k = h_seq_n_models[q];
        for (int64_t f = b; f < e; f += STATS_CHUNK)
            for (int32_t col = 0; col < k; ++col, ++it) {
                it->begin = f;
                it->row = row + (f - b);
                it->slot = count[(size_t)(m + col)]++;
                it->len = (int32_t)std::min<int64_t>(STATS_CHUNK, e - f);
                it->col = col;
            }
        row += e - b;
    }
    Call call(c);
    TRY(call.opened);
    TRY(send(call, S_POST_TAB, t));
    void* d_partial = nullptr;
    TRY(scratch(c, S_POST_PARTIAL, ni * REC * sizeof(double), &d_partial));
    {
        Timer tm(c, SPKD_T_POST_STATS);
        if (ni)
            hipLaunchKernelGGL(k_post_chunk_stats, dim3((unsigned)ni), dim3(STATS_TPB), 0, c->stream, d_frames, d_post,
                               (const PostItem*)t.d.item, (int)n_cols, (double*)d_partial);
        hipLaunchKernelGGL(k_reduce_sets, dim3((unsigned)n_models), dim3(STATS_TPB), 0, c->stream,
                           (const double*)d_partial, (const int64_t*)t.d.model_off, d_stats);
    }
    HIPCHK(c, hipGetLastError());
    return call.finish();
}

// ------------------------------------------------------------------ (9) mixture speaker models and their scores
static_assert(GT_COMP == SPKD_GMM_COMP && GT_MAX_COMP == SPKD_GMM_MAX_COMP && GT_TILE == SPKD_GMM_TILE &&
              GT_CHUNK_TILES == SPKD_GMM_CHUNK_TILES, "the header states the kernels' layout and partition");

namespace {
// The range-set table of spkd_gmm_train and spkd_ubm_stats, as the kernels take it: per range its first
// frame and the ordinal of that frame among its speaker's; per speaker its ranges [set_off], its frame
// count n and its chunks [chunk_off]; per chunk its speaker and its index within the speaker.  A mirrored block.
struct RangeTable {
    struct Tab { long long *begin, *ord, *set_off, *n, *chunk_off; int *chunk_spk, *chunk_idx; } h{}, d{};
    Image host, dev;
    size_t ns = 0, nr = 0, nc = 0;  // speakers, ranges, chunks

    size_t parts(Layout L, Tab& t) const {
        return L.part(t.begin, nr).part(t.ord, nr).part(t.set_off, ns + 1).part(t.n, ns).part(t.chunk_off, ns + 1)
            .part(t.chunk_spk, nc).part(t.chunk_idx, nc).bytes();
    }
    // the checks that the two calls share (`name` opens their messages), the chunks counted, the image filled
    spkd_status build(spkd_ctx* c, const std::string& name, int pin_slot, int64_t n_frames, int64_t n_speakers,
                      const int64_t* h_set_off, const int64_t* h_range_begin, const int64_t* h_range_end) {
        if (h_set_off[0] != 0) return fail(c, SPKD_EINVAL, name + ": set_off[0] must be 0");
        for (int64_t s = 0; s < n_speakers; ++s)
            if (h_set_off[s + 1] <= h_set_off[s]) return fail(c, SPKD_EINVAL, name + ": set_off must ascend: no empty set");
        int64_t n_chunks = 0;
        for (int64_t s = 0; s < n_speakers; ++s) {
            int64_t n = 0;
            for (int64_t r = h_set_off[s]; r < h_set_off[s + 1]; ++r) {
                const int64_t b = h_range_begin[r], e = h_range_end[r];
                if (b < 0 || e < b || e > n_frames) return fail(c, SPKD_EINVAL, name + ": range outside [0, n_frames]");
                n += e - b;
            }
            n_chunks += (n + GT_CHUNK - 1) / GT_CHUNK;
        }
        if (n_chunks > 0x7fffffff) return fail(c, SPKD_EINVAL, name + ": too many frames in one call");
        ns = (size_t)n_speakers, nr = (size_t)h_set_off[n_speakers], nc = (size_t)n_chunks;
        TRY(stage(c, pin_slot, *this));
        std::memcpy(h.begin, h_range_begin, nr * sizeof(int64_t));
        std::memcpy(h.set_off, h_set_off, (ns + 1) * sizeof(int64_t));
        long long chunk = 0;
        for (size_t s = 0; s < ns; ++s) {
            long long n = 0;
            for (int64_t r = h_set_off[s]; r < h_set_off[s + 1]; ++r) {
                h.ord[r] = n;
                n += h_range_end[r] - h_range_begin[r];
            }
            h.n[s] = n;
            h.chunk_off[s] = chunk;
            for (long long i = 0; i < (n + GT_CHUNK - 1) / GT_CHUNK; ++i, ++chunk) {
                h.chunk_spk[chunk] = (int)s;
                h.chunk_idx[chunk] = (int)i;
            }
        }
        h.chunk_off[ns] = chunk;
        return SPKD_OK;
    }
};
}  // namespace

spkd_status spkd_gmm_train(spkd_ctx* c, const float* d_frames, int64_t n_frames, int64_t n_speakers,
                           const int64_t* h_set_off, const int64_t* h_range_begin, const int64_t* h_range_end,
                           int32_t n_comp, int32_t n_iter, int32_t from_model, double var_floor, double* d_gmm,
                           int32_t* h_ok, double* h_loglik) {
    if (!c || n_speakers < 0) return SPKD_EINVAL;
    if (n_speakers == 0) return SPKD_OK;
    if (!d_frames || !h_set_off || !h_range_begin || !h_range_end || !d_gmm || !h_ok || (n_iter > 0 && !h_loglik))
        return fail(c, SPKD_EINVAL, "null argument");
    if (bad_comp(n_comp)) return fail(c, SPKD_EINVAL, "gmm_train: 1 <= n_comp <= 8");
    if (n_iter < 0) return fail(c, SPKD_EINVAL, "gmm_train: n_iter >= 0");
    if (!(var_floor >= 0.0) || !std::isfinite(var_floor)) return fail(c, SPKD_EINVAL, "gmm_train: var_floor must be finite and >= 0");
    if (n_frames < 0 || n_speakers > 0x7fffffff) return fail(c, SPKD_EINVAL, "gmm_train: bad count");
    if ((uintptr_t)d_gmm % 16 || (uintptr_t)d_frames % 4) return fail(c, SPKD_EINVAL, "gmm_train: misaligned buffer (models: 16 bytes)");
    RangeTable t;
    TRY(t.build(c, "gmm_train", PIN_GT_TAB, n_frames, n_speakers, h_set_off, h_range_begin, h_range_end));
    const size_t ns = t.ns, nc = t.nc, nl = ns * (size_t)n_iter;
    // what comes back: the ok flags and the log-likelihoods, through pinned memory as well
    struct Out { double* loglik; int32_t* ok; };
    auto out = mirror<Out>([&](Layout L, Out& o) { return L.part(o.loglik, nl).part(o.ok, ns).bytes(); });
    double *d_part = nullptr, *d_part_ll = nullptr, *d_floor = nullptr;
    TRY(stage(c, PIN_GT_OUT, out));
    Call call(c);
    TRY(call.opened);
    TRY(send(call, S_GT_TAB, t));
    TRY(carve(c, scratch, S_GT_WORK, [&](Layout L) {
        return place(L, out).part(d_part, nc * (size_t)n_comp * GT_COMP).part(d_part_ll, nc).part(d_floor, ns * WAVE).bytes();
    }));
    {
        Timer tm(c, SPKD_T_GMM_TRAIN);
        auto estep = [&](auto hard) {
            if (nc)
                hipLaunchKernelGGL(k_gmm_estep<decltype(hard)::value>, dim3((unsigned)nc), dim3(WAVE), 0, c->stream, d_frames,
                                   t.d.begin, t.d.ord, t.d.set_off, t.d.n, t.d.chunk_spk, t.d.chunk_idx, d_gmm,
                                   (int)n_comp, d_part, d_part_ll);
        };
        auto mstep = [&](int init, int iter) {
            hipLaunchKernelGGL(k_gmm_mstep, dim3((unsigned)ns), dim3(WAVE), 0, c->stream, d_part, d_part_ll, t.d.chunk_off,
                               t.d.n, (int)n_comp, init, from_model ? 0 : 1, var_floor, iter, (int)n_iter, d_gmm, d_floor,
                               out.d.ok, out.d.loglik);
        };
        // the whole loop in one go: the hard pass (floor, first ok, initial model), then n_iter EM steps
        estep(std::true_type());
        mstep(1, 0);
        for (int i = 0; i < n_iter; ++i) {
            estep(std::false_type());
            mstep(0, i);
        }
    }
    HIPCHK(c, hipGetLastError());
    TRY(copy(call, out, hipMemcpyDeviceToHost));
    TRY(call.finish());
    std::memcpy(h_ok, out.h.ok, ns * sizeof(int32_t));
    if (nl) std::memcpy(h_loglik, out.h.loglik, nl * sizeof(double));
    return SPKD_OK;
}

spkd_status spkd_gmm_loglik_seq(spkd_ctx* c, const float* d_frames, int64_t n_frames, const double* d_gmm,
                                int32_t n_comp, int64_t n_models, const int32_t* h_model_ok, int64_t n_seq,
                                const int64_t* h_seq_begin, const int64_t* h_seq_end, const int32_t* h_seq_model,
                                const int32_t* h_seq_n_models, int32_t n_cols, float* d_scores) {
    if (!c || n_seq < 0) return SPKD_EINVAL;
    if (n_seq == 0) return SPKD_OK;
    if (!d_frames || !d_gmm || !h_model_ok || !h_seq_begin || !h_seq_end || !h_seq_model || !h_seq_n_models || !d_scores)
        return fail(c, SPKD_EINVAL, "null argument");
    if (bad_comp(n_comp)) return fail(c, SPKD_EINVAL, "gmm_loglik_seq: 1 <= n_comp <= 8");
    SeqTable t;
    TRY(t.build(c, "gmm_loglik_seq", GT_TILE, PIN_GT_IDX, d_frames, n_frames, d_gmm, n_models, h_model_ok, n_seq,
                h_seq_begin, h_seq_end, h_seq_model, h_seq_n_models, n_cols, d_scores));
    if (!t.nt) return SPKD_OK;
    Call call(c);
    TRY(call.opened);
    TRY(send(call, S_GT_IDX, t));
    {
        Timer tm(c, SPKD_T_GMM_SEQ_LOGLIK);
        hipLaunchKernelGGL(k_gmm_loglik_seq, dim3((unsigned)t.nt), dim3(WAVE), 0, c->stream, d_frames, d_gmm, (int)n_comp,
                           t.d.ok, t.d.begin, t.d.end, t.d.row, t.d.tile, t.d.model, t.d.n_models, t.d.tile_seq,
                           (int)n_cols, d_scores);
    }
    HIPCHK(c, hipGetLastError());
    return call.finish();
}

// ------------------------------------------------------------------ (10) linking by cross-likelihood ratio
static_assert(BW_COMP == SPKD_BW_COMP && CL_MAX_N == SPKD_CLR_MAX_N, "the header states the record and the limit");

spkd_status spkd_ubm_stats(spkd_ctx* c, const float* d_frames, int64_t n_frames, const double* d_ubm, int32_t n_comp,
                           int64_t n_speakers, const int64_t* h_set_off, const int64_t* h_range_begin,
                           const int64_t* h_range_end, double* d_bw, int32_t* h_ok) {
    if (!c || n_speakers < 0) return SPKD_EINVAL;
    if (n_speakers == 0) return SPKD_OK;
    if (!d_frames || !d_ubm || !h_set_off || !h_range_begin || !h_range_end || !d_bw || !h_ok)
        return fail(c, SPKD_EINVAL, "null argument");
    if (bad_comp(n_comp)) return fail(c, SPKD_EINVAL, "ubm_stats: 1 <= n_comp <= 8");
    if (n_frames < 0 || n_speakers > 0x7fffffff) return fail(c, SPKD_EINVAL, "ubm_stats: bad count");
    if ((uintptr_t)d_ubm % 16 || (uintptr_t)d_bw % 16 || (uintptr_t)d_frames % 4)
        return fail(c, SPKD_EINVAL, "ubm_stats: misaligned buffer (model and records: 16 bytes)");
    RangeTable t;
    TRY(t.build(c, "ubm_stats", PIN_UBM_TAB, n_frames, n_speakers, h_set_off, h_range_begin, h_range_end));
    const size_t ns = t.ns, nc = t.nc;
    auto ok = mirror<int32_t*>([&](Layout L, int32_t*& p) { return L.part(p, ns).bytes(); });   // (a block of one array)
    TRY(stage(c, PIN_UBM_OUT, ok));
    Call call(c);
    TRY(call.opened);
    TRY(send(call, S_UBM_TAB, t));
    double* d_part = nullptr;
    TRY(carve(c, scratch, S_UBM_WORK, [&](Layout L) { return place(L, ok).part(d_part, nc * (size_t)n_comp * BW_COMP).bytes(); }));
    {
        Timer tm(c, SPKD_T_UBM_STATS);
        if (nc)
            hipLaunchKernelGGL(k_ubm_estep, dim3((unsigned)nc), dim3(WAVE), 0, c->stream, d_frames, t.d.begin, t.d.ord,
                               t.d.set_off, t.d.n, t.d.chunk_spk, t.d.chunk_idx, d_ubm, (int)n_comp, d_part);
        hipLaunchKernelGGL(k_ubm_reduce, dim3((unsigned)ns), dim3(WAVE), 0, c->stream, d_part, t.d.chunk_off, t.d.n,
                           (int)n_comp, d_bw, ok.d);
    }
    HIPCHK(c, hipGetLastError());
    TRY(copy(call, ok, hipMemcpyDeviceToHost));
    TRY(call.finish());
    std::memcpy(h_ok, ok.h, ns * sizeof(int32_t));
    return SPKD_OK;
}

spkd_status spkd_clr_link(spkd_ctx* c, const double* d_bw, int64_t n, const int32_t* h_ok, const double* d_ubm,
                          int32_t n_comp, double relevance, double threshold, int32_t max_spk, int32_t* h_merge_a,
                          int32_t* h_merge_b, double* h_merge_d, int32_t* h_n_merges, double* h_stat_max,
                          double* h_stat_min) {
    if (!c || n < 0) return SPKD_EINVAL;
    if (n == 0) return SPKD_OK;
    if (!d_bw || !h_ok || !d_ubm || !h_merge_a || !h_merge_b || !h_merge_d || !h_n_merges || !h_stat_max || !h_stat_min)
        return fail(c, SPKD_EINVAL, "null argument");
    if (n > CL_MAX_N) return fail(c, SPKD_EINVAL, "clr_link: at most 4096 speakers");
    if (bad_comp(n_comp)) return fail(c, SPKD_EINVAL, "clr_link: 1 <= n_comp <= 8");
    if (!(relevance > 0.0) || !std::isfinite(relevance)) return fail(c, SPKD_EINVAL, "clr_link: relevance must be finite and > 0");
    if (std::isnan(threshold)) return fail(c, SPKD_EINVAL, "clr_link: threshold is NaN");
    if (max_spk < 0) return fail(c, SPKD_EINVAL, "clr_link: max_spk >= 0");
    if ((uintptr_t)d_bw % 16 || (uintptr_t)d_ubm % 16)
        return fail(c, SPKD_EINVAL, "clr_link: misaligned buffer (model and records: 16 bytes)");
    const double nan = std::nan("");
    if (n == 1) {                                                        // nothing to compare
        *h_n_merges = 0;
        *h_stat_max = *h_stat_min = nan;
        return SPKD_OK;
    }
    const size_t ns = (size_t)n, ne = ns * (size_t)n_comp * BW_COMP;
    struct Out { double *d, *stat; int32_t *a, *b, *nm; };
    auto out = mirror<Out>([&](Layout L, Out& o) { return L.part(o.d, ns).part(o.stat, 2).part(o.a, ns).part(o.b, ns).part(o.nm, 1).bytes(); });
    auto ok = mirror<int32_t*>([&](Layout L, int32_t*& p) { return L.part(p, ns).bytes(); });   // (a block of one array)
    TRY(stage(c, PIN_CLR_OUT, out));
    TRY(stage(c, PIN_CLR_IN, ok));
    std::memcpy(ok.h, h_ok, ns * sizeof(int32_t));
    Call call(c);
    TRY(call.opened);
    double *d_w = nullptr, *d_t = nullptr, *d_n = nullptr;
    void* d_mat = nullptr;
    TRY(carve(c, scratch, S_CLR_WORK, [&](Layout L) { return place(place(L, out), ok).part(d_w, ne).part(d_t, ne).part(d_n, ns).bytes(); }));
    TRY(scratch(c, S_CLR_MAT, ns * ns * sizeof(double), &d_mat));
    TRY(copy(call, ok, hipMemcpyHostToDevice));
    {
        Timer t(c, SPKD_T_CLR_LINK);
        hipLaunchKernelGGL(k_clr_prep, dim3((unsigned)ns), dim3(WAVE), 0, c->stream, d_bw, d_ubm, (int)n_comp, relevance,
                           d_w, d_t, d_n);
        hipLaunchKernelGGL(k_clr_matrix, dim3((unsigned)ns), dim3(CL_MAT_TPB), 0, c->stream, (const double*)d_w,
                           (const double*)d_t, (const double*)d_n, (const int*)ok.d, (int)n, (int)n_comp, (double*)d_mat,
                           c->d_err);
        hipLaunchKernelGGL(k_clr_chain, dim3(1), dim3(CL_TPB), 0, c->stream, d_w, d_t, d_n, (double*)d_mat,
                           (const int*)ok.d, (int)n, (int)n_comp, d_ubm, relevance, threshold, (int)max_spk, (int*)out.d.a,
                           (int*)out.d.b, out.d.d, (int*)out.d.nm, out.d.stat, c->d_err);
    }
    HIPCHK(c, hipGetLastError());
    TRY(copy(call, out, hipMemcpyDeviceToHost));
    const spkd_status st = call.finish();
    if (st != SPKD_OK && st != SPKD_ENONFINITE) return st;
    const int32_t nm = *out.h.nm;                                        // (the log so far when a CLR was not finite)
    *h_n_merges = nm;
    std::memcpy(h_merge_a, out.h.a, (size_t)nm * sizeof(int32_t));
    std::memcpy(h_merge_b, out.h.b, (size_t)nm * sizeof(int32_t));
    std::memcpy(h_merge_d, out.h.d, (size_t)nm * sizeof(double));
    *h_stat_max = out.h.stat[0];
    *h_stat_min = out.h.stat[1];
    return st;
}

// ------------------------------------------------------------------ (10b) feature warping
static_assert(WP_MAX_WINDOW == SPKD_WARP_MAX_WINDOW && WP_TILE == SPKD_WARP_TILE, "the header states the limit and the tile");

namespace {
// The tables of spkd_feature_warp as the kernel takes them: per run its first frame and the compacted ordinal
// of that frame within its set; per set its runs [set_off], its frame count and where its quantile table
// starts; per tile its set and its index within the set; the caller's quantile tables.  A mirrored block.
struct WarpTable {
    struct Tab { long long *begin, *ord, *set_off, *len, *table_off; int *tile_set, *tile_idx; float* table; } h{}, d{};
    Image host, dev;
    size_t ns = 0, nr = 0, nt = 0, nq = 0;   // sets, runs, tiles, floats of the quantile tables
    int n_max = 0;                           // the widest window of a set: min(window, its frames)

    size_t parts(Layout L, Tab& t) const {
        return L.part(t.begin, nr).part(t.ord, nr).part(t.set_off, ns + 1).part(t.len, ns).part(t.table_off, ns)
            .part(t.tile_set, nt).part(t.tile_idx, nt).part(t.table, nq).bytes();
    }
    // the checks of the sets, the runs and the table slices, the tiles counted, the image filled
    spkd_status build(spkd_ctx* c, int64_t n_frames, int64_t n_sets, const int64_t* h_set_off, const int64_t* h_range_begin,
                      const int64_t* h_range_end, int32_t window, const float* h_table, int64_t table_len,
                      const int64_t* h_table_off) {
        if (h_set_off[0] != 0) return fail(c, SPKD_EINVAL, "feature_warp: set_off[0] must be 0");
        for (int64_t s = 0; s < n_sets; ++s)
            if (h_set_off[s + 1] < h_set_off[s]) return fail(c, SPKD_EINVAL, "feature_warp: set_off must not decrease");
        int64_t n_tiles = 0, last_end = 0;
        for (int64_t s = 0; s < n_sets; ++s) {
            int64_t n = 0;
            for (int64_t r = h_set_off[s]; r < h_set_off[s + 1]; ++r) {
                const int64_t b = h_range_begin[r], e = h_range_end[r];
                if (b < 0 || e < b || e > n_frames) return fail(c, SPKD_EINVAL, "feature_warp: range outside [0, n_frames]");
                if (b < last_end) return fail(c, SPKD_EINVAL, "feature_warp: the ranges must be ascending and disjoint");
                last_end = e;
                n += e - b;                  // (disjoint ranges inside [0, n_frames]: no overflow)
            }
            if (n > 0x7fffffffLL) return fail(c, SPKD_EINVAL, "feature_warp: a set of more than 2^31 - 1 frames");
            if (n == 0) continue;
            const int64_t w = n < window ? n : window, off = h_table_off[s];
            if (off < 0 || off > table_len || 2 * w - 1 > table_len - off)
                return fail(c, SPKD_EINVAL, "feature_warp: a table slice outside [0, table_len]");
            if (w > n_max) n_max = (int)w;
            n_tiles += (n + WP_TILE - 1) / WP_TILE;
        }
        if (n_tiles > 0x7fffffff) return fail(c, SPKD_EINVAL, "feature_warp: too many frames in one call");
        ns = (size_t)n_sets, nr = (size_t)h_set_off[n_sets], nt = (size_t)n_tiles, nq = (size_t)table_len;
        if (!nt) return SPKD_OK;
        TRY(stage(c, PIN_WARP_TAB, *this));
        std::memcpy(h.begin, h_range_begin, nr * sizeof(int64_t));
        std::memcpy(h.set_off, h_set_off, (ns + 1) * sizeof(int64_t));
        std::memcpy(h.table_off, h_table_off, ns * sizeof(int64_t));
        std::memcpy(h.table, h_table, nq * sizeof(float));
        size_t tile = 0;
        for (size_t s = 0; s < ns; ++s) {
            long long n = 0;
            for (int64_t r = h_set_off[s]; r < h_set_off[s + 1]; ++r) {
                h.ord[r] = n;
                n += h_range_end[r] - h_range_begin[r];
            }
            h.len[s] = n;
            for (long long i = 0; i < (n + WP_TILE - 1) / WP_TILE; ++i, ++tile) {
                h.tile_set[tile] = (int)s;
                h.tile_idx[tile] = (int)i;
            }
        }
        return SPKD_OK;
    }
};
}  // namespace

spkd_status spkd_feature_warp(spkd_ctx* c, const float* d_frames, int64_t n_frames, int64_t n_sets, const int64_t* h_set_off,
                              const int64_t* h_range_begin, const int64_t* h_range_end, int32_t window, const float* h_table,
                              int64_t table_len, const int64_t* h_table_off, float* d_out) {
    if (!c) return SPKD_EINVAL;
    if (!d_frames || !h_set_off || !h_range_begin || !h_range_end || !h_table || !h_table_off || !d_out)
        return fail(c, SPKD_EINVAL, "feature_warp: null argument");
    if (n_frames < 0 || n_sets < 0 || n_sets > 0x7fffffff || table_len < 0) return fail(c, SPKD_EINVAL, "feature_warp: bad count");
    if (window < 1 || window > WP_MAX_WINDOW) return fail(c, SPKD_EINVAL, "feature_warp: 1 <= window <= 512");
    if ((uintptr_t)d_frames % 16 || (uintptr_t)d_out % 16) return fail(c, SPKD_EINVAL, "feature_warp: frames and output 16-byte aligned");
    {
        const uintptr_t a = (uintptr_t)d_frames, b = (uintptr_t)d_out, bytes = (uintptr_t)n_frames * D * sizeof(float);
        if (a < b + bytes && b < a + bytes) return fail(c, SPKD_EINVAL, "feature_warp: the output overlaps the frames");
    }
    WarpTable t;
    TRY(t.build(c, n_frames, n_sets, h_set_off, h_range_begin, h_range_end, window, h_table, table_len, h_table_off));
    if (!t.nt) return SPKD_OK;
    if (!c->warp_lds_ok) return fail(c, SPKD_EHIP, "feature_warp: the kernel's dynamic LDS size was not admitted on this device");
    Call call(c);
    TRY(call.opened);
    TRY(send(call, S_WARP_TAB, t));
    {
        Timer tm(c, SPKD_T_FEATURE_WARP);
        hipLaunchKernelGGL(k_feature_warp, dim3((unsigned)t.nt), dim3(WP_TPB), wp_lds_bytes(t.n_max), c->stream, d_frames,
                           t.d.begin, t.d.ord, t.d.set_off, t.d.len, t.d.table_off, (const float*)t.d.table, t.d.tile_set,
                           t.d.tile_idx, (int)window, t.n_max, d_out);
    }
    HIPCHK(c, hipGetLastError());
    return call.finish();
}

// ------------------------------------------------------------------ (11) a gallery of enrolled speakers
static_assert(ID_MAX_G == SPKD_GALLERY_MAX_N, "the header states the limit");

spkd_status spkd_clr_identify(spkd_ctx* c, const double* d_probe_bw, int64_t n_probe, const int32_t* h_probe_ok,
                              int64_t n_groups, const int64_t* h_group_off, const double* d_gallery_bw,
                              int64_t n_gallery, const int32_t* h_gallery_ok, const double* d_ubm, int32_t n_comp,
                              double relevance, double threshold, int32_t exclusive, int32_t* h_ident, double* h_score,
                              double* h_second, double* d_scores) {
    if (!c || n_probe < 0) return SPKD_EINVAL;
    if (n_probe == 0) return SPKD_OK;
    if (!d_probe_bw || !h_probe_ok || !h_group_off || !d_ubm || !h_ident || !h_score || !h_second ||
        (n_gallery > 0 && (!d_gallery_bw || !h_gallery_ok)))
        return fail(c, SPKD_EINVAL, "null argument");
    if (n_probe > CL_MAX_N) return fail(c, SPKD_EINVAL, "clr_identify: at most 4096 probes");
    if (n_gallery < 0 || n_gallery > ID_MAX_G) return fail(c, SPKD_EINVAL, "clr_identify: 0 <= n_gallery <= 16384");
    if (n_groups < 1 || n_groups > CL_MAX_N) return fail(c, SPKD_EINVAL, "clr_identify: 1 <= n_groups <= 4096");
    if (h_group_off[0] != 0 || h_group_off[n_groups] != n_probe)
        return fail(c, SPKD_EINVAL, "clr_identify: group_off runs from 0 to n_probe");
    for (int64_t g = 0; g < n_groups; ++g)
        if (h_group_off[g + 1] < h_group_off[g]) return fail(c, SPKD_EINVAL, "clr_identify: group_off must not go back");
    if (bad_comp(n_comp)) return fail(c, SPKD_EINVAL, "clr_identify: 1 <= n_comp <= 8");
    if (!(relevance > 0.0) || !std::isfinite(relevance)) return fail(c, SPKD_EINVAL, "clr_identify: relevance must be finite and > 0");
    if (std::isnan(threshold)) return fail(c, SPKD_EINVAL, "clr_identify: threshold is NaN");
    if (exclusive != 0 && exclusive != 1) return fail(c, SPKD_EINVAL, "clr_identify: exclusive is 0 or 1");
    if ((uintptr_t)d_probe_bw % 16 || (uintptr_t)d_gallery_bw % 16 || (uintptr_t)d_ubm % 16 || (uintptr_t)d_scores % 16)
        return fail(c, SPKD_EINVAL, "clr_identify: misaligned buffer (model, records and scores: 16 bytes)");
    const double nan = std::nan("");
    const size_t S = (size_t)n_probe, G = (size_t)n_gallery, ng = (size_t)n_groups, E = (size_t)n_comp * BW_COMP;
    if (G == 0) {                                                        // nobody is enrolled: every probe is unknown
        for (size_t s = 0; s < S; ++s) {
            h_ident[s] = -1;
            h_score[s] = h_second[s] = nan;
        }
        return SPKD_OK;
    }
    struct In { int32_t *okp, *okg, *off; };
    struct Out { double *score, *second; int32_t* ident; };
    auto in = mirror<In>([&](Layout L, In& t) { return L.part(t.okp, S).part(t.okg, G).part(t.off, ng + 1).bytes(); });
    auto out = mirror<Out>([&](Layout L, Out& o) { return L.part(o.score, S).part(o.second, S).part(o.ident, S).bytes(); });
    TRY(stage(c, PIN_ID_IN, in));
    TRY(stage(c, PIN_ID_OUT, out));
    std::memcpy(in.h.okp, h_probe_ok, S * sizeof(int32_t));
    std::memcpy(in.h.okg, h_gallery_ok, G * sizeof(int32_t));
    for (size_t g = 0; g <= ng; ++g) in.h.off[g] = (int32_t)h_group_off[g];
    Call call(c);
    TRY(call.opened);
    double *d_tp = nullptr, *d_np = nullptr, *d_tg = nullptr, *d_ng = nullptr;
    TRY(carve(c, scratch, S_ID_WORK, [&](Layout L) {
        return place(place(L, out), in).part(d_tp, S * E).part(d_np, S).part(d_tg, G * E).part(d_ng, G).bytes();
    }));
    double* d_mat = d_scores;
    if (!d_mat) {
        void* p = nullptr;
        TRY(scratch(c, S_ID_MAT, S * G * sizeof(double), &p));
        d_mat = (double*)p;
    }
    TRY(copy(call, in, hipMemcpyHostToDevice));
    {
        Timer t(c, SPKD_T_IDENT_SCORES);
        hipLaunchKernelGGL(k_ident_derive, dim3((unsigned)S), dim3(WAVE), 0, c->stream, d_probe_bw, d_ubm, (int)n_comp,
                           relevance, d_tp, d_np);
        hipLaunchKernelGGL(k_ident_derive, dim3((unsigned)G), dim3(WAVE), 0, c->stream, d_gallery_bw, d_ubm, (int)n_comp,
                           relevance, d_tg, d_ng);
        hipLaunchKernelGGL(k_ident_scores, dim3((unsigned)((S + ID_ROWS - 1) / ID_ROWS), (unsigned)((G + ID_COLS - 1) / ID_COLS)),
                           dim3(ID_TPB), 0, c->stream, d_probe_bw, (const double*)d_tp, (const double*)d_np,
                           (const int*)in.d.okp, (int)S, d_gallery_bw, (const double*)d_tg, (const double*)d_ng,
                           (const int*)in.d.okg, (int)G, (int)n_comp, d_mat, c->d_err);
    }
    {
        Timer t(c, SPKD_T_IDENT_ASSIGN);
        hipLaunchKernelGGL(k_ident_assign, dim3((unsigned)ng), dim3(CL_TPB), 0, c->stream, (const double*)d_mat,
                           (const int*)in.d.okp, (const int*)in.d.okg, (const int*)in.d.off, (int)G, threshold, (int)exclusive,
                           (int*)out.d.ident, out.d.score, out.d.second, (const int*)c->d_err);
    }
    HIPCHK(c, hipGetLastError());
    TRY(copy(call, out, hipMemcpyDeviceToHost));
    const spkd_status st = call.finish();
    if (st != SPKD_OK && st != SPKD_ENONFINITE) return st;
    std::memcpy(h_ident, out.h.ident, S * sizeof(int32_t));              // (every ident -1 when a score was not finite)
    std::memcpy(h_score, out.h.score, S * sizeof(double));
    std::memcpy(h_second, out.h.second, S * sizeof(double));
    return st;
}

spkd_status spkd_bw_accumulate(spkd_ctx* c, const double* d_src_bw, int64_t n_src, int32_t n_comp, int64_t n_sets,
                               const int64_t* h_set_off, const int32_t* h_member, const int32_t* h_dst,
                               const int32_t* h_keep, double* d_dst_bw, int64_t n_dst) {
    if (!c || n_sets < 0) return SPKD_EINVAL;
    if (n_sets == 0) return SPKD_OK;
    if (!d_src_bw || !h_set_off || !h_member || !h_dst || !h_keep || !d_dst_bw) return fail(c, SPKD_EINVAL, "null argument");
    if (n_src < 0 || n_dst < 0 || n_src > 0x7fffffff || n_dst > 0x7fffffff || n_sets > n_dst)
        return fail(c, SPKD_EINVAL, "bw_accumulate: bad count (a set per slot at most)");
    if (bad_comp(n_comp)) return fail(c, SPKD_EINVAL, "bw_accumulate: 1 <= n_comp <= 8");
    if (h_set_off[0] != 0) return fail(c, SPKD_EINVAL, "bw_accumulate: set_off[0] must be 0");
    for (int64_t k = 0; k < n_sets; ++k)
        if (h_set_off[k + 1] < h_set_off[k]) return fail(c, SPKD_EINVAL, "bw_accumulate: set_off must not go back");
    const int64_t n_mem = h_set_off[n_sets];
    if (n_mem > 0x7fffffff) return fail(c, SPKD_EINVAL, "bw_accumulate: too many members");
    for (int64_t m = 0; m < n_mem; ++m)
        if (h_member[m] < 0 || h_member[m] >= n_src) return fail(c, SPKD_EINVAL, "bw_accumulate: member outside [0, n_src)");
    {
        std::vector<char> named((size_t)n_dst, 0);
        for (int64_t k = 0; k < n_sets; ++k) {
            if (h_dst[k] < 0 || h_dst[k] >= n_dst) return fail(c, SPKD_EINVAL, "bw_accumulate: slot outside [0, n_dst)");
            if (named[(size_t)h_dst[k]]++) return fail(c, SPKD_EINVAL, "bw_accumulate: a slot is named twice");
        }
    }
    if ((uintptr_t)d_src_bw % 16 || (uintptr_t)d_dst_bw % 16)
        return fail(c, SPKD_EINVAL, "bw_accumulate: misaligned buffer (records: 16 bytes)");
    const size_t ns = (size_t)n_sets, nm = (size_t)n_mem;
    struct Tab { long long* off; int32_t *member, *slot, *keep; };
    auto tab = mirror<Tab>([&](Layout L, Tab& t) { return L.part(t.off, ns + 1).part(t.member, nm).part(t.slot, ns).part(t.keep, ns).bytes(); });
    TRY(stage(c, PIN_ACC_TAB, tab));
    for (size_t k = 0; k <= ns; ++k) tab.h.off[k] = h_set_off[k];
    std::memcpy(tab.h.member, h_member, nm * sizeof(int32_t));
    std::memcpy(tab.h.slot, h_dst, ns * sizeof(int32_t));
    std::memcpy(tab.h.keep, h_keep, ns * sizeof(int32_t));
    Call call(c);
    TRY(call.opened);
    TRY(send(call, S_ACC_TAB, tab));
    {
        Timer t(c, SPKD_T_BW_ACCUMULATE);
        hipLaunchKernelGGL(k_bw_accumulate, dim3((unsigned)ns), dim3(ID_ACC_TPB), 0, c->stream, d_src_bw,
                           (const long long*)tab.d.off, (const int*)tab.d.member, (const int*)tab.d.slot,
                           (const int*)tab.d.keep, (int)(n_comp * BW_COMP), d_dst_bw);
    }
    HIPCHK(c, hipGetLastError());
    return call.finish();
}

// ------------------------------------------------------------------ (5) host helpers
// float('%.12g' % x) without printf for the common range: x = m 2^k exactly, so
// x 10^s (s = 11 - floor(log10 x)) is formed exactly in 128-bit integers, rounded half
// to even to a 12-digit integer q, and q / 10^s (both exact doubles) is one correctly
// rounded IEEE division -- the same value a correctly rounded strtod gives.
static const double kPow10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11,
                                  1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
static const uint64_t kPow10u[20] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull,
                                     10000000ull, 100000000ull, 1000000000ull, 10000000000ull,
                                     100000000000ull, 1000000000000ull, 10000000000000ull,
                                     100000000000000ull, 1000000000000000ull, 10000000000000000ull,
                                     100000000000000000ull, 1000000000000000000ull,
                                     10000000000000000000ull};

static bool roundtrip_fast(double x, double* out) {
    if (!(x >= 1e-3 && x < 1e11)) return false;
    int e10 = (int)std::floor(std::log10(x));
    if (e10 < -3) e10 = -3;
    if (e10 >= 0) { if (x < kPow10[e10]) --e10; else if (e10 + 1 <= 22 && x >= kPow10[e10 + 1]) ++e10; }
    else { if (x * kPow10[-e10] < 1.0) --e10; else if (x * kPow10[-e10 - 1] >= 1.0) ++e10; }
    if (e10 < -3 || e10 > 10) return false;
    int s = 11 - e10;                              // 1 .. 14
    int k;
    const double fr = std::frexp(x, &k);            // x = fr 2^k, 0.5 <= fr < 1
    const uint64_t m = (uint64_t)std::ldexp(fr, 53);   // 53-bit integer mantissa
    k -= 53;                                        // x = m 2^k
    unsigned __int128 prod = (unsigned __int128)m * kPow10u[s];
    uint64_t q;
    if (k >= 0) {
        if (k > 20) return false;
        q = (uint64_t)(prod << k);
    } else {
        const int sh = -k;
        if (sh >= 120) return false;
        const unsigned __int128 one = 1;
        const unsigned __int128 fl = prod >> sh;
        const unsigned __int128 remn = prod & ((one << sh) - 1);
        const unsigned __int128 half = one << (sh - 1);
        q = (uint64_t)fl;
        if (remn > half || (remn == half && (q & 1))) ++q;
    }
    if (q >= 1000000000000ull) {                    // rounded up to 13 digits: one digit less
        // 10^12 exactly: value is 10^(e10+1)
        if (q != 1000000000000ull) return false;
        q = 100000000000ull;
        s -= 1;
    } else if (q < 100000000000ull) {
        return false;                               // exponent estimate off: let printf decide
    }
    *out = s >= 0 ? (double)q / kPow10[s] : (double)q * kPow10[-s];
    return true;
}

static void roundtrip_range(double* v, int64_t lo, int64_t hi) {
    char buf[64];
    for (int64_t i = lo; i < hi; ++i) {
        double r;
        if (roundtrip_fast(v[i], &r)) { v[i] = r; continue; }
        std::snprintf(buf, sizeof buf, "%.12g", v[i]);
        v[i] = std::strtod(buf, nullptr);
    }
}

void spkd_py2_roundtrip(double* v, int64_t n) {
    // correctly rounded printf / strtod, split over a few host threads for big batches
    const int64_t kMinPerThread = 8192;
    int nthreads = (int)std::min<int64_t>(8, n / kMinPerThread);
    if (nthreads <= 1) { roundtrip_range(v, 0, n); return; }
    std::vector<std::thread> pool;
    const int64_t step = (n + nthreads - 1) / nthreads;
    for (int t = 0; t < nthreads; ++t) {
        const int64_t lo = t * step, hi = std::min<int64_t>(n, lo + step);
        if (lo < hi) pool.emplace_back(roundtrip_range, v, lo, hi);
    }
    for (auto& th : pool) th.join();
}

spkd_status spkd_labels_from_merges(int64_t n, int64_t n_merges, const int32_t* h_a, const int32_t* h_b,
                                    int32_t* h_labels) {
    if (n < 0 || n_merges < 0 || (n > 0 && !h_labels) || (n_merges > 0 && (!h_a || !h_b))) return SPKD_EINVAL;
    // ids: the shrinking list of clusters (by representative record); a merge folds
    // list entry b into entry a and closes the gap, like speakers[a].extend(speakers.pop(b))
    std::vector<int32_t> ids((size_t)n), parent((size_t)n);
    for (int64_t i = 0; i < n; ++i) ids[(size_t)i] = parent[(size_t)i] = (int32_t)i;
    int64_t m = n;
    for (int64_t k = 0; k < n_merges; ++k) {
        const int32_t a = h_a[k], b = h_b[k];
        if (a < 0 || b <= a || b >= m) return SPKD_EINVAL;
        parent[(size_t)ids[(size_t)b]] = ids[(size_t)a];
        ids.erase(ids.begin() + b);
        --m;
    }
    // final position of every surviving representative, then path-compressing finds
    std::vector<int32_t> where((size_t)n, -1);
    for (int64_t p = 0; p < m; ++p) where[(size_t)ids[(size_t)p]] = (int32_t)p;
    for (int64_t i = 0; i < n; ++i) {
        int32_t r = (int32_t)i;
        while (parent[(size_t)r] != r) r = parent[(size_t)r];
        int32_t c = (int32_t)i;
        while (parent[(size_t)c] != r) { const int32_t nx = parent[(size_t)c]; parent[(size_t)c] = r; c = nx; }
        h_labels[i] = where[(size_t)r] + 1;
    }
    return SPKD_OK;
}

spkd_status spkd_count_flags(const int32_t* h_flags, const int64_t* h_off, const int32_t* h_n, int64_t n_groups,
                             int32_t* h_out) {
    if (n_groups < 0 || (n_groups > 0 && (!h_flags || !h_off || !h_n || !h_out))) return SPKD_EINVAL;
    for (int64_t g = 0; g < n_groups; ++g) {
        if (h_n[g] < 0 || h_off[g] < 0) return SPKD_EINVAL;
        h_out[g] = count_detections(h_flags + h_off[g], h_n[g]);
    }
    return SPKD_OK;
}

spkd_status spkd_gw_lines(int64_t n_turns, const int64_t* h_off, const int32_t* h_n_det, const double* h_det_start,
                          const double* h_det_maxi, const double* h_final_start, const double* h_turn_start_s,
                          const double* h_turn_end_s, const int64_t* h_turn_begin, const int64_t* h_turn_end,
                          double rate, int text_contract, int64_t n_lines, double* h_times, int64_t* h_frame_b,
                          int64_t* h_frame_e, int64_t* h_index, int32_t* h_line_turn) {
    if (n_turns < 0 || n_lines < 0) return SPKD_EINVAL;
    if (n_turns > 0 && (!h_off || !h_n_det || !h_det_start || !h_det_maxi || !h_final_start || !h_turn_start_s ||
                        !h_turn_end_s || !h_turn_begin || !h_turn_end || !h_times))
        return SPKD_EINVAL;
    int64_t i = 0;
    for (int64_t t = 0; t < n_turns; ++t) {
        const int64_t nd = h_n_det[t];
        if (nd < 0 || i + nd + 1 > n_lines) return SPKD_EINVAL;
        const double ls = h_turn_start_s[t], le = h_turn_end_s[t];
        for (int64_t j = 0; j <= nd; ++j, ++i) {
            const RecipeLine L = recipe_line(h_turn_begin[t], h_turn_end[t] - h_turn_begin[t], h_off[t], j, nd,
                                             h_det_start, h_det_maxi, h_final_start + t, ls, le, rate);
            h_times[2 * i] = L.start_s;
            h_times[2 * i + 1] = L.end_s;
            if (h_frame_b) h_frame_b[i] = L.frame_b;
            if (h_frame_e) h_frame_e[i] = L.frame_e;
            if (h_index) h_index[i] = L.index;
            if (h_line_turn) h_line_turn[i] = (int32_t)t;
        }
    }
    if (i != n_lines) return SPKD_EINVAL;
    if (text_contract) spkd_py2_roundtrip(h_times, 2 * n_lines);
    return SPKD_OK;
}

// Exact Viterbi over a loop of one-state words (include/spkd.h).  Sums and comparisons only, in
// the order the header gives, so that a restatement in fp64 reproduces every bit.
spkd_status spkd_vad_viterbi(int64_t n_frames, int32_t n_states, const float* h_scores, int32_t n_words,
                             const int32_t* h_word_state, const double* h_stay, const double* h_exit,
                             const double* h_enter, int64_t* h_tok_frame, int32_t* h_tok_word, int64_t* h_n_tokens,
                             double* h_score) {
    if (!h_n_tokens || !h_score || n_frames < 0 || n_states < 1 || n_states > GM_MAX_S || n_words < 1 ||
        n_words > GM_MAX_S || !h_word_state || !h_stay || !h_exit || !h_enter)
        return SPKD_EINVAL;
    *h_n_tokens = 0;
    *h_score = -INFINITY;
    for (int32_t j = 0; j < n_words; ++j)
        if (h_word_state[j] < 0 || h_word_state[j] >= n_states) return SPKD_EINVAL;
    if (n_frames == 0) return SPKD_OK;
    if (!h_scores || !h_tok_frame || !h_tok_word) return SPKD_EINVAL;
    const int W = n_words;
    std::vector<int8_t> back((size_t)n_frames * W);     // -1: stayed in the word, i: entered from word i
    double d[GM_MAX_S], nd[GM_MAX_S], obs[GM_MAX_S];
    for (int64_t t = 0; t < n_frames; ++t) {
        bool all_ninf = true;
        for (int j = 0; j < W; ++j) {
            const double o = (double)h_scores[t * n_states + h_word_state[j]];
            obs[j] = std::isnan(o) ? -INFINITY : o;
            all_ninf = all_ninf && obs[j] == -INFINITY;
        }
        if (all_ninf)
            for (int j = 0; j < W; ++j) obs[j] = 0.0;
        if (t == 0) {
            for (int j = 0; j < W; ++j) { d[j] = h_enter[j] + obs[j]; back[(size_t)j] = -1; }
            continue;
        }
        double best = d[0] + h_exit[0];
        int bi = 0;
        for (int i = 1; i < W; ++i) {
            const double v = d[i] + h_exit[i];
            if (v > best) { best = v; bi = i; }
        }
        for (int j = 0; j < W; ++j) {
            const double stay = d[j] + h_stay[j], sw = best + h_enter[j];
            int8_t& b = back[(size_t)t * W + j];
            if (stay >= sw) { nd[j] = stay + obs[j]; b = -1; }
            else { nd[j] = sw + obs[j]; b = (int8_t)bi; }
        }
        for (int j = 0; j < W; ++j) d[j] = nd[j];
    }
    int j = 0;
    for (int i = 1; i < W; ++i)
        if (d[i] > d[j]) j = i;
    *h_score = d[j];
    // backtrack: a token at every frame where the path enters a word (and at frame 0)
    int64_t n = 0;
    for (int64_t t = n_frames - 1; t >= 0; --t) {
        const int8_t b = back[(size_t)t * W + j];
        if (t == 0 || b >= 0) { h_tok_frame[n] = t; h_tok_word[n] = j; ++n; }
        if (t > 0 && b >= 0) j = b;
    }
    std::reverse(h_tok_frame, h_tok_frame + n);
    std::reverse(h_tok_word, h_tok_word + n);
    *h_n_tokens = n;
    return SPKD_OK;
}

spkd_status spkd_labels_from_merges_batch(int64_t n_problems, const int64_t* h_seg_off, const int32_t* h_n_merges,
                                          const int32_t* h_a, const int32_t* h_b, int32_t* h_labels) {
    if (n_problems < 0 || (n_problems > 0 && (!h_seg_off || !h_n_merges || !h_a || !h_b || !h_labels)))
        return SPKD_EINVAL;
    std::atomic<int> bad{0};
    auto work = [&](int64_t lo, int64_t hi) {
        for (int64_t p = lo; p < hi; ++p) {
            const int64_t o = h_seg_off[p];
            if (spkd_labels_from_merges(h_seg_off[p + 1] - o, h_n_merges[p], h_a + o, h_b + o, h_labels + o) != SPKD_OK)
                bad.store(1);
        }
    };
    const int nthreads = (int)std::min<int64_t>(8, n_problems / 16);
    if (nthreads <= 1) {
        work(0, n_problems);
    } else {
        std::vector<std::thread> pool;
        const int64_t step = (n_problems + nthreads - 1) / nthreads;
        for (int t = 0; t < nthreads; ++t) {
            const int64_t lo = t * step, hi = std::min<int64_t>(n_problems, lo + step);
            if (lo < hi) pool.emplace_back(work, lo, hi);
        }
        for (auto& th : pool) th.join();
    }
    return bad.load() ? SPKD_EINVAL : SPKD_OK;
}

}  // extern "C"

#ifdef SPKD_PROFILE
// profiling builds only: phase clocks of k_gw since the last call (cycles summed over
// workgroups: prefix build, scan set-up, log-det jobs, finish + arg-max; scans; turns)
extern "C" int spkd_debug_ahc_prof(unsigned long long* out4) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyFromSymbol(out4, HIP_SYMBOL(spkd::g_ahc_prof), sizeof z) != hipSuccess) return 1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(spkd::g_ahc_prof), z, sizeof z) != hipSuccess) return 1;
    return 0;
}

// the wall clock at which the k_ahc workgroup of each of the first n_prob problems entered and left
// (out[2p], out[2p + 1]), and the clock's rate in kHz; zeroes the array
extern "C" int spkd_debug_ahc_span(unsigned long long* out, int n_prob, int* khz) {
    if (n_prob < 0 || n_prob > spkd::AHC_SPAN_PROBS) return 1;
    std::vector<unsigned long long> z(2 * (size_t)spkd::AHC_SPAN_PROBS, 0ull);
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(spkd::g_ahc_span), 2 * (size_t)n_prob * sizeof(unsigned long long)) != hipSuccess) return 1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(spkd::g_ahc_span), z.data(), z.size() * sizeof(unsigned long long)) != hipSuccess) return 1;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess) return 1;
    return 0;
}

extern "C" int spkd_debug_step_prof(unsigned long long* out8) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(spkd::g_step_prof), sizeof z) != hipSuccess) return 1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(spkd::g_step_prof), z, sizeof z) != hipSuccess) return 1;
    return 0;
}

extern "C" int spkd_debug_pass_prof(unsigned long long* out4) {
    unsigned long long z[4] = {0, 0, 0, 0};
    if (hipMemcpyFromSymbol(out4, HIP_SYMBOL(spkd::g_pass_prof), sizeof z) != hipSuccess) return 1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(spkd::g_pass_prof), z, sizeof z) != hipSuccess) return 1;
    return 0;
}

extern "C" int spkd_debug_gw_prof(unsigned long long* out12) {
    unsigned long long z[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyFromSymbol(out12, HIP_SYMBOL(spkd::g_gw_prof), sizeof z) != hipSuccess) return 1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(spkd::g_gw_prof), z, sizeof z) != hipSuccess) return 1;
    return 0;
}
#endif
