// The hand-off between change detection and clustering: the event slots k_gw leaves per turn
// become recipe lines, and the records behind the lines become the clustering working set.
// The two rules of a line (count_detections, recipe_line) are stated once, for the host walk
// (spkd_count_flags, spkd_gw_lines) and for the kernels alike.
#pragma once
#include "spkd_cd.hpp"
#include "spkd_cluster.hpp"
#include "spkd_device.hpp"

namespace spkd {

// detections of a turn = the ones among its first n_win window flags (what lies behind them in
// reused buffers is not looked at)
__host__ __device__ inline int32_t count_detections(const int32_t* flags, int64_t n_win) {
    int32_t cnt = 0;
    for (int64_t i = 0; i < n_win; ++i) cnt += flags[i] != 0;
    return cnt;
}

struct RecipeLine {
    double start_s, end_s;           // as the change-detection script computes them (before the text round trip)
    int64_t frame_b, frame_e;        // the absolute frames the line's fused record covers
    int64_t index;                   // its event slot = its record in the fused buffer
};

// Line j of a turn with nd detections, the turn being frames [begin, begin + len) with event
// slots from ev_off and VAD times [ls, le]: detection j covers [int(start), int(start + maxi))
// of the turn, the tail line (j == nd) runs from the final start to the turn's end.
// final_start: the turn's entry.  fp64, no contraction into FMAs: host and device round alike.
__host__ __device__ inline RecipeLine recipe_line(int64_t begin, int64_t len, int64_t ev_off, int64_t j, int64_t nd,
                                                  const double* det_start, const double* det_maxi,
                                                  const double* final_start, double ls, double le, double rate) {
#pragma clang fp contract(off)
    RecipeLine L;
    const bool tail = j == nd;
    double fs, fe;                   // the line's frame positions inside the turn
    if (tail) {
        fs = *final_start;
        L.start_s = fs / rate + ls;
        L.end_s = ((le - ls) * rate) / rate + ls;
        fe = 0.0;
    } else {
        fs = det_start[ev_off + j];
        fe = fs + det_maxi[ev_off + j];
        L.start_s = fs / rate + ls;
        L.end_s = fe / rate + ls;
    }
    L.frame_b = begin + (int64_t)fs;
    L.frame_e = tail ? begin + len : begin + (int64_t)fe;
    L.index = ev_off + j;
    return L;
}

// ---- the batch hand-off behind k_gw (spkd_gw_batch): event slots -> recipe lines, on the device.
// All three kernels return at once when the error word is set (a capacity overflow leaves
// counts that mean nothing); the host looks at the word before it uses anything.
constexpr int CP_TPB = 256;
constexpr int CP_SCAN_TPB = 1024;

// per launch position: the turn's detections, filed under the caller's turn index together with
// the position (k_cp_lines finds the turn by it)
__global__ __launch_bounds__(CP_TPB) void k_cp_count(const TurnDesc* __restrict__ turns, int64_t n_turns,
                                                     const int32_t* __restrict__ n_win,
                                                     const int32_t* __restrict__ win_det, const int* __restrict__ err,
                                                     int32_t* __restrict__ n_det, int32_t* __restrict__ pos) {
    if (*err) return;
    const int64_t p = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (p >= n_turns) return;
    const TurnDesc T = turns[p];
    int64_t nw = n_win[T.id];
    nw = nw < 0 ? 0 : (nw > T.ev_cap ? T.ev_cap : nw);
    n_det[T.id] = count_detections(win_det + T.ev_off, nw);
    pos[T.id] = (int32_t)p;
}

// exclusive scan of (detections + 1) over the turns in the caller's order -> first line of every
// turn, line_off[n_turns] = number of lines.  One workgroup: a run of turns per thread.
__global__ __launch_bounds__(CP_SCAN_TPB) void k_cp_scan(const int32_t* __restrict__ n_det, int64_t n_turns,
                                                         const int* __restrict__ err, int64_t* __restrict__ line_off) {
    __shared__ int64_t part[CP_SCAN_TPB];
    const int tid = threadIdx.x;
    if (*err) {
        if (tid == 0) line_off[n_turns] = 0;
        return;
    }
    const int64_t per = (n_turns + CP_SCAN_TPB - 1) / CP_SCAN_TPB;
    const int64_t lo = tid * per < n_turns ? tid * per : n_turns;
    const int64_t hi = lo + per < n_turns ? lo + per : n_turns;
    int64_t sum = 0;
    for (int64_t t = lo; t < hi; ++t) sum += (int64_t)n_det[t] + 1;
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < CP_SCAN_TPB; d <<= 1) {
        const int64_t v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int64_t run = part[tid] - sum;
    for (int64_t t = lo; t < hi; ++t) {
        line_off[t] = run;
        run += (int64_t)n_det[t] + 1;
    }
    if (tid == CP_SCAN_TPB - 1) line_off[n_turns] = part[tid];
}

// per turn (caller's order) its lines, from line_off[t] on
__global__ __launch_bounds__(CP_TPB) void k_cp_lines(const TurnDesc* __restrict__ turns, int64_t n_turns,
                                                     const int32_t* __restrict__ n_det, const int32_t* __restrict__ pos,
                                                     const int64_t* __restrict__ line_off, int64_t n_lines,
                                                     const double* __restrict__ det_start,
                                                     const double* __restrict__ det_maxi,
                                                     const double* __restrict__ final_start,
                                                     const double* __restrict__ turn_start_s,
                                                     const double* __restrict__ turn_end_s, double rate,
                                                     const int* __restrict__ err, double* __restrict__ times,
                                                     int64_t* __restrict__ frame_b, int64_t* __restrict__ frame_e,
                                                     int64_t* __restrict__ index, int32_t* __restrict__ line_turn) {
    if (*err) return;
    const int64_t t = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (t >= n_turns) return;
    const TurnDesc T = turns[pos[t]];
    const int64_t nd = n_det[t];
    const double ls = turn_start_s[t], le = turn_end_s[t];
    int64_t i = line_off[t];
    for (int64_t j = 0; j <= nd && i < n_lines; ++j, ++i) {
        const RecipeLine L = recipe_line(T.begin, T.len, T.ev_off, j, nd, det_start, det_maxi, final_start + t, ls, le, rate);
        times[2 * i] = L.start_s;
        times[2 * i + 1] = L.end_s;
        frame_b[i] = L.frame_b;
        frame_e[i] = L.frame_e;
        index[i] = L.index;
        line_turn[i] = (int32_t)t;
    }
}

// line -> source record of spkd_ahc_fused: -(k + 1) stands for record k of the redo buffer
__global__ __launch_bounds__(256) void k_patch_map(const int64_t* __restrict__ line, int64_t n, int64_t* __restrict__ map) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n) map[line[k]] = -(k + 1);
}

// k_to_quadrec reading every record through the line -> record map, and leaving the packed
// working copy beside the quad one: the record is fetched once, from where the detector (or
// the redo statistics) wrote it.  A map entry outside both buffers sets the capacity bit.
__global__ __launch_bounds__(256) void k_records_from_map(const double* __restrict__ recs, int64_t n_recs,
                                                          const int64_t* __restrict__ map,
                                                          const double* __restrict__ redo, int64_t n_redo,
                                                          int64_t n_rec, double* __restrict__ qr,
                                                          double* __restrict__ packed, int* __restrict__ err) {
    const int64_t c = blockIdx.x;
    if (c >= n_rec) return;
    const int64_t m = map[c];
    const double* g;
    if (m >= 0 && m < n_recs) {
        g = recs + m * REC;
    } else if (m < 0 && -(m + 1) < n_redo) {
        g = redo + (-(m + 1)) * REC;
    } else {
        if (threadIdx.x == 0) atomicOr(err, 4);
        return;
    }
    quadrec_from_packed(g, qr + c * QREC, threadIdx.x);
    double* p = packed + c * REC;
    for (int e = threadIdx.x; e < REC; e += 256) p[e] = g[e];
}

// records d_dst[dst[i]] = d_src[src[i]] (dst = NULL: i)
__global__ __launch_bounds__(256) void k_gather_records(const double* __restrict__ src, const int64_t* __restrict__ si,
                                                        const int64_t* __restrict__ di, int64_t n,
                                                        double* __restrict__ dst) {
    const int64_t i = blockIdx.x;
    if (i >= n) return;
    const double2* s = reinterpret_cast<const double2*>(src + si[i] * REC);
    double2* d = reinterpret_cast<double2*>(dst + (di ? di[i] : i) * REC);
    for (int e = threadIdx.x; e < REC / 2; e += 256) d[e] = s[e];
}

// D[0][1] of every 2-record problem of a batch of matrices (4 doubles each) -> out[p]
__global__ __launch_bounds__(256) void k_take_pair_distance(const double* __restrict__ mat, int64_t n, double* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n) out[p] = mat[4 * p + 1];
}

}  // namespace spkd
