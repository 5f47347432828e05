// range.hip -- exact range search over the (never written) similarity matrix: every document above a per-row bound, however
// many there are (faiss IndexFlatIP.range_search, which faiss runs on the CPU only).  What near-duplicate removal (all pairs
// with cosine > t), decontamination (any evaluation row within t) and per-row radius queries reduce to; top-k cannot answer
// them, because a cluster larger than k is cut off silently.
//
// Row m admits document n iff  s(m, n) > radius[m]  (strict, as faiss does for inner product)  and  n > min_id[m]
// (min_id == NULL: -1 everywhere; min_id[m] = the row's own corpus id makes a self-join return every unordered pair once).
// A NaN radius admits nothing, -inf admits every finite score.  s(m, n) has the bits cx_search_topk gives the pair
// (score_tile.h).  Two calls, so that the caller can read the total and refuse before anything of that size is allocated:
//   cx_range_count  1. range_count_kernel: (query tile x corpus split), rank.hip's walk with a cheaper predicate.  A lane keeps
//                      its four rows' radii and min_ids in registers over the split, compares its 16 scores of a row after
//                      every tile's K loop and keeps the counts in registers: one cross-lane reduction at the end and one
//                      plain store per (row, split, document half of the tile) into the workspace.  Per (query tile, corpus
//                      tile) every wave also stores one flag byte: did it see an admitted pair.  (One byte per wave, written
//                      with 0 or 1 by that wave alone: no two writers, nothing to clear beforehand.)
//                   2. range_sum_kernel: counts[m] = the sum of the row's 2 * nsplit partial counts.
//   cx_range_emit   range_emit_kernel: the same grid.  A workgroup's first output slot of a row is lims[m] + the partial counts
//                      of the splits before its own; it walks its split, SKIPS every tile whose four flag bytes are zero,
//                      recomputes a flagged tile, puts the fp32 scores in LDS (64 KiB operands + 64.5 KiB tile of gfx950's
//                      160 KiB) and one thread per row scans its 128 columns in order and appends (score, id): ascending ids
//                      within a row, since tiles, and splits, are walked in ascending order.  At product hit rates (1e-6 and
//                      below) almost no tile is flagged and the pass costs a sweep over the flags.
// What is skipped and why: corpus tiles whose last column is <= the smallest min_id of the query tile can admit nothing, so
// they are neither computed nor flagged; the splits of a query tile divide the REMAINING tiles, so a self-join's workgroups
// stay balanced while it does half the work.  Columns past N compare false.  Integer adds of per-split counts: the result
// depends on neither nsplit nor query batching nor scheduling; no atomics on global memory.
//
// cx_range_window_count / cx_range_window_emit are the same two kernels instantiated with WIN = true: row m also has an
// exclusive upper id, min_id[m] < n < end_id[m] (cluster-scoped self-joins over label-sorted rows: min_id = own position,
// end_id = the cluster's end).  A query tile walks corpus tiles [t0, t1) only -- t0 from the smallest min_id and t1 from the
// largest end_id among its rows with a non-empty window -- and its flags live at band_ptr[tm] in a workspace that holds one
// flag word per BAND tile (sum of t1 - t0), not per (query tile, corpus tile): M = N = millions of sorted rows fit one call.
// The walk is clamped to band_ptr[tm + 1] - band_ptr[tm] tiles and band_ptr to [0, band_tiles], so no window array can send a
// flag access outside the workspace.
#include <type_traits>
#include "cx_common.h"
#include "score_tile.h"
#include "../../include/contrastors_hip.h"

namespace {

constexpr int SROW = TN + 1;        // fp32 score tile row stride in floats: a row's thread walks its columns bank-conflict free
constexpr int FLAG_CHUNK = 256;     // flags fetched per sweep step of the emit pass: one per thread

struct RangeParams {
    const bf16_t* Q;
    const bf16_t* D;
    long ldq, ldd;
    int M, N, d;
    int nsplit, tiles_n;
    const float* radius;      // (M)
    const int64_t* min_id;    // (M) or NULL
    const int64_t* end_id;    // WIN: (M) or NULL (= N everywhere)
    const int64_t* band_ptr;  // WIN: (tiles_m + 1) first flag word of every query tile; band_tiles = flag words in the workspace
    long band_tiles;
    int* part;                // (M, nsplit, 2) partial counts (workspace; every slot is written)
    uint8_t* flags;           // (tiles_m, tiles_n, 4 waves), WIN: (band_tiles, 4 waves) (workspace; every slot of a walked tile is written)
    int64_t* counts;          // count
    const int64_t* lims;      // emit
    float* out_scores;
    int64_t* out_ids;
};

struct RowLds {
    float rad[TM];     // NaN past M: admits nothing
    int mid[TM];       // min_id clamped to [-1, N]
    int minmid, maxmid;
};

struct WinLds : RowLds {
    int end[TM];       // end_id clamped to [0, N]; rows with an empty window have a NaN radius and stay out of the four bounds
    int minend, maxend;
};

template <bool WIN> using Rows = typename std::conditional<WIN, WinLds, RowLds>::type;

// The tile rows' bounds into LDS and the query tile's walk [t_begin, t_end) for `split`: tiles below t0 = (minmid + 1) / TN end
// at a column <= every row's min_id.  The splits divide the tiles from t0 on.  Both passes call this with the same arguments.
// The flag word of corpus tile t is flags[fbase + t].
CX_DEVICE void row_bounds(const RangeParams& p, RowLds& R, int tm, int split, int tid, int& t_begin, int& t_end, int64_t& fbase) {
    const int m0 = tm * TM;
    if (tid == 0) { R.minmid = 0x7fffffff; R.maxmid = -1; }
    __syncthreads();
    if (tid < TM) {
        const int m = m0 + tid;
        float r = __builtin_nanf("");
        int id = -1;
        if (m < p.M) {
            r = p.radius[m];
            const int64_t v = p.min_id ? p.min_id[m] : (int64_t)-1;
            id = (int)min(max(v, (int64_t)-1), (int64_t)p.N);
            atomicMin(&R.minmid, id);   // (LDS)
            atomicMax(&R.maxmid, id);
        }
        R.rad[tid] = r;
        R.mid[tid] = id;
    }
    __syncthreads();
    const int t0 = min(p.tiles_n, (R.minmid + 1) / TN);
    const int tps = (p.tiles_n - t0 + p.nsplit - 1) / p.nsplit;
    t_begin = min(p.tiles_n, t0 + split * tps);
    t_end = min(p.tiles_n, t_begin + tps);
    fbase = (int64_t)tm * p.tiles_n;
}

// The windowed form: the walk is the band [t0, t1) of the rows whose window min_id < n < end_id is not empty, cut to the
// band_ptr[tm + 1] - band_ptr[tm] flag words the workspace holds for this query tile; the splits divide the band.
CX_DEVICE void row_bounds(const RangeParams& p, WinLds& R, int tm, int split, int tid, int& t_begin, int& t_end, int64_t& fbase) {
    const int m0 = tm * TM;
    if (tid == 0) { R.minmid = 0x7fffffff; R.maxmid = -1; R.minend = 0x7fffffff; R.maxend = 0; }
    __syncthreads();
    if (tid < TM) {
        const int m = m0 + tid;
        float r = __builtin_nanf("");
        int id = -1, e = 0;
        if (m < p.M) {
            const int64_t v = p.min_id ? p.min_id[m] : (int64_t)-1;
            const int64_t w = p.end_id ? p.end_id[m] : (int64_t)p.N;
            id = (int)min(max(v, (int64_t)-1), (int64_t)p.N);
            e = (int)min(max(w, (int64_t)0), (int64_t)p.N);
            if (e > id + 1) {
                r = p.radius[m];
                atomicMin(&R.minmid, id);   // (LDS)
                atomicMax(&R.maxmid, id);
                atomicMin(&R.minend, e);
                atomicMax(&R.maxend, e);
            }
        }
        R.rad[tid] = r;
        R.mid[tid] = id;
        R.end[tid] = e;
    }
    __syncthreads();
    const int64_t lo = min(max(p.band_ptr[tm], (int64_t)0), (int64_t)p.band_tiles);
    const int64_t cap = min(max(p.band_ptr[tm + 1], lo), (int64_t)p.band_tiles) - lo;
    int t0 = 0, t1 = 0;
    if (R.maxend > 0) {   // a non-empty row has mid + 1 < end <= N: t0 < t1 <= tiles_n
        t0 = (R.minmid + 1) / TN;
        t1 = (int)min((int64_t)(R.maxend + TN - 1) / TN, t0 + cap);
    }
    const int tps = (t1 - t0 + p.nsplit - 1) / p.nsplit;
    t_begin = min(t1, t0 + split * tps);
    t_end = min(t1, t_begin + tps);
    fbase = lo - t0;
}

template <bool WIN> struct CountLds {
    char ops[4 * PANEL];
    Rows<WIN> rows;
};

template <bool WIN> __global__ __launch_bounds__(256, 1) void range_count_kernel(RangeParams p) {
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    CountLds<WIN>& L = *reinterpret_cast<CountLds<WIN>*>(dsm);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wq = wave >> 1, wd = wave & 1, l15 = lane & 15, lh = lane >> 4;
    const int tm = blockIdx.x / p.nsplit, split = blockIdx.x % p.nsplit;
    const int m0 = tm * TM;
    int t_begin, t_end;
    int64_t fbase;
    row_bounds(p, L.rows, tm, split, tid, t_begin, t_end, fbase);
    const int maxmid = L.rows.maxmid;
    int minend = 0x7fffffff;
    float rad[4];
    int mid[4], end[4], cnt[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        rad[a] = L.rows.rad[wq * 64 + a * 16 + l15];
        mid[a] = L.rows.mid[wq * 64 + a * 16 + l15];
        cnt[a] = 0;
    }
    if constexpr (WIN) {
        minend = L.rows.minend;
#pragma unroll
        for (int a = 0; a < 4; ++a) end[a] = L.rows.end[wq * 64 + a * 16 + l15];
    }
    int64_t qo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qo[i] = (int64_t)min(m0 + (tid >> 3) + 32 * i, p.M - 1) * p.ldq;   // clamped rows have a NaN radius
    uint8_t* flags = p.flags + fbase * 4 + wave;
    for (int t = t_begin; t < t_end; ++t) {
        const int n0 = t * TN;
        int64_t d_o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) d_o[i] = (int64_t)min(n0 + (tid >> 3) + 32 * i, p.N - 1) * p.ldd;
        f32x4_t acc[4][4];
        tile_scores(p.Q, p.D, qo, d_o, p.d / BK, L.ops, tid, acc);
        // acc[a][b][r] = score(query m0 + wq*64 + a*16 + l15, document n0 + wd*64 + b*16 + 4*lh + r)
        const int nb = n0 + wd * 64 + 4 * lh;
        if (n0 + TN > p.N) {
            // the partial last tile: a column past N compares false with everything
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (nb + b * 16 + r >= p.N) acc[a][b][r] = __builtin_nanf("");
        }
        int hit = 0;
        if (n0 > maxmid && n0 + TN <= minend) {   // (uniform) every column of the tile is inside every row's id bounds: the score test alone
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                int c = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) c += acc[a][b][r] > rad[a] ? 1 : 0;
                cnt[a] += c;
                hit |= c;
            }
        } else {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int lim = mid[a] - nb;   // column nb + c is above the row's min_id  <=>  c > lim
                int c = 0;
                if constexpr (WIN) {
                    const int top = end[a] - nb;   // ... and below its end_id  <=>  c < top
#pragma unroll
                    for (int b = 0; b < 4; ++b)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            c += ((acc[a][b][r] > rad[a]) & (b * 16 + r > lim) & (b * 16 + r < top)) ? 1 : 0;
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b)
#pragma unroll
                        for (int r = 0; r < 4; ++r) c += ((acc[a][b][r] > rad[a]) & (b * 16 + r > lim)) ? 1 : 0;
                }
                cnt[a] += c;
                hit |= c;
            }
        }
        const int any = __any(hit);
        if (lane == 0) flags[(int64_t)t * 4] = any ? 1 : 0;
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int m = m0 + wq * 64 + a * 16 + l15;
        int c = cnt[a];
        c += __shfl_xor(c, 16, 64);
        c += __shfl_xor(c, 32, 64);
        if (lh == 0 && m < p.M) p.part[((int64_t)m * p.nsplit + split) * 2 + wd] = c;
    }
}

// one thread per query row
__global__ __launch_bounds__(256) void range_sum_kernel(const int* __restrict__ part, int M, int nsplit,
                                                        int64_t* __restrict__ counts) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    int64_t c = 0;
    for (int i = 0; i < 2 * nsplit; ++i) c += part[(int64_t)m * 2 * nsplit + i];
    counts[m] = c;
}

template <bool WIN> struct EmitLds {
    char ops[4 * PANEL];
    float tile[TM * SROW];
    Rows<WIN> rows;
    uint8_t live[FLAG_CHUNK];
};

template <bool WIN> __global__ __launch_bounds__(256, 1) void range_emit_kernel(RangeParams p) {
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    EmitLds<WIN>& L = *reinterpret_cast<EmitLds<WIN>*>(dsm);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wq = wave >> 1, wd = wave & 1, l15 = lane & 15, lh = lane >> 4;
    const int tm = blockIdx.x / p.nsplit, split = blockIdx.x % p.nsplit;
    const int m0 = tm * TM;
    int t_begin, t_end;
    int64_t fbase;
    row_bounds(p, L.rows, tm, split, tid, t_begin, t_end, fbase);
    // the scanning thread of row tid: its bounds and its next output slot
    const bool scans = tid < TM && m0 + tid < p.M;
    float my_rad = __builtin_nanf("");
    int my_mid = -1, my_end = p.N;   // columns past N are not looked at
    int64_t off = 0;
    if (scans) {
        my_rad = L.rows.rad[tid];
        my_mid = L.rows.mid[tid];
        if constexpr (WIN) my_end = L.rows.end[tid];
        off = p.lims[m0 + tid];
        const int* pr = p.part + (int64_t)(m0 + tid) * p.nsplit * 2;
        for (int i = 0; i < 2 * split; ++i) off += pr[i];
    }
    int64_t qo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qo[i] = (int64_t)min(m0 + (tid >> 3) + 32 * i, p.M - 1) * p.ldq;
    const uint32_t* flags = reinterpret_cast<const uint32_t*>(p.flags) + fbase;
    for (int c0 = t_begin; c0 < t_end; c0 += FLAG_CHUNK) {
        __syncthreads();   // the previous chunk's L.live has been read
        L.live[tid] = (c0 + tid < t_end && flags[c0 + tid] != 0) ? 1 : 0;
        __syncthreads();
        const int c1 = min(t_end, c0 + FLAG_CHUNK);
        for (int t = c0; t < c1; ++t) {
            if (!L.live[t - c0]) continue;   // (uniform) no admitted pair in this tile: not recomputed
            const int n0 = t * TN;
            int64_t d_o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) d_o[i] = (int64_t)min(n0 + (tid >> 3) + 32 * i, p.N - 1) * p.ldd;
            f32x4_t acc[4][4];
            tile_scores(p.Q, p.D, qo, d_o, p.d / BK, L.ops, tid, acc);   // (its barriers stand between the previous scan and the writes below)
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        L.tile[(wq * 64 + a * 16 + l15) * SROW + wd * 64 + b * 16 + 4 * lh + r] = acc[a][b][r];
            __syncthreads();
            if (scans) {
                const float* row = L.tile + tid * SROW;
                const int ncol = min(TN, my_end - n0);
                for (int c = max(0, my_mid + 1 - n0); c < ncol; ++c) {
                    const float v = row[c];
                    if (v > my_rad) {
                        p.out_scores[off] = v;
                        p.out_ids[off] = n0 + c;
                        ++off;
                    }
                }
            }
        }
    }
}

// nsplit: already resolved (auto_splits / window_splits)
int fill(RangeParams& p, const uint16_t* Q, const uint16_t* D, int M, long N, int d, long ldq, long ldd, const float* radius,
         const int64_t* min_id, int nsplit, void* ws) {
    p.Q = Q; p.D = D; p.ldq = ldq; p.ldd = ldd;
    p.M = M; p.N = (int)N; p.d = d;
    p.nsplit = nsplit;
    p.tiles_n = (int)((N + TN - 1) / TN);
    p.radius = radius; p.min_id = min_id;
    p.part = reinterpret_cast<int*>(ws);
    const long part_bytes = ((long)M * p.nsplit * 2 * (long)sizeof(int) + 15) & ~15L;
    p.flags = reinterpret_cast<uint8_t*>(ws) + part_bytes;
    return (M + TM - 1) / TM;
}

// splits of a query tile's band: enough workgroups to fill the chip, at most one per tile of the mean band (thousands of query
// tiles: 1)
int window_splits(int M, long band_tiles, int nsplit) {
    const int tiles_m = (M + TM - 1) / TM;
    if (nsplit <= 0) nsplit = (SPLIT_TARGET_WG + tiles_m - 1) / tiles_m;
    nsplit = min(nsplit, MAXSPLIT);
    return (int)max(1L, min((long)nsplit, (band_tiles + tiles_m - 1) / tiles_m));
}

int check_args(const void* Q, const void* D, int M, long N, int d, long ldq, long ldd, const void* radius, const void* ws) {
    if (M < 0 || N < 0 || d < 64 || d > 1024 || (d % 64) != 0 || N > MAX_N) return CX_ERR_SHAPE;
    if (M == 0 || N == 0) return CX_OK;
    if (!Q || !D || !radius || !ws) return CX_ERR_ARG;
    if (ldq < d || (ldq % 8) != 0 || ldd < d || (ldd % 8) != 0) return CX_ERR_ALIGN;
    if (((uintptr_t)Q & 15) || ((uintptr_t)D & 15) || ((uintptr_t)ws & 15)) return CX_ERR_ALIGN;
    return CX_OK;
}

}  // namespace

extern "C" {

long cx_range_ws_bytes(int M, long N, int nsplit) {
    if (M <= 0 || N <= 0) return 0;
    const long tiles_m = (M + TM - 1) / TM, tiles_n = (N + TN - 1) / TN;
    const long part_bytes = ((long)M * auto_splits(M, N, nsplit) * 2 * (long)sizeof(int) + 15) & ~15L;
    return part_bytes + tiles_m * tiles_n * 4 + 16;   // partial counts + one flag byte per (query tile, corpus tile, wave)
}

int cx_range_count(const uint16_t* Q, const uint16_t* D, int M, long N, int d, long ldq, long ldd, const float* radius,
                   const int64_t* min_id, int nsplit, void* ws, int64_t* counts, void* stream) {
    const int rc = check_args(Q, D, M, N, d, ldq, ldd, radius, ws);
    if (rc != CX_OK || M == 0 || N == 0) return rc;
    if (!counts) return CX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    RangeParams p = {};
    const int tiles_m = fill(p, Q, D, M, N, d, ldq, ldd, radius, min_id, auto_splits(M, N, nsplit), ws);
    p.counts = counts;
    static CxLdsOptIn opt;
    if (!opt.ensure(reinterpret_cast<const void*>(&range_count_kernel<false>), (int)sizeof(CountLds<false>))) return CX_ERR_LAUNCH;
    hipLaunchKernelGGL(range_count_kernel<false>, dim3(tiles_m * p.nsplit), dim3(256), sizeof(CountLds<false>), s, p);
    if (hipGetLastError() != hipSuccess) return CX_ERR_LAUNCH;
    hipLaunchKernelGGL(range_sum_kernel, dim3((M + 255) / 256), dim3(256), 0, s, p.part, M, p.nsplit, counts);
    return done();
}

int cx_range_emit(const uint16_t* Q, const uint16_t* D, int M, long N, int d, long ldq, long ldd, const float* radius,
                  const int64_t* min_id, int nsplit, const void* ws, const int64_t* lims, float* out_scores, int64_t* out_ids,
                  void* stream) {
    const int rc = check_args(Q, D, M, N, d, ldq, ldd, radius, ws);
    if (rc != CX_OK || M == 0 || N == 0) return rc;
    if (!lims || !out_scores || !out_ids) return CX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    RangeParams p = {};
    const int tiles_m = fill(p, Q, D, M, N, d, ldq, ldd, radius, min_id, auto_splits(M, N, nsplit), const_cast<void*>(ws));
    p.lims = lims; p.out_scores = out_scores; p.out_ids = out_ids;
    static CxLdsOptIn opt;
    if (!opt.ensure(reinterpret_cast<const void*>(&range_emit_kernel<false>), (int)sizeof(EmitLds<false>))) return CX_ERR_LAUNCH;
    hipLaunchKernelGGL(range_emit_kernel<false>, dim3(tiles_m * p.nsplit), dim3(256), sizeof(EmitLds<false>), s, p);
    return done();
}

long cx_range_window_ws_bytes(int M, long N, long band_tiles, int nsplit) {
    if (M <= 0 || N <= 0) return 0;
    band_tiles = max(band_tiles, 0L);
    const long part_bytes = ((long)M * window_splits(M, band_tiles, nsplit) * 2 * (long)sizeof(int) + 15) & ~15L;
    return part_bytes + band_tiles * 4 + 16;   // partial counts + one flag byte per (band tile, wave)
}

int cx_range_window_count(const uint16_t* Q, const uint16_t* D, int M, long N, int d, long ldq, long ldd, const float* radius,
                          const int64_t* min_id, const int64_t* end_id, const int64_t* band_ptr, long band_tiles, int nsplit,
                          void* ws, int64_t* counts, void* stream) {
    const int rc = check_args(Q, D, M, N, d, ldq, ldd, radius, ws);
    if (rc != CX_OK || M == 0 || N == 0) return rc;
    if (!counts || !band_ptr || band_tiles < 0) return CX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    RangeParams p = {};
    const int tiles_m = fill(p, Q, D, M, N, d, ldq, ldd, radius, min_id, window_splits(M, band_tiles, nsplit), ws);
    p.end_id = end_id; p.band_ptr = band_ptr; p.band_tiles = band_tiles;
    p.counts = counts;
    static CxLdsOptIn opt;
    if (!opt.ensure(reinterpret_cast<const void*>(&range_count_kernel<true>), (int)sizeof(CountLds<true>))) return CX_ERR_LAUNCH;
    hipLaunchKernelGGL(range_count_kernel<true>, dim3(tiles_m * p.nsplit), dim3(256), sizeof(CountLds<true>), s, p);
    if (hipGetLastError() != hipSuccess) return CX_ERR_LAUNCH;
    hipLaunchKernelGGL(range_sum_kernel, dim3((M + 255) / 256), dim3(256), 0, s, p.part, M, p.nsplit, counts);
    return done();
}

int cx_range_window_emit(const uint16_t* Q, const uint16_t* D, int M, long N, int d, long ldq, long ldd, const float* radius,
                         const int64_t* min_id, const int64_t* end_id, const int64_t* band_ptr, long band_tiles, int nsplit,
                         const void* ws, const int64_t* lims, float* out_scores, int64_t* out_ids, void* stream) {
    const int rc = check_args(Q, D, M, N, d, ldq, ldd, radius, ws);
    if (rc != CX_OK || M == 0 || N == 0) return rc;
    if (!lims || !out_scores || !out_ids || !band_ptr || band_tiles < 0) return CX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    RangeParams p = {};
    const int tiles_m = fill(p, Q, D, M, N, d, ldq, ldd, radius, min_id, window_splits(M, band_tiles, nsplit),
                             const_cast<void*>(ws));
    p.end_id = end_id; p.band_ptr = band_ptr; p.band_tiles = band_tiles;
    p.lims = lims; p.out_scores = out_scores; p.out_ids = out_ids;
    static CxLdsOptIn opt;
    if (!opt.ensure(reinterpret_cast<const void*>(&range_emit_kernel<true>), (int)sizeof(EmitLds<true>))) return CX_ERR_LAUNCH;
    hipLaunchKernelGGL(range_emit_kernel<true>, dim3(tiles_m * p.nsplit), dim3(256), sizeof(EmitLds<true>), s, p);
    return done();
}

}  // extern "C"
