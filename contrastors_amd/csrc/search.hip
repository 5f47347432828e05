// search.hip -- exact inner-product top-k search (faiss IndexFlatIP.search) for the data-curation stage: consistency
// filtering (scripts/text/index_filtering.py:363-391) and hard-negative mining (scripts/text/get_negatives.py:111-196,
// scripts/text/mine_beir_negatives_full.py:98-136).  The (M x N) score matrix is never written.
//
// Stage 1 (search_tiles_kernel): a workgroup owns one 128-query tile and walks a contiguous range of 128-document tiles
// (its "split" of the corpus).  Scores are bf16 x bf16 -> fp32 on v_mfma_f32_16x16x32_bf16, issued as (A := document rows,
// B := query rows) so that a lane owns one query per 16-block.  Each query row keeps a sorted running top-k list of its
// split in the workspace and its current k-th best score in LDS; the epilogue compares every score with that threshold in
// registers and only rows with a score above it (and below the row's bound) go through the insert path, which gathers the
// tile's admissible candidates, drops the row's excluded ids, ranks them and merges them into the list by rank counting.
// Stage 2 (merge_splits_kernel): per row, every list entry's final rank = its rank in its own list + the number of entries
// of the other lists that beat it (binary search); ranks are unique, so the merge is a scatter with no atomics.
//
// Order: descending score, ties to the lower id -- a strict total order on (score, id).  Every score has ONE instruction
// sequence (the same K order whatever tile or split it falls in), so the result is the unique top-k of that order and is
// bit-identical for any split count.  Rows with fewer than k admissible documents are padded with (-inf, -1).
//
// cx_search_window_topk is stage 1 instantiated with WIN = true: row m also has an id window min_id[m] < n < end_id[m]
// (range.hip's convention), kept in LDS next to thr / bel and tested wherever a column is tested against N.  A query tile walks
// the corpus tiles [t0, t1) only -- t0 from the smallest min_id and t1 from the largest end_id among its rows with a non-empty
// window -- in one piece (nsplit = 1: the band is short, and ids still grow along the walk).  What an IVF index needs: rows
// sorted by list, (query, probed list) pairs sorted by list, so that a 128-pair tile walks a short run of consecutive lists.
// cx_topk_merge_lists is stage 2 behind an indirection: the lists of an output row are named by src and live in (P, k) score /
// id arrays as the search entry points write them; ids may be mapped on the way out (list positions -> original ids).
//
// cx_search_int8_topk is stage 1 over int8 codes with one fp32 scale per row (search_int8_tiles_kernel, below the bf16 kernel):
// its own operand staging, K loop (v_mfma_i32_16x16x64_i8) and scaling epilogue; Cand, SearchLds, insert_row<WIN>,
// merge_lists_kernel<SplitLists> and auto_splits are shared as they are.  cx_search_int8_window_topk is that kernel with
// WIN = true, the way cx_search_window_topk is search_tiles_kernel<true>: the scan of an IVF index over int8 codes.
//
// cx_search_pq_topk is stage 1 over product-quantiser codes (search_pq_tiles_kernel, below the int8 kernel): the bf16 kernel
// with the document panel gathered from a codebook by the tile's code bytes; everything else is shared as it is.
#include <type_traits>
#include "cx_common.h"
#include "../../include/contrastors_hip.h"

namespace {

constexpr int TM = 128, TN = 128, BK = 64;
constexpr int PANEL = TM * BK * 2;   // 16 KiB: one operand's 64-wide K chunk, 128 rows x 128 B
constexpr int MAXK = 1024;
constexpr int MAXSPLIT = 64;
// column indices are int: the last tile's columns reach N + TN - 2, which must not overflow
constexpr long MAX_N = 0x7fffffffL - TN;
constexpr int SPLIT_TARGET_WG = 512; // auto split: (M-tile, split) workgroups for two waves of the 256 CUs

struct Cand {
    float s;
    int id;
};

CX_DEVICE bool beats(Cand a, Cand b) { return a.s > b.s || (a.s == b.s && a.id < b.id); }

// [128 rows][8 chunks of 16 B]: chunk c of row r at r*128 + ((c ^ (r & 7)) << 4)
CX_DEVICE int poff(int r, int c) { return r * 128 + ((c ^ (r & 7)) << 4); }

// LDS writes / global stores of this wave are complete and visible to the wave's later reads (no compiler reordering)
CX_DEVICE void wave_sync() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

struct SearchParams {
    const bf16_t* Q;
    const bf16_t* D;
    long ldq, ldd;
    int M, N, d, k;
    int nsplit, tiles_n, tiles_per_split;
    const int64_t* xptr;   // (M + 1) CSR row pointers into xids (absolute), or null
    const int64_t* xids;
    const float* below;    // (M) exclusive upper bound on the score, or null
    const int64_t* min_id; // WIN: (M) exclusive lower id bound, or null (= -1 everywhere)
    const int64_t* end_id; // WIN: (M) exclusive upper id bound, or null (= N everywhere)
    Cand* lists;           // (M, nsplit, k)
    int* counts;           // (M, nsplit)
};

CX_DEVICE void stage(const SearchParams& p, int m0, int n0, int k0, int tid, uint4 (&sq)[4], uint4 (&sd)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int item = tid + 256 * i, r = item >> 3, c = item & 7;
        const int gm = min(m0 + r, p.M - 1), gn = min(n0 + r, p.N - 1);   // clamped rows are read but never admitted
        sq[i] = *reinterpret_cast<const uint4*>(p.Q + (int64_t)gm * p.ldq + k0 + c * 8);
        sd[i] = *reinterpret_cast<const uint4*>(p.D + (int64_t)gn * p.ldd + k0 + c * 8);
    }
}
CX_DEVICE void commit(char* qbuf, char* dbuf, int tid, const uint4 (&sq)[4], const uint4 (&sd)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int item = tid + 256 * i, r = item >> 3, c = item & 7;
        *reinterpret_cast<uint4*>(qbuf + poff(r, c)) = sq[i];
        *reinterpret_cast<uint4*>(dbuf + poff(r, c)) = sd[i];
    }
}

// number of entries of the sorted list L[0 .. n) that beat e
CX_DEVICE int count_beating(const Cand* L, int n, Cand e) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (beats(L[mid], e)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct SearchLds {
    char ops[4 * PANEL];          // [Q, D] x 2 K-chunk buffers; after the K loop: the 128 x 128 fp32 score tile
    Cand mbuf[4][MAXK];           // per wave: the merged list being built
    Cand cand[4][TN];             // per wave: the tile's admissible candidates of one row, in column order
    Cand sorted[4][TN];           // ... and ranked
    float thr[TM], bel[TM];
    int cnt[TM], flag[TM];
    int any;
};

struct WinSearchLds : SearchLds {
    int mid[TM], end[TM];         // min_id clamped to [-1, N], end_id clamped to [0, N]
    int minmid, maxend;           // over the tile's rows with a non-empty window
};

template <bool WIN> using SearchLdsT = typename std::conditional<WIN, WinSearchLds, SearchLds>::type;

// one wave: insert the admissible scores of tile row `row` (scores in `tile`) into the row's running list
template <bool WIN>
CX_DEVICE void insert_row(const SearchParams& p, SearchLdsT<WIN>& L, const float* tile, int row, int m, int n0, int split,
                          int wave, int lane) {
    const float thr = L.thr[row], bel = L.bel[row];
    const int cnt = L.cnt[row];
    const int64_t x0 = p.xptr ? p.xptr[m] : 0, x1 = p.xptr ? p.xptr[m + 1] : 0;
    Cand* cand = L.cand[wave];
    Cand* srt = L.sorted[wave];
    Cand* mb = L.mbuf[wave];
    int c = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h, n = n0 + j;
        const float s = tile[row * TN + j];
        bool ok = n < p.N && s > thr && s < bel;
        if constexpr (WIN) ok = ok && n > L.mid[row] && n < L.end[row];
        if (ok)
            for (int64_t e = x0; e < x1; ++e)
                if (p.xids[e] == n) ok = false;
        const unsigned long long mask = __ballot(ok);
        const int pos = c + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
        if (ok) cand[pos] = Cand{s, n};
        c += __popcll(mask);
    }
    if (c == 0) return;
    wave_sync();
    for (int i = lane; i < c; i += 64) {
        const Cand e = cand[i];
        int r = 0;
        for (int j = 0; j < c; ++j) r += beats(cand[j], e) ? 1 : 0;
        srt[r] = e;
    }
    wave_sync();
    Cand* list = p.lists + ((int64_t)m * p.nsplit + split) * p.k;
    for (int j = lane; j < cnt; j += 64) {
        const Cand e = list[j];
        const int pos = j + count_beating(srt, c, e);
        if (pos < p.k) mb[pos] = e;
    }
    for (int i = lane; i < c; i += 64) {
        const Cand e = srt[i];
        const int pos = i + count_beating(list, cnt, e);
        if (pos < p.k) mb[pos] = e;
    }
    wave_sync();
    const int ncnt = min(p.k, cnt + c);
    for (int j = lane; j < ncnt; j += 64) list[j] = mb[j];
    if (lane == 0) {
        L.cnt[row] = ncnt;
        // full list: a later score can only enter above the k-th (an equal score has a larger id: ids grow along the split)
        if (ncnt == p.k) L.thr[row] = mb[p.k - 1].s;
    }
    wave_sync();
}

// Every row's threshold, bound, count and flag and, with WIN, its clamped window; t_begin / t_end become the band [t0, t1) of
// the tile's non-empty windows (WIN = false: the split's range stays).  Ends behind a workgroup barrier.
template <bool WIN>
CX_DEVICE void init_rows(const SearchParams& p, SearchLdsT<WIN>& L, int m0, int tid, int& t_begin, int& t_end) {
    if constexpr (WIN) {
        if (tid == 0) { L.minmid = 0x7fffffff; L.maxend = 0; }
        __syncthreads();
    }
    if (tid < TM) {
        const int m = m0 + tid;
        // rows past M never pass the threshold test
        bool live = m < p.M;
        if constexpr (WIN) {
            int id = -1, e = 0;
            if (live) {
                const int64_t v = p.min_id ? p.min_id[m] : (int64_t)-1;
                const int64_t w = p.end_id ? p.end_id[m] : (int64_t)p.N;
                id = (int)min(max(v, (int64_t)-1), (int64_t)p.N);
                e = (int)min(max(w, (int64_t)0), (int64_t)p.N);
                live = e > id + 1;   // ... nor do rows with an empty window, which stay out of the walk's bounds
                if (live) {
                    atomicMin(&L.minmid, id);   // (LDS)
                    atomicMax(&L.maxend, e);
                }
            }
            L.mid[tid] = id;
            L.end[tid] = e;
        }
        L.thr[tid] = live ? -INFINITY : INFINITY;
        L.bel[tid] = (m < p.M && p.below) ? p.below[m] : INFINITY;
        L.cnt[tid] = 0;
        L.flag[tid] = 0;
    }
    if (tid == 0) L.any = 0;
    __syncthreads();
    if constexpr (WIN) {
        // a non-empty row has mid + 1 < end <= N: t_begin < t_end <= tiles_n; a tile of empty windows walks nothing
        t_begin = L.maxend > 0 ? (L.minmid + 1) / TN : 0;
        t_end = L.maxend > 0 ? (L.maxend + TN - 1) / TN : 0;
    }
}

// What fills the staging registers of the bf16 tile walk below.  RowStage: both panels from bf16 rows (stage).
struct RowStage {
    CX_DEVICE void begin_tile(const SearchParams&, int, int) const {}
    CX_DEVICE void operator()(const SearchParams& p, int m0, int n0, int k0, int tid, uint4 (&sq)[4], uint4 (&sd)[4]) const {
        stage(p, m0, n0, k0, tid, sq, sd);
    }
};

// The walk of one (query tile, split) workgroup over its corpus tiles: the body of search_tiles_kernel<WIN> and of
// search_pq_tiles_kernel, which differ in the stager only -- the K loop's MFMA order, the epilogue and the insert path are one
// piece of code, so a score has the same bits whichever way its document panel was filled.
template <bool WIN, class Params, class Lds, class Stager>
CX_DEVICE void search_tiles_walk(const Params& p, Lds& L, const Stager& stager) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wq = wave >> 1, wd = wave & 1, l15 = lane & 15, lh = lane >> 4;
    const int tm = blockIdx.x / p.nsplit, split = blockIdx.x % p.nsplit;
    const int m0 = tm * TM;
    int t_begin = split * p.tiles_per_split, t_end = min(p.tiles_n, t_begin + p.tiles_per_split);
    const int nk = p.d / BK;

    init_rows<WIN>(p, L, m0, tid, t_begin, t_end);

    for (int t = t_begin; t < t_end; ++t) {
        const int n0 = t * TN;
        stager.begin_tile(p, n0, tid);
        f32x4_t acc[4][4];   // [query block qb][document block db]
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        uint4 sq[4], sd[4];
        stager(p, m0, n0, 0, tid, sq, sd);
        commit(L.ops, L.ops + PANEL, tid, sq, sd);
        __syncthreads();
        for (int kc = 0; kc < nk; ++kc) {
            const char* qb_ = L.ops + (kc & 1) * 2 * PANEL;
            const char* db_ = qb_ + PANEL;
            // the last chunk is staged twice (unconditional, so the staging registers never leave the register file)
            stager(p, m0, n0, min(kc + 1, nk - 1) * BK, tid, sq, sd);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8_t fq[4], fd[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    fq[b] = *reinterpret_cast<const bf16x8_t*>(qb_ + poff(wq * 64 + b * 16 + l15, ks * 4 + lh));
                    fd[b] = *reinterpret_cast<const bf16x8_t*>(db_ + poff(wd * 64 + b * 16 + l15, ks * 4 + lh));
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fd[b], fq[a], acc[a][b], 0, 0, 0);
            }
            char* nq = L.ops + ((kc + 1) & 1) * 2 * PANEL;   // read last in chunk kc - 1, behind the barrier below
            commit(nq, nq + PANEL, tid, sq, sd);
            __syncthreads();
        }

        // acc[a][b][r] = score(query m0 + wq*64 + a*16 + l15, document n0 + wd*64 + b*16 + 4*lh + r)
        bool hit = false;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int row = wq * 64 + a * 16 + l15;
            const float thr = L.thr[row], bel = L.bel[row];
            bool h = false;
            if constexpr (WIN) {
                const int nb = n0 + wd * 64 + 4 * lh;
                const int lim = L.mid[row] - nb, top = L.end[row] - nb;   // column nb + c is inside the window  <=>  lim < c < top
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = acc[a][b][r];
                        h |= (v > thr) & (v < bel) & (b * 16 + r > lim) & (b * 16 + r < top);   // (end <= N)
                    }
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = acc[a][b][r];
                        h |= (v > thr) & (v < bel) & (n0 + wd * 64 + b * 16 + 4 * lh + r < p.N);
                    }
            }
            if (h) L.flag[row] = 1;
            hit |= h;
        }
        if (hit) L.any = 1;
        __syncthreads();
        if (L.any) {
            float* tile = reinterpret_cast<float*>(L.ops);   // the operand buffers are free until the next tile
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    *reinterpret_cast<f32x4_t*>(tile + (wq * 64 + a * 16 + l15) * TN + wd * 64 + b * 16 + 4 * lh) = acc[a][b];
            __syncthreads();
            for (int row = wave; row < TM; row += 4)
                if (L.flag[row]) insert_row<WIN>(p, L, tile, row, m0 + row, n0, split, wave, lane);
            __syncthreads();
            if (tid < TM) L.flag[tid] = 0;
            if (tid == 0) L.any = 0;
        }
        __syncthreads();
    }
    if (tid < TM && m0 + tid < p.M) p.counts[(int64_t)(m0 + tid) * p.nsplit + split] = L.cnt[tid];
}

template <bool WIN> __global__ __launch_bounds__(256, 1) void search_tiles_kernel(SearchParams p) {
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    search_tiles_walk<WIN>(p, *reinterpret_cast<SearchLdsT<WIN>*>(dsm), RowStage{});
}

// ---- int8 scalar-quantised rows (cx_search_int8_topk) -----------------------------------------------------------------
// Stage 1 over int8 codes with one fp32 scale per row: acc = sum_j Q[m][j] D[n][j] on v_mfma_i32_16x16x64_i8 (exact in int32;
// |acc| <= 127^2 * 1024 < 2^24, so (float)acc is exact too) and s = ((float)acc * d_scale[n]) * q_scale[m], two fp32
// multiplications in that order.  The operands are issued as in search_tiles_kernel (A := document rows, B := query rows), so
// the accumulator layout, the threshold test, the fp32 tile in LDS, insert_row<false> and the split merge are that kernel's.
// A K chunk is 128 bytes per row = 128 K elements in the same poff swizzle; the 16 bytes a lane feeds to one MFMA are the same
// K positions for both operands, which is all an integer dot product needs.  d % 128 == 64: the last chunk is half used; its
// upper half is staged from the lower half's addresses (never past the row) and the K loop does not read it.
typedef __attribute__((ext_vector_type(4))) int i32x4_t;
constexpr int BK8 = 128;             // int8 K elements (= bytes) per row of a panel: PANEL = TM * BK8 as well

struct Int8Params : SearchParams {   // (Q, D of the base stay null; ldq / ldd count bytes)
    const int8_t* Q8;
    const int8_t* D8;
    const float* q_scale;  // (M)
    const float* d_scale;  // (N)
};

template <bool WIN> struct Int8SearchLds : SearchLdsT<WIN> {
    alignas(16) float dsc[TN];    // the scales of the current corpus tile's rows (read four at a time)
    float qsc[TM];                // ... and of the query tile's rows
};

CX_DEVICE void stage8(const Int8Params& p, int m0, int n0, int k0, int tid, uint4 (&sq)[4], uint4 (&sd)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int item = tid + 256 * i, r = item >> 3, c = item & 7;
        const int gm = min(m0 + r, p.M - 1), gn = min(n0 + r, p.N - 1);   // clamped rows are read but never admitted
        int kb = k0 + c * 16;
        if (kb >= p.d) kb -= 64;   // the unused half of the last chunk: any bytes of the row
        sq[i] = *reinterpret_cast<const uint4*>(p.Q8 + (int64_t)gm * p.ldq + kb);
        sd[i] = *reinterpret_cast<const uint4*>(p.D8 + (int64_t)gn * p.ldd + kb);
    }
}

// WIN = true: the id window of search_tiles_kernel<true>, tested in the same places, and the same band walk [t0, t1) in one
// piece; dsc is loaded from the scales of corpus tile t itself, wherever the band starts.
template <bool WIN> __global__ __launch_bounds__(256, 1) void search_int8_tiles_kernel(Int8Params p) {
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    Int8SearchLds<WIN>& L = *reinterpret_cast<Int8SearchLds<WIN>*>(dsm);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wq = wave >> 1, wd = wave & 1, l15 = lane & 15, lh = lane >> 4;
    const int tm = blockIdx.x / p.nsplit, split = blockIdx.x % p.nsplit;
    const int m0 = tm * TM;
    int t_begin = split * p.tiles_per_split, t_end = min(p.tiles_n, t_begin + p.tiles_per_split);
    const int nk = (p.d + BK8 - 1) / BK8;

    if (tid < TM) L.qsc[tid] = p.q_scale[min(m0 + tid, p.M - 1)];   // (read in the epilogue, behind init_rows' barrier)
    init_rows<WIN>(p, L, m0, tid, t_begin, t_end);

    for (int t = t_begin; t < t_end; ++t) {
        const int n0 = t * TN;
        if (tid < TN) L.dsc[tid] = p.d_scale[min(n0 + tid, p.N - 1)];   // read in the epilogue, behind the K loop's barriers
        i32x4_t acc[4][4];   // [query block qb][document block db]
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = i32x4_t{0, 0, 0, 0};
        uint4 sq[4], sd[4];
        stage8(p, m0, n0, 0, tid, sq, sd);
        commit(L.ops, L.ops + PANEL, tid, sq, sd);
        __syncthreads();
        for (int kc = 0; kc < nk; ++kc) {
            const char* qb_ = L.ops + (kc & 1) * 2 * PANEL;
            const char* db_ = qb_ + PANEL;
            stage8(p, m0, n0, min(kc + 1, nk - 1) * BK8, tid, sq, sd);   // the last chunk is staged twice (unconditional)
            const int nks = (p.d - kc * BK8) > 64 ? 2 : 1;
            for (int ks = 0; ks < nks; ++ks) {
                i32x4_t fq[4], fd[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    fq[b] = *reinterpret_cast<const i32x4_t*>(qb_ + poff(wq * 64 + b * 16 + l15, ks * 4 + lh));
                    fd[b] = *reinterpret_cast<const i32x4_t*>(db_ + poff(wd * 64 + b * 16 + l15, ks * 4 + lh));
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fd[b], fq[a], acc[a][b], 0, 0, 0);
            }
            char* nq = L.ops + ((kc + 1) & 1) * 2 * PANEL;
            commit(nq, nq + PANEL, tid, sq, sd);
            __syncthreads();
        }

        // acc[a][b][r] = the integer dot product of (query m0 + wq*64 + a*16 + l15, document n0 + wd*64 + b*16 + 4*lh + r)
        f32x4_t sc[4][4];
        bool hit = false;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int row = wq * 64 + a * 16 + l15;
            const float thr = L.thr[row], bel = L.bel[row], qs = L.qsc[row];
            bool h = false;
            int lim = 0, top = 0;   // WIN: column nb + c is inside the window  <=>  lim < c < top
            if constexpr (WIN) {
                const int nb = n0 + wd * 64 + 4 * lh;
                lim = L.mid[row] - nb;
                top = L.end[row] - nb;
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const f32x4_t ds = *reinterpret_cast<const f32x4_t*>(&L.dsc[wd * 64 + b * 16 + 4 * lh]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = __fmul_rn(__fmul_rn((float)acc[a][b][r], ds[r]), qs);
                    sc[a][b][r] = v;
                    if constexpr (WIN) h |= (v > thr) & (v < bel) & (b * 16 + r > lim) & (b * 16 + r < top);   // (end <= N)
                    else h |= (v > thr) & (v < bel) & (n0 + wd * 64 + b * 16 + 4 * lh + r < p.N);
                }
            }
            if (h) L.flag[row] = 1;
            hit |= h;
        }
        if (hit) L.any = 1;
        __syncthreads();
        if (L.any) {
            float* tile = reinterpret_cast<float*>(L.ops);   // the operand buffers are free until the next tile
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    *reinterpret_cast<f32x4_t*>(tile + (wq * 64 + a * 16 + l15) * TN + wd * 64 + b * 16 + 4 * lh) = sc[a][b];
            __syncthreads();
            for (int row = wave; row < TM; row += 4)
                if (L.flag[row]) insert_row<WIN>(p, L, tile, row, m0 + row, n0, split, wave, lane);
            __syncthreads();
            if (tid < TM) L.flag[tid] = 0;
            if (tid == 0) L.any = 0;
        }
        __syncthreads();
    }
    if (tid < TM && m0 + tid < p.M) p.counts[(int64_t)(m0 + tid) * p.nsplit + split] = L.cnt[tid];
}

// ---- product-quantised rows (cx_search_pq_topk) -----------------------------------------------------------------------
// Stage 1 over PQ codes (pq.hip): document n is the concatenation of codebook[s][code[n][s]], s < m = d / dsub, bf16 centroids
// of width dsub in {8, 16, 32, 64}.  search_tiles_kernel<false> with another way of filling the document panel: a 16-byte
// piece of the panel is 8 consecutive K elements, i.e. one aligned 16-byte slice of ONE centroid, so the panel is gathered from
// the codebook (256 * d * 2 bytes, resident in L2) instead of read from rows; the corpus itself is read as m bytes per row, once
// per tile, into LDS.  The query half of the staging, commit / poff, the K loop's MFMA order, the epilogue, insert_row<false>
// and the split merge are the bf16 kernel's, so a score has the bits cx_search_topk gives the decoded row.
struct PqParams : SearchParams {     // (D / ldd of the base stay unused)
    const uint8_t* codes;  // (N, m), byte leading dimension ldc >= m, any alignment
    const bf16_t* cb;      // (m, 256, dsub) bf16, 16-B aligned
    long ldc;
    int m, lsub;           // dsub = 1 << lsub
    int flat;              // ldc == m and codes 16-B aligned: a tile's codes are one aligned run of bytes
};

struct PqSearchLds : SearchLds {
    alignas(16) uint8_t code[TN * 128];   // [row of the tile][m]: the codes of the current corpus tile (m <= 128)
};

// The tile's codes; row r >= N - n0 holds the codes of row N - 1 (read but never admitted, as the clamped rows of stage).
CX_DEVICE void load_codes(const PqParams& p, uint8_t* code, int n0, int tid) {
    const int rows = min(TN, p.N - n0);
    const int vec = p.flat ? (rows * p.m) & ~15 : 0;   // bytes copied 16 at a time: inside [n0 * m, N * m)
    const uint8_t* src = p.codes + (int64_t)n0 * p.ldc;
    for (int b = tid * 16; b < vec; b += 256 * 16) *reinterpret_cast<uint4*>(code + b) = *reinterpret_cast<const uint4*>(src + b);
    for (int b = vec + tid; b < TN * p.m; b += 256) {
        const int r = b / p.m, s = b - r * p.m;
        code[b] = p.codes[(int64_t)min(n0 + r, p.N - 1) * p.ldc + s];
    }
}

// stage with the document half gathered: piece (r, c) of chunk k0 is 8 elements from (k0 + 8c) % dsub on of centroid
// code[r][(k0 + 8c) / dsub] of sub-quantiser (k0 + 8c) / dsub.  A code is a byte: the gather stays inside the codebook.
CX_DEVICE void stage_pq(const PqParams& p, const uint8_t* code, int m0, int k0, int tid, uint4 (&sq)[4], uint4 (&sd)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int item = tid + 256 * i, r = item >> 3, c = item & 7;
        const int gm = min(m0 + r, p.M - 1);
        const int kk = k0 + c * 8, s = kk >> p.lsub;
        const int cell = s * 256 + code[r * p.m + s];
        sq[i] = *reinterpret_cast<const uint4*>(p.Q + (int64_t)gm * p.ldq + kk);
        sd[i] = *reinterpret_cast<const uint4*>(p.cb + ((cell << p.lsub) + (kk & ((1 << p.lsub) - 1))));
    }
}

// The stager of the PQ walk: the tile's codes go to LDS before the tile's first chunk (they were last read in the previous
// tile's K loop, behind that tile's barriers), and every chunk's document half is gathered through them.
struct PqStage {
    uint8_t* code;
    CX_DEVICE void begin_tile(const PqParams& p, int n0, int tid) const {
        load_codes(p, code, n0, tid);
        __syncthreads();
    }
    CX_DEVICE void operator()(const PqParams& p, int m0, int, int k0, int tid, uint4 (&sq)[4], uint4 (&sd)[4]) const {
        stage_pq(p, code, m0, k0, tid, sq, sd);
    }
};

__global__ __launch_bounds__(256, 1) void search_pq_tiles_kernel(PqParams p) {
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    PqSearchLds& L = *reinterpret_cast<PqSearchLds*>(dsm);
    search_tiles_walk<false>(p, L, PqStage{L.code});
}

constexpr int MAXLISTS = 256;       // lists merged into one output row (>= MAXSPLIT)

// What the merge orders: (score, reported id).  int64 ids: the reported id of cx_topk_merge_lists is any int64 of id_map.
struct Ent {
    float s;
    int64_t id;
};

// cx_search_topk's workspace: output row m merges the lists m * nsplit + [0, nsplit); a list's length is in counts
struct SplitLists {
    const Cand* lists;
    const int* counts;
    int nsplit, k;
    CX_DEVICE int64_t list_of(int row, int l) const { return (int64_t)row * nsplit + l; }
    CX_DEVICE int count(int64_t r) const { return counts[r]; }
    CX_DEVICE float score(int64_t r, int j) const { return lists[r * k + j].s; }
    CX_DEVICE int64_t id(int64_t r, int j) const { return lists[r * k + j].id; }
};

// (P, k) score / id arrays as the search entry points write them: sorted rows padded with (-inf, -1), so a list ends at its
// first negative id.  Output row m merges the lists src[m][0 .. L); an entry outside [0, P) names no list.  id_map (or null):
// the reported id of position n is id_map[n], n clamped to [0, N) for the read.
struct PaddedLists {
    const float* s;
    const int64_t* ids;
    const int64_t* src;
    const int64_t* id_map;
    int64_t P, N;
    int L, k;
    CX_DEVICE int64_t list_of(int row, int l) const {
        const int64_t r = src[(int64_t)row * L + l];
        return (r >= 0 && r < P) ? r : -1;
    }
    CX_DEVICE int count(int64_t r) const {
        int lo = 0, hi = k;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ids[r * k + mid] >= 0) lo = mid + 1; else hi = mid;
        }
        return lo;
    }
    CX_DEVICE float score(int64_t r, int j) const { return s[r * k + j]; }
    CX_DEVICE int64_t id(int64_t r, int j) const {
        const int64_t n = ids[r * k + j];
        return id_map ? id_map[min(max(n, (int64_t)0), N - 1)] : n;
    }
};

// number of entries of the sorted list r (n entries) that beat e; an id is read only where the scores tie
template <class Lists> CX_DEVICE int count_beating(const Lists& S, int64_t r, int n, Ent e) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const float s = S.score(r, mid);
        const bool b = s != e.s ? s > e.s : S.id(r, mid) < e.id;
        if (b) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one wave per output row: merge the row's L sorted, disjoint lists into its top-k by (score descending, reported id
// ascending).  Every list must be sorted in that order (a list whose reported ids ascend with its positions is).
template <class Lists>
__global__ __launch_bounds__(256) void merge_lists_kernel(Lists S, int M, int L, int k, float* __restrict__ out_s,
                                                          int64_t* __restrict__ out_id) {
    __shared__ int64_t lrow_[4][MAXLISTS];
    __shared__ int lcnt_[4][MAXLISTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave;
    if (row >= M) return;   // (no workgroup barrier below)
    int64_t* lrow = lrow_[wave];
    int* cnt = lcnt_[wave];
    for (int l = lane; l < L; l += 64) {
        const int64_t r = S.list_of(row, l);
        lrow[l] = r;
        cnt[l] = r < 0 ? 0 : min(S.count(r), k);
    }
    wave_sync();
    int total = 0;
    for (int s = 0; s < L; ++s) total += cnt[s];
    for (int idx = lane; idx < L * k; idx += 64) {
        const int s = idx / k, j = idx - s * k;
        if (j >= cnt[s]) continue;
        const Ent e = Ent{S.score(lrow[s], j), S.id(lrow[s], j)};
        int rank = j;
        for (int s2 = 0; s2 < L && rank < k; ++s2)
            if (s2 != s && cnt[s2] > 0) rank += count_beating(S, lrow[s2], cnt[s2], e);
        if (rank < k) {
            out_s[(int64_t)row * k + rank] = e.s;
            out_id[(int64_t)row * k + rank] = e.id;
        }
    }
    for (int r = min(total, k) + lane; r < k; r += 64) {
        out_s[(int64_t)row * k + r] = -INFINITY;
        out_id[(int64_t)row * k + r] = -1;
    }
}

int auto_splits(int M, long N, int nsplit) {
    const int tiles_m = (M + TM - 1) / TM;
    const long tiles_n = (N + TN - 1) / TN;
    if (nsplit <= 0) nsplit = (SPLIT_TARGET_WG + tiles_m - 1) / tiles_m;
    nsplit = min(nsplit, MAXSPLIT);
    return (int)max(1L, min((long)nsplit, tiles_n));
}

}  // namespace

extern "C" {

long cx_search_ws_bytes(int M, long N, int k, int nsplit) {
    if (M <= 0 || N <= 0 || k <= 0) return 0;
    const long s = auto_splits(M, N, nsplit);
    return (long)M * s * ((long)k * (long)sizeof(Cand) + (long)sizeof(int)) + 16;
}

int cx_search_topk(const uint16_t* Q, const uint16_t* D, int M, long N, int d, long ldq, long ldd, int k,
                   const int64_t* excl_ptr, const int64_t* excl_ids, const float* below, int nsplit, void* ws,
                   float* out_scores, int64_t* out_ids, void* stream) {
    if (M < 0 || N < 0 || k < 1 || k > MAXK || d < 64 || d > 1024 || (d % 64) != 0 || N > MAX_N) return CX_ERR_SHAPE;
    if (M == 0) return CX_OK;
    if (!Q || !out_scores || !out_ids || (N > 0 && (!D || !ws)) || (excl_ptr && !excl_ids)) return CX_ERR_ARG;
    if (ldq < d || (ldq % 8) != 0 || (N > 0 && (ldd < d || (ldd % 8) != 0))) return CX_ERR_ALIGN;
    if (((uintptr_t)Q & 15) || ((uintptr_t)D & 15) || ((uintptr_t)ws & 15)) return CX_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int ns = N > 0 ? auto_splits(M, N, nsplit) : 1;
    Cand* lists = reinterpret_cast<Cand*>(ws);
    int* counts = N > 0 ? reinterpret_cast<int*>(lists + (int64_t)M * ns * k) : nullptr;
    if (N > 0) {
        SearchParams p = {};
        p.Q = Q; p.D = D; p.ldq = ldq; p.ldd = ldd;
        p.M = M; p.N = (int)N; p.d = d; p.k = k;
        p.nsplit = ns;
        p.tiles_n = (int)((N + TN - 1) / TN);
        p.tiles_per_split = (p.tiles_n + ns - 1) / ns;
        p.xptr = excl_ptr; p.xids = excl_ids; p.below = below;
        p.lists = lists; p.counts = counts;
        const int tiles_m = (M + TM - 1) / TM;
        static CxLdsOptIn opt;
        if (!opt.ensure(reinterpret_cast<const void*>(&search_tiles_kernel<false>), (int)sizeof(SearchLds))) return CX_ERR_LAUNCH;
        hipLaunchKernelGGL(search_tiles_kernel<false>, dim3(tiles_m * ns), dim3(256), sizeof(SearchLds), s, p);
        if (hipGetLastError() != hipSuccess) return CX_ERR_LAUNCH;
    }
    // N == 0: counts stays null and every row is padding
    const SplitLists S = {lists, counts, ns, k};
    hipLaunchKernelGGL(merge_lists_kernel<SplitLists>, dim3((M + 3) / 4), dim3(256), 0, s, S, M, N > 0 ? ns : 0, k, out_scores,
                       out_ids);
    return hipGetLastError() == hipSuccess ? CX_OK : CX_ERR_LAUNCH;
}

long cx_search_int8_ws_bytes(int M, long N, int k, int nsplit) { return cx_search_ws_bytes(M, N, k, nsplit); }

int cx_search_int8_topk(const int8_t* Q, const int8_t* D, const float* q_scale, const float* d_scale, int M, long N, int d,
                        long ldq, long ldd, int k, const int64_t* excl_ptr, const int64_t* excl_ids, const float* below,
                        int nsplit, void* ws, float* out_scores, int64_t* out_ids, void* stream) {
    if (M < 0 || N < 0 || k < 1 || k > MAXK || d < 64 || d > 1024 || (d % 64) != 0 || N > MAX_N) return CX_ERR_SHAPE;
    if (M == 0) return CX_OK;
    if (!Q || !q_scale || !out_scores || !out_ids || (N > 0 && (!D || !d_scale || !ws)) || (excl_ptr && !excl_ids))
        return CX_ERR_ARG;
    if (ldq < d || (ldq % 16) != 0 || (N > 0 && (ldd < d || (ldd % 16) != 0))) return CX_ERR_ALIGN;
    if (((uintptr_t)Q & 15) || ((uintptr_t)D & 15) || ((uintptr_t)ws & 15)) return CX_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int ns = N > 0 ? auto_splits(M, N, nsplit) : 1;
    Cand* lists = reinterpret_cast<Cand*>(ws);
    int* counts = N > 0 ? reinterpret_cast<int*>(lists + (int64_t)M * ns * k) : nullptr;
    if (N > 0) {
        Int8Params p = {};
        p.Q8 = Q; p.D8 = D; p.q_scale = q_scale; p.d_scale = d_scale; p.ldq = ldq; p.ldd = ldd;
        p.M = M; p.N = (int)N; p.d = d; p.k = k;
        p.nsplit = ns;
        p.tiles_n = (int)((N + TN - 1) / TN);
        p.tiles_per_split = (p.tiles_n + ns - 1) / ns;
        p.xptr = excl_ptr; p.xids = excl_ids; p.below = below;
        p.lists = lists; p.counts = counts;
        const int tiles_m = (M + TM - 1) / TM;
        static CxLdsOptIn opt;
        if (!opt.ensure(reinterpret_cast<const void*>(&search_int8_tiles_kernel<false>), (int)sizeof(Int8SearchLds<false>)))
            return CX_ERR_LAUNCH;
        hipLaunchKernelGGL(search_int8_tiles_kernel<false>, dim3(tiles_m * ns), dim3(256), sizeof(Int8SearchLds<false>), s, p);
        if (hipGetLastError() != hipSuccess) return CX_ERR_LAUNCH;
    }
    const SplitLists S = {lists, counts, ns, k};
    hipLaunchKernelGGL(merge_lists_kernel<SplitLists>, dim3((M + 3) / 4), dim3(256), 0, s, S, M, N > 0 ? ns : 0, k, out_scores,
                       out_ids);
    return hipGetLastError() == hipSuccess ? CX_OK : CX_ERR_LAUNCH;
}

long cx_search_pq_ws_bytes(int M, long N, int k, int nsplit) { return cx_search_ws_bytes(M, N, k, nsplit); }

int cx_search_pq_topk(const uint16_t* Q, const uint8_t* codes, const uint16_t* codebook, int M, long N, int d, int dsub,
                      long ldq, long ldc, int k, const int64_t* excl_ptr, const int64_t* excl_ids, const float* below,
                      int nsplit, void* ws, float* out_scores, int64_t* out_ids, void* stream) {
    if (M < 0 || N < 0 || k < 1 || k > MAXK || d < 64 || d > 1024 || (d % 64) != 0 || N > MAX_N) return CX_ERR_SHAPE;
    if (dsub != 8 && dsub != 16 && dsub != 32 && dsub != 64) return CX_ERR_SHAPE;
    if (M == 0) return CX_OK;
    if (!Q || !out_scores || !out_ids || (N > 0 && (!codes || !codebook || !ws)) || (excl_ptr && !excl_ids)) return CX_ERR_ARG;
    const int m = d / dsub;
    if (ldq < d || (ldq % 8) != 0 || (N > 0 && ldc < m)) return CX_ERR_ALIGN;
    if (((uintptr_t)Q & 15) || ((uintptr_t)codebook & 15) || ((uintptr_t)ws & 15)) return CX_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int ns = N > 0 ? auto_splits(M, N, nsplit) : 1;
    Cand* lists = reinterpret_cast<Cand*>(ws);
    int* counts = N > 0 ? reinterpret_cast<int*>(lists + (int64_t)M * ns * k) : nullptr;
    if (N > 0) {
        PqParams p = {};
        p.Q = Q; p.ldq = ldq;
        p.codes = codes; p.cb = codebook; p.ldc = ldc; p.m = m;
        p.lsub = dsub == 8 ? 3 : dsub == 16 ? 4 : dsub == 32 ? 5 : 6;
        p.flat = (ldc == m && ((uintptr_t)codes & 15) == 0) ? 1 : 0;
        p.M = M; p.N = (int)N; p.d = d; p.k = k;
        p.nsplit = ns;
        p.tiles_n = (int)((N + TN - 1) / TN);
        p.tiles_per_split = (p.tiles_n + ns - 1) / ns;
        p.xptr = excl_ptr; p.xids = excl_ids; p.below = below;
        p.lists = lists; p.counts = counts;
        const int tiles_m = (M + TM - 1) / TM;
        static CxLdsOptIn opt;
        if (!opt.ensure(reinterpret_cast<const void*>(&search_pq_tiles_kernel), (int)sizeof(PqSearchLds))) return CX_ERR_LAUNCH;
        hipLaunchKernelGGL(search_pq_tiles_kernel, dim3(tiles_m * ns), dim3(256), sizeof(PqSearchLds), s, p);
        if (hipGetLastError() != hipSuccess) return CX_ERR_LAUNCH;
    }
    const SplitLists S = {lists, counts, ns, k};
    hipLaunchKernelGGL(merge_lists_kernel<SplitLists>, dim3((M + 3) / 4), dim3(256), 0, s, S, M, N > 0 ? ns : 0, k, out_scores,
                       out_ids);
    return hipGetLastError() == hipSuccess ? CX_OK : CX_ERR_LAUNCH;
}

long cx_search_window_ws_bytes(int M, int k) {
    if (M <= 0 || k <= 0) return 0;
    return (long)M * ((long)k * (long)sizeof(Cand) + (long)sizeof(int)) + 16;
}

int cx_search_window_topk(const uint16_t* Q, const uint16_t* D, int M, long N, int d, long ldq, long ldd, int k,
                          const int64_t* min_id, const int64_t* end_id, const int64_t* excl_ptr, const int64_t* excl_ids,
                          const float* below, void* ws, float* out_scores, int64_t* out_ids, void* stream) {
    if (M < 0 || N < 0 || k < 1 || k > MAXK || d < 64 || d > 1024 || (d % 64) != 0 || N > MAX_N) return CX_ERR_SHAPE;
    if (M == 0) return CX_OK;
    if (!Q || !out_scores || !out_ids || (N > 0 && (!D || !ws)) || (excl_ptr && !excl_ids)) return CX_ERR_ARG;
    if (ldq < d || (ldq % 8) != 0 || (N > 0 && (ldd < d || (ldd % 8) != 0))) return CX_ERR_ALIGN;
    if (((uintptr_t)Q & 15) || ((uintptr_t)D & 15) || ((uintptr_t)ws & 15)) return CX_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    Cand* lists = reinterpret_cast<Cand*>(ws);
    int* counts = N > 0 ? reinterpret_cast<int*>(lists + (int64_t)M * k) : nullptr;
    if (N > 0) {
        SearchParams p = {};
        p.Q = Q; p.D = D; p.ldq = ldq; p.ldd = ldd;
        p.M = M; p.N = (int)N; p.d = d; p.k = k;
        p.nsplit = 1;   // one workgroup walks a query tile's whole band
        p.tiles_n = (int)((N + TN - 1) / TN);
        p.tiles_per_split = p.tiles_n;
        p.xptr = excl_ptr; p.xids = excl_ids; p.below = below;
        p.min_id = min_id; p.end_id = end_id;
        p.lists = lists; p.counts = counts;
        static CxLdsOptIn opt;
        if (!opt.ensure(reinterpret_cast<const void*>(&search_tiles_kernel<true>), (int)sizeof(WinSearchLds))) return CX_ERR_LAUNCH;
        hipLaunchKernelGGL(search_tiles_kernel<true>, dim3((M + TM - 1) / TM), dim3(256), sizeof(WinSearchLds), s, p);
        if (hipGetLastError() != hipSuccess) return CX_ERR_LAUNCH;
    }
    // the row's one list, padded, in the output layout
    const SplitLists S = {lists, counts, 1, k};
    hipLaunchKernelGGL(merge_lists_kernel<SplitLists>, dim3((M + 3) / 4), dim3(256), 0, s, S, M, N > 0 ? 1 : 0, k, out_scores,
                       out_ids);
    return hipGetLastError() == hipSuccess ? CX_OK : CX_ERR_LAUNCH;
}

long cx_search_int8_window_ws_bytes(int M, int k) { return cx_search_window_ws_bytes(M, k); }

int cx_search_int8_window_topk(const int8_t* Q, const int8_t* D, const float* q_scale, const float* d_scale, int M, long N,
                               int d, long ldq, long ldd, int k, const int64_t* min_id, const int64_t* end_id,
                               const int64_t* excl_ptr, const int64_t* excl_ids, const float* below, void* ws,
                               float* out_scores, int64_t* out_ids, void* stream) {
    if (M < 0 || N < 0 || k < 1 || k > MAXK || d < 64 || d > 1024 || (d % 64) != 0 || N > MAX_N) return CX_ERR_SHAPE;
    if (M == 0) return CX_OK;
    if (!Q || !q_scale || !out_scores || !out_ids || (N > 0 && (!D || !d_scale || !ws)) || (excl_ptr && !excl_ids))
        return CX_ERR_ARG;
    if (ldq < d || (ldq % 16) != 0 || (N > 0 && (ldd < d || (ldd % 16) != 0))) return CX_ERR_ALIGN;
    if (((uintptr_t)Q & 15) || ((uintptr_t)D & 15) || ((uintptr_t)ws & 15)) return CX_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    Cand* lists = reinterpret_cast<Cand*>(ws);
    int* counts = N > 0 ? reinterpret_cast<int*>(lists + (int64_t)M * k) : nullptr;
    if (N > 0) {
        Int8Params p = {};
        p.Q8 = Q; p.D8 = D; p.q_scale = q_scale; p.d_scale = d_scale; p.ldq = ldq; p.ldd = ldd;
        p.M = M; p.N = (int)N; p.d = d; p.k = k;
        p.nsplit = 1;   // one workgroup walks a query tile's whole band
        p.tiles_n = (int)((N + TN - 1) / TN);
        p.tiles_per_split = p.tiles_n;
        p.xptr = excl_ptr; p.xids = excl_ids; p.below = below;
        p.min_id = min_id; p.end_id = end_id;
        p.lists = lists; p.counts = counts;
        static CxLdsOptIn opt;
        if (!opt.ensure(reinterpret_cast<const void*>(&search_int8_tiles_kernel<true>), (int)sizeof(Int8SearchLds<true>)))
            return CX_ERR_LAUNCH;
        hipLaunchKernelGGL(search_int8_tiles_kernel<true>, dim3((M + TM - 1) / TM), dim3(256), sizeof(Int8SearchLds<true>), s, p);
        if (hipGetLastError() != hipSuccess) return CX_ERR_LAUNCH;
    }
    // the row's one list, padded, in the output layout
    const SplitLists S = {lists, counts, 1, k};
    hipLaunchKernelGGL(merge_lists_kernel<SplitLists>, dim3((M + 3) / 4), dim3(256), 0, s, S, M, N > 0 ? 1 : 0, k, out_scores,
                       out_ids);
    return hipGetLastError() == hipSuccess ? CX_OK : CX_ERR_LAUNCH;
}

int cx_topk_merge_lists(const float* scores, const int64_t* ids, long P, int k, const int64_t* src, int M, int L,
                        const int64_t* id_map, long N, float* out_scores, int64_t* out_ids, void* stream) {
    if (M < 0 || P < 0 || k < 1 || k > MAXK || L < 1 || L > MAXLISTS || (id_map && N < 1)) return CX_ERR_SHAPE;
    if (M == 0) return CX_OK;
    if (!src || !out_scores || !out_ids || (P > 0 && (!scores || !ids))) return CX_ERR_ARG;
    const PaddedLists S = {scores, ids, src, id_map, (int64_t)P, (int64_t)N, L, k};
    hipLaunchKernelGGL(merge_lists_kernel<PaddedLists>, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, S, M, L, k,
                       out_scores, out_ids);
    return hipGetLastError() == hipSuccess ? CX_OK : CX_ERR_LAUNCH;
}

}  // extern "C"
