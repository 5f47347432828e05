// rank.hip -- the rank of given target columns in a row of the (never written) similarity matrix: what zero-shot top-k
// accuracy (rank(label) < k) and retrieval recall@k (min over a row's positives of rank < k) reduce to
// (sc/trainers/image_text.py:198-254, sc/eval/metrics.py).
//
// For entry e of row m with t = tgt_ids[e]:  out_score[e] = s(m, t),
//   out_rank[e] = #{ n in [0, N) : s(m, n) > s(m, t)  or  (s(m, n) == s(m, t) and n < t) }
// -- the 0-based position of t in search.hip's strict total order (descending score, ties to the lower id).
//
// Scores have search.hip's instruction sequence: v_mfma_f32_16x16x32_bf16 with A := document rows, B := query rows, K
// ascending in 32-wide steps from a zero fp32 accumulator.  An output element of that instruction depends on its own A row
// and B row only, so a pair's score has ONE value whatever tile it is computed in -- the property cx_rescore_topk already
// rests on.  Three launches:
//   1. rank_gather_kernel: a workgroup owns a 128-query tile and walks its CSR entries 128 at a time; the document side of
//      the tile is the GATHERED target rows, so s(m, t) comes out of the tile accumulators; the lane that owns (row of e,
//      column e) writes out_score[e].  One tile per 128 entries, not one per document tile.
//   2. rank_count_kernel: (query tile x corpus split).  A lane holds its four rows' thresholds (score, id) of the current
//      group of PG targets per row in registers, compares its 16 scores of a row against them after every tile's K loop and
//      keeps the counts in registers over the whole split: one cross-lane reduction at the end and one plain store per
//      (entry, split, document half of the tile) into the workspace.  Rows with more than PG targets take further walks
//      (the group loop is inside the kernel: per query tile, so a single long row costs its own tile only).  PG = 1 when
//      no row of the tile has more than one target (labels), else 8.
//   3. rank_sum_kernel: out_rank[e] = the sum of the entry's 2 * nsplit partial counts.  Integer adds: the result depends
//      on neither nsplit nor scheduling, and no atomic is involved.
// No candidate lists, no merge, no k, no fp32 score tile in LDS.
#include "cx_common.h"
#include "score_tile.h"   // TM / TN / BK / PANEL, poff, tile_scores, auto_splits: shared with range.hip
#include "../../include/contrastors_hip.h"

namespace {

constexpr int PGMAX = 8;

struct RankParams {
    const bf16_t* Q;
    const bf16_t* D;
    long ldq, ldd;
    int M, N, d;
    int nsplit, tiles_n, tiles_per_split;
    const int64_t* tptr;   // (M + 1)
    const int64_t* tids;   // (nnz)
    int* part;             // (nnz, nsplit, 2) partial counts (workspace; every slot is written)
    int32_t* out_rank;
    float* out_score;
};

struct GatherLds {
    char ops[4 * PANEL];
    int64_t pl[TM + 1];   // the tile rows' CSR offsets (rows past M repeat the end)
    int erow[TN];         // local query row of the chunk's entry j, -1 past the end
};

__global__ __launch_bounds__(256, 1) void rank_gather_kernel(RankParams p) {
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    GatherLds& L = *reinterpret_cast<GatherLds*>(dsm);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wq = wave >> 1, wd = wave & 1, l15 = lane & 15, lh = lane >> 4;
    const int m0 = blockIdx.x * TM;
    const int64_t e_begin = p.tptr[m0], e_end = p.tptr[min(m0 + TM, p.M)];
    if (tid <= TM) L.pl[tid] = p.tptr[min(m0 + tid, p.M)];
    __syncthreads();
    int64_t qo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qo[i] = (int64_t)min(m0 + (tid >> 3) + 32 * i, p.M - 1) * p.ldq;   // clamped rows own no entry
    for (int64_t e0 = e_begin; e0 < e_end; e0 += TN) {
        if (tid < TN) {
            // the row r with pl[r] <= e < pl[r + 1]: the last r with pl[r] <= e (empty rows share an offset)
            const int64_t e = e0 + tid;
            int lo = 0, hi = TM;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (L.pl[mid] <= e) lo = mid; else hi = mid;
            }
            L.erow[tid] = e < e_end ? lo : -1;
        }
        int64_t d_o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t e = e0 + (tid >> 3) + 32 * i;
            // ids are validated before the launch; the clamp keeps a bad one inside the corpus all the same
            const int64_t t = e < e_end ? p.tids[e] : 0;
            d_o[i] = min(max(t, (int64_t)0), (int64_t)p.N - 1) * p.ldd;
        }
        f32x4_t acc[4][4];
        tile_scores(p.Q, p.D, qo, d_o, p.d / BK, L.ops, tid, acc);   // (its first barrier publishes L.erow)
        // acc[a][b][r] = score(query m0 + wq*64 + a*16 + l15, entry e0 + wd*64 + b*16 + 4*lh + r)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = wd * 64 + b * 16 + 4 * lh + r;
                const int rj = L.erow[j];
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    if (rj == wq * 64 + a * 16 + l15) p.out_score[e0 + j] = acc[a][b][r];
            }
        __syncthreads();   // L.erow is rewritten for the next chunk
    }
}

struct CountLds {
    char ops[4 * PANEL];
    int64_t pbeg[TM], pend[TM];   // the tile rows' CSR ranges (empty past M)
    int maxlen;
};

template <int PG>
CX_DEVICE void count_walk(const RankParams& p, CountLds& L, int m0, int t_begin, int t_end, int g0, int split, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    const int wq = wave >> 1, wd = wave & 1, l15 = lane & 15, lh = lane >> 4;
    float th[4][PG];
    int id[4][PG], cnt[4][PG];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int row = wq * 64 + a * 16 + l15;
        const int64_t pb = L.pbeg[row] + g0, pe = L.pend[row];
#pragma unroll
        for (int g = 0; g < PG; ++g) {
            const bool have = pb + g < pe;
            // padding: no score is above +inf or equal to it with an id below -1 ... nothing is counted and nothing written
            th[a][g] = have ? p.out_score[pb + g] : INFINITY;
            id[a][g] = have ? (int)p.tids[pb + g] : -1;
            cnt[a][g] = 0;
        }
    }
    int64_t qo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qo[i] = (int64_t)min(m0 + (tid >> 3) + 32 * i, p.M - 1) * p.ldq;
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
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int g = 0; g < PG; ++g) {
                const float tv = th[a][g];
                const int lim = id[a][g] - nb;   // column nb + c is below the target's id  <=>  c < lim
                int c = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = acc[a][b][r];
                        c += (v > tv) | ((v == tv) & (b * 16 + r < lim)) ? 1 : 0;
                    }
                cnt[a][g] += c;
            }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int row = wq * 64 + a * 16 + l15;
        const int64_t pb = L.pbeg[row] + g0, pe = L.pend[row];
#pragma unroll
        for (int g = 0; g < PG; ++g) {
            int c = cnt[a][g];
            c += __shfl_xor(c, 16, 64);
            c += __shfl_xor(c, 32, 64);
            if (lh == 0 && pb + g < pe) p.part[((pb + g) * p.nsplit + split) * 2 + wd] = c;
        }
    }
}

__global__ __launch_bounds__(256, 1) void rank_count_kernel(RankParams p) {
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    CountLds& L = *reinterpret_cast<CountLds*>(dsm);
    const int tid = threadIdx.x;
    const int tm = blockIdx.x / p.nsplit, split = blockIdx.x % p.nsplit;
    const int m0 = tm * TM;
    const int t_begin = split * p.tiles_per_split, t_end = min(p.tiles_n, t_begin + p.tiles_per_split);
    if (tid == 0) L.maxlen = 0;
    __syncthreads();
    if (tid < TM) {
        const int m = m0 + tid;
        const int64_t pb = m < p.M ? p.tptr[m] : 0, pe = m < p.M ? p.tptr[m + 1] : 0;
        L.pbeg[tid] = pb;
        L.pend[tid] = pe;
        atomicMax(&L.maxlen, (int)min(pe - pb, (int64_t)0x7fffffff));
    }
    __syncthreads();
    const int maxlen = L.maxlen;
    if (maxlen <= 1) {
        if (maxlen == 1) count_walk<1>(p, L, m0, t_begin, t_end, 0, split, tid);
    } else {
        for (int g0 = 0; g0 < maxlen; g0 += PGMAX) count_walk<PGMAX>(p, L, m0, t_begin, t_end, g0, split, tid);
    }
}

// one wave per query row: its lanes stride over the row's entries
__global__ __launch_bounds__(256) void rank_sum_kernel(const int64_t* __restrict__ tptr, const int* __restrict__ part, int M,
                                                       int nsplit, int32_t* __restrict__ out_rank) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int64_t pe = tptr[row + 1];
    for (int64_t e = tptr[row] + lane; e < pe; e += 64) {
        int c = 0;
        for (int i = 0; i < 2 * nsplit; ++i) c += part[e * 2 * nsplit + i];
        out_rank[e] = c;
    }
}

}  // namespace

extern "C" {

long cx_rank_ws_bytes(int M, long N, long nnz, int nsplit) {
    if (M <= 0 || N <= 0 || nnz <= 0) return 0;
    return nnz * auto_splits(M, N, nsplit) * 2 * (long)sizeof(int) + 16;   // per entry: (split, document half) partial counts
}

int cx_rank_targets(const uint16_t* Q, const uint16_t* D, int M, long N, int d, long ldq, long ldd, const int64_t* tgt_ptr,
                    const int64_t* tgt_ids, int nsplit, void* ws, int32_t* out_rank, float* out_score,
                    void* stream) {
    if (M < 0 || N < 0 || d < 64 || d > 1024 || (d % 64) != 0 || N > MAX_N) return CX_ERR_SHAPE;
    if (M == 0 || N == 0) return CX_OK;
    if (!Q || !D || !tgt_ptr || !tgt_ids || !ws || !out_rank || !out_score) return CX_ERR_ARG;
    if (ldq < d || (ldq % 8) != 0 || ldd < d || (ldd % 8) != 0) return CX_ERR_ALIGN;
    if (((uintptr_t)Q & 15) || ((uintptr_t)D & 15) || ((uintptr_t)ws & 15)) return CX_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    RankParams p = {};
    p.Q = Q; p.D = D; p.ldq = ldq; p.ldd = ldd;
    p.M = M; p.N = (int)N; p.d = d;
    p.nsplit = auto_splits(M, N, nsplit);
    p.tiles_n = (int)((N + TN - 1) / TN);
    p.tiles_per_split = (p.tiles_n + p.nsplit - 1) / p.nsplit;
    p.tptr = tgt_ptr; p.tids = tgt_ids;
    p.part = reinterpret_cast<int*>(ws);
    p.out_rank = out_rank; p.out_score = out_score;
    const int tiles_m = (M + TM - 1) / TM;
    static CxLdsOptIn opt_g, opt_c;
    if (!opt_g.ensure(reinterpret_cast<const void*>(&rank_gather_kernel), (int)sizeof(GatherLds))) return CX_ERR_LAUNCH;
    if (!opt_c.ensure(reinterpret_cast<const void*>(&rank_count_kernel), (int)sizeof(CountLds))) return CX_ERR_LAUNCH;
    hipLaunchKernelGGL(rank_gather_kernel, dim3(tiles_m), dim3(256), sizeof(GatherLds), s, p);
    if (hipGetLastError() != hipSuccess) return CX_ERR_LAUNCH;
    hipLaunchKernelGGL(rank_count_kernel, dim3(tiles_m * p.nsplit), dim3(256), sizeof(CountLds), s, p);
    if (hipGetLastError() != hipSuccess) return CX_ERR_LAUNCH;
    hipLaunchKernelGGL(rank_sum_kernel, dim3((M + 3) / 4), dim3(256), 0, s, tgt_ptr, p.part, M, p.nsplit, out_rank);
    return hipGetLastError() == hipSuccess ? CX_OK : CX_ERR_LAUNCH;
}

}  // extern "C"
