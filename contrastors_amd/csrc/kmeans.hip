// kmeans.hip -- Lloyd's k-means on bf16 points: the assignment (an arg-max over a centroid table, fused with the score tile)
// and the centroid update (a sum of rows by label without float atomics).  contrastors_amd/cluster.py drives them.
//
//   cx_kmeans_assign   kmeans_assign_kernel: a workgroup owns 128 points and walks ALL centroid tiles (no split, no workspace:
//                      with fewer than 128 x CU-count points the grid is simply small).  Scores come from tile_scores
//                      (score_tile.h) with points as the query operand, so a (point, centroid) score has the bits
//                      cx_search_topk gives it; half_norm[c] is subtracted once, in fp32, from the finished accumulator
//                      (Euclidean: argmax x.c - |c|^2 / 2; NULL: plain inner product).  A lane keeps (best, id, second) of
//                      its four points in registers over the whole walk: its columns ascend, so a strict `>` keeps the lower
//                      id.  One cross-lane merge and one LDS merge of the two column halves at the end.  A column past K has
//                      bias +inf, that is value -inf: it never wins and never becomes the second; K == 1 leaves second = -inf.
//   cx_kmeans_partial  kmeans_partial_kernel: one workgroup per PIECE (at most 256 consecutive entries of `order`, the stable
//                      sort of the labels, all of one cluster) sums its rows into one fp32 (d) partial.  HBM-bound row gather:
//                      d / 8 lanes cover a row with 16-B loads, 256 / (d / 8) row groups run side by side, group g takes the
//                      piece's rows g, g + G, ... in that order with four rows in flight, and the groups are added in
//                      ascending g.  A cluster of any size is spread over ceil(count / 256) workgroups.
//   cx_kmeans_finish   kmeans_finish_kernel: one workgroup per cluster adds the cluster's partials in piece order and writes
//                      the count, the fp32 centroid (mean, or the sum scaled to unit L2 norm), its bf16 shadow (the operand of
//                      the next assignment) and half_norm = |shadow|^2 / 2 summed in fp32 over ascending dimension.  An empty
//                      cluster reports count 0 and leaves its centroid, shadow and half_norm untouched.
// The summation order is a function of (labels, N, the piece length) and d only: no atomics, bitwise reproducible.
#include "cx_common.h"
#include "score_tile.h"
#include "../../include/contrastors_hip.h"

namespace {

constexpr int PIECE = CX_KMEANS_PIECE_ROWS;   // rows per piece at most: the ids of a piece sit in LDS, one per thread

struct AssignParams {
    const bf16_t* X;
    const bf16_t* C;
    long ldx, ldc;
    int N, K, d;
    const float* half_norm;   // (K) or NULL
    int* label;               // (N)
    float* best;              // (N)
    float* second;            // (N) or NULL
};

struct AssignLds {
    char ops[4 * PANEL];
    float bias[2][TN];        // the tile's half norms (+inf past K), double-buffered over tiles
    float mbest[2][TM], msec[2][TM];   // per column half of the tile: a row's merged running state
    int mid[2][TM];
};

// (b, i, s) := the best, its id and the second best of the union of two disjoint column sets; ties to the lower id
CX_DEVICE void merge_state(float& b, int& i, float& s, float ob, int oi, float os) {
    const bool w = ob > b || (ob == b && oi < i);
    s = w ? fmaxf(b, os) : fmaxf(s, ob);
    i = w ? oi : i;
    b = w ? ob : b;
}

__global__ __launch_bounds__(256, 1) void kmeans_assign_kernel(AssignParams p) {
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    AssignLds& L = *reinterpret_cast<AssignLds*>(dsm);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wq = wave >> 1, wd = wave & 1, l15 = lane & 15, lh = lane >> 4;
    const int m0 = blockIdx.x * TM;
    float best[4], sec[4];
    int id[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        best[a] = -INFINITY;
        sec[a] = -INFINITY;
        id[a] = 0;
    }
    int64_t qo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qo[i] = (int64_t)min(m0 + (tid >> 3) + 32 * i, p.N - 1) * p.ldx;   // clamped rows are not stored
    const int tiles_k = (p.K + TN - 1) / TN;
    for (int t = 0; t < tiles_k; ++t) {
        const int n0 = t * TN;
        // read after tile_scores' barriers; the other buffer may still be read by a wave in the previous tile's epilogue
        float* bias = L.bias[t & 1];
        if (tid < TN) {
            const int c = n0 + tid;
            bias[tid] = c < p.K ? (p.half_norm ? p.half_norm[c] : 0.f) : INFINITY;
        }
        int64_t d_o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) d_o[i] = (int64_t)min(n0 + (tid >> 3) + 32 * i, p.K - 1) * p.ldc;
        f32x4_t acc[4][4];
        tile_scores(p.X, p.C, qo, d_o, p.d / BK, L.ops, tid, acc);
        // acc[a][b][r] = score(point m0 + wq*64 + a*16 + l15, centroid n0 + wd*64 + b*16 + 4*lh + r): ascending in (b, r)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const f32x4_t bv = *reinterpret_cast<const f32x4_t*>(bias + wd * 64 + b * 16 + 4 * lh);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = n0 + wd * 64 + b * 16 + 4 * lh + r;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const float v = acc[a][b][r] - bv[r];
                    const bool w = v > best[a];   // strict: an equal value at a higher id does not take over
                    sec[a] = w ? best[a] : fmaxf(sec[a], v);
                    id[a] = w ? col : id[a];
                    best[a] = w ? v : best[a];
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float ob = __shfl_xor(best[a], o, 64), os = __shfl_xor(sec[a], o, 64);
            const int oi = __shfl_xor(id[a], o, 64);
            merge_state(best[a], id[a], sec[a], ob, oi, os);
        }
        if (lh == 0) {
            const int row = wq * 64 + a * 16 + l15;
            L.mbest[wd][row] = best[a];
            L.msec[wd][row] = sec[a];
            L.mid[wd][row] = id[a];
        }
    }
    __syncthreads();
    if (tid < TM && m0 + tid < p.N) {
        float b = L.mbest[0][tid], s = L.msec[0][tid];
        int i = L.mid[0][tid];
        merge_state(b, i, s, L.mbest[1][tid], L.mid[1][tid], L.msec[1][tid]);
        p.label[m0 + tid] = i;
        p.best[m0 + tid] = b;
        if (p.second) p.second[m0 + tid] = s;
    }
}

__global__ __launch_bounds__(256) void kmeans_partial_kernel(const bf16_t* __restrict__ X, long ldx, int N, int d,
                                                             const int* __restrict__ order, const int* __restrict__ piece_start,
                                                             const int* __restrict__ piece_end, const int* __restrict__ n_pieces,
                                                             int max_pieces, float* __restrict__ partial) {
    __shared__ int ids[PIECE];
    __shared__ __attribute__((aligned(16))) float red[2048];   // [row group][d]: G * d <= 256 * 8
    const int piece = blockIdx.x, tid = threadIdx.x;
    if (piece >= min(*n_pieces, max_pieces)) return;
    const int s = max(piece_start[piece], 0);
    const int n = min(min(piece_end[piece], N) - s, PIECE);
    if (tid < n) ids[tid] = min(max(order[s + tid], 0), N - 1);
    __syncthreads();
    const int lpr = d >> 3, G = 256 / lpr;   // lanes per row (16 B each), rows side by side
    const int g = tid / lpr, c = tid - g * lpr;
    if (g < G) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const bf16_t* col = X + c * 8;
        auto add = [&](const uint4& v) {
            float f[8];
            unpack8(v, f);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += f[e];
        };
        int j = g;
        for (; j + 3 * G < n; j += 4 * G) {   // four rows in flight, added in run order
            uint4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const uint4*>(col + (int64_t)ids[j + u * G] * ldx);
#pragma unroll
            for (int u = 0; u < 4; ++u) add(v[u]);
        }
        for (; j < n; j += G) add(*reinterpret_cast<const uint4*>(col + (int64_t)ids[j] * ldx));
        float* r = red + g * d + c * 8;
        *reinterpret_cast<float4*>(r) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        *reinterpret_cast<float4*>(r + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
    __syncthreads();
    for (int cidx = tid; cidx < d; cidx += 256) {
        float sum = red[cidx];
        for (int gg = 1; gg < G; ++gg) sum += red[gg * d + cidx];
        partial[(int64_t)piece * d + cidx] = sum;
    }
}

__global__ __launch_bounds__(256) void kmeans_finish_kernel(const float* __restrict__ partial, const int* __restrict__ piece_start,
                                                            const int* __restrict__ piece_end, const int* __restrict__ piece_ptr,
                                                            int d, int max_pieces, int spherical, int* __restrict__ counts,
                                                            float* __restrict__ centroids, bf16_t* __restrict__ shadow, long lds,
                                                            float* __restrict__ half_norm) {
    __shared__ float row[1024];
    __shared__ double norm2;
    const int k = blockIdx.x, tid = threadIdx.x;
    const int p0 = max(piece_ptr[k], 0), p1 = min(piece_ptr[k + 1], max_pieces);
    const int count = p1 > p0 ? piece_end[p1 - 1] - piece_start[p0] : 0;   // the pieces tile the cluster's run
    if (count <= 0) {
        if (tid == 0) counts[k] = 0;
        return;
    }
    for (int c = tid; c < d; c += 256) {
        const float* col = partial + c;
        float sum = 0.f;
        int p = p0;
        for (; p + 8 <= p1; p += 8) {   // eight partials in flight, added in piece order
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = col[(int64_t)(p + u) * d];
#pragma unroll
            for (int u = 0; u < 8; ++u) sum += v[u];
        }
        for (; p < p1; ++p) sum += col[(int64_t)p * d];
        row[c] = sum;
    }
    __syncthreads();
    if (spherical) {
        if (tid == 0) {   // fp64: the row's norm is then off by the final rounding of its elements only
            double n2 = 0.0;
            for (int j = 0; j < d; ++j) n2 += (double)row[j] * (double)row[j];
            norm2 = n2;
        }
        __syncthreads();
        const double inv = norm2 > 0.0 ? 1.0 / sqrt(norm2) : 0.0;
        for (int c = tid; c < d; c += 256) {
            const float v = (float)((double)row[c] * inv);
            centroids[(int64_t)k * d + c] = v;
            shadow[(int64_t)k * lds + c] = f32_to_bf16(v);
        }
        if (tid == 0) {
            counts[k] = count;
            half_norm[k] = 0.f;
        }
        return;
    }
    for (int c = tid; c < d; c += 256) {   // (a thread reads and rewrites its own columns of `row` only)
        const float v = row[c] / (float)count;
        const bf16_t sh = f32_to_bf16(v);
        centroids[(int64_t)k * d + c] = v;
        shadow[(int64_t)k * lds + c] = sh;
        row[c] = bf16_to_f32(sh);
    }
    __syncthreads();
    if (tid == 0) {
        float h = 0.f;
        for (int j = 0; j < d; ++j) h += row[j] * row[j];   // ascending dimension; a bf16 square is exact in fp32
        counts[k] = count;
        half_norm[k] = 0.5f * h;
    }
}

bool bad_dim(int d) { return d < 64 || d > 1024 || (d % 64) != 0; }

}  // namespace

extern "C" {

int cx_kmeans_assign(const uint16_t* X, const uint16_t* C, const float* half_norm, long N, long K, int d, long ldx, long ldc,
                     int32_t* label, float* best, float* second, void* stream) {
    if (N < 0 || K < 1 || bad_dim(d) || N > MAX_N || K > MAX_N) return CX_ERR_SHAPE;
    if (N == 0) return CX_OK;
    if (!X || !C || !label || !best) return CX_ERR_ARG;
    if (ldx < d || (ldx % 8) != 0 || ldc < d || (ldc % 8) != 0) return CX_ERR_ALIGN;
    if (((uintptr_t)X & 15) || ((uintptr_t)C & 15)) return CX_ERR_ALIGN;
    AssignParams p = {};
    p.X = X; p.C = C; p.ldx = ldx; p.ldc = ldc;
    p.N = (int)N; p.K = (int)K; p.d = d;
    p.half_norm = half_norm;
    p.label = label; p.best = best; p.second = second;
    static CxLdsOptIn opt;
    if (!opt.ensure(reinterpret_cast<const void*>(&kmeans_assign_kernel), (int)sizeof(AssignLds))) return CX_ERR_LAUNCH;
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)((N + TM - 1) / TM)), dim3(256), sizeof(AssignLds),
                       (hipStream_t)stream, p);
    return done();
}

int cx_kmeans_partial(const uint16_t* X, long N, int d, long ldx, const int32_t* order, const int32_t* piece_start,
                      const int32_t* piece_end, const int32_t* n_pieces, int max_pieces, float* partial, void* stream) {
    if (N < 0 || max_pieces < 0 || bad_dim(d) || N > MAX_N) return CX_ERR_SHAPE;
    if (N == 0 || max_pieces == 0) return CX_OK;
    if (!X || !order || !piece_start || !piece_end || !n_pieces || !partial) return CX_ERR_ARG;
    if (ldx < d || (ldx % 8) != 0 || ((uintptr_t)X & 15)) return CX_ERR_ALIGN;
    hipLaunchKernelGGL(kmeans_partial_kernel, dim3(max_pieces), dim3(256), 0, (hipStream_t)stream, X, ldx, (int)N, d, order,
                       piece_start, piece_end, n_pieces, max_pieces, partial);
    return done();
}

int cx_kmeans_finish(const float* partial, const int32_t* piece_start, const int32_t* piece_end, const int32_t* piece_ptr, long K,
                     int d, int max_pieces, int spherical, int32_t* counts, float* centroids, uint16_t* shadow, long lds,
                     float* half_norm, void* stream) {
    if (K < 0 || max_pieces < 0 || bad_dim(d) || K > MAX_N) return CX_ERR_SHAPE;
    if (K == 0) return CX_OK;
    if (!partial || !piece_start || !piece_end || !piece_ptr || !counts || !centroids || !shadow || !half_norm) return CX_ERR_ARG;
    if (lds < d) return CX_ERR_ALIGN;
    hipLaunchKernelGGL(kmeans_finish_kernel, dim3((unsigned)K), dim3(256), 0, (hipStream_t)stream, partial, piece_start, piece_end,
                       piece_ptr, d, max_pieces, spherical ? 1 : 0, counts, centroids, shadow, lds, half_norm);
    return done();
}

}  // extern "C"
