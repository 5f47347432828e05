// linear_xent.hip -- the logit-free MLM head: the vocabulary projection z = X W^T + bias fused with the softmax
// cross-entropy over its columns.  The (M, V) logits are never written: the forward keeps an online (max, sum-exp, label logit)
// per token row in registers while it walks the vocabulary, the backward recomputes the logits of one column chunk and writes the
// bf16 gradient G = dloss * (softmax - onehot) in both orientations for the two GEMMs that follow (dX += G W, dW = G^T X).
//
// One 256-thread workgroup owns a 128-row panel of X and one contiguous range of 128-column vocabulary tiles.  Per tile a bf16
// MFMA K-loop (v_mfma_f32_32x32x16_bf16, fp32 accumulate) runs over 64-wide k-slices of X and W that go through a double-buffered
// LDS ring; the ring is fed as ONE flat sequence of (tile, k-slice) steps, so the first slice of the next tile is fetched under the
// last MFMAs of this one and lands while the epilogue runs.  MFMA is issued as (A := W rows, B := X rows), as infonce.hip does: a
// lane then owns one token row per 32-row block and its accumulator registers run along the vocabulary, so max / sum-exp over a
// tile's columns are lane-local.  The two lane halves and the two waves that share a row are folded once, after the walk.
#include "cx_common.h"
#include "../../include/contrastors_hip.h"

namespace {

constexpr int LBM = 128, LBN = 128, LBK = 64;
constexpr int LPANEL = 128 * LBK * 2;   // 16 KiB: one operand's k-slice, 128 rows x 128 B (tile64_off layout)
constexpr int LX_TARGET_WG = 512;       // about two workgroups per CU
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

struct LxParams {
    const bf16_t* X; const bf16_t* W; const float* bias; const int64_t* labels;
    int M, V, K, ldx;
    long ignore_index;
    int tiles_m, nsplit;
    int col0, ntiles, vend;   // the walk: 128-column tiles from column col0; columns >= vend contribute nothing
    float* pmax; float* psum; float* plab;                                    // forward: (M, nsplit) partials, maxima in log2 units
    const float* lse; const float* dloss; bf16_t* G; bf16_t* GT; long ldg, ldgt;   // gradient
};

CX_DEVICE bool lx_ignored(long label, long ignore_index, int V) { return label == ignore_index || label < 0 || label >= V; }

// bias[n .. n+3] with the column tail guarded (n % 4 == 0, bias 16-byte aligned); NULL bias = zeros
CX_DEVICE float4 lx_bias4(const float* __restrict__ bias, int n, int V) {
    if (!bias) return make_float4(0.f, 0.f, 0.f, 0.f);
    if (n + 3 < V) return *reinterpret_cast<const float4*>(bias + n);
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n < V) b.x = bias[n];
    if (n + 1 < V) b.y = bias[n + 1];
    if (n + 2 < V) b.z = bias[n + 2];
    return b;
}

CX_DEVICE void lx_merge(float& m, float& s, float m2, float s2) {
    const float mm = fmaxf(m, m2);
    s = (mm == -INFINITY) ? 0.f : s * exp2f(m - mm) + s2 * exp2f(m2 - mm);
    m = mm;
}

// Tiles [t_begin, t_end) of the walk for the row panel at m0.  epi(acc, n0) runs once per tile with
//   acc[a][b][r] = sum_k W[n][k] X[m][k],   n = n0 + wn*64 + a*32 + acc_row(r, hi),   m = m0 + wm*64 + b*32 + l31
// (rows past M / V are clamped on the load: their values are finite and the epilogue drops them).
template <typename Epi>
CX_DEVICE void lx_walk(const LxParams& p, int m0, int t_begin, int t_end, char* smem, int tid, Epi&& epi) {
    const int lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31;
    const int wm = wave >> 1, wn = wave & 1;
    const int nk = p.K / LBK;
    const int sr = tid >> 3, sc = tid & 7;   // staging: rows sr + 32 i, 16-byte chunk sc of the 128-byte slice row

    size_t xoff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xoff[i] = (size_t)min(m0 + sr + 32 * i, p.M - 1) * p.ldx + sc * 8;

    uint4 sx[4], sw[4];
    auto stage = [&](int n0, int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sx[i] = *reinterpret_cast<const uint4*>(p.X + xoff[i] + k0);
            sw[i] = *reinterpret_cast<const uint4*>(p.W + (size_t)min(n0 + sr + 32 * i, p.V - 1) * p.K + sc * 8 + k0);
        }
    };
    auto commit = [&](char* buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<uint4*>(buf + tile64_off(sr + 32 * i, sc)) = sx[i];
            *reinterpret_cast<uint4*>(buf + LPANEL + tile64_off(sr + 32 * i, sc)) = sw[i];
        }
    };

    f32x16_t acc[2][2];
    auto clear = [&]() {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    };
    clear();

    stage(p.col0 + t_begin * LBN, 0);
    commit(smem);
    __syncthreads();

    const int total = (t_end - t_begin) * nk;
    int t = t_begin, kc = 0;
    for (int s = 0; s < total; ++s) {
        const char* cur = smem + (s & 1) * 2 * LPANEL;
        char* nxt = smem + ((s + 1) & 1) * 2 * LPANEL;
        int nkc = kc + 1, nt = t;
        if (nkc == nk) { nkc = 0; nt = t + 1; }
        if (s + 1 == total) { nkc = kc; nt = t; }   // the last slice is staged twice: the loop body stays branch-free
        stage(p.col0 + nt * LBN, nkc * LBK);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            bf16x8_t fx[2], fw[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                fx[j] = lds_read_frag(cur, tile64_off(wm * 64 + j * 32 + l31, 2 * ks + hi));
                fw[j] = lds_read_frag(cur + LPANEL, tile64_off(wn * 64 + j * 32 + l31, 2 * ks + hi));
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = mfma_bf16_32x32x16(fw[a], fx[b], acc[a][b]);
        }
        commit(nxt);   // nxt was read last in step s - 1, behind the barrier that ended it
        __syncthreads();
        if (kc == nk - 1) {
            epi(acc, p.col0 + t * LBN);
            clear();
        }
        kc = nkc;
        t = nt;
    }
}

CX_DEVICE void lx_coords(const LxParams& p, int& m0, int& t_begin, int& t_end) {
    // consecutive logical ids share a vocabulary range and differ in the row panel; xcd_remap gives each XCD a run of them, so
    // the workgroups that stream the same W tiles sit behind the same L2
    const int lid = xcd_remap(blockIdx.x, p.tiles_m * p.nsplit);
    const int tm = lid % p.tiles_m, sp = lid / p.tiles_m;
    m0 = tm * LBM;
    t_begin = (int)((long)sp * p.ntiles / p.nsplit);
    t_end = (int)((long)(sp + 1) * p.ntiles / p.nsplit);
}

__global__ __launch_bounds__(256, 2) void linxent_fwd_kernel(LxParams p) {
    __shared__ __attribute__((aligned(16))) char smem[4 * LPANEL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31;
    const int wm = wave >> 1, wn = wave & 1;
    int m0, t_begin, t_end;
    lx_coords(p, m0, t_begin, t_end);

    long label[2];
    float mx[2], sm[2], lab[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        label[b] = p.labels[min(m0 + wm * 64 + b * 32 + l31, p.M - 1)];
        mx[b] = -INFINITY; sm[b] = 0.f; lab[b] = 0.f;
    }

    lx_walk(p, m0, t_begin, t_end, smem, tid, [&](f32x16_t (&acc)[2][2], int n0) {
        float tmax[2] = {-INFINITY, -INFINITY};
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = n0 + wn * 64 + a * 32 + 8 * q + 4 * hi;
                const float4 b4 = lx_bias4(p.bias, n, p.V);
                const float bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float v = acc[a][b][4 * q + e] + bv[e];
                        if ((long)(n + e) == label[b]) lab[b] = v;   // (a label >= V never matches: the row is ignored)
                        const float z = (n + e) < p.vend ? v * LOG2E : -INFINITY;
                        acc[a][b][4 * q + e] = z;
                        tmax[b] = fmaxf(tmax[b], z);
                    }
            }
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            if (tmax[b] == -INFINITY) continue;   // none of this lane's 32 columns of the tile is below V
            const float nm = fmaxf(mx[b], tmax[b]);
            float s = sm[b] * exp2f(mx[b] - nm);
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) s += exp2f(acc[a][b][r] - nm);
            sm[b] = s;
            mx[b] = nm;
        }
    });

    // fold the two lane halves, then the two waves that share the row; the ring is free (lx_walk ends on a barrier)
    float* red = reinterpret_cast<float*>(smem);   // [wn][128 rows][3]
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        lx_merge(mx[b], sm[b], __shfl_xor(mx[b], 32, 64), __shfl_xor(sm[b], 32, 64));
        lab[b] += __shfl_xor(lab[b], 32, 64);
        if (hi == 0) {
            float* o = red + (wn * LBM + wm * 64 + b * 32 + l31) * 3;
            o[0] = mx[b]; o[1] = sm[b]; o[2] = lab[b];
        }
    }
    __syncthreads();
    if (tid < LBM && m0 + tid < p.M) {
        float m = red[tid * 3], s = red[tid * 3 + 1];
        lx_merge(m, s, red[(LBM + tid) * 3], red[(LBM + tid) * 3 + 1]);
        const int sp = xcd_remap(blockIdx.x, p.tiles_m * p.nsplit) / p.tiles_m;
        const size_t o = (size_t)(m0 + tid) * p.nsplit + sp;
        p.pmax[o] = m;
        p.psum[o] = s;
        p.plab[o] = red[tid * 3 + 2] + red[(LBM + tid) * 3 + 2];
    }
}

// one wave per row: the splits' partials in fixed order -> lse (natural log) and loss = lse - label logit (0 for ignored rows).
// At most one split saw the label column, the others hold 0: the sum of the label partials is exact in any order.
__global__ __launch_bounds__(256) void linxent_reduce_kernel(const float* __restrict__ pmax, const float* __restrict__ psum,
                                                             const float* __restrict__ plab, const int64_t* __restrict__ labels,
                                                             float* __restrict__ lse, float* __restrict__ loss, int M, int V,
                                                             int nsplit, long ignore_index) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const size_t o = (size_t)row * nsplit;
    float mx = -INFINITY;
    for (int i = lane; i < nsplit; i += 64) mx = fmaxf(mx, pmax[o + i]);
    mx = wave_max(mx);
    float s = 0.f, lb = 0.f;
    for (int i = lane; i < nsplit; i += 64) {
        const float pm = pmax[o + i];
        if (pm > -INFINITY) s += psum[o + i] * exp2f(pm - mx);
        lb += plab[o + i];
    }
    s = wave_sum(s);
    lb = wave_sum(lb);
    if (lane == 0) {
        const float l = (mx + log2f(s)) * LN2;
        lse[row] = l;
        loss[row] = lx_ignored(labels[row], ignore_index, V) ? 0.f : l - lb;
    }
}

// G[m][n - col0] = GT[n - col0][m] = bf16((exp(z - lse) - [n == label]) * dloss[m]) over whole tiles: ignored rows, rows >= M (GT
// only: G has M rows), columns >= vend are written as zeros.
__global__ __launch_bounds__(256, 2) void linxent_grad_kernel(LxParams p) {
    __shared__ __attribute__((aligned(16))) char smem[4 * LPANEL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31;
    const int wm = wave >> 1, wn = wave & 1;
    int m0, t_begin, t_end;
    lx_coords(p, m0, t_begin, t_end);

    long label[2];
    float lse2[2], dl[2];
    int mrow[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int m = m0 + wm * 64 + b * 32 + l31;
        const int mc = min(m, p.M - 1);
        mrow[b] = m;
        label[b] = p.labels[mc];
        lse2[b] = p.lse[mc] * LOG2E;
        dl[b] = (m < p.M && !lx_ignored(label[b], p.ignore_index, p.V)) ? p.dloss[mc] : 0.f;
    }

    lx_walk(p, m0, t_begin, t_end, smem, tid, [&](f32x16_t (&acc)[2][2], int n0) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = n0 + wn * 64 + a * 32 + 8 * q + 4 * hi;
                const int nl = n - p.col0;
                const float4 b4 = lx_bias4(p.bias, n, p.V);
                const float bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    float g[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float z = (acc[a][b][4 * q + e] + bv[e]) * LOG2E;
                        const float pr = exp2f(z - lse2[b]) - ((long)(n + e) == label[b] ? 1.f : 0.f);
                        g[e] = ((n + e) < p.vend && dl[b] != 0.f) ? pr * dl[b] : 0.f;
                    }
                    const uint32_t lo = pack_bf16x2(g[0], g[1]), hi2 = pack_bf16x2(g[2], g[3]);
                    if (mrow[b] < p.M) *reinterpret_cast<uint2*>(p.G + (size_t)mrow[b] * p.ldg + nl) = make_uint2(lo, hi2);
                    // 32 lanes of a half write 64 contiguous bytes of one GT row; the b = 0 / 1 pair completes its 128-byte line
                    p.GT[(size_t)nl * p.ldgt + mrow[b]] = (bf16_t)(lo & 0xffffu);
                    p.GT[(size_t)(nl + 1) * p.ldgt + mrow[b]] = (bf16_t)(lo >> 16);
                    p.GT[(size_t)(nl + 2) * p.ldgt + mrow[b]] = (bf16_t)(hi2 & 0xffffu);
                    p.GT[(size_t)(nl + 3) * p.ldgt + mrow[b]] = (bf16_t)(hi2 >> 16);
                }
            }
    });
}

// dbias[v] = sum_m GT[v][m] in a fixed order (lane-strided 16-byte loads, then the wave butterfly): the bias gradient of the chunk,
// bit-reproducible.  One wave per GT row; cols % 8 == 0.
__global__ __launch_bounds__(256) void linxent_dbias_kernel(const bf16_t* __restrict__ GT, float* __restrict__ dbias, int rows,
                                                            long cols, long ld) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const bf16_t* g = GT + (size_t)row * ld;
    float s = 0.f;
    for (long c = lane * 8; c < cols; c += 64 * 8) {
        float v[8];
        unpack8(*reinterpret_cast<const uint4*>(g + c), v);
        s += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    s = wave_sum(s);
    if (lane == 0) dbias[row] = s;
}

int lx_splits(int tiles_m, int ntiles) {
    const int s = (LX_TARGET_WG + tiles_m - 1) / tiles_m;
    return s < 1 ? 1 : (s > ntiles ? ntiles : s);
}

int lx_check(const void* X, const void* W, const float* bias, int M, int V, int K, int ldx) {
    if (M < 1 || V < 1 || K < 64 || K > 1024 || (K % 64) != 0 || ldx < K) return CX_ERR_SHAPE;
    if ((ldx % 8) != 0 || ((uintptr_t)X % 16) != 0 || ((uintptr_t)W % 16) != 0 || ((uintptr_t)bias % 16) != 0) return CX_ERR_ALIGN;
    return CX_OK;
}

void lx_fill(LxParams& p, const uint16_t* X, const uint16_t* W, const float* bias, const int64_t* labels, int M, int V, int K,
             int ldx, long ignore_index, int col0, int ncols) {
    p.X = X; p.W = W; p.bias = bias; p.labels = labels;
    p.M = M; p.V = V; p.K = K; p.ldx = ldx; p.ignore_index = ignore_index;
    p.tiles_m = (M + LBM - 1) / LBM;
    p.col0 = col0; p.ntiles = (ncols + LBN - 1) / LBN; p.vend = col0 + ncols;
    p.nsplit = lx_splits(p.tiles_m, p.ntiles);
}

}  // namespace

extern "C" {

long cx_linear_xent_ws_floats(int M, int V) {
    if (M < 1 || V < 1) return 0;
    return 3L * M * lx_splits((M + LBM - 1) / LBM, (V + LBN - 1) / LBN);
}

int cx_linear_xent_fwd(const uint16_t* X, const uint16_t* W, const float* bias, const int64_t* labels, float* ws, float* lse,
                       float* loss, int M, int V, int K, int ldx, long ignore_index, void* stream) {
    if (!X || !W || !labels || !ws || !lse || !loss) return CX_ERR_ARG;
    const int rc = lx_check(X, W, bias, M, V, K, ldx);
    if (rc != CX_OK) return rc;
    LxParams p = {};
    lx_fill(p, X, W, bias, labels, M, V, K, ldx, ignore_index, 0, V);
    const size_t sz = (size_t)M * p.nsplit;
    p.pmax = ws; p.psum = ws + sz; p.plab = ws + 2 * sz;
    hipLaunchKernelGGL(linxent_fwd_kernel, dim3(p.tiles_m * p.nsplit), dim3(256), 0, (hipStream_t)stream, p);
    if (hipGetLastError() != hipSuccess) return CX_ERR_LAUNCH;
    hipLaunchKernelGGL(linxent_reduce_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, p.pmax, p.psum, p.plab, labels,
                       lse, loss, M, V, p.nsplit, ignore_index);
    return done();
}

int cx_linear_xent_grad(const uint16_t* X, const uint16_t* W, const float* bias, const int64_t* labels, const float* lse,
                        const float* dloss, uint16_t* G, uint16_t* GT, float* dbias, int M, int V, int K, int ldx, int v0, int Vc,
                        long ignore_index, void* stream) {
    if (!X || !W || !labels || !lse || !dloss || !G || !GT) return CX_ERR_ARG;
    const int rc = lx_check(X, W, bias, M, V, K, ldx);
    if (rc != CX_OK) return rc;
    if (v0 < 0 || (v0 % LBN) != 0 || Vc < 1 || v0 + (long)Vc > V) return CX_ERR_SHAPE;
    if (((uintptr_t)G % 16) != 0 || ((uintptr_t)GT % 16) != 0) return CX_ERR_ALIGN;
    LxParams p = {};
    lx_fill(p, X, W, bias, labels, M, V, K, ldx, ignore_index, v0, Vc);
    p.lse = lse; p.dloss = dloss; p.G = G; p.GT = GT;
    p.ldg = (long)p.ntiles * LBN;
    p.ldgt = (long)p.tiles_m * LBM;
    hipLaunchKernelGGL(linxent_grad_kernel, dim3(p.tiles_m * p.nsplit), dim3(256), 0, (hipStream_t)stream, p);
    if (hipGetLastError() != hipSuccess) return CX_ERR_LAUNCH;
    if (dbias)
        hipLaunchKernelGGL(linxent_dbias_kernel, dim3((Vc + 3) / 4), dim3(256), 0, (hipStream_t)stream, GT, dbias, Vc, p.ldgt, p.ldgt);
    return done();
}

}  // extern "C"
