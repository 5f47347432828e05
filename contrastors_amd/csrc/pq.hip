// pq.hip -- training and encoding of a product quantiser (faiss IndexPQ, 8 bits per sub-quantiser): the storage format of
// PQFlatIndex / cx_search_pq_topk (search.hip).  A row of width d is cut into m = d / dsub sub-vectors, dsub in {8, 16, 32, 64};
// sub-quantiser s has 256 centroids of width dsub.  Codebooks: fp32 masters (m, 256, dsub), their bf16 shadow (round to nearest
// even) and half_norm (m, 256) fp32.  ONLY the shadow is used to encode, decode or score.  tests/pq_ref.py is the contract:
//   half_norm[s][c] = 0.5f * h,  h = 0;  h = fmaf(c_j, c_j, h) for j ascending over the bf16 centroid widened to fp32
//   assign:  acc = 0;  acc = fmaf(x_j, c_j, acc) for j ascending over the sub-vector of the bf16 row;  score = acc - half_norm
//            (one fp32 subtraction);  code = the arg-max over c, ties to the lower c
//   update:  for each (s, c) the fp32 sum of the bf16 rows' sub-vectors whose code is c, element-wise in ascending row order;
//            master = sum / count where count > 0 (an empty cell keeps its master);  then shadow and half_norm again
// Every step is one correctly rounded fp32 operation, spelled (__builtin_fmaf, __fsub_rn, __fadd_rn, __fdiv_rn, __fmul_rn) so
// that no contraction choice is left to the compiler.  A code is a loop index in [0, 256): non-finite input cannot index out of
// range (a NaN score never wins; a row of NaNs gets code 0) and is otherwise unspecified.  No float atomics anywhere.
#include "cx_common.h"
#include "../../include/contrastors_hip.h"

namespace {

constexpr int KSUB = 256;
constexpr int MAX_UPDATE_ROWS = 1 << 24;   // (float)count is exact

CX_DEVICE float half_norm_of(const bf16_t* c, int dsub) {
    float h = 0.f;
    for (int j = 0; j < dsub; ++j) {
        const float v = bf16_to_f32(c[j]);
        h = __builtin_fmaf(v, v, h);
    }
    return __fmul_rn(0.5f, h);
}

__global__ __launch_bounds__(256) void pq_half_norm_kernel(const bf16_t* __restrict__ shadow, int cells, int dsub,
                                                           float* __restrict__ half_norm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < cells) half_norm[i] = half_norm_of(shadow + (int64_t)i * dsub, dsub);
}

// Workgroup (s, row block): the 256 x DSUB bf16 slice of sub-quantiser s (4 - 32 KiB) and its half-norms sit in LDS; a lane
// owns one row, keeps its sub-vector in registers and walks the 256 centroids, so that a wave's centroid reads are
// same-address broadcasts.  Codes leave as single bytes: any byte leading dimension >= m is legal, m = 1 and ldc == m included.
template <int DSUB, bool VEC>
__global__ __launch_bounds__(256) void pq_assign_kernel(const bf16_t* __restrict__ X, long ldx, long n,
                                                        const bf16_t* __restrict__ shadow, const float* __restrict__ half_norm,
                                                        uint8_t* __restrict__ codes, long ldc) {
    __shared__ __attribute__((aligned(16))) bf16_t cb[KSUB * DSUB];
    __shared__ float hn[KSUB];
    const int s = blockIdx.x, tid = threadIdx.x;
    const uint4* src = reinterpret_cast<const uint4*>(shadow + (int64_t)s * KSUB * DSUB);   // (the table is 16-B aligned)
    for (int i = tid; i < KSUB * DSUB / 8; i += 256) reinterpret_cast<uint4*>(cb)[i] = src[i];
    hn[tid] = half_norm[s * KSUB + tid];
    __syncthreads();
    const long nblocks = (n + 255) / 256;
    for (long rb = blockIdx.y; rb < nblocks; rb += gridDim.y) {
        const long row = rb * 256 + tid;
        if (row >= n) continue;   // (no barrier below)
        const bf16_t* xp = X + row * ldx + s * DSUB;
        float x[DSUB];
#pragma unroll
        for (int j0 = 0; j0 < DSUB; j0 += 8) {
            if constexpr (VEC) {
                float f[8];
                unpack8(*reinterpret_cast<const uint4*>(xp + j0), f);
#pragma unroll
                for (int e = 0; e < 8; ++e) x[j0 + e] = f[e];
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) x[j0 + e] = bf16_to_f32(xp[j0 + e]);
            }
        }
        float best = -INFINITY;
        int code = 0;
        for (int c = 0; c < KSUB; ++c) {
            float acc = 0.f;
#pragma unroll
            for (int j0 = 0; j0 < DSUB; j0 += 8) {
                float f[8];
                unpack8(*reinterpret_cast<const uint4*>(cb + c * DSUB + j0), f);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc = __builtin_fmaf(x[j0 + e], f[e], acc);
            }
            const float sc = __fsub_rn(acc, hn[c]);
            if (sc > best) { best = sc; code = c; }   // strict: ties stay with the lower c
        }
        codes[row * ldc + s] = (uint8_t)code;
    }
}

// Workgroup s, thread c: cell (s, c) walks the code column of sub-quantiser s in row order, UROWS rows at a time staged through
// LDS with their sub-vectors, and adds the rows of its code into DSUB fp32 registers.  Sequential on purpose: the order is the
// contract.  Then master, shadow and half-norm of the cell.
constexpr int UROWS = 256;

template <int DSUB, bool VEC>
__global__ __launch_bounds__(256) void pq_update_kernel(const bf16_t* __restrict__ X, long ldx, const uint8_t* __restrict__ codes,
                                                        long ldc, long n, float* __restrict__ masters, bf16_t* __restrict__ shadow,
                                                        float* __restrict__ half_norm) {
    __shared__ __attribute__((aligned(16))) bf16_t xs[UROWS * DSUB];
    __shared__ __attribute__((aligned(16))) uint8_t cs[UROWS];
    const int s = blockIdx.x, tid = threadIdx.x;
    float sum[DSUB];
#pragma unroll
    for (int j = 0; j < DSUB; ++j) sum[j] = 0.f;
    int count = 0;
    for (long r0 = 0; r0 < n; r0 += UROWS) {
        const long row = r0 + tid;
        if (row < n) {
            const bf16_t* xp = X + row * ldx + s * DSUB;
#pragma unroll
            for (int j0 = 0; j0 < DSUB; j0 += 8) {
                if constexpr (VEC) {
                    *reinterpret_cast<uint4*>(xs + tid * DSUB + j0) = *reinterpret_cast<const uint4*>(xp + j0);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) xs[tid * DSUB + j0 + e] = xp[j0 + e];
                }
            }
            cs[tid] = codes[row * ldc + s];
        }
        __syncthreads();
        const int rows = (int)min((long)UROWS, n - r0);
        for (int q = 0; q < rows; q += 16) {
            const uint4 cw = *reinterpret_cast<const uint4*>(cs + q);   // 16 codes, the same address for every lane
            const uint32_t w[4] = {cw.x, cw.y, cw.z, cw.w};
            uint32_t mine = 0;   // bit e: row q + e is in this cell
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (q + e < rows && ((w[e >> 2] >> ((e & 3) * 8)) & 0xff) == (uint32_t)tid) mine |= 1u << e;
            while (mine) {       // ascending e: ascending row order
                const int e = __builtin_ctz(mine);
                mine &= mine - 1;
                const bf16_t* xr = xs + (q + e) * DSUB;
#pragma unroll
                for (int j = 0; j < DSUB; ++j) sum[j] = __fadd_rn(sum[j], bf16_to_f32(xr[j]));
                ++count;
            }
        }
        __syncthreads();
    }
    const int64_t cell = (int64_t)s * KSUB + tid;
    float* mp = masters + cell * DSUB;
    bf16_t* sp = shadow + cell * DSUB;
    float h = 0.f;
#pragma unroll
    for (int j = 0; j < DSUB; ++j) {
        const float mj = count > 0 ? __fdiv_rn(sum[j], (float)count) : mp[j];
        if (count > 0) mp[j] = mj;
        const bf16_t b = f32_to_bf16(mj);
        sp[j] = b;
        const float v = bf16_to_f32(b);
        h = __builtin_fmaf(v, v, h);
    }
    half_norm[cell] = __fmul_rn(0.5f, h);
}

bool dsub_ok(int d, int dsub) {
    return d >= 64 && d <= 1024 && (d % 64) == 0 && (dsub == 8 || dsub == 16 || dsub == 32 || dsub == 64);
}

template <bool VEC>
void launch_assign(int dsub, dim3 grid, hipStream_t st, const bf16_t* X, long ldx, long n, const bf16_t* shadow,
                   const float* hn, uint8_t* codes, long ldc) {
    switch (dsub) {
        case 8: hipLaunchKernelGGL((pq_assign_kernel<8, VEC>), grid, dim3(256), 0, st, X, ldx, n, shadow, hn, codes, ldc); break;
        case 16: hipLaunchKernelGGL((pq_assign_kernel<16, VEC>), grid, dim3(256), 0, st, X, ldx, n, shadow, hn, codes, ldc); break;
        case 32: hipLaunchKernelGGL((pq_assign_kernel<32, VEC>), grid, dim3(256), 0, st, X, ldx, n, shadow, hn, codes, ldc); break;
        default: hipLaunchKernelGGL((pq_assign_kernel<64, VEC>), grid, dim3(256), 0, st, X, ldx, n, shadow, hn, codes, ldc); break;
    }
}

template <bool VEC>
void launch_update(int dsub, int m, hipStream_t st, const bf16_t* X, long ldx, const uint8_t* codes, long ldc, long n,
                   float* masters, bf16_t* shadow, float* hn) {
    const dim3 grid(m);
    switch (dsub) {
        case 8: hipLaunchKernelGGL((pq_update_kernel<8, VEC>), grid, dim3(256), 0, st, X, ldx, codes, ldc, n, masters, shadow, hn); break;
        case 16: hipLaunchKernelGGL((pq_update_kernel<16, VEC>), grid, dim3(256), 0, st, X, ldx, codes, ldc, n, masters, shadow, hn); break;
        case 32: hipLaunchKernelGGL((pq_update_kernel<32, VEC>), grid, dim3(256), 0, st, X, ldx, codes, ldc, n, masters, shadow, hn); break;
        default: hipLaunchKernelGGL((pq_update_kernel<64, VEC>), grid, dim3(256), 0, st, X, ldx, codes, ldc, n, masters, shadow, hn); break;
    }
}

}  // namespace

extern "C" {

int cx_pq_half_norm(const uint16_t* shadow, int d, int dsub, float* half_norm, void* stream) {
    if (!dsub_ok(d, dsub)) return CX_ERR_SHAPE;
    if (!shadow || !half_norm) return CX_ERR_ARG;
    const int cells = d / dsub * KSUB;
    hipLaunchKernelGGL(pq_half_norm_kernel, dim3((cells + 255) / 256), dim3(256), 0, (hipStream_t)stream, shadow, cells, dsub,
                       half_norm);
    return done();
}

int cx_pq_assign(const uint16_t* X, long n, int d, long ldx, const uint16_t* shadow, const float* half_norm, int dsub,
                 uint8_t* codes, long ldc, void* stream) {
    if (n < 0 || !dsub_ok(d, dsub)) return CX_ERR_SHAPE;
    if (n == 0) return CX_OK;
    if (!X || !shadow || !half_norm || !codes) return CX_ERR_ARG;
    const int m = d / dsub;
    if (ldx < d || ldc < m || ((uintptr_t)X & 1) || ((uintptr_t)shadow & 15) || ((uintptr_t)half_norm & 3)) return CX_ERR_ALIGN;
    // eight elements per load where every sub-vector is aligned for it, element loads otherwise
    const bool vec = (ldx % 8) == 0 && ((uintptr_t)X & 15) == 0;
    const long nblocks = (n + 255) / 256;
    const dim3 grid(m, (unsigned)min(nblocks, 65535L));
    if (vec) launch_assign<true>(dsub, grid, (hipStream_t)stream, X, ldx, n, shadow, half_norm, codes, ldc);
    else launch_assign<false>(dsub, grid, (hipStream_t)stream, X, ldx, n, shadow, half_norm, codes, ldc);
    return done();
}

int cx_pq_update(const uint16_t* X, long n, int d, long ldx, const uint8_t* codes, long ldc, int dsub, float* masters,
                 uint16_t* shadow, float* half_norm, void* stream) {
    if (n < 0 || n > MAX_UPDATE_ROWS || !dsub_ok(d, dsub)) return CX_ERR_SHAPE;
    if (n == 0) return CX_OK;
    if (!X || !codes || !masters || !shadow || !half_norm) return CX_ERR_ARG;
    const int m = d / dsub;
    if (ldx < d || ldc < m || ((uintptr_t)X & 1) || ((uintptr_t)masters & 3) || ((uintptr_t)shadow & 1) ||
        ((uintptr_t)half_norm & 3))
        return CX_ERR_ALIGN;
    const bool vec = (ldx % 8) == 0 && ((uintptr_t)X & 15) == 0;
    if (vec) launch_update<true>(dsub, m, (hipStream_t)stream, X, ldx, codes, ldc, n, masters, shadow, half_norm);
    else launch_update<false>(dsub, m, (hipStream_t)stream, X, ldx, codes, ldc, n, masters, shadow, half_norm);
    return done();
}

}  // extern "C"
