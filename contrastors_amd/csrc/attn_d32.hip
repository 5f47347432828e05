// attn_d32.hip -- non-causal variable-length self-attention at head_dim 32, forward and backward (the 384-wide, 12-head small
// encoders).  qkv (T, 3, H, 32) bf16; no rotary tables, no dropout, any max_seqlen: one streaming design for every length.
// Per-element arithmetic as attn_long.inc / attn_window.inc: scale folded into the exponent, exp2, P rounded to bf16 for PV,
// fp32 row sums, natural-log lse.  A translation unit of its own: the head_dim 64 kernels of attention.hip are untouched (the
// few helpers both use are copied here, not moved).
//
// What changes at d = 32, and what these kernels do about it:
//   * a head row is 64 bytes, and heads 2j, 2j + 1 of a token are ONE 128-byte run.  A workgroup owns a HEAD PAIR: its streamed
//     tiles (K / V, or Q / dO) are 64 rows x 128 bytes -- the tile64_off format the long kernels stage by LDS-DMA into a 2-deep
//     ring, one barrier per tile -- with head 2j in columns 0..31 and head 2j + 1 in columns 32..63.  Every line fetched is used
//     whole; out / dQ / dK / dV rows of the pair leave as 128-byte runs through the (dead) ring;
//   * a 32 x 32 score block costs 4 MFMAs here (8 at d = 64) under the same max / exp2 / sum / pack chain: the inner loop is
//     VALU-bound.  The two heads of the pair are a wave's two independent chains: head 0's MFMAs issue under head 1's softmax;
//   * the accumulators halve (O, dQ, dK, dV are one 32 x 32 block per head).  The registers go to occupancy: 32 rows per wave
//     and chain, three workgroups per CU in the backward kernels (the forward, both heads' scores live, stays at two);
//   * odd H: the last head has no partner.  Its workgroup clamps every load to the head's own 64 bytes (the DMA fetches logical
//     chunk c & 3: columns 32..63 of the tile hold a second copy of the head), chain 1 recomputes the same head and is dropped
//     at the stores, which write 64-byte runs.  Nothing outside a row's own bytes is read or written.
// 32x32x16 MFMAs, not 16x16x32: the softmax row stays in the lane dimension with 32 scores of a tile per lane and row-state
// update (16 with the 16-wide shape: twice the max / alpha / sum bookkeeping per score, two shuffle steps per row reduction
// instead of one), and S^T's accumulator registers feed PV's B operand as they are.
#include "cx_common.h"
#include "../../include/contrastors_hip.h"

namespace {

constexpr int D32 = 32;
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr int D32_TILE = 8192;                  // bytes of one 64-row x 128-byte tile (two heads side by side)
constexpr int D32_LDS = 4 * D32_TILE;           // two rings of two tiles
constexpr int D32_LDS_DKV = D32_LDS + 2048;     // + [slot][head][lse 64 | delta 64]

struct D32Params {
    const bf16_t* qkv;     // (T,3,H,32)
    const int32_t* cu;
    bf16_t* out;           // (T,H,32)
    float* lse;            // (H,T)
    const bf16_t* dout;    // (T,H,32)
    float* delta;          // (H,T)
    bf16_t* dqkv;          // (T,3,H,32)
    int H, T;
    float scale;
};

// (copies of attention.hip's helpers)
CX_DEVICE float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }   // v_exp_f32: a probability needs no denormal fix-ups

// accumulator registers 8*half .. 8*half+7 -> bf16 B fragment
CX_DEVICE bf16x8_t pack_frag(const float (&v)[16], int half) {
    union {
        uint32_t u[4];
        bf16x8_t v;
    } x;
#pragma unroll
    for (int e = 0; e < 4; ++e) x.u[e] = pack_bf16x2(v[8 * half + 2 * e], v[8 * half + 2 * e + 1]);
    return x.v;
}

// A-fragment of the TRANSPOSE of a row-major [t][64 f] tile (tile64_off layout) through the transposing LDS read: lane gets
// T[i = f0 + (lane & 31)][k = t0 + 4*hi + {0..3}, t0 + 8 + 4*hi + {0..3}], the reduction order of pack_frag's B fragment
typedef __attribute__((address_space(3))) bf16x4_t* lds_b4_t64;
CX_DEVICE bf16x8_t tile64_tr_frag(const char* tile, int f0, int t0, int lane) {
    const int g = lane >> 4, pp = lane & 15;
    const int t = t0 + 4 * (g >> 1) + (pp >> 2);
    const int f = f0 + 16 * (g & 1) + 4 * (pp & 3);
    union { bf16x4_t h[2]; bf16x8_t v; } u;
    u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b4_t64)(tile + tile64_off(t, f >> 3) + (f & 4) * 2));
    u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b4_t64)(tile + tile64_off(t + 8, f >> 3) + (f & 4) * 2));
    return u.v;
}

// One 1-KiB piece (8 rows x 128 B) of a 64-row tile by LDS-DMA, as long_dma_piece: lane L lands at row piece * 8 + (L >> 3),
// physical chunk L & 7, and fetches the logical chunk that tile64_off puts there -- masked with `cmask`: 7 for a head pair, 3 for
// a lone last head, whose second 64 bytes are a copy of its first (the row's own bytes only).  Rows past `nrows` re-read the last.
CX_DEVICE void d32_dma_piece(uint32_t lds_tile, int piece, const bf16_t* base, uint32_t row_stride_bytes, int row0, int nrows, int cmask,
                             int lane) {
    const int r = piece * 8 + (lane >> 3);
    const int c = ((lane & 7) ^ ((r >> 1) & 7)) & cmask;
    int rr = row0 + r;
    rr = rr < nrows ? rr : nrows - 1;
    const uint32_t off = (uint32_t)rr * row_stride_bytes + (uint32_t)c * 16u;
    const uint32_t m0v = lds_tile + piece * 1024;
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(m0v), "v"(off), "s"(base) : "memory");
}

// pieces {wave, wave + 4} of 64-row tile `tile` of two row-major operands into ring slot `slot`
CX_DEVICE void d32_request(uint32_t lds0, int slot, int wave, const bf16_t* a, uint32_t a_bytes, const bf16_t* b, uint32_t b_bytes, int tile,
                           int len, int cmask, int lane) {
    const uint32_t as = lds0 + slot * D32_TILE, bs = lds0 + (2 + slot) * D32_TILE;
    d32_dma_piece(as, wave, a, a_bytes, tile * 64, len, cmask, lane);
    d32_dma_piece(as, wave + 4, a, a_bytes, tile * 64, len, cmask, lane);
    d32_dma_piece(bs, wave, b, b_bytes, tile * 64, len, cmask, lane);
    d32_dma_piece(bs, wave + 4, b, b_bytes, tile * 64, len, cmask, lane);
}

// The two heads' 32 x 32 accumulator blocks (acc[hd]: element [column acc_row(r, hi)][row lane & 31]) times a per-lane factor,
// through a 4-KiB staging tile out as row runs of `nchunk` 16-byte chunks: 8 = the pair's 128 bytes, 4 = a lone head's 64.
CX_DEVICE void d32_store_rows(char* stage, bf16_t* g0, size_t row_stride, int rows_valid, int nchunk, const f32x16_t (&acc)[2], float mul0,
                              float mul1, int hi, int lane) {
    const int l31 = lane & 31;
#pragma unroll
    for (int hd = 0; hd < 2; ++hd) {
        const float mul = hd ? mul1 : mul0;
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            uint2 pk;
            pk.x = pack_bf16x2(acc[hd][4 * qd] * mul, acc[hd][4 * qd + 1] * mul);
            pk.y = pack_bf16x2(acc[hd][4 * qd + 2] * mul, acc[hd][4 * qd + 3] * mul);
            *reinterpret_cast<uint2*>(stage + tile64_off(l31, hd * 4 + qd) + hi * 8) = pk;
        }
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int r = it * 8 + (lane >> 3), c = lane & 7;
        const uint4 v = *reinterpret_cast<const uint4*>(stage + tile64_off(r, c));
        if (r < rows_valid && c < nchunk) *reinterpret_cast<uint4*>(g0 + (size_t)r * row_stride + c * 8) = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- forward
// 32 query rows per wave, 128 per workgroup, both heads of the pair; K / V tiles of 64 keys x 2 heads through the ring; Q never
// touches LDS (a lane's B fragments are 16-byte chunks of its own query row).
__global__ __launch_bounds__(256, 2) void attn_d32_fwd_kernel(D32Params p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h0 = blockIdx.y * 2, b = blockIdx.z;
    const bool pair = h0 + 1 < p.H;
    const int cmask = pair ? 7 : 3;
    const int t0 = p.cu[b], len = p.cu[b + 1] - t0;
    const int q0 = blockIdx.x * 128;
    if (q0 >= len) return;
    const size_t tok_stride = (size_t)3 * p.H * D32;
    const uint32_t tok_bytes = (uint32_t)tok_stride * 2u;
    const bf16_t* kbase = p.qkv + (size_t)(p.H + h0) * D32 + (size_t)t0 * tok_stride;
    const bf16_t* vbase = kbase + (size_t)p.H * D32;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)smem;
    const int wq0 = q0 + wave * 32;            // this wave's 32 query rows
    const bool wave_live = wq0 < len;

    d32_request(lds0, 0, wave, kbase, tok_bytes, vbase, tok_bytes, 0, len, cmask, lane);

    // Q fragments of both heads straight from global memory (rows past the end re-read the last row; a lone head twice)
    const int q = wq0 + l31;
    bf16x8_t qf[2][2];
    {
        const bf16_t* row = p.qkv + (size_t)(t0 + (q < len ? q : len - 1)) * tok_stride + (size_t)h0 * D32;
#pragma unroll
        for (int hd = 0; hd < 2; ++hd)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) qf[hd][ks] = *reinterpret_cast<const bf16x8_t*>(row + ((hd * 4 + ks * 2 + hi) & cmask) * 8);
    }

    const float sc2 = p.scale * LOG2E;
    float m_run[2] = {-1e30f, -1e30f}, l_run[2] = {0.f, 0.f};
    f32x16_t acc_o[2];
#pragma unroll
    for (int hd = 0; hd < 2; ++hd)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_o[hd][r] = 0.f;

    const int ntiles = (len + 63) >> 6;
#pragma unroll 1
    for (int t = 0; t < ntiles; ++t) {
        // this wave's pieces of tile t have landed (the Q loads are older and complete with them); then everybody's have, and
        // everybody is through tile t - 1: its slot may be refilled
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t + 1 < ntiles) d32_request(lds0, (t + 1) & 1, wave, kbase, tok_bytes, vbase, tok_bytes, t + 1, len, cmask, lane);
        if (!wave_live) continue;
        // (the lane index is made opaque per tile, as in attn_bwd_dq_long_kernel: the LDS addresses derived from it are invariant
        // across tiles, and kept in registers across the loop they spill)
        int lane_t = lane;
        asm volatile("" : "+v"(lane_t));
        const int lane = lane_t, hi = lane >> 5, l31 = lane & 31;
        const char* Ks = smem + (t & 1) * D32_TILE;
        const char* Vs = smem + (2 + (t & 1)) * D32_TILE;
        const int kv0 = t * 64;
        // ragged end (workgroup-uniform): a last tile whose second key block lies wholly past the sequence skips that block
        const bool kb1_live = kv0 + 32 < len;
        // Both heads' score blocks first, then head 0's softmax and PV, then head 1's: in this issue order head 1's score MFMAs
        // run under head 0's exponentials and head 0's PV MFMAs under head 1's.  The scheduling barriers keep that order.
        float s2[2][2][16];
#pragma unroll
        for (int hd = 0; hd < 2; ++hd)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                if (kb == 1 && !kb1_live) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) s2[hd][1][r] = -INFINITY;
                    continue;
                }
                f32x16_t a;
#pragma unroll
                for (int r = 0; r < 16; ++r) a[r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
                    a = mfma_bf16_32x32x16(lds_read_frag(Ks, tile64_off(kb * 32 + l31, hd * 4 + ks * 2 + hi)), qf[hd][ks], a);
#pragma unroll
                for (int r = 0; r < 16; ++r) s2[hd][kb][r] = a[r];
            }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int hd = 0; hd < 2; ++hd) {
            float (&s)[2][16] = s2[hd];
            if (kv0 + 64 > len) {   // the key mask exists only in a partial last tile (wave-uniform)
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (kv0 + kb * 32 + acc_row(r, hi) >= len) s[kb][r] = -INFINITY;
            }
            float mx = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kb][r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64)) * sc2;   // (sc2 > 0: the maximum commutes with the scale)
            // a row with no visible key in this tile keeps m_run (-1e30 at first: exp2(-inf + 1e30) = 0, never a NaN)
            const float m_new = fmaxf(m_run[hd], mx);
            const bool same = m_new == m_run[hd];
            const float alpha = fast_exp2(m_run[hd] - m_new);
            m_run[hd] = m_new;
            float psum = 0.f;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[kb][r] = fast_exp2(__builtin_fmaf(s[kb][r], sc2, -m_new));
                    psum += s[kb][r];
                }
            l_run[hd] = l_run[hd] * alpha + psum;
            // rescale O only when some row's running maximum moved (alpha == 1 exactly otherwise)
            if (!__all(same)) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc_o[hd][r] *= alpha;
            }
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                if (kb == 1 && !kb1_live) continue;
#pragma unroll
                for (int half = 0; half < 2; ++half)
                    acc_o[hd] = mfma_bf16_32x32x16(tile64_tr_frag(Vs, hd * 32, kb * 32 + half * 16, lane), pack_frag(s[kb], half), acc_o[hd]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    __syncthreads();   // every wave is through the last tile: the ring becomes the output staging area (4 KiB per wave)
    if (!wave_live) return;
    float inv[2];
#pragma unroll
    for (int hd = 0; hd < 2; ++hd) {
        const float l_tot = l_run[hd] + __shfl_xor(l_run[hd], 32, 64);
        inv[hd] = 1.f / l_tot;
        if (q < len && hi == 0 && (hd == 0 || pair)) p.lse[(size_t)(h0 + hd) * p.T + t0 + q] = (m_run[hd] + log2f(l_tot)) * LN2;
    }
    d32_store_rows(smem + wave * 4096, p.out + ((size_t)(t0 + wq0) * p.H + h0) * D32, (size_t)p.H * D32, len - wq0, pair ? 8 : 4, acc_o, inv[0],
                   inv[1], hi, lane);
}

// --------------------------------------------------------------------------------------------------------------- backward
// attn_d32_bwd_dq_kernel: the forward's work split; Q, dO and O fragments straight from global memory.  delta = rowsum(dO * O)
// is formed here from the dO chunks the lane holds anyway and written to p.delta for the dK / dV kernel, which runs second.
__global__ __launch_bounds__(256, 3) void attn_d32_bwd_dq_kernel(D32Params p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h0 = blockIdx.y * 2, b = blockIdx.z;
    const bool pair = h0 + 1 < p.H;
    const int cmask = pair ? 7 : 3;
    const int t0 = p.cu[b], len = p.cu[b + 1] - t0;
    const int q0 = blockIdx.x * 128;
    if (q0 >= len) return;
    const size_t tok_stride = (size_t)3 * p.H * D32, o_stride = (size_t)p.H * D32;
    const uint32_t tok_bytes = (uint32_t)tok_stride * 2u;
    const bf16_t* kbase = p.qkv + (size_t)(p.H + h0) * D32 + (size_t)t0 * tok_stride;
    const bf16_t* vbase = kbase + (size_t)p.H * D32;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)smem;
    const int wq0 = q0 + wave * 32;
    const bool wave_live = wq0 < len;

    d32_request(lds0, 0, wave, kbase, tok_bytes, vbase, tok_bytes, 0, len, cmask, lane);

    const int q = wq0 + l31;
    const int qc = q < len ? q : len - 1;
    bf16x8_t qf[2][2], dof[2][2];
    float lse2[2], dl[2];
    {
        const bf16_t* qrow = p.qkv + (size_t)(t0 + qc) * tok_stride + (size_t)h0 * D32;
        const bf16_t* dorow = p.dout + (size_t)(t0 + qc) * o_stride + (size_t)h0 * D32;
        const bf16_t* orow = p.out + (size_t)(t0 + qc) * o_stride + (size_t)h0 * D32;
#pragma unroll
        for (int hd = 0; hd < 2; ++hd) {
            float part = 0.f;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int c = (hd * 4 + ks * 2 + hi) & cmask;   // (a lone head: chain 1 re-reads the head's own chunks)
                qf[hd][ks] = *reinterpret_cast<const bf16x8_t*>(qrow + c * 8);
                const uint4 dv = *reinterpret_cast<const uint4*>(dorow + c * 8);
                const uint4 ov = *reinterpret_cast<const uint4*>(orow + c * 8);
                dof[hd][ks] = __builtin_bit_cast(bf16x8_t, dv);
                float a[8], o[8];
                unpack8(dv, a);
                unpack8(ov, o);
#pragma unroll
                for (int e = 0; e < 8; ++e) part += a[e] * o[e];
            }
            part += __shfl_xor(part, 32, 64);   // the other half of the row's 32 columns
            dl[hd] = part;
            const int hh = pair ? h0 + hd : h0;
            lse2[hd] = p.lse[(size_t)hh * p.T + t0 + qc] * LOG2E;
            if (wave_live && q < len && hi == 0 && (hd == 0 || pair)) p.delta[(size_t)hh * p.T + t0 + q] = part;
        }
    }
    const float sc2 = p.scale * LOG2E;
    f32x16_t acc_dq[2];
#pragma unroll
    for (int hd = 0; hd < 2; ++hd)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_dq[hd][r] = 0.f;

    const int ntiles = (len + 63) >> 6;
#pragma unroll 1
    for (int t = 0; t < ntiles; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (see attn_d32_fwd_kernel)
        __syncthreads();
        if (t + 1 < ntiles) d32_request(lds0, (t + 1) & 1, wave, kbase, tok_bytes, vbase, tok_bytes, t + 1, len, cmask, lane);
        if (!wave_live) continue;
        // (the lane index is made opaque per tile, as in attn_bwd_dq_long_kernel: the LDS addresses derived from it are invariant
        // across tiles, and kept in registers across the loop they spill)
        int lane_t = lane;
        asm volatile("" : "+v"(lane_t));
        const int lane = lane_t, hi = lane >> 5, l31 = lane & 31;
        const char* Ks = smem + (t & 1) * D32_TILE;
        const char* Vs = smem + (2 + (t & 1)) * D32_TILE;
        const int kv0 = t * 64;
        const bool full = kv0 + 64 <= len;
        const bool kb1_live = kv0 + 32 < len;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            if (kb == 1 && !kb1_live) continue;
#pragma unroll
            for (int hd = 0; hd < 2; ++hd) {
                f32x16_t a_s, a_dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) a_s[r] = a_dp[r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const int off = tile64_off(kb * 32 + l31, hd * 4 + ks * 2 + hi);
                    a_s = mfma_bf16_32x32x16(lds_read_frag(Ks, off), qf[hd][ks], a_s);
                    a_dp = mfma_bf16_32x32x16(lds_read_frag(Vs, off), dof[hd][ks], a_dp);
                }
                float ds[16];
                if (full) {  // (wave-uniform) no key mask
#pragma unroll
                    for (int r = 0; r < 16; ++r) ds[r] = fast_exp2(__builtin_fmaf(a_s[r], sc2, -lse2[hd]));
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = kv0 + kb * 32 + acc_row(r, hi);
                        ds[r] = key < len ? fast_exp2(__builtin_fmaf(a_s[r], sc2, -lse2[hd])) : 0.f;
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) ds[r] *= a_dp[r] - dl[hd];
#pragma unroll
                for (int half = 0; half < 2; ++half)
                    acc_dq[hd] = mfma_bf16_32x32x16(tile64_tr_frag(Ks, hd * 32, kb * 32 + half * 16, lane), pack_frag(ds, half), acc_dq[hd]);
            }
        }
    }
    __syncthreads();   // the ring becomes the staging area (4 KiB per wave)
    if (!wave_live) return;
    d32_store_rows(smem + wave * 4096, p.dqkv + (size_t)(t0 + wq0) * tok_stride + (size_t)h0 * D32, tok_stride, len - wq0, pair ? 8 : 4, acc_dq,
                   p.scale, p.scale, hi, lane);
}

// attn_d32_bwd_dkv_kernel: a workgroup owns 128 keys of a head pair (a wave 32: K / V fragments from global memory, dK / dV
// accumulators in registers); Q / dO tiles of 64 query rows x 2 heads through the ring, their transposes for the dK / dV products
// from the transposing LDS read; lse / delta of a tile and both heads through registers (requested one tile ahead) into a small
// ring.  Needs p.delta.  Every dK / dV row is written by exactly one wave: no atomics, the same bits every run.
__global__ __launch_bounds__(256, 3) void attn_d32_bwd_dkv_kernel(D32Params p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* ld_ring = reinterpret_cast<float*>(smem + D32_LDS);   // [slot][head][lse 64 | delta 64]
    const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h0 = blockIdx.y * 2, b = blockIdx.z;
    const bool pair = h0 + 1 < p.H;
    const int cmask = pair ? 7 : 3;
    const int t0 = p.cu[b], len = p.cu[b + 1] - t0;
    const int k0 = blockIdx.x * 128;
    if (k0 >= len) return;
    const size_t tok_stride = (size_t)3 * p.H * D32, o_stride = (size_t)p.H * D32;
    const uint32_t tok_bytes = (uint32_t)tok_stride * 2u, o_bytes = (uint32_t)o_stride * 2u;
    const bf16_t* qbase = p.qkv + (size_t)h0 * D32 + (size_t)t0 * tok_stride;
    const bf16_t* dobase = p.dout + (size_t)h0 * D32 + (size_t)t0 * o_stride;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)smem;
    const int wk0 = k0 + wave * 32;            // this wave's 32 keys
    const bool wave_keys = wk0 < len;
    // lse / delta of a tile: wave 0 fetches head 0's 64 rows, wave 1 head 1's (a lone head's again)
    const size_t ld_row = (size_t)(pair ? h0 + (wave & 1) : h0) * p.T + t0;   // (wave-uniform: scalar bases)

    float pf_lse = 0.f, pf_dl = 0.f;
#define CX_D32_REQUEST_Q(tile)                                                                                                 \
    do {                                                                                                                       \
        d32_request(lds0, (tile) & 1, wave, qbase, tok_bytes, dobase, o_bytes, (tile), len, cmask, lane);                      \
        if (tid < 128) {                                                                                                       \
            int r = (tile) * 64 + lane;                                                                                        \
            const bool ok = r < len;                                                                                           \
            r = ok ? r : len - 1;                                                                                              \
            pf_lse = ok ? p.lse[ld_row + r] * LOG2E : INFINITY; /* rows past the end: P = exp2(-inf) = 0 */                    \
            pf_dl = p.delta[ld_row + r];                                                                                       \
        }                                                                                                                      \
    } while (0)
    CX_D32_REQUEST_Q(0);

    const int key = wk0 + l31;
    const bool key_ok = key < len;
    const bool keys_full = k0 + 128 <= len;
    bf16x8_t kf[2][2], vf[2][2];
    {
        const bf16_t* krow = p.qkv + (size_t)(p.H + h0) * D32 + (size_t)(t0 + (key_ok ? key : len - 1)) * tok_stride;
#pragma unroll
        for (int hd = 0; hd < 2; ++hd)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int c = (hd * 4 + ks * 2 + hi) & cmask;
                kf[hd][ks] = *reinterpret_cast<const bf16x8_t*>(krow + c * 8);
                vf[hd][ks] = *reinterpret_cast<const bf16x8_t*>(krow + (size_t)p.H * D32 + c * 8);
            }
    }
    const float sc2 = p.scale * LOG2E;
    f32x16_t acc_dk[2], acc_dv[2];
#pragma unroll
    for (int hd = 0; hd < 2; ++hd)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_dk[hd][r] = acc_dv[hd][r] = 0.f;

    const int ntiles = (len + 63) >> 6;
#pragma unroll 1
    for (int t = 0; t < ntiles; ++t) {
        // lse / delta of tile t (requested with its DMA) into their slot, the DMA pieces landed, then everybody's
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tid < 128) {
            ld_ring[(t & 1) * 256 + (tid >> 6) * 128 + lane] = pf_lse;
            ld_ring[(t & 1) * 256 + (tid >> 6) * 128 + 64 + lane] = pf_dl;
        }
        __syncthreads();
        if (t + 1 < ntiles) CX_D32_REQUEST_Q(t + 1);
        if (!wave_keys) continue;   // (a wave whose 32 keys lie wholly past the sequence only feeds the ring)
        int lane_t = lane;   // (opaque per tile: see attn_d32_bwd_dq_kernel)
        asm volatile("" : "+v"(lane_t));
        const int lane = lane_t, hi = lane >> 5, l31 = lane & 31;
        const char* Qs = smem + (t & 1) * D32_TILE;
        const char* dOs = smem + (2 + (t & 1)) * D32_TILE;
        const int q0 = t * 64;
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            if (qb == 1 && q0 + 32 >= len) continue;   // (the last tile's second query block lies wholly past the sequence: P = 0)
#pragma unroll
            for (int hd = 0; hd < 2; ++hd) {
                const float* lse_s = ld_ring + (t & 1) * 256 + hd * 128;
                const float* dl_s = lse_s + 64;
                f32x16_t a_s, a_dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) a_s[r] = a_dp[r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const int off = tile64_off(qb * 32 + l31, hd * 4 + ks * 2 + hi);
                    a_s = mfma_bf16_32x32x16(lds_read_frag(Qs, off), kf[hd][ks], a_s);
                    a_dp = mfma_bf16_32x32x16(lds_read_frag(dOs, off), vf[hd][ks], a_dp);
                }
                // one 16-query half at a time (P and dS packed to bf16 as soon as they exist: 16 fewer live registers)
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    union { uint32_t u[4]; bf16x8_t v; } pf, dsf;
#pragma unroll
                    for (int g = 0; g < 2; ++g) {
                        const int qd = 2 * half + g, row = qb * 32 + 8 * qd + 4 * hi;
                        const float4 l4 = *reinterpret_cast<const float4*>(lse_s + row);
                        const float4 d4 = *reinterpret_cast<const float4*>(dl_s + row);
                        const float ll[4] = {l4.x, l4.y, l4.z, l4.w}, dd[4] = {d4.x, d4.y, d4.z, d4.w};
                        float pr[4], ds[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int r = 4 * qd + e;
                            const float pe = fast_exp2(__builtin_fmaf(a_s[r], sc2, -ll[e]));
                            pr[e] = (keys_full || key_ok) ? pe : 0.f;
                            ds[e] = pr[e] * (a_dp[r] - dd[e]);
                        }
                        pf.u[2 * g] = pack_bf16x2(pr[0], pr[1]);
                        pf.u[2 * g + 1] = pack_bf16x2(pr[2], pr[3]);
                        dsf.u[2 * g] = pack_bf16x2(ds[0], ds[1]);
                        dsf.u[2 * g + 1] = pack_bf16x2(ds[2], ds[3]);
                    }
                    acc_dv[hd] = mfma_bf16_32x32x16(tile64_tr_frag(dOs, hd * 32, qb * 32 + half * 16, lane), pf.v, acc_dv[hd]);
                    acc_dk[hd] = mfma_bf16_32x32x16(tile64_tr_frag(Qs, hd * 32, qb * 32 + half * 16, lane), dsf.v, acc_dk[hd]);
                }
            }
        }
    }
    __syncthreads();   // the ring becomes the staging area
    if (!wave_keys) return;
    bf16_t* kr0 = p.dqkv + (size_t)(p.H + h0) * D32 + (size_t)(t0 + wk0) * tok_stride;
    d32_store_rows(smem + wave * 4096, kr0, tok_stride, len - wk0, pair ? 8 : 4, acc_dk, p.scale, p.scale, hi, lane);
    d32_store_rows(smem + 16384 + wave * 4096, kr0 + (size_t)p.H * D32, tok_stride, len - wk0, pair ? 8 : 4, acc_dv, 1.f, 1.f, hi, lane);
}
#undef CX_D32_REQUEST_Q

}  // namespace

extern "C" {

// Self-attention at head_dim 32 (flash_attn_*_qkvpacked_func on (.., 3, H, 32)): one workgroup per 128 rows of a head pair.
int cx_attn_varlen_d32_fwd(const uint16_t* qkv, const int32_t* cu_seqlens, uint16_t* out, float* lse, int B, int H, int T, int max_seqlen,
                           float softmax_scale, void* stream) {
    if (B <= 0 || T <= 0 || max_seqlen <= 0) return CX_OK;
    if (!qkv || !cu_seqlens || !out || !lse || H <= 0) return CX_ERR_ARG;
    D32Params p = {};
    p.qkv = qkv; p.cu = cu_seqlens; p.out = out; p.lse = lse;
    p.H = H; p.T = T; p.scale = softmax_scale;
    hipLaunchKernelGGL(attn_d32_fwd_kernel, dim3((max_seqlen + 127) / 128, (H + 1) / 2, B), dim3(256), D32_LDS, (hipStream_t)stream, p);
    return done();
}

int cx_attn_varlen_d32_bwd(const uint16_t* dout, const uint16_t* qkv, const uint16_t* out, const float* lse, const int32_t* cu_seqlens,
                           float* delta, uint16_t* dqkv, int B, int H, int T, int max_seqlen, float softmax_scale, void* stream) {
    if (B <= 0 || T <= 0 || max_seqlen <= 0) return CX_OK;
    if (!dout || !qkv || !out || !lse || !cu_seqlens || !delta || !dqkv || H <= 0) return CX_ERR_ARG;
    D32Params p = {};
    p.qkv = qkv; p.cu = cu_seqlens;
    p.out = const_cast<uint16_t*>(out); p.lse = const_cast<float*>(lse);
    p.dout = dout; p.delta = delta; p.dqkv = dqkv;
    p.H = H; p.T = T; p.scale = softmax_scale;
    const dim3 grid((max_seqlen + 127) / 128, (H + 1) / 2, B);
    hipLaunchKernelGGL(attn_d32_bwd_dq_kernel, grid, dim3(256), D32_LDS, (hipStream_t)stream, p);
    hipLaunchKernelGGL(attn_d32_bwd_dkv_kernel, grid, dim3(256), D32_LDS_DKV, (hipStream_t)stream, p);
    return done();
}

}  // extern "C"
