// attn_alibi.inc -- self-attention with ALiBi (flash-attn's alibi_slopes, non-causal), forward and backward (included by
// attention.hip inside its namespace, after attn_window.inc: shares AttnParams, the tile64 helpers, long_dma_piece and
// window_request).  For query row i and key j of one sequence, head h of batch entry b:
//     s_ij = scale * (q_i . k_j) - slope[b, h] * |i - j|,   out = softmax(s) V,   lse = logsumexp_j s_ij (the bias is inside).
// The backward recomputes the same P; the slopes get no gradient.  head_dim 64, bf16, variable length, any max_seqlen (one
// streaming design for every length), no rotate-on-load, no dropout.  Work split and data movement are the long kernels'
// (attn_long.inc): 64 query rows per wave and 256 per workgroup in the forward and dQ kernels, 32 keys per wave and 128 per
// workgroup in the dK / dV kernel; the streamed operand in 64-row tiles by LDS-DMA into the 2-deep ring, one barrier per tile,
// the next tile requested right behind it; the resident operand straight from global memory into fragments; results leave as
// whole 128-byte rows through the dead ring.  Per-element arithmetic after the scores as the long kernels (scale folded into
// the exponent, exp2, P rounded to bf16 for PV, fp32 row sums, lse natural log).
//
// Where the bias lives:
//   1. In the INITIAL VALUE of the score accumulator.  The score MFMA chain computes C = A B + C_in; the long kernels zero
//      C_in (16 v_mov per 32 x 32 block).  Here C_in = -(slope / scale) * |i - j|, so the chain leaves q . k - (slope / scale)
//      |i - j| and the existing fma(s, scale * log2e, -m) yields the biased exponent: the max / exp2 / sum / pack chain gains
//      no instruction.  (scale > 0 is assumed, as the maximum already assumes; the host refuses anything else.)  In the
//      accumulator layout one index of (i, j) is the lane's and the other is acc_row(r, hi) = rowoff(r) + 4 hi, rowoff a
//      compile-time constant per register: |i - j| = |d - rowoff(r)| with ONE d per lane and block.
//   2. Sign-resolved blocks.  Row blocks and key blocks are both 32-aligned, so a 32 x 32 block is either the diagonal block
//      of its rows or lies wholly on one side of the diagonal (a wave-uniform test on the two block starts).  Off the
//      diagonal C_in[r] = fma(+-ns, rowoff(r), -+ns * d): one v_fma per element on a per-lane base (packed: half an
//      instruction per score -- the long kernels' zero costs none, their first MFMA takes the inline constant).  Only the one diagonal block per 32 rows and walk takes |d - rowoff(r)| (a subtract, and a multiply with
//      the absolute-value source modifier).  The ragged-end key mask of a partial last tile stays as in the long kernels.
//   3. A head whose slope is 0 zero-initialises (a wave-uniform test on the slope, loaded once per workgroup): its arithmetic
//      is the plain long kernels', and a batch of mixed slopes pays for the bias only where it has one.
// The bias is formed in fp32 beside fp32 dot products.  Row distances are exact (the host refuses max_seqlen >= 2^24); the
// product with slope / scale is rounded once or twice.  At 8192 tokens and slope 0.5 the far-field term is about 3e4 before
// the scale, where one fp32 ulp times scale = 1 / 8 is about 5e-4 in the score -- of a key whose weight is exp(-4096).

// C_in of one 32 x 32 score block.  ns = slope / scale (wave-uniform), d = this lane's (own index) - (first index of the
// block's register dimension) - 4 * hi, so that |i - j| = |d - rowoff(r)|; rk = (lane dimension's block start) - (register
// dimension's block start), wave-uniform and a multiple of 32.
CX_DEVICE void alibi_acc_init(f32x16_t& a, float ns, int d, int rk) {
    if (ns == 0.f) {   // point 3
#pragma unroll
        for (int r = 0; r < 16; ++r) a[r] = 0.f;
    } else if (rk != 0) {   // point 2: every d - rowoff(r) of the block has the sign of rk
        const float m = rk > 0 ? ns : -ns, base = -m * (float)d;
#pragma unroll
        for (int r = 0; r < 16; ++r) a[r] = __builtin_fmaf(m, (float)acc_row(r, 0), base);
    } else {                // the diagonal block
        const float df = (float)d;
#pragma unroll
        for (int r = 0; r < 16; ++r) a[r] = -ns * __builtin_fabsf(df - (float)acc_row(r, 0));
    }
}

// slope / scale of this workgroup's (sequence, head), in an SGPR
CX_DEVICE float alibi_ns(const float* slopes, int sstride, int b, int h, float scale) {
    const float ns = slopes[(size_t)b * sstride + h] / scale;
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, ns)));
}

__global__ __launch_bounds__(256, 2) void attn_fwd_alibi_kernel(AttnParams p, const float* slopes, int sstride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.y, b = blockIdx.z;
    const int t0 = p.cu[b], len = p.cu[b + 1] - t0;
    const int q0 = blockIdx.x * 256;
    if (q0 >= len) return;
    const size_t tok_stride = (size_t)3 * p.H * DH;
    const uint32_t tok_bytes = (uint32_t)tok_stride * 2u;
    const bf16_t* qbase = p.qkv + (size_t)h * DH;
    const bf16_t* kbase = qbase + (size_t)p.H * DH + (size_t)t0 * tok_stride;
    const bf16_t* vbase = kbase + (size_t)p.H * DH;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)smem;
    const int wq0 = q0 + wave * 64;            // this wave's 64 query rows
    const bool wave_live = wq0 < len;
    const float ns = alibi_ns(slopes, sstride, b, h, p.scale);

    window_request(lds0, 0, wave, kbase, tok_bytes, vbase, tok_bytes, 0, len, lane);

    // Q fragments of the two query blocks straight from global memory (rows past the end re-read the last row)
    bf16x8_t qf[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        int q = wq0 + j * 32 + l31;
        q = q < len ? q : len - 1;
        const bf16_t* row = qbase + (size_t)(t0 + q) * tok_stride;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[j][ks] = *reinterpret_cast<const bf16x8_t*>(row + (ks * 2 + hi) * 8);
    }

    const float sc2 = p.scale * LOG2E;
    float m_run[2] = {-1e30f, -1e30f}, l_run[2] = {0.f, 0.f};
    f32x16_t acc_o[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc_o[j][db][r] = 0.f;

    const int ntiles = (len + 63) >> 6;
#pragma unroll 1
    for (int t = 0; t < ntiles; ++t) {
        // this wave's pieces of tile t have landed, then everybody's have, and everybody is through tile t - 1 (see attn_fwd_long_kernel)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t + 1 < ntiles) window_request(lds0, (t + 1) & 1, wave, kbase, tok_bytes, vbase, tok_bytes, t + 1, len, lane);
        if (!wave_live) continue;
        const char* Ks = smem + (t & 1) * LONG_TILE;
        const char* Vs = smem + (2 + (t & 1)) * LONG_TILE;
        const int kv0 = t * 64;
        const int dq = wq0 + l31 - 4 * hi - kv0;   // (query row) - (first key of the tile) - 4 hi

        // ragged end (workgroup-uniform): a last tile whose second key block lies wholly past the sequence skips that block's products
        const bool kb1_live = kv0 + 32 < len;
        float s[2][2][16];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            if (kb == 1 && !kb1_live) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[0][1][r] = s[1][1][r] = -INFINITY;
                continue;
            }
            const int rk = wq0 - kv0 - kb * 32;   // (first row of query block 0) - (first key of the block)
            f32x16_t a0, a1;
            alibi_acc_init(a0, ns, dq - kb * 32, rk);
            alibi_acc_init(a1, ns, dq + 32 - kb * 32, rk + 32);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8_t kf = lds_read_frag(Ks, tile64_off(kb * 32 + l31, ks * 2 + hi));
                a0 = mfma_bf16_32x32x16(kf, qf[0][ks], a0);
                a1 = mfma_bf16_32x32x16(kf, qf[1][ks], a1);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[0][kb][r] = a0[r];
                s[1][kb][r] = a1[r];
            }
        }
        if (kv0 + 64 > len) {   // the key mask exists only in a partial last tile (wave-uniform)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (kv0 + kb * 32 + acc_row(r, hi) >= len) s[j][kb][r] = -INFINITY;
        }
        float alpha[2];
        bool same = true;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float mx = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[j][kb][r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64)) * sc2;   // (sc2 > 0: the maximum commutes with the scale)
            const float m_new = fmaxf(m_run[j], mx);
            same = same && (m_new == m_run[j]);
            alpha[j] = fast_exp2(m_run[j] - m_new);
            m_run[j] = m_new;
            float psum = 0.f;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[j][kb][r] = fast_exp2(__builtin_fmaf(s[j][kb][r], sc2, -m_new));
                    psum += s[j][kb][r];
                }
            l_run[j] = l_run[j] * alpha[j] + psum;
        }
        // rescale O only when some row's running maximum moved (alpha == 1 exactly otherwise).  Under a bias the maximum of a row
        // climbs while the walk approaches its diagonal and rests once past it.
        if (!__all(same)) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int db = 0; db < 2; ++db)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc_o[j][db][r] *= alpha[j];
        }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            if (kb == 1 && !kb1_live) continue;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const bf16x8_t p0 = pack_frag(s[0][kb], half), p1 = pack_frag(s[1][kb], half);
#pragma unroll
                for (int db = 0; db < 2; ++db) {
                    const bf16x8_t vf = tile64_tr_frag(Vs, db * 32, kb * 32 + half * 16, lane);
                    acc_o[0][db] = mfma_bf16_32x32x16(vf, p0, acc_o[0][db]);
                    acc_o[1][db] = mfma_bf16_32x32x16(vf, p1, acc_o[1][db]);
                }
            }
        }
    }

    __syncthreads();   // every wave is through the last tile: the ring becomes the output staging area (8 KiB per wave)
    if (!wave_live) return;
    char* stage = smem + wave * 8192;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float l_tot = l_run[j] + __shfl_xor(l_run[j], 32, 64);
        const float inv = 1.f / l_tot;
        const int qb0 = wq0 + j * 32;
        if (qb0 >= len) break;
        const int q = qb0 + l31;
        char* st = stage + j * 4096;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                uint2 pk;
                pk.x = pack_bf16x2(acc_o[j][db][4 * qd] * inv, acc_o[j][db][4 * qd + 1] * inv);
                pk.y = pack_bf16x2(acc_o[j][db][4 * qd + 2] * inv, acc_o[j][db][4 * qd + 3] * inv);
                *reinterpret_cast<uint2*>(st + tile64_off(l31, db * 4 + qd) + hi * 8) = pk;
            }
        if (q < len && hi == 0) p.lse[(size_t)h * p.T + t0 + q] = (m_run[j] + log2f(l_tot)) * LN2;
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int r = it * 8 + (lane >> 3), c = lane & 7;
            const int qq = qb0 + r;
            const uint4 v = *reinterpret_cast<const uint4*>(st + tile64_off(r, c));
            if (qq < len) *reinterpret_cast<uint4*>(p.out + ((size_t)(t0 + qq) * p.H + h) * DH + c * 8) = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- backward
// attn_bwd_dq_alibi_kernel: the forward's work split; Q and dO fragments straight from global memory; a tile's K / V fragments
// are read once and serve both query blocks.  P is recomputed through the same accumulator initial value, the dP chain starts
// from 0.  delta = rowsum(dO * O) is formed from the dO chunks the lane holds anyway and written to p.delta for the dK / dV
// kernel, which therefore runs second.
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_alibi_kernel(AttnParams p, const float* slopes, int sstride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.y, b = blockIdx.z;
    const int t0 = p.cu[b], len = p.cu[b + 1] - t0;
    const int q0 = blockIdx.x * 256;
    if (q0 >= len) return;
    const size_t tok_stride = (size_t)3 * p.H * DH, o_stride = (size_t)p.H * DH;
    const uint32_t tok_bytes = (uint32_t)tok_stride * 2u;
    const bf16_t* qbase = p.qkv + (size_t)h * DH;
    const bf16_t* kbase = qbase + (size_t)p.H * DH + (size_t)t0 * tok_stride;
    const bf16_t* vbase = kbase + (size_t)p.H * DH;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)smem;
    const int wq0 = q0 + wave * 64;
    const bool wave_live = wq0 < len;
    const float ns = alibi_ns(slopes, sstride, b, h, p.scale);

    window_request(lds0, 0, wave, kbase, tok_bytes, vbase, tok_bytes, 0, len, lane);

    bf16x8_t qf[2][4], dof[2][4];
    float lse2[2], dl[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = wq0 + j * 32 + l31;
        const int qc = q < len ? q : len - 1;
        const bf16_t* qrow = qbase + (size_t)(t0 + qc) * tok_stride;
        const bf16_t* dorow = p.dout + (size_t)(t0 + qc) * o_stride + (size_t)h * DH;
        const bf16_t* orow = p.out + (size_t)(t0 + qc) * o_stride + (size_t)h * DH;
        float part = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            qf[j][ks] = *reinterpret_cast<const bf16x8_t*>(qrow + (ks * 2 + hi) * 8);
            const uint4 dv = *reinterpret_cast<const uint4*>(dorow + (ks * 2 + hi) * 8);
            const uint4 ov = *reinterpret_cast<const uint4*>(orow + (ks * 2 + hi) * 8);
            dof[j][ks] = __builtin_bit_cast(bf16x8_t, dv);
            float a[8], c[8];
            unpack8(dv, a);
            unpack8(ov, c);
#pragma unroll
            for (int e = 0; e < 8; ++e) part += a[e] * c[e];
        }
        part += __shfl_xor(part, 32, 64);   // the other half of the row's 64 columns
        dl[j] = part;
        lse2[j] = p.lse[(size_t)h * p.T + t0 + qc] * LOG2E;
        if (wave_live && q < len && hi == 0) p.delta[(size_t)h * p.T + t0 + q] = part;
    }
    const float sc2 = p.scale * LOG2E;
    f32x16_t acc_dq[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc_dq[j][db][r] = 0.f;

    const int ntiles = (len + 63) >> 6;
#pragma unroll 1
    for (int t = 0; t < ntiles; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (see attn_fwd_long_kernel)
        __syncthreads();
        if (t + 1 < ntiles) window_request(lds0, (t + 1) & 1, wave, kbase, tok_bytes, vbase, tok_bytes, t + 1, len, lane);
        if (!wave_live) continue;
        // (the lane index is made opaque per tile, as in attn_bwd_dq_long_kernel: what derives from it is invariant across tiles
        // and kept in registers across the loop it spills)
        int lane_t = lane;
        asm volatile("" : "+v"(lane_t));
        const int lane = lane_t, hi = lane >> 5, l31 = lane & 31;
        const char* Ks = smem + (t & 1) * LONG_TILE;
        const char* Vs = smem + (2 + (t & 1)) * LONG_TILE;
        const int kv0 = t * 64;
        const int dq = wq0 + l31 - 4 * hi - kv0;
        const bool full = kv0 + 64 <= len;
        const bool kb1_live = kv0 + 32 < len, j1_live = wq0 + 32 < len;   // ragged ends, wave-uniform
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            if (kb == 1 && !kb1_live) continue;
            bf16x8_t kf[4], vf[4];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                kf[ks] = lds_read_frag(Ks, tile64_off(kb * 32 + l31, ks * 2 + hi));
                vf[ks] = lds_read_frag(Vs, tile64_off(kb * 32 + l31, ks * 2 + hi));
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (j == 1 && !j1_live) continue;
                // S first, turned into P in place; then dP (its MFMAs are independent of the exponentials: they overlap)
                f32x16_t a_s;
                alibi_acc_init(a_s, ns, dq + (j - kb) * 32, wq0 - kv0 + (j - kb) * 32);
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) a_s = mfma_bf16_32x32x16(kf[ks], qf[j][ks], a_s);
                float ds[16];
                if (full) {  // (wave-uniform) no key mask
#pragma unroll
                    for (int r = 0; r < 16; ++r) ds[r] = fast_exp2(__builtin_fmaf(a_s[r], sc2, -lse2[j]));
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = kv0 + kb * 32 + acc_row(r, hi);
                        ds[r] = key < len ? fast_exp2(__builtin_fmaf(a_s[r], sc2, -lse2[j])) : 0.f;
                    }
                }
                f32x16_t a_dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) a_dp[r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) a_dp = mfma_bf16_32x32x16(vf[ks], dof[j][ks], a_dp);
#pragma unroll
                for (int r = 0; r < 16; ++r) ds[r] *= a_dp[r] - dl[j];
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const bf16x8_t dsf = pack_frag(ds, half);
#pragma unroll
                    for (int db = 0; db < 2; ++db)   // (K^T fragments re-read per query block, as in attn_bwd_dq_long_kernel)
                        acc_dq[j][db] = mfma_bf16_32x32x16(tile64_tr_frag(Ks, db * 32, kb * 32 + half * 16, lane), dsf, acc_dq[j][db]);
                }
            }
        }
    }
    __syncthreads();   // the ring becomes the staging area (the two blocks of a wave leave one after the other)
    if (!wave_live) return;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int qb0 = wq0 + j * 32;
        if (qb0 >= len) break;
        store_unrotated_rows(smem + wave * 8192 + j * 4096, p.dqkv + (size_t)(t0 + qb0) * tok_stride + (size_t)h * DH, tok_stride, len - qb0,
                             acc_dq[j], p.scale, nullptr, nullptr, 0, hi, lane);
    }
}

// attn_bwd_dkv_alibi_kernel: a workgroup owns 128 keys (a wave 32: K / V fragments straight from global memory, dK / dV
// accumulators in registers), Q / dO tiles of 64 query rows by LDS-DMA into the ring, lse / delta of a tile through registers
// (requested one tile ahead) into a small ring.  Here the lane holds the KEY and the register the query: the same initial
// value with the roles of the two indices exchanged (|i - j| is symmetric).  Needs p.delta.
__global__ __launch_bounds__(256, 3) void attn_bwd_dkv_alibi_kernel(AttnParams p, const float* slopes, int sstride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* ld_ring = reinterpret_cast<float*>(smem + 4 * LONG_TILE);   // [slot][lse 64 | delta 64]
    const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.y, b = blockIdx.z;
    const int t0 = p.cu[b], len = p.cu[b + 1] - t0;
    const int k0 = blockIdx.x * 128;
    if (k0 >= len) return;
    const size_t tok_stride = (size_t)3 * p.H * DH, o_stride = (size_t)p.H * DH;
    const uint32_t tok_bytes = (uint32_t)tok_stride * 2u, o_bytes = (uint32_t)o_stride * 2u;
    const bf16_t* qbase = p.qkv + (size_t)h * DH + (size_t)t0 * tok_stride;
    const bf16_t* dobase = p.dout + (size_t)h * DH + (size_t)t0 * o_stride;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)smem;
    const float ns = alibi_ns(slopes, sstride, b, h, p.scale);

    float pf_lse = 0.f, pf_dl = 0.f;
#define CX_ALIBI_REQUEST_Q(tile)                                                                                               \
    do {                                                                                                                       \
        window_request(lds0, (tile) & 1, wave, qbase, tok_bytes, dobase, o_bytes, (tile), len, lane);                          \
        if (tid < 64) {                                                                                                        \
            int r = (tile) * 64 + tid;                                                                                         \
            const bool ok = r < len;                                                                                           \
            r = ok ? r : len - 1;                                                                                              \
            pf_lse = ok ? p.lse[(size_t)h * p.T + t0 + r] * LOG2E : INFINITY; /* rows past the end: P = exp2(-inf) = 0 */      \
            pf_dl = p.delta[(size_t)h * p.T + t0 + r];                                                                         \
        }                                                                                                                      \
    } while (0)
    CX_ALIBI_REQUEST_Q(0);

    const int wk0 = k0 + wave * 32;            // this wave's 32 keys
    const int key = wk0 + l31;
    const bool key_ok = key < len;
    const bool keys_full = k0 + 128 <= len;
    const bool wave_keys = wk0 < len;
    bf16x8_t kf[4], vf[4];
    {
        // (an opaque copy of the lane index: the chunk offset formed from it here is not the one the stores form after the loop,
        // which was otherwise carried over the loop in a register the loop does not have -- the only scratch use of the kernel)
        int lane_p = lane;
        asm volatile("" : "+v"(lane_p));
        const int hi_p = lane_p >> 5;
        const int kc = key_ok ? key : len - 1;
        const bf16_t* krow = p.qkv + (size_t)(p.H + h) * DH + (size_t)(t0 + kc) * tok_stride;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            kf[ks] = *reinterpret_cast<const bf16x8_t*>(krow + (ks * 2 + hi_p) * 8);
            vf[ks] = *reinterpret_cast<const bf16x8_t*>(krow + (size_t)p.H * DH + (ks * 2 + hi_p) * 8);
        }
    }
    const float sc2 = p.scale * LOG2E;
    f32x16_t acc_dk[2], acc_dv[2];
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_dk[db][r] = acc_dv[db][r] = 0.f;

    const int ntiles = (len + 63) >> 6;
#pragma unroll 1
    for (int t = 0; t < ntiles; ++t) {
        // lse / delta of tile t (requested with its DMA) into their slot, the DMA pieces landed, then everybody's
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tid < 64) {
            ld_ring[(t & 1) * 128 + tid] = pf_lse;
            ld_ring[(t & 1) * 128 + 64 + tid] = pf_dl;
        }
        __syncthreads();
        if (t + 1 < ntiles) CX_ALIBI_REQUEST_Q(t + 1);
        if (!wave_keys) continue;   // (a wave whose 32 keys lie wholly past the sequence only feeds the ring)
        // (the lane index is made opaque per tile, as in attn_bwd_dkv_window_kernel: the LDS addresses and the bias base derived
        // from it are invariant across tiles, and kept in registers across the loop they spill)
        int lane_t = lane;
        asm volatile("" : "+v"(lane_t));
        const int lane = lane_t, hi = lane >> 5, l31 = lane & 31;
        const char* Qs = smem + (t & 1) * LONG_TILE;
        const char* dOs = smem + (2 + (t & 1)) * LONG_TILE;
        const float* lse_s = ld_ring + (t & 1) * 128;
        const float* dl_s = lse_s + 64;
        const int q0 = t * 64;
        const int dk = wk0 + l31 - 4 * hi - q0;   // (key) - (first query row of the tile) - 4 hi
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            if (qb == 1 && q0 + 32 >= len) continue;   // (the last tile's second query block lies wholly past the sequence: P = 0)
            f32x16_t a_s, a_dp;
            alibi_acc_init(a_s, ns, dk - qb * 32, wk0 - q0 - qb * 32);
#pragma unroll
            for (int r = 0; r < 16; ++r) a_dp[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                a_s = mfma_bf16_32x32x16(lds_read_frag(Qs, tile64_off(qb * 32 + l31, ks * 2 + hi)), kf[ks], a_s);
                a_dp = mfma_bf16_32x32x16(lds_read_frag(dOs, tile64_off(qb * 32 + l31, ks * 2 + hi)), vf[ks], a_dp);
            }
            // one 16-query half at a time, P and dS packed to bf16 as soon as they exist (as attn_bwd_dkv_window_kernel: 16 fewer
            // live registers, which the bias' per-lane base and the 168-register budget of three workgroups per CU need)
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
#pragma unroll
                for (int db = 0; db < 2; ++db) {
                    acc_dv[db] = mfma_bf16_32x32x16(tile64_tr_frag(dOs, db * 32, qb * 32 + half * 16, lane), pf.v, acc_dv[db]);
                    acc_dk[db] = mfma_bf16_32x32x16(tile64_tr_frag(Qs, db * 32, qb * 32 + half * 16, lane), dsf.v, acc_dk[db]);
                }
            }
        }
    }
    __syncthreads();   // the ring becomes the staging area
    if (!wave_keys) return;
    bf16_t* kr0 = p.dqkv + (size_t)(p.H + h) * DH + (size_t)(t0 + wk0) * tok_stride;
    store_unrotated_rows(smem + wave * 4096, kr0, tok_stride, len - wk0, acc_dk, p.scale, nullptr, nullptr, 0, hi, lane);
    store_unrotated_rows(smem + 16384 + wave * 4096, kr0 + (size_t)p.H * DH, tok_stride, len - wk0, acc_dv, 1.f, nullptr, nullptr, 0, hi, lane);
}
#undef CX_ALIBI_REQUEST_Q
