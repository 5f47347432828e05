// attn_window.inc -- sliding-window (local) self-attention, forward and backward (included by attention.hip inside its namespace,
// after attn_long.inc: shares AttnParams, the tile64 helpers and long_dma_piece).  Query row i of a sequence attends key j of the
// same sequence iff i - left <= j <= i + right (flash-attn's window_size; the host passes WIN_INF for an unbounded side).
// No rotate-on-load, no dropout.  Per-element arithmetic as the long kernels (scale folded into the exponent, exp2, P rounded to
// bf16 for PV, fp32 row sums, lse natural log).
//
// The long kernels are shaped for S^2: 64 query rows per wave, 256 per workgroup -- under a 129-key band most of what such a
// workgroup stages is dead for most of its waves.  Here the blocks are sized for the band:
//   * 32 rows per wave, 128 per workgroup (queries in the forward / dQ kernels, keys in the dK / dV kernel): a wave's band is
//     32 + left + right wide, the workgroup's 128 + left + right -- at (64, 64) a wave uses 5-6 of the 8-10 32-row blocks its
//     workgroup stages;
//   * the streamed operand (K / V, or Q / dO) arrives in 64-row tiles by LDS-DMA into the 2-deep ring of the long kernels, one
//     barrier per tile, but only the tiles [t_lo, t_hi] that the workgroup's band touches, clamped to the sequence;
//   * a wave skips, per 32-row block of a tile, the products of blocks outside its own rows' band (wave-uniform tests);
//   * the window mask is applied per element from the accumulator's row / column mapping, only in blocks that a band edge or the
//     sequence end crosses: blocks wholly inside every row's window run mask-free (three of a wave's blocks at (64, 64));
//   * delta = rowsum(dO * O) is formed by the SAME MFMA chain as dP (A = the O row in the place of the V row): on the diagonal
//     of a (0, 0) window O == V bitwise, dP == delta bitwise, dS and dQ are exactly 0.
// One score chain per wave (not two as in the long kernels): 32 fewer accumulator registers, three to four workgroups per CU,
// whose barriers and DMA waits cover each other -- a band of four tiles has no steady state to pipeline within one workgroup.

constexpr int WIN_INF = 1 << 30;   // an unbounded side (row and key indices stay below 2^30: no overflow in q +- WIN_INF)

// the diagonal of a 32 x 32 accumulator block into the lane dimension: lane (l31, hi) gets element [row l31][column l31]
CX_DEVICE float acc_diagonal(const f32x16_t& a, int l31, int hi) {
    const int rd = (l31 & 3) | ((l31 >> 3) << 2);   // acc_row(rd, h) == l31 for h = (l31 >> 2) & 1
    float d = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) d = r == rd ? a[r] : d;
    const float other = __shfl_xor(d, 32, 64);
    return hi == ((l31 >> 2) & 1) ? d : other;
}

// pieces {wave, wave + 4} of 64-row tile `tile` of two row-major operands into ring slot `slot` (a function, not a lambda: a
// lambda does not inherit the kernels' target attribute below and would not be inlined into them)
CX_DEVICE void window_request(uint32_t lds0, int slot, int wave, const bf16_t* a, uint32_t a_bytes, const bf16_t* b, uint32_t b_bytes,
                              int tile, int len, int lane) {
    const uint32_t as = lds0 + slot * LONG_TILE, bs = lds0 + (2 + slot) * LONG_TILE;
    long_dma_piece(as, wave, a, a_bytes, tile * 64, len, lane);
    long_dma_piece(as, wave + 4, a, a_bytes, tile * 64, len, lane);
    long_dma_piece(bs, wave, b, b_bytes, tile * 64, len, lane);
    long_dma_piece(bs, wave + 4, b, b_bytes, tile * 64, len, lane);
}

// (no packed fp32 VALU forms in these kernels: the scalar forms cost nothing next to the MFMAs)
#if defined(__HIP_DEVICE_COMPILE__)
#define CX_WINDOW_KERNEL(occ) __global__ __launch_bounds__(256, occ) __attribute__((target("no-packed-fp32-ops")))
#else   // (the host pass knows no such feature)
#define CX_WINDOW_KERNEL(occ) __global__ __launch_bounds__(256, occ)
#endif

CX_WINDOW_KERNEL(4) void attn_fwd_window_kernel(AttnParams p, int wl, int wr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.y, b = blockIdx.z;
    const int t0 = p.cu[b], len = p.cu[b + 1] - t0;
    const int q0 = blockIdx.x * 128;
    if (q0 >= len) return;
    const size_t tok_stride = (size_t)3 * p.H * DH;
    const uint32_t tok_bytes = (uint32_t)tok_stride * 2u;
    const bf16_t* qbase = p.qkv + (size_t)h * DH;
    const bf16_t* kbase = qbase + (size_t)p.H * DH + (size_t)t0 * tok_stride;
    const bf16_t* vbase = kbase + (size_t)p.H * DH;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)smem;
    const int wq0 = q0 + wave * 32;            // this wave's 32 query rows
    const bool wave_live = wq0 < len;
    // key tiles of the workgroup's band, and the keys of this wave's band (both clamped to the sequence)
    const int q_last = min(q0 + 127, len - 1);
    const int t_lo = max(q0 - wl, 0) >> 6, t_hi = min(q_last + wr, len - 1) >> 6;
    const int wlo = wq0 - wl, whi = min(min(wq0 + 31, len - 1) + wr, len - 1);

    window_request(lds0, 0, wave, kbase, tok_bytes, vbase, tok_bytes, t_lo, len, lane);

    // Q fragments straight from global memory (rows past the end re-read the last row)
    const int q = wq0 + l31;
    bf16x8_t qf[4];
    {
        const bf16_t* row = qbase + (size_t)(t0 + (q < len ? q : len - 1)) * tok_stride;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8_t*>(row + (ks * 2 + hi) * 8);
    }
    const int klo = q - wl, khi = min(q + wr, len - 1);   // this lane's row sees keys [klo, khi]

    const float sc2 = p.scale * LOG2E;
    float m_run = -1e30f, l_run = 0.f;
    f32x16_t acc_o[2];
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_o[db][r] = 0.f;

#pragma unroll 1
    for (int t = t_lo; t <= t_hi; ++t) {
        // this wave's pieces of tile t have landed, then everybody's have, and everybody is through tile t - 1 (see attn_fwd_long_kernel)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t < t_hi) window_request(lds0, (t + 1 - t_lo) & 1, wave, kbase, tok_bytes, vbase, tok_bytes, t + 1, len, lane);
        const int kv0 = t * 64;
        if (!wave_live || kv0 + 63 < wlo || kv0 > whi) continue;   // (wave-uniform) the tile lies outside this wave's band
        const char* Ks = smem + ((t - t_lo) & 1) * LONG_TILE;
        const char* Vs = smem + (2 + ((t - t_lo) & 1)) * LONG_TILE;

        bool live[2];
        float s[2][16];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int kb0 = kv0 + kb * 32;
            live[kb] = kb0 + 31 >= wlo && kb0 <= whi;
            if (!live[kb]) {   // P = 0 for the whole block: no products
#pragma unroll
                for (int r = 0; r < 16; ++r) s[kb][r] = -INFINITY;
                continue;
            }
            f32x16_t a;
#pragma unroll
            for (int r = 0; r < 16; ++r) a[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) a = mfma_bf16_32x32x16(lds_read_frag(Ks, tile64_off(kb * 32 + l31, ks * 2 + hi)), qf[ks], a);
            // mask-free when all 32 keys are inside the window of every one of the 32 rows and inside the sequence
            const bool inside = kb0 >= wq0 + 31 - wl && kb0 + 31 <= wq0 + wr && kb0 + 32 <= len;
            if (inside) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[kb][r] = a[r];
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kb0 + acc_row(r, hi);
                    s[kb][r] = (key >= klo && key <= khi) ? a[r] : -INFINITY;
                }
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kb][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64)) * sc2;   // (sc2 > 0: the maximum commutes with the scale)
        // a row with no visible key in this tile keeps m_run (-1e30 at first: exp2(-inf + 1e30) = 0, never a NaN)
        const float m_new = fmaxf(m_run, mx);
        const bool same = m_new == m_run;
        const float alpha = fast_exp2(m_run - m_new);
        m_run = m_new;
        float psum = 0.f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[kb][r] = fast_exp2(__builtin_fmaf(s[kb][r], sc2, -m_new));
                psum += s[kb][r];
            }
        l_run = l_run * alpha + psum;
        if (!__all(same)) {   // (alpha == 1 exactly otherwise)
#pragma unroll
            for (int db = 0; db < 2; ++db)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc_o[db][r] *= alpha;
        }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            if (!live[kb]) continue;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const bf16x8_t pf = pack_frag(s[kb], half);
#pragma unroll
                for (int db = 0; db < 2; ++db)
                    acc_o[db] = mfma_bf16_32x32x16(tile64_tr_frag(Vs, db * 32, kb * 32 + half * 16, lane), pf, acc_o[db]);
            }
        }
    }

    __syncthreads();   // every wave is through the last tile: the ring becomes the output staging area (4 KiB per wave)
    if (!wave_live) return;
    char* st = smem + wave * 4096;
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.f / l_tot;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            uint2 pk;
            pk.x = pack_bf16x2(acc_o[db][4 * qd] * inv, acc_o[db][4 * qd + 1] * inv);
            pk.y = pack_bf16x2(acc_o[db][4 * qd + 2] * inv, acc_o[db][4 * qd + 3] * inv);
            *reinterpret_cast<uint2*>(st + tile64_off(l31, db * 4 + qd) + hi * 8) = pk;
        }
    if (q < len && hi == 0) p.lse[(size_t)h * p.T + t0 + q] = (m_run + log2f(l_tot)) * LN2;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int r = it * 8 + (lane >> 3), c = lane & 7;
        const uint4 v = *reinterpret_cast<const uint4*>(st + tile64_off(r, c));
        if (wq0 + r < len) *reinterpret_cast<uint4*>(p.out + ((size_t)(t0 + wq0 + r) * p.H + h) * DH + c * 8) = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------- backward
// attn_bwd_dq_window_kernel: the forward's work split (32 query rows per wave, the band's K / V tiles through the ring); Q, dO
// and O fragments straight from global memory; writes p.delta for the dK / dV kernel, which therefore runs second.
CX_WINDOW_KERNEL(3) void attn_bwd_dq_window_kernel(AttnParams p, int wl, int wr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.y, b = blockIdx.z;
    const int t0 = p.cu[b], len = p.cu[b + 1] - t0;
    const int q0 = blockIdx.x * 128;
    if (q0 >= len) return;
    const size_t tok_stride = (size_t)3 * p.H * DH, o_stride = (size_t)p.H * DH;
    const uint32_t tok_bytes = (uint32_t)tok_stride * 2u;
    const bf16_t* qbase = p.qkv + (size_t)h * DH;
    const bf16_t* kbase = qbase + (size_t)p.H * DH + (size_t)t0 * tok_stride;
    const bf16_t* vbase = kbase + (size_t)p.H * DH;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)smem;
    const int wq0 = q0 + wave * 32;
    const bool wave_live = wq0 < len;
    const int q_last = min(q0 + 127, len - 1);
    const int t_lo = max(q0 - wl, 0) >> 6, t_hi = min(q_last + wr, len - 1) >> 6;
    const int wlo = wq0 - wl, whi = min(min(wq0 + 31, len - 1) + wr, len - 1);

    window_request(lds0, 0, wave, kbase, tok_bytes, vbase, tok_bytes, t_lo, len, lane);

    const int q = wq0 + l31;
    const int qc = q < len ? q : len - 1;
    bf16x8_t qf[4], dof[4];
    float dl;
    {
        const bf16_t* qrow = qbase + (size_t)(t0 + qc) * tok_stride;
        const bf16_t* dorow = p.dout + (size_t)(t0 + qc) * o_stride + (size_t)h * DH;
        const bf16_t* orow = p.out + (size_t)(t0 + qc) * o_stride + (size_t)h * DH;
        f32x16_t a_dl;
#pragma unroll
        for (int r = 0; r < 16; ++r) a_dl[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            qf[ks] = *reinterpret_cast<const bf16x8_t*>(qrow + (ks * 2 + hi) * 8);
            dof[ks] = *reinterpret_cast<const bf16x8_t*>(dorow + (ks * 2 + hi) * 8);
            // O rows in the place the V rows take in dP below: element [row i][column j] = O_i . dO_j, delta on the diagonal
            a_dl = mfma_bf16_32x32x16(*reinterpret_cast<const bf16x8_t*>(orow + (ks * 2 + hi) * 8), dof[ks], a_dl);
        }
        dl = acc_diagonal(a_dl, l31, hi);
    }
    const float lse2 = p.lse[(size_t)h * p.T + t0 + qc] * LOG2E;
    if (wave_live && q < len && hi == 0) p.delta[(size_t)h * p.T + t0 + q] = dl;
    const int klo = q - wl, khi = min(q + wr, len - 1);
    const float sc2 = p.scale * LOG2E;
    f32x16_t acc_dq[2];
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_dq[db][r] = 0.f;

#pragma unroll 1
    for (int t = t_lo; t <= t_hi; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (see attn_fwd_long_kernel)
        __syncthreads();
        if (t < t_hi) window_request(lds0, (t + 1 - t_lo) & 1, wave, kbase, tok_bytes, vbase, tok_bytes, t + 1, len, lane);
        const int kv0 = t * 64;
        if (!wave_live || kv0 + 63 < wlo || kv0 > whi) continue;
        const char* Ks = smem + ((t - t_lo) & 1) * LONG_TILE;
        const char* Vs = smem + (2 + ((t - t_lo) & 1)) * LONG_TILE;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int kb0 = kv0 + kb * 32;
            if (kb0 + 31 < wlo || kb0 > whi) continue;
            f32x16_t a_s, a_dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) a_s[r] = a_dp[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                a_s = mfma_bf16_32x32x16(lds_read_frag(Ks, tile64_off(kb * 32 + l31, ks * 2 + hi)), qf[ks], a_s);
                a_dp = mfma_bf16_32x32x16(lds_read_frag(Vs, tile64_off(kb * 32 + l31, ks * 2 + hi)), dof[ks], a_dp);
            }
            float ds[16];
            const bool inside = kb0 >= wq0 + 31 - wl && kb0 + 31 <= wq0 + wr && kb0 + 32 <= len;
            if (inside) {
#pragma unroll
                for (int r = 0; r < 16; ++r) ds[r] = fast_exp2(__builtin_fmaf(a_s[r], sc2, -lse2));
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kb0 + acc_row(r, hi);
                    ds[r] = (key >= klo && key <= khi) ? fast_exp2(__builtin_fmaf(a_s[r], sc2, -lse2)) : 0.f;
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) ds[r] *= a_dp[r] - dl;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const bf16x8_t dsf = pack_frag(ds, half);
#pragma unroll
                for (int db = 0; db < 2; ++db)
                    acc_dq[db] = mfma_bf16_32x32x16(tile64_tr_frag(Ks, db * 32, kb * 32 + half * 16, lane), dsf, acc_dq[db]);
            }
        }
    }
    __syncthreads();   // the ring becomes the staging area (4 KiB per wave)
    if (!wave_live) return;
    store_unrotated_rows(smem + wave * 4096, p.dqkv + (size_t)(t0 + wq0) * tok_stride + (size_t)h * DH, tok_stride, len - wq0, acc_dq,
                         p.scale, nullptr, nullptr, 0, hi, lane);
}

// attn_bwd_dkv_window_kernel: a workgroup owns 128 keys (a wave 32: K / V fragments from global memory, dK / dV accumulators in
// registers) and walks only the 64-row Q / dO tiles of the queries that can see them, [k0 - right, k_last + left]; lse / delta of
// a tile through registers into a small ring as in attn_bwd_dkv_long_kernel.  Needs p.delta.
CX_WINDOW_KERNEL(3) void attn_bwd_dkv_window_kernel(AttnParams p, int wl, int wr) {
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
    const int wk0 = k0 + wave * 32;            // this wave's 32 keys
    const bool wave_keys = wk0 < len;
    // query tiles of the workgroup's band (key j is seen by the queries [j - right, j + left]) and the queries of this wave's band
    const int k_last = min(k0 + 127, len - 1);
    const int t_lo = max(k0 - wr, 0) >> 6, t_hi = min(k_last + wl, len - 1) >> 6;
    const int wlo = wk0 - wr, whi = min(min(wk0 + 31, len - 1) + wl, len - 1);

    float pf_lse = 0.f, pf_dl = 0.f;
#define CX_WINDOW_REQUEST_Q(tile)                                                                                              \
    do {                                                                                                                       \
        window_request(lds0, ((tile) - t_lo) & 1, wave, qbase, tok_bytes, dobase, o_bytes, (tile), len, lane);                 \
        if (tid < 64) {                                                                                                        \
            int r = (tile) * 64 + tid;                                                                                         \
            const bool ok = r < len;                                                                                           \
            r = ok ? r : len - 1;                                                                                              \
            pf_lse = ok ? p.lse[(size_t)h * p.T + t0 + r] * LOG2E : INFINITY; /* rows past the end: P = exp2(-inf) = 0 */      \
            pf_dl = p.delta[(size_t)h * p.T + t0 + r];                                                                         \
        }                                                                                                                      \
    } while (0)
    CX_WINDOW_REQUEST_Q(t_lo);

    const int key = wk0 + l31;
    const bool key_ok = key < len;
    bf16x8_t kf[4], vf[4];
    {
        const int kc = key_ok ? key : len - 1;
        const bf16_t* krow = p.qkv + (size_t)(p.H + h) * DH + (size_t)(t0 + kc) * tok_stride;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            kf[ks] = *reinterpret_cast<const bf16x8_t*>(krow + (ks * 2 + hi) * 8);
            vf[ks] = *reinterpret_cast<const bf16x8_t*>(krow + (size_t)p.H * DH + (ks * 2 + hi) * 8);
        }
    }
    // this lane's key is seen by the queries [qlo, qhi]; a key past the end by none
    // (a row index minus WIN_INF is >= 3 * 2^30 as an unsigned number, above every span)
    const int qlo = key_ok ? key - wr : WIN_INF;
    const uint32_t span = (uint32_t)wl + (uint32_t)wr;
    const float sc2 = p.scale * LOG2E;
    f32x16_t acc_dk[2], acc_dv[2];
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_dk[db][r] = acc_dv[db][r] = 0.f;

#pragma unroll 1
    for (int t = t_lo; t <= t_hi; ++t) {
        const int slot = (t - t_lo) & 1;
        // lse / delta of tile t (requested with its DMA) into their slot, the DMA pieces landed, then everybody's
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tid < 64) {
            ld_ring[slot * 128 + tid] = pf_lse;
            ld_ring[slot * 128 + 64 + tid] = pf_dl;
        }
        __syncthreads();
        if (t < t_hi) CX_WINDOW_REQUEST_Q(t + 1);
        const int q0 = t * 64;
        if (!wave_keys || q0 + 63 < wlo || q0 > whi) continue;   // (wave-uniform) no query of the tile sees this wave's keys
        // (the lane index is made opaque per tile, as in attn_bwd_dq_long_kernel: the LDS addresses derived from it are invariant
        // across tiles, and kept in registers across the loop they spill)
        int lane_t = lane;
        asm volatile("" : "+v"(lane_t));
        const int lane = lane_t, hi = lane >> 5, l31 = lane & 31;
        const char* Qs = smem + slot * LONG_TILE;
        const char* dOs = smem + (2 + slot) * LONG_TILE;
        const float* lse_s = ld_ring + slot * 128;
        const float* dl_s = lse_s + 64;
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            const int qb0 = q0 + qb * 32;
            if (qb0 + 31 < wlo || qb0 > whi) continue;
            f32x16_t a_s, a_dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) a_s[r] = a_dp[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                a_s = mfma_bf16_32x32x16(lds_read_frag(Qs, tile64_off(qb * 32 + l31, ks * 2 + hi)), kf[ks], a_s);
                a_dp = mfma_bf16_32x32x16(lds_read_frag(dOs, tile64_off(qb * 32 + l31, ks * 2 + hi)), vf[ks], a_dp);
            }
            // mask-free when every one of the 32 queries sees all 32 keys (queries past the end carry lse = inf: P = 0 either way)
            const bool inside = wk0 >= qb0 + 31 - wl && wk0 + 31 <= qb0 + wr && wk0 + 32 <= len;
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
                        pr[e] = (inside || (uint32_t)(q0 + row + e - qlo) <= span) ? pe : 0.f;
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
#undef CX_WINDOW_REQUEST_Q
#undef CX_WINDOW_KERNEL
