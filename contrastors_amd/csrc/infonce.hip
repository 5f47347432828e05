// infonce.hip -- K13 of SURVEY.md §2b: the InfoNCE / CLIP loss of sc/loss.py:76-132 as ONE similarity GEMM fused
// with the row-softmax cross-entropy; the (N x G) logits are never written to memory in the forward pass.
//
// The contraction runs on the exact-fp32 matrix-core path (v_mfma_f32_32x32x2_f32: bit-for-bit an fmaf chain,
// guide §3) because the loss is < 0.1 % of the step's FLOPs -- spending 1/16 of the bf16 rate
// here buys parity with the fp32 oracle at the 1e-6 level instead of bf16-logit noise (quirk 5, Appendix A).
// MFMA is issued as (A := document rows, B := query rows) so a lane owns ONE query row: the online
// log-sum-exp over documents is lane-local.
// The same tile loop (sgemm_tile) carries the distillation trainer's similarity-KL loss: two products per tile, the soft-maxes of
// both and their KL divergence without either matrix (simkl_kernel, cx_simkl_fwd / cx_simkl_bwd).
#include "cx_common.h"
#include "../../include/contrastors_hip.h"

namespace {

constexpr int SBM = 128, SBN = 128, SBK = 16;
constexpr int STILE = 128 * SBK * 4;  // 8 KiB
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

// [128 rows][16 f32]: 4 chunks of 16 B per 64-B row; chunk c of row r at r*64 + ((c ^ ((r>>2)&3)) << 4)
CX_DEVICE int stile_off(int r, int c) { return r * 64 + ((c ^ ((r >> 2) & 3)) << 4); }

enum Epi { EPI_STORE = 0, EPI_LSE = 1, EPI_GRAD = 2 };

struct SgemmParams {
    const float* A;  // (M,K) lda  -- "query side": lane dimension of the result
    const float* B;  // (N,K) ldb  -- "document side": register dimension of the result
    int M, N, K, lda, ldb;
    int tiles_m, tiles_n;
    // EPI_STORE
    float* C; int ldc;
    // EPI_LSE / EPI_GRAD
    const int64_t* labels;
    float scale;
    float* pmax; float* psum; float* lab;  // workspace views (EPI_LSE)
    int* pidx;                             // EPI_LSE, optional: first column of each 64-column slice that attains its maximum
    int nparts;
    const float* lse; float coef; float* Gm; float* GmT; float* dscale;  // EPI_GRAD
};

struct SRegs { float4 r0, r1; };  // named members, not an array (keeps them in VGPRs)

CX_DEVICE float4 sload(const float* __restrict__ base, int ld, int row0, int nrows, int k0, int K, int item) {
    const int r = item >> 2, c = item & 3;
    int gr = row0 + r;
    gr = gr < nrows ? gr : nrows - 1;
    const int k = k0 + c * 4;
    if (k >= K) return make_float4(0.f, 0.f, 0.f, 0.f);  // K % 4 == 0: a chunk is all-in or all-out
    return *reinterpret_cast<const float4*>(base + (size_t)gr * ld + k);
}
CX_DEVICE void sstage(const float* __restrict__ base, int ld, int row0, int nrows, int k0, int K, int tid,
                      SRegs& regs) {
    regs.r0 = sload(base, ld, row0, nrows, k0, K, tid);
    regs.r1 = sload(base, ld, row0, nrows, k0, K, 256 + tid);
}
CX_DEVICE void scommit(char* tile, int tid, const SRegs& regs) {
    *reinterpret_cast<float4*>(tile + stile_off(tid >> 2, tid & 3)) = regs.r0;
    *reinterpret_cast<float4*>(tile + stile_off((256 + tid) >> 2, tid & 3)) = regs.r1;
}

// One 128 x 128 tile of A B^T over the whole K range into acc (zeroed here): double-buffered LDS ring of 4 tiles, register-staged
// global loads.  Ends on a __syncthreads(), so a second call may reuse the ring at once (simkl_kernel runs two back to back).
// Each accumulator sees its MFMAs in k order whatever surrounds the call: the result bits depend on (A, B, K) alone.
CX_DEVICE void sgemm_tile(const float* __restrict__ A, int lda, int M, const float* __restrict__ B, int ldb, int N, int K,
                          int m0, int n0, char* smem, int tid, f32x16_t (&acc)[2][2]) {
    const int lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31;
    const int wm = wave >> 1, wn = wave & 1;
    const int nk = (K + SBK - 1) / SBK;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    SRegs ar = {}, br = {};
    sstage(A, lda, m0, M, 0, K, tid, ar);
    sstage(B, ldb, n0, N, 0, K, tid, br);
    scommit(smem, tid, ar);
    scommit(smem + STILE, tid, br);
    __syncthreads();

    for (int it = 0; it < nk; ++it) {
        char* cur = smem + (it & 1) * 2 * STILE;
        char* nxt = smem + ((it + 1) & 1) * 2 * STILE;
        const bool more = (it + 1) < nk;
        if (more) {
            sstage(A, lda, m0, M, (it + 1) * SBK, K, tid, ar);
            sstage(B, ldb, n0, N, (it + 1) * SBK, K, tid, br);
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            // lane-half hi reads k = 8g + 4hi + {0..3}; MFMA e consumes element e of both operands, i.e. the
            // reduction pair {8g+e, 8g+4+e}: a permutation of k shared by A and B.
            float4 af[2], bf[2];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                af[b] = *reinterpret_cast<const float4*>(cur + stile_off(wm * 64 + b * 32 + l31, 2 * g + hi));
                bf[b] = *reinterpret_cast<const float4*>(cur + STILE + stile_off(wn * 64 + b * 32 + l31, 2 * g + hi));
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[a].x, af[b].x, acc[a][b], 0, 0, 0);
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[a].y, af[b].y, acc[a][b], 0, 0, 0);
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[a].z, af[b].z, acc[a][b], 0, 0, 0);
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[a].w, af[b].w, acc[a][b], 0, 0, 0);
                }
        }
        if (more) {
            scommit(nxt, tid, ar);
            scommit(nxt + STILE, tid, br);
        }
        __syncthreads();
    }
}

template <int EPI>
__global__ __launch_bounds__(256, 2) void sgemm_nt_kernel(SgemmParams p) {
    __shared__ __attribute__((aligned(16))) char smem[4 * STILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31;
    const int wm = wave >> 1, wn = wave & 1;
    const int nwg = p.tiles_m * p.tiles_n;
    const int lid = xcd_remap(blockIdx.x, nwg);
    const int tn = lid % p.tiles_n, tm = lid / p.tiles_n;
    const int m0 = tm * SBM, n0 = tn * SBN;

    f32x16_t acc[2][2];  // [n-block a][m-block b]
    sgemm_tile(p.A, p.lda, p.M, p.B, p.ldb, p.N, p.K, m0, n0, smem, tid, acc);

    // acc[a][b][r] = sum_k A[m][k] B[n][k],  m = m0 + wm*64 + b*32 + l31,  n = n0 + wn*64 + a*32 + acc_row(r,hi)
    if constexpr (EPI == EPI_STORE) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int m = m0 + wm * 64 + b * 32 + l31;
            if (m >= p.M) continue;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int n = n0 + wn * 64 + a * 32 + 8 * q + 4 * hi;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (n + e < p.N) p.C[(size_t)m * p.ldc + n + e] = acc[a][b][4 * q + e];
                }
        }
    } else if constexpr (EPI == EPI_LSE) {
        const float sc2 = p.scale * LOG2E;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int m = m0 + wm * 64 + b * 32 + l31;
            const int mc = m < p.M ? m : p.M - 1;
            const long label = p.labels[mc];
            float mx = -INFINITY;
            int amx = 0x7fffffff;   // this lane's first column with v == mx (n grows with a, then r: strict > keeps the first)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int n = n0 + wn * 64 + a * 32 + acc_row(r, hi);
                    const float v = n < p.N ? acc[a][b][r] * sc2 : -INFINITY;
                    if (n == label && m < p.M) p.lab[m] = acc[a][b][r] * p.scale;  // exactly one lane owns it
                    acc[a][b][r] = v;
                    if (v > mx) amx = n;
                    mx = fmaxf(mx, v);
                }
            {
                const float omx = __shfl_xor(mx, 32, 64);
                const int oamx = __shfl_xor(amx, 32, 64);
                if (omx > mx || (omx == mx && oamx < amx)) amx = oamx;   // torch.argmax: the first index among equal maxima
                mx = fmaxf(mx, omx);
            }
            float sm = 0.f;
            if (mx > -INFINITY) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int r = 0; r < 16; ++r) sm += exp2f(acc[a][b][r] - mx);
            }
            sm += __shfl_xor(sm, 32, 64);
            if (hi == 0 && m < p.M) {
                const int part = tn * 2 + wn;
                p.pmax[(size_t)m * p.nparts + part] = mx;   // log2 units
                p.psum[(size_t)m * p.nparts + part] = sm;
                if (p.pidx) p.pidx[(size_t)m * p.nparts + part] = amx;
            }
        }
    } else {
        const float sc2 = p.scale * LOG2E;
        float dsc = 0.f;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int m = m0 + wm * 64 + b * 32 + l31;
            const bool m_ok = m < p.M;
            const int mc = m_ok ? m : p.M - 1;
            const long label = p.labels[mc];
            const float lse2 = p.lse[mc] * LOG2E;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int n = n0 + wn * 64 + a * 32 + 8 * q + 4 * hi;
                    float g[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float s = acc[a][b][4 * q + e];
                        const float pr = exp2f(s * sc2 - lse2) - ((n + e) == label ? 1.f : 0.f);
                        const bool ok = m_ok && (n + e) < p.N;
                        g[e] = ok ? pr * p.coef * p.scale : 0.f;
                        dsc += ok ? pr * s * p.coef : 0.f;
                        if (ok) p.GmT[(size_t)(n + e) * p.M + m] = g[e];
                    }
                    if (m_ok) {
                        if (n + 3 < p.N) {
                            *reinterpret_cast<float4*>(p.Gm + (size_t)m * p.N + n) = make_float4(g[0], g[1], g[2], g[3]);
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (n + e < p.N) p.Gm[(size_t)m * p.N + n + e] = g[e];
                        }
                    }
                }
        }
        if (p.dscale) {
            dsc = wave_sum(dsc);
            if (lane == 0) unsafeAtomicAdd(p.dscale, dsc);
        }
    }
}

// one wave per row: fold the per-column-slice partials into lse (natural log) and the per-row loss
// pidx / argmax (optional): the row's arg max over all G columns = the smallest recorded column among the slices whose maximum
// is the row maximum (slices are disjoint column ranges, each recorded its FIRST maximal column) -- what
// `similarity.argmax(dim=1)` of sc/loss.py:127-130 returns, without the similarity matrix.
__global__ __launch_bounds__(256) void lse_combine_kernel(const float* __restrict__ pmax,
                                                          const float* __restrict__ psum,
                                                          const float* __restrict__ lab, float* __restrict__ lse,
                                                          float* __restrict__ loss_rows, int N, int nparts,
                                                          const int* __restrict__ pidx, int* __restrict__ argmax) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    float mx = -INFINITY;
    for (int i = lane; i < nparts; i += 64) mx = fmaxf(mx, pmax[(size_t)row * nparts + i]);
    mx = wave_max(mx);
    if (pidx && argmax) {
        int am = 0x7fffffff;
        for (int i = lane; i < nparts; i += 64)
            if (pmax[(size_t)row * nparts + i] == mx) am = min(am, pidx[(size_t)row * nparts + i]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) am = min(am, __shfl_xor(am, o, 64));
        if (lane == 0) argmax[row] = am;
    }
    float s = 0.f;
    for (int i = lane; i < nparts; i += 64) {
        const float pm = pmax[(size_t)row * nparts + i];
        if (pm > -INFINITY) s += psum[(size_t)row * nparts + i] * exp2f(pm - mx);
    }
    s = wave_sum(s);
    if (lane == 0) {
        const float l = (mx + log2f(s)) * LN2;
        lse[row] = l;
        loss_rows[row] = l - lab[row];
    }
}

// ---- similarity-KL (distillation `kd` loss, sc/trainers/distill.py:347-355): KL(softmax_j t || softmax_j s) per query row for
// t = c <Qt_i, Dt_j>, s = c <Qs_i, Ds_j>, without either (N x G) matrix.
//   kl_i = sum_j p_ij (t_ij - s_ij) - lse_t_i + lse_s_i
// Both products of a tile run sgemm_tile back to back over the same LDS ring; the teacher's result waits in registers (2 x 64
// accumulators per lane).  128 accumulator + 16 staging + 16 fragment registers: __launch_bounds__(256, 2) leaves 256 per lane and
// compiles to 185 (forward) / 181 (gradient) VGPRs with no scratch (-Rpass-analysis=kernel-resource-usage), so two blocks share
// a CU as they do for sgemm_nt_kernel<EPI_GRAD> (177); (256, 1) would buy nothing the kernel uses.
struct SimklParams {
    const float* Qs; const float* Ds; const float* Qt; const float* Dt;
    int N, G, dim_s, dim_t, ldqs, ldds, ldqt, lddt;
    int tiles_m, tiles_n, nparts;
    float c;                                     // 1 / temperature
    float* pmt; float* plt; float* pat; float* pms; float* pls;   // SIMKL_FWD: (N, nparts) partials, maxima in log2 units
    const float* lse_s; const float* lse_t; float coef; float* Gm; float* GmT;   // SIMKL_GRAD
};
enum SimklMode { SIMKL_FWD = 0, SIMKL_GRAD = 1 };

template <int MODE>
__global__ __launch_bounds__(256, 2) void simkl_kernel(SimklParams p) {
    __shared__ __attribute__((aligned(16))) char smem[4 * STILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31;
    const int wm = wave >> 1, wn = wave & 1;
    const int nwg = p.tiles_m * p.tiles_n;
    const int lid = xcd_remap(blockIdx.x, nwg);
    const int tn = lid % p.tiles_n, tm = lid / p.tiles_n;
    const int m0 = tm * SBM, n0 = tn * SBN;

    f32x16_t at[2][2], as[2][2];  // teacher / student, [n-block a][m-block b]
    sgemm_tile(p.Qt, p.ldqt, p.N, p.Dt, p.lddt, p.G, p.dim_t, m0, n0, smem, tid, at);
    sgemm_tile(p.Qs, p.ldqs, p.N, p.Ds, p.ldds, p.G, p.dim_s, m0, n0, smem, tid, as);

    const float c2 = p.c * LOG2E;
    if constexpr (MODE == SIMKL_FWD) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int m = m0 + wm * 64 + b * 32 + l31;
            float mt = -INFINITY, ms = -INFINITY;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int n = n0 + wn * 64 + a * 32 + acc_row(r, hi);
                    if (n < p.G) {
                        mt = fmaxf(mt, at[a][b][r] * c2);
                        ms = fmaxf(ms, as[a][b][r] * c2);
                    }
                }
            mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
            ms = fmaxf(ms, __shfl_xor(ms, 32, 64));
            float lt = 0.f, ls = 0.f, aa = 0.f;
            if (mt > -INFINITY) {   // (the slice has a column below G: then ms is finite too)
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int n = n0 + wn * 64 + a * 32 + acc_row(r, hi);
                        // a column past G gives exactly 0 to all three sums: it is dropped BEFORE t - s, never as (-inf) - (-inf)
                        const bool ok = n < p.G;
                        const float et = ok ? exp2f(at[a][b][r] * c2 - mt) : 0.f;
                        const float es = ok ? exp2f(as[a][b][r] * c2 - ms) : 0.f;
                        const float df = ok ? (at[a][b][r] - as[a][b][r]) * p.c : 0.f;
                        lt += et;
                        ls += es;
                        aa += et * df;
                    }
            }
            lt += __shfl_xor(lt, 32, 64);
            ls += __shfl_xor(ls, 32, 64);
            aa += __shfl_xor(aa, 32, 64);
            if (hi == 0 && m < p.N) {
                const size_t o = (size_t)m * p.nparts + tn * 2 + wn;
                p.pmt[o] = mt; p.plt[o] = lt; p.pat[o] = aa; p.pms[o] = ms; p.pls[o] = ls;
            }
        }
    } else {
        const float k = p.coef * p.c;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int m = m0 + wm * 64 + b * 32 + l31;
            const bool m_ok = m < p.N;
            const int mc = m_ok ? m : p.N - 1;
            const float lt2 = p.lse_t[mc] * LOG2E, ls2 = p.lse_s[mc] * LOG2E;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int n = n0 + wn * 64 + a * 32 + 8 * q + 4 * hi;
                    float g[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float qs = exp2f(as[a][b][4 * q + e] * c2 - ls2);
                        const float pt = exp2f(at[a][b][4 * q + e] * c2 - lt2);
                        const bool ok = m_ok && (n + e) < p.G;
                        g[e] = ok ? (qs - pt) * k : 0.f;
                        if (ok) p.GmT[(size_t)(n + e) * p.N + m] = g[e];
                    }
                    if (m_ok) {
                        if (n + 3 < p.G) {
                            *reinterpret_cast<float4*>(p.Gm + (size_t)m * p.G + n) = make_float4(g[0], g[1], g[2], g[3]);
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (n + e < p.G) p.Gm[(size_t)m * p.G + n + e] = g[e];
                        }
                    }
                }
        }
    }
}

// One row's slices folded: *mx = the row maximum (log2 units), *l = sum_j exp2(v_j - mx), *a (with pa) = the third sum rescaled
// the same way.  Called for the teacher and for the student: equal partials give equal bits.
CX_DEVICE void simkl_fold(const float* __restrict__ pm, const float* __restrict__ pl, const float* __restrict__ pa,
                          int nparts, int lane, float* mx_out, float* l_out, float* a_out) {
    float mx = -INFINITY;
    for (int i = lane; i < nparts; i += 64) mx = fmaxf(mx, pm[i]);
    mx = wave_max(mx);
    float l = 0.f, a = 0.f;
    for (int i = lane; i < nparts; i += 64) {
        const float m = pm[i];
        if (m > -INFINITY) {
            const float w = exp2f(m - mx);
            l += pl[i] * w;
            if (pa) a += pa[i] * w;
        }
    }
    *mx_out = mx;
    *l_out = wave_sum(l);
    if (pa) *a_out = wave_sum(a);
}

// one wave per row.  kl = sum_j p_j (t_j - s_j) + (lse_s - lse_t); the difference of the two log-sum-exps is formed as
// (m_s - m_t) + log2(l_s / l_t): its rounding error scales with the difference, not with the lse (a student close to its teacher
// has kl << lse), and it is exactly 0 for equal partials.
__global__ __launch_bounds__(256) void simkl_combine_kernel(const float* __restrict__ pmt, const float* __restrict__ plt,
                                                            const float* __restrict__ pat, const float* __restrict__ pms,
                                                            const float* __restrict__ pls, float* __restrict__ lse_s,
                                                            float* __restrict__ lse_t, float* __restrict__ kl_rows, int N,
                                                            int nparts) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const size_t o = (size_t)row * nparts;
    float mt, lt, at = 0.f, ms, ls;
    simkl_fold(pmt + o, plt + o, pat + o, nparts, lane, &mt, &lt, &at);
    simkl_fold(pms + o, pls + o, nullptr, nparts, lane, &ms, &ls, nullptr);
    if (lane == 0) {
        lse_t[row] = (mt + log2f(lt)) * LN2;
        lse_s[row] = (ms + log2f(ls)) * LN2;
        kl_rows[row] = at / lt + ((ms - mt) + log2f(ls / lt)) * LN2;
    }
}

template <int EPI>
int launch(const SgemmParams& p, hipStream_t s) {
    hipLaunchKernelGGL((sgemm_nt_kernel<EPI>), dim3(p.tiles_m * p.tiles_n), dim3(256), 0, s, p);
    return hipGetLastError() == hipSuccess ? CX_OK : CX_ERR_LAUNCH;
}

int check_common(int M, int N, int K, int lda, int ldb) {
    if (K <= 0 || (K % 4) != 0) return CX_ERR_SHAPE;
    if ((lda % 4) != 0 || (ldb % 4) != 0) return CX_ERR_ALIGN;
    (void)M; (void)N;
    return CX_OK;
}

}  // namespace

extern "C" {

int cx_sgemm_nt(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                void* stream) {
    if (M <= 0 || N <= 0) return CX_OK;
    int rc = check_common(M, N, K, lda, ldb);
    if (rc != CX_OK) return rc;
    SgemmParams p = {};
    p.A = A; p.B = B; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb;
    p.tiles_m = (M + SBM - 1) / SBM; p.tiles_n = (N + SBN - 1) / SBN;
    p.C = C; p.ldc = ldc;
    return launch<EPI_STORE>(p, (hipStream_t)stream);
}

long cx_infonce_ws_floats(int N, int G) {
    const long nparts = 2L * ((G + SBN - 1) / SBN);
    return (long)N * (2 * nparts + 1);
}
long cx_infonce_argmax_ws_floats(int N, int G) {
    const long nparts = 2L * ((G + SBN - 1) / SBN);
    return (long)N * (3 * nparts + 1);
}

int cx_infonce_fwd(const float* Q, const float* D, const int64_t* labels, float scale, float* ws, float* lse,
                   float* loss_rows, int N, int G, int dim, int ldq, int ldd, void* stream) {
    return cx_infonce_fwd_argmax(Q, D, labels, scale, ws, lse, loss_rows, nullptr, N, G, dim, ldq, ldd, stream);
}

int cx_infonce_fwd_argmax(const float* Q, const float* D, const int64_t* labels, float scale, float* ws, float* lse,
                          float* loss_rows, int32_t* argmax, int N, int G, int dim, int ldq, int ldd, void* stream) {
    if (N <= 0 || G <= 0) return CX_OK;
    if (!Q || !D || !labels || !ws || !lse || !loss_rows) return CX_ERR_ARG;
    int rc = check_common(N, G, dim, ldq, ldd);
    if (rc != CX_OK) return rc;
    SgemmParams p = {};
    p.A = Q; p.B = D; p.M = N; p.N = G; p.K = dim; p.lda = ldq; p.ldb = ldd;
    p.tiles_m = (N + SBM - 1) / SBM; p.tiles_n = (G + SBN - 1) / SBN;
    p.labels = labels; p.scale = scale;
    p.nparts = 2 * p.tiles_n;
    p.pmax = ws;
    p.psum = ws + (size_t)N * p.nparts;
    p.lab = ws + (size_t)2 * N * p.nparts;
    p.pidx = argmax ? reinterpret_cast<int*>(ws + (size_t)2 * N * p.nparts + N) : nullptr;   // (ws: cx_infonce_argmax_ws_floats)
    rc = launch<EPI_LSE>(p, (hipStream_t)stream);
    if (rc != CX_OK) return rc;
    hipLaunchKernelGGL(lse_combine_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, p.pmax, p.psum,
                       p.lab, lse, loss_rows, N, p.nparts, p.pidx, argmax);
    return hipGetLastError() == hipSuccess ? CX_OK : CX_ERR_LAUNCH;
}

int cx_infonce_bwd(const float* Q, const float* D, const int64_t* labels, const float* lse, float scale, float coef,
                   float* Gmat, float* GmatT, float* QT, float* DT, float* dQ, float* dD, float* dscale_accum,
                   int N, int G, int dim, int ldq, int ldd, void* stream) {
    if (N <= 0 || G <= 0) return CX_OK;
    if (!Q || !D || !labels || !lse || !Gmat || !GmatT || !QT || !DT || !dQ || !dD) return CX_ERR_ARG;
    int rc = check_common(N, G, dim, ldq, ldd);
    if (rc != CX_OK) return rc;
    if ((N % 4) != 0 || (G % 4) != 0) return CX_ERR_SHAPE;  // they are the K (and ld) of the two output GEMMs
    SgemmParams p = {};
    p.A = Q; p.B = D; p.M = N; p.N = G; p.K = dim; p.lda = ldq; p.ldb = ldd;
    p.tiles_m = (N + SBM - 1) / SBM; p.tiles_n = (G + SBN - 1) / SBN;
    p.labels = labels; p.scale = scale; p.lse = lse; p.coef = coef;
    p.Gm = Gmat; p.GmT = GmatT; p.dscale = dscale_accum;
    rc = launch<EPI_GRAD>(p, (hipStream_t)stream);
    if (rc != CX_OK) return rc;
    rc = cx_transpose_f32(Q, QT, N, dim, ldq, N, stream);
    if (rc != CX_OK) return rc;
    rc = cx_transpose_f32(D, DT, G, dim, ldd, G, stream);
    if (rc != CX_OK) return rc;
    rc = cx_sgemm_nt(Gmat, DT, dQ, N, dim, G, G, G, dim, stream);   // dQ[m][c] = sum_n Gm[m][n] D[n][c]
    if (rc != CX_OK) return rc;
    return cx_sgemm_nt(GmatT, QT, dD, G, dim, N, N, N, dim, stream); // dD[n][c] = sum_m Gm[m][n] Q[m][c]
}

long cx_simkl_ws_floats(int N, int G) {
    const long nparts = 2L * ((G + SBN - 1) / SBN);
    return (long)N * 5 * nparts;
}

static int simkl_check(int N, int G, int dim_s, int dim_t, int ldqs, int ldds, int ldqt, int lddt) {
    int rc = check_common(N, G, dim_s, ldqs, ldds);
    if (rc != CX_OK) return rc;
    return check_common(N, G, dim_t, ldqt, lddt);
}

static void simkl_fill(SimklParams& p, const float* Qs, const float* Ds, const float* Qt, const float* Dt, float inv_temp,
                       int N, int G, int dim_s, int dim_t, int ldqs, int ldds, int ldqt, int lddt) {
    p.Qs = Qs; p.Ds = Ds; p.Qt = Qt; p.Dt = Dt;
    p.N = N; p.G = G; p.dim_s = dim_s; p.dim_t = dim_t; p.ldqs = ldqs; p.ldds = ldds; p.ldqt = ldqt; p.lddt = lddt;
    p.tiles_m = (N + SBM - 1) / SBM; p.tiles_n = (G + SBN - 1) / SBN; p.nparts = 2 * p.tiles_n;
    p.c = inv_temp;
}

int cx_simkl_fwd(const float* Qs, const float* Ds, const float* Qt, const float* Dt, float inv_temp, float* ws,
                 float* lse_s, float* lse_t, float* kl_rows, int N, int G, int dim_s, int dim_t, int ldqs, int ldds,
                 int ldqt, int lddt, void* stream) {
    if (N <= 0 || G <= 0) return CX_OK;
    if (!Qs || !Ds || !Qt || !Dt || !ws || !lse_s || !lse_t || !kl_rows) return CX_ERR_ARG;
    int rc = simkl_check(N, G, dim_s, dim_t, ldqs, ldds, ldqt, lddt);
    if (rc != CX_OK) return rc;
    SimklParams p = {};
    simkl_fill(p, Qs, Ds, Qt, Dt, inv_temp, N, G, dim_s, dim_t, ldqs, ldds, ldqt, lddt);
    const size_t sz = (size_t)N * p.nparts;
    p.pmt = ws; p.plt = ws + sz; p.pat = ws + 2 * sz; p.pms = ws + 3 * sz; p.pls = ws + 4 * sz;
    hipLaunchKernelGGL((simkl_kernel<SIMKL_FWD>), dim3(p.tiles_m * p.tiles_n), dim3(256), 0, (hipStream_t)stream, p);
    if (hipGetLastError() != hipSuccess) return CX_ERR_LAUNCH;
    hipLaunchKernelGGL(simkl_combine_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, p.pmt, p.plt, p.pat,
                       p.pms, p.pls, lse_s, lse_t, kl_rows, N, p.nparts);
    return hipGetLastError() == hipSuccess ? CX_OK : CX_ERR_LAUNCH;
}

int cx_simkl_bwd(const float* Qs, const float* Ds, const float* Qt, const float* Dt, const float* lse_s,
                 const float* lse_t, float inv_temp, float coef, float* Gmat, float* GmatT, float* QsT, float* DsT,
                 float* dQs, float* dDs, int N, int G, int dim_s, int dim_t, int ldqs, int ldds, int ldqt, int lddt,
                 void* stream) {
    if (N <= 0 || G <= 0) return CX_OK;
    if (!Qs || !Ds || !Qt || !Dt || !lse_s || !lse_t || !Gmat || !GmatT || !QsT || !DsT || !dQs || !dDs) return CX_ERR_ARG;
    int rc = simkl_check(N, G, dim_s, dim_t, ldqs, ldds, ldqt, lddt);
    if (rc != CX_OK) return rc;
    if ((N % 4) != 0 || (G % 4) != 0) return CX_ERR_SHAPE;  // they are the K (and ld) of the two output GEMMs
    SimklParams p = {};
    simkl_fill(p, Qs, Ds, Qt, Dt, inv_temp, N, G, dim_s, dim_t, ldqs, ldds, ldqt, lddt);
    p.lse_s = lse_s; p.lse_t = lse_t; p.coef = coef; p.Gm = Gmat; p.GmT = GmatT;
    hipLaunchKernelGGL((simkl_kernel<SIMKL_GRAD>), dim3(p.tiles_m * p.tiles_n), dim3(256), 0, (hipStream_t)stream, p);
    if (hipGetLastError() != hipSuccess) return CX_ERR_LAUNCH;
    rc = cx_transpose_f32(Qs, QsT, N, dim_s, ldqs, N, stream);
    if (rc != CX_OK) return rc;
    rc = cx_transpose_f32(Ds, DsT, G, dim_s, ldds, G, stream);
    if (rc != CX_OK) return rc;
    rc = cx_sgemm_nt(Gmat, DsT, dQs, N, dim_s, G, G, G, dim_s, stream);   // dQs[m][c] = sum_n Gm[m][n] Ds[n][c]
    if (rc != CX_OK) return rc;
    return cx_sgemm_nt(GmatT, QsT, dDs, G, dim_s, N, N, N, dim_s, stream); // dDs[n][c] = sum_m Gm[m][n] Qs[m][c]
}

}  // extern "C"
