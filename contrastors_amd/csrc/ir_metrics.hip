// ir_metrics.hip -- per-query retrieval metrics (nDCG, MAP, recall, precision, MRR, hit rate at K cut-offs) from the ranks of
// a query's judged documents, as cx_rank_targets (rank.hip) leaves them: CSR rows of (rank, gain) entries on the device.
//
// Every cut-off metric of a query is a function of the ranks of its relevant documents alone, so neither a top-k list nor
// the scores are needed.  An entry with gain > 0 is a relevant document; an entry with gain == 0 is an EXCLUDED document
// (BEIR's ignore_identical_ids): it is taken out of the ranking, i.e. every entry ranked after it moves up by one.
//
// One workgroup per row.  The row is staged in LDS (48 KB at CX_IR_MAX_ROW entries, 1 KB of reduction scratch), the three counts per entry (excluded
// before it, relevant before it, entries with a larger gain) are O(n^2 / 256) compare loops over LDS, the sums are fp64 in a
// fixed order: each lane strides over the entries, a xor-shuffle tree adds the lanes of a wave, lane c adds the four waves
// of cut-off c in order.  No atomics: two runs give the same bits.  The cost of an evaluation is in encode and rank; this is glue.
#include "cx_common.h"

namespace {

constexpr int IR_MAX_ROW = CX_IR_MAX_ROW;
constexpr int IR_MAX_K = CX_IR_MAX_K;
static_assert(IR_MAX_ROW <= 65536 && IR_MAX_ROW * 12 <= 48 * 1024, "before_j / ipos_j are packed in 16 bits each; 48 KB of LDS");
constexpr int NT = 256;
constexpr int NW = NT / 64;

struct IrCutoffs {
    int k[IR_MAX_K];
};

CX_DEVICE double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
CX_DEVICE int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
CX_DEVICE int wave_min_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(NT) void ir_metrics_kernel(const int64_t* __restrict__ row_ptr, const int64_t* __restrict__ ranks,
                                                        const float* __restrict__ gains, IrCutoffs ks, int K,
                                                        double* __restrict__ out, int* __restrict__ nrel) {
    __shared__ int2 s_e[IR_MAX_ROW];        // x: rank, then the adjusted rank a_j;  y: the bits of the gain (<= 0: excluded)
    __shared__ uint32_t s_pos[IR_MAX_ROW];  // scratch for a_j, then before_j | ipos_j << 16 (both < 4096)
    __shared__ double s_sum[IR_MAX_K][NW][3];
    __shared__ int s_cnt[IR_MAX_K][NW][2];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m = blockIdx.x;
    const int64_t beg = row_ptr[m], len = row_ptr[m + 1] - beg;
    double* o = out + m * K * 6;
    if (len < 0 || len > IR_MAX_ROW) {   // (uniform over the workgroup) longer than the staging buffers: NaNs, nothing staged
        if (tid < K * 6) o[tid] = __longlong_as_double(0x7ff8000000000000LL);
        if (tid == 0) nrel[m] = -1;
        return;
    }
    const int n = (int)len;
    for (int j = tid; j < n; j += NT) {
        const int64_t r = ranks[beg + j];
        s_e[j] = make_int2((int)min(max(r, (int64_t)0), (int64_t)0x7fffffff), __float_as_int(gains[beg + j]));
    }
    __syncthreads();
    // a_j = rank_j - #{excluded e : rank_e < rank_j}.  The compare loops below are branch-free so that they unroll: every lane
    // reads the same LDS word (a broadcast), and the loop is bound by that read's latency, not by its rate
    for (int j = tid; j < n; j += NT) {
        const int2 ej = s_e[j];
        int c = 0;
        if (__int_as_float(ej.y) > 0.f) {
#pragma unroll 8
            for (int e = 0; e < n; ++e) {
                const int2 ee = s_e[e];
                c += (!(__int_as_float(ee.y) > 0.f) && ee.x < ej.x) ? 1 : 0;
            }
        }
        s_pos[j] = (uint32_t)(ej.x - c);
    }
    __syncthreads();
    for (int j = tid; j < n; j += NT) s_e[j].x = (int)s_pos[j];
    __syncthreads();
    // before_j = #{relevant i : a_i < a_j};  ipos_j = #{relevant i : gain_i > gain_j or (gain_i == gain_j and i < j)}
    int my_rel = 0;
    for (int j = tid; j < n; j += NT) {
        const int2 ej = s_e[j];
        const float g = __int_as_float(ej.y);
        if (!(g > 0.f)) continue;
        ++my_rel;
        int before = 0, ipos = 0;
#pragma unroll 8
        for (int i = 0; i < n; ++i) {
            const int2 ei = s_e[i];
            const float gi = __int_as_float(ei.y);
            const bool rel = gi > 0.f;
            before += (rel && ei.x < ej.x) ? 1 : 0;
            ipos += (rel && (gi > g || (gi == g && i < j))) ? 1 : 0;
        }
        s_pos[j] = (uint32_t)before | ((uint32_t)ipos << 16);
    }
    my_rel = wave_sum_i32(my_rel);
    if (lane == 0) s_cnt[0][wave][0] = my_rel;
    __syncthreads();
    int R = 0;
    for (int w = 0; w < NW; ++w) R += s_cnt[0][w][0];
    __syncthreads();
    if (tid == 0) nrel[m] = R;
    if (R == 0) {
        if (tid < K * 6) o[tid] = 0.0;
        return;
    }

    for (int c = 0; c < K; ++c) {
        const int k = ks.k[c];
        double dcg = 0.0, idcg = 0.0, ap = 0.0;
        int hits = 0, amin = 0x7fffffff;
        for (int j = tid; j < n; j += NT) {
            const int2 ej = s_e[j];
            const float g = __int_as_float(ej.y);
            if (!(g > 0.f)) continue;
            const int a = ej.x;
            const int before = (int)(s_pos[j] & 0xffffu), ipos = (int)(s_pos[j] >> 16);
            if (a < k) {
                dcg += (double)g / log2((double)a + 2.0);
                ap += (double)(before + 1) / ((double)a + 1.0);
                ++hits;
            }
            if (ipos < k) idcg += (double)g / log2((double)ipos + 2.0);
            amin = min(amin, a);
        }
        dcg = wave_sum_f64(dcg);
        idcg = wave_sum_f64(idcg);
        ap = wave_sum_f64(ap);
        hits = wave_sum_i32(hits);
        amin = wave_min_i32(amin);
        if (lane == 0) {
            s_sum[c][wave][0] = dcg; s_sum[c][wave][1] = idcg; s_sum[c][wave][2] = ap;
            s_cnt[c][wave][0] = hits; s_cnt[c][wave][1] = amin;
        }
    }
    __syncthreads();
    if (tid < K) {   // lane c finishes cut-off c: the four waves' partial sums in order
        const int c = tid, k = ks.k[c];
        double d = 0.0, id = 0.0, p = 0.0;
        int h = 0, am = 0x7fffffff;
        for (int w = 0; w < NW; ++w) {
            d += s_sum[c][w][0]; id += s_sum[c][w][1]; p += s_sum[c][w][2];
            h += s_cnt[c][w][0]; am = min(am, s_cnt[c][w][1]);
        }
        double* oc = o + c * 6;
        oc[0] = id > 0.0 ? d / id : 0.0;
        oc[1] = p / (double)R;
        oc[2] = (double)h / (double)R;
        oc[3] = (double)h / (double)k;
        oc[4] = am < k ? 1.0 / ((double)am + 1.0) : 0.0;
        oc[5] = h > 0 ? 1.0 : 0.0;
    }
}

}  // namespace

extern "C" {

int cx_ir_metrics(const int64_t* row_ptr, const int64_t* ranks, const float* gains, int M, const int* ks, int K, double* out,
                  int* nrel, void* stream) {
    if (M < 0 || K < 1 || K > IR_MAX_K) return CX_ERR_SHAPE;
    if (!ks) return CX_ERR_ARG;
    IrCutoffs c = {};
    for (int i = 0; i < K; ++i) {
        if (ks[i] < 1) return CX_ERR_SHAPE;
        c.k[i] = ks[i];
    }
    if (M == 0) return CX_OK;
    if (!row_ptr || !ranks || !gains || !out || !nrel) return CX_ERR_ARG;
    hipLaunchKernelGGL(ir_metrics_kernel, dim3(M), dim3(NT), 0, (hipStream_t)stream, row_ptr, ranks, gains, c, K, out, nrel);
    return done();
}

}  // extern "C"
