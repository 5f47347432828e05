// mlm_mask.hip -- masked-language-model masking on the device: one launch turns a micro-batch of token ids into
// (masked ids, labels), what transformers.DataCollatorForLanguageModeling.torch_mask_tokens does in the reference's loader
// workers (sc/trainers/mlm.py:70,84).  The masks come from the Philox generator of the dropout kernels (cx_common.h), so they
// are a pure function of (seed, offset, token position): independent of the worker count, reproducible after a resume.
//
// Draw rule (tests/mlm_mask_ref.py):
//   token at flat position g = b * S + s takes ONE philox4x32_10 call,
//       counter (lo32(g), hi32(g), lo32(offset), hi32(offset)), key (lo32(seed), hi32(seed))  ->  (u0, u1, u2, u3)
//   special   its attention mask is 0, or its special_mask byte is non-zero, or its id is in the special-id list
//   target    not special and u0 < T(p),  T(x) = (uint32) fminf(x * 2^32, 4294967040.f)   (the clamp of dropout_keep4)
//   a target becomes   mask_token_id                          if u1 < T(0.8)
//                      (uint64(u2) * random_vocab) >> 32      else if u1 < T(0.9)
//                      its own id                             otherwise
//   (the collator's 80 / 10 / 10 split, which it draws as 0.8, then 0.5 of the rest); u3 is unused
//   labels  = the original id at targets, -100 elsewhere;  out_ids = ids at non-targets
// The result does not depend on the launch geometry, the dtype of ids or its row stride.
//
// Elementwise and HBM-bound (4 or 8 B in per token + the optional masks, 16 B out): a lane owns 4 consecutive tokens of one row.
// Each of its arrays is read / written as 16-B (the byte mask: 4-B) accesses when the lane has 4 tokens and that array's
// address is aligned, one element at a time otherwise (row ends, odd S, odd strides).  The grid is capped and strides over the
// groups.  No atomics; LDS holds the special-id list only; every output element is written once by one lane.
#include "cx_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;      // 256 CUs x 8 workgroups: the cap for memory-bound kernels; the rest is grid-strided
constexpr int kMaxSpecial = 16;

struct MaskPlan {
    uint32_t thr_p, thr_mask, thr_rand;   // T(p), T(0.8), T(0.9)
    uint32_t vocab;
    uint32_t seed_lo, seed_hi, off_lo, off_hi;
    int64_t mask_id;
};

inline uint32_t threshold(float x) { return (uint32_t)fminf(x * 4294967296.f, 4294967040.f); }

CX_DEVICE bool aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// 4 consecutive int64 as two 16-B accesses
CX_DEVICE void load4_i64(const int64_t* p, int64_t (&v)[4]) {
    const longlong2 a = *reinterpret_cast<const longlong2*>(p), b = *reinterpret_cast<const longlong2*>(p + 2);
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
}
CX_DEVICE void store4_i64(int64_t* p, const int64_t (&v)[4]) {
    longlong2 a, b;
    a.x = v[0]; a.y = v[1]; b.x = v[2]; b.y = v[3];
    *reinterpret_cast<longlong2*>(p) = a;
    *reinterpret_cast<longlong2*>(p + 2) = b;
}
CX_DEVICE void load4_ids(const int64_t* p, int64_t (&v)[4]) { load4_i64(p, v); }
CX_DEVICE void load4_ids(const int32_t* p, int64_t (&v)[4]) {
    const int4 a = *reinterpret_cast<const int4*>(p);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
}

template <typename IdT>
__global__ __launch_bounds__(kThreads) void mlm_mask_kernel(const IdT* __restrict__ ids, long stride,
                                                            const int64_t* __restrict__ attn, const uint8_t* __restrict__ spec_mask,
                                                            const int64_t* __restrict__ special_ids, int n_special, MaskPlan plan,
                                                            int64_t* __restrict__ out_ids, int64_t* __restrict__ labels, int S, int nq,
                                                            long n_groups) {
    __shared__ int64_t s_special[kMaxSpecial];
    if ((int)threadIdx.x < n_special) s_special[threadIdx.x] = special_ids[threadIdx.x];
    __syncthreads();

    const uint2 key = make_uint2(plan.seed_lo, plan.seed_hi);
    const long step = (long)gridDim.x * kThreads;
    for (long grp = (long)blockIdx.x * kThreads + threadIdx.x; grp < n_groups; grp += step) {
        const long b = grp / nq;
        const int s0 = (int)(grp - b * nq) * 4;
        const int n = min(4, S - s0);
        const long g0 = b * S + s0;                       // flat position of the lane's first token (outputs, masks, counter)
        const IdT* src = ids + b * stride + s0;
        const bool full = n == 4;

        int64_t id[4] = {0, 0, 0, 0};
        if (full && aligned(src, 16)) {
            load4_ids(src, id);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n) id[j] = (int64_t)src[j];
        }
        bool special[4] = {false, false, false, false};
        if (attn) {
            int64_t a[4] = {1, 1, 1, 1};
            if (full && aligned(attn + g0, 16)) {
                load4_i64(attn + g0, a);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < n) a[j] = attn[g0 + j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) special[j] = a[j] == 0;
        }
        if (spec_mask) {
            uint32_t m = 0;
            if (full && aligned(spec_mask + g0, 4)) {
                m = *reinterpret_cast<const uint32_t*>(spec_mask + g0);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < n) m |= (uint32_t)spec_mask[g0 + j] << (8 * j);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) special[j] |= ((m >> (8 * j)) & 0xffu) != 0;
        }
        for (int k = 0; k < n_special; ++k) {
            const int64_t sid = s_special[k];
#pragma unroll
            for (int j = 0; j < 4; ++j) special[j] |= id[j] == sid;
        }

        int64_t oid[4], lab[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned long long g = (unsigned long long)(g0 + j);
            const uint4 u = philox4x32_10(make_uint4((uint32_t)g, (uint32_t)(g >> 32), plan.off_lo, plan.off_hi), key);
            const bool target = !special[j] && u.x < plan.thr_p;
            const int64_t word = (int64_t)(((unsigned long long)u.z * plan.vocab) >> 32);
            const int64_t repl = u.y < plan.thr_mask ? plan.mask_id : (u.y < plan.thr_rand ? word : id[j]);
            oid[j] = target ? repl : id[j];
            lab[j] = target ? id[j] : (int64_t)-100;
        }

        if (full && aligned(out_ids + g0, 16)) {
            store4_i64(out_ids + g0, oid);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n) out_ids[g0 + j] = oid[j];
        }
        if (full && aligned(labels + g0, 16)) {
            store4_i64(labels + g0, lab);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n) labels[g0 + j] = lab[j];
        }
    }
}

}  // namespace

extern "C" int cx_mlm_mask(const void* ids, int ids_i64, long ids_stride, const int64_t* attention_mask,
                           const uint8_t* special_mask, const int64_t* special_ids, int n_special, long mask_token_id,
                           int random_vocab, float p, unsigned long long seed, unsigned long long offset, int64_t* out_ids,
                           int64_t* labels, int B, int S, void* stream) {
    if (!ids || !out_ids || !labels || (n_special > 0 && !special_ids)) return CX_ERR_ARG;
    if (B < 1 || S < 1 || n_special < 0 || n_special > kMaxSpecial || random_vocab < 1 || !(p >= 0.f && p < 1.f)) return CX_ERR_SHAPE;
    if (ids_stride < S) return CX_ERR_SHAPE;
    MaskPlan plan;
    plan.thr_p = threshold(p);
    plan.thr_mask = threshold(0.8f);
    plan.thr_rand = threshold(0.9f);
    plan.vocab = (uint32_t)random_vocab;
    plan.seed_lo = (uint32_t)seed;
    plan.seed_hi = (uint32_t)(seed >> 32);
    plan.off_lo = (uint32_t)offset;
    plan.off_hi = (uint32_t)(offset >> 32);
    plan.mask_id = (int64_t)mask_token_id;
    const int nq = (S + 3) / 4;
    const long n_groups = (long)B * nq;
    const long want = (n_groups + kThreads - 1) / kThreads;
    const dim3 grid((unsigned)(want < kMaxBlocks ? want : kMaxBlocks));
    if (ids_i64)
        hipLaunchKernelGGL(mlm_mask_kernel<int64_t>, grid, dim3(kThreads), 0, (hipStream_t)stream, (const int64_t*)ids, ids_stride,
                           attention_mask, special_mask, special_ids, n_special, plan, out_ids, labels, S, nq, n_groups);
    else
        hipLaunchKernelGGL(mlm_mask_kernel<int32_t>, grid, dim3(kThreads), 0, (hipStream_t)stream, (const int32_t*)ids, ids_stride,
                           attention_mask, special_mask, special_ids, n_special, plan, out_ids, labels, S, nq, n_groups);
    return done();
}
