// image.hip -- crop + bicubic resize + normalize of a ragged batch of decoded RGB images, one launch per batch
// (sc/dataset/transform.py: RandomResizedCrop(S, BICUBIC) / Resize(S, BICUBIC) + CenterCrop(S), ToTensor, Normalize --
// torchvision on PIL images in the reference's loader workers).  The host keeps the JPEG decode only; this kernel turns
// the decoded HWC uint8 pixels into the (B, 3, S, S) fp32 / bf16 tensor the ViT engine takes.
//
// The arithmetic is PIL's two-pass BICUBIC including its 8-bit intermediate (tests/img_ref.py): per axis and
// output pixel o, centre c = origin + (o + 0.5) * scale (float64), taps [max(int(c - sup + .5), lo), min(int(c + sup + .5), hi)),
// sup = 2 * max(scale, 1), cubic weights (a = -0.5) normalised by their sum; the horizontal pass is rounded half up and clamped
// to 0..255, the vertical pass runs on those levels and is rounded and clamped again.
//
// A workgroup owns a band of output rows of one image:
//   setup    the 3 x 256 table of normalised output values (float64 chain, rounded once), the tap plan of every output
//            column and of the band's rows (first tap, count, first cubic argument, 1 / weight sum) -> LDS
//   pass A   horizontal: every (source row the band needs, output column) -> 8-bit levels in LDS, planar [row][c][x]
//   pass B   vertical out of LDS: every (band row, output column), three channels -> table lookup -> stores contiguous in x
// The band height comes from the image's y scale (band_rows): the source rows of a band fit a fixed LDS budget, or, for the
// largest downscales, a one-row band fits the CU's 160 KB.  Weights are recomputed per tap (a dozen VALU operations next to
// the three byte loads and FMAs of the tap): a table of them would not fit LDS at scale 16, and one code path serves every scale.
// No atomics; each output value is written once by one lane: a repeated launch gives the same bits.
#include "cx_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxS = 512, kMaxSide = 8192;
constexpr double kMaxScale = 16.0;
constexpr int kBandMax = 64;                 // output rows per band at most (the size of the row tap plan)
constexpr int kInterBudget = 48 * 1024;      // bytes of 8-bit intermediate a band aims for: three workgroups per CU
constexpr int kLdsMax = 160 * 1024;
constexpr int kTabBytes = 3 * 256 * 4;

struct Tap {
    int lo, n;      // first source index and number of taps
    float t0, inv;  // cubic argument of the first tap; 1 / sum of the weights (0 if there is no tap)
};

// upper bound on the source rows (or columns) that R consecutive output pixels of an axis with this scale touch:
// last tap end - first tap start < (R - 1) * scale + 2 * support + 1
__host__ __device__ inline int span_cap(int R, double scale) {
    const double fs = scale > 1.0 ? scale : 1.0;
    return (int)((R - 1) * scale) + 2 * (int)(2.0 * fs) + 5;
}
__host__ __device__ inline int band_rows(double y_scale, int S) {
    int R = S < kBandMax ? S : kBandMax;
    while (R > 1 && span_cap(R, y_scale) * 3 * S > kInterBudget) --R;
    return R;
}
__host__ __device__ inline int lds_fixed_bytes(int S) { return kTabBytes + (S + kBandMax) * (int)sizeof(Tap); }

CX_DEVICE float cubic(float t) {
    t = fabsf(t);
    if (t < 1.f) return (1.5f * t - 2.5f) * t * t + 1.f;
    if (t < 2.f) return (((t - 5.f) * t + 8.f) * t - 4.f) * -0.5f;
    return 0.f;
}
CX_DEVICE float tap_weight(const Tap& t, int k, float step) { return cubic(__builtin_fmaf((float)k, step, t.t0)) * t.inv; }

CX_DEVICE Tap axis_tap(int o, int lo, int hi, double origin, double scale) {
    const double fs = scale > 1.0 ? scale : 1.0, support = 2.0 * fs;
    const double c = origin + (o + 0.5) * scale;
    const int a = max((int)(c - support + 0.5), lo), b = min((int)(c + support + 0.5), hi);
    Tap t;
    t.lo = a;
    t.n = b > a ? b - a : 0;
    t.t0 = (float)(((double)a - c + 0.5) / fs);
    t.inv = 1.f;
    const float step = (float)(1.0 / fs);
    float sum = 0.f;
    for (int k = 0; k < t.n; ++k) sum += tap_weight(t, k, step);
    t.inv = sum != 0.f ? 1.f / sum : 0.f;
    return t;
}
CX_DEVICE int level_of(float acc) { return min(max((int)floorf(acc + 0.5f), 0), 255); }

struct Norm3 {
    float mean[3], std[3];
};

template <bool BF16>
__global__ __launch_bounds__(kThreads) void image_transform_kernel(const uint8_t* __restrict__ pixels, const int64_t* __restrict__ offsets,
                                                                   const int32_t* __restrict__ sizes, const int32_t* __restrict__ plan_i,
                                                                   const double* __restrict__ plan_f, void* __restrict__ out, int S,
                                                                   int inter_cap, Norm3 norm) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float* tab = reinterpret_cast<float*>(smem);                        // [3][256]
    Tap* xt = reinterpret_cast<Tap*>(smem + kTabBytes);                 // [S]
    Tap* yt = xt + S;                                                   // [kBandMax]
    uint8_t* inter = smem + lds_fixed_bytes(S);                         // [rows][3][S]

    const int b = blockIdx.y, tid = threadIdx.x;
    const double y_origin = plan_f[4 * b + 0], y_scale = plan_f[4 * b + 1], x_origin = plan_f[4 * b + 2], x_scale = plan_f[4 * b + 3];
    const int R = band_rows(y_scale, S);
    const int y0 = blockIdx.x * R;
    if (y0 >= S) return;
    const int nb = min(R, S - y0);
    const int y_lo = plan_i[4 * b + 0], y_hi = plan_i[4 * b + 1], x_lo = plan_i[4 * b + 2], x_hi = plan_i[4 * b + 3];
    const int W = sizes[2 * b + 1];
    const uint8_t* img = pixels + offsets[b];

    for (int i = tid; i < 3 * 256; i += kThreads) {
        const int c = i >> 8;
        tab[i] = (float)(((double)(i & 255) / 255.0 - (double)norm.mean[c]) / (double)norm.std[c]);
    }
    for (int x = tid; x < S; x += kThreads) xt[x] = axis_tap(x, x_lo, x_hi, x_origin, x_scale);
    for (int y = tid; y < nb; y += kThreads) yt[y] = axis_tap(y0 + y, y_lo, y_hi, y_origin, y_scale);
    __syncthreads();

    // the taps of a later output row start and end no earlier: the band reads source rows [r0, r1)
    const int r0 = yt[0].lo, r1 = yt[nb - 1].lo + yt[nb - 1].n;
    const int nrows = r1 - r0, row_bytes = 3 * S;
    if (nrows * row_bytes > inter_cap) return;   // (span_cap bounds nrows; never taken for a plan the host admitted)

    const float x_step = (float)(1.0 / (x_scale > 1.0 ? x_scale : 1.0)), y_step = (float)(1.0 / (y_scale > 1.0 ? y_scale : 1.0));
    for (int i = tid; i < nrows * S; i += kThreads) {
        const int r = i / S, x = i - r * S;
        const Tap t = xt[x];
        const uint8_t* p = img + ((size_t)(r0 + r) * W + t.lo) * 3;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int k = 0; k < t.n; ++k) {
            const float w = tap_weight(t, k, x_step);
            a0 += w * (float)p[3 * k + 0];
            a1 += w * (float)p[3 * k + 1];
            a2 += w * (float)p[3 * k + 2];
        }
        uint8_t* q = inter + r * row_bytes + x;
        q[0] = (uint8_t)level_of(a0);
        q[S] = (uint8_t)level_of(a1);
        q[2 * S] = (uint8_t)level_of(a2);
    }
    __syncthreads();

    const size_t plane = (size_t)S * S;
    for (int i = tid; i < nb * S; i += kThreads) {
        const int y = i / S, x = i - y * S;
        const Tap t = yt[y];
        const uint8_t* p = inter + (t.lo - r0) * row_bytes + x;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int k = 0; k < t.n; ++k) {
            const float w = tap_weight(t, k, y_step);
            a0 += w * (float)p[k * row_bytes];
            a1 += w * (float)p[k * row_bytes + S];
            a2 += w * (float)p[k * row_bytes + 2 * S];
        }
        const float v0 = tab[level_of(a0)], v1 = tab[256 + level_of(a1)], v2 = tab[512 + level_of(a2)];
        const size_t o = (size_t)b * 3 * plane + (size_t)(y0 + y) * S + x;
        if (BF16) {
            bf16_t* dst = reinterpret_cast<bf16_t*>(out);
            dst[o] = f32_to_bf16(v0);
            dst[o + plane] = f32_to_bf16(v1);
            dst[o + 2 * plane] = f32_to_bf16(v2);
        } else {
            float* dst = reinterpret_cast<float*>(out);
            dst[o] = v0;
            dst[o + plane] = v1;
            dst[o + 2 * plane] = v2;
        }
    }
}

// a pinned host array that the device reads at the same address (hipHostMalloc memory): the pointer itself, NULL for anything else
const void* pinned_device_ptr(const void* host) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, host) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return attr.type == hipMemoryTypeHost && attr.devicePointer == host ? host : nullptr;
}

}  // namespace

extern "C" int cx_image_transform(const uint8_t* pixels, const int64_t* offsets, const int32_t* sizes, const int32_t* plan_i,
                                  const double* plan_f, void* out, int out_bf16, int B, int S, const float* mean3,
                                  const float* std3, void* stream) {
    if (!pixels || !offsets || !sizes || !plan_i || !plan_f || !out || !mean3 || !std3 || B <= 0) return CX_ERR_ARG;
    if (S < 1 || S > kMaxS || B > 65535) return CX_ERR_SHAPE;   // (B is grid.y)
    const int64_t* d_offsets = static_cast<const int64_t*>(pinned_device_ptr(offsets));
    const int32_t* d_sizes = static_cast<const int32_t*>(pinned_device_ptr(sizes));
    const int32_t* d_plan_i = static_cast<const int32_t*>(pinned_device_ptr(plan_i));
    const double* d_plan_f = static_cast<const double*>(pinned_device_ptr(plan_f));
    if (!d_offsets || !d_sizes || !d_plan_i || !d_plan_f) return CX_ERR_ARG;
    Norm3 norm;
    for (int c = 0; c < 3; ++c) {
        norm.mean[c] = mean3[c];
        norm.std[c] = std3[c];
        if (!(std3[c] > 0.f) || !(mean3[c] == mean3[c])) return CX_ERR_ARG;
    }
    int max_bands = 0, max_inter = 0;
    if (offsets[0] < 0) return CX_ERR_SHAPE;
    for (int b = 0; b < B; ++b) {
        const int h = sizes[2 * b], w = sizes[2 * b + 1];
        if (h < 1 || h > kMaxSide || w < 1 || w > kMaxSide) return CX_ERR_SHAPE;
        if (offsets[b + 1] - offsets[b] < (int64_t)3 * h * w) return CX_ERR_SHAPE;
        for (int ax = 0; ax < 2; ++ax) {
            const int lo = plan_i[4 * b + 2 * ax], hi = plan_i[4 * b + 2 * ax + 1], side = ax ? w : h;
            const double origin = plan_f[4 * b + 2 * ax], scale = plan_f[4 * b + 2 * ax + 1];
            if (lo < 0 || hi <= lo || hi > side) return CX_ERR_SHAPE;
            if (!(scale > 0.0) || !(scale <= kMaxScale)) return CX_ERR_SHAPE;
            if (!(origin >= lo - scale) || !(origin + S * scale <= hi + scale)) return CX_ERR_SHAPE;
        }
        const double y_scale = plan_f[4 * b + 1];
        const int R = band_rows(y_scale, S);
        const int bands = (S + R - 1) / R, inter = span_cap(R, y_scale) * 3 * S;
        max_bands = bands > max_bands ? bands : max_bands;
        max_inter = inter > max_inter ? inter : max_inter;
    }
    max_inter = (max_inter + 15) & ~15;
    const int lds = lds_fixed_bytes(S) + max_inter;
    if (lds > kLdsMax) return CX_ERR_SHAPE;
    static CxLdsOptIn opt_f32, opt_bf16;
    const dim3 grid(max_bands, B);
    if (out_bf16) {
        if (!opt_bf16.ensure(reinterpret_cast<const void*>(&image_transform_kernel<true>), kLdsMax)) return CX_ERR_LAUNCH;
        hipLaunchKernelGGL(image_transform_kernel<true>, grid, dim3(kThreads), lds, (hipStream_t)stream, pixels, d_offsets, d_sizes,
                           d_plan_i, d_plan_f, out, S, max_inter, norm);
    } else {
        if (!opt_f32.ensure(reinterpret_cast<const void*>(&image_transform_kernel<false>), kLdsMax)) return CX_ERR_LAUNCH;
        hipLaunchKernelGGL(image_transform_kernel<false>, grid, dim3(kThreads), lds, (hipStream_t)stream, pixels, d_offsets, d_sizes,
                           d_plan_i, d_plan_f, out, S, max_inter, norm);
    }
    return done();
}
