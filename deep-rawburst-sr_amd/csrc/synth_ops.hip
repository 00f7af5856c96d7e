// Synthetic training data on the device: the reference's rgb2rawburst (data/synthetic_burst_generation.py:23-246
// over data/camera_pipeline.py) and its inverse for viewing, process_linear_image_rgb
// (data/postprocessing_functions.py:32-50).  fp32, stream-ordered, no host synchronisation, no allocation; every
// per-image parameter is read from device memory, so the calls can sit in a captured graph.
//
//   dbsr_unprocess_rgb    sRGB crop -> linear sensor space: invert_smoothstep, gamma_expansion, apply_ccm(rgb2cam),
//                         safe_invert_gains, clamp (rgb2rawburst:60-77)
//   dbsr_burst_synth      N affinely transformed, downsampled frames of the linear image, mosaicked (RGGB) with
//                         shot / read noise, plus the RGB burst and the flow to frame 0 (single2lrburst, mosaic,
//                         add_noise); the warp is defined in include/dbsr_hip.h, not by OpenCV's fixed point
//   dbsr_postprocess_rgb  linear sensor space -> sRGB: apply_gains, apply_ccm(cam2rgb), gamma_compression,
//                         apply_smoothstep, with the clamps in between
//
// The arithmetic is the reference's, operation for operation (sinf / asinf / powf / sqrtf and IEEE division, no
// fast variants), and multiply-add contraction is off for the whole file: the tests hold these kernels to the
// reference's own fp32 rounding error, so each product is rounded before it is added, as torch's elementwise ops do.
// Plain global loads and stores (no LDS, no LDS-DMA, no inline assembly); the pointwise kernels move 16 bytes per
// access when the rows allow it.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int NP = 16;                                     // floats per image in `params`

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

struct Cam {                                               // one image's row of `params`
    float m[9];
    float rgb_gain, red_gain, blue_gain;
    bool smoothstep, gamma;
};
__device__ __forceinline__ Cam load_cam(const float* __restrict__ p) {
    Cam c;
#pragma unroll
    for (int i = 0; i < 9; ++i) c.m[i] = p[i];
    c.rgb_gain = p[9];
    c.red_gain = p[10];
    c.blue_gain = p[11];
    c.smoothstep = p[12] != 0.f;
    c.gamma = p[13] != 0.f;
    return c;
}
__device__ __forceinline__ void ccm3(const float (&m)[9], float& r, float& g, float& b) {
    const float o0 = m[0] * r + m[1] * g + m[2] * b;
    const float o1 = m[3] * r + m[4] * g + m[5] * b;
    const float o2 = m[6] * r + m[7] * g + m[8] * b;
    r = o0;
    g = o1;
    b = o2;
}

// rgb2rawburst:60-77 on one pixel
__device__ __forceinline__ void unprocess_px(const Cam& c, float& r, float& g, float& b) {
    float v[3] = {r, g, b};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float x = v[k];
        if (c.smoothstep) x = 0.5f - sinf(asinf(1.0f - 2.0f * clamp01(x)) / 3.0f);
        if (c.gamma) x = powf(fmaxf(x, 1e-8f), 2.2f);
        v[k] = x;
    }
    ccm3(c.m, v[0], v[1], v[2]);
    const float gains[3] = {(1.0f / c.red_gain) / c.rgb_gain, 1.0f / c.rgb_gain, (1.0f / c.blue_gain) / c.rgb_gain};
    const float gray = (v[0] + v[1] + v[2]) / 3.0f;
    const float t = fmaxf(gray - 0.9f, 0.f) / 0.1f;         // inflection 0.9, (1 - 0.9) rounded to fp32
    const float mask = t * t;
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = clamp01(v[k] * fmaxf(mask + (1.0f - mask) * gains[k], gains[k]));
    r = v[0];
    g = v[1];
    b = v[2];
}

// process_linear_image_rgb on one pixel; flags: the caller's DBSR_POST_* switches
__device__ __forceinline__ void postprocess_px(const Cam& c, int flags, float& r, float& g, float& b) {
    float v[3] = {r, g, b};
    if (flags & DBSR_POST_GAINS) {
        v[0] = clamp01(v[0] * (c.red_gain * c.rgb_gain));
        v[1] = clamp01(v[1] * c.rgb_gain);
        v[2] = clamp01(v[2] * (c.blue_gain * c.rgb_gain));
    }
    if (flags & DBSR_POST_CCM) ccm3(c.m, v[0], v[1], v[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float x = clamp01(v[k]);
        if (c.gamma && (flags & DBSR_POST_GAMMA)) x = powf(fmaxf(x, 1e-8f), (float)(1.0 / 2.2));
        if (c.smoothstep && (flags & DBSR_POST_SMOOTHSTEP)) x = 3.0f * (x * x) - 2.0f * (x * x * x);
        v[k] = clamp01(x);
    }
    r = v[0];
    g = v[1];
    b = v[2];
}

// Four adjacent pixels of a row, all three channels.  VEC: W % 4 == 0 and every pointer allows the wide access
// (16 B for the fp32 planes, 4 B for the interleaved bytes), so a quad is one float4 per plane or three dwords.
struct Quad {
    float v[3][4];
};
template <bool VEC>
__device__ __forceinline__ Quad load_planes(const float* __restrict__ img, long long plane, long long o, int n) {
    Quad q;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* p = img + c * plane + o;
        if (VEC) {
            const float4 t = *(const float4*)p;
            q.v[c][0] = t.x; q.v[c][1] = t.y; q.v[c][2] = t.z; q.v[c][3] = t.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) q.v[c][i] = i < n ? p[i] : 0.f;
        }
    }
    return q;
}
template <bool VEC>
__device__ __forceinline__ void store_planes(float* __restrict__ img, long long plane, long long o, int n,
                                             const Quad& q) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* p = img + c * plane + o;
        if (VEC) {
            *(float4*)p = make_float4(q.v[c][0], q.v[c][1], q.v[c][2], q.v[c][3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < n) p[i] = q.v[c][i];
        }
    }
}
// interleaved RGB bytes of pixels [o, o + n): value / 255
template <bool VEC>
__device__ __forceinline__ Quad load_bytes(const unsigned char* __restrict__ src, long long o, int n) {
    unsigned char by[12];
    if (VEC) {
        const unsigned* p = (const unsigned*)(src + 3 * o);
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            const unsigned u = p[w];
#pragma unroll
            for (int k = 0; k < 4; ++k) by[4 * w + k] = (unsigned char)(u >> (8 * k));
        }
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) by[i] = i < 3 * n ? src[3 * o + i] : (unsigned char)0;
    }
    Quad q;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) q.v[c][i] = (float)by[3 * i + c] / 255.0f;
    return q;
}
// interleaved RGB bytes (uint8)(v * 255): torch_to_npimage's truncation (v is already clamped to [0, 1])
template <bool VEC>
__device__ __forceinline__ void store_bytes(unsigned char* __restrict__ dst, long long o, int n, const Quad& q) {
    unsigned char by[12];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) by[3 * i + c] = (unsigned char)(q.v[c][i] * 255.0f);
    if (VEC) {
        unsigned* p = (unsigned*)(dst + 3 * o);
#pragma unroll
        for (int w = 0; w < 3; ++w)
            p[w] = (unsigned)by[4 * w] | ((unsigned)by[4 * w + 1] << 8) | ((unsigned)by[4 * w + 2] << 16) |
                   ((unsigned)by[4 * w + 3] << 24);
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i)
            if (i < 3 * n) dst[3 * o + i] = by[i];
    }
}

// One thread per quad of a row; quads = B * H * ceil(W / 4).
template <bool VEC, bool U8>
__global__ __launch_bounds__(256) void unprocess_kernel(long long quads, int H, int W, const void* __restrict__ src,
                                                        const float* __restrict__ params, float* __restrict__ lin) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= quads) return;
    const int qw = (W + 3) / 4;
    const int xq = (int)(t % qw);
    const long long row = t / qw;                          // b * H + y
    const int b = (int)(row / H), y = (int)(row % H);
    const int x = 4 * xq, n = min(4, W - x);
    const long long plane = (long long)H * W;
    const Cam cam = load_cam(params + (long long)b * NP);
    Quad q = U8 ? load_bytes<VEC>((const unsigned char*)src, (long long)b * plane + (long long)y * W + x, n)
                : load_planes<VEC>((const float*)src + 3 * b * plane, plane, (long long)y * W + x, n);
#pragma unroll
    for (int i = 0; i < 4; ++i) unprocess_px(cam, q.v[0][i], q.v[1][i], q.v[2][i]);
    store_planes<VEC>(lin + 3 * b * plane, plane, (long long)y * W + x, n, q);
}

template <bool VEC>
__global__ __launch_bounds__(256) void postprocess_kernel(long long quads, int H, int W, const float* __restrict__ img,
                                                          const float* __restrict__ params, int flags,
                                                          float* __restrict__ out_f32,
                                                          unsigned char* __restrict__ out_u8) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= quads) return;
    const int qw = (W + 3) / 4;
    const int xq = (int)(t % qw);
    const long long row = t / qw;
    const int b = (int)(row / H), y = (int)(row % H);
    const int x = 4 * xq, n = min(4, W - x);
    const long long plane = (long long)H * W;
    const Cam cam = load_cam(params + (long long)b * NP);
    Quad q = load_planes<VEC>(img + 3 * b * plane, plane, (long long)y * W + x, n);
#pragma unroll
    for (int i = 0; i < 4; ++i) postprocess_px(cam, flags, q.v[0][i], q.v[1][i], q.v[2][i]);
    if (out_f32) store_planes<VEC>(out_f32 + 3 * b * plane, plane, (long long)y * W + x, n, q);
    if (out_u8) store_bytes<VEC>(out_u8, (long long)b * plane + (long long)y * W + x, n, q);
}

// ------------------------------------------------------------------------------------------------- the burst
// bil(P, (x, y)): the four taps around (x, y), weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy, summed in that
// order; a tap outside the H x W plane contributes 0 (cv2.BORDER_CONSTANT).  The float position is clamped before
// it becomes an index, so any `ainv` (NaN included) stays inside the plane: at -2 or W both taps of the axis are
// outside.
struct BilTaps {
    int o[4];                                              // offsets into a plane, -1: outside
    float w[4];
};
__device__ __forceinline__ BilTaps bil_taps(float x, float y, int H, int W) {
    const float xf = floorf(x), yf = floorf(y);
    const float fx = x - xf, fy = y - yf;
    const int x0 = (int)fminf(fmaxf(xf, -2.f), (float)W), y0 = (int)fminf(fmaxf(yf, -2.f), (float)H);
    const bool xin0 = x0 >= 0 && x0 < W, xin1 = x0 + 1 >= 0 && x0 + 1 < W;
    const bool yin0 = y0 >= 0 && y0 < H, yin1 = y0 + 1 >= 0 && y0 + 1 < H;
    BilTaps t;
    t.o[0] = xin0 && yin0 ? y0 * W + x0 : -1;
    t.o[1] = xin1 && yin0 ? y0 * W + x0 + 1 : -1;
    t.o[2] = xin0 && yin1 ? (y0 + 1) * W + x0 : -1;
    t.o[3] = xin1 && yin1 ? (y0 + 1) * W + x0 + 1 : -1;
    t.w[0] = (1.0f - fx) * (1.0f - fy);
    t.w[1] = fx * (1.0f - fy);
    t.w[2] = (1.0f - fx) * fy;
    t.w[3] = fx * fy;
    return t;
}
__device__ __forceinline__ float bil_apply(const float* __restrict__ P, const BilTaps& t) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) s = s + t.w[k] * (t.o[k] >= 0 ? P[t.o[k]] : 0.f);
    return s;
}

// One thread per RAW element position (b, n, y, x): the 2 x 2 quad of RGB pixels (2y + dy, 2x + dx) it is made of.
// RGB: all three channels of each pixel are sampled and burst_rgb is written; otherwise only the channel the RAW
// plane of that pixel takes.  The RAW values come from the same operations either way.
template <bool RGB>
__global__ __launch_bounds__(256) void burst_synth_kernel(long long total, int N, int Hc, int Wc, int bc, int f, int H2,
                                                          int W2, const float* __restrict__ lin,
                                                          const float* __restrict__ ainv,
                                                          const float* __restrict__ noise_levels,
                                                          const float* __restrict__ z, float* __restrict__ burst,
                                                          float* __restrict__ burst_rgb, float* __restrict__ flow) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int Hr = H2 / 2, Wr = W2 / 2;
    const int x = (int)(t % Wr);
    long long r = t / Wr;
    const int y = (int)(r % Hr);
    const long long bn = r / Hr;                           // b * N + n
    const int b = (int)(bn / N);
    const float* A = ainv + bn * 6;
    const float a00 = A[0], a01 = A[1], a02 = A[2], a10 = A[3], a11 = A[4], a12 = A[5];
    const long long plane = (long long)Hc * Wc;
    const float* L = lin + 3 * b * plane;
    const int t0 = (f & 1) ? (f - 1) / 2 : f / 2 - 1, nt = (f & 1) ? 1 : 2;      // the taps T_f
    const float inv = 1.0f / (float)(nt * nt);
    float d00 = 0.f, d01 = 0.f, d02 = 0.f, d10 = 0.f, d11 = 0.f, d12 = 0.f;
    if (flow) {
        const float* A0 = ainv + (long long)b * N * 6;
        d00 = a00 - A0[0]; d01 = a01 - A0[1]; d02 = a02 - A0[2];
        d10 = a10 - A0[3]; d11 = a11 - A0[4]; d12 = a12 - A0[5];
    }
    const float fc = 0.5f * (float)(f - 1);
    float raw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                          // k = 2 dy + dx: R, Gr, Gb, B
        const int dy = k >> 1, dx = k & 1;
        const int ck = dy + dx;                            // 0, 1, 1, 2
        const int Y = 2 * y + dy, X = 2 * x + dx;
        float acc[3] = {0.f, 0.f, 0.f};
        for (int j = 0; j < nt; ++j)
            for (int i = 0; i < nt; ++i) {
                const float px = (float)(bc + f * X + t0 + i), py = (float)(bc + f * Y + t0 + j);
                const float sx = a00 * px + a01 * py + a02, sy = a10 * px + a11 * py + a12;
                const BilTaps tp = bil_taps(sx, sy, Hc, Wc);
                if (RGB) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[c] = acc[c] + bil_apply(L + c * plane, tp);
                } else {
                    acc[ck] = acc[ck] + bil_apply(L + ck * plane, tp);
                }
            }
        if (RGB) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                acc[c] = acc[c] * inv;
                burst_rgb[((bn * 3 + c) * H2 + Y) * W2 + X] = acc[c];
            }
        } else {
            acc[ck] = acc[ck] * inv;
        }
        raw[k] = acc[ck];
        if (flow) {
            const float px = (float)(bc + f * X) + fc, py = (float)(bc + f * Y) + fc;
            flow[((bn * 2 + 0) * H2 + Y) * W2 + X] = (d00 * px + d01 * py + d02) / (float)f;
            flow[((bn * 2 + 1) * H2 + Y) * W2 + X] = (d10 * px + d11 * py + d12) / (float)f;
        }
    }
    float shot = 0.f, read = 0.f;
    if (z) {
        shot = noise_levels[2 * b];
        read = noise_levels[2 * b + 1];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long o = ((bn * 4 + k) * Hr + y) * Wr + x;
        float v = raw[k];
        if (z) v = v + z[o] * sqrtf(v * shot + read);
        burst[o] = clamp01(v);
    }
}

inline bool aligned(const void* p, size_t a) { return p == nullptr || ((uintptr_t)p % a) == 0; }
inline unsigned blocks256(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int dbsr_unprocess_rgb(int B, int Hc, int Wc, const void* src, int src_format, const float* params,
                                  float* lin, void* stream) {
    DBSR_CHECK_ARG(src && params && lin, "unprocess_rgb: null pointer (src, params, lin)");
    DBSR_CHECK_ARG(B > 0 && Hc > 0 && Wc > 0, "unprocess_rgb: bad sizes B %d, Hc %d, Wc %d", B, Hc, Wc);
    DBSR_CHECK_ARG(src_format == DBSR_SRC_F32_NCHW || src_format == DBSR_SRC_U8_NHWC,
                   "unprocess_rgb: unknown src_format %d (0: fp32 NCHW, 1: uint8 NHWC)", src_format);
    DBSR_CHECK_ARG(3LL * B * Hc * Wc < (1LL << 31), "unprocess_rgb: 3 * B * Hc * Wc must be < 2^31");
    const long long quads = (long long)B * Hc * ((Wc + 3) / 4);
    const bool u8 = src_format == DBSR_SRC_U8_NHWC;
    const bool vec = Wc % 4 == 0 && aligned(lin, 16) && aligned(src, u8 ? 4 : 16);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(blocks256(quads)), block(256);
    if (u8 && vec) hipLaunchKernelGGL((unprocess_kernel<true, true>), grid, block, 0, s, quads, Hc, Wc, src, params, lin);
    else if (u8) hipLaunchKernelGGL((unprocess_kernel<false, true>), grid, block, 0, s, quads, Hc, Wc, src, params, lin);
    else if (vec) hipLaunchKernelGGL((unprocess_kernel<true, false>), grid, block, 0, s, quads, Hc, Wc, src, params, lin);
    else hipLaunchKernelGGL((unprocess_kernel<false, false>), grid, block, 0, s, quads, Hc, Wc, src, params, lin);
    DBSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int dbsr_burst_synth(int B, int N, int Hc, int Wc, int bc, int f, const float* lin, const float* ainv,
                                const float* noise_levels, const float* z, float* burst, float* burst_rgb,
                                float* flow, void* stream) {
    DBSR_CHECK_ARG(lin && ainv && burst, "burst_synth: null pointer (lin, ainv, burst)");
    DBSR_CHECK_ARG(B > 0 && N > 0 && Hc > 0 && Wc > 0, "burst_synth: bad sizes B %d, N %d, Hc %d, Wc %d", B, N, Hc, Wc);
    DBSR_CHECK_ARG(f >= 1, "burst_synth: downsample factor %d must be >= 1", f);
    DBSR_CHECK_ARG(bc >= 0 && 2LL * bc < (Hc < Wc ? Hc : Wc), "burst_synth: border_crop %d leaves nothing of %d x %d",
                   bc, Hc, Wc);
    DBSR_CHECK_ARG((Hc - 2 * bc) % f == 0 && (Wc - 2 * bc) % f == 0,
                   "burst_synth: %d x %d inside the border is not divisible by the factor %d", Hc - 2 * bc,
                   Wc - 2 * bc, f);
    const int H2 = (Hc - 2 * bc) / f, W2 = (Wc - 2 * bc) / f;
    DBSR_CHECK_ARG(H2 > 0 && W2 > 0 && H2 % 2 == 0 && W2 % 2 == 0,
                   "burst_synth: the downsampled frame %d x %d must be even (RGGB mosaic)", H2, W2);
    DBSR_CHECK_ARG((z == nullptr) == (noise_levels == nullptr),
                   "burst_synth: z and noise_levels go together (both null: no noise)");
    DBSR_CHECK_ARG(3LL * B * Hc * Wc < (1LL << 31) && 3LL * B * N * H2 * W2 < (1LL << 31),
                   "burst_synth: 3 * B * Hc * Wc and 3 * B * N * H2 * W2 must be < 2^31");
    const long long total = (long long)B * N * (H2 / 2) * (W2 / 2);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(blocks256(total)), block(256);
    if (burst_rgb)
        hipLaunchKernelGGL(burst_synth_kernel<true>, grid, block, 0, s, total, N, Hc, Wc, bc, f, H2, W2, lin, ainv,
                           noise_levels, z, burst, burst_rgb, flow);
    else
        hipLaunchKernelGGL(burst_synth_kernel<false>, grid, block, 0, s, total, N, Hc, Wc, bc, f, H2, W2, lin, ainv,
                           noise_levels, z, burst, burst_rgb, flow);
    DBSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int dbsr_postprocess_rgb(int B, int H, int W, const float* img, const float* params, int flags,
                                    float* out_f32, unsigned char* out_u8, void* stream) {
    DBSR_CHECK_ARG(img && params, "postprocess_rgb: null pointer (img, params)");
    DBSR_CHECK_ARG(out_f32 || out_u8, "postprocess_rgb: no output (out_f32 and out_u8 are both null)");
    DBSR_CHECK_ARG(B > 0 && H > 0 && W > 0, "postprocess_rgb: bad sizes B %d, H %d, W %d", B, H, W);
    DBSR_CHECK_ARG(flags >= 0 && flags < 16, "postprocess_rgb: flags %d (bits: 1 gains, 2 ccm, 4 gamma, 8 smoothstep)",
                   flags);
    DBSR_CHECK_ARG(3LL * B * H * W < (1LL << 31), "postprocess_rgb: 3 * B * H * W must be < 2^31");
    const long long quads = (long long)B * H * ((W + 3) / 4);
    const bool vec = W % 4 == 0 && aligned(img, 16) && aligned(out_f32, 16) && aligned(out_u8, 4);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(blocks256(quads)), block(256);
    if (vec) hipLaunchKernelGGL(postprocess_kernel<true>, grid, block, 0, s, quads, H, W, img, params, flags, out_f32, out_u8);
    else hipLaunchKernelGGL(postprocess_kernel<false>, grid, block, 0, s, quads, H, W, img, params, flags, out_f32, out_u8);
    DBSR_LAUNCH_CHECK();
    return 0;
}
