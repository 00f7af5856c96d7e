// LPIPS (the `lpips` package's v0.1 metric, as image_quality_v2.LPIPS calls it) around the library's fp32 convs:
// the input preparation, the backbone's max-pools and the per-layer distance.  fp32, NHWC, on the caller's
// stream, no host read, no float atomics.
//
//   dbsr_lpips_prep    pred, gt [B,3,H,W] NCHW -> [2B,Hc,Wc,8] NHWC (pred images first): boundary crop, optional
//                      channel flip, optional 2x - 1, then (x - shift) / scale as a division; channels 3..7 zero
//                      (the first conv reads cin_pad(3) = 8 channels).
//   dbsr_maxpool2d     NHWC k x k / stride s, floor mode, no padding; one 16-byte run of channels per lane.
//   dbsr_lpips_layer   one tapped feature tensor [2B,h,w,C] and lin[C] ->
//                        d[b,y,x] = sum_c lin[c] (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2,
//                      its mean over y, x into per_layer[b][layer] and, in layer order, into value[b].
//
// The layer kernel runs one wave per pixel pair.  A lane loads its 16-byte channel pieces of both images once
// (C <= 512: at most two pieces per image) and keeps them; the two squared norms are reduced over the wave, then
// the weighted squared difference of the normalised vectors is formed from the same registers and reduced.  It
// is the two-pass form on purpose: the one-pass expansion in sum w f0^2, sum w f0 f1, sum w f1^2 cancels when
// pred is close to gt.  Every lane of a wave ends a butterfly reduction with the same bits (a + b = b + a), the
// waves of a block add their pixels in a fixed order, and one block adds the per-block partials in a fixed
// order, so two runs are bitwise equal; a block never holds pixels of two images, so an image's value does not
// depend on its batch.
#include "common.hpp"

#include <cmath>

using namespace dbsr;

namespace {

constexpr int LP_WAVES = 4;                       // waves per block of the layer kernel
constexpr int LP_PIX = 32;                        // pixel pairs per block (LP_PIX / LP_WAVES per wave, in turn)
constexpr float LP_EPS = 1e-10f;
constexpr int ALEX_MIN = 31, VGG_MIN = 16;        // smallest crop side: the last pool still has a row

struct LpipsScale { float shift[3], scale[3]; };

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// ------------------------------------------------------------------------------------------------------- prep
// One thread per output pixel of the [2B, Hc, Wc] batch.
__global__ __launch_bounds__(256) void lpips_prep_kernel(int B, int H, int W, int bi, int flip, int normalize,
                                                         const float* __restrict__ pred, const float* __restrict__ gt,
                                                         LpipsScale sc, float* __restrict__ out, int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int Hc = H - 2 * bi, Wc = W - 2 * bi;
    const int x = i % Wc;
    const int t = i / Wc;
    const int y = t % Hc;
    const int n = t / Hc;                          // 0..2B-1
    const float* src = (n < B ? pred + (long long)n * 3 * H * W : gt + (long long)(n - B) * 3 * H * W) +
                       (long long)(bi + y) * W + bi + x;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float a = src[(long long)(flip ? 2 - c : c) * H * W];
        if (normalize) a = 2.f * a - 1.f;
        v[c] = (a - sc.shift[c]) / sc.scale[c];
    }
    float4* o = (float4*)(out + (long long)i * 8);
    o[0] = make_float4(v[0], v[1], v[2], 0.f);
    o[1] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---------------------------------------------------------------------------------------------------- maxpool
// One thread per (output pixel, 4 channels).  NaN propagates, as in torch's max_pool2d.
__global__ __launch_bounds__(256) void maxpool_kernel(int H, int W, int C4, int k, int s, int oh, int ow,
                                                      const float* __restrict__ x, int ldx, float* __restrict__ y,
                                                      int ldy, int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c4 = i % C4;
    int t = i / C4;
    const int ox = t % ow;
    t /= ow;
    const int oy = t % oh;
    const int n = t / oh;
    const float* src = x + (((long long)n * H + (long long)oy * s) * W + (long long)ox * s) * ldx + 4 * c4;
    float4 m = *(const float4*)src;
    for (int dy = 0; dy < k; ++dy)
        for (int dx = 0; dx < k; ++dx) {
            const float4 v = *(const float4*)(src + ((long long)dy * W + dx) * ldx);
            m.x = (v.x > m.x || v.x != v.x) ? v.x : m.x;
            m.y = (v.y > m.y || v.y != v.y) ? v.y : m.y;
            m.z = (v.z > m.z || v.z != v.z) ? v.z : m.z;
            m.w = (v.w > m.w || v.w != v.w) ? v.w : m.w;
        }
    *(float4*)(y + (((long long)n * oh + oy) * ow + ox) * ldy + 4 * c4) = m;
}

// ------------------------------------------------------------------------------------------------------ layer
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// PIECES: 16-byte channel pieces per lane and image (1: C <= 256, 2: C <= 512).
// Block blk of image b owns pixels [blk * LP_PIX, blk * LP_PIX + LP_PIX) of the h*w map; wave wv takes the
// pixels wv, wv + LP_WAVES, ... of them in turn.
template <int PIECES>
__global__ __launch_bounds__(LP_WAVES * 64) void lpips_layer_kernel(int B, int hw, int C, int bpi,
                                                                    const float* __restrict__ feat,
                                                                    const float* __restrict__ lin,
                                                                    float* __restrict__ map,
                                                                    float* __restrict__ partial) {
    __shared__ float ws[LP_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x / bpi, blk = blockIdx.x - b * bpi;
    const float* F0 = feat + (long long)b * hw * C;
    const float* F1 = feat + (long long)(B + b) * hw * C;

    float4 w[PIECES];
    bool on[PIECES];
#pragma unroll
    for (int q = 0; q < PIECES; ++q) {
        const int c = 4 * (lane + 64 * q);
        on[q] = c < C;
        w[q] = on[q] ? *(const float4*)(lin + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }

    // UN pixels' loads are issued before the first is used: one pixel pair is 512 B per piece, too little in
    // flight per wave to keep HBM busy.  The pixels are still finished one by one, in order.
    constexpr int UN = PIECES == 1 ? 4 : 2;
    static_assert((LP_PIX / LP_WAVES) % UN == 0, "pixel groups");
    float acc = 0.f;
    for (int j0 = 0; j0 < LP_PIX / LP_WAVES; j0 += UN) {
        if (blk * LP_PIX + j0 * LP_WAVES + wv >= hw) break;   // wave-uniform; later pixels lie further out
        float4 a[UN][PIECES], g[UN][PIECES];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int p = blk * LP_PIX + (j0 + u) * LP_WAVES + wv;
#pragma unroll
            for (int q = 0; q < PIECES; ++q) {
                const long long o = (long long)p * C + 4 * (lane + 64 * q);
                const bool ld = on[q] && p < hw;
                a[u][q] = ld ? *(const float4*)(F0 + o) : make_float4(0.f, 0.f, 0.f, 0.f);
                g[u][q] = ld ? *(const float4*)(F1 + o) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int p = blk * LP_PIX + (j0 + u) * LP_WAVES + wv;
            if (p < hw) {                                      // wave-uniform
                float s0 = 0.f, s1 = 0.f;
#pragma unroll
                for (int q = 0; q < PIECES; ++q) {
                    s0 = fmaf(a[u][q].x, a[u][q].x, s0); s0 = fmaf(a[u][q].y, a[u][q].y, s0);
                    s0 = fmaf(a[u][q].z, a[u][q].z, s0); s0 = fmaf(a[u][q].w, a[u][q].w, s0);
                    s1 = fmaf(g[u][q].x, g[u][q].x, s1); s1 = fmaf(g[u][q].y, g[u][q].y, s1);
                    s1 = fmaf(g[u][q].z, g[u][q].z, s1); s1 = fmaf(g[u][q].w, g[u][q].w, s1);
                }
                const float n0 = sqrtf(wave_sum(s0)) + LP_EPS, n1 = sqrtf(wave_sum(s1)) + LP_EPS;
                float d = 0.f;
#pragma unroll
                for (int q = 0; q < PIECES; ++q) {
                    float t;
                    t = a[u][q].x / n0 - g[u][q].x / n1; d = fmaf(w[q].x * t, t, d);
                    t = a[u][q].y / n0 - g[u][q].y / n1; d = fmaf(w[q].y * t, t, d);
                    t = a[u][q].z / n0 - g[u][q].z / n1; d = fmaf(w[q].z * t, t, d);
                    t = a[u][q].w / n0 - g[u][q].w / n1; d = fmaf(w[q].w * t, t, d);
                }
                d = wave_sum(d);
                if (map && lane == 0) map[(long long)b * hw + p] = d;
                acc += d;
            }
        }
    }
    if (lane == 0) ws[wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = ws[0];
#pragma unroll
        for (int i = 1; i < LP_WAVES; ++i) s += ws[i];
        partial[blockIdx.x] = s;
    }
}

// One block: per image, the partials added in double in a fixed order (strided per thread, then a tree), the
// mean over the map as fp32 into per_layer[b][layer], and value[b] = (layer ? value[b] : 0) + that.
__global__ __launch_bounds__(256) void lpips_finish_kernel(int B, int bpi, int hw, int layer,
                                                           const float* __restrict__ partial,
                                                           float* __restrict__ per_layer, float* __restrict__ value) {
    __shared__ double red[256];
    for (int b = 0; b < B; ++b) {
        double s = 0.0;
        for (int i = threadIdx.x; i < bpi; i += 256) s += (double)partial[(long long)b * bpi + i];
        __syncthreads();
        red[threadIdx.x] = s;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const float m = (float)(red[0] / (double)hw);
            per_layer[b * 5 + layer] = m;
            value[b] = (layer ? value[b] : 0.f) + m;
        }
    }
}

inline bool layer_c_ok(int C) { return C == 64 || C == 128 || C == 192 || C == 256 || C == 384 || C == 512; }
inline bool layer_sizes_ok(int B, int h, int w, int C) {
    return B > 0 && h > 0 && w > 0 && layer_c_ok(C) && 2LL * B * h * w * C < (1LL << 31);
}
inline int layer_bpi(int h, int w) { return cdiv((long long)h * w, LP_PIX); }

}  // namespace

extern "C" int dbsr_lpips_prep(int B, int H, int W, int boundary_ignore, int net, int bgr2rgb, int normalize,
                               const float* pred, const float* gt, float* out, void* stream) {
    DBSR_CHECK_ARG(pred && gt && out, "lpips_prep: null pointer (pred, gt, out)");
    DBSR_CHECK_ARG(B > 0 && H > 0 && W > 0, "lpips_prep: bad sizes");
    DBSR_CHECK_ARG(net == DBSR_LPIPS_ALEX || net == DBSR_LPIPS_VGG, "lpips_prep: net must be 0 (alex) or 1 (vgg)");
    DBSR_CHECK_ARG(boundary_ignore >= 0 && boundary_ignore < (1 << 28), "lpips_prep: boundary_ignore must be >= 0");
    const long long Hc = (long long)H - 2LL * boundary_ignore, Wc = (long long)W - 2LL * boundary_ignore;
    const int need = net == DBSR_LPIPS_ALEX ? ALEX_MIN : VGG_MIN;
    DBSR_CHECK_ARG(Hc >= need && Wc >= need, "lpips_prep: the crop %lld x %lld is smaller than %d x %d (%s)", Hc, Wc,
                   need, need, net == DBSR_LPIPS_ALEX ? "alex" : "vgg");
    // the output holds 8 channels per pixel of both images: 2 B Hc Wc 8 <= 16/3 B 3 H W
    DBSR_CHECK_ARG((long long)B * 3 * H * W < (1LL << 31) && 2LL * B * Hc * Wc * 8 < (1LL << 31),
                   "lpips_prep: B * C * H * W must be < 2^31 (input, and the 8-channel output of both images)");
    const int total = (int)(2LL * B * Hc * Wc);
    const int grid = cdiv(total, 256);
    DBSR_CHECK_ARG((long long)grid * 256 >= total && (long long)(grid - 1) * 256 < total,
                   "lpips_prep: grid mapping out of range (%d blocks, %d pixels)", grid, total);
    const LpipsScale sc = {{-.030f, -.088f, -.188f}, {.458f, .448f, .450f}};
    hipLaunchKernelGGL(lpips_prep_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, B, H, W,
                       boundary_ignore, bgr2rgb ? 1 : 0, normalize ? 1 : 0, pred, gt, sc, out, total);
    DBSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int dbsr_maxpool2d(int N, int H, int W, int C, int k, int s, const float* x, int ldx, float* y, int ldy,
                              void* stream) {
    DBSR_CHECK_ARG(x && y, "maxpool2d: null pointer (x, y)");
    DBSR_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0, "maxpool2d: bad sizes");
    DBSR_CHECK_ARG(C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ldx >= C && ldy >= C,
                   "maxpool2d: C = %d, ld = %d / %d (multiples of 4, ld >= C)", C, ldx, ldy);
    DBSR_CHECK_ARG(k >= 1 && k <= 8 && s >= 1 && s <= 8, "maxpool2d: window %d, stride %d (1..8)", k, s);
    DBSR_CHECK_ARG(H >= k && W >= k, "maxpool2d: the %d x %d input is smaller than the %d x %d window", H, W, k, k);
    DBSR_CHECK_ARG((long long)N * H * W * ldx < (1LL << 31), "maxpool2d: N * H * W * ld must be < 2^31");
    const int oh = (H - k) / s + 1, ow = (W - k) / s + 1;
    DBSR_CHECK_ARG((long long)N * oh * ow * ldy < (1LL << 31), "maxpool2d: N * H * W * ld must be < 2^31");
    // floor mode: the last window ends inside the input
    DBSR_CHECK_ARG((oh - 1) * s + k <= H && (ow - 1) * s + k <= W, "maxpool2d: window mapping out of range");
    const int total = (int)((long long)N * oh * ow * (C / 4));
    const int grid = cdiv(total, 256);
    DBSR_CHECK_ARG((long long)grid * 256 >= total && (long long)(grid - 1) * 256 < total,
                   "maxpool2d: grid mapping out of range (%d blocks, %d runs)", grid, total);
    hipLaunchKernelGGL(maxpool_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, H, W, C / 4, k, s, oh,
                       ow, x, ldx, y, ldy, total);
    DBSR_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t dbsr_lpips_layer_workspace_bytes(int B, int h, int w, int C) {
    if (!layer_sizes_ok(B, h, w, C)) return 0;
    return (size_t)B * layer_bpi(h, w) * sizeof(float);
}

extern "C" int dbsr_lpips_layer(int B, int h, int w, int C, int layer, const float* feat, const float* lin, float* map,
                                float* per_layer, float* value, void* workspace, size_t workspace_bytes,
                                void* stream) {
    DBSR_CHECK_ARG(feat && lin && per_layer && value, "lpips_layer: null pointer (feat, lin, per_layer, value)");
    DBSR_CHECK_ARG(B > 0 && h > 0 && w > 0, "lpips_layer: bad sizes");
    DBSR_CHECK_ARG(layer_c_ok(C), "lpips_layer: C = %d (64, 128, 192, 256, 384 or 512 channels)", C);
    DBSR_CHECK_ARG(layer >= 0 && layer < 5, "lpips_layer: layer = %d (0..4)", layer);
    DBSR_CHECK_ARG(2LL * B * h * w * C < (1LL << 31), "lpips_layer: 2 * B * h * w * C must be < 2^31");
    const int hw = h * w, bpi = layer_bpi(h, w);
    const size_t need = (size_t)B * bpi * sizeof(float);
    DBSR_CHECK_ARG(workspace && workspace_bytes >= need, "lpips_layer: workspace %zu < %zu bytes",
                   workspace ? workspace_bytes : (size_t)0, need);
    // the blocks of an image cover its pixels, and the last one starts inside the map
    DBSR_CHECK_ARG((long long)bpi * LP_PIX >= hw && (long long)(bpi - 1) * LP_PIX < hw &&
                       (long long)B * bpi < (1LL << 31),
                   "lpips_layer: block mapping out of range (%d blocks per image, %d pixels)", bpi, hw);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(B * bpi)), block(LP_WAVES * 64);
    if (C <= 256)
        hipLaunchKernelGGL(lpips_layer_kernel<1>, grid, block, 0, s, B, hw, C, bpi, feat, lin, map, (float*)workspace);
    else
        hipLaunchKernelGGL(lpips_layer_kernel<2>, grid, block, 0, s, B, hw, C, bpi, feat, lin, map, (float*)workspace);
    DBSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(lpips_finish_kernel, dim3(1), dim3(256), 0, s, B, bpi, hw, layer, (const float*)workspace,
                       per_layer, value);
    DBSR_LAUNCH_CHECK();
    return 0;
}
