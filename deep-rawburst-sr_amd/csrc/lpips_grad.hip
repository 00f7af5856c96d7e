// The gradient of LPIPS (csrc/lpips.hip) with respect to pred: the per-layer distance's backward, the max-pools'
// backward and the first conv's input gradient fused with the transpose of dbsr_lpips_prep.  The stride-1 convs in
// between run their input gradients through dbsr_conv2d (ops.LPIPSPlan.backward).  fp32, NHWC with ld = C, on the
// caller's stream, no host read, no atomics: every output element has one owner that gathers its terms in a fixed
// order, so two runs are bitwise equal.  Only the pred half (frames 0..B-1) gets a gradient.
//
//   dbsr_lpips_layer_backward   with n(f) = f / (r + eps), r = |f|, D = r + eps, u = f / r and
//                               g_c = 2 gvalue[b] / (h w) lin_c (n(f0)_c - n(f1)_c):
//                                 d value[b] / d f0_j = (g_j - u_j (u . g) r / D) / D.
//                               At f0 = 0 this is the limit g_j / eps (dn/df = I / eps), which is what a float64
//                               finite difference gives; torch autograd returns NaN there (sqrt'(0) = inf times 0).
//                               One wave per pixel pair, the lane's 16-byte channel pieces in registers, as the
//                               forward; the two-pass form (n(f0) - n(f1) from the two norms) because the expanded
//                               one cancels when pred is close to gt.
//   dbsr_maxpool2d_backward     each input element adds dy over the windows whose arg-max it is (recomputed from the
//                               saved input; ties go to the first element in row-major window order, torch's
//                               rule); rows and columns that floor mode drops get zero.
//   dbsr_lpips_stem_backward    dy [B,oh,ow,64] (ReLU-gated) -> gpred [B,3,H,W] NCHW: a direct gather over the live
//                               taps (alex 11 x 11 / 4: at most 3 x 3 of them), then the factor 2 of `normalize`, the
//                               division by the channel's scale, the channel flip back and the un-crop; every
//                               element of gpred is written, zeros in the boundary_ignore frame.
#include "common.hpp"

#include <cmath>

using namespace dbsr;

namespace {

constexpr int LG_WAVES = 4;                       // waves per block of the layer kernel (the forward's mapping)
constexpr int LG_PIX = 32;                        // pixel pairs per block
constexpr float LG_EPS = 1e-10f;
constexpr int ALEX_MIN = 31, VGG_MIN = 16;        // smallest crop side (dbsr_lpips_prep)
constexpr int STEM_COUT = 64;

struct StemScale { float scale[3]; };

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ float dot4(const float4& a, const float4& b, float s) {
    s = fmaf(a.x, b.x, s); s = fmaf(a.y, b.y, s); s = fmaf(a.z, b.z, s); s = fmaf(a.w, b.w, s);
    return s;
}

// ------------------------------------------------------------------------------------------------------ layer
// The forward's mapping: block blk of image b owns pixels [blk * LG_PIX, +LG_PIX) of the h*w map, wave wv takes
// the pixels wv, wv + LG_WAVES, ... of them; a lane holds PIECES 16-byte channel pieces of both images.
template <int PIECES>
__global__ __launch_bounds__(LG_WAVES * 64) void lpips_layer_bwd_kernel(int B, int hw, int C, int bpi,
                                                                        const float* __restrict__ feat,
                                                                        const float* __restrict__ lin,
                                                                        const float* __restrict__ gvalue,
                                                                        float* __restrict__ gfeat, int accumulate) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x / bpi, blk = blockIdx.x - b * bpi;
    const float* F0 = feat + (long long)b * hw * C;
    const float* F1 = feat + (long long)(B + b) * hw * C;
    float* G = gfeat + (long long)b * hw * C;
    const float up = 2.f * (gvalue[b] / (float)hw);            // d value / d (the map's pixel), times the square's 2

    float4 w[PIECES];
    bool on[PIECES];
#pragma unroll
    for (int q = 0; q < PIECES; ++q) {
        const int c = 4 * (lane + 64 * q);
        on[q] = c < C;
        w[q] = on[q] ? *(const float4*)(lin + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }

    constexpr int UN = PIECES == 1 ? 4 : 2;                    // pixels whose loads are in flight together
    static_assert((LG_PIX / LG_WAVES) % UN == 0, "pixel groups");
    for (int j0 = 0; j0 < LG_PIX / LG_WAVES; j0 += UN) {
        if (blk * LG_PIX + j0 * LG_WAVES + wv >= hw) break;    // wave-uniform; later pixels lie further out
        float4 a[UN][PIECES], g[UN][PIECES], old[UN][PIECES];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int p = blk * LG_PIX + (j0 + u) * LG_WAVES + wv;
#pragma unroll
            for (int q = 0; q < PIECES; ++q) {
                const long long o = (long long)p * C + 4 * (lane + 64 * q);
                const bool ld = on[q] && p < hw;
                a[u][q] = ld ? *(const float4*)(F0 + o) : make_float4(0.f, 0.f, 0.f, 0.f);
                g[u][q] = ld ? *(const float4*)(F1 + o) : make_float4(0.f, 0.f, 0.f, 0.f);
                old[u][q] = (ld && accumulate) ? *(const float4*)(G + o) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int p = blk * LG_PIX + (j0 + u) * LG_WAVES + wv;
            if (p < hw) {                                      // wave-uniform
                float s0 = 0.f, s1 = 0.f;
#pragma unroll
                for (int q = 0; q < PIECES; ++q) {
                    s0 = dot4(a[u][q], a[u][q], s0);
                    s1 = dot4(g[u][q], g[u][q], s1);
                }
                const float r0 = sqrtf(wave_sum(s0));
                const float D0 = r0 + LG_EPS, D1 = sqrtf(wave_sum(s1)) + LG_EPS;
                const float inv_r = r0 > 0.f ? 1.f / r0 : 0.f;  // f0 = 0: u = 0, the limit dn/df = I / eps
                float4 un[PIECES];
                float ug = 0.f;
#pragma unroll
                for (int q = 0; q < PIECES; ++q) {
                    float4& gg = g[u][q];                       // f1 -> g, the gradient with respect to n(f0)
                    const float4& f = a[u][q];
                    gg.x = up * w[q].x * (f.x / D0 - gg.x / D1);
                    gg.y = up * w[q].y * (f.y / D0 - gg.y / D1);
                    gg.z = up * w[q].z * (f.z / D0 - gg.z / D1);
                    gg.w = up * w[q].w * (f.w / D0 - gg.w / D1);
                    un[q] = make_float4(f.x * inv_r, f.y * inv_r, f.z * inv_r, f.w * inv_r);
                    ug = dot4(un[q], gg, ug);
                }
                const float k = wave_sum(ug) * (r0 / D0);
#pragma unroll
                for (int q = 0; q < PIECES; ++q) {
                    if (!on[q]) continue;
                    const float4& gg = g[u][q];
                    float4 o;
                    o.x = (gg.x - un[q].x * k) / D0;
                    o.y = (gg.y - un[q].y * k) / D0;
                    o.z = (gg.z - un[q].z * k) / D0;
                    o.w = (gg.w - un[q].w * k) / D0;
                    if (accumulate) {
                        o.x += old[u][q].x; o.y += old[u][q].y; o.z += old[u][q].z; o.w += old[u][q].w;
                    }
                    *(float4*)(G + (long long)p * C + 4 * (lane + 64 * q)) = o;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------- pool
// One thread per (input pixel, 4 channels): it walks the windows that hold its pixel in (oy, ox) order, finds each
// window's arg-max as the forward's scan does (first maximum in row-major order; a NaN takes it, as in torch) and
// adds that window's dy where the arg-max is its own element.
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(int H, int W, int C4, int k, int s, int oh, int ow,
                                                          const float* __restrict__ x, const float* __restrict__ dy,
                                                          float* __restrict__ dx, int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int C = 4 * C4;
    const int c4 = i % C4;
    int t = i / C4;
    const int ix = t % W;
    t /= W;
    const int iy = t % H;
    const int n = t / H;
    const int oy_lo = iy - k + 1 <= 0 ? 0 : (iy - k + s) / s, oy_hi = min(iy / s, oh - 1);
    const int ox_lo = ix - k + 1 <= 0 ? 0 : (ix - k + s) / s, ox_hi = min(ix / s, ow - 1);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int oy = oy_lo; oy <= oy_hi; ++oy)
        for (int ox = ox_lo; ox <= ox_hi; ++ox) {
            const float* src = x + (((long long)n * H + (long long)oy * s) * W + (long long)ox * s) * C + 4 * c4;
            float4 m = *(const float4*)src;
            int ax = 0, ay = 0, az = 0, aw = 0;
            for (int wy = 0; wy < k; ++wy)
                for (int wx = 0; wx < k; ++wx) {
                    const float4 v = *(const float4*)(src + ((long long)wy * W + wx) * C);
                    const int e = wy * k + wx;
                    if (v.x > m.x || v.x != v.x) { m.x = v.x; ax = e; }
                    if (v.y > m.y || v.y != v.y) { m.y = v.y; ay = e; }
                    if (v.z > m.z || v.z != v.z) { m.z = v.z; az = e; }
                    if (v.w > m.w || v.w != v.w) { m.w = v.w; aw = e; }
                }
            const int mine = (iy - oy * s) * k + (ix - ox * s);
            const float4 g = *(const float4*)(dy + (((long long)n * oh + oy) * ow + ox) * C + 4 * c4);
            acc.x += ax == mine ? g.x : 0.f;
            acc.y += ay == mine ? g.y : 0.f;
            acc.z += az == mine ? g.z : 0.f;
            acc.w += aw == mine ? g.w : 0.f;
        }
    *(float4*)(dx + (((long long)n * H + iy) * W + ix) * C + 4 * c4) = acc;
}

// ------------------------------------------------------------------------------------------------------- stem
// One thread per pixel of the whole [B, H, W] image.  Inside the crop it gathers, for the three input channels,
// sum over live taps (ky, kx) and the 64 couts of dy[oy, ox, co] w[co][c][ky][kx], oy = (y + P - ky) / S exact and
// in range.  A tap's 64 products run as four chains of 16 (one per component of the 16-byte pieces) that are then
// added pairwise, and the taps are added in (oy, ox) order.
template <int K, int S, int P>
__global__ __launch_bounds__(256) void lpips_stem_bwd_kernel(int H, int W, int bi, int flip, float mul, StemScale sc,
                                                             int oh, int ow, const float* __restrict__ dy,
                                                             const float* __restrict__ w, float* __restrict__ gpred,
                                                             int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int X = i % W;
    const int t = i / W;
    const int Y = t % H;
    const int b = t / H;
    const int y = Y - bi, x = X - bi;
    float g[3] = {0.f, 0.f, 0.f};
    if (y >= 0 && y < H - 2 * bi && x >= 0 && x < W - 2 * bi) {
        const int oy_lo = y + P - K + 1 <= 0 ? 0 : (y + P - K + S) / S, oy_hi = min((y + P) / S, oh - 1);
        const int ox_lo = x + P - K + 1 <= 0 ? 0 : (x + P - K + S) / S, ox_hi = min((x + P) / S, ow - 1);
        for (int oy = oy_lo; oy <= oy_hi; ++oy)
            for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                const int ky = y + P - S * oy, kx = x + P - S * ox;          // in [0, K)
                const float4* d = (const float4*)(dy + (((long long)b * oh + oy) * ow + ox) * STEM_COUT);
                const float* wk = w + ky * K + kx;
                float4 a[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) a[c] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int q = 0; q < STEM_COUT / 4; ++q) {
                    const float4 v = d[q];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        a[c].x = fmaf(v.x, wk[((4 * q + 0) * 3 + c) * K * K], a[c].x);
                        a[c].y = fmaf(v.y, wk[((4 * q + 1) * 3 + c) * K * K], a[c].y);
                        a[c].z = fmaf(v.z, wk[((4 * q + 2) * 3 + c) * K * K], a[c].z);
                        a[c].w = fmaf(v.w, wk[((4 * q + 3) * 3 + c) * K * K], a[c].w);
                    }
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) g[c] += (a[c].x + a[c].y) + (a[c].z + a[c].w);
            }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
        gpred[(((long long)b * 3 + (flip ? 2 - c : c)) * H + Y) * W + X] = (mul * g[c]) / sc.scale[c];
}

inline bool layer_c_ok(int C) { return C == 64 || C == 128 || C == 192 || C == 256 || C == 384 || C == 512; }

}  // namespace

extern "C" int dbsr_lpips_layer_backward(int B, int h, int w, int C, const float* feat, const float* lin,
                                         const float* gvalue, float* gfeat, int accumulate, void* stream) {
    DBSR_CHECK_ARG(feat && lin && gvalue && gfeat, "lpips_layer_backward: null pointer (feat, lin, gvalue, gfeat)");
    DBSR_CHECK_ARG(B > 0 && h > 0 && w > 0, "lpips_layer_backward: bad sizes");
    DBSR_CHECK_ARG(layer_c_ok(C), "lpips_layer_backward: C = %d (64, 128, 192, 256, 384 or 512 channels)", C);
    DBSR_CHECK_ARG(2LL * B * h * w * C < (1LL << 31), "lpips_layer_backward: 2 * B * h * w * C must be < 2^31");
    const int hw = h * w, bpi = cdiv(hw, LG_PIX);
    // the blocks of an image cover its pixels, and the last one starts inside the map
    DBSR_CHECK_ARG((long long)bpi * LG_PIX >= hw && (long long)(bpi - 1) * LG_PIX < hw && (long long)B * bpi < (1LL << 31),
                   "lpips_layer_backward: block mapping out of range (%d blocks per image, %d pixels)", bpi, hw);
    const dim3 grid((unsigned)(B * bpi)), block(LG_WAVES * 64);
    if (C <= 256)
        hipLaunchKernelGGL(lpips_layer_bwd_kernel<1>, grid, block, 0, (hipStream_t)stream, B, hw, C, bpi, feat, lin,
                           gvalue, gfeat, accumulate ? 1 : 0);
    else
        hipLaunchKernelGGL(lpips_layer_bwd_kernel<2>, grid, block, 0, (hipStream_t)stream, B, hw, C, bpi, feat, lin,
                           gvalue, gfeat, accumulate ? 1 : 0);
    DBSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int dbsr_maxpool2d_backward(int N, int H, int W, int C, int k, int s, const float* x, const float* dy,
                                       float* dx, void* stream) {
    DBSR_CHECK_ARG(x && dy && dx, "maxpool2d_backward: null pointer (x, dy, dx)");
    DBSR_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0, "maxpool2d_backward: bad sizes");
    DBSR_CHECK_ARG(C % 4 == 0, "maxpool2d_backward: C = %d (a multiple of 4)", C);
    DBSR_CHECK_ARG((k == 3 || k == 2) && s == 2, "maxpool2d_backward: window %d, stride %d (3 / 2 or 2 / 2)", k, s);
    DBSR_CHECK_ARG(H >= k && W >= k, "maxpool2d_backward: the %d x %d input is smaller than the %d x %d window", H, W,
                   k, k);
    DBSR_CHECK_ARG((long long)N * H * W * C < (1LL << 31), "maxpool2d_backward: N * H * W * C must be < 2^31");
    const int oh = (H - k) / s + 1, ow = (W - k) / s + 1;
    // floor mode: the last window ends inside the input
    DBSR_CHECK_ARG((oh - 1) * s + k <= H && (ow - 1) * s + k <= W, "maxpool2d_backward: window mapping out of range");
    const int total = (int)((long long)N * H * W * (C / 4));
    const int grid = cdiv(total, 256);
    DBSR_CHECK_ARG((long long)grid * 256 >= total && (long long)(grid - 1) * 256 < total,
                   "maxpool2d_backward: grid mapping out of range (%d blocks, %d runs)", grid, total);
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, H, W, C / 4, k, s,
                       oh, ow, x, dy, dx, total);
    DBSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int dbsr_lpips_stem_backward(int B, int H, int W, int boundary_ignore, int net, int bgr2rgb, int normalize,
                                        const float* dy, const float* w, float* gpred, void* stream) {
    DBSR_CHECK_ARG(dy && w && gpred, "lpips_stem_backward: null pointer (dy, w, gpred)");
    DBSR_CHECK_ARG(B > 0 && H > 0 && W > 0, "lpips_stem_backward: bad sizes");
    DBSR_CHECK_ARG(net == DBSR_LPIPS_ALEX || net == DBSR_LPIPS_VGG,
                   "lpips_stem_backward: net must be 0 (alex) or 1 (vgg)");
    DBSR_CHECK_ARG(boundary_ignore >= 0 && boundary_ignore < (1 << 28),
                   "lpips_stem_backward: boundary_ignore must be >= 0");
    const long long Hc = (long long)H - 2LL * boundary_ignore, Wc = (long long)W - 2LL * boundary_ignore;
    const int need = net == DBSR_LPIPS_ALEX ? ALEX_MIN : VGG_MIN;
    DBSR_CHECK_ARG(Hc >= need && Wc >= need, "lpips_stem_backward: the crop %lld x %lld is smaller than %d x %d (%s)",
                   Hc, Wc, need, need, net == DBSR_LPIPS_ALEX ? "alex" : "vgg");
    DBSR_CHECK_ARG((long long)B * 3 * H * W < (1LL << 31), "lpips_stem_backward: B * C * H * W must be < 2^31");
    const int k = net == DBSR_LPIPS_ALEX ? 11 : 3, s = net == DBSR_LPIPS_ALEX ? 4 : 1, p = net == DBSR_LPIPS_ALEX ? 2 : 1;
    const int oh = (int)((Hc + 2 * p - k) / s + 1), ow = (int)((Wc + 2 * p - k) / s + 1);
    DBSR_CHECK_ARG((long long)B * oh * ow * STEM_COUT < (1LL << 31),
                   "lpips_stem_backward: B * oh * ow * 64 must be < 2^31");
    const int total = (int)((long long)B * H * W);
    const int grid = cdiv(total, 256);
    DBSR_CHECK_ARG((long long)grid * 256 >= total && (long long)(grid - 1) * 256 < total,
                   "lpips_stem_backward: grid mapping out of range (%d blocks, %d pixels)", grid, total);
    const StemScale sc = {{.458f, .448f, .450f}};
    const float mul = normalize ? 2.f : 1.f;
    if (net == DBSR_LPIPS_ALEX)
        hipLaunchKernelGGL((lpips_stem_bwd_kernel<11, 4, 2>), dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream,
                           H, W, boundary_ignore, bgr2rgb ? 1 : 0, mul, sc, oh, ow, dy, w, gpred, total);
    else
        hipLaunchKernelGGL((lpips_stem_bwd_kernel<3, 1, 1>), dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, H,
                           W, boundary_ignore, bgr2rgb ? 1 : 0, mul, sc, oh, ow, dy, w, gpred, total);
    DBSR_LAUNCH_CHECK();
    return 0;
}
