// Image-quality metrics: SSIM as the reference scores it (models/loss/msssim.py:22-74 through
// image_quality_v2.py:104-136) and its gradient w.r.t. the prediction.  fp32 NCHW planes.
//
// Per channel plane, over the boundary crop, with the 11-tap Gaussian window w (sigma 1.5, "valid" convolution):
//   mu1 = w*p, mu2 = w*g, s11 = w*p^2 - mu1^2, s22 = w*g^2 - mu2^2, s12 = w*pg - mu1 mu2
//   A1 = 2 mu1 mu2 + C1, A2 = 2 s12 + C2, B1 = mu1^2 + mu2^2 + C1, B2 = s11 + s22 + C2, S = A1 A2 / (B1 B2)
// and the masked mean of S.  The window is an outer product, so both kernels filter rows, then columns, of a
// tile staged in LDS (plain loads and LDS stores; fp32 VALU work, no MFMA shape in it).
//
// Second moments are taken around a per-tile constant m (a ground-truth pixel of the tile): w*p^2 - mu1^2
// cancels to ~1e-7 absolute in fp32, which is 1e-4 of C2 = 9e-4 on smooth [0,1] images, and the same sums of
// (p - m), (g - m) do not.  The taps sum to 1 + delta, not 1, so the centred moments differ from the reference's
// by delta * m * (mu1 + mu2 - m (1 + delta)); that term is added back (delta ~ 1e-7, computed on the host).
//
// Backward (no saved maps): with v the window mask,
//   dS/dp(q) = sum over the windows i that contain q of w(q - i) v_i (Sa_i + 2 p(q) Sb_i + g(q) Sc_i)
//   Sa = 2 mu2 (A2 - A1) / (B1 B2) + 2 mu1 S (1/B2 - 1/B1),  Sb = -S / B2,  Sc = 2 A1 / (B1 B2)
// i.e. three maps pushed through the window's transpose (a full correlation, separable too).  Each block owns a
// tile of input pixels, recomputes the three maps on the tile plus a 10-pixel halo from inputs on a 20-pixel
// halo, and gathers: no atomics, every output written once, bitwise reproducible.  The maps are kept in the
// centred form Sa + m (2 Sb + Sc), Sb, Sc and combined with p - m, g - m, so that the three terms (each ~1/C2)
// do not cancel against each other more than they must.
#include "common.hpp"

#include <cmath>

using namespace dbsr;

namespace {

constexpr int KW = 11, HALO = KW - 1;

struct SsimWin {
    float w[KW];
    float delta;                    // (sum of the 2-D window's float taps) - 1
};

// msssim.gaussian(11, 1.5): exp in double, stored as float, divided by their float sum
SsimWin make_window() {
    SsimWin win;
    float g[KW];
    double s = 0.0;
    for (int x = 0; x < KW; ++x) {
        g[x] = (float)std::exp(-(double)((x - KW / 2) * (x - KW / 2)) / (2.0 * 1.5 * 1.5));
        s += (double)g[x];
    }
    const float fs = (float)s;
    for (int x = 0; x < KW; ++x) win.w[x] = g[x] / fs;
    double s2 = 0.0;                                            // create_window: the float outer product
    for (int y = 0; y < KW; ++y)
        for (int x = 0; x < KW; ++x) s2 += (double)(win.w[y] * win.w[x]);
    win.delta = (float)(s2 - 1.0);
    return win;
}

struct SsimTerms { float S, Sa, Sb, Sc; };

// the five centred window moments -> S and the three gradient maps (Sa in its centred form, see the header)
template <bool GRAD>
__device__ __forceinline__ SsimTerms ssim_terms(float m1c, float m2c, float e11, float e22, float e12, float m,
                                                float delta, float C1, float C2) {
    const float wsum = 1.f + delta;
    const float mu1 = m1c + m * wsum, mu2 = m2c + m * wsum;
    const float dm = delta * m, mw = m * wsum;
    const float s11 = (e11 - m1c * m1c) - dm * (2.f * mu1 - mw);
    const float s22 = (e22 - m2c * m2c) - dm * (2.f * mu2 - mw);
    const float s12 = (e12 - m1c * m2c) - dm * (mu1 + mu2 - mw);
    const float A1 = 2.f * mu1 * mu2 + C1, A2 = 2.f * s12 + C2;
    const float B1 = mu1 * mu1 + mu2 * mu2 + C1, B2 = s11 + s22 + C2;
    const float r1 = 1.f / B1, r2 = 1.f / B2;
    SsimTerms t;
    t.S = (A1 * A2) * (r1 * r2);
    if (GRAD) {
        const float sa = 2.f * mu2 * (A2 - A1) * (r1 * r2) + 2.f * mu1 * t.S * (r2 - r1);
        t.Sb = -t.S * r2;
        t.Sc = 2.f * A1 * (r1 * r2);
        t.Sa = sa + m * (2.f * t.Sb + t.Sc);
    }
    return t;
}

// sum over the block's 256 threads in a fixed order; the result is valid in thread 0.  red: 256 floats
__device__ __forceinline__ float block_sum256(float v, float* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    return red[0];
}

// the tile's centring constant: the ground-truth pixel nearest the tile's centre, inside the crop
__device__ __forceinline__ float tile_const(const float* G, int W, int bi, int Hc, int Wc, int cy, int cx) {
    cy = min(max(cy, 0), Hc - 1);
    cx = min(max(cx, 0), Wc - 1);
    return G[(long long)(bi + cy) * W + bi + cx];
}

// ---------------------------------------------------------------------------------------------------- forward
constexpr int FT = 32;                                   // map tile (FT x FT windows per block)
constexpr int F_IN = FT + HALO, F_IP = F_IN + 1;         // input tile side, its padded row pitch
constexpr int F_HP = FT + 1;                             // row-filtered moments: F_IN rows of FT, padded pitch

// One block per (image, channel, map tile): partial[blk] = {sum valid S, sum valid} over the tile.
__global__ __launch_bounds__(256) void ssim_fwd_kernel(int C, int H, int W, int bi, int tiles_y, int tiles_x,
                                                       const float* __restrict__ pred, const float* __restrict__ gt,
                                                       const unsigned char* __restrict__ valid, SsimWin win, float C1,
                                                       float C2, float* __restrict__ map, float* __restrict__ partial) {
    __shared__ float sp[F_IN * F_IP], sg[F_IN * F_IP];
    __shared__ float hb[5][F_IN * F_HP];
    __shared__ float red[256];
    const int tid = threadIdx.x;
    int blk = blockIdx.x;
    const int tx = blk % tiles_x;
    blk /= tiles_x;
    const int ty = blk % tiles_y;
    const int bc = blk / tiles_y;                         // b * C + c
    const int b = bc / C;
    const int Hc = H - 2 * bi, Wc = W - 2 * bi, Hm = Hc - HALO, Wm = Wc - HALO;
    const int y0 = ty * FT, x0 = tx * FT;                 // the tile's origin in map (= crop) coordinates
    const float* P = pred + (long long)bc * H * W;
    const float* G = gt + (long long)bc * H * W;
    const float m = tile_const(G, W, bi, Hc, Wc, y0 + F_IN / 2, x0 + F_IN / 2);

    for (int i = tid; i < F_IN * F_IN; i += 256) {
        const int r = i / F_IN, x = i - r * F_IN;
        const int yy = y0 + r, xx = x0 + x;
        float p = 0.f, g = 0.f;
        if (yy < Hc && xx < Wc) {
            const long long o = (long long)(bi + yy) * W + bi + xx;
            p = P[o] - m;
            g = G[o] - m;
        }
        sp[r * F_IP + x] = p;
        sg[r * F_IP + x] = g;
    }
    __syncthreads();
    for (int i = tid; i < F_IN * FT; i += 256) {
        const int r = i / FT, x = i - r * FT;
        float a1 = 0.f, a2 = 0.f, a11 = 0.f, a22 = 0.f, a12 = 0.f;
#pragma unroll
        for (int j = 0; j < KW; ++j) {
            const float p = sp[r * F_IP + x + j], g = sg[r * F_IP + x + j];
            const float wp = win.w[j] * p, wg = win.w[j] * g;
            a1 += wp;
            a2 += wg;
            a11 = fmaf(wp, p, a11);
            a22 = fmaf(wg, g, a22);
            a12 = fmaf(wp, g, a12);
        }
        hb[0][r * F_HP + x] = a1;
        hb[1][r * F_HP + x] = a2;
        hb[2][r * F_HP + x] = a11;
        hb[3][r * F_HP + x] = a22;
        hb[4][r * F_HP + x] = a12;
    }
    __syncthreads();
    float acc = 0.f, cnt = 0.f;
    for (int i = tid; i < FT * FT; i += 256) {
        const int r = i / FT, x = i - r * FT;
        float a[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < KW; ++j) {
#pragma unroll
            for (int k = 0; k < 5; ++k) a[k] = fmaf(win.w[j], hb[k][(r + j) * F_HP + x], a[k]);
        }
        const int my = y0 + r, mx = x0 + x;
        if (my < Hm && mx < Wm) {
            const SsimTerms t = ssim_terms<false>(a[0], a[1], a[2], a[3], a[4], m, win.delta, C1, C2);
            if (map) map[((long long)bc * Hm + my) * Wm + mx] = t.S;
            if (!valid || valid[((long long)b * H + bi + HALO / 2 + my) * W + bi + HALO / 2 + mx]) {
                acc += t.S;
                cnt += 1.f;
            }
        }
    }
    const float s = block_sum256(acc, red);
    if (tid == 0) partial[2 * (long long)blockIdx.x] = s;
    const float n = block_sum256(cnt, red);
    if (tid == 0) partial[2 * (long long)blockIdx.x + 1] = n;
}

// One block: sums[b] = {sum over image b's C * tiles partials, the count of its first channel}, then result.
// Partials are added in double in a fixed order (strided per thread, then a tree).
__global__ __launch_bounds__(256) void ssim_finish_kernel(int B, int C, int tiles, const float* __restrict__ partial,
                                                          float* __restrict__ sums, float* __restrict__ result) {
    __shared__ double rs[256], rn[256];
    double tot_s = 0.0, tot_n = 0.0;
    for (int b = 0; b < B; ++b) {
        const float* pb = partial + 2 * (long long)b * C * tiles;
        double s = 0.0, n = 0.0;
        for (int i = threadIdx.x; i < C * tiles; i += 256) {
            s += (double)pb[2 * i];
            if (i < tiles) n += (double)pb[2 * i + 1];
        }
        __syncthreads();
        rs[threadIdx.x] = s;
        rn[threadIdx.x] = n;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if ((int)threadIdx.x < st) {
                rs[threadIdx.x] += rs[threadIdx.x + st];
                rn[threadIdx.x] += rn[threadIdx.x + st];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            sums[2 * b] = (float)rs[0];
            sums[2 * b + 1] = (float)rn[0];
            tot_s += rs[0];
            tot_n += rn[0];
        }
    }
    if (threadIdx.x == 0) {
        const double den = (double)C * tot_n + 1e-12;
        result[0] = (float)(tot_s / den);
        result[1] = (float)(1.0 / den);
    }
}

// --------------------------------------------------------------------------------------------------- backward
constexpr int BH = 16, BW = 32;                          // input pixels owned by a block
constexpr int B_MH = BH + HALO, B_MW = BW + HALO;        // windows that touch them
constexpr int B_IH = BH + 2 * HALO, B_IW = BW + 2 * HALO, B_IP = B_IW + 1;   // inputs those windows read
constexpr int B_HP = B_MW + 1;                           // row-filtered moments: B_IH rows of B_MW
constexpr int B_TP = BW + 1;                             // row-filtered gradient maps: B_MH rows of BW
// LDS regions: [0, IN) inputs (2 planes), later the 3 gradient maps; [IN, IN + HB) the 5 row-filtered moments,
// later the 3 row-filtered gradient maps
constexpr int B_IN_FLOATS = 2 * B_IH * B_IP, B_HB_FLOATS = 5 * B_IH * B_HP;
static_assert(3 * B_MH * B_HP <= B_IN_FLOATS, "gradient maps must fit the input region");
static_assert(3 * B_MH * B_TP <= B_HB_FLOATS, "row-filtered gradient maps must fit the moment region");
static_assert((B_IN_FLOATS + B_HB_FLOATS) * sizeof(float) <= 64 * 1024, "LDS budget");

// One block per (image, channel, BH x BW tile of the whole H x W plane); gpred is written for every pixel.
__global__ __launch_bounds__(256) void ssim_bwd_kernel(int C, int H, int W, int bi, int tiles_y, int tiles_x,
                                                       const float* __restrict__ pred, const float* __restrict__ gt,
                                                       const unsigned char* __restrict__ valid, SsimWin win, float C1,
                                                       float C2, const float* __restrict__ scale_p,
                                                       float* __restrict__ gpred) {
    __shared__ float lds[B_IN_FLOATS + B_HB_FLOATS];
    float* sp = lds;
    float* sg = lds + B_IH * B_IP;
    float* hb = lds + B_IN_FLOATS;                       // hb[k][r][x] at k * B_IH * B_HP + r * B_HP + x
    float* sm = lds;                                     // sm[k][r][x] at k * B_MH * B_HP + r * B_HP + x
    float* tb = lds + B_IN_FLOATS;                       // tb[k][r][x] at k * B_MH * B_TP + r * B_TP + x
    const int tid = threadIdx.x;
    int blk = blockIdx.x;
    const int tx = blk % tiles_x;
    blk /= tiles_x;
    const int ty = blk % tiles_y;
    const int bc = blk / tiles_y;
    const int b = bc / C;
    const int Hc = H - 2 * bi, Wc = W - 2 * bi, Hm = Hc - HALO, Wm = Wc - HALO;
    const int cy0 = ty * BH - bi, cx0 = tx * BW - bi;     // the tile's origin in crop coordinates
    const float* P = pred + (long long)bc * H * W;
    const float* G = gt + (long long)bc * H * W;
    float* O = gpred + (long long)bc * H * W;

    if (cy0 + BH <= 0 || cy0 >= Hc || cx0 + BW <= 0 || cx0 >= Wc) {       // wholly outside the crop
        for (int i = tid; i < BH * BW; i += 256) {
            const int y = ty * BH + i / BW, x = tx * BW + i % BW;
            if (y < H && x < W) O[(long long)y * W + x] = 0.f;
        }
        return;
    }
    const float m = tile_const(G, W, bi, Hc, Wc, cy0 + BH / 2, cx0 + BW / 2);

    for (int i = tid; i < B_IH * B_IW; i += 256) {
        const int r = i / B_IW, x = i - r * B_IW;
        const int yy = cy0 - HALO + r, xx = cx0 - HALO + x;
        float p = 0.f, g = 0.f;
        if (yy >= 0 && yy < Hc && xx >= 0 && xx < Wc) {
            const long long o = (long long)(bi + yy) * W + bi + xx;
            p = P[o] - m;
            g = G[o] - m;
        }
        sp[r * B_IP + x] = p;
        sg[r * B_IP + x] = g;
    }
    __syncthreads();
    for (int i = tid; i < B_IH * B_MW; i += 256) {
        const int r = i / B_MW, x = i - r * B_MW;
        float a1 = 0.f, a2 = 0.f, a11 = 0.f, a22 = 0.f, a12 = 0.f;
#pragma unroll
        for (int j = 0; j < KW; ++j) {
            const float p = sp[r * B_IP + x + j], g = sg[r * B_IP + x + j];
            const float wp = win.w[j] * p, wg = win.w[j] * g;
            a1 += wp;
            a2 += wg;
            a11 = fmaf(wp, p, a11);
            a22 = fmaf(wg, g, a22);
            a12 = fmaf(wp, g, a12);
        }
        const int o = r * B_HP + x;
        hb[o] = a1;
        hb[B_IH * B_HP + o] = a2;
        hb[2 * B_IH * B_HP + o] = a11;
        hb[3 * B_IH * B_HP + o] = a22;
        hb[4 * B_IH * B_HP + o] = a12;
    }
    __syncthreads();                                     // the inputs are dead from here: sm takes their place
    for (int i = tid; i < B_MH * B_MW; i += 256) {
        const int r = i / B_MW, x = i - r * B_MW;
        const int wy = cy0 - HALO + r, wx = cx0 - HALO + x;               // the window's origin (map coordinates)
        float sa = 0.f, sb = 0.f, sc = 0.f;
        if (wy >= 0 && wy < Hm && wx >= 0 && wx < Wm &&
            (!valid || valid[((long long)b * H + bi + HALO / 2 + wy) * W + bi + HALO / 2 + wx])) {
            float a[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < KW; ++j) {
#pragma unroll
                for (int k = 0; k < 5; ++k) a[k] = fmaf(win.w[j], hb[k * B_IH * B_HP + (r + j) * B_HP + x], a[k]);
            }
            const SsimTerms t = ssim_terms<true>(a[0], a[1], a[2], a[3], a[4], m, win.delta, C1, C2);
            sa = t.Sa;
            sb = t.Sb;
            sc = t.Sc;
        }
        const int o = r * B_HP + x;
        sm[o] = sa;
        sm[B_MH * B_HP + o] = sb;
        sm[2 * B_MH * B_HP + o] = sc;
    }
    __syncthreads();                                     // the moments are dead from here: tb takes their place
    // the window's transpose: pixel r gathers from the windows r + j (local index), j = 0..10, with tap 10 - j
    for (int i = tid; i < B_MH * BW; i += 256) {
        const int r = i / BW, x = i - r * BW;
        float a[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < KW; ++j) {
#pragma unroll
            for (int k = 0; k < 3; ++k) a[k] = fmaf(win.w[KW - 1 - j], sm[k * B_MH * B_HP + r * B_HP + x + j], a[k]);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) tb[k * B_MH * B_TP + r * B_TP + x] = a[k];
    }
    __syncthreads();
    const float scale = *scale_p;
    for (int i = tid; i < BH * BW; i += 256) {
        const int r = i / BW, x = i - r * BW;
        const int y = ty * BH + r, xg = tx * BW + x;
        if (y >= H || xg >= W) continue;
        float out = 0.f;
        const int cy = cy0 + r, cx = cx0 + x;
        if (cy >= 0 && cy < Hc && cx >= 0 && cx < Wc) {
            float a[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < KW; ++j) {
#pragma unroll
                for (int k = 0; k < 3; ++k) a[k] = fmaf(win.w[KW - 1 - j], tb[k * B_MH * B_TP + (r + j) * B_TP + x], a[k]);
            }
            const long long o = (long long)y * W + xg;
            const float p = P[o] - m, g = G[o] - m;
            out = scale * (a[0] + 2.f * p * a[1] + g * a[2]);
        }
        O[(long long)y * W + xg] = out;
    }
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
// (k L)^2 as the reference forms it: in double, rounded once when it meets the fp32 maps
inline float ssim_const(double k, float val_range) { return (float)((k * (double)val_range) * (k * (double)val_range)); }
inline size_t ssim_fwd_bytes(int B, int C, int H, int W, int bi) {
    const int Hm = H - 2 * bi - HALO, Wm = W - 2 * bi - HALO;
    return (size_t)B * C * cdiv(Hm, FT) * cdiv(Wm, FT) * 2 * sizeof(float);
}
inline bool ssim_sizes_ok(int B, int C, int H, int W, int bi) {
    return B > 0 && C >= 1 && C <= 4 && H > 0 && W > 0 && bi >= 0 && bi < (1 << 28) &&
           (long long)H - 2LL * bi >= KW && (long long)W - 2LL * bi >= KW && (long long)B * C * H * W < (1LL << 31);
}

}  // namespace

extern "C" size_t dbsr_ssim_workspace_bytes(int B, int C, int H, int W, int boundary_ignore) {
    if (!ssim_sizes_ok(B, C, H, W, boundary_ignore)) return 0;
    return ssim_fwd_bytes(B, C, H, W, boundary_ignore);
}

#define SSIM_CHECK_SIZES(name)                                                                                      \
    DBSR_CHECK_ARG(B > 0 && H > 0 && W > 0, name ": bad sizes");                                                    \
    DBSR_CHECK_ARG(C >= 1 && C <= 4, name ": C = %d (1..4 channels)", C);                                          \
    DBSR_CHECK_ARG(boundary_ignore >= 0 && boundary_ignore < (1 << 28), name ": boundary_ignore must be >= 0");    \
    DBSR_CHECK_ARG((long long)H - 2LL * boundary_ignore >= KW && (long long)W - 2LL * boundary_ignore >= KW,       \
                   name ": the crop %lld x %lld is smaller than the 11 x 11 window",                               \
                   (long long)H - 2LL * boundary_ignore, (long long)W - 2LL * boundary_ignore);                    \
    DBSR_CHECK_ARG((long long)B * C * H * W < (1LL << 31), name ": B * C * H * W must be < 2^31");                  \
    DBSR_CHECK_ARG(val_range > 0.f, name ": val_range must be > 0")

extern "C" int dbsr_ssim_forward(int B, int C, int H, int W, int boundary_ignore, const float* pred, const float* gt,
                                 const unsigned char* valid, float val_range, float* map, float* sums, float* result,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    DBSR_CHECK_ARG(pred && gt && sums && result, "ssim_forward: null pointer (pred, gt, sums, result)");
    SSIM_CHECK_SIZES("ssim_forward");
    const size_t need = ssim_fwd_bytes(B, C, H, W, boundary_ignore);
    DBSR_CHECK_ARG(workspace && workspace_bytes >= need, "ssim_forward: workspace %zu < %zu bytes",
                   workspace ? workspace_bytes : (size_t)0, need);
    const int bi = boundary_ignore;
    const int ty = cdiv(H - 2 * bi - HALO, FT), tx = cdiv(W - 2 * bi - HALO, FT);
    const SsimWin win = make_window();
    const float C1 = ssim_const(0.01, val_range), C2 = ssim_const(0.03, val_range);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ssim_fwd_kernel, dim3((unsigned)(B * C * ty * tx)), dim3(256), 0, s, C, H, W, bi, ty, tx, pred,
                       gt, valid, win, C1, C2, map, (float*)workspace);
    DBSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(ssim_finish_kernel, dim3(1), dim3(256), 0, s, B, C, ty * tx, (const float*)workspace, sums,
                       result);
    DBSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int dbsr_ssim_backward(int B, int C, int H, int W, int boundary_ignore, const float* pred, const float* gt,
                                  const unsigned char* valid, float val_range, const float* scale, float* gpred,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace;
    (void)workspace_bytes;
    DBSR_CHECK_ARG(pred && gt && scale && gpred, "ssim_backward: null pointer (pred, gt, scale, gpred)");
    SSIM_CHECK_SIZES("ssim_backward");
    const int bi = boundary_ignore;
    const int ty = cdiv(H, BH), tx = cdiv(W, BW);
    const SsimWin win = make_window();
    const float C1 = ssim_const(0.01, val_range), C2 = ssim_const(0.03, val_range);
    hipLaunchKernelGGL(ssim_bwd_kernel, dim3((unsigned)(B * C * ty * tx)), dim3(256), 0, (hipStream_t)stream, C, H, W,
                       bi, ty, tx, pred, gt, valid, win, C1, C2, scale, gpred);
    DBSR_LAUNCH_CHECK();
    return 0;
}
