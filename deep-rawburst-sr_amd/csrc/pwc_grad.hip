// Gradients for training PWC-Net (models/alignment/pwcnet.py:41-281 under autograd): what the convolutions of the
// alignment network need beyond the stride-1 3x3 kernels of train_ops.hip, and the transpose of the flow's
// final resize.
//
//   dbsr_conv_wgrad_sd            weight (+ bias) gradient of a k in {1, 3, 4} conv with stride 1 | 2, any dilation
//                                 and pad -- the extractor's stride-2 convs, the refiner's dilated convs, and (roles
//                                 swapped: "input" = dy, "output gradient" = x) ConvTranspose2d(k4, s2, p1)
//   dbsr_conv_dgrad_sd            input gradient of the same family as a gather, one GEMM per output parity class
//   dbsr_dgrad_sd_pack            its weights, [tap][ci][co] in the compute dtype
//   dbsr_act_backward             dpre = dy * act'(y) for ReLU / LeakyReLU(0.1)
//   dbsr_flow_finalize_backward   d(dbsr_flow_finalize's offsets)/d(flow)
//
// wgrad_sd is an implicit GEMM whose reduction axis is the output pixel (all frames in one axis): a block owns a
// 64 co x 64 ci slice of one tap and a contiguous range of 32-pixel steps; per step it stages dy [32 px][64 co] and
// the tap's strided / dilated x pixels [32 px][64 ci] in LDS from registers (zeros outside the image and past the
// channel counts; the next step's loads are in flight during this step's MFMAs), and its four waves take a 32 x 32
// quadrant each.  16-bit operands are read with the transposed LDS read as conv_wgrad_kernel does (train_ops.hip);
// fp32 runs the true-fp32 16x16x4 MFMA.  Every block stores its fp32 partial; wgrad_sd_reduce adds the blocks of a
// pixel split in block order, so two runs are bitwise equal.  The bias gradient is dbsr_chan_sum over dy.
//
// dgrad_sd: dx[iy, ix] collects dy[(iy + pad - ky d) / s, (ix + pad - kx d) / s] over the taps for which both
// divisions are exact, which depends only on (iy mod s, ix mod s).  A wave owns 16 input pixels of ONE such class and
// loops over that class's live taps only (1, 2, 2 and 4 of the 9 for k3 s2 p1), so no MFMA multiplies a structural
// zero.  Both MFMA operands are one 16-B global load per lane (dy rows are K-contiguous in NHWC, the packed weights
// are [ci][co]); there is no LDS and no barrier.
#include <algorithm>
#include <type_traits>
#include "common.hpp"

using namespace dbsr;

extern "C" size_t dbsr_chan_sum_workspace_bytes(int n, int hw, int c);
extern "C" int dbsr_chan_sum(int n, int hw, int c, dbsr_tensor t, float* out, int accumulate, void* workspace,
                             size_t workspace_bytes, void* stream);

namespace {

inline unsigned nblocks(long long total, int bs) { return (unsigned)((total + bs - 1) / bs); }
inline int rup(int v, int m) { return (v + m - 1) / m * m; }
inline size_t rup256(size_t v) { return (v + 255) / 256 * 256; }

template <typename F>
int by_dtype(int dtype, F&& f) {
    if (dtype == DBSR_BF16) return f((bf16_t*)nullptr);
    if (dtype == DBSR_F16) return f((f16_t*)nullptr);
    if (dtype == DBSR_F32) return f((float*)nullptr);
    dbsr_set_error("unsupported dtype %d", dtype);
    return DBSR_E_ARG;
}

bool dtype_ok(int d) { return d == DBSR_F32 || d == DBSR_BF16 || d == DBSR_F16; }
int epp_of(int dtype) { return dtype == DBSR_F32 ? 4 : 8; }          // elements per 16 B

// a slice of c channels whose 16-B pieces are aligned and stay inside the pixel; sets the error itself
bool slice_ok(const dbsr_tensor& t, int c, const char* fn, const char* name) {
    if (!t.ptr || t.map.fpg <= 0) {
        dbsr_set_error("%s: %s is null (or its frame map is empty)", fn, name);
        return false;
    }
    if (!dtype_ok(t.dtype)) {
        dbsr_set_error("%s: %s has unsupported dtype %d", fn, name, t.dtype);
        return false;
    }
    const int e = epp_of(t.dtype);
    if (t.ld <= 0 || t.c0 < 0 || t.ld % e || t.c0 % e) {
        dbsr_set_error("%s: %s needs ld and c0 multiples of 16 bytes (ld %d, c0 %d)", fn, name, t.ld, t.c0);
        return false;
    }
    if (t.c0 + rup(c, e) > t.ld) {
        dbsr_set_error("%s: %s channels [c0, c0 + %d) rounded up to 16 bytes leave the pixel (ld %d, c0 %d)", fn, name, c,
                       t.ld, t.c0);
        return false;
    }
    return true;
}

// the conv family both GEMMs serve; sets the error itself
bool conv_ok(const char* fn, int n, int in_h, int in_w, int cin, int out_h, int out_w, int cout, int k, int s, int d,
             int pad) {
    if (n <= 0 || in_h <= 0 || in_w <= 0 || cin <= 0 || out_h <= 0 || out_w <= 0 || cout <= 0) {
        dbsr_set_error("%s: n, in_h, in_w, cin, out_h, out_w, cout must be > 0", fn);
        return false;
    }
    if (k != 1 && k != 3 && k != 4) {
        dbsr_set_error("%s: kernel size %d not in {1, 3, 4}", fn, k);
        return false;
    }
    if (s != 1 && s != 2) {
        dbsr_set_error("%s: stride %d not in {1, 2}", fn, s);
        return false;
    }
    if (d < 1 || pad < 0 || d > (1 << 20) || pad > (1 << 20)) {
        dbsr_set_error("%s: dilation must be >= 1 and pad >= 0 (got %d, %d)", fn, d, pad);
        return false;
    }
    const long long eh = (long long)in_h + 2LL * pad - (long long)d * (k - 1) - 1;
    const long long ew = (long long)in_w + 2LL * pad - (long long)d * (k - 1) - 1;
    if (eh < 0 || ew < 0 || eh / s + 1 != out_h || ew / s + 1 != out_w) {
        dbsr_set_error("%s: out %d x %d is not the conv's output for in %d x %d (k %d, stride %d, dilation %d, pad %d)",
                       fn, out_h, out_w, in_h, in_w, k, s, d, pad);
        return false;
    }
    if ((long long)n * in_h * in_w >= (1LL << 31) || (long long)n * out_h * out_w >= (1LL << 31)) {
        dbsr_set_error("%s: n * h * w must be < 2^31", fn);
        return false;
    }
    return true;
}

typedef short v4s_t __attribute__((ext_vector_type(4)));
template <typename T>
__device__ __forceinline__ f32x4_t mma16(bf16x8_t a, bf16x8_t b, f32x4_t c) {
    if constexpr (std::is_same_v<T, f16_t>) {
        typedef __attribute__((ext_vector_type(8))) _Float16 hv;
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(hv, a), __builtin_bit_cast(hv, b), c, 0, 0, 0);
    } else {
        typedef __attribute__((ext_vector_type(8))) __bf16 bfv;
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bfv, a), __builtin_bit_cast(bfv, b), c, 0, 0, 0);
    }
}
__device__ __forceinline__ v4s_t tr16(const unsigned char* lds_byte) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s_t*)lds_byte);
}

// ------------------------------------------------------------------------------------------------
// wgrad_sd
// ------------------------------------------------------------------------------------------------
struct ConvP {
    int n, in_h, in_w, cin, out_h, out_w, cout, k, s, d, pad;
};
constexpr int SD_CB = 64;      // (co, ci) block edge
constexpr int SD_PX = 32;      // pixels per step: one 16-bit MFMA k-step, eight fp32 ones

template <typename T>
__global__ __launch_bounds__(256) void wgrad_sd_kernel(ConvP p, int nci, dbsr_tensor x, dbsr_tensor dy,
                                                       float* __restrict__ partial) {
    constexpr int ROWB = SD_CB * (int)sizeof(T) + 16;                // a pixel row of 64 channels + 16 B skew
    constexpr int EPP = 16 / (int)sizeof(T), PPR = SD_CB / EPP;
    constexpr int PIECES = 2 * SD_PX * PPR, PT = PIECES / 256;
    static_assert(PIECES % 256 == 0, "whole pieces per thread");
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * SD_PX * ROWB];
    unsigned char* ldy = lds;                                        // [32 px][64 co]
    unsigned char* lx = lds + SD_PX * ROWB;                          // [32 px][64 ci], the tap's pixels
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = wave >> 1, wj = wave & 1;                         // this wave's 32 x 32 quadrant
    const int co0 = blockIdx.y * SD_CB;
    const int tap = blockIdx.z / nci, ci0 = (blockIdx.z - tap * nci) * SD_CB;
    const int ky = tap / p.k, kx = tap - ky * p.k;
    const int ohw = p.out_h * p.out_w, total = p.n * ohw;
    const int n_steps = (total + SD_PX - 1) / SD_PX;
    const int s0 = (int)((long long)n_steps * blockIdx.x / gridDim.x);
    const int s1 = (int)((long long)n_steps * (blockIdx.x + 1) / gridDim.x);
    f32x4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    u32x4_t pre[PT];
    auto fetch = [&](int step) {
#pragma unroll
        for (int q = 0; q < PT; ++q) {
            const int it = threadIdx.x + q * 256;
            const int row = it / PPR, pc = it - row * PPR;
            const int pix = step * SD_PX + (row & (SD_PX - 1));
            u32x4_t v = {0u, 0u, 0u, 0u};
            if (pix < total) {
                const int f = pix / ohw, r = pix - f * ohw;
                const int oy = r / p.out_w, ox = r - oy * p.out_w;
                if (row < SD_PX) {
                    const int c = co0 + pc * EPP;
                    if (c < p.cout) v = *(const u32x4_t*)(img_ptr<T>(dy, f) + (long long)r * dy.ld + c);
                } else {
                    const int iy = oy * p.s - p.pad + ky * p.d, ix = ox * p.s - p.pad + kx * p.d;
                    const int c = ci0 + pc * EPP;
                    if ((unsigned)iy < (unsigned)p.in_h && (unsigned)ix < (unsigned)p.in_w && c < p.cin)
                        v = *(const u32x4_t*)(img_ptr<T>(x, f) + ((long long)iy * p.in_w + ix) * x.ld + c);
                }
            }
            pre[q] = v;
        }
    };
    if (s0 < s1) fetch(s0);
    for (int st = s0; st < s1; ++st) {
#pragma unroll
        for (int q = 0; q < PT; ++q) {
            const int it = threadIdx.x + q * 256;
            const int row = it / PPR, pc = it - row * PPR;
            *(u32x4_t*)(lds + row * ROWB + pc * 16) = pre[q];       // ldy rows, then the lx rows right after them
        }
        __syncthreads();
        if (st + 1 < s1) fetch(st + 1);
        if constexpr (sizeof(T) == 2) {
            // lane (g, q, pp): rows k = 8g + q (+ 4) of the step, channels 4pp .. 4pp+3 of each 16-channel block;
            // the transposed read hands lane l channel l & 15 of k = 8g .. 8g+7 (conv_wgrad_kernel's scheme)
            const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
            bf16x8_t a[2], b[2];
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int kk = 8 * g + 4 * half + q;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const v4s_t va = tr16(ldy + kk * ROWB + ((wi * 2 + i) * 16 + 4 * pp) * 2);
                    const v4s_t vb = tr16(lx + kk * ROWB + ((wj * 2 + i) * 16 + 4 * pp) * 2);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        a[i][4 * half + e] = va[e];
                        b[i][4 * half + e] = vb[e];
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = mma16<T>(a[i], b[j], acc[i][j]);
        } else {
            const int kq = lane >> 4, m = lane & 15;
#pragma unroll
            for (int k4 = 0; k4 < SD_PX / 4; ++k4) {
                const float* arow = (const float*)(ldy + (k4 * 4 + kq) * ROWB);
                const float* brow = (const float*)(lx + (k4 * 4 + kq) * ROWB);
                float av[2], bv[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    av[i] = arow[(wi * 2 + i) * 16 + m];
                    bv[i] = brow[(wj * 2 + i) * 16 + m];
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // C[m = co][n = ci]: lane holds co 4 (lane >> 4) + r of block i, ci lane & 15 of block j
    float* out = partial + (((long long)blockIdx.x * gridDim.y + blockIdx.y) * gridDim.z + blockIdx.z) * (SD_CB * SD_CB);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                out[((wi * 2 + i) * 16 + 4 * (lane >> 4) + r) * SD_CB + (wj * 2 + j) * 16 + (lane & 15)] = acc[i][j][r];
}

// dw[co][ci][tap] (+)= the pixel splits' partials, split 0 first
__global__ __launch_bounds__(256) void wgrad_sd_reduce_kernel(int nbx, int nco, int nci, int taps, int cout, int cin,
                                                              const float* __restrict__ partial, float* __restrict__ dw,
                                                              int accumulate) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)cout * cin * taps) return;
    const int tap = (int)(idx % taps);
    const int ci = (int)((idx / taps) % cin), co = (int)(idx / ((long long)taps * cin));
    const int nz = taps * nci;
    const long long slot = (long long)(co / SD_CB) * nz + tap * nci + ci / SD_CB;
    const int off = (co % SD_CB) * SD_CB + ci % SD_CB;
    float s = 0.f;
    for (int b = 0; b < nbx; ++b) s += partial[((long long)b * nco * nz + slot) * (SD_CB * SD_CB) + off];
    dw[idx] = accumulate ? dw[idx] + s : s;
}

int wgrad_sd_nbx(long long total_px, int cin, int cout, int k) {
    const long long steps = (total_px + SD_PX - 1) / SD_PX;
    const long long nyz = (long long)((cout + SD_CB - 1) / SD_CB) * ((cin + SD_CB - 1) / SD_CB) * k * k;
    return (int)std::max<long long>(1, std::min<long long>(steps, std::min<long long>(64, 1024 / nyz)));
}

// ------------------------------------------------------------------------------------------------
// dgrad_sd
// ------------------------------------------------------------------------------------------------
constexpr int DG_COQ = 32;     // packed co padding: one 16-bit k-step

__global__ void dgrad_sd_pack_kernel(const float* __restrict__ w, int cout, int cin, int k, int cip, int cop,
                                     int dtype, void* __restrict__ wp) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)k * k * cip * cop) return;
    const int co = (int)(idx % cop), ci = (int)((idx / cop) % cip), tap = (int)(idx / ((long long)cop * cip));
    const float v = (co < cout && ci < cin) ? w[((long long)co * cin + ci) * k * k + tap] : 0.f;
    if (dtype == DBSR_F32) ((float*)wp)[idx] = v;
    else if (dtype == DBSR_BF16) ((bf16_t*)wp)[idx] = f2bf(v);
    else ((f16_t*)wp)[idx] = (f16_t)v;
}

// U: 16-pixel units per (frame, class), sized for the largest class
template <typename T>
__global__ __launch_bounds__(256) void dgrad_sd_kernel(ConvP p, int cip, int cop, int U, dbsr_tensor dy,
                                                       const T* __restrict__ wp, dbsr_tensor dx) {
    constexpr int EPP = 16 / (int)sizeof(T);
    constexpr int KS = sizeof(T) == 2 ? 32 : 4;                      // co per MFMA
    const int lane = threadIdx.x & 63;
    const int unit = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int ncls = p.s * p.s;
    if (unit >= p.n * ncls * U) return;                              // whole waves leave; no barrier below
    const int u = unit % U, cls = (unit / U) % ncls, f = unit / (U * ncls);
    const int py = cls / p.s, px = cls - py * p.s;
    const int clh = py < p.in_h ? (p.in_h - py + p.s - 1) / p.s : 0;
    const int clw = px < p.in_w ? (p.in_w - px + p.s - 1) / p.s : 0;
    const int npx = clh * clw;
    if (u * 16 >= npx) return;
    const int m = lane & 15, kq = lane >> 4;
    const int cp = u * 16 + m;
    const bool live = cp < npx;
    const int cy = live ? cp / clw : 0, cx = live ? cp - cy * clw : 0;
    const int iy = cy * p.s + py, ix = cx * p.s + px;
    const int ci0 = blockIdx.y * 64;
    const int nj = min(4, (cip - ci0) / 16);                         // 16-channel blocks of this ci tile
    const int coe = (p.cout + EPP - 1) / EPP * EPP;                  // dy channels that may be read
    const int kend = (p.cout + KS - 1) / KS * KS;
    const T* dyf = img_ptr<T>(dy, f);
    f32x4_t acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int ky = 0; ky < p.k; ++ky) {
        const int ry = py + p.pad - ky * p.d;
        if (((ry % p.s) + p.s) % p.s) continue;                      // wave-uniform: not a tap of this class
        const int ny = iy + p.pad - ky * p.d, oy = ny / p.s;
        const bool vy = live && ny >= 0 && oy < p.out_h;
        for (int kx = 0; kx < p.k; ++kx) {
            const int rx = px + p.pad - kx * p.d;
            if (((rx % p.s) + p.s) % p.s) continue;
            const int nx = ix + p.pad - kx * p.d, ox = nx / p.s;
            const bool ok = vy && nx >= 0 && ox < p.out_w;
            const T* arow = dyf + (ok ? ((long long)oy * p.out_w + ox) * dy.ld : 0);
            const T* wt = wp + (long long)(ky * p.k + kx) * cip * cop + (long long)(ci0 + m) * cop;
            for (int co = 0; co < kend; co += KS) {
                if constexpr (sizeof(T) == 2) {
                    const int cg = co + 8 * kq;
                    u32x4_t av = {0u, 0u, 0u, 0u};
                    if (ok && cg < coe) av = *(const u32x4_t*)(arow + cg);
                    const bf16x8_t a = __builtin_bit_cast(bf16x8_t, av);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < nj) {
                            const u32x4_t bv = *(const u32x4_t*)(wt + (long long)j * 16 * cop + cg);
                            acc[j] = mma16<T>(a, __builtin_bit_cast(bf16x8_t, bv), acc[j]);
                        }
                } else {
                    const int cg = co + kq;
                    const float a = (ok && cg < coe) ? arow[cg] : 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < nj) {
                            const float b = wt[(long long)j * 16 * cop + cg];
                            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[j], 0, 0, 0);
                        }
                }
            }
        }
    }
    // C[m = pixel][n = ci]: lane holds pixels 4 (lane >> 4) + r, channel lane & 15 of block j; the slice's pad
    // channels (up to 16 B) are written as zeros
    const int cst = (p.cin + EPP - 1) / EPP * EPP;
    T* dxf = img_ptr<T>(dx, f);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int cq = u * 16 + 4 * kq + r;
        if (cq >= npx) continue;
        const int qy = cq / clw, qx = cq - qy * clw;
        T* o = dxf + ((long long)(qy * p.s + py) * p.in_w + qx * p.s + px) * dx.ld;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ci = ci0 + j * 16 + m;
            if (j < nj && ci < cst) elem<T>::st(o + ci, ci < p.cin ? acc[j][r] : 0.f);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// activation backward
// ------------------------------------------------------------------------------------------------
// 0.1f * d rounded ONCE to T.  16-bit: the product is exact in double; it is brought to fp32 rounded to odd (the
// truncated value with the sticky bit), which the final fp32 -> 16-bit rounding cannot tell from the exact product.
template <typename T>
__device__ __forceinline__ float slope_once(float d) {
    if constexpr (sizeof(T) == 4) {
        return 0.1f * d;
    } else {
        const double q = (double)d * (double)0.1f;
        float t = (float)q;
        const double r = q - (double)t;
        if (r < 0.0 || r > 0.0) {
            unsigned b = __float_as_uint(t);
            if ((r < 0.0) == (t > 0.f)) b -= 1u;                     // |q| < |t|: one step towards zero
            t = __uint_as_float(b | 1u);
        }
        return t;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void act_bwd_kernel(long long npix, int hw, int c, int act, dbsr_tensor dy,
                                                      dbsr_tensor y, dbsr_tensor dpre) {
    const int groups = (c + 7) / 8;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix * groups) return;
    const int g = (int)(idx % groups);
    const long long pix = idx / groups;
    const int f = (int)(pix / hw), rr = (int)(pix - (long long)f * hw);
    float d[8], v[8], o[8];
    load8(img_ptr<T>(dy, f) + (long long)rr * dy.ld + g * 8, d);
    load8(img_ptr<T>(y, f) + (long long)rr * y.ld + g * 8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float neg = act == DBSR_ACT_LRELU ? slope_once<T>(d[j]) : 0.f;
        o[j] = g * 8 + j < c ? (v[j] > 0.f ? d[j] : neg) : 0.f;
    }
    store8(img_ptr<T>(dpre, f) + (long long)rr * dpre.ld + g * 8, o);
}

// ------------------------------------------------------------------------------------------------
// flow_finalize backward.  Thread = one coarse pixel, both channels; it walks the fine pixels whose bilinear
// footprint (PyTorch's align_corners=False source index, clamped at 0) contains it, rows outer, columns inner.
// The weights, the products and the sums are double (the fp32 source index of a non-dyadic ratio is off by a few
// 2^-24 of the image size, far more than a sum of a dozen terms loses), rounded to fp32 once at the end.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double touch_weight(int dst, int c, int in_size, int out_size) {
    double src = (double)in_size / (double)out_size * ((double)dst + 0.5) - 0.5;
    if (src < 0.0) src = 0.0;
    int i0 = (int)src;
    if (i0 > in_size - 1) i0 = in_size - 1;
    const int i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    const double l1 = src - (double)i0, l0 = 1.0 - l1;
    return (i0 == c ? l0 : 0.0) + (i1 == c ? l1 : 0.0);
}
// fine indices whose source index can lie in (c - 1, c + 1), one to spare on each side
__device__ __forceinline__ void touch_range(int c, int in_size, int out_size, int& lo, int& hi) {
    const double inv = (double)out_size / (double)in_size;
    lo = max(0, (int)floor(((double)c - 0.5) * inv - 0.5) - 1);
    hi = min(out_size - 1, (int)ceil(((double)c + 1.5) * inv - 0.5) + 1);
}

__global__ __launch_bounds__(256) void flow_finalize_bwd_kernel(int P, int hf, int wf, int H, int W, double sx, double sy,
                                                                const float* __restrict__ doff, dbsr_tensor dflow) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)P * hf * wf) return;
    const int p = (int)(idx / (hf * wf)), rr = (int)(idx - (long long)p * hf * wf);
    const int cy = rr / wf, cx = rr - cy * wf;
    int ylo, yhi, xlo, xhi;
    touch_range(cy, hf, H, ylo, yhi);
    touch_range(cx, wf, W, xlo, xhi);
    const float* g = doff + (long long)p * 2 * H * W;
    double a0 = 0.0, a1 = 0.0;
    for (int Y = ylo; Y <= yhi; ++Y) {
        const double wy = touch_weight(Y, cy, hf, H);
        if (wy == 0.0) continue;
        for (int X = xlo; X <= xhi; ++X) {
            const double wgt = wy * touch_weight(X, cx, wf, W);
            a0 += wgt * (double)g[(long long)Y * W + X];
            a1 += wgt * (double)g[(long long)H * W + (long long)Y * W + X];
        }
    }
    float* o = img_ptr<float>(dflow, p) + (long long)rr * dflow.ld;
    o[0] = (float)(20.0 * sx * a0);
    o[1] = (float)(20.0 * sy * a1);
}

}  // namespace

// ================================================================================================
extern "C" size_t dbsr_conv_wgrad_sd_workspace_bytes(int n, int out_h, int out_w, int cin, int cout, int k) {
    if (n <= 0 || out_h <= 0 || out_w <= 0 || cin <= 0 || cout <= 0 || (k != 1 && k != 3 && k != 4)) return 0;
    const long long total = (long long)n * out_h * out_w;
    if (total >= (1LL << 31)) return 0;
    const int nbx = wgrad_sd_nbx(total, cin, cout, k);
    const size_t slots = (size_t)nbx * ((cout + SD_CB - 1) / SD_CB) * ((cin + SD_CB - 1) / SD_CB) * k * k;
    return rup256(slots * SD_CB * SD_CB * sizeof(float)) + rup256(dbsr_chan_sum_workspace_bytes(n, out_h * out_w, cout));
}

extern "C" int dbsr_conv_wgrad_sd(int n, int in_h, int in_w, dbsr_tensor x, int cin, int out_h, int out_w,
                                  dbsr_tensor dy, int cout, int k, int stride, int dil, int pad, float* dw, float* db,
                                  int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "conv_wgrad_sd";
    DBSR_CHECK_ARG(dw && workspace, "conv_wgrad_sd: null dw / workspace");
    if (!conv_ok(fn, n, in_h, in_w, cin, out_h, out_w, cout, k, stride, dil, pad)) return DBSR_E_ARG;
    if (!slice_ok(x, cin, fn, "x") || !slice_ok(dy, cout, fn, "dy")) return DBSR_E_ARG;
    DBSR_CHECK_ARG(x.dtype == dy.dtype, "conv_wgrad_sd: x and dy must share one dtype (got %d, %d)", x.dtype, dy.dtype);
    DBSR_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "conv_wgrad_sd: workspace must be 16-byte aligned");
    const size_t need = dbsr_conv_wgrad_sd_workspace_bytes(n, out_h, out_w, cin, cout, k);
    DBSR_CHECK_ARG(workspace_bytes >= need, "conv_wgrad_sd: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const long long total = (long long)n * out_h * out_w;
    const int nbx = wgrad_sd_nbx(total, cin, cout, k);
    const int nco = (cout + SD_CB - 1) / SD_CB, nci = (cin + SD_CB - 1) / SD_CB, taps = k * k;
    const ConvP p{n, in_h, in_w, cin, out_h, out_w, cout, k, stride, dil, pad};
    hipStream_t s = (hipStream_t)stream;
    float* partial = (float*)workspace;
    int rc = by_dtype(x.dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        hipLaunchKernelGGL(wgrad_sd_kernel<T>, dim3(nbx, nco, taps * nci), dim3(256), 0, s, p, nci, x, dy, partial);
        DBSR_LAUNCH_CHECK();
        return 0;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(wgrad_sd_reduce_kernel, dim3(nblocks((long long)cout * cin * taps, 256)), dim3(256), 0, s, nbx, nco,
                       nci, taps, cout, cin, partial, dw, accumulate);
    DBSR_LAUNCH_CHECK();
    if (db) {
        const size_t off = rup256((size_t)nbx * nco * nci * taps * SD_CB * SD_CB * sizeof(float));
        return dbsr_chan_sum(n, out_h * out_w, cout, dy, db, accumulate, (char*)workspace + off, workspace_bytes - off,
                             stream);
    }
    return 0;
}

extern "C" size_t dbsr_dgrad_sd_packed_elems(int cout, int cin, int k) {
    if (cout <= 0 || cin <= 0 || (k != 1 && k != 3 && k != 4)) return 0;
    return (size_t)k * k * rup(cin, 16) * rup(cout, DG_COQ);
}

extern "C" int dbsr_dgrad_sd_pack(const float* w, int cout, int cin, int k, int dtype, void* w_packed, void* stream) {
    DBSR_CHECK_ARG(w && w_packed, "dgrad_sd_pack: null w / w_packed");
    DBSR_CHECK_ARG(cout > 0 && cin > 0, "dgrad_sd_pack: cout, cin must be > 0");
    DBSR_CHECK_ARG(k == 1 || k == 3 || k == 4, "dgrad_sd_pack: kernel size %d not in {1, 3, 4}", k);
    DBSR_CHECK_ARG(dtype_ok(dtype), "dgrad_sd_pack: unsupported dtype %d", dtype);
    DBSR_CHECK_ARG(((uintptr_t)w_packed & 15) == 0, "dgrad_sd_pack: w_packed must be 16-byte aligned");
    const long long total = (long long)dbsr_dgrad_sd_packed_elems(cout, cin, k);
    hipLaunchKernelGGL(dgrad_sd_pack_kernel, dim3(nblocks(total, 256)), dim3(256), 0, (hipStream_t)stream, w, cout, cin, k,
                       rup(cin, 16), rup(cout, DG_COQ), dtype, w_packed);
    DBSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int dbsr_conv_dgrad_sd(int n, int in_h, int in_w, dbsr_tensor dx, int cin, int out_h, int out_w,
                                  dbsr_tensor dy, int cout, int k, int stride, int dil, int pad, const void* w_packed,
                                  void* stream) {
    const char* fn = "conv_dgrad_sd";
    DBSR_CHECK_ARG(w_packed, "conv_dgrad_sd: null w_packed");
    if (!conv_ok(fn, n, in_h, in_w, cin, out_h, out_w, cout, k, stride, dil, pad)) return DBSR_E_ARG;
    if (!slice_ok(dx, cin, fn, "dx") || !slice_ok(dy, cout, fn, "dy")) return DBSR_E_ARG;
    DBSR_CHECK_ARG(dx.dtype == dy.dtype, "conv_dgrad_sd: dx and dy must share one dtype (got %d, %d)", dx.dtype, dy.dtype);
    DBSR_CHECK_ARG(((uintptr_t)w_packed & 15) == 0, "conv_dgrad_sd: w_packed must be 16-byte aligned");
    const ConvP p{n, in_h, in_w, cin, out_h, out_w, cout, k, stride, dil, pad};
    const int cip = rup(cin, 16), cop = rup(cout, DG_COQ);
    const int U = (((in_h + stride - 1) / stride) * ((in_w + stride - 1) / stride) + 15) / 16;
    const long long units = (long long)n * stride * stride * U;
    DBSR_CHECK_ARG(units < (1LL << 31), "conv_dgrad_sd: too many pixels");
    return by_dtype(dx.dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        hipLaunchKernelGGL(dgrad_sd_kernel<T>, dim3(nblocks(units, 4), (cip + 63) / 64), dim3(256), 0, (hipStream_t)stream,
                           p, cip, cop, U, dy, (const T*)w_packed, dx);
        DBSR_LAUNCH_CHECK();
        return 0;
    });
}

extern "C" int dbsr_act_backward(int n, int hw, int c, int act, dbsr_tensor dy, dbsr_tensor y, dbsr_tensor dpre,
                                 void* stream) {
    const char* fn = "act_backward";
    DBSR_CHECK_ARG(n > 0 && hw > 0 && c > 0, "act_backward: n, hw, c must be > 0");
    DBSR_CHECK_ARG(act == DBSR_ACT_RELU || act == DBSR_ACT_LRELU, "act_backward: act %d is neither ReLU nor LeakyReLU", act);
    if (!slice_ok(dy, c, fn, "dy") || !slice_ok(y, c, fn, "y") || !slice_ok(dpre, c, fn, "dpre")) return DBSR_E_ARG;
    DBSR_CHECK_ARG(dy.dtype == y.dtype && dy.dtype == dpre.dtype, "act_backward: dy, y and dpre must share one dtype");
    const int c8 = rup(c, 8);                                        // a thread owns 8 channels
    DBSR_CHECK_ARG(dy.c0 + c8 <= dy.ld && y.c0 + c8 <= y.ld && dpre.c0 + c8 <= dpre.ld,
                   "act_backward: channels [c0, c0 + %d) rounded up to 8 leave the pixel", c);
    const long long npix = (long long)n * hw;
    DBSR_CHECK_ARG(npix < (1LL << 31), "act_backward: n * hw must be < 2^31");
    return by_dtype(dy.dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        hipLaunchKernelGGL(act_bwd_kernel<T>, dim3(nblocks(npix * (c8 / 8), 256)), dim3(256), 0, (hipStream_t)stream, npix,
                           hw, c, act, dy, y, dpre);
        DBSR_LAUNCH_CHECK();
        return 0;
    });
}

extern "C" int dbsr_flow_finalize_backward(int P, int hf, int wf, int H, int W, int Hp, int Wp, const float* doffsets,
                                           dbsr_tensor dflow, void* stream) {
    DBSR_CHECK_ARG(doffsets && dflow.ptr && dflow.map.fpg > 0, "flow_finalize_backward: null doffsets / dflow");
    DBSR_CHECK_ARG(dflow.dtype == DBSR_F32, "flow_finalize_backward: dflow must be f32");
    DBSR_CHECK_ARG(P > 0 && hf > 0 && wf > 0 && H > 0 && W > 0 && Hp > 0 && Wp > 0,
                   "flow_finalize_backward: P, hf, wf, H, W, Hp, Wp must be > 0");
    DBSR_CHECK_ARG(dflow.ld > 0 && dflow.c0 >= 0 && dflow.c0 + 2 <= dflow.ld,
                   "flow_finalize_backward: dflow channels [c0, c0 + 2) leave the pixel");
    DBSR_CHECK_ARG((long long)P * hf * wf < (1LL << 31) && (long long)P * H * W < (1LL << 30),
                   "flow_finalize_backward: too many pixels");
    hipLaunchKernelGGL(flow_finalize_bwd_kernel, dim3(nblocks((long long)P * hf * wf, 256)), dim3(256), 0,
                       (hipStream_t)stream, P, hf, wf, H, W, (double)W / (double)Wp, (double)H / (double)Hp, doffsets,
                       dflow);
    DBSR_LAUNCH_CHECK();
    return 0;
}
