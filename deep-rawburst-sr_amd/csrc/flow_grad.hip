// Flow gradients: the backward of the two bilinear samplers with respect to the flow, and the export of caller
// supplied offsets into the training forward.
//
//   dbsr_warp_flow_backward   d(dbsr_warp_bilinear)/d(flow)  (models/layers/warp.py:19-46 under autograd:
//                             grid_sample's zero-padding backward w.r.t. the grid, align_corners=False; for this
//                             warp d(ix)/d(fx) = 1, the normalise / unnormalise pair cancels)
//   dbsr_backwarp_backward    d(dbsr_backwarp)/d(input, flow) (models/alignment/pwcnet.py:16-38; the mask is
//                             thresholded in place and carries no gradient)
//   dbsr_offsets_export       full-resolution offsets -> the trainer's `offsets` copy and the offset-feature
//                             extractor's input `om` (offsets % modulo, reference frame zero: what dbsr_flow_finalize
//                             writes from PWC-Net's quarter-resolution flow)
//
// warp flow backward: every output pixel owns its two results, so there are no atomics and the result is
// deterministic.  LPP lanes share a pixel, lane = 8-channel group (16-byte loads of dout and of the four corners),
// fp32 accumulation, a shuffle reduction over the LPP lanes at the end.  At the training shape (c = 512, 16-bit) a
// wave row is one pixel: 1 KiB of dout and up to 4 KiB of corners per pixel, HBM- and gather-bound like the forward's
// warp512_bf16_kernel; warp_flow512_bwd_kernel shapes it the same way (four pixels per wave, every load issued
// before the first use), with the same XCD-contiguous block order so neighbouring pixels' corners share one L2.
// The sample position is the forward's fp32 expression and floorf (dbsr_ops.hip warp_kernel): the same cell.
//
// backwarp backward: din is accumulated with fp32 atomics into an fp32 buffer that the entry point zeroes first
// (as dbsr_warp_backward does for the DBSR warp), so its summation order is NOT fixed: values are equal run to run
// up to fp32 summation order.  dflow is owner-computes (one lane group per pixel, shuffle reduction) and
// deterministic.  Position and mask arithmetic are the forward's (pwc_ops.hip backwarp_kernel).
#include <type_traits>
#include "common.hpp"

using namespace dbsr;

namespace {

inline unsigned nblocks(long long total, int bs) { return (unsigned)((total + bs - 1) / bs); }

template <typename F>
int by_dtype(int dtype, F&& f) {
    if (dtype == DBSR_BF16) return f((bf16_t*)nullptr);
    if (dtype == DBSR_F16) return f((f16_t*)nullptr);
    if (dtype == DBSR_F32) return f((float*)nullptr);
    dbsr_set_error("unsupported dtype %d", dtype);
    return DBSR_E_ARG;
}

bool map_ok(const dbsr_tensor& t) { return t.ptr && t.map.fpg > 0; }
bool vec_ok(const dbsr_tensor& t, int v) { return t.ld % v == 0 && t.c0 % v == 0; }
bool dtype_ok(int d) { return d == DBSR_F32 || d == DBSR_BF16 || d == DBSR_F16; }

template <int LPP>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int off = LPP / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ------------------------------------------------------------------------------------------------
// dflow_x[p] = sum_c dout[p,c] * (wy0 * (v01 - v00) + wy1 * (v11 - v10))
// dflow_y[p] = sum_c dout[p,c] * (wx0 * (v10 - v00) + wx1 * (v11 - v01)),   v = 0 outside the image
// ------------------------------------------------------------------------------------------------
template <typename T, int LPP>
__global__ __launch_bounds__(256) void warp_flow_bwd_kernel(int n, int h, int w, int groups, dbsr_tensor feat,
                                                            dbsr_tensor dout, const float* __restrict__ flow,
                                                            long long fis, float* __restrict__ dflow, long long dis,
                                                            int accumulate) {
    // contiguous pixel ranges per XCD, as the forward (speed only: a bijection of the block index)
    const unsigned b = blockIdx.x, nb = gridDim.x, xcd = b & 7, q8 = nb >> 3, r8 = nb & 7;
    const unsigned lb = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (b >> 3);
    constexpr int PPB = 256 / LPP;
    const int sl = threadIdx.x & (LPP - 1);
    long long pix = (long long)lb * PPB + threadIdx.x / LPP;
    if constexpr (LPP == 64) pix = (long long)__builtin_amdgcn_readfirstlane((unsigned)pix);   // wave-uniform
    const int hw = h * w;
    if (pix >= (long long)n * hw) return;                 // whole lane groups leave together
    const int p = (int)(pix / hw), rr = (int)(pix - (long long)p * hw);
    const int y = rr / w, x = rr - y * w;
    const float* fl = flow + (long long)p * fis + rr;
    const float gx = ((float)x + 0.5f) + fl[0];
    const float gy = ((float)y + 0.5f) + fl[hw];
    const float gxn = 2.0f * gx / (float)w - 1.0f, gyn = 2.0f * gy / (float)h - 1.0f;
    const float ix = ((gxn + 1.f) * (float)w - 1.f) / 2.f;
    const float iy = ((gyn + 1.f) * (float)h - 1.f) / 2.f;
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    // (a position far outside the image: every corner is out, the int conversion saturates and stays out)
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float wx1 = ix - fx0, wx0 = 1.f - wx1, wy1 = iy - fy0, wy0 = 1.f - wy1;
    const bool vx0 = (unsigned)x0 < (unsigned)w, vx1 = (unsigned)x0 + 1u < (unsigned)w;
    const bool vy0 = (unsigned)y0 < (unsigned)h, vy1 = (unsigned)y0 + 1u < (unsigned)h;
    const bool ok00 = vy0 && vx0, ok01 = vy0 && vx1, ok10 = vy1 && vx0, ok11 = vy1 && vx1;
    const T* base = img_ptr<T>(feat, p);
    // in-bounds corners only: the offsets of the others are never used
    const long long o00 = ((long long)y0 * w + x0) * feat.ld, o01 = o00 + feat.ld;
    const long long o10 = o00 + (long long)w * feat.ld, o11 = o10 + feat.ld;
    const T* dp = img_ptr<T>(dout, p) + (long long)rr * dout.ld;
    float ax = 0.f, ay = 0.f;
    if (ok00 || ok01 || ok10 || ok11) {
        for (int g = sl; g < groups; g += LPP) {
            float d[8], v00[8], v01[8], v10[8], v11[8];
            load8(dp + g * 8, d);
#pragma unroll
            for (int j = 0; j < 8; ++j) v00[j] = v01[j] = v10[j] = v11[j] = 0.f;
            if (ok00) load8(base + o00 + g * 8, v00);
            if (ok01) load8(base + o01 + g * 8, v01);
            if (ok10) load8(base + o10 + g * 8, v10);
            if (ok11) load8(base + o11 + g * 8, v11);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float sx = fmaf(wy1, v11[j] - v10[j], wy0 * (v01[j] - v00[j]));
                const float sy = fmaf(wx1, v11[j] - v01[j], wx0 * (v10[j] - v00[j]));
                ax = fmaf(d[j], sx, ax);
                ay = fmaf(d[j], sy, ay);
            }
        }
    }
    ax = group_sum<LPP>(ax);
    ay = group_sum<LPP>(ay);
    if (sl == 0) {
        float* o = dflow + (long long)p * dis + rr;
        if (accumulate) {
            o[0] += ax;
            o[hw] += ay;
        } else {
            o[0] = ax;
            o[hw] = ay;
        }
    }
}

// c == 512 in 16 bits (the training shape: a wave is one 1-KiB pixel row per load): each wave takes PPW consecutive
// pixels and issues all 5 * PPW loads (dout and the four corners) before consuming any, as warp512_bf16_kernel
// does -- with one pixel per wave only five loads are in flight and the kernel waits on latency.  A corner outside
// the image is loaded from the image's first pixel (an in-bounds address) and selected to 0.
template <typename T, int PPW>
__global__ __launch_bounds__(256) void warp_flow512_bwd_kernel(int n, int h, int w, dbsr_tensor feat, dbsr_tensor dout,
                                                               const float* __restrict__ flow, long long fis,
                                                               float* __restrict__ dflow, long long dis,
                                                               int accumulate) {
    const unsigned b = blockIdx.x, nb = gridDim.x, xcd = b & 7, q8 = nb >> 3, r8 = nb & 7;
    const unsigned lb = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (b >> 3);
    const unsigned gw = __builtin_amdgcn_readfirstlane(lb * 4 + (threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int hw = h * w;
    const unsigned total = (unsigned)n * hw;
    int tapoff[PPW][4];
    bool ok[PPW][4], live[PPW];
    float wx0[PPW], wx1[PPW], wy0[PPW], wy1[PPW];
    const T* fbase[PPW];
    const T* dptr[PPW];
    float* optr[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const unsigned pix = gw * PPW + i;
        live[i] = pix < total;
        const unsigned pc = live[i] ? pix : 0;
        const int p = (int)(pc / hw), rr = (int)(pc - (unsigned)p * hw);
        const int y = rr / w, x = rr - y * w;
        const float* fl = flow + (long long)p * fis + rr;
        const float gx = ((float)x + 0.5f) + fl[0];
        const float gy = ((float)y + 0.5f) + fl[hw];
        const float gxn = 2.0f * gx / (float)w - 1.0f, gyn = 2.0f * gy / (float)h - 1.0f;
        const float ix = ((gxn + 1.f) * (float)w - 1.f) / 2.f;
        const float iy = ((gyn + 1.f) * (float)h - 1.f) / 2.f;
        const float fx0 = floorf(ix), fy0 = floorf(iy);
        const int x0 = (int)fx0, y0 = (int)fy0;
        wx1[i] = ix - fx0; wx0[i] = 1.f - wx1[i];
        wy1[i] = iy - fy0; wy0[i] = 1.f - wy1[i];
        const bool vx[2] = {(unsigned)x0 < (unsigned)w, (unsigned)x0 + 1u < (unsigned)w};
        const bool vy[2] = {(unsigned)y0 < (unsigned)h, (unsigned)y0 + 1u < (unsigned)h};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            ok[i][t] = vx[t & 1] && vy[t >> 1];
            // (unsigned arithmetic: a saturated x0 / y0 far outside wraps harmlessly and is not used)
            const unsigned ux = (unsigned)x0 + (t & 1), uy = (unsigned)y0 + (t >> 1);
            tapoff[i][t] = ok[i][t] ? (int)((uy * (unsigned)w + ux) * (unsigned)feat.ld) : 0;
        }
        fbase[i] = img_ptr<T>(feat, p) + lane * 8;
        dptr[i] = img_ptr<T>(dout, p) + (long long)rr * dout.ld + lane * 8;
        optr[i] = dflow + (long long)p * dis + rr;
    }
    u32x4_t v[PPW][4], d[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        d[i] = *(const u32x4_t*)dptr[i];
#pragma unroll
        for (int t = 0; t < 4; ++t) v[i][t] = *(const u32x4_t*)(fbase[i] + tapoff[i][t]);
    }
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        float ax = 0.f, ay = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                float c[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float val = s ? H16<T>::hi(v[i][t][e]) : H16<T>::lo(v[i][t][e]);
                    c[t] = ok[i][t] ? val : 0.f;
                }
                const float dv = s ? H16<T>::hi(d[i][e]) : H16<T>::lo(d[i][e]);
                const float sx = fmaf(wy1[i], c[3] - c[2], wy0[i] * (c[1] - c[0]));
                const float sy = fmaf(wx1[i], c[3] - c[1], wx0[i] * (c[2] - c[0]));
                ax = fmaf(dv, sx, ax);
                ay = fmaf(dv, sy, ay);
            }
        }
        ax = group_sum<64>(ax);
        ay = group_sum<64>(ay);
        if (lane == 0 && live[i]) {
            if (accumulate) {
                optr[i][0] += ax;
                optr[i][hw] += ay;
            } else {
                optr[i][0] = ax;
                optr[i][hw] = ay;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// backwarp backward.  Lane = channels g*8 .. g*8+7 of a pixel for g = sl, sl + LPP, ...
// ------------------------------------------------------------------------------------------------
template <typename T, int LPP>
__global__ __launch_bounds__(256) void backwarp_bwd_kernel(int n, int h, int w, int C, dbsr_tensor in, dbsr_tensor flow,
                                                           float scale, dbsr_tensor dout, dbsr_tensor din,
                                                           dbsr_tensor dflow) {
    constexpr int PPB = 256 / LPP;
    const int sl = threadIdx.x & (LPP - 1);
    const long long pix = (long long)blockIdx.x * PPB + threadIdx.x / LPP;
    if (pix >= (long long)n * h * w) return;              // whole lane groups leave together
    const int p = (int)(pix / (h * w));
    const int rr = (int)(pix - (long long)p * h * w);
    const int y = rr / w, x = rr - y * w;
    const float* fl = img_ptr<float>(flow, p) + (long long)rr * flow.ld;
    const float fx = fl[0] * scale, fy = fl[1] * scale;
    const float gxn = (-1.0f + (2.0f * x + 1.0f) / (float)w) + fx / (((float)w - 1.0f) / 2.0f);
    const float gyn = (-1.0f + (2.0f * y + 1.0f) / (float)h) + fy / (((float)h - 1.0f) / 2.0f);
    const float ix = ((gxn + 1.f) * (float)w - 1.f) / 2.f;
    const float iy = ((gyn + 1.f) * (float)h - 1.f) / 2.f;
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float wx1 = ix - fx0, wx0 = 1.f - wx1, wy1 = iy - fy0, wy0 = 1.f - wy1;
    const bool vx0 = (unsigned)x0 < (unsigned)w, vx1 = (unsigned)x0 + 1u < (unsigned)w;
    const bool vy0 = (unsigned)y0 < (unsigned)h, vy1 = (unsigned)y0 + 1u < (unsigned)h;
    const bool ok00 = vy0 && vx0, ok01 = vy0 && vx1, ok10 = vy1 && vx0, ok11 = vy1 && vx1;
    const float w00 = ok00 ? wy0 * wx0 : 0.f, w01 = ok01 ? wy0 * wx1 : 0.f;
    const float w10 = ok10 ? wy1 * wx0 : 0.f, w11 = ok11 ? wy1 * wx1 : 0.f;
    const float mass = w00 + w01 + w10 + w11;
    const bool keep = mass > 0.999f;                      // the forward's mask
    float ax = 0.f, ay = 0.f;
    if (keep) {
        const long long o00 = (long long)y0 * w + x0, o01 = o00 + 1, o10 = o00 + w, o11 = o10 + 1;
        const T* dp = img_ptr<T>(dout, p) + (long long)rr * dout.ld;
        const T* base = dflow.ptr ? img_ptr<T>(in, p) : nullptr;
        float* gi = din.ptr ? img_ptr<float>(din, p) : nullptr;
        const int groups = (C + 7) / 8;
        for (int g = sl; g < groups; g += LPP) {
            const int c_end = min(C, g * 8 + 8);
            for (int c = g * 8; c < c_end; ++c) {
                const float d = elem<T>::ld(dp + c);
                if (gi) {
                    if (ok00) atomicAdd(gi + o00 * din.ld + c, w00 * d);
                    if (ok01) atomicAdd(gi + o01 * din.ld + c, w01 * d);
                    if (ok10) atomicAdd(gi + o10 * din.ld + c, w10 * d);
                    if (ok11) atomicAdd(gi + o11 * din.ld + c, w11 * d);
                }
                if (base) {
                    const float v00 = ok00 ? elem<T>::ld(base + o00 * in.ld + c) : 0.f;
                    const float v01 = ok01 ? elem<T>::ld(base + o01 * in.ld + c) : 0.f;
                    const float v10 = ok10 ? elem<T>::ld(base + o10 * in.ld + c) : 0.f;
                    const float v11 = ok11 ? elem<T>::ld(base + o11 * in.ld + c) : 0.f;
                    ax = fmaf(d, fmaf(wy1, v11 - v10, wy0 * (v01 - v00)), ax);
                    ay = fmaf(d, fmaf(wx1, v11 - v01, wx0 * (v10 - v00)), ay);
                }
            }
        }
    }
    if (dflow.ptr) {
        ax = group_sum<LPP>(ax);
        ay = group_sum<LPP>(ay);
        if (sl == 0) {
            // d(ix)/d(flow_x) = scale * (2 / (W - 1)) * (W / 2): flow / ((W - 1) / 2) on an align_corners=False grid
            float* o = img_ptr<float>(dflow, p) + (long long)rr * dflow.ld;
            o[0] = keep ? ax * (scale * ((float)w / ((float)w - 1.0f))) : 0.f;
            o[1] = keep ? ay * (scale * ((float)h / ((float)h - 1.0f))) : 0.f;
        }
    }
}

__global__ void zero_slice_kernel(int n, int hw, int C, dbsr_tensor t) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)n * hw * C) return;
    const int c = (int)(idx % C);
    const long long pix = idx / C;
    const int p = (int)(pix / hw), rr = (int)(pix - (long long)p * hw);
    img_ptr<float>(t, p)[(long long)rr * t.ld + c] = 0.f;
}

// ------------------------------------------------------------------------------------------------
// offsets export: thread = (frame, pixel).  The remainder is dbsr_flow_finalize's (torch.remainder).
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void offsets_export_kernel(int B, int N, int hw, const float* __restrict__ flow, long long fis,
                                      float* __restrict__ offsets, float modulo, dbsr_tensor om) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)B * N * hw) return;
    const int f = (int)(idx / hw), rr = (int)(idx - (long long)f * hw);
    const int b = f / N, nn = f - b * N;
    if (nn == 0) {
        if (om.ptr) {
            T* o = img_ptr<T>(om, f) + (long long)rr * om.ld;
            elem<T>::st(o, 0.f);
            elem<T>::st(o + 1, 0.f);
        }
        return;
    }
    const int p = b * (N - 1) + nn - 1;
    const float* fl = flow + (long long)p * fis + rr;
    const float v[2] = {fl[0], fl[hw]};
    if (offsets) {
        float* op = offsets + (long long)p * 2 * hw + rr;
        op[0] = v[0];
        op[hw] = v[1];
    }
    if (om.ptr) {
        T* o = img_ptr<T>(om, f) + (long long)rr * om.ld;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float m = v[c];
            if (modulo != 0.f) {
                m = fmodf(v[c], modulo);
                if (m != 0.f && ((m < 0.f) != (modulo < 0.f))) m += modulo;
            }
            elem<T>::st(o + c, m);
        }
    }
}

}  // namespace

extern "C" int dbsr_warp_flow_backward(int n, int h, int w, int c, dbsr_tensor feat, dbsr_tensor dout,
                                       const float* flow, long long flow_img_stride, float* dflow,
                                       long long dflow_img_stride, int accumulate, void* stream) {
    DBSR_CHECK_ARG(map_ok(feat) && map_ok(dout) && flow && dflow, "warp_flow_backward: null feat / dout / flow / dflow");
    DBSR_CHECK_ARG(dtype_ok(feat.dtype) && feat.dtype == dout.dtype, "warp_flow_backward: feat and dout must share "
                   "one dtype (f32, bf16 or f16)");
    DBSR_CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0, "warp_flow_backward: n, h, w, c must be > 0");
    DBSR_CHECK_ARG(c % 8 == 0, "warp_flow_backward: c must be a multiple of 8 (got %d)", c);
    DBSR_CHECK_ARG(vec_ok(feat, 8) && vec_ok(dout, 8), "warp_flow_backward: ld/c0 must be multiples of 8");
    DBSR_CHECK_ARG(feat.c0 >= 0 && dout.c0 >= 0 && feat.c0 + c <= feat.ld && dout.c0 + c <= dout.ld,
                   "warp_flow_backward: the slice [c0, c0 + c) exceeds ld");
    const long long hw = (long long)h * w;
    DBSR_CHECK_ARG(hw * n < (1LL << 31), "warp_flow_backward: n * h * w must be < 2^31");
    DBSR_CHECK_ARG(flow_img_stride >= 2 * hw && dflow_img_stride >= 2 * hw,
                   "warp_flow_backward: flow / dflow image strides must be >= 2 * h * w");
    const int groups = c / 8;
    const long long px = hw * n;
    hipStream_t s = (hipStream_t)stream;
    return by_dtype(feat.dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
#define DBSR_WFB(LPP)                                                                                               \
    hipLaunchKernelGGL((warp_flow_bwd_kernel<T, LPP>), dim3(nblocks(px, 256 / LPP)), dim3(256), 0, s, n, h, w, groups, \
                       feat, dout, flow, flow_img_stride, dflow, dflow_img_stride, accumulate)
        if constexpr (sizeof(T) == 2) {
            if (groups == 64 && hw * feat.ld < (1LL << 31)) {
                constexpr int PPW = 4;
                hipLaunchKernelGGL((warp_flow512_bwd_kernel<T, PPW>), dim3(nblocks((px + PPW - 1) / PPW, 4)), dim3(256),
                                   0, s, n, h, w, feat, dout, flow, flow_img_stride, dflow, dflow_img_stride,
                                   accumulate);
                DBSR_LAUNCH_CHECK();
                return 0;
            }
        }
        if (groups >= 64) DBSR_WFB(64);
        else if (groups >= 16) DBSR_WFB(16);
        else if (groups >= 4) DBSR_WFB(4);
        else DBSR_WFB(1);
#undef DBSR_WFB
        DBSR_LAUNCH_CHECK();
        return 0;
    });
}

extern "C" int dbsr_backwarp_backward(int n, int h, int w, int c, dbsr_tensor in, dbsr_tensor flow, float scale,
                                      dbsr_tensor dout, dbsr_tensor din, dbsr_tensor dflow, void* stream) {
    DBSR_CHECK_ARG(din.ptr || dflow.ptr, "backwarp_backward: din and dflow are both null");
    DBSR_CHECK_ARG(map_ok(flow) && map_ok(dout), "backwarp_backward: null flow / dout");
    DBSR_CHECK_ARG(flow.dtype == DBSR_F32 && dtype_ok(dout.dtype), "backwarp_backward: flow is f32, dout f32 / bf16 / f16");
    DBSR_CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0, "backwarp_backward: n, h, w, c must be > 0");
    DBSR_CHECK_ARG((long long)n * h * w < (1LL << 31), "backwarp_backward: n * h * w must be < 2^31");
    DBSR_CHECK_ARG(flow.c0 >= 0 && flow.c0 + 2 <= flow.ld && dout.c0 >= 0 && dout.c0 + c <= dout.ld,
                   "backwarp_backward: flow / dout slice exceeds ld");
    if (dflow.ptr) {
        DBSR_CHECK_ARG(map_ok(in) && in.dtype == dout.dtype && in.c0 >= 0 && in.c0 + c <= in.ld,
                       "backwarp_backward: dflow needs the forward's input, of dout's dtype");
        DBSR_CHECK_ARG(map_ok(dflow) && dflow.dtype == DBSR_F32 && dflow.c0 >= 0 && dflow.c0 + 2 <= dflow.ld,
                       "backwarp_backward: dflow is an f32 NHWC tensor with 2 channels");
    }
    if (din.ptr)
        DBSR_CHECK_ARG(map_ok(din) && din.dtype == DBSR_F32 && din.c0 >= 0 && din.c0 + c <= din.ld,
                       "backwarp_backward: din is an f32 NHWC tensor with c channels (fp32 atomics)");
    hipStream_t s = (hipStream_t)stream;
    const long long px = (long long)n * h * w;
    if (din.ptr) {
        hipLaunchKernelGGL(zero_slice_kernel, dim3(nblocks(px * c, 256)), dim3(256), 0, s, n, h * w, c, din);
        DBSR_LAUNCH_CHECK();
    }
    const int groups = (c + 7) / 8;
    return by_dtype(dout.dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
#define DBSR_BWB(LPP)                                                                                               \
    hipLaunchKernelGGL((backwarp_bwd_kernel<T, LPP>), dim3(nblocks(px, 256 / LPP)), dim3(256), 0, s, n, h, w, c, in, \
                       flow, scale, dout, din, dflow)
        if (groups >= 16) DBSR_BWB(16);
        else if (groups >= 8) DBSR_BWB(8);
        else if (groups >= 4) DBSR_BWB(4);
        else if (groups >= 2) DBSR_BWB(2);
        else DBSR_BWB(1);
#undef DBSR_BWB
        DBSR_LAUNCH_CHECK();
        return 0;
    });
}

extern "C" int dbsr_offsets_export(int B, int N, int H, int W, const float* flow, long long flow_img_stride,
                                   float* offsets, float modulo, dbsr_tensor offs_mod, void* stream) {
    DBSR_CHECK_ARG(flow && (offsets || offs_mod.ptr), "offsets_export: null flow, or nothing to write");
    DBSR_CHECK_ARG(B > 0 && N > 1 && H > 0 && W > 0, "offsets_export: B, H, W > 0 and N > 1");
    const long long hw = (long long)H * W;
    DBSR_CHECK_ARG(hw * B * N < (1LL << 31), "offsets_export: B * N * H * W must be < 2^31");
    DBSR_CHECK_ARG(flow_img_stride >= 2 * hw, "offsets_export: flow image stride must be >= 2 * H * W");
    if (offs_mod.ptr)
        DBSR_CHECK_ARG(map_ok(offs_mod) && dtype_ok(offs_mod.dtype) && offs_mod.c0 >= 0 && offs_mod.c0 + 2 <= offs_mod.ld,
                       "offsets_export: bad offs_mod");
    const int dt = offs_mod.ptr ? offs_mod.dtype : DBSR_F32;
    return by_dtype(dt, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        hipLaunchKernelGGL(offsets_export_kernel<T>, dim3(nblocks(hw * B * N, 256)), dim3(256), 0, (hipStream_t)stream,
                           B, N, (int)hw, flow, flow_img_stride, offsets, modulo, offs_mod);
        DBSR_LAUNCH_CHECK();
        return 0;
    });
}
