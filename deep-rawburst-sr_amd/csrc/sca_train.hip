// Real-world fine-tuning objective (train_settings/dbsr/default_realworld.py:65-79, actors/dbsr_actors.py:50-95):
// the L1 error between the spatially and colour-aligned prediction and the ground truth, over the validity
// mask and the boundary crop, and its gradient w.r.t. the prediction.  In the reference the flow is computed
// under no_grad and the colour matrix C is fitted from the ground truth and the warped base frame only
// (spatial_color_alignment.py:87-108), so with pw = warp(pred, flow) and m_k = sum_c pw_c C[c][k]
//   loss    = weight * sum(valid * |m - gt|) / (3 * sum(valid) + 1e-12)        (image_quality_v2.py:47-66)
//   dL/dpw  = scale * valid * sum_k C[c][k] sign(m_k - gt_k),   scale = weight / (3 * sum(valid) + 1e-12)
//   dL/dpred = warp^T(dL/dpw)                                  (the bilinear taps' transpose: a scatter-add)
// fp32 NCHW planes as sca_ops.hip; the warp is models/layers/warp.py:19-46 (bilinear, zeros padding,
// align_corners=False) with the float op sequence of dbsr_warp_bilinear.  Everything stays on the device: the
// loss and the scale are written by a one-block reduction in a fixed order (bitwise reproducible), the backward
// reads the scale from memory.  All kernels are HBM / latency bound: a thread per pixel, planes read and
// written coalesced, the 4 bilinear taps of neighbouring pixels served by the L2.
#include "common.hpp"

#include <algorithm>

using namespace dbsr;

namespace {

inline unsigned nblk(long long n, int per = 256) { return (unsigned)((n + per - 1) / per); }

struct Taps { int x0, y0; float wx1, wy1; };
// bilinear taps of output pixel (x, y) (grid_sample, zeros, align_corners=False; warp_kernel's op sequence)
__device__ __forceinline__ Taps taps_of(int x, int y, int w, int h, float fx, float fy) {
    const float gx = ((float)x + 0.5f) + fx, gy = ((float)y + 0.5f) + fy;
    const float gxn = 2.0f * gx / (float)w - 1.0f, gyn = 2.0f * gy / (float)h - 1.0f;
    const float ix = ((gxn + 1.f) * (float)w - 1.f) / 2.f, iy = ((gyn + 1.f) * (float)h - 1.f) / 2.f;
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    Taps t;
    // far-away / non-finite coordinates: no tap in the frame (x0 = -2 keeps both columns out)
    const bool ok = fx0 >= -1.f && fx0 < (float)w && fy0 >= -1.f && fy0 < (float)h;
    t.x0 = ok ? (int)fx0 : -2;
    t.y0 = ok ? (int)fy0 : -2;
    t.wx1 = ix - fx0;
    t.wy1 = iy - fy0;
    return t;
}

__device__ __forceinline__ float sgn(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// sum over the block's 256 threads, waves in order (fixed order); every thread gets the result.  red: 4 floats
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// One pass over the pixels (256 consecutive ones of the flat [B][H][W] index per block, as l1_loss_bwd_kernel:
// with flow, c_mat and valid NULL the |d| partials are bitwise that kernel's).  Per block: partial[blk][0] =
// sum valid |m - gt|; for the s-th image the block touches (s < slots): partial[blk][1 + 2s] = sum valid
// (m - gt)^2, partial[blk][2 + 2s] = sum valid.
__global__ __launch_bounds__(256) void al1_fwd_kernel(int B, int H, int W, int bi, int slots,
                                                      const float* __restrict__ pred, const float* __restrict__ flow,
                                                      const float* __restrict__ cmat,
                                                      const unsigned char* __restrict__ valid,
                                                      const float* __restrict__ gt, float* __restrict__ gpw,
                                                      float* __restrict__ partial) {
    const int hw = H * W;
    const int total = B * hw;                                   // < 2^31 (checked by the caller)
    const int idx = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const int b_first = (int)(((long long)blockIdx.x * 256) / hw);
    float s = 0.f, sq = 0.f, cnt = 0.f;
    int slot = -1;
    if (idx < total) {
        const int b = idx / hw, rr = idx - b * hw;
        const int y = rr / W, x = rr - y * W;
        slot = b - b_first;
        const bool in = y >= bi && y < H - bi && x >= bi && x < W - bi;
        float g[3] = {0.f, 0.f, 0.f};
        if (in && (!valid || valid[idx])) {
            const float* P = pred + (long long)b * 3 * hw;
            float pw[3] = {0.f, 0.f, 0.f};
            if (flow) {
                const float* fl = flow + (long long)b * 2 * hw;
                const Taps t = taps_of(x, y, W, H, fl[rr], fl[hw + rr]);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int xx = t.x0 + (k & 1), yy = t.y0 + (k >> 1);
                    if ((unsigned)xx >= (unsigned)W || (unsigned)yy >= (unsigned)H) continue;
                    const float wt = ((k & 1) ? t.wx1 : 1.f - t.wx1) * ((k >> 1) ? t.wy1 : 1.f - t.wy1);
                    const int o = yy * W + xx;
#pragma unroll
                    for (int c = 0; c < 3; ++c) pw[c] = fmaf(wt, P[o + c * hw], pw[c]);
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) pw[c] = P[rr + c * hw];
            }
            float C[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
            if (cmat) {
#pragma unroll
                for (int i = 0; i < 9; ++i) C[i] = cmat[b * 9 + i];
            }
            float sg[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float m = cmat ? pw[0] * C[k] + pw[1] * C[3 + k] + pw[2] * C[6 + k] : pw[k];
                const float d = m - gt[(long long)b * 3 * hw + k * hw + rr];
                s += fabsf(d);
                sq = fmaf(d, d, sq);
                sg[k] = sgn(d);
            }
            cnt = 1.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) g[c] = cmat ? C[c * 3] * sg[0] + C[c * 3 + 1] * sg[1] + C[c * 3 + 2] * sg[2] : sg[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) gpw[(long long)b * 3 * hw + c * hw + rr] = g[c];
    }
    __shared__ float red[256];
    __shared__ float red4[4];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    float* out = partial + (long long)blockIdx.x * (1 + 2 * slots);
    if (threadIdx.x == 0) out[0] = red[0];
    for (int sl = 0; sl < slots; ++sl) {
        const float a = block_sum(slot == sl ? sq : 0.f, red4);
        const float c = block_sum(slot == sl ? cnt : 0.f, red4);
        if (threadIdx.x == 0) {
            out[1 + 2 * sl] = a;
            out[2 + 2 * sl] = c;
        }
    }
}

// Block 0: loss[1] = scale = weight / (3 sum valid + 1e-12), loss[0] = scale * sum of the |d| partials (strided
// per-thread sums, then a tree: sum_all_kernel's order).  Block 1 + b: stats[b] = {sum valid (m - gt)^2, sum
// valid} of image b, from the slots of the blocks that touch it.
__global__ __launch_bounds__(256) void al1_finish_kernel(int nb, int hw, int slots, const float* __restrict__ partial,
                                                         float weight, float* __restrict__ loss,
                                                         float* __restrict__ stats) {
    __shared__ float red[256];
    __shared__ double dred[256];
    const int stride = 1 + 2 * slots;
    if (blockIdx.x == 0) {
        float s = 0.f;
        double c = 0.0;
        for (int i = threadIdx.x; i < nb; i += 256) {
            s += partial[(long long)i * stride];
            for (int sl = 0; sl < slots; ++sl) c += (double)partial[(long long)i * stride + 2 + 2 * sl];
        }
        red[threadIdx.x] = s;
        dred[threadIdx.x] = c;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if ((int)threadIdx.x < st) {
                red[threadIdx.x] += red[threadIdx.x + st];
                dred[threadIdx.x] += dred[threadIdx.x + st];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const float scale = weight / ((float)(3.0 * dred[0]) + 1e-12f);
            loss[0] = red[0] * scale;
            loss[1] = scale;
        }
        return;
    }
    if (!stats) return;
    const int b = (int)blockIdx.x - 1;
    const int lo = (int)(((long long)b * hw) / 256), hi = (int)((((long long)b + 1) * hw - 1) / 256);
    double a = 0.0, c = 0.0;
    for (int i = lo + (int)threadIdx.x; i <= hi; i += 256) {
        const int sl = b - (int)(((long long)i * 256) / hw);
        a += (double)partial[(long long)i * stride + 1 + 2 * sl];
        c += (double)partial[(long long)i * stride + 2 + 2 * sl];
    }
    for (int pass = 0; pass < 2; ++pass) {
        __syncthreads();
        dred[threadIdx.x] = pass ? c : a;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if ((int)threadIdx.x < st) dred[threadIdx.x] += dred[threadIdx.x + st];
            __syncthreads();
        }
        if (threadIdx.x == 0) stats[b * 2 + pass] = (float)dred[0];
    }
}

__global__ __launch_bounds__(256) void al1_zero_kernel(long long n4, float4* __restrict__ p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) p[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// warp^T as a scatter-add: acc[b][c][tap of p] += w_tap * (C g[p])_c, fp32 atomics on 3 planes.  A wave's 64
// pixels of a row add to ~65 contiguous floats per plane and tap row (256-B segments); pixels whose gradient is
// zero (outside the crop or the mask) add nothing.
__global__ __launch_bounds__(256) void al1_scatter_kernel(int B, int H, int W, const float* __restrict__ flow,
                                                          const float* __restrict__ g, const float* __restrict__ cmat,
                                                          float* __restrict__ acc) {
    const int hw = H * W;
    const int idx = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (idx >= B * hw) return;
    const int b = idx / hw, rr = idx - b * hw;
    const int y = rr / W, x = rr - y * W;
    const float* G = g + (long long)b * 3 * hw + rr;
    float v[3] = {G[0], G[hw], G[2 * hw]};
    if (v[0] == 0.f && v[1] == 0.f && v[2] == 0.f) return;
    if (cmat) {
        const float* C = cmat + b * 9;
        const float a0 = v[0], a1 = v[1], a2 = v[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = C[c * 3] * a0 + C[c * 3 + 1] * a1 + C[c * 3 + 2] * a2;
    }
    const float* fl = flow + (long long)b * 2 * hw;
    const Taps t = taps_of(x, y, W, H, fl[rr], fl[hw + rr]);
    float* A = acc + (long long)b * 3 * hw;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int xx = t.x0 + (k & 1), yy = t.y0 + (k >> 1);
        if ((unsigned)xx >= (unsigned)W || (unsigned)yy >= (unsigned)H) continue;
        const float wt = ((k & 1) ? t.wx1 : 1.f - t.wx1) * ((k >> 1) ? t.wy1 : 1.f - t.wy1);
        const int o = yy * W + xx;
#pragma unroll
        for (int c = 0; c < 3; ++c) atomicAdd(A + o + c * hw, wt * v[c]);
    }
}

// dpred = scale * src (src: the scatter's sums, or with no flow C g itself) into fp32 NCHW gpred and / or the
// ReLU-gated NHWC dpre of the predictor's backward ([pred > 0] * dpred: what l1_loss_bwd_kernel / relu_grad_kernel
// write).  V8: 16-bit dpre with exactly 8 channels per pixel, one 16-B store (channels 3..7 zero).
template <typename T, bool V8>
__global__ __launch_bounds__(256) void al1_out_kernel(int B, int H, int W, const float* __restrict__ pred,
                                                      const float* __restrict__ src, const float* __restrict__ cmat,
                                                      const float* __restrict__ scale_p, float* __restrict__ gpred,
                                                      dbsr_tensor dpre) {
    const int hw = H * W;
    const int idx = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (idx >= B * hw) return;
    const int b = idx / hw, rr = idx - b * hw;
    const float scale = scale_p ? *scale_p : 1.f;
    const long long o = (long long)b * 3 * hw + rr;
    float v[3] = {src[o], src[o + hw], src[o + 2 * hw]};
    if (cmat) {
        const float* C = cmat + b * 9;
        const float a0 = v[0], a1 = v[1], a2 = v[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = C[c * 3] * a0 + C[c * 3 + 1] * a1 + C[c * 3 + 2] * a2;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] *= scale;
    if (gpred) {
#pragma unroll
        for (int c = 0; c < 3; ++c) gpred[o + c * hw] = v[c];
    }
    if (dpre.ptr) {
        float gv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 3; ++c) gv[c] = pred[o + c * hw] > 0.f ? v[c] : 0.f;
        T* d = img_ptr<T>(dpre, b) + (long long)rr * dpre.ld;
        if constexpr (V8) {
            store8(d, gv);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) elem<T>::st(d + c, gv[c]);
        }
    }
}

inline int al1_slots(int B, int hw) { return std::min(B, 255 / hw + 2); }
inline size_t al1_fwd_bytes(int B, int H, int W) {
    const long long total = (long long)B * H * W;
    return (size_t)nblk(total) * (1 + 2 * al1_slots(B, H * W)) * sizeof(float);
}
inline size_t al1_bwd_bytes(int B, int H, int W) { return ((size_t)B * 3 * H * W * sizeof(float) + 15) / 16 * 16; }

}  // namespace

extern "C" size_t dbsr_aligned_l1_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || (long long)B * H * W >= (1LL << 31)) return 0;
    return std::max(al1_fwd_bytes(B, H, W), al1_bwd_bytes(B, H, W));
}

extern "C" int dbsr_aligned_l1_forward(int B, int H, int W, int boundary_ignore, const float* pred, const float* flow,
                                       const float* c_mat, const unsigned char* valid, const float* gt, float weight,
                                       float* g_pw, float* loss, float* stats, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    DBSR_CHECK_ARG(pred && gt && g_pw && loss && workspace, "aligned_l1_forward: null pointer");
    DBSR_CHECK_ARG(B > 0 && boundary_ignore >= 0 && H > 2 * boundary_ignore && W > 2 * boundary_ignore,
                   "aligned_l1_forward: bad sizes (H, W must exceed 2 * boundary_ignore)");
    DBSR_CHECK_ARG((long long)B * H * W < (1LL << 31), "aligned_l1_forward: B * H * W must be < 2^31");
    DBSR_CHECK_ARG(workspace_bytes >= al1_fwd_bytes(B, H, W), "aligned_l1_forward: workspace %zu < %zu bytes",
                   workspace_bytes, al1_fwd_bytes(B, H, W));
    const int slots = al1_slots(B, H * W);
    const unsigned nb = nblk((long long)B * H * W);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(al1_fwd_kernel, dim3(nb), dim3(256), 0, s, B, H, W, boundary_ignore, slots, pred, flow, c_mat,
                       valid, gt, g_pw, (float*)workspace);
    DBSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(al1_finish_kernel, dim3(stats ? 1 + B : 1), dim3(256), 0, s, (int)nb, H * W, slots,
                       (const float*)workspace, weight, loss, stats);
    DBSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int dbsr_aligned_l1_backward(int B, int H, int W, const float* pred, const float* flow, const float* g_pw,
                                        const float* c_mat, const float* scale, float* gpred, dbsr_tensor dpre,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    DBSR_CHECK_ARG(g_pw && (gpred || dpre.ptr), "aligned_l1_backward: null pointer (g_pw, and gpred or dpre)");
    DBSR_CHECK_ARG(B > 0 && H > 0 && W > 0 && (long long)B * H * W < (1LL << 31),
                   "aligned_l1_backward: bad sizes (B * H * W must be < 2^31)");
    if (dpre.ptr) {
        DBSR_CHECK_ARG(pred, "aligned_l1_backward: dpre needs pred (the ReLU gate)");
        DBSR_CHECK_ARG(dpre.map.fpg > 0 && dpre.ld >= dpre.c0 + 3, "aligned_l1_backward: bad dpre");
        DBSR_CHECK_ARG(dpre.dtype == DBSR_F32 || dpre.dtype == DBSR_BF16 || dpre.dtype == DBSR_F16,
                       "aligned_l1_backward: unsupported dtype %d", dpre.dtype);
    }
    hipStream_t s = (hipStream_t)stream;
    const long long total = (long long)B * H * W;
    const float* src = g_pw;
    if (flow) {
        DBSR_CHECK_ARG(workspace && workspace_bytes >= al1_bwd_bytes(B, H, W),
                       "aligned_l1_backward: workspace %zu < %zu bytes", workspace_bytes, al1_bwd_bytes(B, H, W));
        DBSR_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "aligned_l1_backward: workspace must be 16-B aligned");
        const long long n4 = (long long)(al1_bwd_bytes(B, H, W) / 16);
        hipLaunchKernelGGL(al1_zero_kernel, dim3(nblk(n4)), dim3(256), 0, s, n4, (float4*)workspace);
        hipLaunchKernelGGL(al1_scatter_kernel, dim3(nblk(total)), dim3(256), 0, s, B, H, W, flow, g_pw, c_mat,
                           (float*)workspace);
        DBSR_LAUNCH_CHECK();
        src = (const float*)workspace;
    }
    const float* cm = flow ? nullptr : c_mat;                 // (with a flow the scatter applied C)
    const bool v8 = dpre.ptr && dpre.dtype != DBSR_F32 && dpre.ld == 8 && dpre.c0 == 0;
    const dim3 grid(nblk(total));
    if (!dpre.ptr || dpre.dtype == DBSR_F32)
        hipLaunchKernelGGL((al1_out_kernel<float, false>), grid, dim3(256), 0, s, B, H, W, pred, src, cm, scale, gpred, dpre);
    else if (dpre.dtype == DBSR_BF16 && v8)
        hipLaunchKernelGGL((al1_out_kernel<bf16_t, true>), grid, dim3(256), 0, s, B, H, W, pred, src, cm, scale, gpred, dpre);
    else if (dpre.dtype == DBSR_BF16)
        hipLaunchKernelGGL((al1_out_kernel<bf16_t, false>), grid, dim3(256), 0, s, B, H, W, pred, src, cm, scale, gpred, dpre);
    else if (v8)
        hipLaunchKernelGGL((al1_out_kernel<f16_t, true>), grid, dim3(256), 0, s, B, H, W, pred, src, cm, scale, gpred, dpre);
    else
        hipLaunchKernelGGL((al1_out_kernel<f16_t, false>), grid, dim3(256), 0, s, B, H, W, pred, src, cm, scale, gpred, dpre);
    DBSR_LAUNCH_CHECK();
    return 0;
}
