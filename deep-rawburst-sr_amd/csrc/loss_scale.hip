// Dynamic loss scaling for 16-bit training (torch.amp.GradScaler's rule), entirely on the device: the training
// step reads nothing back to the host and replays as HIP graphs, so the scale, the overflow flag, the skip
// decision and Adam's step number all live in one small state buffer (dbsr_hip.h, DBSR_LS_*) that these
// kernels read and write.  Four ops, in step order:
//   dbsr_l1_loss_backward_scaled  dbsr_l1_loss_backward with dpre multiplied by state.scale (the loss stays
//                                 unscaled): 1/count ~ 4.7e-8 at configs[3] is below fp16's smallest subnormal
//   dbsr_grad_unscale_check       g *= 1/scale over the flat fp32 gradients, found_inf |= any inf / NaN
//   dbsr_adam_step_guarded        dbsr_adam_step unless found_inf; bias corrections from state.adam_step + 1
//   dbsr_loss_scale_update        back off / grow the scale, count the step or the skip, clear found_inf
#include "common.hpp"

#include <type_traits>

using namespace dbsr;

namespace {

inline unsigned nblocks(long long total, int bs) { return (unsigned)((total + bs - 1) / bs); }
bool map_ok(const dbsr_tensor& t) { return t.ptr && t.map.fpg > 0; }

__device__ __forceinline__ float ls_scale(const void* state) { return ((const float*)state)[DBSR_LS_SCALE]; }

// ------------------------------------------------------------------------------------------------
// l1_loss_bwd_kernel / l1_loss_bwd8_kernel of train_ops.hip with the gradient's magnitude inv_count * scale
// (scale from the state buffer; inv_count * 1.0f is inv_count, so scale 1 is bitwise the unscaled op).
// The |pred - gt| partial sums, and so the loss, do not see the scale.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void l1_scaled_kernel(int B, int C, int H, int W, int bi,
                                                        const float* __restrict__ pred, const float* __restrict__ gt,
                                                        float inv_count, const void* __restrict__ state,
                                                        dbsr_tensor dpre, float* __restrict__ partial) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)B * H * W;
    const float mag = inv_count * ls_scale(state);
    float s = 0.f;
    if (idx < total) {
        const int b = (int)(idx / ((long long)H * W));
        const int rr = (int)(idx - (long long)b * H * W);
        const int y = rr / W, x = rr - y * W;
        const bool in = y >= bi && y < H - bi && x >= bi && x < W - bi;
        T* o = img_ptr<T>(dpre, b) + (long long)rr * dpre.ld;
        for (int c = 0; c < C; ++c) {
            const long long off = ((long long)b * C + c) * H * W + rr;
            const float d = pred[off] - gt[off];
            float gv = 0.f;
            if (in) {
                s += fabsf(d);
                gv = pred[off] > 0.f ? (d > 0.f ? mag : (d < 0.f ? -mag : 0.f)) : 0.f;
            }
            elem<T>::st(o + c, gv);
        }
    }
    __shared__ float red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// 16-bit dpre with exactly 8 channels per pixel (c0 0, C <= 8): 4 pixels per thread, one 16-B store per pixel
template <typename T>
__global__ __launch_bounds__(256) void l1_scaled8_kernel(int B, int C, int H, int W, int bi,
                                                         const float* __restrict__ pred, const float* __restrict__ gt,
                                                         float inv_count, const void* __restrict__ state,
                                                         dbsr_tensor dpre, float* __restrict__ partial) {
    const long long total = (long long)B * H * W;
    const long long hw = (long long)H * W;
    const float mag = inv_count * ls_scale(state);
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long long idx = ((long long)blockIdx.x * 4 + u) * 256 + threadIdx.x;
        if (idx >= total) break;
        const int b = (int)(idx / hw);
        const int rr = (int)(idx - (long long)b * hw);
        const int y = rr / W, x = rr - y * W;
        const bool in = y >= bi && y < H - bi && x >= bi && x < W - bi;
        float gv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < C; ++c) {
            const long long off = ((long long)b * C + c) * hw + rr;
            const float pv = pred[off], d = pv - gt[off];
            if (in) {
                s += fabsf(d);
                gv[c] = pv > 0.f ? (d > 0.f ? mag : (d < 0.f ? -mag : 0.f)) : 0.f;
            }
        }
        store8(img_ptr<T>(dpre, b) + (long long)rr * 8, gv);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// the loss from the blocks' partial sums, in train_ops.hip's sum_all_kernel order (bitwise its result)
__global__ __launch_bounds__(256) void l1_finish_kernel(int n, const float* __restrict__ partial,
                                                        float* __restrict__ out, float scale) {
    float s = 0.f;
#pragma unroll 8
    for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
    __shared__ float red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0] * scale;
}

// ------------------------------------------------------------------------------------------------
// g *= 1 / scale in place, found_inf |= any product that is inf or NaN (exponent bits all ones; an inf or NaN
// gradient stays one under the multiply, and a product that overflows is one too).  HBM-bound, 8 B per
// element: 16-B loads and stores over the 16-B aligned body, grid-stride; the (up to 3) elements before the
// first aligned address and after the last whole vector go to block 0's first threads.  One atomic OR per
// block that saw a bad value, none otherwise.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(256) void unscale_check_kernel(long long n, float* g, long long head, long long nvec,
                                                            void* state) {
    const float inv = 1.0f / ls_scale(state);
    unsigned bad = 0;
    float4* body = (float4*)(g + head);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long long)gridDim.x * 256) {
        float4 v = body[i];
        v.x *= inv;
        v.y *= inv;
        v.z *= inv;
        v.w *= inv;
        bad |= nonfinite(v.x) | nonfinite(v.y) | nonfinite(v.z) | nonfinite(v.w);
        body[i] = v;
    }
    if (blockIdx.x == 0) {
        // scalar ends: [0, head) and [head + 4 nvec, n), at most 3 elements each
        const long long tail0 = head + 4 * nvec;
        const long long ends = head + (n - tail0);
        if ((long long)threadIdx.x < ends) {
            const long long i = (long long)threadIdx.x < head ? (long long)threadIdx.x : tail0 + (threadIdx.x - head);
            const float v = g[i] * inv;
            bad |= nonfinite(v);
            g[i] = v;
        }
    }
    if (__syncthreads_or((int)bad) && threadIdx.x == 0) atomicOr((int*)state + DBSR_LS_FOUND_INF, 1);
}

// ------------------------------------------------------------------------------------------------
// adam_kernel of train_ops.hip (torch.optim.Adam, weight_decay 0, amsgrad False), skipped whole when the
// step's gradients overflowed, with t = state.adam_step + 1 in the bias corrections: a skipped step does not
// advance t (torch.amp.GradScaler.step does not call optimizer.step then).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adam_guarded_kernel(long long n, float* __restrict__ p,
                                                           const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, float lr, float b1, float b2,
                                                           float eps, float gscale, const void* __restrict__ state) {
    const int* si = (const int*)state;
    if (si[DBSR_LS_FOUND_INF] != 0) return;                    // (block-uniform: before the barrier is fine)
    __shared__ float bc[2];
    if (threadIdx.x == 0) {
        const float t = (float)(si[DBSR_LS_ADAM_STEP] + 1);
        bc[0] = 1.f - powf(b1, t);
        bc[1] = sqrtf(1.f - powf(b2, t));
    }
    __syncthreads();
    const float bc1 = bc[0], bc2_sqrt = bc[1];
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i] * gscale;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    // torch: p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)
    p[i] -= (lr / bc1) * mi / (sqrtf(vi) / bc2_sqrt + eps);
}

// torch.amp.GradScaler.update (grad_scaler.py: _amp_update_scale_), one thread
__global__ void loss_scale_update_kernel(void* state, float growth, float backoff, int interval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float* sf = (float*)state;
    int* si = (int*)state;
    if (si[DBSR_LS_FOUND_INF] != 0) {
        sf[DBSR_LS_SCALE] *= backoff;
        si[DBSR_LS_GROWTH_TRACKER] = 0;
        si[DBSR_LS_SKIPPED] += 1;
    } else {
        si[DBSR_LS_ADAM_STEP] += 1;
        const int tr = si[DBSR_LS_GROWTH_TRACKER] + 1;
        if (tr == interval) {
            sf[DBSR_LS_SCALE] *= growth;
            si[DBSR_LS_GROWTH_TRACKER] = 0;
        } else {
            si[DBSR_LS_GROWTH_TRACKER] = tr;
        }
    }
    si[DBSR_LS_FOUND_INF] = 0;
}

}  // namespace

// ================================================================================================
extern "C" int dbsr_l1_loss_backward_scaled(int B, int C, int H, int W, int boundary_ignore, const float* pred,
                                            const float* gt, const void* state, dbsr_tensor dpre, float* loss,
                                            void* workspace, size_t workspace_bytes, void* stream) {
    DBSR_CHECK_ARG(pred && gt && state && loss && workspace && map_ok(dpre), "l1_loss_backward_scaled: null pointer");
    DBSR_CHECK_ARG(B > 0 && C > 0 && H > 2 * boundary_ignore && W > 2 * boundary_ignore && boundary_ignore >= 0 &&
                   dpre.ld >= dpre.c0 + C, "l1_loss_backward_scaled: bad sizes");
    const long long total = (long long)B * H * W;
    const unsigned nb = nblocks(total, 256);
    DBSR_CHECK_ARG(workspace_bytes >= nb * sizeof(float), "l1_loss_backward_scaled: workspace < %u floats", nb);
    const float count = (float)B * C * (H - 2 * boundary_ignore) * (W - 2 * boundary_ignore);
    hipStream_t s = (hipStream_t)stream;
    const bool v8 = dpre.dtype != DBSR_F32 && dpre.ld == 8 && dpre.c0 == 0 && C <= 8;
    const unsigned nb8 = nblocks(total, 1024);            // 4 pixels per thread
    auto launch = [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        if constexpr (sizeof(T) == 2) {
            if (v8) {
                hipLaunchKernelGGL((l1_scaled8_kernel<T>), dim3(nb8), dim3(256), 0, s, B, C, H, W, boundary_ignore,
                                   pred, gt, 1.0f / count, state, dpre, (float*)workspace);
                DBSR_LAUNCH_CHECK();
                return 0;
            }
        }
        hipLaunchKernelGGL((l1_scaled_kernel<T>), dim3(nb), dim3(256), 0, s, B, C, H, W, boundary_ignore, pred, gt,
                           1.0f / count, state, dpre, (float*)workspace);
        DBSR_LAUNCH_CHECK();
        return 0;
    };
    int rc;
    if (dpre.dtype == DBSR_BF16) rc = launch((bf16_t*)nullptr);
    else if (dpre.dtype == DBSR_F16) rc = launch((f16_t*)nullptr);
    else if (dpre.dtype == DBSR_F32) rc = launch((float*)nullptr);
    else DBSR_CHECK_ARG(false, "l1_loss_backward_scaled: unsupported dtype %d", dpre.dtype);
    if (rc) return rc;
    hipLaunchKernelGGL(l1_finish_kernel, dim3(1), dim3(256), 0, s, (int)(v8 ? nb8 : nb), (const float*)workspace, loss,
                       1.0f / count);
    DBSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int dbsr_grad_unscale_check(long long n, float* grad, void* state, void* stream) {
    DBSR_CHECK_ARG(grad && state, "grad_unscale_check: null pointer");
    DBSR_CHECK_ARG(n > 0, "grad_unscale_check: n must be > 0");
    DBSR_CHECK_ARG(((uintptr_t)grad & 3) == 0, "grad_unscale_check: grad must be 4-B aligned");
    long long head = (long long)(((16 - ((uintptr_t)grad & 15)) & 15) / 4);      // floats before the 16-B boundary
    if (head > n) head = n;
    const long long nvec = (n - head) / 4;
    // grid-stride: at most 8 blocks of 256 threads per CU of the 256 (each thread then has several 16-B pieces)
    long long blocks = (nvec + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(unscale_check_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, n, grad, head,
                       nvec, state);
    DBSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int dbsr_adam_step_guarded(long long n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                      float lr, float beta1, float beta2, float eps, float grad_scale,
                                      const void* state, void* stream) {
    DBSR_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && state, "adam_step_guarded: null pointer");
    DBSR_CHECK_ARG(n > 0, "adam_step_guarded: n must be > 0");
    hipLaunchKernelGGL(adam_guarded_kernel, dim3(nblocks(n, 256)), dim3(256), 0, (hipStream_t)stream, n, param, grad,
                       exp_avg, exp_avg_sq, lr, beta1, beta2, eps, grad_scale, state);
    DBSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int dbsr_loss_scale_update(void* state, float growth_factor, float backoff_factor, int growth_interval,
                                      void* stream) {
    DBSR_CHECK_ARG(state, "loss_scale_update: null pointer");
    DBSR_CHECK_ARG(growth_factor > 0.f && backoff_factor > 0.f, "loss_scale_update: factors must be > 0");
    DBSR_CHECK_ARG(growth_interval >= 1, "loss_scale_update: growth_interval must be >= 1");
    hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, growth_factor,
                       backoff_factor, growth_interval);
    DBSR_LAUNCH_CHECK();
    return 0;
}
