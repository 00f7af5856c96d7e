// Objectives of the fused training step (models/loss/image_quality_v2.py:24-101): PixelWiseError's four metrics
// with their gradients, the per-image squared-error statistics PSNR needs, PSNR itself, and the predictor's ReLU
// gate of an upstream gradient under a loss scale.  HBM-bound fp32 VALU kernels: plain loads, vector stores, no
// atomics, nothing read back.  Every sum goes through per-block partials in the workspace and one finishing
// block that adds them in a fixed order, so two runs are bitwise equal.
//   dbsr_objective_step      pred, gt -> the ReLU-gated NHWC dpre of the predictor's backward (both layouts of
//                            dbsr_l1_loss_backward), the raw and the weighted loss, per-image {sum d^2, count}
//   dbsr_objective_forward   the same losses with an optional validity mask and an unnormalised fp32 NCHW gradient
//                            (the count is a sum over the mask: the scale is a device scalar, as dbsr_aligned_l1_*)
//   dbsr_psnr_from_stats     per-image PSNR from those statistics, inf / NaN images dropped, then the mean
//   dbsr_relu_grad_scaled    dbsr_relu_grad times the loss-scale state's scale
#include "common.hpp"

#include <type_traits>

using namespace dbsr;

namespace {

inline unsigned nblocks(long long total, int bs) { return (unsigned)((total + bs - 1) / bs); }
bool map_ok(const dbsr_tensor& t) { return t.ptr && t.map.fpg > 0; }

constexpr float CHARB_EPS2 = 1e-6f;               // eps ** 2 with eps = 1e-3 (image_quality_v2.py:41-42)

// One pixel's three differences -> the metric's terms (term[c]; l2_sqrt has one term per pixel, in term[0]) and
// the unnormalised gradient m[c] = count * dmetric/dpred_c; sq = sum_c d_c^2.
__device__ __forceinline__ void metric_pixel(int metric, const float (&d)[3], float (&term)[3], float (&m)[3], float& sq) {
    sq = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    if (metric == DBSR_METRIC_L1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            term[c] = fabsf(d[c]);
            m[c] = d[c] > 0.f ? 1.f : (d[c] < 0.f ? -1.f : 0.f);
        }
    } else if (metric == DBSR_METRIC_L2) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            term[c] = d[c] * d[c];
            m[c] = 2.f * d[c];
        }
    } else if (metric == DBSR_METRIC_CHARBONNIER) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float r = sqrtf(d[c] * d[c] + CHARB_EPS2);
            term[c] = r;
            m[c] = d[c] / r;
        }
    } else {                                       // l2_sqrt: the gradient is 0 where the norm is 0
        const float n = sqrtf(sq);
        term[0] = n;
        term[1] = term[2] = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = n > 0.f ? d[c] / n : 0.f;
    }
}

// Block sums of two doubles (256 threads: wave shuffles, then the four waves in order); valid in thread 0.
__device__ __forceinline__ void block_sum2(double& a, double& b, double (*red)[2]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    __syncthreads();                               // (the previous round's reads of red are done)
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][0] = a;
        red[threadIdx.x >> 6][1] = b;
    }
    __syncthreads();
    a = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    b = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
}

// Workspace of one call (host and device agree through this struct): nb blocks of `pix` pixels, ns image slots per
// block (a block of consecutive pixels of the flat [B][H][W] index touches at most ns images).
struct Layout {
    int nb, pix, ns;
    size_t off_d, off_s, bytes;                    // float part[nb] at 0; double dpart[nb]; double spart[nb][ns][2]
};
inline Layout layout(int B, long long hw, int pix) {
    Layout l;
    const long long total = (long long)B * hw;
    l.pix = pix;
    l.nb = (int)((total + pix - 1) / pix);
    long long ns = (pix - 1) / hw + 2;
    l.ns = (int)(ns < B ? ns : B);
    l.off_d = ((size_t)l.nb * sizeof(float) + 15) & ~(size_t)15;
    l.off_s = l.off_d + (((size_t)l.nb * sizeof(double) + 15) & ~(size_t)15);
    l.bytes = l.off_s + (size_t)l.nb * l.ns * 2 * sizeof(double);
    return l;
}

// ------------------------------------------------------------------------------------------------
// The step op.  PPT 1: one pixel per thread, 256 per block, channels [c0, c0 + 3) of dpre written one by one
// (l1_loss_bwd_kernel's layout and float sum order).  PPT 4: 16-bit dpre with ld 8, c0 0 -- four pixels per thread,
// one 16-B store per pixel with channels 3..7 zero (l1_loss_bwd8_kernel's).  fpart: the metric's terms summed in
// float exactly as those kernels sum |d| (the l1 loss is bitwise theirs); dpart: the same terms in double (the
// other metrics' loss); spart: per image slot {sum d^2, pixels} over the crop.
// ------------------------------------------------------------------------------------------------
template <typename T, int PPT>
__global__ __launch_bounds__(256) void objective_step_kernel(int B, int H, int W, int bi, int metric, float wic,
                                                             const float* __restrict__ pred,
                                                             const float* __restrict__ gt,
                                                             const float* __restrict__ gextra,
                                                             const void* __restrict__ state, dbsr_tensor dpre,
                                                             int ns, float* __restrict__ fpart,
                                                             double* __restrict__ dpart, double* __restrict__ spart) {
    const long long hw = (long long)H * W;
    const long long total = (long long)B * hw;
    const float scale = state ? ((const float*)state)[DBSR_LS_SCALE] : 1.0f;
    const float mag = wic * scale;
    const long long first = (long long)blockIdx.x * (256 * PPT);
    const int b0 = (int)(first / hw);
    long long last = first + 256 * PPT - 1;
    if (last > total - 1) last = total - 1;
    const int nslot = (int)(last / hw) - b0 + 1;   // block-uniform, <= ns
    float s = 0.f;
    double sd = 0.0;
    float psq[PPT];
    int pslot[PPT];
#pragma unroll
    for (int u = 0; u < PPT; ++u) {
        psq[u] = 0.f;
        pslot[u] = -1;
    }
#pragma unroll
    for (int u = 0; u < PPT; ++u) {
        const long long idx = first + (long long)u * 256 + threadIdx.x;
        if (idx >= total) break;
        const int b = (int)(idx / hw);
        const int rr = (int)(idx - (long long)b * hw);
        const int y = rr / W, x = rr - y * W;
        const bool in = y >= bi && y < H - bi && x >= bi && x < W - bi;
        float pv[3], d[3], term[3], m[3], sq;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long long off = ((long long)b * 3 + c) * hw + rr;
            pv[c] = pred[off];
            d[c] = pv[c] - gt[off];
        }
        metric_pixel(metric, d, term, m, sq);
        float gv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (in) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                s += term[c];
                sd += (double)term[c];
                float g = m[c] * mag;
                if (gextra) g += gextra[((long long)b * 3 + c) * hw + rr] * scale;
                gv[c] = pv[c] > 0.f ? g : 0.f;
            }
            psq[u] = sq;
            pslot[u] = b - b0;
        }
        if constexpr (PPT == 4) {
            store8(img_ptr<T>(dpre, b) + (long long)rr * 8, gv);
        } else {
            T* o = img_ptr<T>(dpre, b) + (long long)rr * dpre.ld;
#pragma unroll
            for (int c = 0; c < 3; ++c) elem<T>::st(o + c, gv[c]);
        }
    }
    // the float sum, in the order of the l1 kernels
    if constexpr (PPT == 4) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        __shared__ float red4[4];
        if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) fpart[blockIdx.x] = red4[0] + red4[1] + red4[2] + red4[3];
    } else {
        __shared__ float red[256];
        red[threadIdx.x] = s;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
            __syncthreads();
        }
        if (threadIdx.x == 0) fpart[blockIdx.x] = red[0];
    }
    __shared__ double dred[4][2];
    double zero = 0.0;
    block_sum2(sd, zero, dred);
    if (threadIdx.x == 0) dpart[blockIdx.x] = sd;
    for (int k = 0; k < nslot; ++k) {
        double a = 0.0, n = 0.0;
#pragma unroll
        for (int u = 0; u < PPT; ++u)
            if (pslot[u] == k) {
                a += (double)psq[u];
                n += 1.0;
            }
        block_sum2(a, n, dred);
        if (threadIdx.x == 0) {
            double* o = spart + ((long long)blockIdx.x * ns + k) * 2;
            o[0] = a;
            o[1] = n;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The forward form: optional mask, the unnormalised gradient valid * m as fp32 NCHW (g NULL: none), every element
// written (zero outside the crop).  One pixel per thread; the loss terms in double only.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void objective_fwd_kernel(int B, int H, int W, int bi, int metric,
                                                            const float* __restrict__ pred,
                                                            const float* __restrict__ gt,
                                                            const unsigned char* __restrict__ valid,
                                                            float* __restrict__ g, int ns, double* __restrict__ dpart,
                                                            double* __restrict__ spart) {
    const long long hw = (long long)H * W;
    const long long total = (long long)B * hw;
    const long long first = (long long)blockIdx.x * 256;
    const int b0 = (int)(first / hw);
    long long last = first + 255;
    if (last > total - 1) last = total - 1;
    const int nslot = (int)(last / hw) - b0 + 1;
    const long long idx = first + threadIdx.x;
    double sd = 0.0;
    float psq = 0.f;
    int pslot = -1;
    if (idx < total) {
        const int b = (int)(idx / hw);
        const int rr = (int)(idx - (long long)b * hw);
        const int y = rr / W, x = rr - y * W;
        bool in = y >= bi && y < H - bi && x >= bi && x < W - bi;
        if (in && valid) in = valid[idx] != 0;
        float d[3], term[3], m[3], sq;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long long off = ((long long)b * 3 + c) * hw + rr;
            d[c] = pred[off] - gt[off];
        }
        metric_pixel(metric, d, term, m, sq);
        if (in) {
#pragma unroll
            for (int c = 0; c < 3; ++c) sd += (double)term[c];
            psq = sq;
            pslot = b - b0;
        }
        if (g) {
#pragma unroll
            for (int c = 0; c < 3; ++c) g[((long long)b * 3 + c) * hw + rr] = in ? m[c] : 0.f;
        }
    }
    __shared__ double dred[4][2];
    double zero = 0.0;
    block_sum2(sd, zero, dred);
    if (threadIdx.x == 0) dpart[blockIdx.x] = sd;
    for (int k = 0; k < nslot; ++k) {
        double a = pslot == k ? (double)psq : 0.0, n = pslot == k ? 1.0 : 0.0;
        block_sum2(a, n, dred);
        if (threadIdx.x == 0) {
            double* o = spart + ((long long)blockIdx.x * ns + k) * 2;
            o[0] = a;
            o[1] = n;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// One block finishes: loss[0] = the raw loss, loss[1] = weight * loss[0], loss[2] = weight / denominator (the
// gradient's scale); stats[b] = {sum d^2, elements} of image b in double.  fpart (the unmasked l1 of the step op):
// the float partials in sum_all_kernel's order times inv_count, bitwise dbsr_l1_loss_backward's loss; else the
// double partials over the denominator: count, or masked elems * sum(valid) + 1e-12.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void objective_finish_kernel(int nb, int B, long long hw, int pix, int ns, int elems,
                                                               int masked, float weight, float inv_count, double count,
                                                               const float* __restrict__ fpart,
                                                               const double* __restrict__ dpart,
                                                               const double* __restrict__ spart,
                                                               float* __restrict__ loss, double* __restrict__ stats) {
    __shared__ float red[256];
    __shared__ double dred[256];
    float fs = 0.f;
    if (fpart) {
#pragma unroll 8
        for (int i = threadIdx.x; i < nb; i += 256) fs += fpart[i];
    }
    double ds = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) ds += dpart[i];
    red[threadIdx.x] = fs;
    dred[threadIdx.x] = ds;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            red[threadIdx.x] += red[threadIdx.x + st];
            dred[threadIdx.x] += dred[threadIdx.x + st];
        }
        __syncthreads();
    }
    // per-image statistics: a wave per image, its lanes over the image's blocks, then the lanes in a fixed order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = wave; b < B; b += 4) {
        const long long k0 = ((long long)b * hw) / pix, k1 = ((long long)(b + 1) * hw - 1) / pix;
        double a = 0.0, n = 0.0;
        for (long long k = k0 + lane; k <= k1; k += 64) {
            const int slot = b - (int)((k * pix) / hw);
            const double* p = spart + (k * ns + slot) * 2;
            a += p[0];
            n += p[1];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a += __shfl_xor(a, o, 64);
            n += __shfl_xor(n, o, 64);
        }
        if (lane == 0) {
            stats[2 * b] = a;
            stats[2 * b + 1] = n * 3.0;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double denom = count;
        if (masked) {
            double nv = 0.0;
            for (int b = 0; b < B; ++b) nv += stats[2 * b + 1];
            denom = nv * (elems / 3.0) + 1e-12;
        }
        const float raw = (fpart && !masked) ? red[0] * inv_count : (float)(dred[0] / denom);
        loss[0] = raw;
        loss[1] = weight * raw;
        loss[2] = masked ? (float)((double)weight / denom) : weight * inv_count;
    }
}

// PSNR(boundary_ignore, max_value) of image_quality_v2.py:69-101 from stats: one thread, B values.
__global__ void psnr_kernel(int B, const double* __restrict__ stats, int masked, float max_value,
                            const float* __restrict__ max_values, float* __restrict__ out,
                            float* __restrict__ per_image) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double sum = 0.0;
    int kept = 0;
    for (int b = 0; b < B; ++b) {
        const double mse = stats[2 * b] / (stats[2 * b + 1] + (masked ? 1e-12 : 0.0));
        const double mv = max_values ? (double)max_values[b] : (double)max_value;
        const float v = (float)(20.0 * log10(mv) - 10.0 * log10(mse));
        if (per_image) per_image[b] = v;
        if ((__float_as_uint(v) & 0x7f800000u) != 0x7f800000u) {      // neither inf nor NaN
            sum += (double)v;
            ++kept;
        }
    }
    out[0] = kept ? (float)(sum / kept) : 0.f;
}

template <typename T>
__global__ __launch_bounds__(256) void relu_grad_scaled_kernel(int B, int C, int H, int W,
                                                               const float* __restrict__ pred,
                                                               const float* __restrict__ gout,
                                                               const void* __restrict__ state, dbsr_tensor dpre) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)B * H * W) return;
    const float scale = ((const float*)state)[DBSR_LS_SCALE];
    const int b = (int)(idx / ((long long)H * W));
    const int rr = (int)(idx - (long long)b * H * W);
    T* o = img_ptr<T>(dpre, b) + (long long)rr * dpre.ld;
    for (int c = 0; c < C; ++c) {
        const long long off = ((long long)b * C + c) * H * W + rr;
        elem<T>::st(o + c, pred[off] > 0.f ? gout[off] * scale : 0.f);
    }
}

bool metric_ok(int metric) { return metric >= DBSR_METRIC_L1 && metric <= DBSR_METRIC_CHARBONNIER; }

template <class F>
int by_dtype3(int dtype, F&& f) {
    if (dtype == DBSR_BF16) return f((bf16_t*)nullptr);
    if (dtype == DBSR_F16) return f((f16_t*)nullptr);
    return f((float*)nullptr);
}

}  // namespace

// ================================================================================================
// one size for every call: the larger of the two block decompositions
static size_t workspace_need(int B, long long hw) {
    const Layout a = layout(B, hw, 256), b = layout(B, hw, 1024);
    return a.bytes > b.bytes ? a.bytes : b.bytes;
}

extern "C" size_t dbsr_objective_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return workspace_need(B, (long long)H * W);
}

extern "C" int dbsr_objective_step(int B, int H, int W, int boundary_ignore, int metric, float weight,
                                   const float* pred, const float* gt, const float* gextra, const void* state,
                                   dbsr_tensor dpre, float* loss, double* stats, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    DBSR_CHECK_ARG(pred && gt && loss && stats && workspace && map_ok(dpre), "objective_step: null pointer");
    DBSR_CHECK_ARG(metric_ok(metric), "objective_step: unknown metric code %d", metric);
    DBSR_CHECK_ARG(B > 0 && boundary_ignore >= 0 && H > 2 * boundary_ignore && W > 2 * boundary_ignore &&
                   dpre.ld >= dpre.c0 + 3 && dpre.c0 >= 0, "objective_step: bad sizes");
    DBSR_CHECK_ARG((long long)H * W < (1ll << 31) && (long long)B * 3 * H * W < (1ll << 40),
                   "objective_step: too many elements");
    DBSR_CHECK_ARG(dpre.dtype == DBSR_F32 || dpre.dtype == DBSR_BF16 || dpre.dtype == DBSR_F16,
                   "objective_step: unsupported dtype %d", dpre.dtype);
    const bool v8 = dpre.dtype != DBSR_F32 && dpre.ld == 8 && dpre.c0 == 0;
    const size_t esz = dpre.dtype == DBSR_F32 ? 4 : 2;
    DBSR_CHECK_ARG(((uintptr_t)dpre.ptr % (v8 ? 16 : esz)) == 0 && (!v8 || dpre.img_stride % 8 == 0),
                   "objective_step: dpre is misaligned (%d B needed)", v8 ? 16 : (int)esz);
    const long long hw = (long long)H * W;
    const Layout l = layout(B, hw, v8 ? 1024 : 256);
    DBSR_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && workspace_bytes >= workspace_need(B, hw),
                   "objective_step: workspace < %zu bytes or not 16-B aligned", workspace_need(B, hw));
    const int hc = H - 2 * boundary_ignore, wc = W - 2 * boundary_ignore;
    // (the float product of dbsr_l1_loss_backward: its 1 / count is the l1 gradient's magnitude, bit for bit)
    const float count = metric == DBSR_METRIC_L2_SQRT ? (float)B * hc * wc : (float)B * 3 * hc * wc;
    const float inv_count = 1.0f / count;
    hipStream_t s = (hipStream_t)stream;
    float* fpart = (float*)workspace;
    double* dpart = (double*)((char*)workspace + l.off_d);
    double* spart = (double*)((char*)workspace + l.off_s);
    int rc = by_dtype3(dpre.dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        if constexpr (sizeof(T) == 2) {
            if (v8) {
                hipLaunchKernelGGL((objective_step_kernel<T, 4>), dim3((unsigned)l.nb), dim3(256), 0, s, B, H, W,
                                   boundary_ignore, metric, weight * inv_count, pred, gt, gextra, state, dpre, l.ns,
                                   fpart, dpart, spart);
                DBSR_LAUNCH_CHECK();
                return 0;
            }
        }
        hipLaunchKernelGGL((objective_step_kernel<T, 1>), dim3((unsigned)l.nb), dim3(256), 0, s, B, H, W,
                           boundary_ignore, metric, weight * inv_count, pred, gt, gextra, state, dpre, l.ns, fpart,
                           dpart, spart);
        DBSR_LAUNCH_CHECK();
        return 0;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(objective_finish_kernel, dim3(1), dim3(256), 0, s, l.nb, B, hw, l.pix, l.ns, 3, 0, weight,
                       inv_count, (double)count, metric == DBSR_METRIC_L1 ? (const float*)fpart : (const float*)nullptr,
                       (const double*)dpart, (const double*)spart, loss, stats);
    DBSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int dbsr_objective_forward(int B, int H, int W, int boundary_ignore, int metric, float weight,
                                      const float* pred, const float* gt, const unsigned char* valid, float* g,
                                      float* loss, double* stats, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    DBSR_CHECK_ARG(pred && gt && loss && stats && workspace, "objective_forward: null pointer");
    DBSR_CHECK_ARG(metric_ok(metric), "objective_forward: unknown metric code %d", metric);
    DBSR_CHECK_ARG(!valid || metric == DBSR_METRIC_L1 || metric == DBSR_METRIC_L2,
                   "objective_forward: a mask goes with l1 and l2 only (metric code %d)", metric);
    DBSR_CHECK_ARG(B > 0 && boundary_ignore >= 0 && H > 2 * boundary_ignore && W > 2 * boundary_ignore,
                   "objective_forward: bad sizes");
    DBSR_CHECK_ARG((long long)H * W < (1ll << 31) && (long long)B * 3 * H * W < (1ll << 40),
                   "objective_forward: too many elements");
    const long long hw = (long long)H * W;
    const Layout l = layout(B, hw, 256);
    DBSR_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && workspace_bytes >= workspace_need(B, hw),
                   "objective_forward: workspace < %zu bytes or not 16-B aligned", workspace_need(B, hw));
    const int hc = H - 2 * boundary_ignore, wc = W - 2 * boundary_ignore;
    const float count = metric == DBSR_METRIC_L2_SQRT ? (float)B * hc * wc : (float)B * 3 * hc * wc;
    hipStream_t s = (hipStream_t)stream;
    double* dpart = (double*)((char*)workspace + l.off_d);
    double* spart = (double*)((char*)workspace + l.off_s);
    hipLaunchKernelGGL(objective_fwd_kernel, dim3((unsigned)l.nb), dim3(256), 0, s, B, H, W, boundary_ignore, metric,
                       pred, gt, valid, g, l.ns, dpart, spart);
    DBSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(objective_finish_kernel, dim3(1), dim3(256), 0, s, l.nb, B, hw, l.pix, l.ns, 3, valid ? 1 : 0,
                       weight, 1.0f / count, (double)count, (const float*)nullptr, (const double*)dpart,
                       (const double*)spart, loss, stats);
    DBSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int dbsr_psnr_from_stats(int B, const double* stats, int masked, float max_value, const float* max_values,
                                    float* out, float* per_image, void* stream) {
    DBSR_CHECK_ARG(stats && out, "psnr_from_stats: null pointer");
    DBSR_CHECK_ARG(B > 0, "psnr_from_stats: B must be > 0");
    DBSR_CHECK_ARG(max_values || max_value > 0.f, "psnr_from_stats: max_value must be > 0");
    hipLaunchKernelGGL(psnr_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, B, stats, masked ? 1 : 0, max_value,
                       max_values, out, per_image);
    DBSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int dbsr_relu_grad_scaled(int B, int C, int H, int W, const float* pred, const float* gout,
                                     const void* state, dbsr_tensor dpre, void* stream) {
    DBSR_CHECK_ARG(pred && gout && state && map_ok(dpre), "relu_grad_scaled: null pointer");
    DBSR_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && dpre.ld >= dpre.c0 + C && dpre.c0 >= 0,
                   "relu_grad_scaled: bad sizes");
    DBSR_CHECK_ARG(dpre.dtype == DBSR_F32 || dpre.dtype == DBSR_BF16 || dpre.dtype == DBSR_F16,
                   "relu_grad_scaled: unsupported dtype %d", dpre.dtype);
    return by_dtype3(dpre.dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        hipLaunchKernelGGL((relu_grad_scaled_kernel<T>), dim3(nblocks((long long)B * H * W, 256)), dim3(256), 0,
                           (hipStream_t)stream, B, C, H, W, pred, gout, state, dpre);
        DBSR_LAUNCH_CHECK();
        return 0;
    });
}
