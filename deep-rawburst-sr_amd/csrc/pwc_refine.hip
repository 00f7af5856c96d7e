// Fused tail of the PWC-Net refiner on the 16x16 level (pwcnet.py:186-207 + the residual flow of :231): refiner
// convs 1-6 (128 -> 128 d2, 128 -> 128 d4, 128 -> 96 d8, 96 -> 64 d16, 64 -> 32, 32 -> 2) in one launch.
//
// A pair's whole 16x16x128 image is 64 KiB, so it fits one CU's LDS and no conv of the chain needs a halo from
// another block: one 512-thread block owns one pair, keeps two ping-pong activation images in LDS (pwc_dense's
// pixel-row layout: +8 channels of row padding) and only weights cross memory between the input load and the flow
// store.  Each conv's LeakyReLU(conv + bias) is rounded to the storage dtype when it is written to LDS -- the
// storage points of the per-conv path -- and the last conv adds the level's flow (fp32) and stores fp32.
//
// Waves: a column tile is one image row (16 pixels); a wave owns MBW 16-cout blocks x R image rows, and every conv
// has exactly 8 such units (the 16 rows give enough parallelism that no conv splits K, so there is no reduction
// through LDS).  A-fragments stream from L2 (the chunk-major copy of dbsr_conv_pack_weights, one KiB per k-step)
// one (tap row, channel chunk) group ahead of their MFMAs; every A-fragment is used for R column tiles.
//
// Taps that read only zero padding are not issued: with dilation d on a 16-row image, tap row ky of output row y
// reads image row y + (ky - 1) d; where that lies outside the image for a wave's row (a compile-time fact given
// the wave's row group), neither the weights nor the MFMAs of that (tap row, row) are issued.  For d = 8 that is
// one of the three tap rows for every row, for d = 4 / 2 one for the outer 4 / 2 rows; d = 16 is the centre tap
// alone (packed as a 1x1 conv by the engine).  Out-of-image columns (and rows of the d = 1 convs) read a shared
// zero row.
#include "common.hpp"

#include <type_traits>

using namespace dbsr;

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bfv8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 hv8_t;

template <typename T>
__device__ __forceinline__ f32x4_t mma16x16x32(u32x4_t a, bf16x8_t b, f32x4_t c) {
    if constexpr (std::is_same<T, bf16_t>::value)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bfv8_t, a), __builtin_bit_cast(bfv8_t, b), c,
                                                       0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(hv8_t, a), __builtin_bit_cast(hv8_t, b), c,
                                                      0, 0, 0);
}

constexpr int RS = 16;                        // image size (rows = columns)
constexpr int PLD = 128 + 8;                  // LDS pixel row (elements): 128 channels + 8 of padding
constexpr int ROWE = RS * PLD;                // elements per image row
constexpr int IMG = RS * ROWE;                // elements per activation image
constexpr int ZERO_OFF = 2 * IMG;             // the shared zero row follows the two images
constexpr int SMEM_ELEMS = 2 * IMG + PLD;
static_assert(SMEM_ELEMS * 2 <= 160 * 1024, "pwc_refine: LDS");
static_assert((RS - 1 + RS) * ROWE < (1 << 30), "pwc_refine: offsets");

struct RefineConv {
    const void* w;          // packed weights: the chunk-major copy (3x3), the row layout (1x1)
    const float* bias;
};
struct RefineArgs {
    int P;
    dbsr_tensor x;          // [P][16][16][>= 128], 16-bit
    dbsr_tensor res;        // fp32 [P][16][16][>= 2]: the level's flow
    dbsr_tensor flow;       // fp32 [P][16][16][>= 2]
    RefineConv cv[6];
};

// One conv of the chain.  D: dilation (0: a 1x1 conv), CIN / COUT: channels, MBW x R: 16-cout blocks x image rows
// per wave, SKIP: dead (tap row, row) pairs are compile-time facts of the row group (YS: a row base with the row
// group's liveness) and are not issued, LAST: the flow conv.
template <int D_, int CIN_, int COUT_, int MBW_, int R_, bool SKIP_, bool LAST_>
struct ConvSpec {
    static constexpr int D = D_, CIN = CIN_, COUT = COUT_, MBW = MBW_, R = R_;
    static constexpr bool SKIP = SKIP_, LAST = LAST_;
    static constexpr int KT = D == 0 ? 1 : 3;                 // taps per side
    static constexpr int NCH = CIN / 32;                      // 32-channel chunks (k-steps per tap)
    static constexpr int MB = (COUT + 15) / 16;
    static constexpr int NRG = RS / R;                        // row groups
    static constexpr int NA = KT * MBW;                       // A-fragments per (tap row, chunk) group
    static_assert(CIN % 32 == 0 && (MB / MBW) * MBW == MB && (MB / MBW) * NRG == 8, "pwc_refine: 8 wave units");
    static constexpr bool BIG = NCH % 2 == 0 && NCH * KT * NA > 18;   // streamed group by group (else loaded up front)
};

__host__ __device__ constexpr bool row_live(int d, int ky, int y) { return y + (ky - 1) * d >= 0 && y + (ky - 1) * d < RS; }
// tap rows [ky0, ky1) that any of the R rows from ys reads inside the image
template <class S> __host__ __device__ constexpr bool ky_live(int ky, int ys) {
    if (!S::SKIP) return true;
    for (int r = 0; r < S::R; ++r)
        if (row_live(S::D, ky, ys + r)) return true;
    return false;
}

template <typename T> struct RefineCtx {
    T* smem;
    const RefineArgs* a;
    int lane, wave, g, col, pair;
};

template <class S, int YS, typename T>
__device__ __forceinline__ void refine_conv(const RefineCtx<T>& c, const RefineConv& cv, int in_off, int out_off) {
    constexpr int KT = S::KT, NCH = S::NCH, MBW = S::MBW, R = S::R, NA = S::NA, D = S::D;
    const int mg = c.wave / S::NRG, rg = c.wave - mg * S::NRG;
    const int m_first = mg * MBW, r0 = rg * R;
    constexpr int KY0 = KT == 1 ? 0 : (ky_live<S>(0, YS) ? 0 : 1);
    constexpr int KY1 = KT == 1 ? 1 : (ky_live<S>(2, YS) ? 3 : 2);
    constexpr int NKY = KY1 - KY0;

    // A-fragment of (16-cout block m_first + mi, chunk ch, tap): lane (g, col) holds row col, k = 8g .. 8g + 7
    auto a_ptr = [&](int mi, int ch, int tap) -> const T* {
        const int m0 = m_first + mi;
        if constexpr (D != 0) {
            // chunk-major copy [cout / 16][chunk][tap][4 k-groups][16 rows][8]: one contiguous KiB per k-step
            return (const T*)cv.w + (long long)((m0 * NCH + ch) * 9 + tap) * 512 + c.lane * 8;
        } else {
            // 1x1: the row layout [cout_pad][CIN], rows read in the copy's order (pipe_cout_perm), so every conv
            // has one epilogue
            const int co = 32 * (m0 >> 1) + 8 * (c.col >> 2) + 4 * (m0 & 1) + (c.col & 3);
            return (const T*)cv.w + co * S::CIN + ch * 32 + c.g * 8;
        }
    };
    auto load_group = [&](u32x4_t (&dst)[NA], int ky, int ch) {
#pragma unroll
        for (int kx = 0; kx < KT; ++kx)
#pragma unroll
            for (int mi = 0; mi < MBW; ++mi) dst[kx * MBW + mi] = *(const u32x4_t*)a_ptr(mi, ch, ky * KT + kx);
    };

    // B-fragment addressing: lane (g, col) reads pixel (y + (ky-1) D, col + (kx-1) D), channels ch*32 + 8g ..
    int cb[KT];
    bool cvalid[KT];
#pragma unroll
    for (int kx = 0; kx < KT; ++kx) {
        const int xk = c.col + (KT == 1 ? 0 : (kx - 1) * D);
        cvalid[kx] = xk >= 0 && xk < RS;
        cb[kx] = in_off + (r0 * RS + xk) * PLD + c.g * 8;
    }
    const int zb = ZERO_OFF + c.g * 8;

    f32x4_t acc[MBW][R];
#pragma unroll
    for (int mi = 0; mi < MBW; ++mi)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[mi][r] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // the MFMAs of one (tap row ky, chunk ch) group
    auto compute = [&](auto ky_, const u32x4_t (&ab)[NA], int ch) {
        constexpr int ky = decltype(ky_)::value;
        constexpr int dy = KT == 1 ? 0 : (ky - 1) * D;
#pragma unroll
        for (int kx = 0; kx < KT; ++kx) {
            bf16x8_t B[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (S::SKIP && !row_live(D, ky, YS + r)) continue;
                bool ok = cvalid[kx];
                if (!S::SKIP && KT != 1) ok = ok && r0 + r + dy >= 0 && r0 + r + dy < RS;
                const int off = (ok ? cb[kx] + (r + dy) * ROWE : zb) + ch * 32;
                B[r] = *(const bf16x8_t*)(c.smem + off);
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (S::SKIP && !row_live(D, ky, YS + r)) continue;
#pragma unroll
                for (int mi = 0; mi < MBW; ++mi) acc[mi][r] = mma16x16x32<T>(ab[kx * MBW + mi], B[r], acc[mi][r]);
            }
        }
    };

    if constexpr (S::BIG) {
        // groups (ky, ch) in order, the next group's A-fragments in flight during the current group's MFMAs
        u32x4_t a0[NA], a1[NA];
        load_group(a0, KY0, 0);
        __syncthreads();                               // the previous conv's outputs are in LDS
        StaticFor<0, NKY>::run([&](auto kyi) {
            constexpr int ky = KY0 + decltype(kyi)::value;
            constexpr bool last_ky = ky + 1 == KY1;
#pragma unroll 1
            for (int ch = 0; ch < NCH; ch += 2) {
                load_group(a1, ky, ch + 1);
                compute(std::integral_constant<int, ky>{}, a0, ch);
                const bool more = ch + 2 < NCH;
                if (more || !last_ky) load_group(a0, more ? ky : ky + 1, more ? ch + 2 : 0);
                compute(std::integral_constant<int, ky>{}, a1, ch + 1);
            }
        });
    } else {
        // a small conv: all of the wave's A-fragments up front (they arrive while the block waits at the barrier)
        u32x4_t aa[NKY * NCH][NA];
        StaticFor<0, NKY * NCH>::run([&](auto gi) {
            constexpr int i = decltype(gi)::value;
            load_group(aa[i], KY0 + i / NCH, i % NCH);
        });
        __syncthreads();
        StaticFor<0, NKY * NCH>::run([&](auto gi) {
            constexpr int i = decltype(gi)::value;
            compute(std::integral_constant<int, KY0 + i / NCH>{}, aa[i], i % NCH);
        });
    }

    // epilogue: MFMA row 4g + r of block m0 is cout 32(m0 >> 1) + 8g + 4(m0 & 1) + r (pipe_cout_perm)
#pragma unroll
    for (int mi = 0; mi < MBW; ++mi) {
        const int m0 = m_first + mi;
        const int co0 = 32 * (m0 >> 1) + 8 * c.g + 4 * (m0 & 1);
        if constexpr (!S::LAST) {
            float b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = cv.bias ? cv.bias[co0 + j] : 0.f;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float s = acc[mi][r][j] + b[j];
                    v[j] = s > 0.f ? s : 0.1f * s;
                }
                *(u32x2_t*)(c.smem + out_off + ((r0 + r) * RS + c.col) * PLD + co0) =
                    u32x2_t{H16<T>::pack(v[0], v[1]), H16<T>::pack(v[2], v[3])};
            }
        } else if (c.g == 0) {
            // the flow: conv + bias + the level's flow (fp32), couts 0 and 1 of block 0
            const RefineArgs& a = *c.a;
            const float* rs = (const float*)a.res.ptr + map_frame(a.res.map, c.pair) * a.res.img_stride + a.res.c0;
            float* fo = (float*)a.flow.ptr + map_frame(a.flow.map, c.pair) * a.flow.img_stride + a.flow.c0;
            const float b0 = cv.bias ? cv.bias[0] : 0.f, b1 = cv.bias ? cv.bias[1] : 0.f;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int px = (r0 + r) * RS + c.col;
                fo[(long long)px * a.flow.ld] = acc[mi][r][0] + b0 + rs[(long long)px * a.res.ld];
                fo[(long long)px * a.flow.ld + 1] = acc[mi][r][1] + b1 + rs[(long long)px * a.res.ld + 1];
            }
        }
    }
}

// a conv whose dead taps depend on the wave's row group: the row group's liveness class picks the instantiation
// (rows below / from the image's middle; within each half the R rows of a group share every tap row's fate only
// where R rows do not straddle a liveness edge, which holds for the specs below: edges at d, 16 - d and R | 8)
template <class S, typename T>
__device__ __forceinline__ void refine_conv_skip(const RefineCtx<T>& c, const RefineConv& cv, int in_off, int out_off) {
    const int rg = c.wave % S::NRG;
    if (rg * S::R < RS / 2)
        refine_conv<S, 0>(c, cv, in_off, out_off);
    else
        refine_conv<S, RS / 2>(c, cv, in_off, out_off);
}

//                       D   CIN COUT MBW R  SKIP   LAST
using Conv1 = ConvSpec<  2, 128, 128, 2, 8, true,  false>;
using Conv2 = ConvSpec<  4, 128, 128, 2, 8, true,  false>;
using Conv3 = ConvSpec<  8, 128,  96, 3, 4, true,  false>;
using Conv4 = ConvSpec<  0,  96,  64, 1, 8, false, false>;
using Conv5 = ConvSpec<  1,  64,  32, 1, 4, false, false>;
using Conv6 = ConvSpec<  1,  32,   2, 1, 2, false, true>;
// SKIP with YS = 0 or 8 stands for every row group of its half: a group of R rows from r0 must see, for each tap
// row, the liveness of rows YS .. YS + R - 1.  R = 8: r0 = YS.  Conv3 (d = 8, R = 4): row y reads y - 8 iff y >= 8
// and y + 8 iff y < 8, the same for every row of a half.
static_assert(Conv1::R == 8 && Conv2::R == 8 && Conv3::D == 8 && 8 % Conv3::R == 0, "pwc_refine: liveness classes");

template <typename T>
__global__ __launch_bounds__(512) void pwc_refine_kernel(RefineArgs a) {
    __shared__ __attribute__((aligned(16))) u32x4_t smem_[SMEM_ELEMS / 8];
    RefineCtx<T> c;
    c.smem = (T*)smem_;
    c.a = &a;
    c.lane = threadIdx.x & 63;
    c.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    c.g = c.lane >> 4;
    c.col = c.lane & 15;
    c.pair = blockIdx.x;
    // the pair's image into buffer 0 (16 x 16-byte pieces per pixel), the zero row
    const T* xin = img_ptr<T>(a.x, c.pair);
    for (int i = threadIdx.x; i < RS * RS * 16; i += 512) {
        const int px = i >> 4, q = i & 15;
        *(u32x4_t*)(c.smem + px * PLD + q * 8) = *(const u32x4_t*)(xin + (long long)px * a.x.ld + q * 8);
    }
    if (threadIdx.x < PLD / 8) *(u32x4_t*)(c.smem + ZERO_OFF + threadIdx.x * 8) = u32x4_t{0u, 0u, 0u, 0u};
    // (each conv's barrier comes after its first weight loads are issued)
    refine_conv_skip<Conv1>(c, a.cv[0], 0, IMG);
    refine_conv_skip<Conv2>(c, a.cv[1], IMG, 0);
    refine_conv_skip<Conv3>(c, a.cv[2], 0, IMG);
    refine_conv<Conv4, 0>(c, a.cv[3], IMG, 0);
    refine_conv<Conv5, 0>(c, a.cv[4], 0, IMG);
    refine_conv<Conv6, 0>(c, a.cv[5], IMG, 0);
}

struct RefineShape { int cin, cout, ksize, dil; };
const RefineShape kRefineConvs[6] = {{128, 128, 3, 2}, {128, 128, 3, 4}, {128, 96, 3, 8},
                                     {96, 64, 1, 1},   {64, 32, 3, 1},   {32, 2, 3, 1}};
}  // namespace

extern "C" int dbsr_pwc_refine_supported(int h, int w, int dtype) {
    return h == RS && w == RS && (dtype == DBSR_BF16 || dtype == DBSR_F16) ? 1 : 0;
}

extern "C" int dbsr_pwc_refine(int P, int h, int w, dbsr_tensor x, const dbsr_pwc_refine_conv* convs,
                               dbsr_tensor res_flow, dbsr_tensor flow_out, void* stream) {
    DBSR_CHECK_ARG(x.ptr && x.map.fpg > 0 && res_flow.ptr && res_flow.map.fpg > 0 && flow_out.ptr &&
                   flow_out.map.fpg > 0 && convs, "pwc_refine: null tensor");
    DBSR_CHECK_ARG(h == RS && w == RS, "pwc_refine: serves the 16x16 level only (got %dx%d; dbsr_pwc_refine_supported)",
                   h, w);
    DBSR_CHECK_ARG(x.dtype == DBSR_BF16 || x.dtype == DBSR_F16, "pwc_refine: x must be bf16 or fp16");
    DBSR_CHECK_ARG(P > 0, "pwc_refine: no pairs");
    DBSR_CHECK_ARG(x.ld % 8 == 0 && x.c0 % 8 == 0 && x.c0 + 128 <= x.ld, "pwc_refine: x needs 128 channels, 16-B aligned");
    DBSR_CHECK_ARG(res_flow.dtype == DBSR_F32 && res_flow.c0 + 2 <= res_flow.ld,
                   "pwc_refine: the residual flow must be fp32 with >= 2 channels");
    DBSR_CHECK_ARG(flow_out.dtype == DBSR_F32 && flow_out.c0 + 2 <= flow_out.ld,
                   "pwc_refine: flow_out must be fp32 with >= 2 channels");
    RefineArgs a;
    a.P = P; a.x = x; a.res = res_flow; a.flow = flow_out;
    for (int i = 0; i < 6; ++i) {
        const dbsr_pwc_refine_conv& c = convs[i];
        const RefineShape& s = kRefineConvs[i];
        DBSR_CHECK_ARG(c.w, "pwc_refine: conv %d: null weights", i);
        DBSR_CHECK_ARG(c.cin == s.cin && c.cout == s.cout && c.ksize == s.ksize && (s.ksize == 1 || c.dil == s.dil),
                       "pwc_refine: conv %d must be %d -> %d, %dx%d, dilation %d (got %d -> %d, %dx%d, dilation %d)", i,
                       s.cin, s.cout, s.ksize, s.ksize, s.dil, c.cin, c.cout, c.ksize, c.ksize, c.dil);
        // 3x3: the chunk-major copy follows the round_up(cout, 64) x (9 cin) row-major weights (dbsr_conv_packed_elems)
        const void* wp = s.ksize == 3 ? (const char*)c.w + (size_t)((s.cout + 63) / 64 * 64) * 9 * s.cin * 2 : c.w;
        a.cv[i] = RefineConv{wp, c.bias};
    }
    if (x.dtype == DBSR_BF16)
        hipLaunchKernelGGL(pwc_refine_kernel<bf16_t>, dim3((unsigned)P), dim3(512), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(pwc_refine_kernel<f16_t>, dim3((unsigned)P), dim3(512), 0, (hipStream_t)stream, a);
    DBSR_LAUNCH_CHECK();
    return 0;
}
