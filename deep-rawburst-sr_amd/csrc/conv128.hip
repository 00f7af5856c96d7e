// The weight-stationary 3x3 conv for 128 -> 128 channels (dbsr_conv2d picks it; the selection is in conv2d.hip).
// Its own translation unit so the kernel builds in seconds.
#include "conv_core.hpp"

#include <algorithm>

namespace dbsr {

// ------------------------------------------------------------------------------------------------
// 128 -> 128 3x3/s1/p1 conv with both operands' reuse on chip: the weight predictor's input conv and its
// ResBlocks (merging.py:86-90, 98-101: seven 128-channel convs over every frame of the burst, ~71 GFLOP each at the
// bench shape).  The pipelined kernel streams a 64-cout tile's weights through the LDS with every 48 x 8 tile (one
// 1-KiB LDS-DMA piece per ~200 FLOP); the weight-stationary kernel's registers hold a whole cout tile only for
// Cin <= 64.  Here the eight waves of a block split the couts only: wave p holds couts 16 p .. 16 p + 15 over the
// whole K (4 chunks x 9 taps of A-fragments, 144 VGPRs, gathered once from the chunk-major copy so that lanes l and
// l + 32 hold adjacent 4-cout groups: ks128_sched.hpp lane_cout), so only the tile's halo moves through the LDS
// (one piece per ~820 FLOP) and no partial sum ever leaves a wave.
//
// Per 16 x 8 output tile: the 18 x 10-pixel halo of all 128 channels is LDS-DMA'd one tile ahead into a double
// buffer (halo_phys swizzle; chunk images 184 pixels apart so the swizzle parity is the chunk-local one;
// out-of-frame pixels land zeros).  One barrier publishes it.  Every wave then keeps the accumulators of all 8
// output rows live and, chunk by chunk, walks the 10 halo rows: the B-fragment of (chunk, halo row i, kx) is read
// once and feeds output rows y = i - ky, ky = 0 .. 2, with tap 3 ky + kx -- 120 reads for 288 MFMAs, one
// software-pipelined stream per tile (inline-asm ds_read_b128 AHEAD fragments before use, a counted lgkmcnt per
// fragment).  A row receives taps 0 .. 8 of chunk 0, then of chunk 1, ...: one in-order fp32 MFMA chain from zero
// over k-step = chunk * 9 + tap, then the bias.  Rows 2 pr, 2 pr + 1 are final after halo row 2 pr + 3 of the last
// chunk; their epilogue (bias, act, then lanes l / l + 32 swap halves so that each lane holds 8 consecutive couts of
// one pixel; residual, act, gate; one 16-B store) runs under the remaining MFMAs.  The next tile's DMA pieces, the
// residual and the gate loads sit at fixed positions of the stream (ks128_sched.hpp).
// Block -> tiles: rb_tile (a full round of 256 tiles XCD-contiguous); grid = min(CUs or cap, tiles).
// ------------------------------------------------------------------------------------------------
template <typename T, int EPI>
__global__ __launch_bounds__(512, 1) void conv3x3_ks128_kernel(ConvK k, int tiles_x, int tiles_y, int ntiles) {
    using namespace ks128;
    DBSR_OWN_SIMDS();
    __shared__ __attribute__((aligned(16))) u32x4_t lds[LDS_U4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, col = lane & 15;
    const int H = k.in_h, W = k.in_w;
    // epilogues (the pipelined kernel's): 1 bias + ReLU, 2 bias + residual then ReLU, 3 bias, 0 run-time act /
    // residual / post-act, 5 as 0 then the training dgrad's ReLU-backward gate (out *= gate > 0)
    constexpr bool RT = EPI == 0 || EPI == 5, has_gate = EPI == 5;
    const bool has_res = EPI == 2 || (RT && k.r != nullptr);
    auto act1 = [&](float v) {
        if constexpr (EPI == 1) return fmaxf(v, 0.f);
        else if constexpr (RT) return apply_act(v, k.act);
        else return v;
    };
    auto act2 = [&](float v) {
        if constexpr (EPI == 2) return fmaxf(v, 0.f);
        else if constexpr (RT) return apply_act(v, k.post_act);
        else return v;
    };

    // this wave's A-fragments: MFMA row m of lane (k-group g, m) is cout lane_cout(wave, m), gathered from piece
    // (packed_block * 4 + chunk) * 9 + tap, row packed_row of the chunk-major copy
    Frag<T> w[NCH][9];
    {
        const int m = col;
        const char* wsrc = (const char*)k.w_pipe + (size_t)packed_block(wave, m) * (NCH * 9 * 1024) +
                           (g * 16 + packed_row(wave, m)) * 16;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) w[c][tap].load((const T*)(wsrc + (c * 9 + tap) * 1024));
    }
    // accumulator r of this lane is cout co4 + r; after the swap the lane stores couts co8 .. co8 + 7 of row
    // 2 pr + (g >> 1), pixel col
    const int co4 = lane_cout(wave, 4 * g), co8 = 16 * wave + 8 * (g & 1);
    float bv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[r] = k.bias ? k.bias[co4 + r] : 0.f;          // (cout == 128)
    const int prow = (g >> 1) * k.out_w + col;
    const int yl = prow * k.y_ld + co8, rl = has_res ? prow * k.r_ld + co8 : 0, gl = has_gate ? prow * k.g_ld + co8 : 0;

    struct Tile { const T* xf; long long y_off, r_off, g_off; int y0, x0; };
    auto decode = [&](int i) {
        const int t = rb_tile(i, blockIdx.x, gridDim.x, ntiles);
        const int tx = t % tiles_x, r = t / tiles_x, ty = r % tiles_y, f = r / tiles_y;
        Tile tl;
        tl.y0 = ty * TH; tl.x0 = tx * TW;
        tl.xf = (const T*)k.x + map_frame(k.xm, f) * k.x_is;
        const long long pix = (long long)tl.y0 * k.out_w + tl.x0;
        tl.y_off = map_frame(k.ym, f) * k.y_is + k.y_c0 + pix * k.y_ld;
        tl.r_off = has_res ? map_frame(k.rm, f) * k.r_is + k.r_c0 + pix * k.r_ld : 0;
        tl.g_off = has_gate ? map_frame(k.gm, f) * k.g_is + k.g_c0 + pix * k.g_ld : 0;
        return tl;
    };
    const int my_tiles = ntiles / (int)gridDim.x + ((int)blockIdx.x < ntiles % (int)gridDim.x ? 1 : 0);

    // halo DMA: piece `it` of this wave is item wave + 8 it (clamped: surplus slots rewrite the last piece with
    // identical bytes); lane -> (chunk, halo pixel, physical k-group slot), tile-invariant
    const int pix_b = k.x_ld * (int)sizeof(T);
    const unsigned frame_bytes = (unsigned)((long long)H * W * pix_b);
    const unsigned lds0 = (unsigned)(unsigned long long)(__attribute__((address_space(3))) u32x4_t*)lds;
    // (the run-time epilogues need the registers: they form a piece's two words again at every issue, from a lane id
    // the compiler cannot hoist out of the tile loop)
    auto piece = [&](int it, int ln, int& rc, int& off) {
        const int item = min(wave + NW * it, PIECES - 1);
        const int qq = item * 16 + (ln >> 2), c = qq / CPX, p = qq - c * CPX, ph = ln & 3;
        const int gg = piece_kgroup(p, ph);
        const int r = p / HW, cc = p - r * HW;
        rc = p < HPX ? (r << 16) | cc : 0x7fff7fff;             // pixel slots past the halo land zeros
        off = (r * W + cc) * pix_b + c * 64 + gg * 16;
    };
    int h_rc[RT ? 1 : PER], h_off[RT ? 1 : PER];
    if constexpr (!RT) {
#pragma unroll
        for (int it = 0; it < PER; ++it) piece(it, lane, h_rc[it], h_off[it]);
    }
    auto dma = [&](int it, const Tile& tl, int buf) {
        const int item = min(wave + NW * it, PIECES - 1);
        int rc, off;
        if constexpr (RT) {
            int ln = lane;
            asm volatile("" : "+v"(ln));
            piece(it, ln, rc, off);
        } else {
            rc = h_rc[it];
            off = h_off[it];
        }
        const int hy = tl.y0 - 1 + (rc >> 16), hx = tl.x0 - 1 + (rc & 0xffff);
        const bool ok = (unsigned)hy < (unsigned)H && (unsigned)hx < (unsigned)W;
        const int base = ((tl.y0 - 1) * W + (tl.x0 - 1)) * pix_b;
        lds_dma16(tl.xf, frame_bytes, ok ? base + off : BUF_OOB, 0, lds0 + (unsigned)((buf * BUF_U4 + item * 64) * 16));
    };
    // B-fragment reads: byte address of pixel col + rho, k-group g (frag_slot), rho = pixel offset & 7, in the halo
    // buffer of the current tile (moved to the other buffer after every tile)
    unsigned ba[8];
#pragma unroll
    for (int rho = 0; rho < 8; ++rho) ba[rho] = lds0 + 16u * (4 * col + frag_slot(col + rho, g));

    Tile cur = decode(0);
    if (my_tiles > 0) {
#pragma unroll
        for (int it = 0; it < PER; ++it) dma(it, cur, 0);
    }
    vm_drain();
    const long long y_pair = 2LL * k.out_w * k.y_ld, r_pair = 2LL * k.out_w * k.r_ld, g_pair = 2LL * k.out_w * k.g_ld;
    for (int ti = 0; ti < my_tiles; ++ti) {
        // this wave's DMA pieces of tile ti landed: they are older than every store of tile ti - 1, so the youngest
        // TH / 2 vector-memory operations may stay in flight; then everyone's
        DBSR_VM_WAIT(TH / 2);
        __syncthreads();
        const bool more = ti + 1 < my_tiles;
        const Tile nxt = more ? decode(ti + 1) : cur;
        const int buf = ti & 1;
        f32x4_t acc[TH];
        u32x4_t resv[TH / 2], gatev[has_gate ? TH / 2 : 1];
        Frag<T> bq[AHEAD];
        auto rd = [&](auto n_) {
            constexpr int n = decltype(n_)::value, c = read_chunk(n), imm = read_pix(n);
            // (asm operands name this lambda's own locals: clang does not capture for asm operands)
            const unsigned a = ba[imm & 7];
            bf16x8_t v;
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(a), "i"(16 * (c * CH_U4 + 4 * imm)));
            bq[n % AHEAD].v = v;
        };
        // rows 2 pr, 2 pr + 1: bias, act, halves swapped between lanes l and l + 32, residual, act, gate, 16-B store
        auto epilogue = [&](auto pr_) {
            constexpr int pr = decltype(pr_)::value;
            // the loaded residual and gate are first touched here, behind this position's fragment wait: without the
            // pin the compiler converts them right behind their loads and the stream waits out the memory latency
            if (has_res) asm volatile("" : "+v"(resv[pr]));
            if constexpr (has_gate) asm volatile("" : "+v"(gatev[pr]));
            float v[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float a0 = act1(acc[2 * pr][r] + bv[r]), a1 = act1(acc[2 * pr + 1][r] + bv[r]);
                // lanes 32 .. 63 of the first operand <-> lanes 0 .. 31 of the second: lane l < 32 ends with row
                // 2 pr's couts co8 .. + 3 (its own) and + 4 .. + 7 (lane l + 32's); lane l + 32 with row 2 pr + 1's
                const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(a0), __float_as_uint(a1), false, false);
                v[r] = __uint_as_float(s[0]);
                v[4 + r] = __uint_as_float(s[1]);
            }
            if (has_res) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[2 * e] = act2(v[2 * e] + H16<T>::lo(resv[pr][e]));
                    v[2 * e + 1] = act2(v[2 * e + 1] + H16<T>::hi(resv[pr][e]));
                }
            }
            if constexpr (has_gate) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[2 * e] = H16<T>::lo(gatev[pr][e]) > 0.f ? v[2 * e] : 0.f;
                    v[2 * e + 1] = H16<T>::hi(gatev[pr][e]) > 0.f ? v[2 * e + 1] : 0.f;
                }
            }
            u32x4_t o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = H16<T>::pack(v[2 * e], v[2 * e + 1]);
            *(u32x4_t*)((T*)k.y + cur.y_off + pr * y_pair + yl) = o;
        };

        StaticFor<0, AHEAD>::run([&](auto n_) { rd(n_); });
        StaticFor<0, READS>::run([&](auto n_) {
            constexpr int n = decltype(n_)::value, c = read_chunk(n);
            // reads issued after read n: n + 1 .. n + AHEAD - 1
            constexpr int newer = AHEAD - 1 < READS - 1 - n ? AHEAD - 1 : READS - 1 - n;
            bf16x8_t v = bq[n % AHEAD].v;
            asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(v) : "i"(newer));
            Frag<T> b;
            b.v = v;
            StaticFor<0, 3>::run([&](auto ky_) {
                constexpr int ky = decltype(ky_)::value;
                if constexpr (feeds(n, ky)) {
                    constexpr int y = read_row(n) - ky, tap = 3 * ky + read_kx(n);
                    const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
                    acc[y] = mma(w[c][tap], b, kstep(n, ky) == 0 ? z : acc[y]);
                }
            });
            if constexpr (n + AHEAD < READS) rd(std::integral_constant<int, n + AHEAD>{});
            // side work at its stream position: the next tile's halo pieces, residual and gate loads, epilogues
            StaticFor<0, PER>::run([&](auto it_) {
                constexpr int it = decltype(it_)::value;
                if constexpr (n == dma_at(it)) {
                    if (more) dma(it, nxt, buf ^ 1);
                }
            });
            StaticFor<0, TH / 2>::run([&](auto pr_) {
                constexpr int pr = decltype(pr_)::value;
                if constexpr (n == res_at(pr, RT)) {
                    if (has_res) resv[pr] = *(const u32x4_t*)((const T*)k.r + cur.r_off + pr * r_pair + rl);
                }
                if constexpr (has_gate && n == gate_at(pr))
                    gatev[pr] = *(const u32x4_t*)((const T*)k.gt + cur.g_off + pr * g_pair + gl);
                if constexpr (n == pair_done(pr)) epilogue(pr_);
            });
        });
        cur = nxt;
#pragma unroll
        for (int rho = 0; rho < 8; ++rho) ba[rho] += buf ? (unsigned)(-BUF_U4 * 16) : (unsigned)(BUF_U4 * 16);
    }
    vm_drain();                         // (no LDS-DMA outstanding at s_endpgm: tools/isa_audit.py)
}

// a 128 -> 128 conv of n_frames frames (multiples of 16 x 8) on grid = min(cap or CUs, tiles) persistent blocks
int ks128_launch(const ConvK& k, int n_frames, bool f16, int epi, int max_blocks, int cus, hipStream_t s) {
    const char* why = ks128::launch_error(k.out_h, k.out_w, k.in_h, k.in_w, n_frames, (long long)k.x_ld * 2, k.y_ld,
                                          k.y_c0, k.r != nullptr, k.r_ld, k.r_c0, k.gt != nullptr, k.g_ld, k.g_c0);
    DBSR_CHECK_ARG(why == nullptr, "conv2d: the 128-channel weight-stationary kernel cannot run this: %s", why);
    const int tiles_x = k.out_w / ks128::TW, tiles_y = k.out_h / ks128::TH;
    const long long nt = (long long)n_frames * tiles_x * tiles_y;
    DBSR_CHECK_ARG(nt > 0 && nt < (1LL << 31), "conv2d: bad tile count for the 128-channel weight-stationary kernel");
    const int ntiles = (int)nt;
    int grid = max_blocks > 0 ? std::min(max_blocks, cus) : cus;
    grid = std::min(grid, ntiles);
    DBSR_CHECK_ARG(rb_mapping_ok(grid, ntiles), "conv2d: tile mapping out of range (grid %d, %d tiles)", grid, ntiles);
#define DBSR_KS_LAUNCH(TT, E) \
    hipLaunchKernelGGL((conv3x3_ks128_kernel<TT, E>), dim3(grid), dim3(512), 0, s, k, tiles_x, tiles_y, ntiles)
#define DBSR_KS_EPI(TT)                          \
    switch (epi) {                               \
        case 1: DBSR_KS_LAUNCH(TT, 1); break;    \
        case 2: DBSR_KS_LAUNCH(TT, 2); break;    \
        case 3: DBSR_KS_LAUNCH(TT, 3); break;    \
        case 5: DBSR_KS_LAUNCH(TT, 5); break;    \
        default: DBSR_KS_LAUNCH(TT, 0); break;   \
    }
    if (f16) {
        DBSR_KS_EPI(f16_t)
    } else {
        DBSR_KS_EPI(bf16_t)
    }
#undef DBSR_KS_EPI
#undef DBSR_KS_LAUNCH
    DBSR_LAUNCH_CHECK();
    return 0;
}

}  // namespace dbsr
