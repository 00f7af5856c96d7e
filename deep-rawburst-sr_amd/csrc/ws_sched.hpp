// Tile geometry and the row-rolling schedule of the weight-stationary 3x3 kernel's 64-cout body (conv2d.hip,
// ws_rows_body: Cin <= 64, 16 x 16 and 16 x 8 tiles) as plain constexpr C++: the kernel's unrolled stream is generated
// from these functions, and tests/test_ws_sched.py builds them into a stand-alone program (tools/ws_sched_check.cpp,
// under the host sanitizers) that replays one tile against a scalar convolution.
#pragma once
#include "ks128_sched.hpp"

namespace dbsr {
namespace wsr {

constexpr int TW = 16, WM = 64;                               // tile width, couts per block
constexpr int NW = 8, WC = 2, WP = 4;                         // waves: 2 across the couts (32 each) x 4 across the rows
constexpr int AHEAD = 3;                                      // B-fragments in flight ahead of their MFMAs
constexpr int RES_LEAD = 6;                                   // reads between a row's residual load and its epilogue

// halo swizzle and DMA-piece lane map: those of the 128-channel kernel (conv_core.hpp's halo_phys)
using ks128::frag_slot;
using ks128::piece_kgroup;

template <int TH_, int NCH_>
struct Sched {
    static constexpr int TH = TH_, NCH = NCH_;
    static constexpr int RPW = TH / WP;                       // output rows per wave
    static constexpr int HW = TW + 2, HH = TH + 2, NQ = HW * HH;
    static constexpr int IN_ITEMS = (NQ + 15) / 16;           // 1-KiB halo pieces per 32-channel chunk image
    static constexpr int CPX = IN_ITEMS * 16;                 // pixel slots per chunk image
    static constexpr int CH_U4 = CPX * 4;                     // 16-B slots per chunk image
    static constexpr int ITEMS = NCH * IN_ITEMS;              // pieces per tile
    static constexpr int PER = (ITEMS + NW - 1) / NW;         // pieces per wave per tile
    static constexpr int STAGE_U4 = ITEMS * 64;               // one halo buffer
    static constexpr int W_PIECES = (WM / 16) * NCH * 9;      // the cout tile's chunk-major weights, 1-KiB pieces
    static constexpr int W_PER = (W_PIECES + NW - 1) / NW;
    // [halo 0][halo 1][bias]; the block's weights are staged once at [halo 1 ...) before the first tile
    static constexpr int LDS_U4 = 2 * STAGE_U4 > STAGE_U4 + W_PIECES * 64 ? 2 * STAGE_U4 : STAGE_U4 + W_PIECES * 64;
    static_assert(TH % WP == 0 && RPW >= 1 && CPX % 8 == 0 && (LDS_U4 + WM / 4) * 16 <= 160 * 1024, "ws rows tile");

    // The B-fragment stream of one wave and tile: read n is (chunk, halo row i of the wave's RPW + 2, kx),
    // chunk-major; the fragment is read once and feeds the wave's rows y = i - ky (0 <= y < RPW) with tap 3 ky + kx,
    // for both of the wave's 16-cout blocks.
    static constexpr int RPC = (RPW + 2) * 3;                 // reads per chunk
    static constexpr int READS = NCH * RPC;                   // reads per wave per tile
    static constexpr int MFMAS = NCH * 9 * RPW * 2;           // MFMAs per wave per tile
    static constexpr int read_chunk(int n) { return n / RPC; }
    static constexpr int read_row(int n) { return n % RPC / 3; }
    static constexpr int read_kx(int n) { return n % 3; }
    // halo pixel of the wave's first row, column 0 (the wave adds wp * RPW * HW + its column)
    static constexpr int read_pix(int n) { return read_row(n) * HW + read_kx(n); }
    static constexpr bool feeds(int n, int ky) { return read_row(n) - ky >= 0 && read_row(n) - ky < RPW; }
    static constexpr int kstep(int n, int ky) { return read_chunk(n) * 9 + 3 * ky + read_kx(n); }
    // row y of the wave is final after this read's MFMAs (the last chunk's halo row y + 2, kx = 2): its epilogue
    // and its 16-byte store follow at that position
    static constexpr int row_done(int y) { return (NCH - 1) * RPC + (y + 2) * 3 + 2; }
    // side work: this wave's DMA piece `it` of the next tile, all before dma_span(); then the residual / gate load of
    // row y, RES_LEAD reads ahead of its epilogue where the DMA pieces leave room
    static constexpr int dma_span() { return row_done(0) - RES_LEAD > PER ? row_done(0) - RES_LEAD : PER; }
    static constexpr int dma_at(int it) { return it * dma_span() / PER; }
    static constexpr int res_at(int y) { return row_done(y) - RES_LEAD > dma_span() ? row_done(y) - RES_LEAD : dma_span(); }
    // vector-memory operations a wave may leave in flight at the tile barrier: its RPW stores, which are younger
    // than every DMA piece
    static constexpr int STORES = RPW;

    // every output row receives k-steps 0 .. 9 NCH - 1 in order, once each; every read stays inside its chunk image
    // (for the last wave too); every DMA piece is issued before the first residual load and the first store of the
    // tile (the tile loop's counted vmcnt wait relies on it); every load before its epilogue
    static constexpr bool schedule_ok() {
        int next[RPW] = {}, total = 0;
        for (int n = 0; n < READS; ++n) {
            if ((WP - 1) * RPW * HW + read_pix(n) + TW - 1 >= NQ) return false;
            if (16 * (read_chunk(n) * CH_U4 + 4 * read_pix(n)) >= 65536) return false;   // the ds_read's offset field
            for (int ky = 0; ky < 3; ++ky)
                if (feeds(n, ky)) {
                    const int y = read_row(n) - ky;
                    if (kstep(n, ky) != next[y]) return false;
                    ++next[y];
                    total += 2;
                }
        }
        for (int y = 0; y < RPW; ++y)
            if (next[y] != NCH * 9) return false;
        if (total != MFMAS) return false;
        for (int y = 0; y < RPW; ++y) {
            if (row_done(y) >= READS || (y > 0 && row_done(y) <= row_done(y - 1))) return false;
            for (int n = row_done(y) + 1; n < READS; ++n)       // no later read feeds a finished row
                for (int ky = 0; ky < 3; ++ky)
                    if (feeds(n, ky) && read_row(n) - ky == y) return false;
            if (res_at(y) < dma_span() || res_at(y) >= row_done(y)) return false;
        }
        for (int it = 0; it < PER; ++it)
            if (dma_at(it) < 0 || dma_at(it) >= dma_span() || dma_at(it) >= row_done(0) ||
                (it > 0 && dma_at(it) < dma_at(it - 1)))
                return false;
        return row_done(RPW - 1) == READS - 1 && AHEAD >= 1 && AHEAD < RPC && dma_span() < row_done(0);
    }
};

static_assert(Sched<16, 2>::schedule_ok() && Sched<16, 1>::schedule_ok() && Sched<8, 2>::schedule_ok(),
              "ws row-rolling schedule");
static_assert(Sched<16, 2>::READS == 36 && Sched<16, 2>::MFMAS == 144, "16 x 16 tile at cin 64");

}  // namespace wsr
}  // namespace dbsr
