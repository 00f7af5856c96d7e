// Tile geometry and the row-rolling schedule of the fused 32-channel ResBlock kernel (conv2d.hip, resblock32_kernel)
// as plain constexpr C++: the kernel's unrolled streams are generated from these functions, and
// tests/test_rb32_sched.py builds them into a stand-alone program (tools/rb32_sched_check.cpp, under the host
// sanitizers) that replays one tile against a scalar ResBlock.
#pragma once
#include "ks128_sched.hpp"

namespace dbsr {
namespace rb32 {

constexpr int TW = 32, TH = 16;                               // output tile
constexpr int MW = TW + 2, MH = TH + 2, MPX = MW * MH;        // conv1 region (the intermediate) 34 x 18
constexpr int IW = TW + 4, IH = TH + 4, IPX = IW * IH;        // input halo 36 x 20
constexpr int IN_PIECES = (IPX + 15) / 16;                    // 45 1-KiB halo pieces
constexpr int IN_U4 = IN_PIECES * 64;                         // one halo buffer, 16-B slots
constexpr int MID_U4 = (MPX + 15) / 16 * 16 * 4;              // the intermediate image, 16-B slots
constexpr int NW = 8, NS = 2, NB = 4;                         // waves: 2 column strips of 16 x 4 row bands
constexpr int PER = (IN_PIECES + NW - 1) / NW;                // DMA pieces per wave per tile
constexpr int AHEAD = 4;                                      // LDS reads in flight ahead of their use
constexpr int LDS_BYTES = (2 * IN_U4 + MID_U4) * 16 + 64 * 4;
static_assert(LDS_BYTES <= 160 * 1024, "resblock LDS");

// both images keep pixel p's four 16-B k-groups in slots 4 p .. 4 p + 3, k-group g at frag_slot(p, g)
using ks128::frag_slot;
using ks128::piece_kgroup;

constexpr int wave_strip(int w) { return w & 1; }
constexpr int wave_band(int w) { return w >> 1; }

// ---- conv1, the 32 main columns: band b of a strip is c1_rows(b) intermediate rows from c1_row0(b) ----
constexpr int c1_rows(int b) { return b < 2 ? 5 : 4; }
constexpr int c1_row0(int b) { return b < 2 ? 5 * b : 10 + 4 * (b - 2); }
static_assert(c1_row0(NB - 1) + c1_rows(NB - 1) == MH, "conv1 bands cover the intermediate's rows");

// The B-fragment stream of a band of NR rows: read n is (input row i of the band's NR + 2, kx); the fragment is read
// once and feeds the band's rows r = i - ky (0 <= r < NR) with tap 3 ky + kx, in both 16-cout blocks.
template <int NR_>
struct Rows {
    static constexpr int NR = NR_;
    static constexpr int READS = (NR + 2) * 3;
    static constexpr int MFMAS = NR * 9 * 2;
    static constexpr int read_row(int n) { return n / 3; }
    static constexpr int read_kx(int n) { return n % 3; }
    static constexpr bool feeds(int n, int ky) { return read_row(n) - ky >= 0 && read_row(n) - ky < NR; }
    static constexpr int tap(int n, int ky) { return 3 * ky + read_kx(n); }
    // row r is final after this read's MFMAs (input row r + 2, kx = 2): its epilogue follows at that position
    static constexpr int row_done(int r) { return (r + 2) * 3 + 2; }
    // every row receives taps 0 .. 8 in order, once each, and none after its epilogue
    static constexpr bool schedule_ok() {
        int next[NR] = {}, total = 0;
        for (int n = 0; n < READS; ++n)
            for (int ky = 0; ky < 3; ++ky)
                if (feeds(n, ky)) {
                    const int r = read_row(n) - ky;
                    if (tap(n, ky) != next[r] || n > row_done(r)) return false;
                    ++next[r];
                    total += 2;
                }
        for (int r = 0; r < NR; ++r)
            if (next[r] != 9 || row_done(r) >= READS) return false;
        return total == MFMAS && row_done(NR - 1) == READS - 1 && AHEAD >= 1 && AHEAD < READS;
    }
};
static_assert(Rows<5>::schedule_ok() && Rows<4>::schedule_ok(), "conv1 row-rolling schedule");
// pixel offset of read n from the lane's base pixel, in an image `iw` pixels wide
template <int NR> constexpr int rows_pix(int n, int iw) { return Rows<NR>::read_row(n) * iw + Rows<NR>::read_kx(n); }

// ---- conv1, the two edge columns (32, 33) x 18 rows: 36 pixels flattened column by column into three 16-pixel
// groups with per-lane addresses, one each for three of the four 4-row-band waves; 9 reads (tap order), 18 MFMAs ----
constexpr int EDGE_PX = 2 * MH, EDGE_GROUPS = (EDGE_PX + 15) / 16;
constexpr int edge_group(int w) { return c1_rows(wave_band(w)) == 4 && w - 2 * NS < EDGE_GROUPS ? w - 2 * NS : -1; }
constexpr int edge_row(int e) { return e % MH; }
constexpr int edge_col(int e) { return TW + e / MH; }
constexpr int EDGE_READS = 9, EDGE_MFMAS = 18;
constexpr int edge_pix(int tap) { return (tap / 3) * IW + tap % 3; }

// conv1's LDS reads and MFMAs of wave w per tile
constexpr int c1_reads(int w) { return (c1_rows(wave_band(w)) + 2) * 3 + (edge_group(w) >= 0 ? EDGE_READS : 0); }
constexpr int c1_mfmas(int w) { return c1_rows(wave_band(w)) * 18 + (edge_group(w) >= 0 ? EDGE_MFMAS : 0); }
constexpr bool conv1_ok() {
    int total = 0, groups = 0;
    for (int w = 0; w < NW; ++w) {
        if (c1_mfmas(w) > 90) return false;                  // no wave does more than the five-group batch body did
        total += c1_mfmas(w);
        groups += edge_group(w) >= 0;
    }
    return total == (MPX + 15) / 16 * 18 && groups == EDGE_GROUPS;
}
static_assert(conv1_ok(), "conv1 work split");

// ---- conv2: a wave is (strip, band of 4 output rows) and walks the band's 6 intermediate rows.  Its LDS stream has
// 22 items: the 18 fragments, and behind the fragment that finishes output row y the row's residual (the input
// halo's centre pixel), which the row's epilogue consumes ----
struct Conv2 {
    static constexpr int NR = TH / NB;                        // 4
    static constexpr int FRAGS = (NR + 2) * 3, ITEMS = FRAGS + NR, MFMAS = NR * 18;
    static constexpr bool is_res(int n) { return n >= 9 && (n - 9) % 4 == 0; }
    static constexpr int res_row(int n) { return (n - 9) / 4; }
    // fragment index (as Rows<4>'s read n) of a fragment item
    static constexpr int frag(int n) { return n < 9 ? n : 9 + 3 * ((n - 9) / 4) + (n - 9) % 4 - 1; }
    static constexpr int epilogue_at(int y) { return 9 + 4 * y; }
    static constexpr bool schedule_ok() {
        int nf = 0, nr = 0;
        for (int n = 0; n < ITEMS; ++n) {
            if (is_res(n)) {
                // the residual item of row y directly follows the row's last fragment
                if (res_row(n) != nr || n != epilogue_at(nr) || n == 0 || is_res(n - 1) ||
                    frag(n - 1) != Rows<NR>::row_done(nr))
                    return false;
                ++nr;
            } else {
                if (frag(n) != nf) return false;
                ++nf;
            }
        }
        return nf == FRAGS && nr == NR && is_res(ITEMS - 1) && AHEAD < ITEMS;
    }
};
static_assert(Conv2::schedule_ok(), "conv2 row-rolling schedule");
// a wave's stores of a tile (one per output row): all younger than its DMA pieces of the next tile, which are issued
// before conv1 and drained at the tile's second barrier, so the first barrier of the next tile may leave them in flight
constexpr int STORES = Conv2::NR;

}  // namespace rb32
}  // namespace dbsr
