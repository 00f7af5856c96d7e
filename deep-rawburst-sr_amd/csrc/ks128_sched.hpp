// Tile geometry and the row-rolling schedule of the 128 -> 128 weight-stationary 3x3 kernel (conv128.hip) as plain
// constexpr C++: the kernel's unrolled loops are generated from these functions, the launch checks them on the host,
// and tests/test_ks128_sched.py builds them into a stand-alone program (under the host sanitizers) that replays the
// schedule against a scalar convolution.
#pragma once

namespace dbsr {
namespace ks128 {

constexpr int TW = 16, TH = 8;                                // output tile (frames must be multiples)
constexpr int HW = TW + 2, HH = TH + 2, HPX = HW * HH;        // halo 18 x 10 = 180 pixels
constexpr int CPX = 184;                                      // pixel slots per chunk image (a multiple of 8)
constexpr int NCH = 4;                                        // 32-channel chunks
constexpr int CH_U4 = CPX * 4;                                // 16-B slots per chunk image
constexpr int PIECES = NCH * CPX / 16;                        // 46 1-KiB halo pieces per tile
constexpr int BUF_U4 = NCH * CH_U4;                           // one halo buffer (47,104 B)
constexpr int NBUF = 2;                                       // halo buffers: the DMA runs one tile ahead
constexpr int NW = 8;                                         // waves per block, 16 couts each
constexpr int PER = (PIECES + NW - 1) / NW;                   // DMA pieces per wave per tile
constexpr int LDS_U4 = NBUF * BUF_U4;
static_assert(LDS_U4 * 16 <= 160 * 1024, "ks128 LDS");
static_assert(CPX % 8 == 0 && CPX >= HPX && (NCH * CPX) % 16 == 0, "chunk images");

// Halo swizzle inside a chunk image: pixel p keeps its four 16-B k-groups in slots 4 p .. 4 p + 3, k-group g in slot
// frag_slot(p, g) (conv_core.hpp's halo_phys); lane ph of a DMA piece's pixel therefore fetches k-group
// piece_kgroup(p, ph)
constexpr int frag_slot(int p, int g) { return 2 * (g & 1) + ((g >> 1) ^ ((p >> 2) & 1)); }
constexpr int piece_kgroup(int p, int ph) { return 2 * ((ph & 1) ^ ((p >> 2) & 1)) + (ph >> 1); }
constexpr bool swizzle_ok() {
    for (int p = 0; p < CPX; ++p)
        for (int g = 0; g < 4; ++g)
            if (frag_slot(p, g) < 0 || frag_slot(p, g) > 3 || piece_kgroup(p, frag_slot(p, g)) != g) return false;
    return true;
}
static_assert(swizzle_ok(), "ks128 halo swizzle");

// The B-fragment stream of one tile: read n is (chunk, halo row, kx), chunk-major; each fragment is read once and
// feeds output rows y = i - ky (0 <= y < TH) with tap 3 ky + kx.
constexpr int RPC = HH * 3;                                   // reads per chunk (30)
constexpr int READS = NCH * RPC;                              // reads per wave per tile (120)
constexpr int MFMAS = NCH * 9 * TH;                           // MFMAs per wave per tile (288)
constexpr int AHEAD = 4;                                      // fragments in flight ahead of their MFMAs
constexpr int read_chunk(int n) { return n / RPC; }
constexpr int read_row(int n) { return n % RPC / 3; }
constexpr int read_kx(int n) { return n % 3; }
constexpr int read_pix(int n) { return read_row(n) * HW + read_kx(n); }        // halo pixel of output column 0
constexpr bool feeds(int n, int ky) { return read_row(n) - ky >= 0 && read_row(n) - ky < TH; }
// k-step (chunk * 9 + tap) that read n contributes to row read_row(n) - ky
constexpr int kstep(int n, int ky) { return read_chunk(n) * 9 + 3 * ky + read_kx(n); }
// rows 2 pr, 2 pr + 1 are final after this read's MFMAs (the last chunk's halo row 2 pr + 3, kx = 2)
constexpr int pair_done(int pr) { return (NCH - 1) * RPC + (2 * pr + 3) * 3 + 2; }
// stream positions of the side work: this wave's DMA piece `it` of the next tile, the residual / gate loads of a
// row pair (the run-time epilogues load `late`, two pairs in flight: their activations and the gate need the registers)
constexpr int dma_at(int it) { return 3 + 9 * it; }
constexpr int res_at(int pr, bool late) { return late ? pair_done(pr) - 12 : 2 * RPC + 2 * pr; }
constexpr int gate_at(int pr) { return pair_done(pr) - 11; }

// every output row receives k-steps 0 .. 35 in order, once each; every read stays inside its chunk image; the DMA
// pieces are all issued before the first store of the tile (the tile loop's vmcnt wait counts on it) and every
// load before its epilogue
constexpr bool schedule_ok() {
    int next[TH] = {}, total = 0;
    for (int n = 0; n < READS; ++n) {
        if (read_pix(n) + TW - 1 >= HPX) return false;
        for (int ky = 0; ky < 3; ++ky)
            if (feeds(n, ky)) {
                const int y = read_row(n) - ky;
                if (kstep(n, ky) != next[y]) return false;
                ++next[y];
                ++total;
            }
    }
    for (int y = 0; y < TH; ++y)
        if (next[y] != NCH * 9) return false;
    if (total != MFMAS) return false;
    for (int pr = 0; pr < TH / 2; ++pr) {
        if (pair_done(pr) >= READS || (pr > 0 && pair_done(pr) <= pair_done(pr - 1))) return false;
        for (int y = 2 * pr; y < 2 * pr + 2; ++y)              // no later read feeds a finished row
            for (int n = pair_done(pr) + 1; n < READS; ++n)
                for (int ky = 0; ky < 3; ++ky)
                    if (feeds(n, ky) && read_row(n) - ky == y) return false;
        for (int late = 0; late < 2; ++late)
            if (res_at(pr, late != 0) < 0 || res_at(pr, late != 0) >= pair_done(pr)) return false;
        if (gate_at(pr) < 0 || gate_at(pr) >= pair_done(pr)) return false;
    }
    for (int it = 0; it < PER; ++it) {
        if (dma_at(it) < 0 || dma_at(it) >= pair_done(0) || (it > 0 && dma_at(it) <= dma_at(it - 1))) return false;
        for (int late = 0; late < 2; ++late)
            if (dma_at(it) >= res_at(0, late != 0)) return false;
    }
    return pair_done(TH / 2 - 1) == READS - 1 && AHEAD >= 1 && AHEAD < RPC;
}
static_assert(schedule_ok(), "ks128 row-rolling schedule");

// Couts of a wave's lanes.  MFMA row m = 4 g + r of wave p is cout 16 p + 8 (g & 1) + 4 (g >> 1) + r, so lanes l
// and l + 32 (g and g + 2) hold adjacent 4-cout groups of the same pixel; after the halves of two output rows are
// swapped between them, lane group g stores couts 16 p + 8 (g & 1) .. + 7 of row 2 pr + (g >> 1).
constexpr int lane_cout(int p, int m) { return 16 * p + 8 * ((m >> 2) & 1) + 4 * (m >> 3) + (m & 3); }
// where the chunk-major packed copy keeps that cout: 16-cout block and row inside it (the packer's
// pipe_cout_perm: row m of block b of a 64-cout tile is cout 32 (b >> 1) + 8 (m >> 2) + 4 (b & 1) + (m & 3))
constexpr int packed_block(int p, int m) { return 2 * (p >> 1) + (m >> 3); }
constexpr int packed_row(int p, int m) { return 4 * (2 * (p & 1) + ((m >> 2) & 1)) + (m & 3); }
constexpr int packed_cout(int blk, int row) {
    return 64 * (blk >> 2) + 32 * ((blk & 3) >> 1) + 8 * (row >> 2) + 4 * (blk & 1) + (row & 3);
}
constexpr bool gather_ok() {
    bool seen[128] = {};
    for (int p = 0; p < NW; ++p)
        for (int m = 0; m < 16; ++m) {
            const int co = lane_cout(p, m);
            if (co < 0 || co >= 128 || seen[co]) return false;
            seen[co] = true;
            if (packed_block(p, m) < 0 || packed_block(p, m) >= 8 || packed_row(p, m) < 0 || packed_row(p, m) >= 16)
                return false;
            if (packed_cout(packed_block(p, m), packed_row(p, m)) != co) return false;
        }
    return true;
}
static_assert(gather_ok(), "ks128 cout gather");

// what a launch must satisfy beyond use_ks128's contract (nullptr: fine), checked before every launch
inline const char* launch_error(int out_h, int out_w, int in_h, int in_w, long long n_frames, long long x_ld_bytes,
                                int y_ld, int y_c0, bool has_res, int r_ld, int r_c0, bool has_gate, int g_ld,
                                int g_c0) {
    if (out_h <= 0 || out_w <= 0 || out_h % TH || out_w % TW) return "frame not a multiple of the 16 x 8 tile";
    if (in_h != out_h || in_w != out_w) return "input and output frames differ";
    if (n_frames <= 0) return "no frames";
    if (n_frames * (out_h / TH) * (out_w / TW) >= (1LL << 31)) return "tile count past 2^31";
    if (x_ld_bytes < 256 || (long long)in_h * in_w * x_ld_bytes >= (1LL << 31)) return "frame past 32-bit offsets";
    // a lane's row-pair offsets are 32-bit: (row * W + col) * ld + cout over the tile's 8 rows
    const long long ldmax = y_ld > r_ld ? (y_ld > g_ld ? y_ld : g_ld) : (r_ld > g_ld ? r_ld : g_ld);
    if ((long long)TH * out_w * ldmax + 128 >= (1LL << 31)) return "tile rows past 32-bit offsets";
    if (y_ld % 8 || y_c0 % 8 || y_ld < 128) return "output not 16-byte aligned";
    if (has_res && (r_ld % 8 || r_c0 % 8)) return "residual not 16-byte aligned";
    if (has_gate && (g_ld % 8 || g_c0 % 8)) return "gate not 16-byte aligned";
    return nullptr;
}

}  // namespace ks128
}  // namespace dbsr
