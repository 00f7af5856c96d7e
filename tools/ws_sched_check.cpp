// Stand-alone host replay of the weight-stationary kernel's row-rolling body (csrc/ws_sched.hpp), built with the host
// sanitizers by tests/test_ws_sched.py:  c++ -std=c++17 -fsanitize=address,undefined -I<csrc> ...
// For each of (16 x 16, NCH 2), (16 x 16, NCH 1) and (16 x 8, NCH 2):
//  1. one tile through a model of the LDS: the DMA pieces of the 8 waves place the halo (lane -> chunk, pixel,
//     k-group), every wave's fragment reads fetch it back through frag_slot at the kernel's address arithmetic (base
//     register of pixel offset & 7 + immediate), and the MFMAs of the row-rolling schedule are summed per
//     (row, pixel, cout) in integers against a direct 3x3 convolution -- every array access bounds-checked by the
//     sanitizer;
//  2. the stream positions: DMA pieces before loads before epilogues, the vmcnt count of the tile loop, no MFMA
//     into a row after its epilogue.
#include "ws_sched.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace dbsr::wsr;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static unsigned rng_state = 12345u;
static int rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (int)(rng_state >> 24) % 7 - 3; }

template <int TH, int NCH>
static void replay() {
    using S = Sched<TH, NCH>;
    // ---- 1. one tile ----
    const int CIN = NCH * 32;
    std::vector<int> halo(CIN * S::NQ), wt(WM * CIN * 9);
    for (auto& v : halo) v = rnd();
    for (auto& v : wt) v = rnd();
    // LDS model: slot -> (channel base of its 8 values, pixel) or -1 (zeros)
    struct Slot { int ch0, pix; };
    std::vector<Slot> ldsm(S::STAGE_U4, Slot{-2, -2});
    for (int wave = 0; wave < NW; ++wave)
        for (int it = 0; it < S::PER; ++it) {
            const int item = wave + NW * it < S::ITEMS - 1 ? wave + NW * it : S::ITEMS - 1;
            const int cch = item / S::IN_ITEMS, ii = item % S::IN_ITEMS;
            for (int lane = 0; lane < 64; ++lane) {
                const int p = ii * 16 + (lane >> 2);
                // the kernel forms the lane's k-group from the lane id alone
                const int gg = piece_kgroup(lane >> 2, lane & 3);
                CHECK(gg == piece_kgroup(p, lane & 3));
                const int slot = item * 64 + lane;
                CHECK(slot >= 0 && slot < S::STAGE_U4 && cch >= 0 && cch < NCH);
                ldsm[slot] = p < S::NQ ? Slot{cch * 32 + gg * 8, p} : Slot{-1, -1};
            }
        }
    for (const auto& sl : ldsm) CHECK(sl.ch0 != -2);            // every slot of the buffer is written
    std::vector<long long> acc(TH * TW * WM, 0);
    std::vector<int> steps(TH * TW * WM, 0);
    int reads = 0, mfmas = 0;
    for (int wave = 0; wave < NW; ++wave) {
        const int wc = wave % WC, wp = wave / WC;
        reads = 0;
        mfmas = 0;
        for (int n = 0; n < S::READS; ++n) {
            const int c = S::read_chunk(n), imm = S::read_pix(n);
            const int imm_off = 16 * (c * S::CH_U4 + 4 * imm);  // the ds_read's offset field
            CHECK(imm_off >= 0 && imm_off < 65536);
            ++reads;
            for (int lane = 0; lane < 64; ++lane) {
                const int g = lane >> 4, col = lane & 15;
                const int P0 = wp * S::RPW * S::HW + col;
                const int ba = 16 * (4 * P0 + frag_slot(P0 + (imm & 7), g));   // the base register of imm & 7
                const int byte = ba + imm_off;
                CHECK(byte % 16 == 0 && byte / 16 < S::STAGE_U4);
                const Slot sl = ldsm.at(byte / 16);
                CHECK(sl.pix == P0 + imm && sl.ch0 == c * 32 + g * 8);
            }
            for (int ky = 0; ky < 3; ++ky) {
                if (!S::feeds(n, ky)) continue;
                mfmas += 2;                                     // both 16-cout blocks of the wave
                const int y = S::read_row(n) - ky, tap = 3 * ky + S::read_kx(n), st = S::kstep(n, ky);
                CHECK(y >= 0 && y < S::RPW && tap >= 0 && tap < 9 && st == c * 9 + tap);
                CHECK(n <= S::row_done(y));                     // no MFMA into a row after its epilogue
                const int row = wp * S::RPW + y;
                for (int col = 0; col < TW; ++col)
                    for (int co = wc * 32; co < wc * 32 + 32; ++co) {
                        const int o = (row * TW + col) * WM + co;
                        CHECK(steps[o] == st);                  // the in-order chain
                        ++steps[o];
                        long long s = 0;
                        for (int ch = 0; ch < 32; ++ch)
                            s += (long long)wt[(co * CIN + c * 32 + ch) * 9 + tap] *
                                 halo[(c * 32 + ch) * S::NQ + wp * S::RPW * S::HW + col + imm];
                        acc[o] += s;
                    }
            }
        }
        CHECK(reads == S::READS && mfmas == S::MFMAS);
    }
    for (int y = 0; y < TH; ++y)
        for (int col = 0; col < TW; ++col)
            for (int co = 0; co < WM; ++co) {
                long long s = 0;
                for (int ch = 0; ch < CIN; ++ch)
                    for (int ky = 0; ky < 3; ++ky)
                        for (int kx = 0; kx < 3; ++kx)
                            s += (long long)wt[(co * CIN + ch) * 9 + 3 * ky + kx] *
                                 halo[ch * S::NQ + (y + ky) * S::HW + col + kx];
                CHECK(acc[(y * TW + col) * WM + co] == s);
                CHECK(steps[(y * TW + col) * WM + co] == NCH * 9);
            }

    // ---- 2. stream positions ----
    CHECK(S::schedule_ok());
    int last_dma = -1;
    for (int it = 0; it < S::PER; ++it) {
        CHECK(it == 0 || S::dma_at(it) >= S::dma_at(it - 1));
        last_dma = S::dma_at(it) > last_dma ? S::dma_at(it) : last_dma;
    }
    int stores_after = 0;
    for (int y = 0; y < S::RPW; ++y) {
        CHECK(last_dma < S::res_at(y) && S::res_at(y) < S::row_done(y));
        stores_after += S::row_done(y) > last_dma;
        int last = -1;                                          // the row's last MFMA is at its epilogue's position
        for (int n = 0; n < S::READS; ++n)
            for (int ky = 0; ky < 3; ++ky)
                if (S::feeds(n, ky) && S::read_row(n) - ky == y) last = n;
        CHECK(last == S::row_done(y));
    }
    // every DMA piece of a tile is older than its RPW stores: the tile loop may leave that many operations in flight
    CHECK(stores_after == S::STORES && S::STORES == S::RPW);
    std::printf("ws rows %dx%d nch %d: %d reads, %d MFMAs per wave per tile\n", TW, TH, NCH, reads, mfmas);
}

int main() {
    replay<16, 2>();
    replay<16, 1>();
    replay<8, 2>();
    if (fails) {
        std::printf("%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("ws rows schedule ok\n");
    return 0;
}
