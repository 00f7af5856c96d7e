// Stand-alone host replay of the 128 -> 128 weight-stationary kernel's bookkeeping (csrc/ks128_sched.hpp), built with
// the host sanitizers by tests/test_ks128_sched.py:  c++ -std=c++17 -fsanitize=address,undefined -I<csrc> ...
//  1. one tile through a model of the LDS: the 46 DMA pieces place the halo (lane -> chunk, pixel, k-group), the 120
//     fragment reads fetch it back through frag_slot at the kernel's address arithmetic (base register of
//     pixel offset & 7 + immediate), and the MFMAs of the row-rolling schedule are summed per (row, pixel, cout)
//     in integers against a direct 3x3 convolution -- every array access bounds-checked by the sanitizer;
//  2. the stream positions: DMA before loads before epilogues, the vmcnt count of the tile loop;
//  3. the lane -> cout gather and the lane-pair swap: every (row, pixel, 8-cout group) stored exactly once;
//  4. launch_error's accept / reject cases.
#include "ks128_sched.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace dbsr::ks128;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static unsigned rng_state = 12345u;
static int rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (int)(rng_state >> 24) % 7 - 3; }

int main() {
    // ---- 1. one tile ----
    const int CIN = NCH * 32;
    std::vector<int> halo(CIN * HPX), wt(128 * CIN * 9);
    for (auto& v : halo) v = rnd();
    for (auto& v : wt) v = rnd();
    // LDS model: slot -> (channel base of its 8 values, pixel) or -1 (zeros)
    struct Slot { int ch0, pix; };
    std::vector<Slot> ldsm(BUF_U4, Slot{-2, -2});
    for (int wave = 0; wave < NW; ++wave)
        for (int it = 0; it < PER; ++it) {
            const int item = wave + NW * it < PIECES - 1 ? wave + NW * it : PIECES - 1;
            for (int lane = 0; lane < 64; ++lane) {
                const int qq = item * 16 + (lane >> 2), c = qq / CPX, p = qq - c * CPX, ph = lane & 3;
                const int gg = piece_kgroup(p, ph);
                const int slot = item * 64 + lane;
                CHECK(slot >= 0 && slot < BUF_U4);
                CHECK(c >= 0 && c < NCH);
                ldsm[slot] = p < HPX ? Slot{c * 32 + gg * 8, p} : Slot{-1, -1};
            }
        }
    for (const auto& sl : ldsm) CHECK(sl.ch0 != -2);            // every slot of the buffer is written
    std::vector<long long> acc(TH * TW * 128, 0);
    std::vector<int> steps(TH * TW * 128, 0);
    int reads = 0, mfmas = 0;
    for (int n = 0; n < READS; ++n) {
        const int c = read_chunk(n), imm = read_pix(n);
        const int imm_off = 16 * (c * CH_U4 + 4 * imm);        // the ds_read's offset field
        CHECK(imm_off >= 0 && imm_off < 65536);
        ++reads;
        for (int lane = 0; lane < 64; ++lane) {
            const int g = lane >> 4, col = lane & 15;
            const int ba = 16 * (4 * col + frag_slot(col + (imm & 7), g));   // the base register of imm & 7
            const int byte = ba + imm_off;
            CHECK(byte % 16 == 0 && byte / 16 < BUF_U4);
            const Slot sl = ldsm.at(byte / 16);
            CHECK(sl.pix == col + imm && sl.ch0 == c * 32 + g * 8);
        }
        for (int ky = 0; ky < 3; ++ky) {
            if (!feeds(n, ky)) continue;
            ++mfmas;
            const int y = read_row(n) - ky, tap = 3 * ky + read_kx(n), st = kstep(n, ky);
            CHECK(y >= 0 && y < TH && tap >= 0 && tap < 9 && st == c * 9 + tap);
            for (int col = 0; col < TW; ++col)
                for (int co = 0; co < 128; ++co) {
                    const int o = (y * TW + col) * 128 + co;
                    CHECK(steps[o] == st);                      // the in-order chain
                    ++steps[o];
                    long long s = 0;
                    for (int ch = 0; ch < 32; ++ch)
                        s += (long long)wt[(co * CIN + c * 32 + ch) * 9 + tap] * halo[(c * 32 + ch) * HPX + col + imm];
                    acc[o] += s;
                }
        }
    }
    CHECK(reads == READS && mfmas == MFMAS);
    for (int y = 0; y < TH; ++y)
        for (int col = 0; col < TW; ++col)
            for (int co = 0; co < 128; ++co) {
                long long s = 0;
                for (int ch = 0; ch < CIN; ++ch)
                    for (int ky = 0; ky < 3; ++ky)
                        for (int kx = 0; kx < 3; ++kx)
                            s += (long long)wt[(co * CIN + ch) * 9 + 3 * ky + kx] * halo[ch * HPX + (y + ky) * HW + col + kx];
                CHECK(acc[(y * TW + col) * 128 + co] == s);
                CHECK(steps[(y * TW + col) * 128 + co] == NCH * 9);
            }

    // ---- 2. stream positions ----
    CHECK(schedule_ok());
    for (int late = 0; late < 2; ++late) {
        int last_dma = -1;
        for (int it = 0; it < PER; ++it) last_dma = dma_at(it) > last_dma ? dma_at(it) : last_dma;
        for (int pr = 0; pr < TH / 2; ++pr) {
            CHECK(last_dma < res_at(pr, late != 0) && res_at(pr, late != 0) < pair_done(pr));
            CHECK(last_dma < gate_at(pr) && gate_at(pr) < pair_done(pr));
        }
        // every DMA piece of a tile is older than its TH / 2 stores: the tile loop may leave TH / 2 operations in flight
        int stores_after = 0;
        for (int pr = 0; pr < TH / 2; ++pr) stores_after += pair_done(pr) > last_dma;
        CHECK(stores_after == TH / 2);
    }
    // a row's last MFMA precedes its epilogue and nothing touches it afterwards
    for (int y = 0; y < TH; ++y) {
        int last = -1;
        for (int n = 0; n < READS; ++n)
            for (int ky = 0; ky < 3; ++ky)
                if (feeds(n, ky) && read_row(n) - ky == y) last = n;
        CHECK(last == pair_done(y / 2) - (y % 2 ? 0 : 3));
        CHECK(last <= pair_done(y / 2));
    }

    // ---- 3. cout gather and the lane-pair swap ----
    CHECK(gather_ok() && swizzle_ok());
    std::vector<int> stored(TH * TW * 16, 0);
    for (int p = 0; p < NW; ++p)
        for (int pr = 0; pr < TH / 2; ++pr)
            for (int lane = 0; lane < 64; ++lane) {
                const int g = lane >> 4, col = lane & 15, partner = lane ^ 32, pg = partner >> 4;
                // v[0..3]: lanes < 32 keep their own row 2 pr, lanes >= 32 receive the partner's row 2 pr + 1;
                // v[4..7]: lanes < 32 receive the partner's row 2 pr, lanes >= 32 keep their own row 2 pr + 1
                const int lo_src = lane < 32 ? g : pg, hi_src = lane < 32 ? pg : g;
                const int co8 = 16 * p + 8 * (g & 1), row = 2 * pr + (g >> 1);
                for (int r = 0; r < 4; ++r) {
                    CHECK(lane_cout(p, 4 * lo_src + r) == co8 + r);
                    CHECK(lane_cout(p, 4 * hi_src + r) == co8 + 4 + r);
                }
                ++stored.at((row * TW + col) * 16 + co8 / 8);
            }
    for (int v : stored) CHECK(v == 1);

    // ---- 4. launch checks ----
    CHECK(launch_error(48, 48, 48, 48, 112, 256, 128, 0, true, 128, 0, false, 0, 0) == nullptr);
    CHECK(launch_error(128, 128, 128, 128, 3, 256, 128, 0, true, 128, 0, true, 128, 0) == nullptr);
    CHECK(launch_error(16, 16, 16, 16, 104, 2 * 565, 565 + 7, 8, false, 0, 0, false, 0, 0) != nullptr);   // y_ld % 8
    CHECK(launch_error(48, 56, 48, 56, 112, 256, 128, 0, false, 0, 0, false, 0, 0) != nullptr);           // W % 16
    CHECK(launch_error(44, 48, 44, 48, 112, 256, 128, 0, false, 0, 0, false, 0, 0) != nullptr);           // H % 8
    CHECK(launch_error(48, 48, 46, 46, 112, 256, 128, 0, false, 0, 0, false, 0, 0) != nullptr);           // no padding
    CHECK(launch_error(48, 48, 48, 48, 0, 256, 128, 0, false, 0, 0, false, 0, 0) != nullptr);
    CHECK(launch_error(48, 48, 48, 48, 1LL << 40, 256, 128, 0, false, 0, 0, false, 0, 0) != nullptr);     // tile count
    CHECK(launch_error(4096, 4096, 4096, 4096, 1, 256, 128, 0, false, 0, 0, false, 0, 0) != nullptr);     // 2^32-B frame
    CHECK(launch_error(48, 48, 48, 48, 112, 256, 128, 4, false, 0, 0, false, 0, 0) != nullptr);           // y_c0 % 8
    CHECK(launch_error(48, 48, 48, 48, 112, 256, 128, 0, true, 132, 0, false, 0, 0) != nullptr);          // r_ld % 8
    CHECK(launch_error(48, 48, 48, 48, 112, 256, 128, 0, false, 0, 0, true, 128, 2) != nullptr);          // g_c0 % 8
    CHECK(launch_error(8, 1 << 20, 8, 1 << 20, 1, 256, 1 << 10, 0, false, 0, 0, false, 0, 0) != nullptr); // 32-bit rows

    if (fails) {
        std::printf("%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("ks128 schedule ok: %d reads, %d MFMAs per wave per tile\n", reads, mfmas);
    return 0;
}
