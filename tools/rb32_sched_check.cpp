// Stand-alone host replay of the fused 32-channel ResBlock kernel's row-rolling body (csrc/rb32_sched.hpp), built with
// the host sanitizers by tests/test_rb32_sched.py:  c++ -std=c++17 -fsanitize=address,undefined -I<csrc> ...
// One tile -- a frame of exactly one tile (every edge a frame edge), then the interior tile of a 3 x 3-tile frame --
// goes through a model of the LDS: the DMA pieces of the 8 waves place the input halo (lane -> pixel, k-group; pixels
// outside the frame land zeros), every wave's conv1 stream fetches its fragments back at the kernel's address
// arithmetic (base register of pixel offset & 7 + immediate), sums its MFMAs per (pixel, cout) in integers and writes
// relu(conv1 + b1) -- zeros outside the frame -- into the intermediate image; the conv2 streams read that image and
// their residual items the halo's centre.  Checked against a scalar ResBlock on the whole frame: every conv1 pixel of
// the 34 x 18 region and every conv2 pixel of the tile is produced exactly once, each from taps 0 .. 8 in order, every
// read lands on the slot that holds its pixel and k-group (the sanitizer bounds-checks every access), a row's epilogue
// follows its last MFMA, and a wave's DMA pieces of the next tile all precede its stores.
#include "rb32_sched.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace dbsr::rb32;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static unsigned rng_state = 2463534242u;
static int rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (int)(rng_state >> 24) % 5 - 2; }

constexpr int C = 32;
struct Slot { int pix, kg; long long v[8]; };                  // pix -2: never written; -1: zeros past the image

struct Frame {
    int H, W;
    std::vector<long long> x, mid, out;                         // [y][x][c]
    std::vector<int> w1, w2, b1, b2;                            // [co][ci][tap]
    long long at(const std::vector<long long>& t, int y, int xx, int c) const {
        return (y < 0 || y >= H || xx < 0 || xx >= W) ? 0 : t[((size_t)y * W + xx) * C + c];
    }
    Frame(int H_, int W_) : H(H_), W(W_), x((size_t)H_ * W_ * C), mid(x.size()), out(x.size()), w1(C * C * 9),
                            w2(C * C * 9), b1(C), b2(C) {
        for (auto& v : x) v = rnd();
        for (auto& v : w1) v = rnd();
        for (auto& v : w2) v = rnd();
        for (auto& v : b1) v = rnd();
        for (auto& v : b2) v = rnd();
        for (int pass = 0; pass < 2; ++pass)
            for (int y = 0; y < H; ++y)
                for (int xx = 0; xx < W; ++xx)
                    for (int co = 0; co < C; ++co) {
                        long long s = 0;
                        for (int tap = 0; tap < 9; ++tap)
                            for (int ci = 0; ci < C; ++ci)
                                s += (pass ? w2 : w1)[(co * C + ci) * 9 + tap] *
                                     at(pass ? mid : x, y + tap / 3 - 1, xx + tap % 3 - 1, ci);
                        s += pass ? b2[co] + at(x, y, xx, co) : b1[co];
                        (pass ? out : mid)[((size_t)y * W + xx) * C + co] = s > 0 ? s : 0;
                    }
    }
};

// the 16 x 32 B operand of one MFMA: lane (g, col) fetches k-group g of its pixel
struct BFrag { long long k[16][C]; };

// a fragment read of a wave: lane (g, col) at base pixel P0(col) reads pixel P0 + imm, k-group g of `img`
template <typename P0F>
static BFrag read_frag(const std::vector<Slot>& img, P0F P0, int imm) {
    BFrag b;
    const int imm_off = 64 * imm;                               // the ds_read's offset field
    CHECK(imm_off >= 0 && imm_off < 65536);
    for (int lane = 0; lane < 64; ++lane) {
        const int g = lane >> 4, col = lane & 15, p0 = P0(col);
        const int byte = 16 * (4 * p0 + frag_slot(p0 + (imm & 7), g)) + imm_off;   // base register of imm & 7
        CHECK(byte % 16 == 0);
        const Slot& sl = img.at(byte / 16);
        CHECK(sl.pix == p0 + imm && sl.kg == g);
        for (int e = 0; e < 8; ++e) b.k[col][8 * g + e] = sl.v[e];
    }
    return b;
}

struct Acc {
    long long v[16][C];
    int steps[2];
    bool done;
};
static void mfma(Acc& a, const std::vector<int>& w, const BFrag& b, int tap, int& count) {
    CHECK(!a.done);                                             // no MFMA into a row after its epilogue
    for (int h = 0; h < 2; ++h) {
        CHECK(a.steps[h] == tap);                               // the in-order chain from zero
        ++a.steps[h];
        ++count;
    }
    for (int col = 0; col < 16; ++col)
        for (int co = 0; co < C; ++co) {
            long long s = 0;
            for (int ci = 0; ci < C; ++ci) s += w[(co * C + ci) * 9 + tap] * b.k[col][ci];
            a.v[col][co] = (tap == 0 ? 0 : a.v[col][co]) + s;
        }
}

static void replay(int H, int W, int y0, int x0) {
    const Frame f(H, W);
    // ---- the input halo by DMA ----
    std::vector<Slot> lin(IN_U4, Slot{-2, -2, {}});
    for (int wave = 0; wave < NW; ++wave)
        for (int it = 0; it < PER; ++it) {
            const int piece = wave + NW * it < IN_PIECES - 1 ? wave + NW * it : IN_PIECES - 1;
            for (int lane = 0; lane < 64; ++lane) {
                const int p = piece * 16 + (lane >> 2), gg = piece_kgroup(p, lane & 3);
                Slot sl{p < IPX ? p : -1, gg, {}};
                const int hy = y0 - 2 + p / IW, hx = x0 - 2 + p % IW;
                for (int e = 0; e < 8; ++e) sl.v[e] = p < IPX ? f.at(f.x, hy, hx, 8 * gg + e) : 0;
                lin.at(piece * 64 + lane) = sl;
            }
        }
    for (const auto& sl : lin) CHECK(sl.pix != -2);
    for (int p = 0; p < IPX; ++p)
        for (int g = 0; g < 4; ++g) CHECK(lin.at(4 * p + frag_slot(p, g)).pix == p && lin.at(4 * p + frag_slot(p, g)).kg == g);

    // ---- conv1 ----
    std::vector<Slot> lmid(MID_U4, Slot{-2, -2, {}});
    std::vector<int> made1(MPX, 0);
    int reads1[NW] = {}, mfmas1[NW] = {};
    auto mid_write = [&](const Acc& a, int col, int r, int c) {
        const int p = r * MW + c, fy = y0 - 1 + r, fx = x0 - 1 + c;
        CHECK(a.steps[0] == 9 && a.steps[1] == 9);              // the epilogue comes after the last MFMA
        const bool inside = fy >= 0 && fy < H && fx >= 0 && fx < W;
        ++made1.at(p);
        for (int g = 0; g < 4; ++g) {
            Slot sl{p, g, {}};
            for (int e = 0; e < 8; ++e) {
                const long long s = a.v[col][8 * g + e] + f.b1[8 * g + e];
                sl.v[e] = inside ? (s > 0 ? s : 0) : 0;
                CHECK(sl.v[e] == f.at(f.mid, fy, fx, 8 * g + e));
            }
            lmid.at(4 * p + frag_slot(p, g)) = sl;
        }
    };
    auto band1 = [&](auto rows, int wave) {
        using S = decltype(rows);
        const int R0 = c1_row0(wave_band(wave)), c0 = 16 * wave_strip(wave);
        std::vector<Acc> acc(S::NR, Acc{{}, {0, 0}, false});
        for (int n = 0; n < S::READS; ++n) {
            const int imm = S::read_row(n) * IW + S::read_kx(n);
            CHECK(imm == rows_pix<S::NR>(n, IW));
            const BFrag b = read_frag(lin, [&](int col) { return R0 * IW + c0 + col; }, imm);
            ++reads1[wave];
            for (int ky = 0; ky < 3; ++ky)
                if (S::feeds(n, ky)) mfma(acc.at(S::read_row(n) - ky), f.w1, b, S::tap(n, ky), mfmas1[wave]);
            for (int r = 0; r < S::NR; ++r)
                if (n == S::row_done(r)) {
                    for (int col = 0; col < 16; ++col) mid_write(acc[r], col, R0 + r, c0 + col);
                    acc[r].done = true;
                }
        }
        for (const auto& a : acc) CHECK(a.done);
    };
    for (int wave = 0; wave < NW; ++wave) {
        CHECK(c1_rows(wave_band(wave)) == 5 || c1_rows(wave_band(wave)) == 4);
        if (c1_rows(wave_band(wave)) == 5) band1(Rows<5>{}, wave);
        else band1(Rows<4>{}, wave);
        const int eg = edge_group(wave);
        if (eg < 0) continue;
        Acc a{{}, {0, 0}, false};
        auto epx = [&](int col) { return 16 * eg + col < EDGE_PX - 1 ? 16 * eg + col : EDGE_PX - 1; };
        for (int tap = 0; tap < EDGE_READS; ++tap) {
            const BFrag b =
                read_frag(lin, [&](int col) { return edge_row(epx(col)) * IW + edge_col(epx(col)); }, edge_pix(tap));
            ++reads1[wave];
            mfma(a, f.w1, b, tap, mfmas1[wave]);
        }
        for (int col = 0; col < 16; ++col)
            if (16 * eg + col < EDGE_PX) mid_write(a, col, edge_row(epx(col)), edge_col(epx(col)));
    }
    for (int p = 0; p < MPX; ++p) CHECK(made1[p] == 1);          // every pixel of the 34 x 18 region exactly once

    // ---- conv2 ----
    using S2 = Conv2;
    using R2 = Rows<S2::NR>;
    std::vector<int> made2(TW * TH, 0);
    int reads2 = 0, mfmas2 = 0, stores = 0;
    for (int wave = 0; wave < NW; ++wave) {
        const int R0 = S2::NR * wave_band(wave), c0 = 16 * wave_strip(wave);
        std::vector<Acc> acc(S2::NR, Acc{{}, {0, 0}, false});
        reads2 = mfmas2 = stores = 0;
        for (int n = 0; n < S2::ITEMS; ++n) {
            ++reads2;
            if (S2::is_res(n)) {
                const int y = S2::res_row(n);
                CHECK(n == S2::epilogue_at(y));
                const BFrag rq = read_frag(lin, [&](int col) { return (R0 + 2) * IW + c0 + 2 + col; }, y * IW);
                Acc& a = acc.at(y);
                CHECK(a.steps[0] == 9 && a.steps[1] == 9 && !a.done);
                a.done = true;
                ++stores;
                for (int col = 0; col < 16; ++col) {
                    ++made2.at((R0 + y) * TW + c0 + col);
                    for (int co = 0; co < C; ++co) {
                        const long long s = a.v[col][co] + f.b2[co] + rq.k[col][co];
                        CHECK((s > 0 ? s : 0) == f.at(f.out, y0 + R0 + y, x0 + c0 + col, co));
                    }
                }
            } else {
                const int fr = S2::frag(n);
                const BFrag b = read_frag(lmid, [&](int col) { return R0 * MW + c0 + col; }, rows_pix<S2::NR>(fr, MW));
                for (int ky = 0; ky < 3; ++ky)
                    if (R2::feeds(fr, ky)) mfma(acc.at(R2::read_row(fr) - ky), f.w2, b, R2::tap(fr, ky), mfmas2);
            }
        }
        CHECK(reads2 == S2::ITEMS && mfmas2 == S2::MFMAS);
        // the wave's order of vector-memory operations in a tile: PER DMA pieces (before conv1), then its stores
        // (conv2's epilogues, after the second barrier's drain): the first barrier may leave STORES in flight
        CHECK(stores == STORES);
    }
    for (int p = 0; p < TW * TH; ++p) CHECK(made2[p] == 1);      // every pixel of the tile exactly once

    int total1 = 0;
    for (int wave = 0; wave < NW; ++wave) {
        CHECK(reads1[wave] == c1_reads(wave) && mfmas1[wave] == c1_mfmas(wave) && mfmas1[wave] <= 90);
        total1 += mfmas1[wave];
    }
    CHECK(total1 == 39 * 18);
    std::printf("rb32 rows frame %dx%d tile (%d, %d):", W, H, x0, y0);
    for (int wave = 0; wave < NW; ++wave)
        std::printf(" w%d %d+%d/%d+%d", wave, reads1[wave], reads2, mfmas1[wave], mfmas2);
    std::printf(" (LDS reads conv1+conv2 / MFMAs conv1+conv2 per wave per tile)\n");
}

int main() {
    replay(TH, TW, 0, 0);
    replay(3 * TH, 3 * TW, TH, TW);
    int most = 0;
    for (int w = 0; w < NW; ++w) most = c1_reads(w) + Conv2::ITEMS > most ? c1_reads(w) + Conv2::ITEMS : most;
    std::printf("rb32 rows: at most %d LDS reads for %d MFMAs per wave per tile\n", most, 90 + Conv2::MFMAS);
    if (fails) {
        std::printf("%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("rb32 rows schedule ok\n");
    return 0;
}
