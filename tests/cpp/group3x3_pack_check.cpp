// tests/cpp/group3x3_pack_check.cpp - no GPU: the fragment planes of group3x3_pack (conv_group3x3.hip) walked lane by lane the way the
// g3x3_i8_* kernels index them (tile / slab / row block / step / k-group, the tap decode, the 0x80 shift and 128 * sum(w)), against a
// plain grouped convolution, for every Cg class, both input types, stride 1 | 2 and pad 0 | 1. Exit status 0 = equal.
// The walk restates the kernel's index arithmetic: a change there must be repeated here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
namespace saber_mi355x { void group3x3_pack(const int8_t* q, int c, int cg, std::vector<uint8_t>& out); }
int main() {
    int bad = 0;
    for (int cg : {4, 8, 16, 32, 64}) for (int C : {64, 128, 192}) for (int U8 = 0; U8 < 2; ++U8) for (int stride = 1; stride <= 2; ++stride) for (int pad = 0; pad < 2; ++pad) {
        if (C % cg || C == cg) continue;
        const int PT = 1;      // pixel tiles per wave
        const int N = 2, H = 5, W = 7, OH = (H + 2 * pad - 3) / stride + 1, OW = (W + 2 * pad - 3) / stride + 1, M = N * OH * OW;
        std::vector<int8_t> q((size_t)C * cg * 9);
        for (auto& v : q) v = (int8_t)(rand() % 256 - 128);
        std::vector<uint8_t> x((size_t)N * H * W * C);
        for (auto& v : x) v = (uint8_t)(rand() % 256);
        std::vector<uint8_t> wp;
        saber_mi355x::group3x3_pack(q.data(), C, cg, wp);
        const int NB = cg <= 16 ? 4 : (cg == 32 ? 2 : 1), RPB = 4 / NB, CPT = 4 / NB, STEPS = (9 + NB - 1) / NB, nslab = C / 64;
        if (wp.size() != (size_t)nslab * 4 * STEPS * 1024) { printf("size\n"); return 1; }
        std::vector<int> comp(C, 0);
        for (int k = 0; k < C; ++k) { int s = 0; for (int i = 0; i < cg * 9; ++i) s += q[(size_t)k * cg * 9 + i]; comp[k] = 128 * s; }
        std::vector<long> got((size_t)M * C, -12345);
        const unsigned nwaves = (unsigned)((M + 16 * PT - 1) / (16 * PT) * nslab);
        for (unsigned wave = 0; wave < nwaves; ++wave) {
            const unsigned slab = wave % nslab, tile = wave / nslab;
            for (int t = 0; t < PT; ++t) for (int rb = 0; rb < 4; ++rb) {
                // acc[row][col]
                long acc[16][16] = {};
                for (int st = 0; st < STEPS; ++st) {
                    const int bs = rb / RPB;
                    for (int kg = 0; kg < 4; ++kg) for (int col = 0; col < 16; ++col) {
                        const int p = (int)((tile * PT + t) * 16u) + col;
                        const bool pok = p < M;
                        const int n = p / (OH * OW), rem = p - n * OH * OW, oy = rem / OW, ox = rem - oy * OW;
                        const int tap = st * NB + kg / CPT, ti = (tap * 11) >> 5, tj = tap - 3 * ti;
                        const int iy = oy * stride - pad + ti, ix = ox * stride - pad + tj;
                        int8_t b[16];
                        for (int j = 0; j < 16; ++j) {
                            uint8_t v = 0;
                            if (pok && tap < 9 && iy >= 0 && iy < H && ix >= 0 && ix < W) {
                                const size_t off = (size_t)n * H * W * C + slab * 64 + (kg % CPT) * 16 + ((size_t)iy * W + ix) * C + bs * (64 / NB) + j;
                                if (off >= x.size()) { printf("OOB x\n"); return 1; }
                                v = x[off];
                            }
                            if (U8) v ^= 0x80;
                            b[j] = (int8_t)v;
                        }
                        for (int r = 0; r < 16; ++r) {
                            const int alane = kg * 16 + r;
                            const size_t wo = (size_t)slab * (4 * STEPS * 1024) + (size_t)alane * 16 + (size_t)(rb * STEPS + st) * 1024;
                            if (wo + 16 > wp.size()) { printf("OOB w\n"); return 1; }
                            for (int j = 0; j < 16; ++j) acc[r][col] += (long)(int8_t)wp[wo + j] * b[j];
                        }
                    }
                }
                for (int kg = 0; kg < 4; ++kg) for (int col = 0; col < 16; ++col) {
                    const int p = (int)((tile * PT + t) * 16u) + col;
                    if (p >= M) continue;
                    const int c0 = slab * 64 + rb * 16 + kg * 4;
                    for (int c = 0; c < 4; ++c) got[(size_t)p * C + c0 + c] = acc[kg * 4 + c][col] + (U8 ? comp[c0 + c] : 0);
                }
            }
        }
        for (int p = 0; p < M; ++p) for (int k = 0; k < C; ++k) {
            const int n = p / (OH * OW), rem = p % (OH * OW), oy = rem / OW, ox = rem % OW, g = k / cg;
            long a = 0;
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
                const int iy = oy * stride - pad + i, ix = ox * stride - pad + j;
                if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
                for (int ci = 0; ci < cg; ++ci) {
                    const uint8_t xv = x[((size_t)(n * H + iy) * W + ix) * C + g * cg + ci];
                    a += (long)(U8 ? (int)xv : (int)(int8_t)xv) * q[((size_t)k * cg + ci) * 9 + i * 3 + j];
                }
            }
            if (a != got[(size_t)p * C + k]) { if (bad++ < 5) printf("MISMATCH cg %d C %d u8 %d s %d p %d PT %d: pixel %d k %d want %ld got %ld\n", cg, C, U8, stride, pad, PT, p, k, a, got[(size_t)p * C + k]); }
        }
    }
    printf(bad ? "FAILED %d\n" : "emulation ok\n", bad);
    return bad != 0;
}
