// tests/cpp/sep_pack_check.cpp - no GPU: the fragment stream of sep_pw_pack (conv_sep.hip) walked lane by lane the way phase 1 of the
// sep_dw3x3_pw_i8 kernels indexes it (channel slice / wave / 64-channel group / k-step / accumulator / k-group, the padded LDS pixel pitch,
// the lane's 16 consecutive output channels), against the OIHW weights of a plain 1x1 convolution, for C = 32 (half a k-step), 64, 96, 1024,
// K with and without a whole last group, and EVERY launch form. Exit status 0 = equal and no walk left the stream, the tile or the output.
// The walk restates the kernel's index arithmetic: a change there must be repeated here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
namespace saber_mi355x {
void sep_pw_pack(const int8_t* w_kc, int k, int c, std::vector<uint8_t>& out);
bool conv_sep_form(int code, int* rows, int* kper, int* waves);
bool conv_sep_form_ok(int code, int c, int k);
size_t conv_sep_lds_bytes(int rows, int c);
}
int main() {
    using namespace saber_mi355x;
    int bad = 0, forms = 0, walks = 0;
    bool splits = false;
    for (int code = 1; code <= 15; ++code) forms += conv_sep_form(code, nullptr, nullptr, nullptr) ? 1 : 0;
    if (forms < 2) { printf("fewer than two forms\n"); return 1; }
    const int shapes[][2] = {{32, 64}, {32, 32}, {64, 128}, {96, 96}, {1024, 1024}, {64, 32}, {512, 1024}};
    for (const auto& sh : shapes) {
        const int C = sh[0], K = sh[1];
        std::vector<int8_t> w((size_t)K * C);
        for (auto& v : w) v = (int8_t)(rand() % 256 - 128);
        std::vector<uint8_t> wp;
        sep_pw_pack(w.data(), K, C, wp);
        const int gall = (K + 63) / 64, cvp = (C + 63) / 64 * 4, pch = cvp + 1, ksn = cvp / 4;
        if (wp.size() != (size_t)gall * ksn * 4 * 1024) { printf("size\n"); return 1; }
        int any = 0;
        for (int code = 1; code <= 15; ++code) {
            int rows, kper, waves;
            if (!conv_sep_form(code, &rows, &kper, &waves) || !conv_sep_form_ok(code, C, K)) continue;
            ++any; ++walks;
            const int NPX = 16 * rows, kgroups = kper ? kper / 64 : gall, nslices = (gall + kgroups - 1) / kgroups;
            if (kper % 64) { printf("kper\n"); return 1; }
            if (nslices > 1) splits = true;
            if (conv_sep_lds_bytes(rows, C) != (size_t)NPX * pch * 16) { printf("lds size\n"); return 1; }
            // the LDS tile as phase 0 leaves it: mid[px][pch chunks], bytes beyond C zero, the padding chunk poisoned
            std::vector<int8_t> mid((size_t)NPX * pch * 16, 77);
            for (int px = 0; px < NPX; ++px)
                for (int c = 0; c < cvp * 16; ++c) mid[((size_t)px * pch) * 16 + c] = c < C ? (int8_t)(rand() % 256 - 128) : 0;
            std::vector<long> got((size_t)NPX * K, -1234567);
            std::vector<int> hits((size_t)NPX * K, 0);
            for (int slice = 0; slice < nslices; ++slice)
                for (int wave = 0; wave < waves; ++wave) {
                    const int g0 = slice * kgroups, g1 = g0 + kgroups < gall ? g0 + kgroups : gall;
                    for (int g = g0 + wave; g < g1; g += waves)
                        for (int j = 0; j < rows; ++j)
                            for (int mf = 0; mf < 4; ++mf) {
                                long acc[16][16] = {};      // [row][col]
                                for (int ks = 0; ks < ksn; ++ks)
                                    for (int kg = 0; kg < 4; ++kg)
                                        for (int col = 0; col < 16; ++col) {
                                            const size_t bo = ((size_t)(j * 16 + col) * pch + ks * 4 + kg) * 16;
                                            if (bo + 16 > mid.size() || ks * 4 + kg >= cvp) { printf("OOB tile\n"); return 1; }
                                            for (int r = 0; r < 16; ++r) {
                                                const int alane = kg * 16 + r;
                                                const size_t wo = ((size_t)g * ksn * 256 + alane + (size_t)(ks * 4 + mf) * 64) * 16;
                                                if (wo + 16 > wp.size()) { printf("OOB w\n"); return 1; }
                                                for (int b = 0; b < 16; ++b) acc[r][col] += (long)(int8_t)wp[wo + b] * mid[bo + b];
                                            }
                                        }
                                for (int kg = 0; kg < 4; ++kg)
                                    for (int col = 0; col < 16; ++col) {
                                        const int cg = g * 64 + kg * 16;
                                        if (cg >= K) continue;
                                        for (int c = 0; c < 4; ++c) {
                                            const size_t o = (size_t)(j * 16 + col) * K + cg + mf * 4 + c;
                                            if (o >= got.size()) { printf("OOB y\n"); return 1; }
                                            got[o] = acc[kg * 4 + c][col];
                                            ++hits[o];
                                        }
                                    }
                            }
                }
            for (int px = 0; px < NPX; ++px)
                for (int k = 0; k < K; ++k) {
                    long a = 0;
                    for (int c = 0; c < C; ++c) a += (long)w[(size_t)k * C + c] * mid[((size_t)px * pch) * 16 + c];
                    if (a != got[(size_t)px * K + k] || hits[(size_t)px * K + k] != 1) {
                        if (bad++ < 5) printf("MISMATCH C %d K %d form %d: pixel %d k %d want %ld got %ld (%d writers)\n", C, K, code, px, k, a, got[(size_t)px * K + k], hits[(size_t)px * K + k]);
                    }
                }
        }
        if (!any) { printf("no form for C %d K %d\n", C, K); return 1; }
    }
    if (!splits) { printf("no form splits K\n"); return 1; }
    printf(bad ? "FAILED %d\n" : "emulation ok (%d forms, %d walks)\n", bad ? bad : forms, walks);
    return bad != 0;
}
