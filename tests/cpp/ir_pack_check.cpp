// tests/cpp/ir_pack_check.cpp - no GPU: the two fragment streams of ir_pack (conv_ir.hip) walked lane by lane the way the
// ir_expand_dw_project_i8 kernels index them - the expand stream per chunk of 64 expanded channels / halo fragment / k-step / accumulator /
// k-group with the padded xin pixel pitch, the project stream per accumulator unit (64 output channels x one pixel fragment, wave w owns
// units w, w + 4, ...) one k-step per chunk with the 5-chunk mid pitch - against the OIHW weights of two plain 1x1 convolutions, for
// (Cin, Ce, Cout) = (16, 96, 24), (24, 144, 24), (160, 960, 320) and every launch form of a 7 x 7 and a 14 x 20 image. Every output has one
// writer, every byte of the streams beyond K and beyond C is zero, no walk leaves a stream, an LDS buffer or the output.
// Exit status 0 = equal. The walk restates the kernel's index arithmetic: a change there must be repeated here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
namespace saber_mi355x {
struct IrGeom { int th, tw, nf, hh, hw, hpf, tiles_x, tiles_y; size_t lds; };
void ir_pack(const int8_t* w_kc, int k, int c, std::vector<uint8_t>& out);
bool conv_ir_geom(int code, int cin, int ce, int cout, int oh, int ow, int stride, IrGeom* g);
const char* conv_ir_form_name(int code);
}
using namespace saber_mi355x;

// the stream's layout: [group][k-step][accumulator][lane][16]; every byte either one weight or a zero of the padding
static int check_layout(const std::vector<int8_t>& w, int K, int C, const std::vector<uint8_t>& s) {
    const int groups = (K + 63) / 64, ksn = (C + 63) / 64;
    if (s.size() != (size_t)groups * ksn * 4 * 1024) { printf("stream size K %d C %d\n", K, C); return 1; }
    std::vector<int> hits((size_t)K * C, 0);
    for (int g = 0; g < groups; ++g)
        for (int ks = 0; ks < ksn; ++ks)
            for (int mf = 0; mf < 4; ++mf)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 16; ++j) {
                        const int rho = lane & 15, kq = lane >> 4;
                        const int ch = g * 64 + (rho >> 2) * 16 + mf * 4 + (rho & 3), c = ks * 64 + kq * 16 + j;
                        const int8_t v = (int8_t)s[((((size_t)g * ksn + ks) * 4 + mf) * 64 + lane) * 16 + j];
                        if (ch >= K || c >= C) {
                            if (v != 0) { printf("nonzero padding K %d C %d at channel %d input %d\n", K, C, ch, c); return 1; }
                        } else {
                            if (v != w[(size_t)ch * C + c]) { printf("wrong weight K %d C %d at channel %d input %d\n", K, C, ch, c); return 1; }
                            ++hits[(size_t)ch * C + c];
                        }
                    }
    for (int h : hits)
        if (h != 1) { printf("a weight with %d places K %d C %d\n", h, K, C); return 1; }
    return 0;
}

int main() {
    int bad = 0, walks = 0, forms = 0;
    for (int code = 1; code <= 7; ++code) forms += conv_ir_form_name(code)[0] ? 1 : 0;
    if (forms < 2) { printf("fewer than two forms\n"); return 1; }
    const int shapes[][3] = {{16, 96, 24}, {24, 144, 24}, {160, 960, 320}};
    const int images[][2] = {{7, 7}, {14, 20}};
    for (const auto& sh : shapes) {
        const int Cin = sh[0], Ce = sh[1], Cout = sh[2];
        std::vector<int8_t> we((size_t)Ce * Cin), wp((size_t)Cout * Ce);
        for (auto& v : we) v = (int8_t)(rand() % 256 - 128);
        for (auto& v : wp) v = (int8_t)(rand() % 256 - 128);
        std::vector<uint8_t> se, sp;
        ir_pack(we.data(), Ce, Cin, se);
        ir_pack(wp.data(), Cout, Ce, sp);
        if (check_layout(we, Ce, Cin, se) || check_layout(wp, Cout, Ce, sp)) return 1;
        const int kse = (Cin + 63) / 64, pchx = kse * 4 + 1, ksp = (Ce + 63) / 64, G = (Cout + 63) / 64, PCH = 5, NW = 4, MAXU = 5;
        for (const auto& im : images)
            for (int stride = 1; stride <= 2; ++stride)
                for (int code = 1; code <= 7; ++code) {
                    IrGeom g;
                    const int oh = (im[0] - 1) / stride + 1, ow = (im[1] - 1) / stride + 1;
                    if (!conv_ir_geom(code, Cin, Ce, Cout, oh, ow, stride, &g)) continue;
                    ++walks;
                    const int HP = g.hh * g.hw, HPP = g.hpf * 16, NPX = g.nf * 16, nunits = G * g.nf;
                    if (HPP < HP || NPX < g.th * g.tw || nunits > NW * MAXU || g.tiles_x * g.tw < ow || g.tiles_y * g.th < oh ||
                        g.hh != (g.th - 1) * stride + 3 || g.hw != (g.tw - 1) * stride + 3 ||
                        g.lds != (size_t)16 * ((size_t)HPP * pchx + (size_t)HPP * PCH + (size_t)NPX * PCH) || g.lds > 80 * 1024) {
                        printf("geometry of form %d\n", code);
                        return 1;
                    }
                    // ---- the expand stream: xin as phase 0 leaves it (bytes beyond Cin zero, the padding chunk poisoned) -> ebuf[hp][64] per chunk
                    std::vector<int8_t> xin((size_t)HPP * pchx * 16, 77);
                    for (int hp = 0; hp < HPP; ++hp)
                        for (int c = 0; c < kse * 64; ++c) xin[(size_t)hp * pchx * 16 + c] = c < Cin ? (int8_t)(rand() % 256 - 128) : 0;
                    std::vector<long> e((size_t)HPP * ksp * 64, -1234567);
                    std::vector<int> eh((size_t)HPP * ksp * 64, 0);
                    for (int cc = 0; cc < ksp; ++cc)
                        for (int wave = 0; wave < NW; ++wave)
                            for (int f = wave; f < g.hpf; f += NW)
                                for (int mf = 0; mf < 4; ++mf) {
                                    long acc[16][16] = {};      // [row][col]
                                    for (int ks = 0; ks < kse; ++ks)
                                        for (int kg = 0; kg < 4; ++kg)
                                            for (int col = 0; col < 16; ++col) {
                                                const size_t bo = ((size_t)(f * 16 + col) * pchx + ks * 4 + kg) * 16;
                                                if (bo + 16 > xin.size()) { printf("OOB xin\n"); return 1; }
                                                for (int r = 0; r < 16; ++r) {
                                                    const int alane = kg * 16 + r;
                                                    const size_t wo = ((size_t)cc * kse * 256 + alane + (size_t)(ks * 4 + mf) * 64) * 16;
                                                    if (wo + 16 > se.size()) { printf("OOB expand stream\n"); return 1; }
                                                    for (int b = 0; b < 16; ++b) acc[r][col] += (long)(int8_t)se[wo + b] * xin[bo + b];
                                                }
                                            }
                                    for (int kg = 0; kg < 4; ++kg)
                                        for (int col = 0; col < 16; ++col)
                                            for (int c = 0; c < 4; ++c) {
                                                const size_t o = ((size_t)(f * 16 + col) * ksp + cc) * 64 + kg * 16 + mf * 4 + c;
                                                if (o >= e.size()) { printf("OOB ebuf\n"); return 1; }
                                                e[o] = acc[kg * 4 + c][col];
                                                ++eh[o];
                                            }
                                }
                    for (int hp = 0; hp < HPP; ++hp)
                        for (int k = 0; k < ksp * 64; ++k) {
                            long a = 0;
                            if (k < Ce)
                                for (int c = 0; c < Cin; ++c) a += (long)we[(size_t)k * Cin + c] * xin[(size_t)hp * pchx * 16 + c];
                            const size_t o = (size_t)hp * ksp * 64 + k;
                            if (a != e[o] || eh[o] != 1) {
                                if (bad++ < 5) printf("EXPAND MISMATCH %d/%d/%d form %d: pixel %d k %d want %ld got %ld (%d writers)\n", Cin, Ce, Cout, code, hp, k, a, e[o], eh[o]);
                            }
                        }
                    // ---- the project stream: mid[px][64] per chunk (channels beyond Ce zero, the padding chunk poisoned), accumulated across chunks
                    std::vector<int8_t> mid((size_t)ksp * NPX * PCH * 16, 77);
                    for (int cc = 0; cc < ksp; ++cc)
                        for (int px = 0; px < NPX; ++px)
                            for (int c = 0; c < 64; ++c) mid[(((size_t)cc * NPX + px) * PCH) * 16 + c] = cc * 64 + c < Ce ? (int8_t)(rand() % 256 - 128) : 0;
                    std::vector<long> got((size_t)NPX * Cout, -1234567);
                    std::vector<int> hits((size_t)NPX * Cout, 0);
                    for (int wave = 0; wave < NW; ++wave)
                        for (int ui = 0; ui < MAXU; ++ui) {
                            const int u = wave + ui * NW;
                            if (u >= nunits) continue;
                            const int gg = u / g.nf, f = u - gg * g.nf;
                            for (int mf = 0; mf < 4; ++mf) {
                                long acc[16][16] = {};
                                for (int cc = 0; cc < ksp; ++cc)
                                    for (int kg = 0; kg < 4; ++kg)
                                        for (int col = 0; col < 16; ++col) {
                                            const size_t bo = (((size_t)cc * NPX + f * 16 + col) * PCH + kg) * 16;
                                            if (bo + 16 > mid.size()) { printf("OOB mid\n"); return 1; }
                                            for (int r = 0; r < 16; ++r) {
                                                const int alane = kg * 16 + r;
                                                const size_t wo = (((size_t)gg * ksp + cc) * 256 + alane + (size_t)mf * 64) * 16;
                                                if (wo + 16 > sp.size()) { printf("OOB project stream\n"); return 1; }
                                                for (int b = 0; b < 16; ++b) acc[r][col] += (long)(int8_t)sp[wo + b] * mid[bo + b];
                                            }
                                        }
                                for (int kg = 0; kg < 4; ++kg)
                                    for (int col = 0; col < 16; ++col) {
                                        const int cg = gg * 64 + kg * 16;
                                        if (cg >= Cout) continue;
                                        for (int c = 0; c < 4; ++c) {
                                            const int ch = cg + mf * 4 + c;
                                            if (ch >= Cout) continue;      // Cout % 16 == 8: the half that is not stored
                                            const size_t o = (size_t)(f * 16 + col) * Cout + ch;
                                            if (o >= got.size()) { printf("OOB y\n"); return 1; }
                                            got[o] = acc[kg * 4 + c][col];
                                            ++hits[o];
                                        }
                                    }
                            }
                        }
                    for (int px = 0; px < NPX; ++px)
                        for (int k = 0; k < Cout; ++k) {
                            long a = 0;
                            for (int c = 0; c < Ce; ++c) a += (long)wp[(size_t)k * Ce + c] * mid[(((size_t)(c / 64) * NPX + px) * PCH) * 16 + c % 64];
                            if (a != got[(size_t)px * Cout + k] || hits[(size_t)px * Cout + k] != 1) {
                                if (bad++ < 5) printf("PROJECT MISMATCH %d/%d/%d form %d: pixel %d k %d want %ld got %ld (%d writers)\n", Cin, Ce, Cout, code, px, k, a, got[(size_t)px * Cout + k], hits[(size_t)px * Cout + k]);
                            }
                        }
                }
    }
    if (walks < 12) { printf("only %d walks\n", walks); return 1; }
    printf(bad ? "FAILED %d\n" : "emulation ok (%d forms, %d walks)\n", bad ? bad : forms, walks);
    return bad != 0;
}
