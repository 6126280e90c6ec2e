// tests/cpp/deconv_pack_check.cpp - no GPU: a walk of the bf16-plane deconv kernel's weight stream (deconv_b3_pack, anakin_amd/csrc/deconv.hip).
// The layout is restated here from its description - [phase][tap][32-deep slab][16-channel tile][plane][lane] x 8 bf16, phase = 2 (a mod 2) +
// (b mod 2), taps row-major inside a phase, lane (row r = lane & 15, group g = lane >> 4) element j = w[ci = 32 s + 8 g + j][ko = 16 tile + r][a][b] -
// and every (phase, tap, c, k) weight must be found exactly once in each plane, the three planes summing to the f32 weight exactly.
// Also deconv_b3_ok's range against the header's words. Exit status 0 = as stated.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
namespace saber_mi355x {
int deconv_b3_taps(int ks, int (*ab)[2]);
void deconv_b3_pack(const float* w_ckab, int c, int k, int ks, std::vector<uint8_t>& out);
bool deconv_b3_ok(int n, int h, int w, int c, int k, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int group);
bool deconv_b3_form(int form, int* th);
}
using namespace saber_mi355x;

static float bf(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float v;
    std::memcpy(&v, &u, 4);
    return v;
}

int main() {
    int bad = 0;
    long walked = 0;
    const int shapes[][3] = {{32, 16, 2}, {64, 48, 4}, {32, 32, 3}, {96, 80, 4}, {128, 64, 2}};
    for (const auto& sh : shapes) {
        const int c = sh[0], k = sh[1], ks = sh[2];
        std::vector<float> w((size_t)c * k * ks * ks);
        uint32_t st = 12345u + c * 7 + k * 3 + ks;
        for (float& v : w) {      // full 24-bit mantissas over a few binades, both signs
            st = st * 1664525u + 1013904223u;
            const uint32_t u = ((st >> 31) << 31) | ((120u + ((st >> 8) & 7u)) << 23) | (st & 0x7fffffu);
            std::memcpy(&v, &u, 4);
        }
        std::vector<uint8_t> out;
        deconv_b3_pack(w.data(), c, k, ks, out);
        // the tap order, restated
        std::vector<int> ta, tb;
        for (int rh = 0; rh < 2; ++rh)
            for (int rw = 0; rw < 2; ++rw)
                for (int a = rh; a < ks; a += 2)
                    for (int b = rw; b < ks; b += 2) { ta.push_back(a); tb.push_back(b); }
        int ab[16][2];
        const int ntap = deconv_b3_taps(ks, ab);
        if (ntap != ks * ks || (int)ta.size() != ntap) { printf("tap count %d for k %d\n", ntap, ks); return 1; }
        for (int t = 0; t < ntap; ++t)
            if (ab[t][0] != ta[t] || ab[t][1] != tb[t]) { printf("tap order k %d t %d\n", ks, t); ++bad; }
        const int nslab = c / 32, ntile = k / 16;
        if (out.size() != (size_t)ntap * nslab * ntile * 3 * 64 * 16) { printf("stream size c %d k %d ks %d: %zu\n", c, k, ks, out.size()); return 1; }
        const uint16_t* o = (const uint16_t*)out.data();
        std::vector<int> seen[3];
        for (auto& s : seen) s.assign(w.size(), 0);
        for (int t = 0; t < ntap; ++t)
            for (int s = 0; s < nslab; ++s)
                for (int tile = 0; tile < ntile; ++tile)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const int ci = 32 * s + 8 * (lane >> 4) + j, ko = 16 * tile + (lane & 15);
                            const size_t wi = (((size_t)ci * k + ko) * ks + ta[t]) * ks + tb[t];
                            const size_t frag = ((size_t)(t * nslab + s) * ntile + tile) * 3;
                            float p[3];
                            for (int pl = 0; pl < 3; ++pl) {
                                p[pl] = bf(o[((frag + pl) * 64 + lane) * 8 + j]);
                                ++seen[pl][wi];
                            }
                            // x = h + m + l exactly; h the nearest bf16 of x, m of the rest
                            if ((double)p[0] + (double)p[1] + (double)p[2] != (double)w[wi]) { if (bad < 8) printf("planes of w[%zu] do not sum to it\n", wi); ++bad; }
                            const float a0 = p[0] < 0 ? -p[0] : p[0], a1 = p[1] < 0 ? -p[1] : p[1], a2 = p[2] < 0 ? -p[2] : p[2];
                            if (a0 == 0.f || a1 > a0 / 128.f || a2 > a0 / 16384.f) { if (bad < 8) printf("plane magnitudes of w[%zu]\n", wi); ++bad; }
                            ++walked;
                        }
        for (int pl = 0; pl < 3; ++pl)
            for (size_t i = 0; i < w.size(); ++i)
                if (seen[pl][i] != 1) { if (bad < 8) printf("c %d k %d ks %d: weight %zu is in plane %d %d times\n", c, k, ks, i, pl, seen[pl][i]); ++bad; }
    }
    // eligibility, as include/saber_hip.h words it
    for (int ks = 1; ks <= 5; ++ks)
        for (int pad = 0; pad <= 4; ++pad)
            for (int stride = 1; stride <= 3; ++stride)
                for (int c = 16; c <= 96; c += 16)
                    for (int k = 8; k <= 48; k += 8)
                        for (int group = 1; group <= 2; ++group)
                            for (int dil = 1; dil <= 2; ++dil) {
                                const bool want = group == 1 && dil == 1 && stride == 2 && ks >= 2 && ks <= 4 && pad <= ks - 1 && c % 32 == 0 && k % 16 == 0;
                                if (deconv_b3_ok(2, 5, 7, c, k, ks, ks, stride, stride, pad, pad, dil, dil, group) != want) { printf("range ks %d pad %d stride %d c %d k %d\n", ks, pad, stride, c, k); ++bad; }
                            }
    if (deconv_b3_ok(1, 5, 5, 32, 16, 2, 3, 2, 2, 0, 0, 1, 1, 1) || deconv_b3_ok(1, 5, 5, 32, 16, 3, 3, 2, 1, 0, 0, 1, 1, 1)) { printf("per-axis geometry accepted\n"); ++bad; }
    int th = 0;
    if (!deconv_b3_form(1, &th) || th != 4 || !deconv_b3_form(2, &th) || th != 2 || deconv_b3_form(0, &th) || deconv_b3_form(3, &th)) { printf("forms\n"); ++bad; }
    if (!bad) printf("deconv pack ok: %ld stream elements walked\n", walked);
    return bad ? 1 : 0;
}
