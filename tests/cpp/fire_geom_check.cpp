// tests/cpp/fire_geom_check.cpp - no GPU: conv_fire_geom (conv_fire.hip) accepts and rejects what kernels.h states, and the form table's
// geometry is what the kernel indexes: S in {16, 32, 48, 64}; C, E1, E3 multiples of 16 in 16 .. 512; codes 1 (4 x 16) and 2 (2 x 16) only;
// tile, halo, fragment counts, tile counts of ragged images and the LDS footprint (xin pitch = k-steps * 4 + 1 chunks, sbuf pitch 5 chunks)
// below the limit; every halo position phase 2 reads lies inside the halo. Exit status 0 = as stated.
#include <cstdio>
#include <cstddef>
namespace saber_mi355x {
struct FireGeom { int th, tw, nf, hh, hw, hpf, tiles_x, tiles_y; size_t lds; };
bool conv_fire_geom(int code, int c, int s, int e1, int e3, int h, int w, FireGeom* g);
const char* conv_fire_form_name(int code);
}
using namespace saber_mi355x;

int main() {
    int bad = 0, accepted = 0;
    auto expect = [&](bool got, bool want, const char* what, int a, int b) {
        if (got != want) { printf("%s (%d, %d): got %d\n", what, a, b, (int)got); ++bad; }
    };
    for (int code = -1; code <= 4; ++code)
        for (int s = 0; s <= 80; s += 8)
            for (int c = 0; c <= 528; c += 8)
                for (int e = 8; e <= 528; e += 104) {
                    const bool in_range = (code == 1 || code == 2) && (s == 16 || s == 32 || s == 48 || s == 64) && c >= 16 && c <= 512 && c % 16 == 0 &&
                                          e >= 16 && e <= 512 && e % 16 == 0;
                    FireGeom g;
                    const bool ok = conv_fire_geom(code, c, s, e, 16 + (e % 16 ? 0 : 32), 13, 33, &g);
                    expect(ok, in_range, "range", code * 1000 + s, c);
                    if (!ok) continue;
                    ++accepted;
                    const int rows = code == 1 ? 4 : 2, kss = (c + 63) / 64;
                    if (g.th != rows || g.tw != 16 || g.nf != rows || g.nf * 16 != g.th * g.tw || g.hh != rows + 2 || g.hw != 18 ||
                        g.hpf != (g.hh * g.hw + 15) / 16 || g.tiles_x != 3 || g.tiles_y != (13 + rows - 1) / rows ||
                        g.lds != (size_t)16 * g.hpf * 16 * (kss * 4 + 1 + 5) || g.lds > 80 * 1024 - 64) { printf("geometry code %d c %d\n", code, c); ++bad; }
                    for (int p = 0; p < g.nf * 16; ++p)      // phase 2: tile pixel p reads halo rows ty .. ty + 2, columns tx .. tx + 2
                        if ((p / g.tw + 2) * g.hw + p % g.tw + 2 >= g.hh * g.hw) { printf("halo read outside, code %d p %d\n", code, p); ++bad; }
                }
    expect(conv_fire_geom(1, 64, 16, 64, 64, 0, 5, nullptr), false, "empty image", 0, 5);
    expect(conv_fire_geom(1, 64, 16, 64, 72, 5, 5, nullptr), false, "E3 % 16", 64, 72);
    expect(conv_fire_geom(2, 512, 64, 256, 256, 1, 1, nullptr), true, "fire9 at 1x1", 1, 1);
    if (conv_fire_form_name(1)[0] == 0 || conv_fire_form_name(2)[0] == 0 || conv_fire_form_name(3)[0] != 0 || conv_fire_form_name(0)[0] != 0) { printf("form names\n"); ++bad; }
    if (!bad && accepted > 100) printf("fire geom ok: %d accepted shapes walked\n", accepted);
    return bad ? 1 : 0;
}
