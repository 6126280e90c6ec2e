// tests/cpp/resize_table_check.cpp - no GPU: the host side of saber_hip_resize_create, resize_axis_table (anakin_amd/csrc/resize.hip), printed
// for tests/test_resize_cpu.py to compare bit for bit with tests/resize_util.py's restatement of the reference's index arithmetic.
// Arguments in groups of five: mode in out scale_bits(hex, the float's bits) sizes_given. Per group one line
//   "table <k> <ok>" followed by out lines "<i0> <i1> <frac bits, hex>" when ok. Without arguments: the refusals, exit status 0 = as stated.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
namespace saber_mi355x {
struct ResizeTap {
    int i0, i1;
    float frac;
    int pad;
};
bool resize_axis_table(int mode, int in, int out, float scale, bool sizes_given, std::vector<ResizeTap>& t);
bool resize_rows_ok(int c, int in_nchw, int out_nchw);
bool resize_x2_tables_ok(bool nearest, int in, const std::vector<ResizeTap>& t);
}
using namespace saber_mi355x;

int main(int argc, char** argv) {
    std::vector<ResizeTap> t;
    if (argc == 1) {
        int bad = 0;
        for (int mode : {0, 3}) bad += resize_axis_table(mode, 5, 1, 0.f, true, t);      // the reference divides by out - 1
        bad += resize_axis_table(2, 5, 4, 0.f, false, t) + resize_axis_table(2, 5, 4, -1.f, false, t);      // mode 2: no positive scale
        bad += resize_axis_table(2, 2, 4, 1.f, false, t);                  // scale 1 over 4 outputs of 2 inputs: i0 = 2, 3 are beyond the input
        bad += resize_axis_table(0, 0, 4, 0.f, true, t) + resize_axis_table(1, 4, 0, 0.f, true, t) + resize_axis_table(4, 4, 4, 0.f, true, t);
        bad += !resize_axis_table(1, 7, 1, 0.f, true, t) || t.size() != 1 || t[0].i0 != 3 || t[0].i1 != 4 || t[0].frac != 0.f;      // mode 1 to one row: the middle
        bad += !resize_axis_table(2, 5, 12, 2.5f, false, t) || t[11].i0 != 4 || t[11].i1 != 5;      // the zero tap at the edge keeps its index
        bad += !resize_rows_ok(8, 0, 0) || resize_rows_ok(6, 0, 0) || resize_rows_ok(8, 1, 0) || resize_rows_ok(8, 0, 1);
        // form 2's condition: an x2 table in modes 1 and 3 keeps every tap within one row of o / 2, at small and large sizes; others do not pass
        for (int in : {1, 2, 3, 7, 112, 1460}) {
            bad += !resize_axis_table(1, in, 2 * in, 0.f, true, t) || !resize_x2_tables_ok(false, in, t);
            bad += resize_x2_tables_ok(false, in + 1, t);                                     // not 2 x in entries
            if (in <= 112) bad += !resize_axis_table(3, in, 2 * in, 0.f, true, t) || !resize_x2_tables_ok(true, in, t);
        }
        bad += !resize_axis_table(1, 4, 8, 0.f, true, t);
        t[5].i1 = 4;                                                                          // a tap beyond the input
        bad += resize_x2_tables_ok(false, 4, t);
        bad += !resize_axis_table(3, 8, 4, 0.f, true, t) || resize_x2_tables_ok(true, 2, t);   // a downscale's table is no x2 table
        if (!bad) printf("resize tables ok\n");
        return bad ? 1 : 0;
    }
    if ((argc - 1) % 5) return 2;
    for (int k = 0; k < (argc - 1) / 5; ++k) {
        char** a = argv + 1 + 5 * k;
        const uint32_t bits = (uint32_t)strtoul(a[3], nullptr, 16);
        float scale;
        std::memcpy(&scale, &bits, 4);
        const bool ok = resize_axis_table(atoi(a[0]), atoi(a[1]), atoi(a[2]), scale, atoi(a[4]) != 0, t);
        printf("table %d %d\n", k, (int)ok);
        if (!ok) continue;
        for (const ResizeTap& e : t) {
            uint32_t fb;
            std::memcpy(&fb, &e.frac, 4);
            printf("%d %d %08x\n", e.i0, e.i1, fb);
        }
    }
    return 0;
}
