// tests/cpp/stage_c64_pack_check.cpp - no GPU: the weight stream of pack_stage1_c64_stream (api_chain.hip) walked wave by wave, fragment by
// fragment, lane by lane the way conv_stage1_c64_kernel (conv_stage_coop.hip) reads it - wave w's 17 fragments of 1 KB at (w * 17 + r) * 1024,
// a lane's 16 bytes at lane * 16; fragment r = tap r of the 3x3 conv (r < 9), accumulator r - 9 of the first 1x1 conv (9 <= r < 13), k-step
// r - 13 of the last 1x1 conv - against the OIHW weights of the three convolutions. An MFMA A fragment's row rho = lane & 15 is the output
// channel of accumulator row rho (the C/D map: row = (lane >> 4) * 4 + register), its k-group kq = lane >> 4 the 16 input channels the B
// operand's lane group kq holds:
//   3x3:          channel w * 16 + rho,                                   input kq * 16 + j of the halo pixel's 64 channels
//   1x1 + eltwise: channel w * 64 + (rho >> 2) * 16 + mf * 4 + (rho & 3)   (cg = w * 64 + fq * 16, accumulator mf, register r),  input kq * 16 + j
//   last 1x1:     channel w * 16 + rho,                                   input ks * 64 + kq * 16 + j of the y1 tile's 256 channels
// Every weight byte has exactly one place, every place holds its weight, the stream is exactly 4 x 17 KB. Exit status 0 = equal.
// The walk restates the kernel's index arithmetic: a change there must be repeated here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
void pack_stage1_c64_stream(const int8_t* w3, const int8_t* wa, const int8_t* wb, std::vector<uint8_t>& out);

int main() {
    const int C = 64, K1 = 256, NW = 4, F0 = 9, F1 = 4, F2 = 4, FB = F0 + F1 + F2;
    for (int seed = 1; seed <= 3; ++seed) {
        srand(seed);
        std::vector<int8_t> w3((size_t)C * C * 9), wa((size_t)K1 * C), wb((size_t)C * K1);
        for (auto* v : {&w3, &wa, &wb})
            for (auto& b : *v) b = (int8_t)(rand() % 256 - 128);
        std::vector<uint8_t> s;
        pack_stage1_c64_stream(w3.data(), wa.data(), wb.data(), s);
        if (s.size() != (size_t)NW * FB * 1024) { printf("stream size %zu\n", s.size()); return 1; }
        if (s.size() != w3.size() + wa.size() + wb.size()) { printf("the stream is not a permutation of the weights\n"); return 1; }
        std::vector<int> h3(w3.size(), 0), ha(wa.size(), 0), hb(wb.size(), 0);
        for (int w = 0; w < NW; ++w)
            for (int r = 0; r < FB; ++r)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 16; ++j) {
                        const int rho = lane & 15, kq = lane >> 4;
                        const int8_t got = (int8_t)s[(((size_t)w * FB + r) * 64 + lane) * 16 + j];
                        size_t idx;
                        int8_t want;
                        if (r < F0) {                       // phase 0: fr[tap], B operand = halo chunk fq of pixel (dy, dx) + frow
                            const int ch = w * 16 + rho, c = kq * 16 + j;
                            idx = ((size_t)ch * C + c) * 9 + r;
                            want = w3[idx];
                            ++h3[idx];
                        } else if (r < F0 + F1) {           // phase 1: accumulator mf = r - 9, B operand = mid chunk fq
                            const int mf = r - F0;
                            const int ch = w * 64 + (rho >> 2) * 16 + mf * 4 + (rho & 3), c = kq * 16 + j;
                            idx = (size_t)ch * C + c;
                            want = wa[idx];
                            ++ha[idx];
                        } else {                            // phase 2: k-step ks = r - 13, B operand = y1 tile chunk ks * 4 + fq
                            const int ks = r - F0 - F1;
                            const int ch = w * 16 + rho, c = ks * 64 + kq * 16 + j;
                            idx = (size_t)ch * K1 + c;
                            want = wb[idx];
                            ++hb[idx];
                        }
                        if (got != want) { printf("seed %d wave %d fragment %d lane %d byte %d: %d, want %d\n", seed, w, r, lane, j, got, want); return 1; }
                    }
        for (auto* h : {&h3, &ha, &hb})
            for (int n : *h)
                if (n != 1) { printf("a weight with %d places\n", n); return 1; }
    }
    printf("stage c64 stream ok\n");
    return 0;
}
