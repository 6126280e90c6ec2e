// anakin_amd/csrc/conv_fire.hip - SqueezeNet's Fire module in one launch (gfx950): the 1x1 squeeze conv, the 1x1 and the padded 3x3 expand
// convs that both read it, and the channel concat of the two, INT8. The inner edge is only 16 .. 64 channels wide - the opposite case from
// conv_ir.hip, whose inner edges are six times wider than its input: one squeeze tile with a one-pixel halo in LDS (S padded to ONE 64-deep
// k-step: 80 bytes per pixel with the bank-spreading chunk) feeds both expand convs, each of which stores straight into its half of the
// concatenated tensor. Four operators - three convs and a copy - become one launch; neither the squeeze edge nor the two expand edges
// reach memory (the squeeze edge only when the caller asks for it).
//
//   workgroup = a tile of th x 16 pixels of one image (nf fragments of 16) x ALL of E1 + E3: no workgroup waits for another - no atomics, no
//   counters; plain vector loads and stores.
//
//   phase 0: the tile's input halo - (th + 2) x 18 pixels x C - into LDS as xin[pixel][pchx], the bytes as they are in memory, zero outside
//   the image and beyond C up to a whole k-step (conv_ir.hip's phase 0 at stride 1).
//   phase 1, squeeze: v_mfma_i32_16x16x64_i8 in the operand convention of conv_ir.hip - weights the A operand, LDS pixels the B operand (u8
//   input XOR 0x80 on the way, comp = 128 * sum(w) corrects it). A wave owns halo fragments wave, wave + 4, ...; chain_out_pack requantises to
//   u8 exactly where the squeeze op would store - to y_squeeze from the workgroup in whose own pixels the halo pixel lies, when that edge is
//   wanted - and to sbuf[halo pixel][64] XOR 0x80, the s8 form the expand MFMAs take (their comp corrects it).
//   A HALO PIXEL OUTSIDE THE IMAGE IS WRITTEN AS ZERO BYTES (0x80 in that form), NOT COMPUTED: the 3x3 conv pads its INPUT edge with zeros,
//   and squeeze(0) = relu(bias') is not zero. Channels S .. 63 hold zero bytes too (the constants are padded with zeros) against zero weights.
//   phase 2, expands: a unit is (64 output channels of one of the two convs, one pixel fragment); wave w owns units w, w + 4, ... one after
//   the other. expand1x1: ONE k-step at the pixel's own halo position; expand3x3: NINE k-steps, one per tap, at the nine positions around it -
//   each tap padded to 64 deep. (For S = 16 / 32 several taps would fit one k-step; not done: the B operand of a lane is ONE 16-byte LDS
//   read of one pixel, a packed step needs the lane's 16 bytes from the tap its k-group belongs to - a different addressing per k-group and
//   a second weight layout - for a launch that is bound by its boundaries, not by its MFMAs, at these sizes: profiles/fire/README.md.)
//   Each conv's own requant epilogue (its scale, bias', comp) and one 16-byte store per lane at channel 0 / E1 of the output pixel.
//   Every output byte is the byte the separate ops store.
#include "epilogue_pack.h"

#include <atomic>
#include <vector>

namespace saber_mi355x {

typedef unsigned fr4u __attribute__((ext_vector_type(4)));

template <bool U8>
__device__ __forceinline__ void fire_body(const FireKArgs& a) {
    extern __shared__ v4i fire_lds[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63, col = lane & 15, kg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = nt >> 6;
    const int n = (int)blockIdx.x / a.tiles_per_img, rem = (int)blockIdx.x - n * a.tiles_per_img;
    const int tyi = rem / a.tiles_x;
    const int y0 = tyi * a.th, x0 = (rem - tyi * a.tiles_x) * a.tw;      // the tile's first pixel
    const int iy0 = y0 - 1, ix0 = x0 - 1;                                // the halo's first pixel (pad 1)
    const int HP = a.hh * a.hw, HPP = a.hpf * 16;                        // halo pixels, ... rounded up to whole fragments
    const int kss = (a.C + 63) >> 6, pchx = kss * 4 + 1;                 // squeeze k-steps; xin pixel pitch in chunks
    constexpr int PCH = 5;                                               // sbuf pixel pitch: 64 bytes + one chunk
    v4i* xin = fire_lds;
    v4i* sbuf = xin + HPP * pchx;
    const char* xn = (const char*)a.x + (size_t)n * a.H * a.W * a.C;

    // ================= phase 0: the input halo -> LDS ====================================================================================
    for (int it = tid; it < HPP * kss * 4; it += nt) {
        const int hp = it / (kss * 4), cv = it - hp * (kss * 4);
        const int hy = hp / a.hw, hx = hp - hy * a.hw;
        const int iy = iy0 + hy, ix = ix0 + hx;
        fr4u v = {0u, 0u, 0u, 0u};
        if (hp < HP && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W && cv * 16 < a.C)      // (C % 16 == 0: a whole chunk or none)
            v = *(const fr4u*)(xn + ((size_t)iy * a.W + ix) * a.C + cv * 16);
        xin[hp * pchx + cv] = __builtin_bit_cast(v4i, v);
    }
    __syncthreads();

    // ================= phase 1: squeeze over tile + halo -> sbuf (and y_squeeze) ==========================================================
    {
        const int xmask = U8 ? (int)0x80808080u : 0;
        const int s0 = kg * 16;                     // the lane's 16 consecutive squeezed channels
        const v4i* pp = (const v4i*)a.sprm + (s0 >> 2) * 3;
        const v4i* wl = (const v4i*)a.ws + lane;
        v4f sc[4], bi[4];
#pragma unroll
        for (int mf = 0; mf < 4; ++mf) {
            sc[mf] = __builtin_bit_cast(v4f, pp[mf * 3]);
            bi[mf] = __builtin_bit_cast(v4f, pp[mf * 3 + 1]);
        }
        for (int f = wave; f < a.hpf; f += nw) {
            v4i e[4];
#pragma unroll
            for (int mf = 0; mf < 4; ++mf) e[mf] = pp[mf * 3 + 2];
            const int hp = f * 16 + col;
            for (int ks = 0; ks < kss; ++ks) {
                v4i b = xin[hp * pchx + ks * 4 + kg];
                b.x ^= xmask; b.y ^= xmask; b.z ^= xmask; b.w ^= xmask;
#pragma unroll
                for (int mf = 0; mf < 4; ++mf) e[mf] = mma_step(wl[(ks * 4 + mf) * 64], b, e[mf]);
            }
            const int hy = hp / a.hw, hx = hp - hy * a.hw;
            const int iy = iy0 + hy, ix = ix0 + hx;
            const bool inside = hp < HP && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            fr4u o = {0u, 0u, 0u, 0u};              // outside the image: the 3x3 conv's zero padding
            if (inside) {
#pragma unroll
                for (int mf = 0; mf < 4; ++mf) o[mf] = chain_out_pack(e[mf], v4i{0, 0, 0, 0}, bi[mf], sc[mf], 0.f, 0.f, 0u);
                // the squeeze edge: every image pixel lies in the own pixels of exactly one tile
                if (a.y_s != nullptr && s0 < a.S && iy >= y0 && iy < y0 + a.th && ix >= x0 && ix < x0 + a.tw)
                    *(fr4u*)((char*)a.y_s + (((size_t)n * a.H + iy) * a.W + ix) * a.S + s0) = o;
            }
            o = o ^ fr4u{0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
            sbuf[hp * PCH + kg] = __builtin_bit_cast(v4i, o);
        }
    }
    __syncthreads();

    // ================= phase 2: both expand convs from sbuf -> their halves of y ===========================================================
    const int G1 = (a.E1 + 63) >> 6, G3 = (a.E3 + 63) >> 6, nunits = (G1 + G3) * a.nf;
    const int CT = a.E1 + a.E3;
    for (int u = wave; u < nunits; u += nw) {
        const int g = u / a.nf, f = u - g * a.nf;
        const bool is3 = g >= G1;
        const int gg = is3 ? g - G1 : g;
        const int p = f * 16 + col;
        const int ty = p / a.tw, tx = p - ty * a.tw;
        const int tyc = ty < a.th ? ty : 0;          // (a fragment row beyond the tile reads a position inside LDS and is never stored)
        const int cg = gg * 64 + kg * 16;            // the lane's 16 consecutive output channels of its conv
        const v4i* pp = (const v4i*)(is3 ? a.prm3 : a.prm1) + (cg >> 2) * 3;
        v4i acc[4];
#pragma unroll
        for (int mf = 0; mf < 4; ++mf) acc[mf] = pp[mf * 3 + 2];
        if (!is3) {
            const v4i b = sbuf[((tyc + 1) * a.hw + tx + 1) * PCH + kg];
            const v4i* wl = (const v4i*)a.w1 + (size_t)gg * 256 + lane;
#pragma unroll
            for (int mf = 0; mf < 4; ++mf) acc[mf] = mma_step(wl[mf * 64], b, acc[mf]);
        } else {
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int i = t / 3, j = t - i * 3;
                const v4i b = sbuf[((tyc + i) * a.hw + tx + j) * PCH + kg];
                const v4i* wl = (const v4i*)a.w3 + ((size_t)t * G3 + gg) * 256 + lane;
#pragma unroll
                for (int mf = 0; mf < 4; ++mf) acc[mf] = mma_step(wl[mf * 64], b, acc[mf]);
            }
        }
        const int oy = y0 + ty, ox = x0 + tx;
        if (cg >= (is3 ? a.E3 : a.E1) || ty >= a.th || oy >= a.H || ox >= a.W) continue;
        fr4u o;
#pragma unroll
        for (int mf = 0; mf < 4; ++mf)
            o[mf] = chain_out_pack(acc[mf], v4i{0, 0, 0, 0}, __builtin_bit_cast(v4f, pp[mf * 3 + 1]), __builtin_bit_cast(v4f, pp[mf * 3]), 0.f, 0.f, 0u);
        *(fr4u*)((char*)a.y + (((size_t)n * a.H + oy) * a.W + ox) * CT + (is3 ? a.E1 : 0) + cg) = o;
    }
}

// stable names: a kernel trace shows the input type (the tile is a launch parameter)
__global__ __launch_bounds__(256) void fire_squeeze_expand_i8_u8(const FireKArgs a) { fire_body<true>(a); }
__global__ __launch_bounds__(256) void fire_squeeze_expand_i8_s8(const FireKArgs a) { fire_body<false>(a); }

// THE table of launch forms, in the autotuner's candidate order: rows x 16 pixel tiles
static const struct { int code, rows; const char* name; } fire_forms[] = {
    {1, 4, "4x16"},
    {2, 2, "2x16"},
};
const char* conv_fire_form_name(int code) {
    for (const auto& f : fire_forms)
        if (f.code == code) return f.name;
    return "";
}
bool conv_fire_geom(int code, int c, int s, int e1, int e3, int h, int w, FireGeom* out) {
    int rows = -1;
    for (const auto& f : fire_forms)
        if (f.code == code) rows = f.rows;
    if (rows < 0 || (s != 16 && s != 32 && s != 48 && s != 64) || c < 16 || c > 512 || c % 16 || e1 < 16 || e1 > 512 || e1 % 16 || e3 < 16 || e3 > 512 ||
        e3 % 16 || h <= 0 || w <= 0)
        return false;
    FireGeom g;
    g.th = rows; g.tw = 16; g.nf = rows;
    g.hh = rows + 2; g.hw = 18;
    g.hpf = (g.hh * g.hw + 15) / 16;
    g.tiles_x = (w + 15) / 16; g.tiles_y = (h + rows - 1) / rows;
    g.lds = (size_t)16 * g.hpf * 16 * (((c + 63) / 64) * 4 + 1 + 5);
    if (g.lds > FIRE_LDS_LIMIT) return false;
    if (out) *out = g;
    return true;
}

hipError_t conv_fire_prepare() {
    static std::atomic<bool> done[64];      // per device, zero-initialised
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess || dev < 0 || dev >= 64) return e != hipSuccess ? e : hipErrorInvalidDevice;
    if (done[dev].load(std::memory_order_acquire)) return hipSuccess;
    const void* fns[] = {(const void*)fire_squeeze_expand_i8_u8, (const void*)fire_squeeze_expand_i8_s8};
    for (const void* f : fns)
        if ((e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FIRE_LDS_LIMIT)) != hipSuccess) return e;
    done[dev].store(true, std::memory_order_release);
    return hipSuccess;
}

hipError_t launch_conv_fire(int code, bool in_u8, const FireKArgs& a0, hipStream_t s) {
    FireGeom g;
    if (!conv_fire_geom(code, a0.C, a0.S, a0.E1, a0.E3, a0.H, a0.W, &g)) return hipErrorInvalidValue;
    if (a0.N <= 0 || !a0.x || !a0.y || !a0.ws || !a0.sprm || !a0.w1 || !a0.prm1 || !a0.w3 || !a0.prm3) return hipErrorInvalidValue;
    FireKArgs a = a0;
    a.th = g.th; a.tw = g.tw; a.nf = g.nf; a.hh = g.hh; a.hw = g.hw; a.hpf = g.hpf;
    a.tiles_x = g.tiles_x; a.tiles_per_img = g.tiles_x * g.tiles_y;
    const size_t wgs = (size_t)a.N * a.tiles_per_img;
    if (wgs >= ((size_t)1 << 31)) return hipErrorInvalidValue;
    hipError_t e = conv_fire_prepare();
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)wgs), block(256);
    if (in_u8) hipLaunchKernelGGL(fire_squeeze_expand_i8_u8, grid, block, g.lds, s, a);
    else hipLaunchKernelGGL(fire_squeeze_expand_i8_s8, grid, block, g.lds, s, a);
    return hipGetLastError();
}

}  // namespace saber_mi355x
