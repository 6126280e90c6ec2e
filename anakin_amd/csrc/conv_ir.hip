// anakin_amd/csrc/conv_ir.hip - MobileNet-v2's inverted-residual block in one launch (gfx950): the 1x1 expand conv, the depthwise 3x3 conv
// and the 1x1 linear project conv, INT8, with the eltwise sum of the project conv and the block's input where the block has one. The two
// inner edges are six times wider than the block's input and output (96 .. 960 channels against 16 .. 160) and nothing outside the block
// reads them: as three launches they cost two kernel boundaries (2.3 - 2.7 us each on this part) and two wide round trips through
// memory; here a workgroup keeps its piece of both in LDS, 64 channels at a time. The counterpart of conv_sep.hip (MobileNet-v1) and
// conv1x1_chain.hip (ResNet).
//
//   workgroup = a tile of th x tw output pixels of one image (nf fragments of 16 pixels) x ALL of Cout: the project conv reduces over all of
//   Ce, so no workgroup waits for another one - no atomics, no counters; plain vector loads and stores.
//
//   phase 0, once: the tile's input halo - ((th - 1) * stride + 3) x ((tw - 1) * stride + 3) pixels x Cin - into LDS as xin[pixel][pchx],
//   the bytes as they are in memory, zero outside the image and beyond Cin up to a whole k-step of 64. The pixel pitch is the k-steps plus ONE
//   16-byte chunk, so the 16 lanes of a fragment column hit 16 different bank groups (conv_sep.hip, conv1x1_chain.hip: PCH).
//
//   then, for each chunk of 64 expanded channels:
//   (a) expand: v_mfma_i32_16x16x64_i8 in the operand convention of conv_igemm_impl.h / conv_sep.hip - weights the A operand, LDS pixels the
//       B operand (u8 input XOR 0x80 on the way, comp = 128 * sum(w) corrects it). A wave owns halo fragments wave, wave + 4, ...;
//       chain_out_pack (epilogue_pack.h) requantises to u8 exactly where the expand op would store: ebuf[halo pixel][64] - and y_expand, from
//       the workgroup in whose own pixels the halo pixel lies, when that edge is wanted.
//       A HALO PIXEL OUTSIDE THE IMAGE IS WRITTEN AS ZERO BYTES, NOT COMPUTED: the depthwise conv pads its INPUT edge with zeros, and
//       expand(0) = relu(bias') is not zero.
//   (b) depthwise: work item = (tile pixel, 16-byte channel vector): nine taps from ebuf in int32, chain_out_pack, 16 bytes to mid[pixel][64]
//       XOR 0x80 (the s8 form the MFMA takes; the project op's comp corrects it) - and to y_dw when that edge is wanted.
//   (c) project: ONE k-step of the project conv into int32 accumulators that live across the chunks. An accumulator unit is (64 output
//       channels, one pixel fragment); wave w owns units w, w + 4, ... (at most IR_MAX_UNITS / 4 of them).
//   After the last chunk: the project op's epilogue (chain_out_pack, or chain_elt_pack with the 16 residual bytes of x for the fused eltwise)
//   and one 16-byte store per lane - 8-byte stores where Cout % 16 == 8 (a pixel is then only 8-byte aligned).
//   Nothing crosses an edge in float or int32: every output byte is the byte the three (four) separate ops store.
//
//   Tile pixels beyond the image read halo positions inside LDS like any other and are never stored.
#include "epilogue_pack.h"

#include <algorithm>
#include <atomic>
#include <vector>

namespace saber_mi355x {

typedef unsigned ir4u __attribute__((ext_vector_type(4)));
typedef unsigned ir2u __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int ir_u8(unsigned v, int b) { return (int)((v >> (8 * b)) & 0xffu); }
__device__ __forceinline__ int ir_s8(unsigned v, int b) { return (int)(int8_t)(v >> (8 * b)); }

// 16 bytes at p: one vector where a16 (every pixel 16-byte aligned), else two 8-byte halves
__device__ __forceinline__ ir4u ir_load16(const char* p, bool a16) {
    if (a16) return *(const ir4u*)p;
    const ir2u lo = *(const ir2u*)p, hi = *(const ir2u*)(p + 8);
    return ir4u{lo.x, lo.y, hi.x, hi.y};
}
__device__ __forceinline__ void ir_store16(char* p, ir4u v, bool a16) {
    if (a16) {
        *(ir4u*)p = v;
    } else {
        *(ir2u*)p = ir2u{v.x, v.y};
        *(ir2u*)(p + 8) = ir2u{v.z, v.w};
    }
}

template <bool U8>
__device__ __forceinline__ void ir_body(const IrKArgs& a) {
    extern __shared__ v4i ir_lds[];
    constexpr int MAXU = IR_MAX_UNITS / 4;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63, col = lane & 15, kg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = nt >> 6;
    const int n = (int)blockIdx.x / a.tiles_per_img, rem = (int)blockIdx.x - n * a.tiles_per_img;
    const int tyi = rem / a.tiles_x;
    const int y0 = tyi * a.th, x0 = (rem - tyi * a.tiles_x) * a.tw;      // the tile's first output pixel
    const int iy0 = y0 * a.stride - 1, ix0 = x0 * a.stride - 1;         // the halo's first input pixel (pad 1)
    const int HP = a.hh * a.hw, HPP = a.hpf * 16;                       // halo pixels, ... rounded up to whole fragments
    const int kse = (a.Cin + 63) >> 6, pchx = kse * 4 + 1;              // expand k-steps; xin pixel pitch in chunks
    const int ksp = (a.Ce + 63) >> 6;                                   // chunks of the expanded channels = project k-steps
    const int G = (a.Cout + 63) >> 6, nunits = G * a.nf;
    constexpr int PCH = 5;                                              // ebuf / mid pixel pitch: 64 bytes + one chunk
    v4i* xin = ir_lds;
    v4i* ebuf = xin + HPP * pchx;
    v4i* mid = ebuf + HPP * PCH;
    const char* xn = (const char*)a.x + (size_t)n * a.H * a.W * a.Cin;
    const bool xa16 = (a.Cin & 15) == 0;

    // ================= phase 0: the input halo -> LDS =================================================================================
    for (int it = tid; it < HPP * kse * 4; it += nt) {
        const int hp = it / (kse * 4), cv = it - hp * (kse * 4);
        const int hy = hp / a.hw, hx = hp - hy * a.hw;
        const int iy = iy0 + hy, ix = ix0 + hx;
        ir4u v = {0u, 0u, 0u, 0u};
        if (hp < HP && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W && cv * 16 < a.Cin) {
            const char* p = xn + ((size_t)iy * a.W + ix) * a.Cin + cv * 16;
            if (cv * 16 + 16 <= a.Cin) {
                v = ir_load16(p, xa16);
            } else {      // Cin % 16 == 8: the last 8 channels, the rest of the chunk stays zero
                const ir2u lo = *(const ir2u*)p;
                v.x = lo.x; v.y = lo.y;
            }
        }
        xin[hp * pchx + cv] = __builtin_bit_cast(v4i, v);
    }

    v4i acc[MAXU][4];
#pragma unroll
    for (int ui = 0; ui < MAXU; ++ui) {
        const int u = wave + ui * nw;
        const int g = u < nunits ? u / a.nf : 0;
        const v4i* pp = (const v4i*)a.pprm + ((g * 64 + kg * 16) >> 2) * 3;
#pragma unroll
        for (int mf = 0; mf < 4; ++mf) acc[ui][mf] = pp[mf * 3 + 2];
    }
    const int xmask = U8 ? (int)0x80808080u : 0;

    for (int cc = 0; cc < ksp; ++cc) {
        __syncthreads();      // xin is staged (first chunk); the previous chunk's project step has read mid, its depthwise step ebuf
        // ================= (a) expand: the halo's 64 channels of this chunk -> ebuf (and y_expand) ====================================
        {
            const int ce0 = cc * 64 + kg * 16;      // the lane's 16 consecutive expanded channels
            const v4i* pp = (const v4i*)a.eprm + (ce0 >> 2) * 3;
            const v4i* wl = (const v4i*)a.we + (size_t)cc * kse * 256 + lane;
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
                for (int ks = 0; ks < kse; ++ks) {
                    v4i b = xin[hp * pchx + ks * 4 + kg];
                    b.x ^= xmask; b.y ^= xmask; b.z ^= xmask; b.w ^= xmask;
#pragma unroll
                    for (int mf = 0; mf < 4; ++mf) e[mf] = mma_step(wl[(ks * 4 + mf) * 64], b, e[mf]);
                }
                const int hy = hp / a.hw, hx = hp - hy * a.hw;
                const int iy = iy0 + hy, ix = ix0 + hx;
                const bool inside = hp < HP && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
                ir4u o = {0u, 0u, 0u, 0u};      // outside the image: the depthwise conv's zero padding
                if (inside) {
#pragma unroll
                    for (int mf = 0; mf < 4; ++mf) o[mf] = chain_out_pack(e[mf], v4i{0, 0, 0, 0}, bi[mf], sc[mf], 0.f, 0.f, 0u);
                    // the expanded edge: every image pixel lies in the own pixels of exactly one tile
                    if (a.y_e != nullptr && ce0 < a.Ce && iy >= y0 * a.stride && iy < (y0 + a.th) * a.stride && ix >= x0 * a.stride &&
                        ix < (x0 + a.tw) * a.stride)
                        *(ir4u*)((char*)a.y_e + (((size_t)n * a.H + iy) * a.W + ix) * a.Ce + ce0) = o;
                }
                ebuf[hp * PCH + kg] = __builtin_bit_cast(v4i, o);
            }
        }
        __syncthreads();
        // ================= (b) depthwise 3x3 from ebuf -> mid (and y_dw) =================================================================
        for (int it = tid; it < a.nf * 64; it += nt) {
            const int p = it >> 2, cvi = it & 3;
            const int ch = cc * 64 + cvi * 16;
            const int ty = p / a.tw, tx = p - ty * a.tw;
            ir4u out = {0u, 0u, 0u, 0u};
            if (ch < a.Ce && ty < a.th) {
                int s[16];
#pragma unroll
                for (int c = 0; c < 16; ++c) s[c] = 0;
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const ir4u xv = __builtin_bit_cast(ir4u, ebuf[((ty * a.stride + i) * a.hw + tx * a.stride + j) * PCH + cvi]);
                        const ir4u wt = *(const ir4u*)((const char*)a.wdw + (size_t)(i * 3 + j) * a.Ce + ch);
#pragma unroll
                        for (int c = 0; c < 16; ++c) s[c] += ir_u8(xv[c >> 2], c & 3) * ir_s8(wt[c >> 2], c & 3);
                    }
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const v4f b = *(const v4f*)(a.dw_bias + ch + 4 * v), sc = *(const v4f*)(a.dw_scale + ch + 4 * v);
                    out[v] = chain_out_pack(v4i{s[4 * v], s[4 * v + 1], s[4 * v + 2], s[4 * v + 3]}, v4i{0, 0, 0, 0}, b, sc, 0.f, 0.f, 0u);
                }
                const int oy = y0 + ty, ox = x0 + tx;
                if (a.y_d != nullptr && oy < a.OH && ox < a.OW) *(ir4u*)((char*)a.y_d + (((size_t)n * a.OH + oy) * a.OW + ox) * a.Ce + ch) = out;
                out = out ^ ir4u{0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
            }
            mid[p * PCH + cvi] = __builtin_bit_cast(v4i, out);
        }
        __syncthreads();
        // ================= (c) project: one k-step into the accumulators ==================================================================
#pragma unroll
        for (int ui = 0; ui < MAXU; ++ui) {
            const int u = wave + ui * nw;
            if (u < nunits) {
                const int g = u / a.nf, f = u - g * a.nf;
                const v4i b = mid[(f * 16 + col) * PCH + kg];
                const v4i* wl = (const v4i*)a.wp + ((size_t)g * ksp + cc) * 256 + lane;
#pragma unroll
                for (int mf = 0; mf < 4; ++mf) acc[ui][mf] = mma_step(wl[mf * 64], b, acc[ui][mf]);
            }
        }
    }

    // ================= the project conv's epilogue (+ the eltwise sum with x) ============================================================
    const float lo = a.p_relu ? 0.f : -3.0e38f;
    const float off = a.out_u8 ? 0.f : 128.f;
    const unsigned xm = a.out_u8 ? 0u : 0x80808080u;
    const float lo_s8 = a.p_relu ? 0.f : -128.f;
    const float res_lo = a.res_relu ? 0.f : -3.0e38f;
    const bool ya16 = (a.Cout & 15) == 0;
#pragma unroll
    for (int ui = 0; ui < MAXU; ++ui) {
        const int u = wave + ui * nw;
        if (u >= nunits) continue;
        const int g = u / a.nf, f = u - g * a.nf;
        const int cg = g * 64 + kg * 16;            // the lane's 16 consecutive output channels
        const int p = f * 16 + col;
        const int ty = p / a.tw, tx = p - ty * a.tw;
        const int oy = y0 + ty, ox = x0 + tx;
        if (cg >= a.Cout || ty >= a.th || oy >= a.OH || ox >= a.OW) continue;
        const bool half = cg + 16 > a.Cout;         // Cout % 16 == 8: the last 8 channels
        const v4i* pp = (const v4i*)a.pprm + (cg >> 2) * 3;
        const size_t pix = ((size_t)n * a.OH + oy) * a.OW + ox;
        ir4u rs = {0u, 0u, 0u, 0u};
        if (a.elt) {                                // the residual is the block's input: same pixel, Cin == Cout, s8
            const char* rp = (const char*)a.x + pix * a.Cin + cg;
            if (half) {
                const ir2u r2 = *(const ir2u*)rp;
                rs.x = r2.x; rs.y = r2.y;
            } else {
                rs = ir_load16(rp, ya16);
            }
        }
        ir4u o;
#pragma unroll
        for (int mf = 0; mf < 4; ++mf) {
            const v4f sc = __builtin_bit_cast(v4f, pp[mf * 3]), bi = __builtin_bit_cast(v4f, pp[mf * 3 + 1]);
            o[mf] = a.elt ? chain_elt_pack(acc[ui][mf], v4i{0, 0, 0, 0}, bi, sc, rs[mf], lo_s8, res_lo, a)
                          : chain_out_pack(acc[ui][mf], v4i{0, 0, 0, 0}, bi, sc, lo, off, xm);
        }
        char* yp = (char*)a.y + pix * a.Cout + cg;
        if (half) *(ir2u*)yp = ir2u{o.x, o.y};
        else ir_store16(yp, o, ya16);
    }
}

// stable names: a kernel trace shows the input type (the tile is a launch parameter)
__global__ __launch_bounds__(256) void ir_expand_dw_project_i8_u8(const IrKArgs a) { ir_body<true>(a); }
__global__ __launch_bounds__(256) void ir_expand_dw_project_i8_s8(const IrKArgs a) { ir_body<false>(a); }

// THE table of launch forms, in the autotuner's candidate order. rows x 16 tiles for the large images; img: tiles as wide as the image (at most 16
// columns) and as many rows as the accumulator units, the LDS limit and an even split of the image allow - the whole 7 x 7 image, the whole or
// half of a 14 x 14 one: no halo recompute between column tiles, few workgroups with much work each
static const struct { int code, rows; const char* name; } ir_forms[] = {
    {1, 4, "4x16"},
    {2, 2, "2x16"},
    {3, 0, "img"},
};
const char* conv_ir_form_name(int code) {
    for (const auto& f : ir_forms)
        if (f.code == code) return f.name;
    return "";
}
bool conv_ir_geom(int code, int cin, int ce, int cout, int oh, int ow, int stride, IrGeom* out) {
    int rows = -1;
    for (const auto& f : ir_forms)
        if (f.code == code) rows = f.rows;
    if (rows < 0 || cin < 8 || cin > 192 || cin % 8 || ce < 16 || ce > 1024 || ce % 16 || cout < 8 || cout > 320 || cout % 8 || oh <= 0 || ow <= 0 ||
        (stride != 1 && stride != 2))
        return false;
    const int G = (cout + 63) / 64, kse = (cin + 63) / 64;
    IrGeom g;
    auto fill = [&](int th, int tw) {
        g.th = th; g.tw = tw; g.nf = (th * tw + 15) / 16;
        g.hh = (th - 1) * stride + 3; g.hw = (tw - 1) * stride + 3;
        g.hpf = (g.hh * g.hw + 15) / 16;
        g.tiles_x = (ow + tw - 1) / tw; g.tiles_y = (oh + th - 1) / th;
        g.lds = (size_t)16 * ((size_t)g.hpf * 16 * (kse * 4 + 1) + (size_t)g.hpf * 16 * 5 + (size_t)g.nf * 16 * 5);
    };
    if (rows > 0) {
        fill(rows, 16);
    } else {
        if (ow > 16) return false;
        const int nfmax = std::min(IR_MAX_UNITS / G, 16);
        int th = std::min(oh, nfmax * 16 / ow);
        if (th < 1) return false;
        int tys = (oh + th - 1) / th;
        fill((oh + tys - 1) / tys, ow);
        while (g.lds > IR_LDS_LIMIT && g.th > 1) {      // more, smaller row tiles until two workgroups fit a CU
            ++tys;
            fill((oh + tys - 1) / tys, ow);
        }
    }
    if (G * g.nf > IR_MAX_UNITS || g.lds > IR_LDS_LIMIT) return false;
    if (out) *out = g;
    return true;
}

// a 1x1 conv's weights [K][C] -> [group of 64 output channels][k-step of 64 input channels][accumulator 0..3][lane] x 16 bytes: lane
// (rho = lane & 15, kq = lane >> 4) of accumulator mf holds input channels ks * 64 + kq * 16 .. + 15 of output channel
// group * 64 + (rho >> 2) * 16 + mf * 4 + (rho & 3), so a lane ends up with 16 CONSECUTIVE output channels of its pixel; zero beyond K and,
// byte by byte, beyond C (C % 16 == 8)
void ir_pack(const int8_t* w, int k, int c, std::vector<uint8_t>& out) {
    const int groups = (k + 63) / 64, ksn = (c + 63) / 64;
    out.assign((size_t)groups * ksn * 4 * 1024, 0);
    for (int g = 0; g < groups; ++g)
        for (int ks = 0; ks < ksn; ++ks)
            for (int mf = 0; mf < 4; ++mf)
                for (int lane = 0; lane < 64; ++lane) {
                    const int rho = lane & 15, kq = lane >> 4;
                    const int ch = g * 64 + (rho >> 2) * 16 + mf * 4 + (rho & 3), c0 = ks * 64 + kq * 16;
                    if (ch >= k) continue;
                    uint8_t* dst = &out[((((size_t)g * ksn + ks) * 4 + mf) * 64 + lane) * 16];
                    for (int j = 0; j < 16 && c0 + j < c; ++j) dst[j] = (uint8_t)w[(size_t)ch * c + c0 + j];
                }
}

hipError_t conv_ir_prepare() {
    static std::atomic<bool> done[64];      // per device, zero-initialised; two threads that both find it unset set the same attributes
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess || dev < 0 || dev >= 64) return e != hipSuccess ? e : hipErrorInvalidDevice;
    if (done[dev].load(std::memory_order_acquire)) return hipSuccess;
    const void* fns[] = {(const void*)ir_expand_dw_project_i8_u8, (const void*)ir_expand_dw_project_i8_s8};
    for (const void* f : fns)
        if ((e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)IR_LDS_LIMIT)) != hipSuccess) return e;
    done[dev].store(true, std::memory_order_release);
    return hipSuccess;
}

hipError_t launch_conv_ir(int code, bool in_u8, const IrKArgs& a0, hipStream_t s) {
    IrGeom g;
    if (!conv_ir_geom(code, a0.Cin, a0.Ce, a0.Cout, a0.OH, a0.OW, a0.stride, &g)) return hipErrorInvalidValue;
    if (a0.N <= 0 || a0.H <= 0 || a0.W <= 0 || !a0.x || !a0.y || !a0.we || !a0.wp || !a0.eprm || !a0.pprm || !a0.wdw || !a0.dw_bias || !a0.dw_scale)
        return hipErrorInvalidValue;
    if (a0.OH != (a0.H - 1) / a0.stride + 1 || a0.OW != (a0.W - 1) / a0.stride + 1) return hipErrorInvalidValue;      // 3x3, pad 1
    if (a0.elt && (in_u8 || a0.Cin != a0.Cout || a0.stride != 1 || a0.out_u8)) return hipErrorInvalidValue;
    IrKArgs a = a0;
    a.th = g.th; a.tw = g.tw; a.nf = g.nf; a.hh = g.hh; a.hw = g.hw; a.hpf = g.hpf;
    a.tiles_x = g.tiles_x; a.tiles_per_img = g.tiles_x * g.tiles_y;
    const size_t wgs = (size_t)a.N * a.tiles_per_img;
    if (wgs >= ((size_t)1 << 31)) return hipErrorInvalidValue;
    hipError_t e = conv_ir_prepare();
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)wgs), block(256);
    if (in_u8) hipLaunchKernelGGL(ir_expand_dw_project_i8_u8, grid, block, g.lds, s, a);
    else hipLaunchKernelGGL(ir_expand_dw_project_i8_s8, grid, block, g.lds, s, a);
    return hipGetLastError();
}

}  // namespace saber_mi355x
