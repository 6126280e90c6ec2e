// anakin_amd/csrc/conv_dw3x3.hip - depthwise 3x3 convolution (group == C == K, dilation 1, stride 1 | 2, pad 0 | 1) on NHWC
// tensors, INT8 and FP32: the 13 depthwise layers of MobileNet-v1, which otherwise run on conv_direct_kernel (conv_igemm.hip:
// one output element per thread, byte-wide / dword-wide loads).
//
// A depthwise layer has no reduction over channels - 9 multiply-adds per output element - so it is bound by memory (or, on the
// small late layers, by the launch itself); the kernels are organised around 16-byte accesses:
//   * a lane owns ONE channel vector of 16 bytes - 16 channels of an INT8 tensor, 4 of an FP32 one - for its whole life. Lanes
//     are numbered channel vector first, then output column, then row strip, then image, so the 64 lanes of a wave read
//     consecutive 16-byte pieces of an input row (1 KB per load instruction at stride 1) and write consecutive pieces of an
//     output row;
//   * its 9 weight vectors (w: [tap][C], packed by saber_hip_conv2d_set_weights) are loaded once into 36 registers;
//   * it computes a strip of RS output rows of its column. The (RS - 1) * stride + 3 input rows of the strip are read once,
//     three 16-byte loads per row, and every row is added into the (up to three) output rows it contributes to while it is
//     in registers: 4.5 loads per output at RS = 4 / stride 1 instead of 9. The overlap between neighbouring columns is
//     left to the vector L1 (the neighbouring lanes of the same wave ask for the same lines in the same instruction).
// Forms (launch_conv_dw3x3 `form`):
//   1 "rows4" (FP32) / "rows2" (INT8): RS = 4 / 2, 256 threads - the large early layers (112 x 112 x 32 .. 64), where a strip
//     still leaves thousands of waves. INT8 keeps 16 int32 accumulators per output row (and the compiler keeps the 144 weight
//     bytes sign-extended): strips of 2 rows stay at two waves per SIMD, strips of 4 would run at one;
//   2 "px": RS = 1, 64 threads - the small late layers (14 x 14 x 512, 7 x 7 x 1024 at batch 1): a few thousand lanes in
//     all, every output its own lane and every wave its own workgroup so that they spread over the CUs.
// No LDS, no barriers; plain vector loads and stores.
//
// Arithmetic (the bits of conv_direct_kernel with Cg == 1, which the tests compare against):
//   INT8: the true s8 / u8 activation times the s8 weight accumulated in int32 (exact; padded taps read as zero), then the
//         project's INT8 epilogue without contraction - (float)acc, + bias', * scale, relu, rintf, saturate (chain_out_pack,
//         epilogue_pack.h) or the f32 store.
//   FP32: acc = 0, acc = fmaf(x, w, acc) over the taps kh-major / kw-minor with padded taps contributing fmaf(0, w, acc),
//         then + bias, relu / leaky relu. Streaming the input rows keeps that order: the rows of one output arrive as
//         kh = 0, 1, 2.
#include "epilogue_pack.h"

namespace saber_mi355x {

struct DwKArgs {
    const void* x;
    const void* w;        // [9][C] s8 or f32
    void* y;
    const float* bias;    // INT8: bias' (may be null); FP32: bias (may be null)
    const float* scale;   // INT8 only
    int H, W, C, OH, OW;
    int stride, pad;
    int cv;               // channel vectors per pixel: C / 16 (INT8), C / 4 (FP32)
    int nstrips;          // row strips per image: ceil(OH / RS)
    unsigned total;       // lanes of the launch: N * nstrips * OW * cv
    int out_dtype, relu;
    float neg_slope;
};

typedef unsigned v4u __attribute__((ext_vector_type(4)));

template <bool U8>
__device__ __forceinline__ int dw_byte(unsigned v, int b) {
    return U8 ? (int)((v >> (8 * b)) & 0xffu) : (int)(int8_t)(v >> (8 * b));
}

// S: compile-time stride (1 | 2), or 0 = read a.stride (RS == 1 only: nothing is shared between rows there)
template <bool F32, bool U8, int RS, int S, int NT>
__device__ __forceinline__ void dw3x3_body(const DwKArgs& a) {
    static_assert(S != 0 || RS == 1, "a run-time stride needs RS == 1");
    const unsigned g = blockIdx.x * (unsigned)NT + threadIdx.x;
    if (g >= a.total) return;
    const int stride = S ? S : a.stride;
    const unsigned cvi = g % (unsigned)a.cv;
    unsigned q = g / (unsigned)a.cv;
    const int ox = (int)(q % (unsigned)a.OW);
    q /= (unsigned)a.OW;
    const int oy0 = (int)(q % (unsigned)a.nstrips) * RS;
    const int n = (int)(q / (unsigned)a.nstrips);
    const size_t cbyte = (size_t)cvi * 16;                       // byte offset of the lane's channel vector inside a pixel
    const size_t pix_bytes = (size_t)a.C * (F32 ? 4 : 1);

    v4u wv[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wv[t] = *(const v4u*)((const char*)a.w + (size_t)t * pix_bytes + cbyte);

    const int ix0 = ox * stride - a.pad;
    const int iy0 = oy0 * stride - a.pad;
    const char* xn = (const char*)a.x + (size_t)n * a.H * a.W * pix_bytes + cbyte;
    bool cok[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) cok[j] = ix0 + j >= 0 && ix0 + j < a.W;

    int acc_i[RS][F32 ? 1 : 16];
    v4f acc_f[RS];
#pragma unroll
    for (int o = 0; o < RS; ++o) {
        acc_f[o] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < (F32 ? 1 : 16); ++c) acc_i[o][c] = 0;
    }

    constexpr int SS = S ? S : 1;                                // (RS == 1: the three rows of the one output)
    constexpr int NR = (RS - 1) * SS + 3;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int iy = iy0 + r;
        const bool rok = iy >= 0 && iy < a.H;
        v4u xv[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            xv[j] = v4u{0u, 0u, 0u, 0u};
            if (rok && cok[j]) xv[j] = *(const v4u*)(xn + ((size_t)iy * a.W + (ix0 + j)) * pix_bytes);
        }
#pragma unroll
        for (int o = 0; o < RS; ++o) {
            const int i = r - o * SS;                            // tap row of output row o that input row r is
            if (i < 0 || i > 2) continue;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const v4u wt = wv[i * 3 + j];
                if (F32) {
                    const v4f xf = __builtin_bit_cast(v4f, xv[j]), wf = __builtin_bit_cast(v4f, wt);
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc_f[o][c] = __fmaf_rn(xf[c], wf[c], acc_f[o][c]);
                } else {
#pragma unroll
                    for (int c = 0; c < 16; ++c)
                        acc_i[o][F32 ? 0 : c] += dw_byte<U8>(xv[j][c >> 2], c & 3) * dw_byte<false>(wt[c >> 2], c & 3);
                }
            }
        }
    }

    // epilogue: per-channel constants of the lane's vector, then RS stores of 16 bytes (INT8 with f32 output: 4 x 16 bytes)
    const int c0 = (int)cvi * (F32 ? 4 : 16);
    if (F32) {
        v4f b = {0.f, 0.f, 0.f, 0.f};
        if (a.bias) b = *(const v4f*)(a.bias + c0);
#pragma unroll
        for (int o = 0; o < RS; ++o) {
            if (oy0 + o >= a.OH) break;
            v4f d = acc_f[o];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float v = d[c];
                if (a.bias) v = __fadd_rn(v, b[c]);
                if (a.relu) v = v > 0.f ? v : (a.neg_slope == 0.f ? 0.f : __fmul_rn(v, a.neg_slope));
                d[c] = v;
            }
            *(v4f*)((char*)a.y + (((size_t)n * a.OH + oy0 + o) * a.OW + ox) * pix_bytes + cbyte) = d;
        }
    } else {
        v4f b[4], sc[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            b[v] = a.bias ? *(const v4f*)(a.bias + c0 + 4 * v) : v4f{0.f, 0.f, 0.f, 0.f};   // ((float)acc + 0.f == (float)acc: the bits of "no bias")
            sc[v] = *(const v4f*)(a.scale + c0 + 4 * v);
        }
        const bool ou8 = a.out_dtype == DT_U8;
        const float lo = a.relu ? 0.f : -3.0e38f;
        const float off = ou8 ? 0.f : 128.f;
        const unsigned xm = ou8 ? 0u : 0x80808080u;
#pragma unroll
        for (int o = 0; o < RS; ++o) {
            if (oy0 + o >= a.OH) break;
            const size_t opix = ((size_t)n * a.OH + oy0 + o) * a.OW + ox;
            if (a.out_dtype == DT_F32) {
                float* yp = (float*)a.y + opix * a.C + c0;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    v4f d;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        float t = (float)acc_i[o][F32 ? 0 : 4 * v + c];
                        t = __fadd_rn(t, b[v][c]);
                        t = __fmul_rn(t, sc[v][c]);
                        if (a.relu) t = t < 0.f ? 0.f : t;
                        d[c] = t;
                    }
                    *(v4f*)(yp + 4 * v) = d;
                }
            } else {
                v4u out;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const v4i ac = {acc_i[o][F32 ? 0 : 4 * v], acc_i[o][F32 ? 0 : 4 * v + 1], acc_i[o][F32 ? 0 : 4 * v + 2], acc_i[o][F32 ? 0 : 4 * v + 3]};
                    out[v] = chain_out_pack(ac, v4i{0, 0, 0, 0}, b[v], sc[v], lo, off, xm);
                }
                *(v4u*)((char*)a.y + opix * (size_t)a.C + cbyte) = out;
            }
        }
    }
}

// stable names: a kernel trace shows which form, stride and input type ran
#define DW_KERNEL(name, F32, U8, RS, S, NT) \
    __global__ __launch_bounds__(NT) void name(const DwKArgs a) { dw3x3_body<F32, U8, RS, S, NT>(a); }
DW_KERNEL(dw3x3_i8_rows2_s1_u8, false, true, 2, 1, 256)
DW_KERNEL(dw3x3_i8_rows2_s1_s8, false, false, 2, 1, 256)
DW_KERNEL(dw3x3_i8_rows2_s2_u8, false, true, 2, 2, 256)
DW_KERNEL(dw3x3_i8_rows2_s2_s8, false, false, 2, 2, 256)
DW_KERNEL(dw3x3_i8_px_u8, false, true, 1, 0, 64)
DW_KERNEL(dw3x3_i8_px_s8, false, false, 1, 0, 64)
DW_KERNEL(dw3x3_f32_rows4_s1, true, false, 4, 1, 256)
DW_KERNEL(dw3x3_f32_rows4_s2, true, false, 4, 2, 256)
DW_KERNEL(dw3x3_f32_px, true, false, 1, 0, 64)
#undef DW_KERNEL

const char* conv_dw3x3_form_name(int form, bool f32) { return form == 1 ? (f32 ? "rows4" : "rows2") : (form == 2 ? "px" : ""); }

// the geometry the kernels are written for (the caller checks layouts, dtypes and the residual mode)
bool conv_dw3x3_ok(bool f32, int n, int c, int k, int group, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                   int dil_w, int oh, int ow) {
    if (group != c || k != c || kh != 3 || kw != 3 || dil_h != 1 || dil_w != 1) return false;
    if (stride_h != stride_w || (stride_h != 1 && stride_h != 2) || pad_h != pad_w || pad_h < 0 || pad_h > 1) return false;
    if (c % (f32 ? 4 : 16)) return false;
    return (size_t)n * oh * ow * (size_t)(c / (f32 ? 4 : 16)) < ((size_t)1 << 31);      // one lane per (channel vector, output pixel) at most
}

hipError_t launch_conv_dw3x3(int form, bool f32, const ConvKArgs& c, hipStream_t s) {
    if (form < 1 || form > DW3X3_FORMS) return hipErrorInvalidValue;
    const int rs = form == 1 ? (f32 ? 4 : 2) : 1, nt = form == 1 ? 256 : 64;
    DwKArgs a;
    a.x = c.x; a.w = c.w; a.y = c.y; a.bias = c.bias; a.scale = c.scale;
    a.H = c.H; a.W = c.W; a.C = c.C; a.OH = c.OH; a.OW = c.OW;
    a.stride = c.stride_h; a.pad = c.pad_h;
    a.cv = c.C / (f32 ? 4 : 16);
    a.nstrips = (c.OH + rs - 1) / rs;
    a.total = (unsigned)((size_t)c.N * a.nstrips * c.OW * a.cv);
    a.out_dtype = c.out_dtype; a.relu = c.relu; a.neg_slope = c.neg_slope;
    const dim3 grid((a.total + nt - 1) / nt), block(nt);
    const bool s2 = a.stride == 2, u8 = c.in_u8 != 0;
    if (f32) {
        if (form == 2) hipLaunchKernelGGL(dw3x3_f32_px, grid, block, 0, s, a);
        else if (s2) hipLaunchKernelGGL(dw3x3_f32_rows4_s2, grid, block, 0, s, a);
        else hipLaunchKernelGGL(dw3x3_f32_rows4_s1, grid, block, 0, s, a);
    } else if (form == 2) {
        if (u8) hipLaunchKernelGGL(dw3x3_i8_px_u8, grid, block, 0, s, a);
        else hipLaunchKernelGGL(dw3x3_i8_px_s8, grid, block, 0, s, a);
    } else if (s2) {
        if (u8) hipLaunchKernelGGL(dw3x3_i8_rows2_s2_u8, grid, block, 0, s, a);
        else hipLaunchKernelGGL(dw3x3_i8_rows2_s2_s8, grid, block, 0, s, a);
    } else {
        if (u8) hipLaunchKernelGGL(dw3x3_i8_rows2_s1_u8, grid, block, 0, s, a);
        else hipLaunchKernelGGL(dw3x3_i8_rows2_s1_s8, grid, block, 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace saber_mi355x
