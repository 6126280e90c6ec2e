// anakin_amd/csrc/conv_group3x3.hip - grouped 3x3 INT8 convolution on the i8 matrix cores: group > 1 with Cg == Kg in
// {4, 8, 16, 32, 64} channels per group, C % 64 == 0, dilation 1, stride 1 | 2, pad 0 | 1, NHWC 8-bit in, NHWC s8 / u8 / f32 out,
// no residual - ResNeXt's branch2b layers (32 groups of 4 .. 32 channels), which otherwise run on conv_direct_kernel
// (conv_igemm.hip: one output element per thread, a serial loop of 9 * Cg byte loads).
//
// A wave owns 16 x PT output pixels (consecutive in n * OH * OW) x one slab of 64 consecutive output channels. With Cg == Kg and
// Cg | 64 the slab's output channels read exactly the slab's 64 input channels: 64 contiguous bytes per pixel and tap. The
// reduction runs on v_mfma_i32_16x16x64_i8 in the operand convention of conv_igemm_impl.h: weights are the A operand
// (row = lane & 15 = output channel of a 16-channel row block), pixels the B operand (col = lane & 15), k-group = lane >> 4 picks
// the lane's 16-byte chunk of the 64-byte K-step; a lane ends up with 4 consecutive output channels of one pixel per row block.
// What the 64 bytes of one K-step of row block rb are depends on Cg:
//   Cg <= 16   4 taps x the row block's own 16 input channels: 3 steps (taps 9 .. 11 carry zero weights), B differs per row block.
//              Where the 16 channels span several groups (Cg 4 / 8) the weight fragment is block-diagonal - zero wherever the
//              input channel's group is not the row's; zero times a foreign byte is exact in integers;
//   Cg == 32   2 taps x the group's 32 channels: 5 steps (tap 9 zero), two row blocks share a B;
//   Cg == 64   1 tap x 64 channels: 9 steps, the four row blocks share B.
// Every lane loads its 16-byte operand chunks straight from global memory (no LDS, no barriers; plain vector loads and stores):
// the weights are packed in fragment order by saber_hip_conv2d_set_weights - [slab][row block][step][lane] x 16 bytes, so a wave
// reads 1 KB contiguous per fragment - and the 9-fold tap overlap of the activations is left to the vector L1, as in conv_dw3x3.hip.
// One form (launch_conv_group3x3 `form` 1, "w16"): PT = 1, 16 pixels per wave. PT = 4 - every weight fragment loaded once and used on
// four pixel tiles - was measured 1.4 - 2.8x slower than PT = 1 on all seven ResNeXt-50 shapes at batch 1 and 8 (13 - 16 us against
// 5.6 - 10.8 us per launch, profiles/group3x3/README.md: 124 - 156 VGPRs, a quarter of the waves) and is not instantiated.
//
// Arithmetic (the bits of conv_direct_kernel, which the tests compare against): the exact int32 sum of activation x weight over
// the taps inside the image. u8 activations are XORed with 0x80 on the way in (x - 128 as s8), an out-of-image tap is fed 0x80
// (s8 input: 0), and the exact int32 term comp[k] = 128 * sum(w[k]) corrects both; then the project's INT8 epilogue without
// contraction - (float)acc, + bias', * scale, relu, rintf, saturate (chain_out_pack, epilogue_pack.h) or the f32 store.
#include "epilogue_pack.h"

#include <vector>

namespace saber_mi355x {

struct GroupKArgs {
    const void* x;
    const void* w;        // fragment-ordered planes: [C / 64][4][steps][64 lanes][16]
    void* y;
    const float* bias;    // bias' (may be null)
    const float* scale;
    const int* comp;      // u8 input: 128 * sum(w[k])
    int H, W, C, OH, OW, M;
    int stride, pad;
    int nslab;            // C / 64
    unsigned nwaves;      // pixel tiles x slabs
    int out_dtype, relu;
};

// CGC: 0 = Cg <= 16, 1 = Cg == 32, 2 = Cg == 64
template <int CGC, bool U8, int PT>
__device__ __forceinline__ void g3x3_body(const GroupKArgs& a) {
    constexpr int NB = CGC == 0 ? 4 : (CGC == 1 ? 2 : 1);      // distinct B operands per step (= taps per step)
    constexpr int RPB = 4 / NB;                                // row blocks that share one
    constexpr int CPT = 4 / NB;                                // 16-byte chunks per tap
    constexpr int STEPS = (9 + NB - 1) / NB;
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= a.nwaves) return;
    const int lane = threadIdx.x & 63, col = lane & 15, kg = lane >> 4;
    const unsigned slab = wave % (unsigned)a.nslab, tile = wave / (unsigned)a.nslab;

    // the lane's pixel of each of the wave's PT tiles
    const char* xn[PT];
    int iy0[PT], ix0[PT];
    bool pok[PT];
    const int ohw = a.OH * a.OW;
#pragma unroll
    for (int t = 0; t < PT; ++t) {
        const int p = (int)((tile * PT + t) * 16u) + col;
        pok[t] = p < a.M;
        const int n = p / ohw, rem = p - n * ohw, oy = rem / a.OW, ox = rem - oy * a.OW;
        iy0[t] = oy * a.stride - a.pad;
        ix0[t] = ox * a.stride - a.pad;
        xn[t] = (const char*)a.x + (size_t)n * a.H * a.W * a.C + (size_t)slab * 64 + (size_t)(kg % CPT) * 16;
    }

    v4i acc[PT][4];
#pragma unroll
    for (int t = 0; t < PT; ++t)
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) acc[t][rb] = v4i{0, 0, 0, 0};

    const char* wl = (const char*)a.w + (size_t)slab * (4 * STEPS * 1024) + (size_t)lane * 16;
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
        const int tap = st * NB + kg / CPT;                    // the tap of the lane's chunk (9 .. 11: zero weights)
        const int ti = (tap * 11) >> 5, tj = tap - 3 * ti;      // tap / 3, tap % 3 for tap < 12
#pragma unroll
        for (int bs = 0; bs < NB; ++bs) {
            v4i b[PT];
#pragma unroll
            for (int t = 0; t < PT; ++t) {
                const int iy = iy0[t] + ti, ix = ix0[t] + tj;
                v4i v = {0, 0, 0, 0};
                if (pok[t] && tap < 9 && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                    v = *(const v4i*)(xn[t] + ((size_t)iy * a.W + ix) * a.C + bs * (64 / NB));
                if (U8) v = v ^ v4i{(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
                b[t] = v;
            }
#pragma unroll
            for (int r = 0; r < RPB; ++r) {
                const int rb = bs * RPB + r;
                const v4i wf = *(const v4i*)(wl + (size_t)(rb * STEPS + st) * 1024);
#pragma unroll
                for (int t = 0; t < PT; ++t) acc[t][rb] = mma_step(wf, b[t], acc[t][rb]);
            }
        }
    }

    // epilogue: the lane holds channels c0 .. c0 + 3 of its pixel per row block - one 4-byte (f32 output: 16-byte) NHWC store each
    const bool ou8 = a.out_dtype == DT_U8;
    const float lo = a.relu ? 0.f : -3.0e38f;
    const float off = ou8 ? 0.f : 128.f;
    const unsigned xm = ou8 ? 0u : 0x80808080u;
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        const int c0 = (int)slab * 64 + rb * 16 + kg * 4;
        const v4f bv = a.bias ? *(const v4f*)(a.bias + c0) : v4f{0.f, 0.f, 0.f, 0.f};      // ((float)acc + 0.f == (float)acc: the bits of "no bias")
        const v4f sc = *(const v4f*)(a.scale + c0);
        const v4i cp = U8 ? *(const v4i*)(a.comp + c0) : v4i{0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < PT; ++t) {
            if (!pok[t]) continue;
            const size_t o = (size_t)((int)((tile * PT + t) * 16u) + col) * a.C + c0;
            if (a.out_dtype == DT_F32) {
                v4f d;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float v = (float)(acc[t][rb][c] + cp[c]);
                    v = __fadd_rn(v, bv[c]);
                    v = __fmul_rn(v, sc[c]);
                    if (a.relu) v = v < 0.f ? 0.f : v;
                    d[c] = v;
                }
                *(v4f*)((float*)a.y + o) = d;
            } else {
                *(unsigned*)((char*)a.y + o) = chain_out_pack(acc[t][rb], cp, bv, sc, lo, off, xm);
            }
        }
    }
}

// stable names: a kernel trace shows which form, channel class and input type ran
#define G3X3_KERNEL(name, CGC, U8, PT) \
    __global__ __launch_bounds__(256) void name(const GroupKArgs a) { g3x3_body<CGC, U8, PT>(a); }
G3X3_KERNEL(g3x3_i8_w16_cg16_u8, 0, true, 1)
G3X3_KERNEL(g3x3_i8_w16_cg16_s8, 0, false, 1)
G3X3_KERNEL(g3x3_i8_w16_cg32_u8, 1, true, 1)
G3X3_KERNEL(g3x3_i8_w16_cg32_s8, 1, false, 1)
G3X3_KERNEL(g3x3_i8_w16_cg64_u8, 2, true, 1)
G3X3_KERNEL(g3x3_i8_w16_cg64_s8, 2, false, 1)
#undef G3X3_KERNEL

const char* conv_group3x3_form_name(int form) { return form == 1 ? "w16" : ""; }

int conv_group3x3_steps(int cg) { return cg <= 16 ? 3 : (cg == 32 ? 5 : 9); }

// the geometry the kernels are written for (the caller checks layouts, dtypes and the residual mode)
bool conv_group3x3_ok(int n, int c, int k, int group, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                      int oh, int ow) {
    if (group <= 1 || group == c || c % group || k != c || c % 64) return false;
    const int cg = c / group;
    if (cg != 4 && cg != 8 && cg != 16 && cg != 32 && cg != 64) return false;
    if (kh != 3 || kw != 3 || dil_h != 1 || dil_w != 1) return false;
    if (stride_h != stride_w || (stride_h != 1 && stride_h != 2) || pad_h != pad_w || pad_h < 0 || pad_h > 1) return false;
    return ((size_t)n * oh * ow + 64) * (size_t)(c / 64) < ((size_t)1 << 31);      // pixel index and wave count stay in 32 bits
}

// One weight fragment plane per (slab, row block, step): byte j of lane (r = lane & 15, kg = lane >> 4) is the weight of output
// channel slab * 64 + rb * 16 + r for the (tap, input channel) that byte of the K-step stands for; zero for taps >= 9 and for
// input channels outside the row's group. q: s8 weights [K][Cg][3][3].
void group3x3_pack(const int8_t* q, int c, int cg, std::vector<uint8_t>& out) {
    const int nb = cg <= 16 ? 4 : (cg == 32 ? 2 : 1), rpb = 4 / nb, cpt = 4 / nb, steps = conv_group3x3_steps(cg);
    out.assign((size_t)(c / 64) * 4 * steps * 1024, 0);
    for (int s = 0; s < c / 64; ++s)
        for (int rb = 0; rb < 4; ++rb)
            for (int st = 0; st < steps; ++st)
                for (int lane = 0; lane < 64; ++lane) {
                    const int r = lane & 15, kg = lane >> 4;
                    const int k = s * 64 + rb * 16 + r;
                    const int tap = st * nb + kg / cpt;
                    if (tap >= 9) continue;
                    uint8_t* dst = &out[((((size_t)s * 4 + rb) * steps + st) * 64 + lane) * 16];
                    for (int j = 0; j < 16; ++j) {
                        const int ci = s * 64 + (rb / rpb) * (64 / nb) + (kg % cpt) * 16 + j;
                        if (ci / cg != k / cg) continue;
                        dst[j] = (uint8_t)q[((size_t)k * cg + ci % cg) * 9 + tap];
                    }
                }
}

hipError_t launch_conv_group3x3(int form, const ConvKArgs& c, int group, hipStream_t s) {
    if (form < 1 || form > G3X3_FORMS || (c.in_u8 && !c.comp)) return hipErrorInvalidValue;
    const int pt = 1, cg = c.C / group;
    GroupKArgs a;
    a.x = c.x; a.w = c.w; a.y = c.y; a.bias = c.bias; a.scale = c.scale; a.comp = c.comp;
    a.H = c.H; a.W = c.W; a.C = c.C; a.OH = c.OH; a.OW = c.OW; a.M = c.M;
    a.stride = c.stride_h; a.pad = c.pad_h;
    a.nslab = c.C / 64;
    a.nwaves = (unsigned)(((size_t)c.M + 16 * pt - 1) / (16 * pt) * a.nslab);
    a.out_dtype = c.out_dtype; a.relu = c.relu;
    const dim3 grid((a.nwaves + 3) / 4), block(256);
    const int cgc = cg <= 16 ? 0 : (cg == 32 ? 1 : 2);
#define G3X3_LAUNCH(k) hipLaunchKernelGGL(k, grid, block, 0, s, a)
    switch (cgc * 2 + (c.in_u8 ? 0 : 1)) {
    case 0: G3X3_LAUNCH(g3x3_i8_w16_cg16_u8); break;
    case 1: G3X3_LAUNCH(g3x3_i8_w16_cg16_s8); break;
    case 2: G3X3_LAUNCH(g3x3_i8_w16_cg32_u8); break;
    case 3: G3X3_LAUNCH(g3x3_i8_w16_cg32_s8); break;
    case 4: G3X3_LAUNCH(g3x3_i8_w16_cg64_u8); break;
    default: G3X3_LAUNCH(g3x3_i8_w16_cg64_s8); break;
    }
#undef G3X3_LAUNCH
    return hipGetLastError();
}

}  // namespace saber_mi355x
