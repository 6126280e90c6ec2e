// anakin_amd/csrc/conv1x1_gpool.hip - INT8 1x1 convolution 512 -> (1537 .. 2048) channels on <= 64 pixels per image
// (+ fused eltwise) + GLOBAL AVERAGE POOLING of its output, one launch (gfx950): ResNet's res5c_branch2c + res5c + pool5.
//
// Until now this op ran img_conv_kernel (stage_xcd.hip): the XCD-resident stage's phase body behind an ordinary grid. That
// body reads its StagePhase record from device memory before it can form an address, carries the 3x3 instance's registers,
// splits the 8-step reduction over the four waves (64 KB of int32 partials through LDS, one barrier) and pools through LDS
// behind a second barrier. None of that is needed for ONE 1x1 conv:
//   * every parameter arrives by value in the kernel arguments;
//   * workgroup = (image, 64 output channels) as before, grid = images x 32, but wave w owns channel tile w (16 channels),
//     the WHOLE reduction (8 k-steps) and all four 16-pixel fragments: 32 MFMAs and 8 weight fragments per wave as before,
//     no cross-wave reduction;
//   * the image (<= 64 pixels x 512 B) comes into LDS by DMA once (pixel pitch 528 B, a zero row for the unused pixel
//     slots); the wave's weights, constants and residual words are requested before the ONE wait and the ONE barrier;
//   * the pooling stays inside the wave: a lane holds 4 channels x its pixel of each fragment, so the 8-bit outputs are
//     summed over the fragments in registers and over the 16 pixel lanes by a butterfly; one lane per channel quad applies
//     the pooling op's arithmetic and stores 4 bytes.
// The weights are the stage packing ([cu][wave][k-step of the wave][tile][lane], pack_stage_weights with nt = 4, kq = 2),
// indexed for the other split. Outputs are the bits of img_conv_kernel's: int32 sums in any order are exact, the
// requantisation is epilogue_pack.h's, the pooling arithmetic is rintf((float)sum * (1 / hw)), saturated.
#include "epilogue_pack.h"

namespace saber_mi355x {

namespace {
constexpr int kCin = 512, kPch = kCin / 16 + 1;      // LDS pixel pitch in 16-byte chunks
constexpr int kImgChunks = ((64 + 1) * kPch + 63) / 64 * 64;
}  // namespace

__global__ __launch_bounds__(256) void conv1x1_gpool_kernel(const GpoolKArgs a) {
    __shared__ v4i img_lds[kImgChunks];
    SABER_TL_DECL;
    SABER_TL(0);
    // (every field live here: one batch of scalar loads for the kernel arguments, kernels.h pin_hot_args)
    asm volatile("" ::"s"(a.x), "s"(a.y), "s"(a.res), "s"(a.y_pool), "s"(a.w), "s"(a.prm), "s"(a.zero), "s"(a.hw), "s"(a.cout),
                 "s"(a.in_u8), "s"(a.relu), "s"(a.out_u8), "s"(a.elt), "s"(a.res_relu), "s"(a.coeff_conv), "s"(a.scale_conv),
                 "s"(a.coeff_res), "s"(a.scale_res), "s"(a.pool_idiv));
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fq = lane >> 4;
    const int cu = (int)(blockIdx.x & 31u), img = (int)(blockIdx.x >> 5);
    const int HW = a.hw, cout = a.cout;
    // ---- the image -> LDS: chunk L = pixel * kPch + c; pixels >= HW and chunk 32 of a pixel come from the zero page ----------
    {
        const char* xg = (const char*)a.x + (size_t)img * HW * kCin;
        const int nA = (int)(((unsigned)(HW + 1) * kPch + 63u) / 64u);
        for (int i = wave; i < nA; i += 4) {
            const unsigned L = (unsigned)(i * 64 + lane);
            const unsigned hp = L / (unsigned)kPch, cc = L - hp * kPch;
            const bool in = hp < (unsigned)HW && cc < (unsigned)(kCin / 16);
            const char* src = in ? xg + (size_t)hp * kCin + cc * 16 : (const char*)a.zero;
            lds_dma16(src, img_lds + i * 64);
        }
    }
    // ---- this wave's weights (tile `wave`, all 8 k-steps), constants and residual words: requested before the wait ------------
    v4i wreg[8];
    {
        const v4i* wp = (const v4i*)a.w + lane;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) wreg[ks] = wp[(size_t)((cu * 4 + ks / 2) * 8 + (ks % 2) * 4 + wave) * 64];
    }
    const int ch = cu * 64 + wave * 16 + fq * 4;         // this lane's 4 output channels
    const bool ch_ok = ch < cout;
    v4i prm[3];
    {
        const v4i* pp = (const v4i*)a.prm + (ch / 4) * 3;
#pragma unroll
        for (int r = 0; r < 3; ++r) prm[r] = pp[r];
    }
    const bool elt = a.elt != 0;
    unsigned rs[4] = {0u, 0u, 0u, 0u};
    if (elt) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int p = m * 16 + frow;             // (address select, not a branch: the load itself is unconditional)
            const char* rp = (p < HW && ch_ok) ? (const char*)a.res + ((size_t)img * HW + p) * cout + ch : (const char*)a.zero;
            rs[m] = *(const unsigned*)rp;
        }
    }
    SABER_TL(1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    SABER_TL(2);
    // ---- D[16 channels][64 pixel slots] = W[16][512] X[512][64] ----------------------------------------------------------------
    const int xmask = a.in_u8 ? (int)0x80808080u : 0;
    v4i acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = v4i{0, 0, 0, 0};
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        v4i bf[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int p = m * 16 + frow;
            const int q = p < HW ? p : HW;               // HW: the zero row
            v4i b = img_lds[q * kPch + ks * 4 + fq];
            b.x ^= xmask; b.y ^= xmask; b.z ^= xmask; b.w ^= xmask;
            bf[m] = b;
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[m] = mma_step(wreg[ks], bf[m], acc[m]);
    }
    SABER_TL(3);
    // ---- requantise, store y, pool ---------------------------------------------------------------------------------------------
    const float lo = a.relu ? 0.f : -3.0e38f;
    const float off = a.out_u8 ? 0.f : 128.f;
    const unsigned xo = a.out_u8 ? 0u : 0x80808080u;
    const float lo_s8 = a.relu ? 0.f : -128.f;
    const float res_lo = a.res_relu ? 0.f : -3.0e38f;
    struct { float coeff_conv, scale_conv, coeff_res, scale_res; } ec = {a.coeff_conv, a.scale_conv, a.coeff_res, a.scale_res};
    const bool u8o = a.out_u8 && !elt;                   // (the eltwise epilogue writes s8)
    char* yout = (char*)a.y + (size_t)img * HW * cout + ch;
    int ps[4] = {0, 0, 0, 0};
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int p = m * 16 + frow;
        unsigned o;
        if (elt) o = chain_elt_pack(acc[m], prm[2], __builtin_bit_cast(v4f, prm[1]), __builtin_bit_cast(v4f, prm[0]), rs[m], lo_s8, res_lo, ec);
        else o = chain_out_pack(acc[m], prm[2], __builtin_bit_cast(v4f, prm[1]), __builtin_bit_cast(v4f, prm[0]), lo, off, xo);
        if (p < HW && ch_ok) *(unsigned*)(yout + (size_t)p * cout) = o;
        // global average pooling of the 8-bit values just stored: exact int32 sums, the four fragments first (unused slots: 0)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int b = (int)((o >> (8 * t)) & 0xffu);
            const int v = u8o ? b : (int)(int8_t)b;
            ps[t] += p < HW ? v : 0;
        }
    }
    SABER_TL(4);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int s = 1; s < 16; s <<= 1) ps[t] += __shfl_xor(ps[t], s, 64);
    if (frow == 0 && ch_ok) {      // one lane per channel quad: the pooling op's arithmetic
        unsigned w = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float f = rintf(__fmul_rn((float)ps[t], a.pool_idiv));
            const int q = u8o ? (int)fminf(fmaxf(f, 0.f), 255.f) : (int)fminf(fmaxf(f, -128.f), 127.f);
            w |= (unsigned)(q & 0xff) << (8 * t);
        }
        *(unsigned*)((char*)a.y_pool + (size_t)img * cout + ch) = w;
    }
    SABER_TL(5);
    SABER_TL_FLUSH();
}

bool conv1x1_gpool_ok(int cin, int cout, int hw) { return cin == kCin && cout % 16 == 0 && cout > 1536 && cout <= 2048 && hw >= 1 && hw <= 64; }

hipError_t launch_conv1x1_gpool(const GpoolKArgs& a, hipStream_t s) {
    if (!conv1x1_gpool_ok(kCin, a.cout, a.hw) || a.n_img <= 0 || a.n_img > (1 << 20)) return hipErrorInvalidValue;
    if (!a.x || !a.y || !a.y_pool || !a.w || !a.prm || !a.zero || (a.elt && !a.res)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(conv1x1_gpool_kernel, dim3(a.n_img * 32), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace saber_mi355x
