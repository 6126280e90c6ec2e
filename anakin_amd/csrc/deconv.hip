// anakin_amd/csrc/deconv.hip - FP32 transposed convolution (SaberDeconv2D; the reference: saber/funcs/deconv.h, x86 SaberCol2ImDeconv =
// GEMM + col2im). Both kernels GATHER: every output element is produced by one lane in one fixed order - no atomics, no zero-fill pass,
// no workspace - so two runs and two nets answer bit-identically whatever else the device does.
//
//   y[n, ko, oh, ow] = bias[ko] + sum x[n, ci, ih, iw] * w[ci, ko mod (K / g), a, b]
//       over ci in ko's group and the taps (a, b) with  oh = ih * stride_h - pad_h + a * dil_h  (ow likewise),  0 <= ih < H, 0 <= iw < W
//   OH = (H - 1) * stride_h + dil_h * (kh - 1) + 1 - 2 * pad_h      (no output padding);  relu = clamp at 0
//
// deconv_direct_f32 (form 0): one output element per lane, any group / dilation / per-axis geometry / layout / C / K. Taps row-major,
// channels ascending inside a tap, one fmaf per term. Weights repacked on the host to [tap][ci][K / g] (lanes along ko read contiguously).
//
// deconv_b3_f32 (forms 1, 2): stride 2, kh == kw in {2, 3, 4}, group 1, dilation 1, NHWC, C % 32 == 0, K % 16 == 0, on the bf16 matrix cores
// with the three-plane scheme of conv_igemm_impl.h (x = h + m + l exactly, six plane products in mma_step3's order, term-major over a
// wave's accumulators). Decomposed by OUTPUT PHASE: with t = oh + pad, phase r = t mod 2 and cell q = t div 2, phase r uses the taps
// a = r + 2 j < k on input row q - j. A stride-2 deconv is therefore four small stride-1 convs (k = 2: 1 tap each, a 1x1 conv C -> 4K stored
// pixel-shuffled; k = 4: 2 x 2 taps each; k = 3: 4 / 2 / 2 / 1 taps) over ONE input tile. A workgroup owns TH x 16 cells of one image x 64
// output channels; per 32-channel slab it stages the (TH + hal) x (16 + hal) input pixels those cells read (hal = ceil(k / 2) - 1 halo rows
// and columns above / left) ONCE into LDS as three bf16 planes - pixels outside the image are zero bytes - and runs all four phases from
// there; the accumulators of the four phases live across the slabs. Weight fragments never touch LDS: packed at set_weights as
// [phase][tap][32-deep slab][16-channel tile][plane][lane] x 16 bytes, streamed from global memory. A lane ends up with 4 consecutive
// output channels of one pixel: a store instruction covers 64 contiguous bytes per pixel. Cells whose output pixel falls outside
// [0, OH) x [0, OW) are computed and not stored. The reduction order of an output element - slabs ascending, taps row-major inside a
// slab, the six plane products - does not depend on the tile form: the forms are bit-identical to each other.
#include "conv_igemm_impl.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace saber_mi355x {

namespace {

__global__ __launch_bounds__(256) void deconv_direct_f32_kernel(const DeconvKArgs a) {
    const size_t total = (size_t)a.N * a.OH * a.OW * a.K;
    const int Cg = a.C / a.group, Kg = a.K / a.group;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        int n, ko, oh, ow;
        size_t r = idx;
        if (a.out_nchw) {
            ow = (int)(r % a.OW); r /= a.OW;
            oh = (int)(r % a.OH); r /= a.OH;
            ko = (int)(r % a.K); n = (int)(r / a.K);
        } else {
            ko = (int)(r % a.K); r /= a.K;
            ow = (int)(r % a.OW); r /= a.OW;
            oh = (int)(r % a.OH); n = (int)(r / a.OH);
        }
        const int g = ko / Kg, kl = ko - g * Kg;
        float acc = 0.f;
        for (int ta = 0; ta < a.kh; ++ta) {
            const int th = oh + a.pad_h - ta * a.dil_h;
            if (th < 0 || th % a.stride_h) continue;
            const int ih = th / a.stride_h;
            if (ih >= a.H) continue;
            for (int tb = 0; tb < a.kw; ++tb) {
                const int tw = ow + a.pad_w - tb * a.dil_w;
                if (tw < 0 || tw % a.stride_w) continue;
                const int iw = tw / a.stride_w;
                if (iw >= a.W) continue;
                const float* wp = a.w + ((size_t)(ta * a.kw + tb) * a.C + (size_t)g * Cg) * Kg + kl;
                if (a.in_nchw) {
                    const float* xp = a.x + (((size_t)n * a.C + (size_t)g * Cg) * a.H + ih) * a.W + iw;
                    const size_t hw = (size_t)a.H * a.W;
                    for (int ci = 0; ci < Cg; ++ci) acc = __fmaf_rn(xp[ci * hw], wp[(size_t)ci * Kg], acc);
                } else {
                    const float* xp = a.x + (((size_t)n * a.H + ih) * a.W + iw) * a.C + (size_t)g * Cg;
                    for (int ci = 0; ci < Cg; ++ci) acc = __fmaf_rn(xp[ci], wp[(size_t)ci * Kg], acc);
                }
            }
        }
        if (a.bias) acc = __fadd_rn(acc, a.bias[ko]);
        if (a.relu) acc = acc > 0.f ? acc : 0.f;
        a.y[idx] = acc;
    }
}

__device__ __forceinline__ int dc_swz(int row, int q) { return ((0x9C >> (2 * q)) & 3) ^ ((row >> 2) & 3); }

// KS: kernel size (2 | 3 | 4); TH: cell rows per workgroup (4 | 2); 4 waves = 2 (channel halves of the 64) x 2 (row halves of the tile),
// TM = 2 sixteen-channel tiles per wave
template <int KS, int TH>
__global__ __launch_bounds__(256) void deconv_b3_f32_kernel(const DeconvKArgs a) {
    constexpr int HAL = (KS + 1) / 2 - 1;
    constexpr int TW = 16, HWID = TW + HAL, HP = (TH + HAL) * HWID;
    constexpr int XCH = HP * 4;                      // 16-byte chunks of one plane of the tile (32 bf16 = 64 B per pixel)
    constexpr int XIT = (XCH + 255) / 256;
    constexpr int TM = 2, TN = TH / 2;
    constexpr int NT0 = (KS + 1) / 2, NT1 = KS / 2;  // taps of phase 0 / 1 along one axis

    __shared__ v4i lds[2][3][XCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int frow = lane & 15, fq = lane >> 4;

    // workgroup -> (image, cell tile, 64-channel block); channel blocks of one tile are neighbours (they read the same pixels)
    const int nky = (a.K + 63) >> 6;
    int b = blockIdx.x;
    const int ky = b % nky; b /= nky;
    const int tx = b % a.tiles_x; b /= a.tiles_x;
    const int ty = b % a.tiles_y;
    const int n = b / a.tiles_y;
    const int q0 = a.q0_h + ty * TH, c0 = a.q0_w + tx * TW;      // first cell of the tile
    const int ntile = a.K >> 4, nslab = a.C >> 5;

    // ---- staging: thread -> (tile pixel, 8-channel group) items, fixed for all slabs -----------------------------------------
    int x_off[XIT], x_dst[XIT];
#pragma unroll
    for (int it = 0; it < XIT; ++it) {
        const int idx = tid + it * 256;
        const int hp = idx >> 2, q = idx & 3;
        const int hy = hp / HWID, hx = hp - hy * HWID;
        const int iy = q0 - HAL + hy, ix = c0 - HAL + hx;
        const bool ok = idx < XCH && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
        x_off[it] = ok ? ((n * a.H + iy) * a.W + ix) * a.C + q * 8 : -1;       // in f32 elements (launcher: N * H * W * C < 2^31)
        x_dst[it] = idx < XCH ? hp * 4 + dc_swz(hp, q) : -1;
    }
    v4i xv[XIT][2];
    auto load_chunk = [&](int cc) {
#pragma unroll
        for (int it = 0; it < XIT; ++it) {
            xv[it][0] = v4i{0, 0, 0, 0};
            xv[it][1] = v4i{0, 0, 0, 0};
            if (x_off[it] >= 0) {
                const v4i* p = (const v4i*)(a.x + x_off[it] + cc * 32);
                xv[it][0] = p[0];
                xv[it][1] = p[1];
            }
        }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int it = 0; it < XIT; ++it) {
            if (x_dst[it] < 0) continue;
            const v4f f0 = __builtin_bit_cast(v4f, xv[it][0]), f1 = __builtin_bit_cast(v4f, xv[it][1]);
            unsigned h[4], m[4], l[4];
            split3_pair(f0.x, f0.y, h[0], m[0], l[0]);
            split3_pair(f0.z, f0.w, h[1], m[1], l[1]);
            split3_pair(f1.x, f1.y, h[2], m[2], l[2]);
            split3_pair(f1.z, f1.w, h[3], m[3], l[3]);
            lds[buf][0][x_dst[it]] = v4i{(int)h[0], (int)h[1], (int)h[2], (int)h[3]};
            lds[buf][1][x_dst[it]] = v4i{(int)m[0], (int)m[1], (int)m[2], (int)m[3]};
            lds[buf][2][x_dst[it]] = v4i{(int)l[0], (int)l[1], (int)l[2], (int)l[3]};
        }
    };

    // ---- weights: this wave's TM tiles (a tile past K / 16 re-reads the last one and is never stored) ---------------------------
    int wt[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int t = ky * 4 + wm * TM + i;
        wt[i] = (t < ntile ? t : ntile - 1) * (3 * 64) + lane;
    }
    const v4i* wf = (const v4i*)a.wfrag;

    v4f acc[4][TM][TN];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[p][i][j] = v4f{0.f, 0.f, 0.f, 0.f};

    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};      // mma_step3's order: small terms first
    for (int cc = 0; cc < nslab; ++cc) {
        const int buf = cc & 1;
        const bool more = cc + 1 < nslab;
        if (more) load_chunk(cc + 1);
        const v4i (*L)[XCH] = lds[buf];
        int tap = 0;      // running index into the stream's [phase][tap] order
#pragma unroll
        for (int rh = 0; rh < 2; ++rh)
#pragma unroll
            for (int rw = 0; rw < 2; ++rw)
#pragma unroll
                for (int ja = 0; ja < (rh ? NT1 : NT0); ++ja)
#pragma unroll
                    for (int jb = 0; jb < (rw ? NT1 : NT0); ++jb, ++tap) {
                        v4i af[TM][3], bf[TN][3];
                        const size_t wbase = (size_t)(tap * nslab + cc) * ntile * (3 * 64);
#pragma unroll
                        for (int i = 0; i < TM; ++i)
#pragma unroll
                            for (int pl = 0; pl < 3; ++pl) af[i][pl] = wf[wbase + wt[i] + pl * 64];
#pragma unroll
                        for (int j = 0; j < TN; ++j) {
                            const int hp = (wn * TN + j + HAL - ja) * HWID + frow + HAL - jb;
                            const int ci = hp * 4 + dc_swz(hp, fq);
#pragma unroll
                            for (int pl = 0; pl < 3; ++pl) bf[j][pl] = L[pl][ci];
                        }
#pragma unroll
                        for (int tt = 0; tt < 6; ++tt)
#pragma unroll
                            for (int i = 0; i < TM; ++i)
#pragma unroll
                                for (int j = 0; j < TN; ++j)
                                    acc[rh * 2 + rw][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                                        __builtin_bit_cast(v8bf, af[i][PA[tt]]), __builtin_bit_cast(v8bf, bf[j][PB[tt]]), acc[rh * 2 + rw][i][j], 0, 0, 0);
                    }
        if (more) {
            store_chunk(buf ^ 1);
            __syncthreads();
        }
    }

    // ---- epilogue: phase (rh, rw) of cell (q, c) is output pixel (2 q + rh - pad, 2 c + rw - pad) -------------------------------
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int t = ky * 4 + wm * TM + i;
        if (t >= ntile) continue;
        const int kb = t * 16 + fq * 4;
        const float4 bs = a.bias ? *(const float4*)(a.bias + kb) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float b4[4] = {bs.x, bs.y, bs.z, bs.w};
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int oh = 2 * (q0 + wn * TN + j) + (p >> 1) - a.pad_h, ow = 2 * (c0 + frow) + (p & 1) - a.pad_w;
                if (oh < 0 || oh >= a.OH || ow < 0 || ow >= a.OW) continue;
                float o[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float d = __fadd_rn(acc[p][i][j][r], b4[r]);
                    if (a.relu) d = d > 0.f ? d : 0.f;
                    o[r] = d;
                }
                *(float4*)(a.y + (((size_t)n * a.OH + oh) * a.OW + ow) * a.K + kb) = make_float4(o[0], o[1], o[2], o[3]);
            }
    }
}

}  // namespace

hipError_t launch_deconv_direct_f32(const DeconvKArgs& a, hipStream_t s) {
    const size_t total = (size_t)a.N * a.OH * a.OW * a.K;
    if (!total) return hipSuccess;
    const size_t blocks = std::min<size_t>((total + 255) / 256, (size_t)256 * 64);
    hipLaunchKernelGGL(deconv_direct_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

bool deconv_b3_form(int form, int* th) {
    if (form != 1 && form != 2) return false;
    *th = form == 1 ? 4 : 2;
    return true;
}
bool deconv_b3_ok(int n, int h, int w, int c, int k, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int group) {
    if (group != 1 || dil_h != 1 || dil_w != 1 || stride_h != 2 || stride_w != 2 || kh != kw || kh < 2 || kh > 4) return false;
    if (c < 32 || c % 32 || k < 16 || k % 16 || pad_h < 0 || pad_w < 0 || pad_h > kh - 1 || pad_w > kw - 1) return false;
    if (n < 1 || h < 1 || w < 1 || (double)n * h * w * c >= 2.0e9) return false;      // (the staging offsets are 32-bit element indices)
    return ((long long)h - 1) * 2 + kh - 2 * pad_h >= 1 && ((long long)w - 1) * 2 + kw - 2 * pad_w >= 1;
}
// the order of the fragment stream: phase = 2 rh + rw, then taps (ja, jb) row-major with a = rh + 2 ja, b = rw + 2 jb
int deconv_b3_taps(int ks, int (*ab)[2]) {
    int n = 0;
    for (int rh = 0; rh < 2; ++rh)
        for (int rw = 0; rw < 2; ++rw)
            for (int ja = 0; rh + 2 * ja < ks; ++ja)
                for (int jb = 0; rw + 2 * jb < ks; ++jb) {
                    if (ab) { ab[n][0] = rh + 2 * ja; ab[n][1] = rw + 2 * jb; }
                    ++n;
                }
    return n;
}
static void bf16_split3(float x, uint16_t* out) {      // x = h + m + l, conversions round to nearest even (split3_pair on the host)
    auto to_bf = [](float v) -> uint16_t {
        uint32_t u;
        std::memcpy(&u, &v, 4);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
        u += 0x7fffu + ((u >> 16) & 1u);
        return (uint16_t)(u >> 16);
    };
    auto from_bf = [](uint16_t b) -> float {
        const uint32_t u = (uint32_t)b << 16;
        float v;
        std::memcpy(&v, &u, 4);
        return v;
    };
    float r = x;
    for (int pl = 0; pl < 3; ++pl) {
        out[pl] = to_bf(r);
        r = r - from_bf(out[pl]);
    }
}
void deconv_b3_pack(const float* w_ckab, int c, int k, int ks, std::vector<uint8_t>& out) {
    int ab[16][2];
    const int ntap = deconv_b3_taps(ks, ab), nslab = c / 32, ntile = k / 16;
    out.assign((size_t)ntap * nslab * ntile * 3 * 64 * 16, 0);
    uint16_t* o = (uint16_t*)out.data();
    for (int t = 0; t < ntap; ++t)
        for (int s = 0; s < nslab; ++s)
            for (int tile = 0; tile < ntile; ++tile)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int ci = 32 * s + 8 * (lane >> 4) + j, ko = 16 * tile + (lane & 15);
                        uint16_t p3[3];
                        bf16_split3(w_ckab[(((size_t)ci * k + ko) * ks + ab[t][0]) * ks + ab[t][1]], p3);
                        const size_t frag = ((size_t)(t * nslab + s) * ntile + tile) * 3;
                        for (int pl = 0; pl < 3; ++pl) o[((frag + pl) * 64 + lane) * 8 + j] = p3[pl];
                    }
}
hipError_t launch_deconv_b3_f32(int form, const DeconvKArgs& a, hipStream_t s) {
    int th;
    if (!deconv_b3_form(form, &th) || !a.wfrag || a.in_nchw || a.out_nchw ||
        !deconv_b3_ok(a.N, a.H, a.W, a.C, a.K, a.kh, a.kw, a.stride_h, a.stride_w, a.pad_h, a.pad_w, a.dil_h, a.dil_w, a.group))
        return hipErrorInvalidValue;
    DeconvKArgs b = a;
    // cells: t = o + pad runs over [pad, O - 1 + pad]
    b.q0_h = a.pad_h / 2;
    b.q0_w = a.pad_w / 2;
    const int qh = (a.OH - 1 + a.pad_h) / 2 - b.q0_h + 1, qw = (a.OW - 1 + a.pad_w) / 2 - b.q0_w + 1;
    b.tiles_y = (qh + th - 1) / th;
    b.tiles_x = (qw + 15) / 16;
    const long long grid = (long long)a.N * b.tiles_y * b.tiles_x * ((a.K + 63) / 64);
    if (grid <= 0 || grid > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 g((unsigned)grid), blk(256);
#define DECONV_B3(KS)                                                                        \
    if (th == 4) hipLaunchKernelGGL((deconv_b3_f32_kernel<KS, 4>), g, blk, 0, s, b);         \
    else hipLaunchKernelGGL((deconv_b3_f32_kernel<KS, 2>), g, blk, 0, s, b);
    if (a.kh == 2) { DECONV_B3(2) }
    else if (a.kh == 3) { DECONV_B3(3) }
    else { DECONV_B3(4) }
#undef DECONV_B3
    return hipGetLastError();
}

}  // namespace saber_mi355x
