// anakin_amd/csrc/conv_sep.hip - a depthwise 3x3 INT8 convolution and the pointwise 1x1 INT8 convolution that reads it, in one
// launch (gfx950): MobileNet-v1's separable pair (13 of them, C 32 .. 1024, K 64 .. 1024, stride 1 | 2), the counterpart of the
// ResNet chains of conv1x1_chain.hip. Two launches cost a kernel boundary (2.3 - 2.7 us on this part) and a write + re-read of the
// depthwise edge; here a workgroup keeps its tile of that edge in LDS.
//
//   workgroup = a tile of ROWS x 16 output pixels of one image x a slice of the pointwise conv's output channels (64 * kgroups of
//   them; a form that splits K over several workgroups has each of them recompute the depthwise tile - 9 multiply-adds per element,
//   cheap next to a second launch when there are only a few tiles: 7 x 7 x 1024 at batch 1 has 49 pixels). No workgroup talks to
//   another one: no atomics, no counters, no waiting; plain vector loads and stores.
//
//   phase 0, depthwise: work item = (tile pixel, 16-byte channel vector), channel vector fastest, so a wave reads consecutive
//   16-byte pieces of an input pixel. The arithmetic of conv_dw3x3.hip's one-pixel form: the true s8 / u8 activation times the s8
//   weight in int32, padded taps read as zero, then chain_out_pack (epilogue_pack.h). The 16 result bytes go to LDS as
//   mid[pixel][C] - and to y_dw from the workgroups of channel slice 0 when the edge is wanted. A u8 intermediate is stored XOR 0x80
//   (x - 128 as s8), the form the i8 MFMA takes; the pointwise op's comp = 128 * sum(w) corrects it, as in every u8-input kernel here.
//   Tile pixels beyond the image are CLAMPED to its last row / column (computed, never stored): every thread reaches the barrier.
//   The pixel pitch is C rounded up to a k-step of 64 bytes plus ONE 16-byte chunk: the 16 lanes of a fragment column (consecutive
//   pixels, same chunk) then hit 16 different bank groups (conv1x1_chain.hip: PCH). For C % 64 == 32 the second half of the last
//   k-step is zero in LDS and in the packed weights.
//
//   phase 1, pointwise, after one __syncthreads(): v_mfma_i32_16x16x64_i8 in the operand convention of conv_igemm_impl.h - weights
//   the A operand (row = lane & 15), the LDS tile the B operand (pixel = lane & 15), k-group = lane >> 4. A wave owns groups of 64
//   output channels (wave, wave + waves, ... of the workgroup's slice): 4 accumulators x ROWS pixel fragments. The host packs the
//   weights as 1 KB fragments [group][k-step][accumulator][lane] with row rho of accumulator mf = channel
//   group * 64 + (rho >> 2) * 16 + mf * 4 + (rho & 3), so a lane ends up with 16 CONSECUTIVE channels of its pixel: one 16-byte
//   store. Accumulators start at comp (exact integer sum, any order); epilogue = chain_out_pack with the pointwise op's constants.
//   K % 64 == 32: the last group's upper half has zero weights and is not stored.
//
// Results: y_pw, and y_dw where asked for, hold the bits of the two separate launches - the pointwise conv consumes exactly the
// bytes the depthwise one would have stored.
#include "epilogue_pack.h"

#include <atomic>
#include <vector>

namespace saber_mi355x {

typedef unsigned v4u __attribute__((ext_vector_type(4)));

template <bool U8>
__device__ __forceinline__ int sep_byte(unsigned v, int b) {
    return U8 ? (int)((v >> (8 * b)) & 0xffu) : (int)(int8_t)(v >> (8 * b));
}

template <bool U8, int ROWS>
__device__ __forceinline__ void sep_body(const SepKArgs& a) {
    extern __shared__ v4i sep_lds[];      // mid[NPX][pch]
    constexpr int NPX = 16 * ROWS;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int slice = (int)(blockIdx.x % (unsigned)a.nslices), t = (int)(blockIdx.x / (unsigned)a.nslices);
    const int n = t / a.tiles_per_img, rem = t - n * a.tiles_per_img;
    const int ty = rem / a.tiles_x;
    const int y0 = ty * ROWS, x0 = (rem - ty * a.tiles_x) * 16;
    const int cv = a.C >> 4;                       // channel vectors per pixel
    const int cvp = ((a.C + 63) >> 6) << 2;        // ... rounded up to whole k-steps
    const int pch = cvp + 1;                       // LDS pixel pitch in chunks

    // ================= phase 0: the depthwise conv of the tile -> LDS (and y_dw) ==================================================
    {
        const float lo = a.dw_relu ? 0.f : -3.0e38f;
        const float off = a.mid_u8 ? 0.f : 128.f;
        const unsigned xm = a.mid_u8 ? 0u : 0x80808080u;
        const unsigned lx = a.mid_u8 ? 0x80808080u : 0u;      // u8 -> the s8 form the MFMA reads
        const bool wr = a.y_dw != nullptr && slice == 0;
        const char* xn = (const char*)a.x + (size_t)n * a.H * a.W * a.C;
        // the channel vector whose 9 weight vectors and 8 constant vectors are in registers. Where cvp divides the workgroup's threads
        // (every power-of-two C, all of MobileNet's) a thread meets ONE channel vector and loads them once; for the other channel counts
        // (C = 96, 160, 192, ...: cvp = 8, 12, 12) the vector changes from item to item and they are loaded again per item - correct, not fast
        int cur = -1;
        v4u wv[9];
        v4f b[4], sc[4];
        for (int it = tid; it < NPX * cvp; it += nt) {
            const int px = it / cvp, cvi = it - px * cvp;
            v4u out = {0u, 0u, 0u, 0u};
            if (cvi < cv) {
                const size_t cbyte = (size_t)cvi * 16;
                if (cvi != cur) {
                    cur = cvi;
#pragma unroll
                    for (int tp = 0; tp < 9; ++tp) wv[tp] = *(const v4u*)((const char*)a.wdw + (size_t)tp * a.C + cbyte);
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        b[v] = *(const v4f*)(a.dw_bias + cvi * 16 + 4 * v);
                        sc[v] = *(const v4f*)(a.dw_scale + cvi * 16 + 4 * v);
                    }
                }
                const int oyu = y0 + (px >> 4), oxu = x0 + (px & 15);
                const bool ok = oyu < a.OH && oxu < a.OW;
                const int oy = oyu < a.OH ? oyu : a.OH - 1, ox = oxu < a.OW ? oxu : a.OW - 1;      // clamped: computed, not stored
                const int iy0 = oy * a.stride - a.pad, ix0 = ox * a.stride - a.pad;
                int acc[16];
#pragma unroll
                for (int c = 0; c < 16; ++c) acc[c] = 0;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const int iy = iy0 + i;
                    const bool rok = iy >= 0 && iy < a.H;
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const int ix = ix0 + j;
                        v4u xv = {0u, 0u, 0u, 0u};
                        if (rok && ix >= 0 && ix < a.W) xv = *(const v4u*)(xn + ((size_t)iy * a.W + ix) * a.C + cbyte);
                        const v4u wt = wv[i * 3 + j];
#pragma unroll
                        for (int c = 0; c < 16; ++c) acc[c] += sep_byte<U8>(xv[c >> 2], c & 3) * sep_byte<false>(wt[c >> 2], c & 3);
                    }
                }
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const v4i ac = {acc[4 * v], acc[4 * v + 1], acc[4 * v + 2], acc[4 * v + 3]};
                    out[v] = chain_out_pack(ac, v4i{0, 0, 0, 0}, b[v], sc[v], lo, off, xm);
                }
                if (wr && ok) *(v4u*)((char*)a.y_dw + (((size_t)n * a.OH + oy) * a.OW + ox) * a.C + cbyte) = out;
                out = out ^ v4u{lx, lx, lx, lx};
            }
            sep_lds[px * pch + cvi] = __builtin_bit_cast(v4i, out);
        }
    }
    __syncthreads();

    // ================= phase 1: the pointwise conv on the LDS tile ==================================================================
    const int lane = tid & 63, col = lane & 15, kg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = nt >> 6;
    const int ksn = cvp >> 2;                       // k-steps of 64 input channels
    const int gall = (a.K + 63) >> 6;
    const int g0 = slice * a.kgroups, g1 = g0 + a.kgroups < gall ? g0 + a.kgroups : gall;
    const float lo = a.pw_relu ? 0.f : -3.0e38f;
    const float off = a.out_u8 ? 0.f : 128.f;
    const unsigned xm = a.out_u8 ? 0u : 0x80808080u;
    for (int g = g0 + wave; g < g1; g += nw) {
        const int cg = g * 64 + kg * 16;            // the lane's 16 consecutive output channels
        const v4i* pp = (const v4i*)a.prm + (cg >> 2) * 3;
        v4i acc[4][ROWS];
#pragma unroll
        for (int mf = 0; mf < 4; ++mf)
#pragma unroll
            for (int j = 0; j < ROWS; ++j) acc[mf][j] = pp[mf * 3 + 2];
        const v4i* wl = (const v4i*)a.wpw + (size_t)g * ksn * 256 + lane;
        for (int ks = 0; ks < ksn; ++ks) {
            v4i bp[ROWS];
#pragma unroll
            for (int j = 0; j < ROWS; ++j) bp[j] = sep_lds[(j * 16 + col) * pch + ks * 4 + kg];
#pragma unroll
            for (int mf = 0; mf < 4; ++mf) {
                const v4i wf = wl[(ks * 4 + mf) * 64];
#pragma unroll
                for (int j = 0; j < ROWS; ++j) acc[mf][j] = mma_step(wf, bp[j], acc[mf][j]);
            }
        }
        if (cg >= a.K) continue;                    // (K % 64 == 32: the padded half of the last group)
        v4f sc[4], bi[4];
#pragma unroll
        for (int mf = 0; mf < 4; ++mf) {
            sc[mf] = __builtin_bit_cast(v4f, pp[mf * 3]);
            bi[mf] = __builtin_bit_cast(v4f, pp[mf * 3 + 1]);
        }
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            const int oy = y0 + j, ox = x0 + col;
            if (oy >= a.OH || ox >= a.OW) continue;
            v4u o;
#pragma unroll
            for (int mf = 0; mf < 4; ++mf) o[mf] = chain_out_pack(acc[mf][j], v4i{0, 0, 0, 0}, bi[mf], sc[mf], lo, off, xm);
            *(v4u*)((char*)a.y_pw + (((size_t)n * a.OH + oy) * a.OW + ox) * a.K + cg) = o;
        }
    }
}

// stable names: a kernel trace shows the tile height and the input type
#define SEP_KERNEL(name, U8, ROWS) \
    __global__ __launch_bounds__(256) void name(const SepKArgs a) { sep_body<U8, ROWS>(a); }
SEP_KERNEL(sep_dw3x3_pw_i8_r4_u8, true, 4)
SEP_KERNEL(sep_dw3x3_pw_i8_r4_s8, false, 4)
SEP_KERNEL(sep_dw3x3_pw_i8_r2_u8, true, 2)
SEP_KERNEL(sep_dw3x3_pw_i8_r2_s8, false, 2)
SEP_KERNEL(sep_dw3x3_pw_i8_r1_u8, true, 1)
SEP_KERNEL(sep_dw3x3_pw_i8_r1_s8, false, 1)
#undef SEP_KERNEL

// THE table of launch forms, in the autotuner's candidate order. kper 0: one workgroup per pixel tile computes every output channel.
static const struct { int code, rows, kper, waves; } sep_forms[] = {
    {1, 4, 0, 4},        // 64 pixels x all of K: the large early layers
    {2, 2, 0, 4},        // 32 pixels x all of K
    {3, 2, 256, 4},      // K split: 32 pixels x 256 channels, a 64-channel group per wave
    {4, 1, 256, 4},      // K split: 16 pixels x 256 channels
    {5, 1, 64, 1},       // K split: 16 pixels x 64 channels, one wave per workgroup - the 7 x 7 and 14 x 14 tails at batch 1
};
bool conv_sep_form(int code, int* rows, int* kper, int* waves) {
    for (const auto& f : sep_forms)
        if (f.code == code) {
            if (rows) *rows = f.rows;
            if (kper) *kper = f.kper;
            if (waves) *waves = f.waves;
            return true;
        }
    return false;
}
bool conv_sep_form_ok(int code, int c, int k) {
    int rows, kper, waves;
    if (!conv_sep_form(code, &rows, &kper, &waves)) return false;
    if (c % 32 || c < 32 || c > 1024 || k % 32 || k < 32) return false;
    return kper == 0 || kper < (k + 63) / 64 * 64;      // a splitting form needs at least two slices
}
size_t conv_sep_lds_bytes(int rows, int c) { return (size_t)16 * rows * ((c + 63) / 64 * 4 + 1) * 16; }

// the pointwise conv's weights [K][C] -> [group of 64 output channels][k-step of 64 input channels][accumulator 0..3][lane] x 16 bytes:
// lane (rho = lane & 15, kq = lane >> 4) of accumulator mf holds input channels ks * 64 + kq * 16 .. + 15 of output channel
// group * 64 + (rho >> 2) * 16 + mf * 4 + (rho & 3); zero beyond K and beyond C
void sep_pw_pack(const int8_t* w, int k, int c, std::vector<uint8_t>& out) {
    const int groups = (k + 63) / 64, ksn = (c + 63) / 64;
    out.assign((size_t)groups * ksn * 4 * 1024, 0);
    for (int g = 0; g < groups; ++g)
        for (int ks = 0; ks < ksn; ++ks)
            for (int mf = 0; mf < 4; ++mf)
                for (int lane = 0; lane < 64; ++lane) {
                    const int rho = lane & 15, kq = lane >> 4;
                    const int ch = g * 64 + (rho >> 2) * 16 + mf * 4 + (rho & 3), c0 = ks * 64 + kq * 16;
                    if (ch >= k || c0 >= c) continue;
                    uint8_t* dst = &out[((((size_t)g * ksn + ks) * 4 + mf) * 64 + lane) * 16];
                    for (int j = 0; j < 16; ++j) dst[j] = (uint8_t)w[(size_t)ch * c + c0 + j];
                }
}

static constexpr int SEP_LDS_MAX = 160 * 1024 - 64;
hipError_t conv_sep_prepare() {
    static std::atomic<bool> done[64];      // per device, zero-initialised; two threads that both find it unset set the same attributes
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess || dev < 0 || dev >= 64) return e != hipSuccess ? e : hipErrorInvalidDevice;
    if (done[dev].load(std::memory_order_acquire)) return hipSuccess;
    const void* fns[] = {(const void*)sep_dw3x3_pw_i8_r4_u8, (const void*)sep_dw3x3_pw_i8_r4_s8, (const void*)sep_dw3x3_pw_i8_r2_u8,
                         (const void*)sep_dw3x3_pw_i8_r2_s8, (const void*)sep_dw3x3_pw_i8_r1_u8, (const void*)sep_dw3x3_pw_i8_r1_s8};
    for (const void* f : fns)
        if ((e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, SEP_LDS_MAX)) != hipSuccess) return e;
    done[dev].store(true, std::memory_order_release);
    return hipSuccess;
}

// a.kgroups / a.nslices / a.tiles_* are set here from the form
hipError_t launch_conv_sep(int code, bool in_u8, const SepKArgs& a0, hipStream_t s) {
    int rows, kper, waves;
    if (!conv_sep_form(code, &rows, &kper, &waves) || !conv_sep_form_ok(code, a0.C, a0.K)) return hipErrorInvalidValue;
    if (a0.N <= 0 || a0.OH <= 0 || a0.OW <= 0 || !a0.x || !a0.y_pw) return hipErrorInvalidValue;
    SepKArgs a = a0;
    const int gall = (a.K + 63) / 64;
    a.kgroups = kper ? kper / 64 : gall;
    a.nslices = (gall + a.kgroups - 1) / a.kgroups;
    a.tiles_x = (a.OW + 15) / 16;
    a.tiles_per_img = a.tiles_x * ((a.OH + rows - 1) / rows);
    const size_t wgs = (size_t)a.N * a.tiles_per_img * a.nslices;
    const size_t lds = conv_sep_lds_bytes(rows, a.C);
    if (wgs >= ((size_t)1 << 31) || lds > (size_t)SEP_LDS_MAX) return hipErrorInvalidValue;
    hipError_t e = conv_sep_prepare();
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)wgs), block(64 * waves);
#define SEP_LAUNCH(k) hipLaunchKernelGGL(k, grid, block, lds, s, a)
    switch (rows * 2 + (in_u8 ? 0 : 1)) {
    case 8: SEP_LAUNCH(sep_dw3x3_pw_i8_r4_u8); break;
    case 9: SEP_LAUNCH(sep_dw3x3_pw_i8_r4_s8); break;
    case 4: SEP_LAUNCH(sep_dw3x3_pw_i8_r2_u8); break;
    case 5: SEP_LAUNCH(sep_dw3x3_pw_i8_r2_s8); break;
    case 2: SEP_LAUNCH(sep_dw3x3_pw_i8_r1_u8); break;
    case 3: SEP_LAUNCH(sep_dw3x3_pw_i8_r1_s8); break;
    default: return hipErrorInvalidValue;
    }
#undef SEP_LAUNCH
    return hipGetLastError();
}

}  // namespace saber_mi355x
