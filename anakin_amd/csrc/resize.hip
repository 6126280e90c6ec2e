// anakin_amd/csrc/resize.hip - FP32 resize (SaberResize; the reference: saber/funcs/resize.h, x86 saber/funcs/impl/x86/saber_resize.cpp,
// its four ResizeType modes). Bandwidth kernels: the output is scale_h * scale_w times the input and is written once.
//
// Which input rows / columns an output row / column reads, and with which fraction, is decided on the HOST (resize_axis_table below, in
// exactly the reference's float steps) and handed over as two small tables of OH and OW entries; the kernels only read tables.
//   bilinear:  w00 = float((1.0 - fh) * (1.0 - fw)), w01 = float(fw * (1.0 - fh)), w10 = float(fh * (1.0 - fw)), w11 = float(fw * fh)
//              (double products, each rounded to float once); y = ((w00 * tl + w01 * tr) + w10 * bl) + w11 * br, every product and sum
//              rounded to float32 (no fma). A tap whose index is >= the input size reads as 0 (RESIZE_CUSTOM's right / bottom edge).
//   nearest:   y = x[i0_h][i0_w], a copy.
// The fused sum: y = relu?(c0 * r + c1 * b) with r the resized value ROUNDED TO FLOAT FIRST and the expression of eltwise_sum_f32_kernel
// (elementwise.hip) - one launch equals resize followed by the eltwise launch bit for bit.
//
// resize_direct_f32 (form 0): one lane per output element in the output's own order, grid-stride; any mode / size / C, NCHW or NHWC on
// either side. resize_rows_f32 (form 1): NHWC on both sides, C % 4 == 0: a lane owns one float4 of channels of one output pixel, lanes run
// along the channels and then along the output row - 16-byte loads and stores, contiguous per pixel; the four weights (two table reads, four
// double products) are computed once per float4. resize_x2_f32 (form 2): an integer x2 in modes 1 and 3 under form 1's conditions: a lane
// owns a float4 of channels of one INPUT pixel, reads its 3 x 3 neighbourhood once and writes the cell's 2 x 2 output pixels. Per element
// all forms evaluate the same expression: bit-identical.
#include "kernels.h"

#include <cmath>

namespace saber_mi355x {

// ---- host: one axis of the index / fraction table, the reference's steps in float32 (volatile: every step is rounded to float, whatever
// the host compiler would like to contract) ------------------------------------------------------------------------------------------------
bool resize_axis_table(int mode, int in, int out, float scale, bool sizes_given, std::vector<ResizeTap>& t) {
    t.clear();
    if (in <= 0 || out <= 0 || mode < 0 || mode > 3) return false;
    if ((mode == 0 || mode == 3) && out == 1) return false;      // the reference divides by zero there
    volatile float s = 0.f;
    if (mode == 0 || mode == 3) {
        s = (float)(in - 1) / (float)(out - 1);
    } else if (mode == 1) {
        s = (float)in / (float)out;
    } else {
        volatile float sc = sizes_given ? (float)out / (float)in : scale;
        if (!(sc > 0.f)) return false;
        s = 1.f / sc;
    }
    t.resize((size_t)out);
    for (int o = 0; o < out; ++o) {
        ResizeTap e{0, 0, 0.f, 0};
        if (mode == 3) {
            volatile float p = (float)o * s;
            int idx = (int)((double)p + 0.5);
            if (idx < 0) idx = 0;
            e.i0 = e.i1 = idx;
        } else {
            volatile float f;
            if (mode == 1) {
                volatile float a = (float)o + 0.5f;
                volatile float m = s * a;
                f = m - 0.5f;
                if (f < 0.f) f = 0.f;
            } else {
                f = (float)o * s;
            }
            if (!(f >= 0.f) || f >= 2147483520.f) return false;
            e.i0 = (int)f;
            e.i1 = mode == 2 ? e.i0 + 1 : e.i0 + (e.i0 < in - 1 ? 1 : 0);
            volatile float fr = f - (float)e.i0;
            e.frac = fr;
        }
        if (e.i0 >= in) return false;
        t[(size_t)o] = e;
    }
    return true;
}

namespace {

__device__ __forceinline__ void resize_weights(float fh, float fw, float* w) {
    const double dh = (double)fh, dw = (double)fw;
    const double nh = __dsub_rn(1.0, dh), nw = __dsub_rn(1.0, dw);
    w[0] = (float)__dmul_rn(nh, nw);
    w[1] = (float)__dmul_rn(dw, nh);
    w[2] = (float)__dmul_rn(dh, nw);
    w[3] = (float)__dmul_rn(dw, dh);
}
__device__ __forceinline__ float resize_mix(const float* w, float tl, float tr, float bl, float br) {
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w[0], tl), __fmul_rn(w[1], tr)), __fmul_rn(w[2], bl)), __fmul_rn(w[3], br));
}
__device__ __forceinline__ float resize_sum(float r, float b, float c0, float c1, int relu) {
    const float t = __fadd_rn(__fmul_rn(c0, r), __fmul_rn(c1, b));
    return relu ? (t > 0.f ? t : 0.f) : t;
}

// form 0: gid is the output element's index in the output's own layout
template <bool NEAREST, bool FUSED>
__global__ __launch_bounds__(256) void resize_direct_f32_kernel(const ResizeKArgs a) {
    const size_t total = (size_t)a.N * a.OH * a.OW * a.C;
    for (size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (size_t)gridDim.x * 256) {
        int n, c, oh, ow;
        size_t r = gid;
        if (a.out_nchw) {
            ow = (int)(r % a.OW); r /= a.OW;
            oh = (int)(r % a.OH); r /= a.OH;
            c = (int)(r % a.C); n = (int)(r / a.C);
        } else {
            c = (int)(r % a.C); r /= a.C;
            ow = (int)(r % a.OW); r /= a.OW;
            oh = (int)(r % a.OH); n = (int)(r / a.OH);
        }
        const ResizeTap th = a.th[oh], tw = a.tw[ow];
        // element (ih, iw) of this image and channel
        const size_t base = a.in_nchw ? ((size_t)n * a.C + c) * a.H * a.W : (size_t)n * a.H * a.W * a.C + c;
        const size_t sh = a.in_nchw ? (size_t)a.W : (size_t)a.W * a.C, sw = a.in_nchw ? 1 : (size_t)a.C;
        float v;
        if (NEAREST) {
            v = a.x[base + th.i0 * sh + tw.i0 * sw];
        } else {
            const bool h1 = th.i1 < a.H, w1 = tw.i1 < a.W;
            const float tl = a.x[base + th.i0 * sh + tw.i0 * sw];
            const float tr = w1 ? a.x[base + th.i0 * sh + tw.i1 * sw] : 0.f;
            const float bl = h1 ? a.x[base + th.i1 * sh + tw.i0 * sw] : 0.f;
            const float br = (h1 && w1) ? a.x[base + th.i1 * sh + tw.i1 * sw] : 0.f;
            float w[4];
            resize_weights(th.frac, tw.frac, w);
            v = resize_mix(w, tl, tr, bl, br);
        }
        if (FUSED) v = resize_sum(v, a.b[gid], a.c0, a.c1, a.relu);
        a.y[gid] = v;
    }
}

// form 1: NHWC in and out, C % 4 == 0; gid = (output pixel, float4 of channels)
template <bool NEAREST, bool FUSED>
__global__ __launch_bounds__(256) void resize_rows_f32_kernel(const ResizeKArgs a) {
    const int c4n = a.C >> 2;
    const size_t total = (size_t)a.N * a.OH * a.OW * c4n;
    const float4* __restrict__ x = (const float4*)a.x;
    for (size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (size_t)gridDim.x * 256) {
        size_t r = gid;
        const int c4 = (int)(r % c4n); r /= c4n;
        const int ow = (int)(r % a.OW); r /= a.OW;
        const int oh = (int)(r % a.OH);
        const int n = (int)(r / a.OH);
        const ResizeTap th = a.th[oh], tw = a.tw[ow];
        const size_t row0 = ((size_t)n * a.H + th.i0) * a.W, row1 = ((size_t)n * a.H + th.i1) * a.W;
        float4 v;
        if (NEAREST) {
            v = x[(row0 + tw.i0) * c4n + c4];
        } else {
            const bool h1 = th.i1 < a.H, w1 = tw.i1 < a.W;
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 tl = x[(row0 + tw.i0) * c4n + c4];
            const float4 tr = w1 ? x[(row0 + tw.i1) * c4n + c4] : z;
            const float4 bl = h1 ? x[(row1 + tw.i0) * c4n + c4] : z;
            const float4 br = (h1 && w1) ? x[(row1 + tw.i1) * c4n + c4] : z;
            float w[4];
            resize_weights(th.frac, tw.frac, w);
            v = make_float4(resize_mix(w, tl.x, tr.x, bl.x, br.x), resize_mix(w, tl.y, tr.y, bl.y, br.y), resize_mix(w, tl.z, tr.z, bl.z, br.z),
                            resize_mix(w, tl.w, tr.w, bl.w, br.w));
        }
        if (FUSED) {
            const float4 b = ((const float4*)a.b)[gid];
            v = make_float4(resize_sum(v.x, b.x, a.c0, a.c1, a.relu), resize_sum(v.y, b.y, a.c0, a.c1, a.relu), resize_sum(v.z, b.z, a.c0, a.c1, a.relu),
                            resize_sum(v.w, b.w, a.c0, a.c1, a.relu));
        }
        ((float4*)a.y)[gid] = v;
    }
}

// form 2: integer x2 (OH = 2 H, OW = 2 W), NHWC in and out, C % 4 == 0, modes 1 and 3; gid = (INPUT pixel, float4 of channels). A lane reads
// its pixel's 3 x 3 neighbourhood once (nearest: the pixel alone) and writes the 2 x 2 output pixels of its cell, each with its own table
// entries and weights - the taps of output 2 i + a lie in rows i - 1 .. i + 1 (checked on the host: resize_x2_tables_ok), picked from
// registers. Per element the expression is form 0's: bit-identical.
__device__ __forceinline__ float4 sel3(const float4& a, const float4& b, const float4& c, int k) { return k == 0 ? a : (k == 1 ? b : c); }
template <bool NEAREST, bool FUSED>
__global__ __launch_bounds__(256) void resize_x2_f32_kernel(const ResizeKArgs a) {
    const int c4n = a.C >> 2;
    const size_t total = (size_t)a.N * a.H * a.W * c4n;
    const float4* __restrict__ x = (const float4*)a.x;
    for (size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (size_t)gridDim.x * 256) {
        size_t r = gid;
        const int c4 = (int)(r % c4n); r /= c4n;
        const int j = (int)(r % a.W); r /= a.W;
        const int i = (int)(r % a.H);
        const int n = (int)(r / a.H);
        float4 nb[3][3];
        if (NEAREST) {
            nb[1][1] = x[(((size_t)n * a.H + i) * a.W + j) * c4n + c4];
        } else {
#pragma unroll
            for (int dr = 0; dr < 3; ++dr) {
                const int rr = min(max(i - 1 + dr, 0), a.H - 1);
#pragma unroll
                for (int dc = 0; dc < 3; ++dc) {
                    const int cc = min(max(j - 1 + dc, 0), a.W - 1);
                    nb[dr][dc] = x[(((size_t)n * a.H + rr) * a.W + cc) * c4n + c4];
                }
            }
        }
#pragma unroll
        for (int pa = 0; pa < 2; ++pa) {
            const int oh = 2 * i + pa;
            const ResizeTap th = a.th[oh];
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) {
                const int ow = 2 * j + pb;
                float4 v;
                if (NEAREST) {
                    v = nb[1][1];
                } else {
                    const ResizeTap tw = a.tw[ow];
                    const int r0 = th.i0 - (i - 1), r1 = th.i1 - (i - 1), q0 = tw.i0 - (j - 1), q1 = tw.i1 - (j - 1);
                    const float4 t0[3] = {sel3(nb[0][0], nb[1][0], nb[2][0], r0), sel3(nb[0][1], nb[1][1], nb[2][1], r0), sel3(nb[0][2], nb[1][2], nb[2][2], r0)};
                    const float4 t1[3] = {sel3(nb[0][0], nb[1][0], nb[2][0], r1), sel3(nb[0][1], nb[1][1], nb[2][1], r1), sel3(nb[0][2], nb[1][2], nb[2][2], r1)};
                    const float4 tl = sel3(t0[0], t0[1], t0[2], q0), tr = sel3(t0[0], t0[1], t0[2], q1);
                    const float4 bl = sel3(t1[0], t1[1], t1[2], q0), br = sel3(t1[0], t1[1], t1[2], q1);
                    float w[4];
                    resize_weights(th.frac, tw.frac, w);
                    v = make_float4(resize_mix(w, tl.x, tr.x, bl.x, br.x), resize_mix(w, tl.y, tr.y, bl.y, br.y), resize_mix(w, tl.z, tr.z, bl.z, br.z),
                                    resize_mix(w, tl.w, tr.w, bl.w, br.w));
                }
                const size_t oi = (((size_t)n * a.OH + oh) * a.OW + ow) * c4n + c4;
                if (FUSED) {
                    const float4 b = ((const float4*)a.b)[oi];
                    v = make_float4(resize_sum(v.x, b.x, a.c0, a.c1, a.relu), resize_sum(v.y, b.y, a.c0, a.c1, a.relu), resize_sum(v.z, b.z, a.c0, a.c1, a.relu),
                                    resize_sum(v.w, b.w, a.c0, a.c1, a.relu));
                }
                ((float4*)a.y)[oi] = v;
            }
        }
    }
}

unsigned resize_grid(size_t lanes) {      // the streaming kernels' stride: at most 8 192 workgroups of 256 lanes
    size_t b = (lanes + 255) / 256;
    if (b > 8192) b = 8192;
    if (b == 0) b = 1;
    return (unsigned)b;
}

}  // namespace

bool resize_rows_ok(int c, int in_nchw, int out_nchw) { return c > 0 && c % 4 == 0 && !in_nchw && !out_nchw; }

// form 2's condition on the tables of one axis: out = 2 in; nearest: output o reads input o / 2; bilinear: both taps of output o lie within
// one input row / column of o / 2 and inside the input
bool resize_x2_tables_ok(bool nearest, int in, const std::vector<ResizeTap>& t) {
    if ((long long)t.size() != 2LL * in) return false;
    for (int o = 0; o < 2 * in; ++o) {
        const ResizeTap& e = t[(size_t)o];
        const int cell = o >> 1;
        if (nearest ? e.i0 != cell : (e.i0 < cell - 1 || e.i0 > cell + 1 || e.i1 < cell - 1 || e.i1 > cell + 1 || e.i0 < 0 || e.i1 >= in)) return false;
    }
    return true;
}

hipError_t launch_resize_f32(int form, const ResizeKArgs& a, hipStream_t s) {
    const bool fused = a.b != nullptr, nearest = a.nearest != 0;
    const size_t elems = (size_t)a.N * a.OH * a.OW * a.C;
    if (form == 2) {      // (the caller has checked the tables: resize_x2_tables_ok)
        if (!resize_rows_ok(a.C, a.in_nchw, a.out_nchw) || a.OH != 2 * a.H || a.OW != 2 * a.W) return hipErrorInvalidValue;
        const dim3 grid(resize_grid(elems / 16)), block(256);
        if (nearest && fused) hipLaunchKernelGGL((resize_x2_f32_kernel<true, true>), grid, block, 0, s, a);
        else if (nearest) hipLaunchKernelGGL((resize_x2_f32_kernel<true, false>), grid, block, 0, s, a);
        else if (fused) hipLaunchKernelGGL((resize_x2_f32_kernel<false, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((resize_x2_f32_kernel<false, false>), grid, block, 0, s, a);
        return hipGetLastError();
    }
    if (form == 1) {
        if (!resize_rows_ok(a.C, a.in_nchw, a.out_nchw)) return hipErrorInvalidValue;
        const dim3 grid(resize_grid(elems / 4)), block(256);
        if (nearest && fused) hipLaunchKernelGGL((resize_rows_f32_kernel<true, true>), grid, block, 0, s, a);
        else if (nearest) hipLaunchKernelGGL((resize_rows_f32_kernel<true, false>), grid, block, 0, s, a);
        else if (fused) hipLaunchKernelGGL((resize_rows_f32_kernel<false, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((resize_rows_f32_kernel<false, false>), grid, block, 0, s, a);
        return hipGetLastError();
    }
    if (form != 0) return hipErrorInvalidValue;
    const dim3 grid(resize_grid(elems)), block(256);
    if (nearest && fused) hipLaunchKernelGGL((resize_direct_f32_kernel<true, true>), grid, block, 0, s, a);
    else if (nearest) hipLaunchKernelGGL((resize_direct_f32_kernel<true, false>), grid, block, 0, s, a);
    else if (fused) hipLaunchKernelGGL((resize_direct_f32_kernel<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((resize_direct_f32_kernel<false, false>), grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace saber_mi355x
