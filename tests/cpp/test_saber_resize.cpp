// tests/cpp/test_saber_resize.cpp - SaberResize<MI355X, AK_FLOAT> through the Saber interface (init -> dispatch, the stand-in headers of
// include/saber_mi355x.hpp), in the style of the reference's test/saber/test_saber_resize.cpp: the four ResizeType modes over scales and
// explicit sizes, both layouts, every form the op accepts, against a host restatement of the reference's arithmetic in float32 (index and
// fraction in float steps, the four weights as double products rounded once, products and sums rounded to float). Pass: every output bit
// equal. An INT8 op type answers SaberUnImplError; a second input (the output size as a tensor) too.
// Built with the other C++ tests; run on the GPU by tests/test_gpu_resize.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "saber_mi355x.hpp"

using namespace anakin::saber;

static int g_fail = 0, g_run = 0;

struct Tap { int i0, i1; float fr; };
static Tap axis_tap(int mode, int in, int out, float scale, bool sizes, int o) {
    volatile float s, f = 0.f;
    if (mode == 0 || mode == 3) s = (float)(in - 1) / (float)(out - 1);
    else if (mode == 1) s = (float)in / (float)out;
    else { volatile float sc = sizes ? (float)out / (float)in : scale; s = 1.f / sc; }
    Tap t{0, 0, 0.f};
    if (mode == 3) {
        volatile float p = (float)o * s;
        t.i0 = t.i1 = (int)((double)p + 0.5);
        return t;
    }
    if (mode == 1) {
        volatile float a = (float)o + 0.5f;
        volatile float m = s * a;
        f = m - 0.5f;
        if (f < 0.f) f = 0.f;
    } else {
        f = (float)o * s;
    }
    t.i0 = (int)f;
    t.i1 = mode == 2 ? t.i0 + 1 : t.i0 + (t.i0 < in - 1 ? 1 : 0);
    volatile float fr = f - (float)t.i0;
    t.fr = fr;
    return t;
}

static void resize_case(int N, int C, int H, int W, int mode, float sh, float sw, int out_h, int out_w, bool in_nchw, bool out_nchw, unsigned seed,
                        Context<MI355X>& ctx) {
    std::mt19937 rng(seed);
    std::normal_distribution<float> nd(0.f, 1.f);
    const bool sizes = out_h != -1 && out_w != -1;
    volatile float ph = (float)H * sh, pw = (float)W * sw;
    const int OH = sizes ? out_h : (int)std::floor(ph), OW = sizes ? out_w : (int)std::floor(pw);
    std::vector<float> x((size_t)N * C * H * W), want((size_t)N * C * OH * OW);      // NCHW-logical
    for (auto& v : x) v = nd(rng);
    for (int oh = 0; oh < OH; ++oh)
        for (int ow = 0; ow < OW; ++ow) {
            const Tap th = axis_tap(mode, H, OH, sh, sizes, oh), tw = axis_tap(mode, W, OW, sw, sizes, ow);
            const float w00 = (float)((1.0 - th.fr) * (1.0 - tw.fr)), w01 = (float)(tw.fr * (1.0 - th.fr)), w10 = (float)(th.fr * (1.0 - tw.fr)),
                        w11 = (float)((double)tw.fr * th.fr);
            for (int n = 0; n < N; ++n)
                for (int c = 0; c < C; ++c) {
                    const float* p = &x[((size_t)n * C + c) * H * W];
                    float& o = want[(((size_t)n * C + c) * OH + oh) * OW + ow];
                    if (mode == 3) { o = p[th.i0 * W + tw.i0]; continue; }
                    const float tl = p[th.i0 * W + tw.i0], tr = tw.i1 < W ? p[th.i0 * W + tw.i1] : 0.f, bl = th.i1 < H ? p[th.i1 * W + tw.i0] : 0.f,
                                br = (tw.i1 < W && th.i1 < H) ? p[th.i1 * W + tw.i1] : 0.f;
                    volatile float a = w00 * tl, b = w01 * tr, cc = w10 * bl, d = w11 * br;
                    volatile float s1 = a + b;
                    volatile float s2 = s1 + cc;
                    volatile float s3 = s2 + d;
                    o = s3;
                }
        }
    auto to_layout = [&](const std::vector<float>& nchw, int hh, int ww, bool keep) {
        if (keep) return nchw;
        std::vector<float> o(nchw.size());
        for (int n = 0; n < N; ++n)
            for (int c = 0; c < C; ++c)
                for (int y = 0; y < hh; ++y)
                    for (int xx = 0; xx < ww; ++xx) o[(((size_t)n * hh + y) * ww + xx) * C + c] = nchw[(((size_t)n * C + c) * hh + y) * ww + xx];
        return o;
    };
    Tensor<MI355X> tin(in_nchw ? Shape({N, C, H, W}, Layout_NCHW) : Shape({N, H, W, C}, Layout_NHWC), AK_FLOAT);
    Tensor<MI355X> tout(out_nchw ? Shape({N, C, OH, OW}, Layout_NCHW) : Shape({N, OH, OW, C}, Layout_NHWC), AK_FLOAT);
    tin.copy_from_host(to_layout(x, H, W, in_nchw).data());
    const std::vector<float> want_l = to_layout(want, OH, OW, out_nchw);
    ResizeParam<MI355X> rp((ResizeType)mode, sw, sh, out_w, out_h);
    std::vector<Tensor<MI355X>*> ins{&tin}, outs{&tout};
    SaberResize<MI355X, AK_FLOAT> op;
    SaberStatus st = op.init(ins, outs, rp, ctx);
    std::vector<float> got(want.size());
    for (int form = 0; form < 2 && st == SaberSuccess; ++form) {
        if (op.set_tile(form) != 0) continue;      // a form this op does not have
        std::vector<float> fill(want.size(), 77.f);
        tout.copy_from_host(fill.data());
        st = op.dispatch(ins, outs, rp);
        (void)hipStreamSynchronize(ctx.get_compute_stream());
        tout.copy_to_host(got.data());
        ++g_run;
        if (st != SaberSuccess || std::memcmp(got.data(), want_l.data(), got.size() * 4) != 0) {
            ++g_fail;
            size_t diff = 0;
            for (size_t i = 0; i < got.size(); ++i) diff += std::memcmp(&got[i], &want_l[i], 4) != 0;
            printf("FAIL N=%d C=%d HxW=%dx%d mode=%d scale=%g,%g out=%d,%d nchw=%d,%d form=%d status=%d differing=%zu [%s]\n", N, C, H, W, mode, sh, sw, out_h,
                   out_w, in_nchw, out_nchw, form, (int)st, diff, op.algo());
        }
    }
    if (st != SaberSuccess && !g_fail) { ++g_fail; printf("FAIL init status=%d\n", (int)st); }
    SaberResize<MI355X, AK_INT8> op8;
    if (op8.init(ins, outs, rp, ctx) != SaberUnImplError) { ++g_fail; printf("FAIL AK_INT8 resize did not answer SaberUnImplError\n"); }
    std::vector<Tensor<MI355X>*> two{&tin, &tin};
    SaberResize<MI355X, AK_FLOAT> op2;
    if (op2.init(two, outs, rp, ctx) != SaberUnImplError) { ++g_fail; printf("FAIL the two-input form did not answer SaberUnImplError\n"); }
}

int main() {
    if (!saber_hip_device_ok()) {
        printf("no gfx950 device: the MI355X Saber target has no fallback\n");
        return 2;
    }
    Context<MI355X> ctx(0, 0, 0);
    unsigned seed = 1900;
    for (int mode = 0; mode < 4; ++mode) {
        resize_case(2, 8, 5, 7, mode, 0.f, 0.f, 11, 13, false, false, ++seed, ctx);       // explicit sizes, NHWC: forms 0 and 1
        resize_case(1, 4, 4, 6, mode, 2.f, 2.f, -1, -1, false, false, ++seed, ctx);        // x2 by scale
        resize_case(2, 3, 9, 11, mode, 0.f, 0.f, 4, 5, true, true, ++seed, ctx);           // downscale, NCHW
        resize_case(1, 5, 3, 5, mode, 2.5f, 1.5f, -1, -1, true, false, ++seed, ctx);       // unequal scales, NCHW -> NHWC
        resize_case(3, 12, 6, 1, mode, 0.f, 0.f, 12, 3, false, true, ++seed, ctx);         // an input axis of 1, NHWC -> NCHW
    }
    printf("%d/%d resize cases bit for bit\n", g_run - g_fail, g_run);
    return g_fail ? 1 : 0;
}
