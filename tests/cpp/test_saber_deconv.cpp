// tests/cpp/test_saber_deconv.cpp - SaberDeconv2D<MI355X, AK_FLOAT> through the Saber interface (init -> dispatch, the stand-in headers of
// include/saber_mi355x.hpp), in the style of the reference's test/saber/test_saber_deconv.cpp: a sweep over kernel / stride / pad /
// dilation / group / bias / relu / layout, every form the op accepts, against a double-precision scatter that restates the col2im rule
// (input pixel (ih, iw), tap (a, b) -> output (ih * stride - pad + a * dil, ...)). Pass: the project's two FP32 criteria at 1e-4; the
// bf16-plane forms bit-identical to each other. AK_INT8 answers SaberUnImplError, as the reference's stub does.
// Built with the other C++ tests; run on the GPU by tests/test_gpu_deconv.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "saber_mi355x.hpp"

using namespace anakin::saber;

static int g_fail = 0, g_run = 0;

static void deconv_case(int N, int C, int H, int W, int K, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int group, bool bias_term,
                        bool relu, bool in_nchw, bool out_nchw, unsigned seed, Context<MI355X>& ctx) {
    std::mt19937 rng(seed);
    std::normal_distribution<float> nd(0.f, 1.f);
    const int OH = (H - 1) * sh + dh * (kh - 1) + 1 - 2 * ph, OW = (W - 1) * sw + dw * (kw - 1) + 1 - 2 * pw;
    const int Cg = C / group, Kg = K / group;
    std::vector<float> x((size_t)N * C * H * W), w((size_t)C * Kg * kh * kw), b(K);      // x: NCHW-logical, w: [C][K / g][kh][kw]
    for (auto& v : x) v = nd(rng);
    for (auto& v : w) v = 0.3f * nd(rng);
    for (auto& v : b) v = nd(rng);
    std::vector<double> want((size_t)N * K * OH * OW, 0.0);
    for (int n = 0; n < N; ++n)
        for (int ci = 0; ci < C; ++ci)
            for (int ih = 0; ih < H; ++ih)
                for (int iw = 0; iw < W; ++iw) {
                    const double xv = x[(((size_t)n * C + ci) * H + ih) * W + iw];
                    for (int a = 0; a < kh; ++a)
                        for (int bb = 0; bb < kw; ++bb) {
                            const int oh = ih * sh - ph + a * dh, ow = iw * sw - pw + bb * dw;
                            if (oh < 0 || oh >= OH || ow < 0 || ow >= OW) continue;
                            for (int kl = 0; kl < Kg; ++kl)
                                want[(((size_t)n * K + (ci / Cg) * Kg + kl) * OH + oh) * OW + ow] += xv * w[(((size_t)ci * Kg + kl) * kh + a) * kw + bb];
                        }
                }
    double vmax = 0.0, vmean = 0.0;
    for (size_t i = 0; i < want.size(); ++i) {
        const int k = (int)(i / ((size_t)OH * OW) % K);
        if (bias_term) want[i] += b[k];
        if (relu && want[i] < 0.0) want[i] = 0.0;
        vmax = std::max(vmax, std::fabs(want[i]));
        vmean += std::fabs(want[i]);
    }
    vmean /= (double)want.size();

    auto to_layout = [&](const std::vector<float>& nchw, int ch, int hh, int ww, bool keep) {
        if (keep) return nchw;
        std::vector<float> o(nchw.size());
        for (int n = 0; n < N; ++n)
            for (int c = 0; c < ch; ++c)
                for (int y = 0; y < hh; ++y)
                    for (int xx = 0; xx < ww; ++xx) o[(((size_t)n * hh + y) * ww + xx) * ch + c] = nchw[(((size_t)n * ch + c) * hh + y) * ww + xx];
        return o;
    };
    Tensor<MI355X> tin(in_nchw ? Shape({N, C, H, W}, Layout_NCHW) : Shape({N, H, W, C}, Layout_NHWC), AK_FLOAT);
    Tensor<MI355X> tout(out_nchw ? Shape({N, K, OH, OW}, Layout_NCHW) : Shape({N, OH, OW, K}, Layout_NHWC), AK_FLOAT);
    tin.copy_from_host(to_layout(x, C, H, W, in_nchw).data());
    HostBlob hw(Shape({Kg, C, kh, kw}), AK_FLOAT, w.data());      // num() * group = output channels (deconv_compute_shape); the memory is [C][K / g][kh][kw]
    HostBlob hb(Shape({1, K, 1, 1}), AK_FLOAT, b.data());
    ActivationParam<MI355X> act = relu ? ActivationParam<MI355X>(Active_relu) : ActivationParam<MI355X>();
    ConvParam<MI355X> cp(group, ph, pw, sh, sw, dh, dw, &hw, bias_term ? &hb : nullptr, act);
    std::vector<Tensor<MI355X>*> ins{&tin}, outs{&tout};
    SaberDeconv2D<MI355X, AK_FLOAT> op;
    SaberStatus st = op.init(ins, outs, cp, ctx);
    std::vector<float> got(want.size()), first_b3;
    for (int form = 0; form < 3 && st == SaberSuccess; ++form) {
        if (op.set_tile(form) != 0) continue;      // a form this op does not have
        std::vector<float> fill(want.size(), 77.f);
        tout.copy_from_host(fill.data());
        st = op.dispatch(ins, outs, cp);
        (void)hipStreamSynchronize(ctx.get_compute_stream());
        tout.copy_to_host(got.data());
        ++g_run;
        double e_max = 0.0, e_el = 0.0;
        for (size_t i = 0; i < want.size(); ++i) {
            size_t gi = i;
            if (!out_nchw) {
                const int xx = (int)(i % OW), y = (int)(i / OW % OH), k = (int)(i / ((size_t)OW * OH) % K), n = (int)(i / ((size_t)OW * OH * K));
                gi = (((size_t)n * OH + y) * OW + xx) * K + k;
            }
            const double d = std::fabs((double)got[gi] - want[i]);
            e_max = std::max(e_max, d / std::max(vmax, 1e-30));
            e_el = std::max(e_el, d / (std::fabs(want[i]) + vmean + 1e-30));
        }
        bool bad = st != SaberSuccess || !(e_max <= 1e-4) || !(e_el <= 1e-4);
        if (form && first_b3.empty()) first_b3 = got;
        else if (form && std::memcmp(first_b3.data(), got.data(), got.size() * 4) != 0) bad = true;
        if (bad) {
            ++g_fail;
            printf("FAIL N=%d C=%d HxW=%dx%d K=%d k=%dx%d stride=%d,%d pad=%d,%d dil=%d,%d group=%d bias=%d relu=%d nchw=%d,%d form=%d status=%d e_max=%g e_el=%g [%s]\n",
                   N, C, H, W, K, kh, kw, sh, sw, ph, pw, dh, dw, group, bias_term, relu, in_nchw, out_nchw, form, (int)st, e_max, e_el, op.algo());
        }
    }
    if (st != SaberSuccess && !g_fail) { ++g_fail; printf("FAIL init status=%d\n", (int)st); }
    // the INT8 op type is the reference's stub
    SaberDeconv2D<MI355X, AK_INT8> op8;
    if (op8.init(ins, outs, cp, ctx) != SaberUnImplError) { ++g_fail; printf("FAIL AK_INT8 deconv did not answer SaberUnImplError\n"); }
}

int main() {
    if (!saber_hip_device_ok()) {
        printf("no gfx950 device: the MI355X Saber target has no fallback\n");
        return 2;
    }
    Context<MI355X> ctx(0, 0, 0);
    unsigned seed = 900;
    for (int bias : {0, 1})
        for (int relu : {0, 1}) {
            deconv_case(2, 32, 3, 5, 16, 2, 2, 2, 2, 0, 0, 1, 1, 1, bias, relu, false, false, ++seed, ctx);      // bf16-plane forms: k2 s2
            deconv_case(1, 64, 5, 7, 48, 4, 4, 2, 2, 1, 1, 1, 1, 1, bias, relu, false, false, ++seed, ctx);      // k4 s2 p1
            deconv_case(2, 32, 4, 6, 32, 3, 3, 2, 2, 1, 1, 1, 1, 1, bias, relu, false, false, ++seed, ctx);      // k3 s2 p1
            deconv_case(2, 8, 4, 5, 6, 3, 3, 1, 1, 1, 1, 1, 1, 2, bias, relu, true, true, ++seed, ctx);          // direct: group 2, NCHW
            deconv_case(1, 6, 5, 6, 7, 3, 3, 1, 1, 2, 2, 2, 2, 1, bias, relu, true, false, ++seed, ctx);         // dilation 2, NCHW -> NHWC
            deconv_case(2, 5, 4, 5, 4, 2, 3, 2, 1, 0, 1, 1, 1, 1, bias, relu, false, true, ++seed, ctx);         // per-axis geometry, NHWC -> NCHW
        }
    printf("%d/%d deconv cases within 1e-4\n", g_run - g_fail, g_run);
    return g_fail ? 1 : 0;
}
