// anakin_amd/csrc/api_deconv.hip - transposed convolution (saber_hip_deconv2d_*): the reference's Deconv<T, AK_FLOAT> (saber/funcs/deconv.h;
// x86 SaberCol2ImDeconv = GEMM + col2im). FP32 only - the reference's AK_INT8 deconv is an unimplemented stub. A type of its own: the conv
// selection tables know nothing of it.
#include "api_internal.h"

static inline int deconv_out(int in, int pad, int k, int dil, int stride) {      // deconv_compute_shape, funcs_utils.h:56-82
    const long long o = ((long long)in - 1) * stride + (long long)dil * (k - 1) + 1 - 2LL * pad;
    return o < 1 || o > 0x7fffffffLL ? 0 : (int)o;
}

bool deconv_form_valid(const saber_hip_deconv* op, int form) {
    int th;
    return form == 0 || (op->b3_ok && deconv_b3_form(form, &th));
}
void for_each_deconv_form(const saber_hip_deconv* op, const std::function<void(int form)>& fn) {
    for (int f = 0; f <= DECONV_B3_FORMS; ++f)
        if (deconv_form_valid(op, f)) fn(f);
}
// The static rule names a bf16-plane form only for the measured rows where it was not above form 0 by more than form 0's own spread on both
// protocols (cold and warm windows; profiles/deconv/README.md), keyed by the op's shape as sep_static_form is. Everything else runs form 0
// unless autotuned.
int deconv_static_form(const saber_hip_deconv* op) {
    if (!op->b3_ok) return 0;
    struct Row { int n, hw, c, k, ks, pad, form; };      // batch, H = W, C, K, kh = kw, pad_h = pad_w
    static const Row rows[] = {      // written by `scripts/bench_deconv.py table`: the fastest form within form 0's spread on both protocols
        {1, 28, 1024, 512, 2, 0, 2},      // 1024 -> 512 @ 28^2 k2 p0 batch 1: 78.6 us against 669.6 (cold), 75.2 against 528.9 (warm)
        {8, 28, 1024, 512, 2, 0, 2},      // 1024 -> 512 @ 28^2 k2 p0 batch 8: 198.9 us against 4169.8 (cold), 195.8 against 4047.5 (warm)
        {1, 56, 512, 256, 2, 0, 2},      // 512 -> 256 @ 56^2 k2 p0 batch 1: 45.0 us against 586.1 (cold), 41.2 against 478.8 (warm)
        {8, 56, 512, 256, 2, 0, 2},      // 512 -> 256 @ 56^2 k2 p0 batch 8: 205.3 us against 4162.6 (cold), 205.5 against 4092.2 (warm)
        {1, 112, 256, 128, 2, 0, 2},      // 256 -> 128 @ 112^2 k2 p0 batch 1: 36.9 us against 562.8 (cold), 33.8 against 507.0 (warm)
        {8, 112, 256, 128, 2, 0, 1},      // 256 -> 128 @ 112^2 k2 p0 batch 8: 213.1 us against 4570.2 (cold), 202.1 against 4412.0 (warm)
        {1, 224, 128, 64, 2, 0, 2},      // 128 -> 64 @ 224^2 k2 p0 batch 1: 38.2 us against 580.0 (cold), 34.6 against 562.5 (warm)
        {1, 8, 512, 256, 4, 1, 2},      // 512 -> 256 @ 8^2 k4 p1 batch 1: 151.1 us against 510.2 (cold), 93.8 against 301.3 (warm)
        {8, 8, 512, 256, 4, 1, 2},      // 512 -> 256 @ 8^2 k4 p1 batch 8: 149.8 us against 711.9 (cold), 112.8 against 606.1 (warm)
        {1, 16, 256, 128, 4, 1, 2},      // 256 -> 128 @ 16^2 k4 p1 batch 1: 78.2 us against 259.1 (cold), 36.7 against 118.1 (warm)
        {8, 16, 256, 128, 4, 1, 2},      // 256 -> 128 @ 16^2 k4 p1 batch 8: 81.4 us against 507.6 (cold), 52.7 against 359.1 (warm)
        {1, 32, 128, 64, 4, 1, 2},      // 128 -> 64 @ 32^2 k4 p1 batch 1: 44.8 us against 134.3 (cold), 20.6 against 62.9 (warm)
        {8, 32, 128, 64, 4, 1, 2},      // 128 -> 64 @ 32^2 k4 p1 batch 8: 47.2 us against 407.1 (cold), 29.7 against 316.4 (warm)
        {1, 64, 64, 32, 4, 1, 2},      // 64 -> 32 @ 64^2 k4 p1 batch 1: 23.0 us against 191.8 (cold), 12.5 against 118.5 (warm)
        {8, 64, 64, 32, 4, 1, 2},      // 64 -> 32 @ 64^2 k4 p1 batch 8: 46.5 us against 699.1 (cold), 43.4 against 598.7 (warm)
        {1, 28, 256, 128, 3, 1, 1},      // 256 -> 128 @ 28^2 k3 p1 batch 1: 66.8 us against 264.1 (cold), 32.5 against 125.1 (warm)
        {8, 28, 256, 128, 3, 1, 1},      // 256 -> 128 @ 28^2 k3 p1 batch 8: 69.8 us against 832.3 (cold), 44.8 against 715.8 (warm)
    };
    const saber_hip_conv_desc& d = op->d;
    for (const Row& r : rows)
        if (r.n == d.n && r.hw == d.h && d.h == d.w && r.c == d.c && r.k == d.k && r.ks == d.kh && r.pad == d.pad_h && d.pad_h == d.pad_w) return r.form;
    return 0;
}
static const char* deconv_form_name(int form) { return form == 1 ? "deconv_b3_f32_4x16" : (form == 2 ? "deconv_b3_f32_2x16" : "deconv_direct_f32"); }
// the one writer of op->form: the fragment stream is packed when a bf16-plane form is first selected on an op that has its weights
static int deconv_set_form(saber_hip_deconv* op, int form) {
    if (!deconv_form_valid(op, form)) return fail(SABER_HIP_INVALID_VALUE, "deconv: no such form for this op (0 direct; 1 | 2 the bf16-plane tiles: group 1, dilation 1, NHWC f32, c % 32 == 0, k % 16 == 0, stride 2, kh == kw in 2 .. 4, pad <= kh - 1)");
    if (form && op->weights_set && !op->d_wfrag.p) {
        std::vector<uint8_t> frag;
        deconv_b3_pack(op->w_host.data(), op->d.c, op->d.k, op->d.kh, frag);
        HIP_TRY(op->d_wfrag.upload(frag));
    }
    op->form = form;
    op->algo_name = deconv_form_name(form);
    return SABER_HIP_OK;
}

int saber_hip_deconv2d_create(const saber_hip_conv_desc* desc, saber_hip_deconv_t** out) {
    if (!desc || !out) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    *out = nullptr;
    const saber_hip_conv_desc& d = *desc;
    if (d.n <= 0 || d.h <= 0 || d.w <= 0 || d.c <= 0 || d.k <= 0 || d.kh <= 0 || d.kw <= 0 || d.stride_h <= 0 || d.stride_w <= 0 || d.dil_h <= 0 ||
        d.dil_w <= 0 || d.group <= 0 || d.pad_h < 0 || d.pad_w < 0)
        return fail(SABER_HIP_INVALID_VALUE, "deconv: bad geometry");
    if (d.c % d.group || d.k % d.group) return fail(SABER_HIP_INVALID_VALUE, "deconv: c and k must be multiples of group");
    if (d.int8_weights || d.in_dtype != SABER_HIP_F32 || d.out_dtype != SABER_HIP_F32)
        return fail(SABER_HIP_UNIMPL, "deconv: FP32 only (the reference's AK_INT8 deconv is an unimplemented stub)");
    if (d.res_mode || d.res_act || d.res_stride || d.res_h || d.res_w || d.res_has_dtype || d.res_dtype)
        return fail(SABER_HIP_INVALID_VALUE, "deconv: no residual mode (the res_* fields must be zero)");
    if ((d.in_layout != SABER_HIP_NHWC && d.in_layout != SABER_HIP_NCHW) || (d.out_layout != SABER_HIP_NHWC && d.out_layout != SABER_HIP_NCHW))
        return fail(SABER_HIP_INVALID_VALUE, "deconv: layout is NHWC or NCHW");
    if (d.act != SABER_HIP_ACT_NONE && d.act != SABER_HIP_ACT_RELU) return fail(SABER_HIP_INVALID_VALUE, "deconv: the activation is none or relu");
    if (!(d.act_negative_slope == 0.f)) return fail(SABER_HIP_INVALID_VALUE, "deconv: negative_slope must be 0 (the reference's deconv relu is a clamp at 0)");
    if (d.kh > 1024 || d.kw > 1024 || d.dil_h > 65536 || d.dil_w > 65536 || d.stride_h > 65536 || d.stride_w > 65536)
        return fail(SABER_HIP_INVALID_VALUE, "deconv: bad geometry");
    const int oh = deconv_out(d.h, d.pad_h, d.kh, d.dil_h, d.stride_h), ow = deconv_out(d.w, d.pad_w, d.kw, d.dil_w, d.stride_w);
    if (!oh || !ow) return fail(SABER_HIP_INVALID_VALUE, "deconv: bad geometry (empty output)");
    if ((double)d.n * oh * ow * d.k >= 9.0e18 || (double)d.n * d.h * d.w * d.c >= 9.0e18 || (double)d.c * (d.k / d.group) * d.kh * d.kw >= 2.0e9)
        return fail(SABER_HIP_INVALID_VALUE, "deconv: tensor too large");
    saber_hip_deconv* op = new saber_hip_deconv();
    op->d = d;
    op->oh = oh;
    op->ow = ow;
    op->b3_ok = d.in_layout == SABER_HIP_NHWC && d.out_layout == SABER_HIP_NHWC && (double)d.n * oh * ow * d.k < 2.0e9 &&
                deconv_b3_ok(d.n, d.h, d.w, d.c, d.k, d.kh, d.kw, d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w, d.group);
    (void)deconv_set_form(op, deconv_static_form(op));
    *out = op;
    return SABER_HIP_OK;
}

int saber_hip_deconv2d_set_weights(saber_hip_deconv_t* op, const float* w, const float* bias) {
    if (!op || !w) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    const saber_hip_conv_desc& d = op->d;
    const int kg = d.k / d.group, taps = d.kh * d.kw;
    const size_t nw = (size_t)d.c * kg * taps;
    op->w_host.assign(w, w + nw);
    std::vector<float> rp(nw);      // [tap][c][k / group]
    for (int ci = 0; ci < d.c; ++ci)
        for (int kl = 0; kl < kg; ++kl)
            for (int t = 0; t < taps; ++t) rp[((size_t)t * d.c + ci) * kg + kl] = w[((size_t)ci * kg + kl) * taps + t];
    // every packing follows: a live op is drained first, then all device buffers are replaced (none keeps planes of the old weights)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(op->d_w.upload(rp));
    op->d_bias.release();
    op->has_bias = bias != nullptr;
    if (bias) HIP_TRY(op->d_bias.upload(std::vector<float>(bias, bias + d.k)));
    op->d_wfrag.release();
    op->weights_set = true;
    return deconv_set_form(op, op->form);
}

void saber_hip_deconv2d_out_shape(const saber_hip_deconv_t* op, int* oh, int* ow) {
    if (oh) *oh = op ? op->oh : 0;
    if (ow) *ow = op ? op->ow : 0;
}
const char* saber_hip_deconv2d_algo(const saber_hip_deconv_t* op) { return op ? op->algo_name.c_str() : ""; }
int saber_hip_deconv2d_set_tile(saber_hip_deconv_t* op, int form) {
    if (!op) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    return deconv_set_form(op, form);
}
int saber_hip_deconv2d_get_tile(const saber_hip_deconv_t* op) { return op ? op->form : 0; }
void saber_hip_deconv2d_destroy(saber_hip_deconv_t* op) { delete op; }

int saber_hip_deconv2d_run(saber_hip_deconv_t* op, const void* x, void* y, saber_hip_stream_t stream) {
    if (!op || !x || !y) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    if (!op->weights_set) return fail(SABER_HIP_INVALID_VALUE, "set_weights not called");
    if (g_capture) return capture_deconv(op, x, y);
    const saber_hip_conv_desc& d = op->d;
    DeconvKArgs a{};
    a.x = (const float*)x;
    a.w = op->d_w.p;
    a.wfrag = op->d_wfrag.p;
    a.bias = op->has_bias ? op->d_bias.p : nullptr;
    a.y = (float*)y;
    a.N = d.n; a.H = d.h; a.W = d.w; a.C = d.c; a.K = d.k; a.OH = op->oh; a.OW = op->ow;
    a.kh = d.kh; a.kw = d.kw; a.stride_h = d.stride_h; a.stride_w = d.stride_w; a.pad_h = d.pad_h; a.pad_w = d.pad_w;
    a.dil_h = d.dil_h; a.dil_w = d.dil_w; a.group = d.group;
    a.in_nchw = d.in_layout == SABER_HIP_NCHW; a.out_nchw = d.out_layout == SABER_HIP_NCHW; a.relu = d.act == SABER_HIP_ACT_RELU;
    if (op->form) HIP_TRY(launch_deconv_b3_f32(op->form, a, (hipStream_t)stream));
    else HIP_TRY(launch_deconv_direct_f32(a, (hipStream_t)stream));
    return SABER_HIP_OK;
}
