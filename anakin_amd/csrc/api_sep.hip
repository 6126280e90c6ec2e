// anakin_amd/csrc/api_sep.hip - separable pairs: a depthwise 3x3 INT8 conv and the pointwise 1x1 INT8 conv that reads it in one launch
// (conv_sep.hip): eligibility, the owned weight / constant tables, create / run / set_tile, the executor's static choice.
#include "api_internal.h"

static bool is_8bit(int dt) { return dt == SABER_HIP_S8 || dt == SABER_HIP_U8; }

// the pair is one conv_sep.hip can run; *why: what is missing
bool conv_sep_ok(const saber_hip_conv* dw, const saber_hip_conv* pw, std::string* why) {
    auto no = [&](const char* m) {
        if (why) *why = m;
        return false;
    };
    const saber_hip_conv_desc &dd = dw->d, &dp = pw->d;
    if (!dw->is_i8 || !pw->is_i8) return no("separable pair: both ops must be INT8 convs");
    if (!dw_ok(dw) || dd.in_layout != SABER_HIP_NHWC || dd.out_layout != SABER_HIP_NHWC || !is_8bit(dw->x_dtype) || !is_8bit(dd.out_dtype) ||
        dd.act_negative_slope != 0.f || dw->gpool || dw->pair_k2 || dw->pool_fused || dw->pool2)
        return no("separable pair: the head must be a depthwise 3x3 INT8 conv (stride 1 | 2, pad 0 | 1, 8-bit NHWC in and out, no residual)");
    if (dd.c % 32 || dd.c < 32 || dd.c > 1024) return no("separable pair: C % 32 == 0, 32 <= C <= 1024");
    if (pw->algo != ALGO_IGEMM_I8 || pw->epi != EPI_I8_CONV || dp.kh != 1 || dp.kw != 1 || dp.stride_h != 1 || dp.stride_w != 1 || dp.pad_h != 0 ||
        dp.pad_w != 0 || dp.dil_h != 1 || dp.dil_w != 1 || dp.group != 1 || dp.res_mode != SABER_HIP_RES_NONE || pw->pair_k2 || pw->pool_fused ||
        pw->pool2 || pw->gpool || pw->pre_quant || pw->pre_pad || pw->c_eff != dp.c || dp.act_negative_slope != 0.f ||
        dp.in_layout != SABER_HIP_NHWC || dp.out_layout != SABER_HIP_NHWC || !is_8bit(dp.out_dtype))
        return no("separable pair: the second op must be a plain 1x1 / stride-1 INT8 conv (no residual, no fused pooling, not a pair, 8-bit NHWC output)");
    if (dp.c != dd.k || dp.in_dtype != dd.out_dtype || pw->x_dtype != dd.out_dtype || dp.n != dd.n || dp.h != dw->oh || dp.w != dw->ow)
        return no("separable pair: the 1x1 conv must read the depthwise conv's output (same n / h / w, c == k, same 8-bit type)");
    if (dp.k % 32 || dp.k < 32) return no("separable pair: K % 32 == 0");
    return true;
}

bool sep_form_valid(const saber_hip_sep* sp, int code) { return conv_sep_form_ok(code, sp->dw->d.c, sp->pw->d.k); }
void for_each_sep_form(const saber_hip_sep* sp, const std::function<void(int code)>& fn) {
    for (int code = 1; code <= SEP_MAX_CODE; ++code)      // (the table in conv_sep.hip lists its codes in ascending order)
        if (sep_form_valid(sp, code)) fn(code);
}
static std::string sep_form_name(int code) {
    int rows = 0, kper = 0, waves = 0;
    if (!conv_sep_form(code, &rows, &kper, &waves)) return "";
    return std::to_string(rows) + "x16" + (kper ? "_k" + std::to_string(kper) : "") + (waves != 4 ? "_w" + std::to_string(waves) : "");
}
static void sep_select(saber_hip_sep* sp, int code) {
    sp->form = code;
    sp->name = "sep_dw3x3_pw_i8_" + sep_form_name(code);
}

// The executor's static choice for a site: a form code, or 0 = the two launches. A form is named only for a shape that was MEASURED, where it
// beat both timings of the two tuned launches of the same run by more than that run's spread (profiles/sep/README.md, written by
// scripts/bench_sep.py shapes: cold-L2 medians, candidates alternating in one process) - and, of those rows, only where the margin is at
// least 10 %: the spread of one run was 0.00 - 0.24 us, a tenth of a 10 us pair is beyond any of them. Every row cites its figures
// (form us against separate us, twice). Every other shape - other batch sizes, other resolutions, the 14 x 14 and 7 x 7 layers, where the
// two launches won - answers 0 and leaves the forms to saber_hip_net_autotune.
static const struct { int c, h, stride, k, n, form; } sep_measured_wins[] = {
    {32, 112, 1, 64, 1, 2},       //  8.36 against 10.40 / 10.40 (1.24x)   (batch 8: 17.64 against 15.16 / 15.28 - the two launches won)
    {64, 112, 2, 128, 1, 5},      //  7.32 against 10.40 / 10.44 (1.42x)
    {64, 112, 2, 128, 8, 1},      // 10.76 against 12.92 / 12.92 (1.20x)
    {128, 56, 1, 128, 1, 2},      //  8.92 against 10.24 / 10.28 (1.15x)
    {128, 56, 1, 128, 8, 1},      // 13.08 against 14.76 / 14.76 (1.13x)
    {128, 56, 2, 256, 1, 2},      //  9.12 against 10.12 / 10.12 (1.11x)
    {128, 56, 2, 256, 8, 2},      //  9.40 against 11.24 / 11.32 (1.20x)
    {256, 28, 1, 256, 8, 2},      // 11.96 against 13.28 / 13.52 (1.11x)   (batch 1: 11.44 against 10.32 / 10.36 - the two launches won)
    {256, 28, 2, 512, 8, 4},      //  9.64 against 11.00 / 11.04 (1.14x)   (batch 1: 9.40 against 9.92 / 9.96, 1.06x - won, but under the 10 % margin)
};
int sep_static_form(const saber_hip_sep* sp) {
    const saber_hip_conv_desc &d = sp->dw->d;
    for (const auto& r : sep_measured_wins)
        if (d.c == r.c && d.h == r.h && d.w == r.h && d.stride_h == r.stride && d.pad_h == 1 && sp->pw->d.k == r.k && d.n == r.n && sep_form_valid(sp, r.form))
            return r.form;
    return 0;
}

int saber_hip_conv2d_sep_create(saber_hip_conv_t* dw, saber_hip_conv_t* pw, saber_hip_sep_t** out) {
    if (!dw || !pw || !out) return fail(SABER_HIP_INVALID_VALUE, "separable pair: null argument");
    if (!dw->weights_set || !pw->weights_set) return fail(SABER_HIP_UNIMPL, "separable pair: both ops need their weights set");
    std::string why;
    if (!conv_sep_ok(dw, pw, &why)) return fail(SABER_HIP_UNIMPL, why);
    const int C = dw->d.c, K = pw->d.k, KP = round_up(K, 64);
    if ((int)dw->wq_oihw.size() != C * 9 || (int)pw->wq_oihw.size() != K * C || (int)dw->scale_host.size() < C || (int)pw->scale_host.size() < K)
        return fail(SABER_HIP_UNIMPL, "separable pair: the ops' quantised weights are not those of a depthwise 3x3 / a 1x1 conv");
    // the depthwise conv's [tap][C] weights and constants (zeros for "no bias": (float)acc + 0.f == (float)acc)
    std::vector<uint8_t> wdw((size_t)9 * C), wpw, prm((size_t)KP / 4 * 48, 0);
    for (int c = 0; c < C; ++c)
        for (int t = 0; t < 9; ++t) wdw[(size_t)t * C + c] = (uint8_t)dw->wq_oihw[(size_t)c * 9 + t];
    std::vector<float> dbias(C, 0.f), dscale(dw->scale_host.begin(), dw->scale_host.begin() + C);
    if (dw->has_bias && (int)dw->bias_p_host.size() >= C) std::copy(dw->bias_p_host.begin(), dw->bias_p_host.begin() + C, dbias.begin());
    // the pointwise conv's fragment stream and {scale[4], bias'[4], comp[4]} per 4 output channels (comp: 128 * sum(w) for a u8 intermediate)
    sep_pw_pack(pw->wq_oihw.data(), K, C, wpw);
    for (int k = 0; k < K; ++k) {
        float* f = (float*)(prm.data() + (size_t)(k / 4) * 48);
        int* ip = (int*)(prm.data() + (size_t)(k / 4) * 48 + 32);
        f[k & 3] = pw->scale_host[k];
        f[4 + (k & 3)] = (pw->has_bias && (int)pw->bias_p_host.size() > k) ? pw->bias_p_host[k] : 0.f;
        ip[k & 3] = (int)pw->comp_host.size() > k ? pw->comp_host[k] : 0;
    }
    if (pw->x_dtype == DT_U8 && (int)pw->comp_host.size() < K) return fail(SABER_HIP_UNIMPL, "separable pair: the 1x1 conv has no u8 compensation");
    auto* sp = new saber_hip_sep();
    sp->dw = dw; sp->pw = pw;
    hipError_t e = sp->d_wdw.upload(wdw);
    if (e == hipSuccess) e = sp->d_wpw.upload(wpw);
    if (e == hipSuccess) e = sp->d_prm.upload(prm);
    if (e == hipSuccess) e = sp->d_dw_bias.upload(dbias);
    if (e == hipSuccess) e = sp->d_dw_scale.upload(dscale);
    if (e == hipSuccess) e = conv_sep_prepare();
    if (e != hipSuccess) {
        delete sp;
        return hip_fail(e, "separable pair: device copies");
    }
    int first = 0;
    for_each_sep_form(sp, [&](int code) { if (!first) first = code; });
    sep_select(sp, first);
    *out = sp;
    return SABER_HIP_OK;
}
void saber_hip_conv2d_sep_destroy(saber_hip_sep_t* sp) { delete sp; }
int saber_hip_conv2d_sep_set_tile(saber_hip_sep_t* sp, int code) {
    if (!sp) return fail(SABER_HIP_INVALID_VALUE, "separable pair: null argument");
    if (!sep_form_valid(sp, code)) return fail(SABER_HIP_INVALID_VALUE, "separable pair: no launch form with that code for this pair");
    sep_select(sp, code);
    return SABER_HIP_OK;
}
int saber_hip_conv2d_sep_get_tile(const saber_hip_sep_t* sp) { return sp ? sp->form : 0; }
const char* saber_hip_conv2d_sep_algo(const saber_hip_sep_t* sp) { return sp ? sp->name.c_str() : ""; }
int saber_hip_conv2d_sep_run(saber_hip_sep_t* sp, const void* x, void* y_dw, void* y_pw, saber_hip_stream_t stream) {
    if (g_capture) return capture_unsupported("saber_hip_conv2d_sep_run (an executor-level object: saber_hip_net_optimize forms it itself)");
    if (!sp || !x || !y_pw) return fail(SABER_HIP_INVALID_VALUE, "separable pair: null argument");
    const saber_hip_conv *dw = sp->dw, *pw = sp->pw;
    SepKArgs a;
    std::memset(&a, 0, sizeof a);
    a.x = x; a.wdw = sp->d_wdw.p; a.dw_bias = sp->d_dw_bias.p; a.dw_scale = sp->d_dw_scale.p;
    a.wpw = sp->d_wpw.p; a.prm = sp->d_prm.p; a.y_dw = y_dw; a.y_pw = y_pw;
    a.N = dw->d.n; a.H = dw->d.h; a.W = dw->d.w; a.C = dw->d.c; a.OH = dw->oh; a.OW = dw->ow; a.K = pw->d.k;
    a.stride = dw->d.stride_h; a.pad = dw->d.pad_h;
    a.dw_relu = dw->d.act == SABER_HIP_ACT_RELU; a.mid_u8 = dw->d.out_dtype == SABER_HIP_U8;
    a.pw_relu = pw->d.act == SABER_HIP_ACT_RELU; a.out_u8 = pw->d.out_dtype == SABER_HIP_U8;
    HIP_TRY(launch_conv_sep(sp->form, dw->x_dtype == DT_U8, a, (hipStream_t)stream));
    return SABER_HIP_OK;
}
