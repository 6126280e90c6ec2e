// anakin_amd/csrc/api_ir.hip - inverted-residual blocks: a 1x1 expand, a depthwise 3x3 and a 1x1 linear project INT8 conv (+ the fused eltwise
// sum with the block's input) in one launch (conv_ir.hip): eligibility, the owned weight / constant tables, create / run / set_tile, the
// executor's static choice.
#include "api_internal.h"

static bool is_8bit(int dt) { return dt == SABER_HIP_S8 || dt == SABER_HIP_U8; }

// a plain 1x1 / stride-1 INT8 conv over 8-bit NHWC tensors: no fused pooling, not a pair, nothing staged in a workspace
static bool plain_1x1(const saber_hip_conv* c) {
    const saber_hip_conv_desc& d = c->d;
    return c->is_i8 && c->epi == EPI_I8_CONV && d.kh == 1 && d.kw == 1 && d.stride_h == 1 && d.stride_w == 1 && d.pad_h == 0 && d.pad_w == 0 &&
           d.dil_h == 1 && d.dil_w == 1 && d.group == 1 && !c->pair_k2 && !c->pool_fused && !c->pool2 && !c->gpool && !c->pre_quant && !c->pre_pad &&
           c->c_eff == d.c && d.act_negative_slope == 0.f && d.in_layout == SABER_HIP_NHWC && d.out_layout == SABER_HIP_NHWC &&
           is_8bit(c->x_dtype) && is_8bit(d.out_dtype);
}

// the three ops are a block conv_ir.hip can run; *why: what is missing. A property of the descriptors alone (weights are create's business)
bool conv_ir_ok(const saber_hip_conv* ex, const saber_hip_conv* dw, const saber_hip_conv* pr, std::string* why) {
    auto no = [&](const char* m) {
        if (why) *why = m;
        return false;
    };
    const saber_hip_conv_desc &de = ex->d, &dd = dw->d, &dp = pr->d;
    if (!ex->is_i8 || !dw->is_i8 || !pr->is_i8) return no("inverted residual: the three ops must be INT8 convs");
    if (!plain_1x1(ex) || de.res_mode != SABER_HIP_RES_NONE || de.act != SABER_HIP_ACT_RELU || de.out_dtype != SABER_HIP_U8)
        return no("inverted residual: the expand op must be a plain 1x1 / stride-1 INT8 conv with relu and u8 NHWC output (no residual, no fused pooling)");
    if (de.c % 8 || de.c < 8 || de.c > 192) return no("inverted residual: Cin % 8 == 0, 8 <= Cin <= 192");
    if (!dw_ok(dw) || dd.in_layout != SABER_HIP_NHWC || dd.out_layout != SABER_HIP_NHWC || dd.act_negative_slope != 0.f || dw->gpool || dw->pair_k2 ||
        dw->pool_fused || dw->pool2 || dd.kh != 3 || dd.kw != 3 || dd.dil_h != 1 || dd.dil_w != 1 || dd.pad_h != 1 || dd.pad_w != 1 ||
        dd.stride_h != dd.stride_w || (dd.stride_h != 1 && dd.stride_h != 2) || dd.act != SABER_HIP_ACT_RELU || dw->x_dtype != DT_U8 ||
        dd.out_dtype != SABER_HIP_U8)
        return no("inverted residual: the second op must be a depthwise 3x3 INT8 conv with dilation 1, pad 1, stride 1 | 2, relu, u8 NHWC in and out");
    if (dd.c % 16 || dd.c > 1024) return no("inverted residual: Ce % 16 == 0, Ce <= 1024");
    if (dd.c != de.k || dd.n != de.n || dd.h != ex->oh || dd.w != ex->ow)
        return no("inverted residual: the depthwise conv must read the expand conv's output (same n / h / w, c == k)");
    if (!plain_1x1(pr) || pr->x_dtype != DT_U8 || pr->algo != ALGO_IGEMM_I8)
        return no("inverted residual: the project op must be a plain 1x1 / stride-1 INT8 conv over the depthwise conv's u8 output (no fused pooling, not a pair)");
    if (dp.c != dd.k || dp.n != dd.n || dp.h != dw->oh || dp.w != dw->ow)
        return no("inverted residual: the project conv must read the depthwise conv's output (same n / h / w, c == k)");
    if (dp.k % 8 || dp.k < 8 || dp.k > 320) return no("inverted residual: Cout % 8 == 0, Cout <= 320");
    if (dp.res_mode == SABER_HIP_RES_NONE) {
        if (!((dp.out_dtype == SABER_HIP_S8 && dp.act == SABER_HIP_ACT_NONE) || (dp.out_dtype == SABER_HIP_U8 && dp.act == SABER_HIP_ACT_RELU)))
            return no("inverted residual: a project op without residual is s8 without relu or u8 with relu");
    } else if (dp.res_mode == SABER_HIP_RES_ELTWISE) {
        if (dp.out_dtype != SABER_HIP_S8 || dp.res_stride > 1)
            return no("inverted residual: the fused eltwise writes s8 and reads its residual unstrided (res_stride <= 1)");
        if (ex->x_dtype != DT_S8 || de.c != dp.k || dd.stride_h != 1)
            return no("inverted residual: the fused eltwise's residual is the block's input: s8, Cin == Cout, stride 1");
    } else {
        return no("inverted residual: the project op's residual mode must be NONE or ELTWISE");
    }
    bool any = false;
    for (int code = 1; code <= IR_MAX_CODE; ++code) any |= conv_ir_geom(code, de.c, dd.c, dp.k, dw->oh, dw->ow, dd.stride_h, nullptr);
    if (!any) return no("inverted residual: no launch form fits this block");
    return true;
}

bool ir_form_valid(const saber_hip_ir* ir, int code) {
    return conv_ir_geom(code, ir->expand->d.c, ir->dw->d.c, ir->project->d.k, ir->dw->oh, ir->dw->ow, ir->dw->d.stride_h, nullptr);
}
void for_each_ir_form(const saber_hip_ir* ir, const std::function<void(int code)>& fn) {
    for (int code = 1; code <= IR_MAX_CODE; ++code)      // (the table in conv_ir.hip lists its codes in ascending order)
        if (ir_form_valid(ir, code)) fn(code);
}
static void ir_select(saber_hip_ir* ir, int code) {
    ir->form = code;
    ir->name = std::string("ir_expand_dw_project_i8_") + conv_ir_form_name(code);
}

// The executor's static choice for a site: a form code, or 0 = the three launches. As sep_static_form (api_sep.hip): a form is named only for a
// shape that was MEASURED (profiles/ir/README.md, written by scripts/bench_ir.py blocks: cold-L2 medians of 15, candidates alternating in one
// process, the tuned separate launches timed twice) where it beat both timings of the separate launches by more than their spread - and, of
// those rows, only where the margin is at least 10 %: the run-to-run spread of launch-bound kernels (0.00 - 0.36 us here, interquartile
// ranges up to 0.7 us) is well inside a tenth of a 15 - 55 us block. Every row cites its figures (form us against separate us, twice).
// Every other shape - other batch sizes, other resolutions, every block at 28 x 28 and below, where the three launches won - answers 0
// and leaves the forms to saber_hip_net_autotune.
static const struct { int cin, ce, cout, h, stride, n, form; } ir_measured_wins[] = {
    {24, 144, 24, 56, 1, 1, 2},      // conv3_2: 16.96 against 19.00 / 18.84 (1.11x)
    {24, 144, 24, 56, 1, 8, 1},      // conv3_2: 21.36 against 54.52 / 54.16 (2.54x)
    {24, 144, 32, 56, 2, 8, 2},      // conv4_1: 18.92 against 49.60 / 49.64 (2.62x)      (batch 1: 19.36 against 18.08 / 18.04 - the three launches won)
    // (conv3_1 at batch 8 - 16, 96, 24, 112, stride 2 - won by 1.07x with form 1: under the margin, left to the autotuner)
};
int ir_static_form(const saber_hip_ir* ir) {
    const saber_hip_conv_desc& d = ir->dw->d;
    for (const auto& r : ir_measured_wins)
        if (ir->expand->d.c == r.cin && d.c == r.ce && ir->project->d.k == r.cout && d.h == r.h && d.w == r.h && d.stride_h == r.stride &&
            d.n == r.n && ir_form_valid(ir, r.form))
            return r.form;
    return 0;
}

// {scale[4], bias'[4], comp[4]} per 4 channels, padded to a multiple of 64 channels; comp = 128 * sum(w[k]) for a u8 input (computed here: a
// conv on the direct path - Cin % 16 == 8 - carries no compensation of its own)
static std::vector<uint8_t> ir_prm(const saber_hip_conv* c, int k, int cin) {
    std::vector<uint8_t> prm((size_t)round_up(k, 64) / 4 * 48, 0);
    for (int o = 0; o < k; ++o) {
        float* f = (float*)(prm.data() + (size_t)(o / 4) * 48);
        int* ip = (int*)(prm.data() + (size_t)(o / 4) * 48 + 32);
        f[o & 3] = c->scale_host[o];
        f[4 + (o & 3)] = (c->has_bias && (int)c->bias_p_host.size() > o) ? c->bias_p_host[o] : 0.f;
        int s = 0;
        for (int i = 0; i < cin; ++i) s += (int)c->wq_oihw[(size_t)o * cin + i];
        ip[o & 3] = c->x_dtype == DT_U8 ? 128 * s : 0;
    }
    return prm;
}

int saber_hip_conv2d_ir_create(saber_hip_conv_t* ex, saber_hip_conv_t* dw, saber_hip_conv_t* pr, saber_hip_ir_t** out) {
    if (!ex || !dw || !pr || !out) return fail(SABER_HIP_INVALID_VALUE, "inverted residual: null argument");
    std::string why;
    if (!conv_ir_ok(ex, dw, pr, &why)) return fail(SABER_HIP_UNIMPL, why);
    if (!ex->weights_set || !dw->weights_set || !pr->weights_set) return fail(SABER_HIP_UNIMPL, "inverted residual: the three ops need their weights set");
    const int Cin = ex->d.c, Ce = dw->d.c, Cout = pr->d.k;
    if ((int)ex->wq_oihw.size() != Ce * Cin || (int)dw->wq_oihw.size() != Ce * 9 || (int)pr->wq_oihw.size() != Cout * Ce ||
        (int)ex->scale_host.size() < Ce || (int)dw->scale_host.size() < Ce || (int)pr->scale_host.size() < Cout)
        return fail(SABER_HIP_UNIMPL, "inverted residual: the ops' quantised weights are not those of a 1x1 / a depthwise 3x3 / a 1x1 conv");
    std::vector<uint8_t> we, wp, wdw((size_t)9 * Ce);
    ir_pack(ex->wq_oihw.data(), Ce, Cin, we);
    ir_pack(pr->wq_oihw.data(), Cout, Ce, wp);
    for (int c = 0; c < Ce; ++c)
        for (int t = 0; t < 9; ++t) wdw[(size_t)t * Ce + c] = (uint8_t)dw->wq_oihw[(size_t)c * 9 + t];
    // the depthwise conv's constants (zeros for "no bias": (float)acc + 0.f == (float)acc)
    std::vector<float> dbias(Ce, 0.f), dscale(dw->scale_host.begin(), dw->scale_host.begin() + Ce);
    if (dw->has_bias && (int)dw->bias_p_host.size() >= Ce) std::copy(dw->bias_p_host.begin(), dw->bias_p_host.begin() + Ce, dbias.begin());
    auto* ir = new saber_hip_ir();
    ir->expand = ex; ir->dw = dw; ir->project = pr;
    ir->scale_conv = pr->out_scale;
    hipError_t e = ir->d_we.upload(we);
    if (e == hipSuccess) e = ir->d_wp.upload(wp);
    if (e == hipSuccess) e = ir->d_wdw.upload(wdw);
    if (e == hipSuccess) e = ir->d_eprm.upload(ir_prm(ex, Ce, Cin));
    if (e == hipSuccess) e = ir->d_pprm.upload(ir_prm(pr, Cout, Ce));
    if (e == hipSuccess) e = ir->d_dw_bias.upload(dbias);
    if (e == hipSuccess) e = ir->d_dw_scale.upload(dscale);
    if (e == hipSuccess) e = conv_ir_prepare();
    if (e != hipSuccess) {
        delete ir;
        return hip_fail(e, "inverted residual: device copies");
    }
    int first = 0;
    for_each_ir_form(ir, [&](int code) { if (!first) first = code; });
    ir_select(ir, first);
    *out = ir;
    return SABER_HIP_OK;
}
void saber_hip_conv2d_ir_destroy(saber_hip_ir_t* ir) { delete ir; }
int saber_hip_conv2d_ir_set_tile(saber_hip_ir_t* ir, int code) {
    if (!ir) return fail(SABER_HIP_INVALID_VALUE, "inverted residual: null argument");
    if (!ir_form_valid(ir, code)) return fail(SABER_HIP_INVALID_VALUE, "inverted residual: no launch form with that code for this block");
    ir_select(ir, code);
    return SABER_HIP_OK;
}
int saber_hip_conv2d_ir_get_tile(const saber_hip_ir_t* ir) { return ir ? ir->form : 0; }
const char* saber_hip_conv2d_ir_algo(const saber_hip_ir_t* ir) { return ir ? ir->name.c_str() : ""; }
int saber_hip_conv2d_ir_run(saber_hip_ir_t* ir, const void* x, void* y_expand, void* y_dw, void* y, saber_hip_stream_t stream) {
    if (g_capture) return capture_unsupported("saber_hip_conv2d_ir_run (an executor-level object: saber_hip_net_optimize forms it itself)");
    if (!ir || !x || !y) return fail(SABER_HIP_INVALID_VALUE, "inverted residual: null argument");
    const saber_hip_conv *ex = ir->expand, *dw = ir->dw, *pr = ir->project;
    IrKArgs a;
    std::memset(&a, 0, sizeof a);
    a.x = x; a.we = ir->d_we.p; a.eprm = ir->d_eprm.p; a.wdw = ir->d_wdw.p; a.dw_bias = ir->d_dw_bias.p; a.dw_scale = ir->d_dw_scale.p;
    a.wp = ir->d_wp.p; a.pprm = ir->d_pprm.p; a.y_e = y_expand; a.y_d = y_dw; a.y = y;
    a.N = ex->d.n; a.H = ex->d.h; a.W = ex->d.w; a.Cin = ex->d.c; a.Ce = dw->d.c; a.OH = dw->oh; a.OW = dw->ow; a.Cout = pr->d.k;
    a.stride = dw->d.stride_h;
    a.out_u8 = pr->d.out_dtype == SABER_HIP_U8; a.p_relu = pr->d.act == SABER_HIP_ACT_RELU;
    a.elt = pr->d.res_mode == SABER_HIP_RES_ELTWISE; a.res_relu = pr->d.res_act == SABER_HIP_ACT_RELU;
    a.coeff_conv = pr->d.coeff_conv; a.scale_conv = ir->scale_conv; a.coeff_res = pr->d.coeff_res; a.scale_res = pr->d.scale_res;
    HIP_TRY(launch_conv_ir(ir->form, ex->x_dtype == DT_U8, a, (hipStream_t)stream));
    return SABER_HIP_OK;
}
