// anakin_amd/csrc/api_fire.hip - Fire modules: a 1x1 squeeze conv, the 1x1 and the padded 3x3 expand convs that both read it and the channel
// concat of the two, INT8, in one launch (conv_fire.hip): eligibility, the owned weight / constant tables, create / run / set_tile, the
// executor's static choice.
#include "api_internal.h"

// a plain stride-1 INT8 conv with relu over 8-bit NHWC tensors writing u8: no residual, no fused pooling, not a pair, nothing staged
static bool plain_relu_u8(const saber_hip_conv* c, int k, int pad) {
    const saber_hip_conv_desc& d = c->d;
    return c->is_i8 && c->epi == EPI_I8_CONV && d.kh == k && d.kw == k && d.stride_h == 1 && d.stride_w == 1 && d.pad_h == pad && d.pad_w == pad &&
           d.dil_h == 1 && d.dil_w == 1 && d.group == 1 && !c->pair_k2 && !c->pool_fused && !c->pool2 && !c->gpool && !c->pre_quant && !c->pre_pad &&
           c->c_eff == d.c && d.act_negative_slope == 0.f && d.in_layout == SABER_HIP_NHWC && d.out_layout == SABER_HIP_NHWC &&
           (c->x_dtype == DT_S8 || c->x_dtype == DT_U8) && d.out_dtype == SABER_HIP_U8 && d.act == SABER_HIP_ACT_RELU && d.res_mode == SABER_HIP_RES_NONE;
}

// the three ops are a module conv_fire.hip can run; *why: what is missing. A property of the descriptors alone
bool conv_fire_ok(const saber_hip_conv* sq, const saber_hip_conv* e1, const saber_hip_conv* e3, std::string* why) {
    auto no = [&](const char* m) {
        if (why) *why = m;
        return false;
    };
    if (!plain_relu_u8(sq, 1, 0)) return no("fire: the squeeze op must be a plain 1x1 / stride-1 INT8 conv with relu, s8 | u8 NHWC in, u8 NHWC out");
    if (!plain_relu_u8(e1, 1, 0) || e1->x_dtype != DT_U8) return no("fire: the first expand op must be a plain 1x1 / stride-1 INT8 conv with relu, u8 NHWC in and out");
    if (!plain_relu_u8(e3, 3, 1) || e3->x_dtype != DT_U8) return no("fire: the second expand op must be a plain 3x3 / stride-1 / pad-1 INT8 conv with relu, u8 NHWC in and out");
    const saber_hip_conv_desc &ds = sq->d, &d1 = e1->d, &d3 = e3->d;
    if (d1.c != ds.k || d3.c != ds.k || d1.n != ds.n || d3.n != ds.n || d1.h != sq->oh || d3.h != sq->oh || d1.w != sq->ow || d3.w != sq->ow)
        return no("fire: both expand convs must read the squeeze conv's output (same n / h / w, c == k)");
    bool any = false;
    for (int code = 1; code <= FIRE_MAX_CODE; ++code) any |= conv_fire_geom(code, ds.c, ds.k, d1.k, d3.k, ds.h, ds.w, nullptr);
    if (!any) return no("fire: S in {16, 32, 48, 64}; C, E1, E3 multiples of 16 up to 512; no launch form fits otherwise");
    return true;
}

bool fire_form_valid(const saber_hip_fire* fr, int code) {
    return conv_fire_geom(code, fr->squeeze->d.c, fr->squeeze->d.k, fr->e1->d.k, fr->e3->d.k, fr->squeeze->d.h, fr->squeeze->d.w, nullptr);
}
void for_each_fire_form(const saber_hip_fire* fr, const std::function<void(int code)>& fn) {
    for (int code = 1; code <= FIRE_MAX_CODE; ++code)
        if (fire_form_valid(fr, code)) fn(code);
}
static void fire_select(saber_hip_fire* fr, int code) {
    fr->form = code;
    fr->name = std::string("fire_squeeze_expand_i8_") + conv_fire_form_name(code);
}

// The executor's static choice for a site: a form code, or 0 = the four launches. As ir_static_form: a form is named only for a shape that was
// MEASURED (profiles/fire/README.md, written by scripts/bench_fire.py modules: cold-L2 medians of 15, candidates alternating in one process,
// the tuned four launches timed twice) where it beat both timings of the four launches by more than their spread and by at least 10 % -
// here in BOTH comparisons the table holds: eagerly enqueued, and each side replayed as a hipGraph of its own (fire6 at batch 8 won 1.13x
// eagerly but 1.09x replayed: left to the autotuner). Every row cites its eager figures (form us against four us, twice). Every other shape -
// other batch sizes, other resolutions, every module at 13 x 13, where the four launches won or the margin is small - answers 0 and leaves
// the forms to saber_hip_net_autotune.
static const struct { int c, s, e1, e3, h, n, form; } fire_measured_wins[] = {
    {64, 16, 64, 64, 55, 1, 2},        // fire2:  9.2 against 28.9 / 24.6
    {64, 16, 64, 64, 55, 8, 1},        // fire2: 12.7 against 19.3 / 22.4
    {128, 16, 64, 64, 55, 1, 2},       // fire3: 10.3 against 16.0 / 16.0 (1.55x)
    {128, 16, 64, 64, 55, 8, 1},       // fire3: 14.0 against 18.4 / 18.3 (1.31x)
    {128, 32, 128, 128, 27, 1, 2},     // fire4: 11.7 against 16.1 / 16.1 (1.38x)
    {128, 32, 128, 128, 27, 8, 2},     // fire4: 11.6 against 17.9 / 17.9 (1.54x)
    {256, 32, 128, 128, 27, 1, 2},     // fire5: 13.6 against 16.4 / 16.4 (1.20x)
    {256, 32, 128, 128, 27, 8, 2},     // fire5: 13.4 against 17.9 / 17.8 (1.33x)
};
int fire_static_form(const saber_hip_fire* fr) {
    const saber_hip_conv_desc& d = fr->squeeze->d;
    for (const auto& r : fire_measured_wins)
        if (d.c == r.c && d.k == r.s && fr->e1->d.k == r.e1 && fr->e3->d.k == r.e3 && d.h == r.h && d.w == r.h && d.n == r.n && fire_form_valid(fr, r.form))
            return r.form;
    return 0;
}

// {scale[4], bias'[4], comp[4]} per 4 channels, padded to a multiple of 64 channels; comp = 128 * sum(w[k]) over the whole reduction for a u8 input
static std::vector<uint8_t> fire_prm(const saber_hip_conv* c, int k, int red) {
    std::vector<uint8_t> prm((size_t)round_up(k, 64) / 4 * 48, 0);
    for (int o = 0; o < k; ++o) {
        float* f = (float*)(prm.data() + (size_t)(o / 4) * 48);
        int* ip = (int*)(prm.data() + (size_t)(o / 4) * 48 + 32);
        f[o & 3] = c->scale_host[o];
        f[4 + (o & 3)] = (c->has_bias && (int)c->bias_p_host.size() > o) ? c->bias_p_host[o] : 0.f;
        int s = 0;
        for (int i = 0; i < red; ++i) s += (int)c->wq_oihw[(size_t)o * red + i];
        ip[o & 3] = c->x_dtype == DT_U8 ? 128 * s : 0;
    }
    return prm;
}

int saber_hip_conv2d_fire_create(saber_hip_conv_t* sq, saber_hip_conv_t* e1, saber_hip_conv_t* e3, saber_hip_fire_t** out) {
    if (!sq || !e1 || !e3 || !out) return fail(SABER_HIP_INVALID_VALUE, "fire: null argument");
    std::string why;
    if (!conv_fire_ok(sq, e1, e3, &why)) return fail(SABER_HIP_UNIMPL, why);
    if (!sq->weights_set || !e1->weights_set || !e3->weights_set) return fail(SABER_HIP_UNIMPL, "fire: the three ops need their weights set");
    const int C = sq->d.c, S = sq->d.k, E1 = e1->d.k, E3 = e3->d.k;
    if ((int)sq->wq_oihw.size() != S * C || (int)e1->wq_oihw.size() != E1 * S || (int)e3->wq_oihw.size() != E3 * S * 9 || (int)sq->scale_host.size() < S ||
        (int)e1->scale_host.size() < E1 || (int)e3->scale_host.size() < E3)
        return fail(SABER_HIP_UNIMPL, "fire: the ops' quantised weights are not those of a 1x1 / a 1x1 / a 3x3 conv");
    std::vector<uint8_t> ws, w1, w3, tap;
    ir_pack(sq->wq_oihw.data(), S, C, ws);
    ir_pack(e1->wq_oihw.data(), E1, S, w1);
    std::vector<int8_t> wt((size_t)E3 * S);
    for (int t = 0; t < 9; ++t) {      // [tap][group of 64][4][64 lanes][16]: each tap a 1x1 conv of its own
        for (int o = 0; o < E3; ++o)
            for (int c = 0; c < S; ++c) wt[(size_t)o * S + c] = e3->wq_oihw[((size_t)o * S + c) * 9 + t];
        ir_pack(wt.data(), E3, S, tap);
        w3.insert(w3.end(), tap.begin(), tap.end());
    }
    auto* fr = new saber_hip_fire();
    fr->squeeze = sq; fr->e1 = e1; fr->e3 = e3;
    hipError_t e = fr->d_ws.upload(ws);
    if (e == hipSuccess) e = fr->d_w1.upload(w1);
    if (e == hipSuccess) e = fr->d_w3.upload(w3);
    if (e == hipSuccess) e = fr->d_sprm.upload(fire_prm(sq, S, C));
    if (e == hipSuccess) e = fr->d_prm1.upload(fire_prm(e1, E1, S));
    if (e == hipSuccess) e = fr->d_prm3.upload(fire_prm(e3, E3, S * 9));
    if (e == hipSuccess) e = conv_fire_prepare();
    if (e != hipSuccess) {
        delete fr;
        return hip_fail(e, "fire: device copies");
    }
    int first = 0;
    for_each_fire_form(fr, [&](int code) { if (!first) first = code; });
    fire_select(fr, first);
    *out = fr;
    return SABER_HIP_OK;
}
void saber_hip_conv2d_fire_destroy(saber_hip_fire_t* fr) { delete fr; }
int saber_hip_conv2d_fire_set_tile(saber_hip_fire_t* fr, int code) {
    if (!fr) return fail(SABER_HIP_INVALID_VALUE, "fire: null argument");
    if (!fire_form_valid(fr, code)) return fail(SABER_HIP_INVALID_VALUE, "fire: no launch form with that code for this module");
    fire_select(fr, code);
    return SABER_HIP_OK;
}
int saber_hip_conv2d_fire_get_tile(const saber_hip_fire_t* fr) { return fr ? fr->form : 0; }
const char* saber_hip_conv2d_fire_algo(const saber_hip_fire_t* fr) { return fr ? fr->name.c_str() : ""; }
int saber_hip_conv2d_fire_run(saber_hip_fire_t* fr, const void* x, void* y_squeeze, void* y, saber_hip_stream_t stream) {
    if (g_capture) return capture_unsupported("saber_hip_conv2d_fire_run (an executor-level object)");
    if (!fr || !x || !y) return fail(SABER_HIP_INVALID_VALUE, "fire: null argument");
    const saber_hip_conv* sq = fr->squeeze;
    FireKArgs a;
    std::memset(&a, 0, sizeof a);
    a.x = x; a.ws = fr->d_ws.p; a.sprm = fr->d_sprm.p; a.w1 = fr->d_w1.p; a.prm1 = fr->d_prm1.p; a.w3 = fr->d_w3.p; a.prm3 = fr->d_prm3.p;
    a.y_s = y_squeeze; a.y = y;
    a.N = sq->d.n; a.H = sq->d.h; a.W = sq->d.w; a.C = sq->d.c; a.S = sq->d.k; a.E1 = fr->e1->d.k; a.E3 = fr->e3->d.k;
    HIP_TRY(launch_conv_fire(fr->form, sq->x_dtype == DT_U8, a, (hipStream_t)stream));
    return SABER_HIP_OK;
}
