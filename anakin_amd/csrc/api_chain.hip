// anakin_amd/csrc/api_chain.hip - conv1x1 chains: two (or conv3x3 + two) INT8 convolutions in one launch (conv1x1_chain.hip).
#include "api_internal.h"

// ------------------------------------------------------------------------------------------------
// chain forms: THE table of what a set_tile code means. A row holds for one C and the kinds of chain in `kinds` (1X1: conv1x1 + eltwise ->
// conv1x1 | 3X3: led by the block's conv3x3 | HEAD: conv3x3, stride 1 | 2, -> conv1x1 + eltwise | PAIR: strided head -> sibling pair). Per C the
// rows are in the autotuner's candidate order; a chain's first row is create's default; its placement-dependent rows come last and fall back
// to the row in front of them.
// ------------------------------------------------------------------------------------------------
enum : unsigned { CK_1X1 = 1, CK_3X3 = 2, CK_HEAD = 4, CK_PAIR = 8, CK_LED = CK_3X3 | CK_HEAD, CK_ANY = 15 };
static unsigned chain_kind(const saber_hip_chain* ch) { return !ch->c3 ? CK_1X1 : (ch->b2 ? CK_PAIR : (ch->b ? CK_3X3 : CK_HEAD)); }
static const struct { int c1; unsigned kinds; ChainForm f; } chain_forms[] = {
    // C, kinds             code rows waves split coop stream  placement
    {64, CK_ANY,            {4, 4, 4, 1, 1, CS_BASE, false}},
    {64, CK_ANY,            {2, 2, 4, 1, 1, CS_BASE, false}},
    {128, CK_1X1 | CK_LED,  {2, 2, 4, 1, 1, CS_BASE, false}},
    {128, CK_1X1 | CK_LED,  {1, 1, 4, 1, 1, CS_BASE, false}},
    {128, CK_1X1 | CK_LED,  {6, 2, 8, 1, 1, CS_W8, false}},
    {128, CK_1X1 | CK_LED,  {5, 1, 8, 1, 1, CS_W8, false}},
    {256, CK_1X1 | CK_LED,  {1, 1, 4, 1, 1, CS_BASE, false}},
    {256, CK_1X1,           {9, 1, 4, 2, 1, CS_SPLIT, false}},
    {256, CK_1X1,           {11, 1, 8, 2, 1, CS_SPLIT8, false}},
    {256, CK_LED,           {3, 1, 8, 1, 1, CS_W8, false}},
    {256, CK_3X3,           {7, 1, 8, 1, 2, CS_COOP2, true}},
    {256, CK_3X3,           {15, 2, 8, 1, 4, CS_COOP4, true}},
    {512, CK_1X1,           {1, 1, 4, 1, 1, CS_BASE, false}},
    {512, CK_1X1,           {9, 1, 4, 2, 1, CS_SPLIT, false}},
};
static void for_each_chain_form(const saber_hip_chain* ch, const std::function<void(const ChainForm&)>& fn) {
    for (const auto& r : chain_forms)
        if (r.c1 == ch->c1 && (r.kinds & chain_kind(ch))) fn(r.f);
}
static ChainForm chain_form_where(const saber_hip_chain* ch, const std::function<bool(const ChainForm& row, const ChainForm& found)>& take) {
    ChainForm f;
    for_each_chain_form(ch, [&](const ChainForm& c) { if (take(c, f)) f = c; });
    return f;
}
ChainForm chain_form(const saber_hip_chain* ch, int code) { return chain_form_where(ch, [&](const ChainForm& c, const ChainForm&) { return c.code == code; }); }
ChainForm chain_form_default(const saber_hip_chain* ch) { return chain_form_where(ch, [](const ChainForm&, const ChainForm& f) { return !f.code; }); }
ChainForm chain_form_plain(const saber_hip_chain* ch) { return chain_form_where(ch, [](const ChainForm& c, const ChainForm&) { return !c.placement; }); }
bool chain_form_valid(const saber_hip_chain* ch, int code) {
    const ChainForm f = chain_form(ch, code);
    return f.code && ch->d_stream[f.stream].p && (f.coop != 4 || ch->stage1);
}
std::string chain_form_name(const saber_hip_chain* ch) {
    const ChainForm& f = ch->form;
    const std::string c = std::to_string(ch->c1), w8 = f.waves == 8 && f.coop == 1 ? "_w8" : "";
    if (!ch->c3) return "chain1x1_c" + c + "_px" + std::to_string(16 * f.rows) + (f.split == 2 ? "_split2" : "") + w8;
    return std::string("conv3x3+") + (ch->b2 ? "conv1x1+pair1x1_c" : (ch->b ? "chain1x1_c" : "conv1x1_c")) + c + "_" + std::to_string(f.rows) + "x16" + w8 +
           (f.coop == 2 ? "_coop2" : "") + (f.coop == 4 ? "_coop4" : "");
}
void for_each_chain_candidate(const saber_hip_chain* ch, bool shared_device, const std::function<void(const ChainForm&)>& fn) {
    for_each_chain_form(ch, [&](const ChainForm& c) { if (!(shared_device && c.placement) && chain_form_valid(ch, c.code)) fn(c); });
}

// ------------------------------------------------------------------------------------------------
// conv1x1 chain: `a` (1x1, fused SaberEltwise epilogue, s8 out) feeding `b` (1x1, s8 / u8 out) in one launch
// ------------------------------------------------------------------------------------------------
static bool chain_1x1(const saber_hip_conv* o, bool sub_res_ok = false) {
    const saber_hip_conv_desc& d = o->d;
    return o->is_i8 && o->weights_set && !o->gpool && o->algo == ALGO_IGEMM_I8 && o->epi == EPI_I8_CONV && d.kh == 1 && d.kw == 1 &&
           d.stride_h == 1 && d.stride_w == 1 && d.pad_h == 0 && d.pad_w == 0 && d.group == 1 && !o->pair_k2 &&
           !o->pool_fused && !o->pool2 && !o->pre_quant && !o->pre_pad && o->c_eff == d.c && d.act_negative_slope == 0.f &&
           d.in_layout == SABER_HIP_NHWC && d.out_layout == SABER_HIP_NHWC && (d.res_stride <= 1 || sub_res_ok);
}
static void pack_chain_params(const saber_hip_conv* o, size_t chunks_pad, std::vector<uint8_t>& out) {
    const int K = o->d.k;
    out.assign(chunks_pad * 16, 0);
    for (int k4 = 0; k4 < K / 4; ++k4) {
        float* f = (float*)(out.data() + (size_t)k4 * 48);
        int* ip = (int*)(out.data() + (size_t)k4 * 48 + 32);
        for (int r = 0; r < 4; ++r) {
            const int k = k4 * 4 + r;
            f[r] = o->scale_host.empty() ? 1.f : o->scale_host[k];
            f[4 + r] = (o->has_bias && !o->bias_p_host.empty()) ? o->bias_p_host[k] : 0.f;
            ip[r] = o->comp_host.empty() ? 0 : o->comp_host[k];
        }
    }
}
// one conv's weights [K][C] -> per wave, groups of 16*mfg channels, steps ordered [group][k-step][accumulator], each step
// = 64 lanes x 16 bytes in MFMA A-operand order (row = lane & 15, k-group = lane >> 4); row rho of accumulator mf is
// channel  base + (rho >> 2) * 4*mfg + mf*4 + (rho & 3)   (conv1x1_chain.hip)
static void pack_chain_weights(const int8_t* w, int K, int C, int mfg, int wave, std::vector<uint8_t>& out, int kbase = 0,
                               int nw = 4, int ks0 = 0) {
    // K: channels of this workgroup's share (rows kbase .. kbase + K - 1 of w), nw waves; ks0: the k-step the stream starts with
    // (cooperative form: the k-steps over this workgroup's OWN half of the input channels come first)
    const int kw = K / nw, groups = kw / (16 * mfg), ksn = C / 64;
    for (int g = 0; g < groups; ++g)
        for (int ksi = 0; ksi < ksn; ++ksi)
            for (int mf = 0; mf < mfg; ++mf) {
                const int ks = (ks0 + ksi) % ksn;
                for (int lane = 0; lane < 64; ++lane) {
                    const int rho = lane & 15, kq = lane >> 4;
                    const int ch = kbase + wave * kw + g * 16 * mfg + (rho >> 2) * 4 * mfg + mf * 4 + (rho & 3);
                    const int8_t* src = w + (size_t)ch * C + ks * 64 + kq * 16;
                    out.insert(out.end(), (const uint8_t*)src, (const uint8_t*)src + 16);
                }
            }
}
// the 3x3 conv's weights [K][C][3][3] -> per wave, steps ordered [tap][k-step][accumulator] (conv1x1_chain.hip phase 0)
static void pack_chain_weights3(const int8_t* w, int C, int wave, std::vector<uint8_t>& out, int nw = 4, int kbase = 0, int kcount = 0) {
    // kcount > 0: this workgroup's share of the output channels (rows kbase .. kbase + kcount - 1)
    const int kw = (kcount ? kcount : C) / nw, mf0 = kw / 16, ksn = C / 64;
    for (int tap = 0; tap < 9; ++tap)
        for (int ks = 0; ks < ksn; ++ks)
            for (int mf = 0; mf < mf0; ++mf)
                for (int lane = 0; lane < 64; ++lane) {
                    const int rho = lane & 15, kq = lane >> 4;
                    const int ch = kbase + wave * kw + (rho >> 2) * 4 * mf0 + mf * 4 + (rho & 3);
                    for (int t = 0; t < 16; ++t) {
                        const int c = ks * 64 + kq * 16 + t;
                        out.push_back((uint8_t)w[((size_t)ch * C + c) * 9 + tap]);
                    }
                }
}
// one 1 KB MFMA A-operand fragment (64 lanes x 16 bytes: row = lane & 15, k-group = lane >> 4) of a 1x1 conv's weights [K][C]: rows =
// channels ch_base + (rho >> 2) * 4*mfg + mf*4 + (rho & 3), input channels ks*64 .. +63; and of a 3x3 conv's [K][C][3][3] at one tap
static void pack_frag1(const int8_t* w, int C, int ch_base, int mfg, int mf, int ks, std::vector<uint8_t>& out) {
    for (int lane = 0; lane < 64; ++lane) {
        const int rho = lane & 15, kq = lane >> 4;
        const int8_t* src = w + (size_t)(ch_base + (rho >> 2) * 4 * mfg + mf * 4 + (rho & 3)) * C + ks * 64 + kq * 16;
        out.insert(out.end(), (const uint8_t*)src, (const uint8_t*)src + 16);
    }
}
static void pack_frag3(const int8_t* w, int C, int ch_base, int tap, int ks, std::vector<uint8_t>& out) {
    for (int lane = 0; lane < 64; ++lane) {
        const int rho = lane & 15, kq = lane >> 4;
        for (int t = 0; t < 16; ++t) out.push_back((uint8_t)w[((size_t)(ch_base + rho) * C + ks * 64 + kq * 16 + t) * 9 + tap]);
    }
}
// the four-workgroup cooperative form's streams (conv_chain_coop.hip: conv_chain_coop4_c256_kernel), C = 256: per (quarter q, wave w =
// K-half kh * 4 + n-tile nt), in consumption order:
//   3x3, channels q*64 + nt*16 .. +15:        [tap][k-step kh*2 + {0, 1}]                                        18 fragments
//   1x1 + eltwise, channels q*256 + w*32 ..:  [k-step (q + i) % 4, i = 0..3][accumulator 0, 1]                    8 (its own mid k-step first)
//   1x1, channels q*64 + nt*16 .. +15:        k-steps (q*4 + j) % 16, j = kh*2 + {0, 1} then 4 + kh*6 + {0..5}    8 (its own y1 channels first)
static void pack_coop4_stream(const int8_t* w3, const int8_t* wa, const int8_t* wb, std::vector<uint8_t>& out) {
    const int C = 256, K1 = 1024;
    for (int q = 0; q < 4; ++q)
        for (int w = 0; w < 8; ++w) {
            const int nt = w & 3, kh = w >> 2;
            for (int tap = 0; tap < 9; ++tap)
                for (int kl = 0; kl < 2; ++kl) pack_frag3(w3, C, q * 64 + nt * 16, tap, kh * 2 + kl, out);
            for (int i = 0; i < 4; ++i)
                for (int mf = 0; mf < 2; ++mf) pack_frag1(wa, C, q * 256 + w * 32, 2, mf, (q + i) & 3, out);
            for (int jj = 0; wb && jj < 8; ++jj) {      // (wb == nullptr: a stage's tail has no second 1x1 conv - 26 fragments per (quarter, wave))
                const int j = jj < 2 ? kh * 2 + jj : 4 + kh * 6 + (jj - 2);
                pack_frag1(wb, K1, q * 64 + nt * 16, 1, 0, (q * 4 + j) & 15, out);
            }
        }
}
// ... and the stream of a stage's HEAD (conv_stage4_c256_kernel<.., HEAD>: the sibling pair in front of the run, 512 -> 1024 | 256), per
// (quarter q, wave w = K-half kh * 4 + n-tile nt), in consumption order:
//   a (the shortcut), channels q*256 + w*32 .. +31:    [k-step 0..7][accumulator 0, 1]    16 fragments
//   b (the 3x3 input), channels q*64 + nt*16 .. +15:   k-steps kh*4 + {0..3}               4
static void pack_stage_head_stream(const saber_hip_conv* a, const saber_hip_conv* b, std::vector<uint8_t>& out) {
    const int C0 = 512;
    for (int q = 0; q < 4; ++q)
        for (int w = 0; w < 8; ++w) {
            const int nt = w & 3, kh = w >> 2;
            for (int ks = 0; ks < 8; ++ks)
                for (int mf = 0; mf < 2; ++mf) pack_frag1(a->wq_oihw.data(), C0, q * 256 + w * 32, 2, mf, ks, out);
            for (int j = 0; j < 4; ++j) pack_frag1(b->wq_oihw.data(), C0, q * 64 + nt * 16, 1, 0, kh * 4 + j, out);
        }
}
// ... and the one-workgroup-per-tile stage kernel's (conv_stage1_c128_kernel), C = 128: per wave w, in consumption order:
//   3x3, channels w*16 .. +15: [tap][k-step 0, 1] (18) | 1x1 + eltwise, channels w*64 .. +63: [k-step 0, 1][accumulator 0..3] (8) |
//   1x1, channels w*16 .. +15: [k-step 0..7] (8)
static void pack_stage1_c128_stream(const saber_hip_conv* c3, const saber_hip_conv* a, const saber_hip_conv* b, std::vector<uint8_t>& out) {
    const int C = 128, K1 = 512;
    for (int w = 0; w < 8; ++w) {
        for (int tap = 0; tap < 9; ++tap)
            for (int ks = 0; ks < 2; ++ks) pack_frag3(c3->wq_oihw.data(), C, w * 16, tap, ks, out);
        for (int ks = 0; ks < 2; ++ks)
            for (int mf = 0; mf < 4; ++mf) pack_frag1(a->wq_oihw.data(), C, w * 64, 4, mf, ks, out);
        for (int ks = 0; ks < 8; ++ks) pack_frag1(b->wq_oihw.data(), K1, w * 16, 1, 0, ks, out);
    }
}
// ... and the C = 64 stage kernel's (conv_stage1_c64_kernel, four waves): per wave w, in consumption order:
//   3x3, channels w*16 .. +15: [tap] (9) | 1x1 + eltwise, channels w*64 .. +63: [accumulator 0..3] (4) | 1x1, channels w*16 .. +15: [k-step 0..3] (4)
void pack_stage1_c64_stream(const int8_t* w3, const int8_t* wa, const int8_t* wb, std::vector<uint8_t>& out) {
    const int C = 64, K1 = 256;
    for (int w = 0; w < 4; ++w) {
        for (int tap = 0; tap < 9; ++tap) pack_frag3(w3, C, w * 16, tap, 0, out);
        for (int mf = 0; mf < 4; ++mf) pack_frag1(wa, C, w * 64, 4, mf, 0, out);
        for (int ks = 0; ks < 4; ++ks) pack_frag1(wb, K1, w * 16, 1, 0, ks, out);
    }
}
// ------------------------------------------------------------------------------------------------
// stem conv + max pooling + the sibling pair of 1x1 convs on the pooled tensor in ONE launch (conv_stem.h)
// ------------------------------------------------------------------------------------------------
int saber_hip_conv2d_stem_pair_create(saber_hip_conv_t* stem, const saber_hip_conv_t* a, const saber_hip_conv_t* b, saber_hip_stem_pair_t** out) {
    if (!stem || !a || !b || !out) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    const saber_hip_conv_desc& ds = stem->d;
    if (!stem->pool_fused || !stem->weights_set || ds.k != 64 || (ds.out_dtype != SABER_HIP_U8 && ds.out_dtype != SABER_HIP_S8))
        return fail(SABER_HIP_INVALID_VALUE, "stem pair: the head must be the fused stem conv + max pooling with 64 output channels (8-bit)");
    auto plain1x1 = [&](const saber_hip_conv* o) {
        const saber_hip_conv_desc& d = o->d;
        return o->is_i8 && o->weights_set && o->algo == ALGO_IGEMM_I8 && o->epi == EPI_I8_CONV && d.res_mode == SABER_HIP_RES_NONE &&
               !o->pair_k2 && !o->pool_fused && !o->pool2 && !o->pre_quant && !o->pre_pad && d.kh == 1 && d.kw == 1 && d.stride_h == 1 &&
               d.stride_w == 1 && d.pad_h == 0 && d.pad_w == 0 && d.group == 1 && d.c == 64 && o->c_eff == 64 && d.k % 32 == 0 &&
               d.in_layout == SABER_HIP_NHWC && d.out_layout == SABER_HIP_NHWC && d.act_negative_slope == 0.f &&
               (d.out_dtype == SABER_HIP_S8 || d.out_dtype == SABER_HIP_U8) && d.n == ds.n && d.h == stem->pool_oh && d.w == stem->pool_ow &&
               (o->x_dtype == DT_U8) == (ds.out_dtype == SABER_HIP_U8) && (int)o->wq_oihw.size() == d.k * 64;
    };
    if (!plain1x1(a) || !plain1x1(b) || a->d.k + b->d.k > 320)
        return fail(SABER_HIP_INVALID_VALUE, "stem pair: two plain 1x1 / stride-1 INT8 convs (64 -> k, k % 32 == 0, k_a + k_b <= 320, 8-bit NHWC outputs) "
                                              "on the pooled tensor");
    auto* sp = new saber_hip_stem_pair();
    sp->stem = stem; sp->a = a; sp->b = b;
    const int K1 = a->d.k, Kt = K1 + b->d.k;
    std::vector<int8_t> wcat((size_t)Kt * 64);
    std::memcpy(wcat.data(), a->wq_oihw.data(), (size_t)K1 * 64);
    std::memcpy(wcat.data() + (size_t)K1 * 64, b->wq_oihw.data(), (size_t)b->d.k * 64);
    std::vector<uint8_t> w, pa, pb, prm(256 * 16, 0);
    w.reserve((size_t)Kt * 64);
    for (int g = 0; g < Kt / 32; ++g)
        for (int mf = 0; mf < 2; ++mf) pack_frag1(wcat.data(), 64, g * 32, 2, mf, 0, w);
    pack_chain_params(a, (size_t)K1 / 4 * 3, pa);
    pack_chain_params(b, (size_t)b->d.k / 4 * 3, pb);
    std::memcpy(prm.data(), pa.data(), pa.size());
    std::memcpy(prm.data() + pa.size(), pb.data(), pb.size());
    hipError_t e = sp->d_w.upload(w);
    if (e == hipSuccess) e = sp->d_prm.upload(prm);
    if (e != hipSuccess) {
        delete sp;
        return hip_fail(e, "stem pair: device copies");
    }
    *out = sp;
    return SABER_HIP_OK;
}
void saber_hip_conv2d_stem_pair_destroy(saber_hip_stem_pair_t* sp) { delete sp; }
int saber_hip_conv2d_stem_pair_run(saber_hip_stem_pair_t* sp, const void* x, void* y_pool, void* y_a, void* y_b, void* workspace,
                                   saber_hip_stream_t stream) {
    if (g_capture) return capture_unsupported("saber_hip_conv2d_stem_pair_run (an executor-level object: saber_hip_net_optimize forms it itself)");
    if (!sp || !x || !y_a || !y_b) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    saber_hip_conv* op = sp->stem;
    if (op->ws_bytes && !workspace) return fail(SABER_HIP_INVALID_VALUE, "workspace required");
    saber_mi355x::StemPairKArgs ka;
    const int rc = stem_pool_args(op, x, y_pool, workspace, (hipStream_t)stream, &ka.c);
    if (rc) return rc;
    ka.t.w = sp->d_w.p; ka.t.prm = sp->d_prm.p; ka.t.y1 = y_a; ka.t.y2 = y_b;
    ka.t.K1 = sp->a->d.k; ka.t.K2 = sp->b->d.k;
    ka.t.relu1 = sp->a->d.act == SABER_HIP_ACT_RELU; ka.t.relu2 = sp->b->d.act == SABER_HIP_ACT_RELU;
    ka.t.u8_1 = sp->a->d.out_dtype == SABER_HIP_U8; ka.t.u8_2 = sp->b->d.out_dtype == SABER_HIP_U8;
    HIP_TRY(saber_mi355x::launch_conv_stem_pool_pair(op->pre_quant ? 1 : 0, ka, (hipStream_t)stream));
    return SABER_HIP_OK;
}
saber_hip_chain::~saber_hip_chain() {
    if (h_coop_err) (void)hipHostFree(h_coop_err);
    delete stage1;
}
// ------------------------------------------------------------------------------------------------
// stage: a run of 3x3-led C = 256 (or 128, or 64) chains in ONE persistent launch (conv_stage_coop.hip)
// ------------------------------------------------------------------------------------------------
// ceil(2^32 / d) for the kernels' __umulhi divisions by a tile count; 0 for d == 1 (they then skip the division)
static unsigned div_magic(int d) { return d >= 2 ? (unsigned)((0x100000000ull + (unsigned)d - 1) / (unsigned)d) : 0u; }
// tail (optional): the strided head behind the run - conv3x3 / stride 2 + conv1x1 with the shortcut sub-sampled by 2, no second 1x1 conv -
// whose 3x3 conv reads the last block's second output and whose shortcut is the last block's first output; it then runs inside the launch
// whenever stage_run is given its output
// head_a / head_b (optional, both or none): the sibling pair in front of the run - two plain 1x1 convs over one 512-channel tensor whose
// outputs are exactly the first block's shortcut (head_a: 1024 channels, s8) and 3x3 input (head_b: 256 channels); they then run inside the
// launch whenever stage_run is given head_b's output
static int stage_build(saber_hip_chain* const* chains, int n, bool per_image, saber_hip_chain* tail, saber_hip_chain_stage** out,
                       const saber_hip_conv* head_a = nullptr, const saber_hip_conv* head_b = nullptr) {
    if (!chains || n <= 0 || n > saber_mi355x::STAGE4_LONG || !out) return fail(SABER_HIP_INVALID_VALUE, "stage: 1..24 chains");
    if (head_a || head_b) {
        if (!head_a || !head_b) return fail(SABER_HIP_INVALID_VALUE, "null argument");
        if (!chains[0] || chains[0]->c1 != 256) return fail(SABER_HIP_INVALID_VALUE, "stage: a head goes with a C = 256 stage only");
        if (!per_image) return fail(SABER_HIP_INVALID_VALUE, "stage: a head needs an image per XCD");
        for (const saber_hip_conv* o : {head_a, head_b})
            if (o->d.res_mode != SABER_HIP_RES_NONE) return fail(SABER_HIP_INVALID_VALUE, "stage: the head's convs carry no residual");
        for (const saber_hip_conv* o : {head_a, head_b}) {
            const saber_hip_conv_desc& d = o->d;
            if (!o->is_i8 || !o->weights_set || o->algo != ALGO_IGEMM_I8 || o->epi != EPI_I8_CONV || o->pair_k2 || o->pool_fused || o->pool2 || o->gpool ||
                o->pre_quant || o->pre_pad || d.kh != 1 || d.kw != 1 || d.stride_h != 1 || d.stride_w != 1 || d.pad_h != 0 || d.pad_w != 0 || d.group != 1 ||
                o->c_eff != d.c || d.act_negative_slope != 0.f || d.in_layout != SABER_HIP_NHWC || d.out_layout != SABER_HIP_NHWC ||
                (d.out_dtype != SABER_HIP_S8 && d.out_dtype != SABER_HIP_U8))
                return fail(SABER_HIP_INVALID_VALUE, "stage: the head must be two plain 1x1 / stride 1 / pad 0 INT8 NHWC convs with weights set");
        }
        if (head_a->d.c != 512 || head_b->d.c != 512) return fail(SABER_HIP_INVALID_VALUE, "stage: the head's convs read 512 channels");
        if (head_a->d.k != 1024 || head_b->d.k != 256) return fail(SABER_HIP_INVALID_VALUE, "stage: the head's convs write 1024 and 256 channels");
        const saber_hip_conv_desc &d0 = chains[0]->a->d, &da = head_a->d, &db = head_b->d;
        if (!chains[0]->c3 || da.n != d0.n || da.h != d0.h || da.w != d0.w || db.n != d0.n || db.h != d0.h || db.w != d0.w || head_a->x_dtype != head_b->x_dtype ||
            da.out_dtype != SABER_HIP_S8 || (db.out_dtype == SABER_HIP_U8) != (chains[0]->c3->x_dtype == DT_U8))
            return fail(SABER_HIP_INVALID_VALUE, "stage: the head's outputs must be the first block's shortcut (s8) and 3x3 input (its dtype), one input tensor");
    }
    if (tail) {
        if (!chains[0] || chains[0]->c1 != 256 || tail->c1 != 256) return fail(SABER_HIP_INVALID_VALUE, "stage: a tail goes with a C = 256 stage only");
        if (n < 2 || !per_image || n + 1 > saber_mi355x::STAGE4_LONG) return fail(SABER_HIP_INVALID_VALUE, "stage: a tail needs 2..23 blocks, an image per XCD");
        if (!tail->c3 || tail->b || tail->b2 || tail->c3->d.stride_h != 2 || tail->c3->d.stride_w != 2)
            return fail(SABER_HIP_INVALID_VALUE, "stage: the tail must be a conv3x3 / stride 2 + conv1x1 chain without a second 1x1 conv");
        if (tail->a->d.res_stride != 2) return fail(SABER_HIP_INVALID_VALUE, "stage: the tail's shortcut must be sub-sampled by 2");
    }
    if (n > 1 && !per_image) return fail(SABER_HIP_INVALID_VALUE, "stage: several blocks need an image per XCD");
    if (n < 2 && chains[0] && (chains[0]->c1 == 128 || chains[0]->c1 == 64)) return fail(SABER_HIP_INVALID_VALUE, "stage: at C = 128 / 64 a stage is at least two blocks");
    const saber_hip_chain* c0 = chains[0];
    std::vector<saber_mi355x::StageBlk> blk;
    for (int k = 0; k < n; ++k) {
        const saber_hip_chain* ch = chains[k];
        const uint8_t* stream = !ch ? nullptr : (ch->c1 == 256 ? ch->d_stream[CS_COOP4].p : (ch->c1 == 128 || ch->c1 == 64 ? ch->d_stream_stage1.p : nullptr));
        if (!ch || ch->c1 != c0->c1 || !ch->c3 || !ch->b || !stream || ch->c3->d.stride_h != 1)
            return fail(SABER_HIP_INVALID_VALUE, "stage: every block must be a conv3x3 (stride 1) + conv1x1 + conv1x1 chain at C = 256 (or all at C = 128, or all at C = 64)");
        const saber_hip_conv_desc& da = ch->a->d;
        if (da.n != c0->a->d.n || da.h != c0->a->d.h || da.w != c0->a->d.w) return fail(SABER_HIP_INVALID_VALUE, "stage: blocks of one tensor shape");
        if (k && ((ch->c3->x_dtype == DT_U8) != (chains[k - 1]->b->d.out_dtype == SABER_HIP_U8)))
            return fail(SABER_HIP_INVALID_VALUE, "stage: a block's 3x3 conv reads what the previous block's last conv writes");
        saber_mi355x::StageBlk B;
        std::memset(&B, 0, sizeof B);
        B.wstream = stream; B.prm0 = ch->d_prm0.p; B.prm1 = ch->d_prm1.p; B.prm2 = ch->d_prm2.p;
        B.coeff_conv = da.coeff_conv; B.scale_conv = ch->scale_conv; B.coeff_res = da.coeff_res; B.scale_res = da.scale_res;
        B.in0_u8 = ch->c3->x_dtype == DT_U8; B.relu0 = ch->c3->d.act == SABER_HIP_ACT_RELU;
        B.in_u8 = ch->a->x_dtype == DT_U8; B.relu1 = da.act == SABER_HIP_ACT_RELU; B.res_relu = da.res_act == SABER_HIP_ACT_RELU;
        B.relu2 = ch->b->d.act == SABER_HIP_ACT_RELU; B.out_u8_2 = ch->b->d.out_dtype == SABER_HIP_U8;
        blk.push_back(B);
    }
    const saber_hip_conv_desc& d0 = c0->a->d;
    if (tail) {
        const saber_hip_conv_desc &d3 = tail->c3->d, &da = tail->a->d;
        if (d3.n != d0.n || d3.h != d0.h || d3.w != d0.w || da.res_h != d0.h || da.res_w != d0.w)
            return fail(SABER_HIP_INVALID_VALUE, "stage: the tail's 3x3 conv and shortcut read tensors of the blocks' shape");
        if ((tail->c3->x_dtype == DT_U8) != (chains[n - 1]->b->d.out_dtype == SABER_HIP_U8))
            return fail(SABER_HIP_INVALID_VALUE, "stage: the tail's 3x3 conv reads what the last block's last conv writes");
    }
    saber_hip_chain_stage* st = new saber_hip_chain_stage();
    st->chains.assign(chains, chains + n);
    st->c1 = c0->c1;
    st->n = d0.n; st->h = d0.h; st->w = d0.w;
    st->tiles_x = (d0.w + 15) / 16;
    st->tiles_per_img = st->tiles_x * ((d0.h + 1) / 2);
    st->per_image = per_image;
    // every workgroup of an image must hold a CU of its XCD at once (one workgroup per CU: 235 - 250 VGPRs); C = 256: four workgroups per
    // tile, edge counters for one column tile; C = 128: one per tile, 1 / 2 / 4 column tiles (arrivals per edge: a power of two);
    // C = 64: one per tile and SEVERAL workgroups per CU (conv_stage1_c64_kernel: 128 VGPRs, 22 KB of LDS) - as many as the runtime's
    // occupancy query gives this kernel, so what it cannot keep resident is refused here and never waited for
    const int wg_per_tile = st->c1 == 256 ? 4 : 1;
    const int wg_per_cu = st->c1 == 64 ? saber_mi355x::conv_stage1_c64_blocks_per_cu() : 1;
    const bool fits = d0.n <= 8 && st->tiles_per_img * wg_per_tile <= 32 * wg_per_cu &&
                      (st->c1 == 256 ? st->tiles_x == 1 : (st->tiles_x == 1 || st->tiles_x == 2 || st->tiles_x == 4));
    if ((per_image && !fits) || (st->c1 != 256 && !per_image)) {
        delete st;
        return fail(SABER_HIP_INVALID_VALUE, "stage: an image per XCD needs batch <= 8 and every workgroup of an image resident on its XCD's 32 CUs (C = 256: "
                    "width <= 16, <= 8 tiles of 2 x 16 pixels; C = 128: width <= 64, <= 32 tiles; C = 64: width <= 64, <= 32 x the kernel's workgroups per CU)");
    }
    const size_t tiles = (size_t)d0.n * st->tiles_per_img;
    hipError_t e = hipSuccess;
    if (tail) {      // its constants are block n of the table (prm2: unused, the launch copies it like a block's - any readable constants do)
        std::vector<uint8_t> ts;
        if (tail->tail_w3.empty() || tail->tail_wa.empty()) {
            delete st;
            return fail(SABER_HIP_INVALID_VALUE, "stage: the tail chain holds no copy of its members' weights");
        }
        pack_coop4_stream(tail->tail_w3.data(), tail->tail_wa.data(), nullptr, ts);      // (the weights the CHAIN was created with, like its constants)
        e = st->d_tail_stream.upload(ts);
        const saber_hip_conv_desc& da = tail->a->d;
        saber_mi355x::StageBlk B;
        std::memset(&B, 0, sizeof B);
        B.wstream = st->d_tail_stream.p; B.prm0 = tail->d_prm0.p; B.prm1 = tail->d_prm1.p; B.prm2 = tail->d_prm0.p;
        B.coeff_conv = da.coeff_conv; B.scale_conv = tail->scale_conv; B.coeff_res = da.coeff_res; B.scale_res = da.scale_res;
        B.in0_u8 = tail->c3->x_dtype == DT_U8; B.relu0 = tail->c3->d.act == SABER_HIP_ACT_RELU;
        B.in_u8 = tail->a->x_dtype == DT_U8; B.relu1 = da.act == SABER_HIP_ACT_RELU; B.res_relu = da.res_act == SABER_HIP_ACT_RELU;
        blk.push_back(B);
        st->tail = tail;
    }
    if (head_a) {      // its constants are the table's FIRST entry, in front of block 0's: a launch passes d_blk + 1 (prm0: unused, the launch copies it like a block's)
        std::vector<uint8_t> hs, p1, p2;
        pack_stage_head_stream(head_a, head_b, hs);
        pack_chain_params(head_a, (size_t)head_a->d.k / 4 * 3, p1);
        pack_chain_params(head_b, ((size_t)head_b->d.k / 4 * 3 + 63) / 64 * 64 + 64, p2);      // (+ slack: whole 64-chunk blocks are copied)
        if (e == hipSuccess) e = st->d_head_stream.upload(hs);
        if (e == hipSuccess) e = st->d_head_prm1.upload(p1);
        if (e == hipSuccess) e = st->d_head_prm2.upload(p2);
        saber_mi355x::StageBlk B;
        std::memset(&B, 0, sizeof B);
        B.wstream = st->d_head_stream.p; B.prm0 = st->d_head_prm2.p; B.prm1 = st->d_head_prm1.p; B.prm2 = st->d_head_prm2.p;
        B.in_u8 = head_a->x_dtype == DT_U8; B.relu1 = head_a->d.act == SABER_HIP_ACT_RELU;
        B.relu2 = head_b->d.act == SABER_HIP_ACT_RELU; B.out_u8_2 = head_b->d.out_dtype == SABER_HIP_U8;
        blk.insert(blk.begin(), B);
        st->head_a = head_a; st->head_b = head_b;
    }
    if (e == hipSuccess) e = st->d_blk.upload(blk);
    if (e == hipSuccess && st->c1 == 256) e = st->d_grp_ctr.alloc_zero(tiles * 32);
    if (e == hipSuccess) e = st->d_img_ctr.alloc_zero((size_t)d0.n * (st->tiles_per_img + 1) * 16);
    if (e == hipSuccess) e = st->d_xcc.alloc_zero(tiles * 32);
    if (e == hipSuccess && st->c1 == 256) e = st->d_xch.alloc_zero(tiles * 32 * 256);
    if (e == hipSuccess) e = hipHostMalloc((void**)&st->h_err, sizeof(unsigned), hipHostMallocMapped);
    if (e != hipSuccess) {
        delete st;
        return hip_fail(e, "stage: device buffers");
    }
    *st->h_err = 0u;
    *out = st;
    return SABER_HIP_OK;
}
template <int MAXB>
static int stage_launch(saber_hip_chain_stage* st, const void* x, const void* res, void* const* y1, void* const* y2, void* y_tail, void* y_head, hipStream_t s) {
    saber_mi355x::Stage4KArgs<MAXB> k;
    std::memset(&k, 0, sizeof k);
    k.x = x; k.res = res; k.zero = zero_page();
    if (!k.zero) return fail(SABER_HIP_RUNTIME_ERROR, "stage: zero page");
    k.blk = st->d_blk.p + (st->head_a ? 1 : 0); k.grp_ctr = st->d_grp_ctr.p; k.img_ctr = st->d_img_ctr.p; k.xch = st->d_xch.p; k.xcc = st->d_xcc.p; k.err = st->h_err;
    k.nblk = (int)st->chains.size(); k.N = st->n; k.H = st->h; k.W = st->w;
    k.tiles_x = st->tiles_x; k.tiles_per_img = st->tiles_per_img;
    k.mg_tiles_x = div_magic(st->tiles_x); k.mg_tpi = div_magic(st->tiles_per_img); k.mg_wpi = div_magic(st->tiles_per_img * 4);
    k.per_image = st->per_image;
    for (int i = 0; i < k.nblk; ++i) { k.y1[i] = y1[i]; k.y2[i] = y2[i]; }
    if (y_tail) k.y1[k.nblk] = y_tail;      // (the slot behind the last block's: stage_run has picked an argument block with room for it)
    k.head_y = y_head;                      // (with a head x is the pair's input and res is not read)
    HIP_TRY(st->c1 == 256 ? saber_mi355x::launch_conv_stage4(k, y_tail != nullptr, y_head != nullptr, s)
                          : (st->c1 == 128 ? saber_mi355x::launch_conv_stage1_c128(k, s) : saber_mi355x::launch_conv_stage1_c64(k, s)));
    return SABER_HIP_OK;
}
int stage_run(saber_hip_chain_stage* st, const void* x, const void* res, void* const* y1, void* const* y2, hipStream_t s, void* y_tail, void* y_head) {
    if (y_tail && !st->tail) return fail(SABER_HIP_INVALID_VALUE, "stage: created without a tail");
    if (y_head && !st->head_a) return fail(SABER_HIP_INVALID_VALUE, "stage: created without a head");
    if (*(volatile unsigned*)st->h_err) {      // an earlier launch found cooperating workgroups on different XCDs or timed out in a barrier
        *(volatile unsigned*)st->h_err = 0u;
        return fail(SABER_HIP_RUNTIME_ERROR, "cooperative stage: an earlier launch's workgroups did not share an XCD or timed out at a barrier "
                    "(its outputs are not valid)");
    }
    return (int)st->chains.size() + (y_tail ? 1 : 0) <= saber_mi355x::STAGE4_SHORT ? stage_launch<saber_mi355x::STAGE4_SHORT>(st, x, res, y1, y2, y_tail, y_head, s)
                                                                                   : stage_launch<saber_mi355x::STAGE4_LONG>(st, x, res, y1, y2, y_tail, y_head, s);
}
int saber_hip_conv2d_stage_create(saber_hip_chain_t* const* chains, int n, saber_hip_chain_stage_t** out) {
    if (!xcd_round_robin()) return fail(SABER_HIP_UNIMPL, "stage: this device does not place workgroup b on XCD b % 8");
    return stage_build(chains, n, true, nullptr, out);
}
int saber_hip_conv2d_stage_create_tail(saber_hip_chain_t* const* chains, int n, saber_hip_chain_t* tail, saber_hip_chain_stage_t** out) {
    if (!tail) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    if (!xcd_round_robin()) return fail(SABER_HIP_UNIMPL, "stage: this device does not place workgroup b on XCD b % 8");
    return stage_build(chains, n, true, tail, out);
}
int saber_hip_conv2d_stage_create_head(saber_hip_chain_t* const* chains, int n, saber_hip_chain_t* tail, const saber_hip_conv_t* head_a,
                                       const saber_hip_conv_t* head_b, saber_hip_chain_stage_t** out) {
    if (!head_a || !head_b) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    if (!xcd_round_robin()) return fail(SABER_HIP_UNIMPL, "stage: this device does not place workgroup b on XCD b % 8");
    return stage_build(chains, n, true, tail, out, head_a, head_b);
}
void saber_hip_conv2d_stage_destroy(saber_hip_chain_stage_t* st) { delete st; }
int saber_hip_conv2d_stage_run(saber_hip_chain_stage_t* st, const void* x, const void* res, void* const* y1, void* const* y2, saber_hip_stream_t stream) {
    if (g_capture) return capture_unsupported("saber_hip_conv2d_stage_run (saber_hip_net_optimize forms stages itself)");
    if (!st || !x || !res || !y1 || !y2) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    // (C = 64: a null y1[i] of a block that is not the last leaves that tensor unwritten - its tile stays in LDS for block i + 1)
    for (size_t i = 0; i < st->chains.size(); ++i)
        if ((!y1[i] && !(st->c1 == 64 && i + 1 < st->chains.size())) || !y2[i]) return fail(SABER_HIP_INVALID_VALUE, "stage: an output pointer per block");
    return stage_run(st, x, res, y1, y2, (hipStream_t)stream);
}
int saber_hip_conv2d_stage_run_tail(saber_hip_chain_stage_t* st, const void* x, const void* res, void* const* y1, void* const* y2, void* y_tail,
                                    saber_hip_stream_t stream) {
    if (g_capture) return capture_unsupported("saber_hip_conv2d_stage_run_tail (saber_hip_net_optimize forms stages itself)");
    if (!st || !x || !res || !y1 || !y2 || !y_tail) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    for (size_t i = 0; i < st->chains.size(); ++i)
        if (!y1[i] || !y2[i]) return fail(SABER_HIP_INVALID_VALUE, "stage: an output pointer per block");
    return stage_run(st, x, res, y1, y2, (hipStream_t)stream, y_tail);
}
int saber_hip_conv2d_stage_run_head(saber_hip_chain_stage_t* st, const void* x_head, void* y_head_b, void* const* y1, void* const* y2, void* y_tail,
                                    saber_hip_stream_t stream) {
    if (g_capture) return capture_unsupported("saber_hip_conv2d_stage_run_head (saber_hip_net_optimize forms stages itself)");
    if (!st || !x_head || !y_head_b || !y1 || !y2) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    for (size_t i = 0; i < st->chains.size(); ++i)
        if (!y1[i] || !y2[i]) return fail(SABER_HIP_INVALID_VALUE, "stage: an output pointer per block");
    return stage_run(st, x_head, nullptr, y1, y2, (hipStream_t)stream, y_tail, y_head_b);
}
// the weight stream of one layout, in the order the waves of the forms that read it consume it (conv1x1_chain.hip, conv_chain_coop.hip)
static void pack_chain_stream(const saber_hip_chain* ch, ChainStream layout, std::vector<uint8_t>& out) {
    const saber_hip_conv *c3 = ch->c3, *a = ch->a, *b = ch->b;
    const int c = ch->c1, k1 = ch->k1, k2 = ch->k2, c2 = b ? b->d.c : 0, k2w = k2 / 2;
    const int nw = layout == CS_BASE || layout == CS_SPLIT ? 4 : 8;      // waves per workgroup
    const int8_t *w3 = c3 ? c3->wq_oihw.data() : nullptr, *wa = a->wq_oihw.data(), *wb = b ? b->wq_oihw.data() : nullptr;
    std::vector<int8_t> wcat;       // the pair's rows one after the other
    if (ch->b2) {
        wcat.assign(b->wq_oihw.begin(), b->wq_oihw.end());
        wcat.insert(wcat.end(), ch->b2->wq_oihw.begin(), ch->b2->wq_oihw.end());
        wb = wcat.data();
    }
    // accumulators per channel group of the second conv: its channels per wave / 16, at most 4 (pair: 160 channels per wave = 5 groups of 32)
    auto mfg = [&](int k) { return ch->b2 ? 2 : std::min(4, k / nw / 16); };
    switch (layout) {
    case CS_BASE: case CS_W8:        // per wave [3x3][1x1 + eltwise][1x1]
        for (int w = 0; w < nw; ++w) {
            if (c3) pack_chain_weights3(w3, c, w, out, nw);
            pack_chain_weights(wa, k1, c, 4, w, out, 0, nw);
            if (b) pack_chain_weights(wb, k2, c2, mfg(k2), w, out, 0, nw);
        }
        break;
    case CS_SPLIT: case CS_SPLIT8:   // [half][wave]: the whole first conv, half of the second conv's channels
        for (int half = 0; half < 2; ++half)
            for (int w = 0; w < nw; ++w) {
                pack_chain_weights(wa, k1, c, 4, w, out, 0, nw);
                pack_chain_weights(wb, k2w, c2, mfg(k2w), w, out, half * k2w, nw);
            }
        break;
    case CS_COOP2:      // per (half, wave) [3x3: 16 channels][1x1: 64 channels][1x1: 16 channels], each half's own k-steps first
        for (int half = 0; half < 2; ++half)
            for (int w = 0; w < nw; ++w) {
                pack_chain_weights3(w3, c, w, out, nw, half * (c / 2), c / 2);
                pack_chain_weights(wa, k1 / 2, c, 4, w, out, half * (k1 / 2), nw, half * (c / 128));
                pack_chain_weights(wb, k2w, c2, 1, w, out, half * k2w, nw, half * (c2 / 128));
            }
        break;
    default: pack_coop4_stream(w3, wa, wb, out);      // CS_COOP4
    }
}
static int chain_build(saber_hip_conv* c3, saber_hip_conv* a, saber_hip_conv* b, saber_hip_chain_t** out, saber_hip_conv* b2 = nullptr) {
    // b == nullptr (with c3): conv3x3 + first 1x1 conv only; b2 (with c3 / stride 2 and b): b and b2 are the sibling pair that reads a's output
    if (!a || !out || (!b && !c3) || (b2 && (!b || !c3))) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    const bool pair2 = b2 != nullptr;
    // a sub-sampled shortcut (saber_hip_conv_desc::res_stride) is read by the conv3x3 + conv1x1 form with a strided head only
    const bool strided = c3 && (!b || pair2) && c3->d.stride_h == 2 && c3->d.stride_w == 2;
    if (pair2 && !strided) return fail(SABER_HIP_INVALID_VALUE, "chain: a sibling pair follows the strided head (conv3x3 / stride 2 + conv1x1 + eltwise) only");
    if (!chain_1x1(a, strided) || (b && !chain_1x1(b)) || (b2 && !chain_1x1(b2)))
        return fail(SABER_HIP_INVALID_VALUE, "chain: both ops must be plain 1x1 stride-1 INT8 NHWC convs with weights set");
    if (strided != (a->d.res_stride > 1) || (strided && a->d.res_stride != 2))
        return fail(SABER_HIP_INVALID_VALUE, "chain: a stride-2 head goes with a shortcut sub-sampled by 2 (and only with one)");
    const saber_hip_conv_desc& da = a->d;
    if (da.res_mode != SABER_HIP_RES_ELTWISE || da.out_dtype != SABER_HIP_S8 || (da.res_has_dtype && da.res_dtype != SABER_HIP_S8))
        return fail(SABER_HIP_INVALID_VALUE, "chain: the first conv must carry the fused eltwise epilogue with s8 residual and output");
    if (b) {
        const saber_hip_conv_desc& db = b->d;
        if (db.res_mode != SABER_HIP_RES_NONE || b->x_dtype != DT_S8 || (db.out_dtype != SABER_HIP_S8 && db.out_dtype != SABER_HIP_U8))
            return fail(SABER_HIP_INVALID_VALUE, "chain: the second conv must be a plain s8-input conv with an 8-bit output");
        if (db.n != da.n || db.h != a->oh || db.w != a->ow || db.c != da.k || (!pair2 && db.k != da.c))
            return fail(SABER_HIP_INVALID_VALUE, "chain: shapes must be C -> 4C -> C with C in {64,128,256,512} on the same pixels");
    }
    if (pair2) {
        const saber_hip_conv_desc &db = b->d, &d2 = b2->d;
        if (d2.res_mode != SABER_HIP_RES_NONE || b2->x_dtype != DT_S8 || (d2.out_dtype != SABER_HIP_S8 && d2.out_dtype != SABER_HIP_U8) || d2.n != da.n ||
            d2.h != a->oh || d2.w != a->ow || d2.c != da.k || da.c != 64 || db.k % 32 || db.k + d2.k != 640 || d2.k <= 0)
            return fail(SABER_HIP_INVALID_VALUE, "chain: the sibling pair after a strided head: 64 -> 256 (+ eltwise) -> k_b | k_b2 with k_b + k_b2 = 640, k_b % 32 == 0, 8-bit outputs");
    }
    if (!conv1x1_chain_ok(da.c, da.k, da.c))
        return fail(SABER_HIP_INVALID_VALUE, "chain: shapes must be C -> 4C -> C with C in {64,128,256,512} on the same pixels");
    if (c3) {
        const saber_hip_conv_desc& d3 = c3->d;
        const bool ok = c3->is_i8 && c3->weights_set && c3->algo == ALGO_IGEMM_I8 && c3->epi == EPI_I8_CONV && d3.kh == 3 && d3.kw == 3 &&
                        d3.stride_h == (strided ? 2 : 1) && d3.stride_w == d3.stride_h && d3.pad_h == 1 && d3.pad_w == 1 && d3.dil_h == 1 && d3.dil_w == 1 &&
                        d3.group == 1 && !c3->pair_k2 && !c3->pool_fused && !c3->pool2 && !c3->pre_quant && !c3->pre_pad &&
                        c3->c_eff == d3.c && d3.act_negative_slope == 0.f && d3.in_layout == SABER_HIP_NHWC &&
                        d3.out_layout == SABER_HIP_NHWC && d3.res_mode == SABER_HIP_RES_NONE && d3.c == da.c && d3.k == da.c &&
                        d3.n == da.n && c3->oh == da.h && c3->ow == da.w && da.c <= 256 &&
                        (d3.out_dtype == SABER_HIP_S8 || d3.out_dtype == SABER_HIP_U8) &&
                        (d3.out_dtype == SABER_HIP_U8) == (a->x_dtype == DT_U8);
        if (!ok) return fail(SABER_HIP_INVALID_VALUE, "chain: the head must be the 3x3 pad-1 INT8 conv (C -> C, C <= 256; stride 1, or 2 in front of a lone 1x1 conv) whose 8-bit output the first 1x1 conv reads");
    }
    saber_hip_chain* ch = new saber_hip_chain();
    const int k2 = b ? b->d.k + (pair2 ? b2->d.k : 0) : 0;
    ch->c3 = c3; ch->a = a; ch->b = b; ch->b2 = b2; ch->c1 = da.c; ch->k1 = da.k; ch->k2 = k2;
    ch->scale_conv = a->out_scale;
    if (c3 && !b && da.c == 256 && strided) {      // a possible tail of a stage launch: the stage packs its stream from THESE weights (copies at create)
        ch->tail_w3 = c3->wq_oihw;
        ch->tail_wa = a->wq_oihw;
    }
    ch->form = chain_form_default(ch);
    // one stream per layout that some form of this chain reads; the placement-dependent ones only where the device places workgroups the
    // way their hand-off relies on (probed once per device)
    std::vector<uint8_t> p0, p1, p2;
    hipError_t e = hipSuccess;
    for (int l = 0; l < CS_COUNT && e == hipSuccess; ++l) {
        bool needed = false;
        for_each_chain_form(ch, [&](const ChainForm& f) { needed = needed || (f.stream == l && (!f.placement || xcd_round_robin())); });
        if (!needed) continue;
        std::vector<uint8_t> stream;
        pack_chain_stream(ch, (ChainStream)l, stream);
        e = ch->d_stream[l].upload(stream);
    }
    pack_chain_params(a, (size_t)da.k / 4 * 3, p1);
    if (b) pack_chain_params(b, ((size_t)k2 / 4 * 3 + 63) / 64 * 64 + 64, p2);      // (+ 64 chunks of slack: the cooperative kernel DMAs whole 64-chunk blocks)
    if (pair2) {                    // b2's constants behind b's (48 bytes per 4 channels)
        std::vector<uint8_t> pb2;
        pack_chain_params(b2, (size_t)b2->d.k / 4 * 3, pb2);
        std::memcpy(p2.data() + (size_t)b->d.k / 4 * 48, pb2.data(), pb2.size());
    }
    if (e == hipSuccess && ch->d_stream[CS_COOP2].p) {      // tiles of one row x 16 columns
        ch->coop_tiles = da.n * da.h * ((da.w + 15) / 16);
        e = ch->d_coop_ctr.alloc_zero((size_t)ch->coop_tiles * 32);      // a 128-byte line per (tile, barrier)
        if (e == hipSuccess) e = ch->d_coop_xcc.alloc_zero((size_t)ch->coop_tiles * 32);
        if (e == hipSuccess) e = ch->d_coop_xch.alloc_zero((size_t)ch->coop_tiles * 16 * da.c);
        if (e == hipSuccess) e = hipHostMalloc((void**)&ch->h_coop_err, sizeof(unsigned), hipHostMallocMapped);
        if (e == hipSuccess) *ch->h_coop_err = 0u;
    }
    if (e == hipSuccess && (da.c == 128 || da.c == 64) && c3 && b && !pair2 && c3->d.stride_h == 1 && xcd_round_robin()) {
        std::vector<uint8_t> s1;
        if (da.c == 128) pack_stage1_c128_stream(c3, a, b, s1);
        else pack_stage1_c64_stream(c3->wq_oihw.data(), a->wq_oihw.data(), b->wq_oihw.data(), s1);
        e = ch->d_stream_stage1.upload(s1);
    }
    if (e == hipSuccess) e = ch->d_prm1.upload(p1);
    if (e == hipSuccess && b) e = ch->d_prm2.upload(p2);
    if (e == hipSuccess && c3) {
        pack_chain_params(c3, ((size_t)da.c / 4 * 3 + 63) / 64 * 64 + 64, p0);
        e = ch->d_prm0.upload(p0);
    }
    if (e != hipSuccess) {
        delete ch;
        return hip_fail(e, "chain: device copies");
    }
    if (ch->d_stream[CS_COOP4].p) {      // the four-workgroup form = a one-block stage, tiles spread over all XCDs
        const int rc = stage_build(&ch, 1, false, nullptr, &ch->stage1);
        if (rc != SABER_HIP_OK) {
            delete ch;
            return rc;
        }
    }
    *out = ch;
    return SABER_HIP_OK;
}
int saber_hip_conv2d_chain_create(saber_hip_conv_t* a, saber_hip_conv_t* b, saber_hip_chain_t** out) {
    if (!b) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    return chain_build(nullptr, a, b, out);
}
int saber_hip_conv2d_chain_create3(saber_hip_conv_t* conv3x3, saber_hip_conv_t* a, saber_hip_conv_t* b, saber_hip_chain_t** out) {
    if (!conv3x3) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    return chain_build(conv3x3, a, b, out);
}
int saber_hip_conv2d_chain_create3_pair(saber_hip_conv_t* conv3x3, saber_hip_conv_t* a, saber_hip_conv_t* pair_a, saber_hip_conv_t* pair_b,
                                        saber_hip_chain_t** out) {
    if (!conv3x3 || !pair_a || !pair_b) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    return chain_build(conv3x3, a, pair_a, out, pair_b);
}
void saber_hip_conv2d_chain_destroy(saber_hip_chain_t* ch) { delete ch; }
int saber_hip_conv2d_chain_set_tile(saber_hip_chain_t* ch, int tn) {
    if (!ch) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    if (!chain_form_valid(ch, tn)) return fail(SABER_HIP_INVALID_VALUE, "chain: no kernel form with that code for this chain");
    ch->form = chain_form(ch, tn);
    return SABER_HIP_OK;
}
int saber_hip_conv2d_chain_get_tile(const saber_hip_chain_t* ch) { return ch ? ch->form.code : 0; }
int saber_hip_conv2d_chain_run(saber_hip_chain_t* ch, const void* x, const void* res, void* y_a, void* y_b,
                               saber_hip_stream_t stream) {
    return saber_hip_conv2d_chain_run3(ch, x, res, y_a, y_b, nullptr, stream);
}
int saber_hip_conv2d_chain_run3(saber_hip_chain_t* ch, const void* x, const void* res, void* y_a, void* y_b, void* y_c,
                                saber_hip_stream_t stream) {
    if (g_capture) return capture_unsupported("saber_hip_conv2d_chain_run (saber_hip_net_optimize forms chains itself)");
    if (!ch || !x || !res || !y_a || (ch->b && !y_b) || (ch->b2 && !y_c)) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    const saber_hip_conv *a = ch->a, *b = ch->b;
    ChainKArgs k;
    std::memset(&k, 0, sizeof k);
    k.x = x; k.res = res;
    const ChainForm f = ch->form;
    k.wstream = ch->d_stream[f.stream].p;
    k.prm1 = ch->d_prm1.p;
    k.prm2 = ch->d_prm2.p;
    k.y1 = y_a; k.y2 = y_b;
    k.M = a->d.n * a->oh * a->ow;
    k.in_u8 = a->x_dtype == DT_U8;
    k.relu1 = a->d.act == SABER_HIP_ACT_RELU;
    k.res_relu = a->d.res_act == SABER_HIP_ACT_RELU;
    k.coeff_conv = a->d.coeff_conv; k.scale_conv = ch->scale_conv; k.coeff_res = a->d.coeff_res; k.scale_res = a->d.scale_res;
    if (b) {
        k.relu2 = b->d.act == SABER_HIP_ACT_RELU;
        k.out_u8_2 = b->d.out_dtype == SABER_HIP_U8;
    }
    if (ch->b2) {
        k.y2b = y_c;
        k.k2_split = b->d.k;
        k.relu2b = ch->b2->d.act == SABER_HIP_ACT_RELU;
        k.out_u8_2b = ch->b2->d.out_dtype == SABER_HIP_U8;
    }
    if (ch->c3) {   // x is the 3x3 conv's input; tiles of f.rows rows x 16 columns
        k.prm0 = ch->d_prm0.p;
        k.zero = zero_page();
        if (!k.zero) return fail(SABER_HIP_RUNTIME_ERROR, "chain: zero page");
        k.N = a->d.n; k.H = a->d.h; k.W = a->d.w;
        k.tiles_x = (k.W + 15) / 16;
        k.tiles_per_img = k.tiles_x * ((k.H + f.rows - 1) / f.rows);
        k.mg_tiles_x = div_magic(k.tiles_x);
        k.mg_tpi = div_magic(k.tiles_per_img);
        k.in0_u8 = ch->c3->x_dtype == DT_U8;
        k.relu0 = ch->c3->d.act == SABER_HIP_ACT_RELU;
        k.s0 = ch->c3->d.stride_h;
        k.H0 = ch->c3->d.h; k.W0 = ch->c3->d.w;
        if (a->d.res_stride > 1) { k.res_sub = a->d.res_stride; k.res_H = a->d.res_h; k.res_W = a->d.res_w; }
    }
    if (f.coop == 4) {      // four cooperating workgroups per tile of 2 x 16 pixels: a one-block stage
        const int rc = stage_run(ch->stage1, x, res, &y_a, &y_b, (hipStream_t)stream);
        if (rc != SABER_HIP_OK) ch->form = chain_form_plain(ch);
        return rc;
    }
    if (f.coop == 2) {      // two cooperating workgroups per pixel tile
        if (*(volatile unsigned*)ch->h_coop_err) {      // an earlier launch found its halves on different XCDs or timed out in a barrier
            *(volatile unsigned*)ch->h_coop_err = 0u;
            ch->form = chain_form_plain(ch);
            return fail(SABER_HIP_RUNTIME_ERROR, "cooperative chain: an earlier launch's workgroup pairs did not share an XCD or timed out at their "
                        "barrier (its outputs are not valid); the chain now runs the single-workgroup form");
        }
        const CoopKArgs ck{k, ch->d_coop_ctr.p, ch->d_coop_xch.p, ch->d_coop_xcc.p, ch->h_coop_err, ch->coop_tiles};
        HIP_TRY(launch_conv_chain_coop(ck, (hipStream_t)stream));
        return SABER_HIP_OK;
    }
    HIP_TRY(launch_conv1x1_chain(k, ch->c1, ch->k1, ch->k2, f.rows, f.waves, f.split, ch->c3 ? 1 : 0, (hipStream_t)stream));
    return SABER_HIP_OK;
}

