// anakin_amd/csrc/api_select.hip - which kernel a convolution launches: the selection record (ConvSel, api_internal.h) and the ONE function
// per concern that interprets it - eligibility, the on-demand buffers, the ABI code in both directions, the name, the kernel identity, the
// launch - and the list of candidates the autotuners time. A new kernel family is one enumerator and one case in each switch below.
#include "api_internal.h"

// ================================================================================================
// eligibility: the families an op's descriptor and packed weights admit
// ================================================================================================
// the depthwise 3x3 kernels exist for this op (conv_dw3x3.hip): group == c == k, 3x3, dilation 1, stride 1 | 2, pad 0 | 1, 8-bit NHWC in /
// NHWC out with C % 16 == 0 or f32 NHWC in / out with C % 4 == 0, no residual. A property of the descriptor: known at create
bool dw_ok(const saber_hip_conv* op) {
    const saber_hip_conv_desc& d = op->d;
    if (op->algo != ALGO_DIRECT_I8 && op->algo != ALGO_DIRECT_F32) return false;
    if (d.res_mode != SABER_HIP_RES_NONE || op->pre_quant || op->pre_pad || op->pre_transpose || d.out_layout != SABER_HIP_NHWC) return false;
    if (op->is_i8 && op->epi != EPI_I8_CONV) return false;
    return conv_dw3x3_ok(!op->is_i8, d.n, d.c, d.k, d.group, d.kh, d.kw, d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w, op->oh, op->ow);
}
// the grouped 3x3 INT8 kernels exist for this op (conv_group3x3.hip): group > 1, not depthwise, Cg == Kg in {4, 8, 16, 32, 64}, C % 64 == 0, 3x3,
// dilation 1, stride 1 | 2, pad 0 | 1, 8-bit NHWC in, NHWC s8 / u8 / f32 out, no residual. A property of the descriptor: known at create
bool group_ok(const saber_hip_conv* op) {
    const saber_hip_conv_desc& d = op->d;
    if (op->algo != ALGO_DIRECT_I8 || !op->is_i8 || op->epi != EPI_I8_CONV) return false;
    if (d.res_mode != SABER_HIP_RES_NONE || op->pre_quant || op->pre_pad || d.in_layout != SABER_HIP_NHWC || d.out_layout != SABER_HIP_NHWC) return false;
    if (d.in_dtype != SABER_HIP_S8 && d.in_dtype != SABER_HIP_U8) return false;
    return conv_group3x3_ok(d.n, d.c, d.k, d.group, d.kh, d.kw, d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w, op->oh, op->ow);
}
// the pointwise kernels (planes packed on demand by pw_prepare): 0 = the persistent register-weights kernel, 1 .. 4 = the reduction-split one
static bool pw_variant_ok(const saber_hip_conv* op, int variant) {
    if (!pw_eligible(op)) return false;
    if (variant == 0) return conv1x1_pw_ok(op->c_eff, op->d.k);
    int tm, p, dd, mb;
    return conv1x1_pwk_variant(variant, &tm, &p, &dd, &mb) && conv1x1_pwk_ok(op->d.n * op->d.h * op->d.w, op->c_eff, op->d.k) &&
           (op->c_eff >> 7) >= dd;      // (slabs in flight <= slabs per wave)
}
// (tile, stage depth) combinations of the bf16-plane kernels (planes uploaded by set_weights): depth 2 below 128 x 128; the 256-row tile
// reads 256 weight rows per workgroup without a row predicate, the planes are padded to multiples of 128 rows
bool b3_tile_ok(const saber_hip_conv* op, int tile, int ks) {
    if (op->algo != ALGO_IGEMM_F32 || !op->d_w3.p || tile < 0 || tile >= TILE_COUNT_B3 || (ks != 1 && ks != 2)) return false;
    if (ks == 2 && (tile == TILE_128x128 || tile >= TILE_W8_128x128)) return false;
    if (tile == TILE_W8_256x128 && ((op->d.k + 127) / 128) % 2 != 0) return false;
    return true;
}
static bool b3h_ok(const saber_hip_conv* op, int variant) {      // the halo variant exists for this op (planes packed by set_weights)
    int bmk, th, tm, thr;
    if (!conv3x3_b3h_variant(variant, &bmk, &th, &tm, &thr)) return false;
    if ((variant >= 6) != (op->d.kh == 1)) return false;       // 1..5: the 3x3 forms, 6..8: pointwise
    if (variant >= 6 && op->pool2) return false;
    return op->algo == ALGO_IGEMM_F32 && (tm == 1 ? op->d_w3h1.p : op->d_w3h2.p) != nullptr && !op->pair_k2;
}
bool fc_small_ok(const saber_hip_conv* op) {
    if (op->algo == ALGO_IGEMM_F32)   // FP32 fc: a 1x1 "conv" on a [m, 1, 1, k] NHWC tensor, plain f32 epilogue, no residual
        return op->epi == EPI_F32 && op->d.h == 1 && op->d.w == 1 && op->d.kh == 1 && op->d.kw == 1 && !op->pre_transpose &&
               op->d.out_layout == SABER_HIP_NHWC && op->d.res_mode == SABER_HIP_RES_NONE && !op->pair_k2 && !op->pool2 &&
               fc_f32_small_ok(op->d.n, op->c_eff, op->Kg_pad);
    return op->algo == ALGO_IGEMM_I8 && (op->epi == EPI_I8_FC_S8 || op->epi == EPI_I8_FC_U8) && op->d.h == 1 && op->d.w == 1 &&
           fc_i8_small_ok(op->d.n, op->c_eff, op->Kg_pad);
}
static bool halo_ok(const saber_hip_conv* op) {
    const saber_hip_conv_desc& d = op->d;
    return op->algo == ALGO_IGEMM_I8 && op->epi == EPI_I8_CONV && d.kh == 3 && d.kw == 3 && d.stride_h == 1 &&
           d.stride_w == 1 && d.dil_h == 1 && d.dil_w == 1 && d.group == 1 && op->c_eff % 64 == 0 && d.pad_h <= 1 &&
           d.pad_w <= 1;
}
bool stem_ok(const saber_hip_conv* op) {
    const saber_hip_conv_desc& d = op->d;
    return op->algo == ALGO_IGEMM_I8_C4 && op->epi == EPI_I8_CONV && d.kh == 7 && d.kw == 7 && d.stride_h == 2 &&
           d.stride_w == 2 && d.dil_h == 1 && d.dil_w == 1 && d.group == 1;
}
// FP32 split-K (b3 kernels): 2^sh workgroups per tile; needs >= 2 stages per split, a bounded partial buffer, and the
// workgroup -> XCD placement the hand-off relies on (checked once per device). split_prepare allocates the buffers.
static bool split_ok(const saber_hip_conv* op, int tile, int ks, int sh) {
    if (sh == 0) return true;
    if (sh < 0 || sh > 3 || !b3_tile_ok(op, tile, ks)) return false;
    if (op->no_placement) return false;      // a net that shares its device: the splits' common XCD is a dispatch property of an idle GPU
    const int steps = (op->Kg + 32 * ks - 1) / (32 * ks);
    if ((steps >> sh) < 2) return false;
    const size_t m = (size_t)op->d.n * op->oh * op->ow;
    if ((m + 127) * ((size_t)op->d.k + 127) * 4 * 8 > ((size_t)96 << 20)) return false;   // partial buffer: <= 96 MB
    return xcd_round_robin();
}
// the implicit-GEMM parameters name a kernel: wave groups (dma 2 / 4) need stage depth 4 and a tile <= 64x64 (32x32 for 4 groups), the
// NHWC4 first-layer path has the register-staged kernels only
static bool igemm_params_ok(const saber_hip_conv* op, const ConvSel& s) {
    if (s.tile < 0 || s.tile >= TILE_COUNT || (s.ks != 1 && s.ks != 2 && s.ks != 4)) return false;
    if (s.dma != 0 && s.dma != 1 && s.dma != 2 && s.dma != 4) return false;
    if (s.dma && op->algo == ALGO_IGEMM_I8_C4) return false;
    if (s.dma >= 2 && (s.ks != 4 || s.tile > TILE_64x64)) return false;
    return s.dma != 4 || s.tile == TILE_32x32;
}

bool sel_valid(const saber_hip_conv* op, const ConvSel& s) {
    switch (s.fam) {
    // (an op on the direct kernel carries implicit-GEMM parameters it never launches: get_tile has always answered them, and callers try
    // the same list of codes on every op, so they are kept to the same rule)
    case FAM_DIRECT: return op->algo > ALGO_IGEMM_F32 && igemm_params_ok(op, s);
    case FAM_IGEMM: return op->algo <= ALGO_IGEMM_F32 && igemm_params_ok(op, s);
    case FAM_B3: return s.dma == 0 && b3_tile_ok(op, s.tile, s.ks) && split_ok(op, s.tile, s.ks, s.ksplit);
    case FAM_STEM: return stem_ok(op);
    case FAM_HALO: return halo_ok(op) && !op->pair_k2 && (s.variant == 4 || s.variant == 8);
    case FAM_IMG: return halo_ok(op) && !op->pair_k2 && conv3x3_img_feasible(op->c_eff, op->ow, op->oh, op->d.n, s.img_nw, s.img_ib, s.img_rb);
    case FAM_IMG1: return img_conv_ok(op);
    case FAM_FC_SMALL: return fc_small_ok(op);
    case FAM_B3H: return b3h_ok(op, s.variant);
    case FAM_PW: return pw_variant_ok(op, s.variant);
    case FAM_DW: return dw_ok(op) && s.variant >= 1 && s.variant <= DW3X3_FORMS;
    case FAM_GROUP: return group_ok(op) && s.variant >= 1 && s.variant <= G3X3_FORMS;
    }
    return false;
}
static const char* sel_requirements(ConvFamily fam) {
    switch (fam) {
    case FAM_DIRECT:
    case FAM_IGEMM: return "implicit GEMM: tile 0..5, stage depth 1 / 2 / 4, staging 1..4 (register-staged only on the NHWC4 path); wave groups need "
                           "stage depth 4 and a tile <= 64x64 (32x32 for 4 groups)";
    case FAM_B3: return "bf16x3: FP32 implicit-GEMM conv with C % 8 == 0 (not an fc), tile 0..9, stage depth 1 (or 2 below 128x128), 256x128 only for k "
                        "padded to a multiple of 256; split-K: 2 / 4 / 8 splits with >= 2 stages each, bounded output, 8 x 32 CU device";
    case FAM_STEM: return "stem kernel needs an INT8 7x7 stride-2 conv with <= 4 channels";
    case FAM_HALO: return "halo kernel needs an INT8 3x3 stride-1 conv with C % 64 == 0";
    case FAM_IMG: return "small-image 3x3 kernel: needs an INT8 3x3 stride-1 conv with C in {64,128,256,512} and a slab (images x rows) that fits its "
                         "LDS / accumulator budget";
    case FAM_IMG1: return "image-resident kernel: 1x1 / 3x3 stride-1 INT8 conv on <= 64 pixels per image with ResNet res5 channel shapes";
    case FAM_FC_SMALL: return "small-batch fc kernel: INT8 fc with <= 16 rows and k <= 4096";
    case FAM_B3H: return "bf16x3 halo kernel: FP32 NHWC stride-1 conv, 3x3 pad 1 with C % 32 == 0 (variant 1..5) or 1x1 with C % 64 == 0 (6..8)";
    case FAM_PW: return "pointwise kernels: FP32 NHWC 1x1 / stride-1 conv, K % 64 == 0, C in {64, 128} (variant 0) or C % 128 == 0 (1..4)";
    case FAM_DW: return "depthwise 3x3 kernels: group == c == k, 3x3, dilation 1, stride 1 | 2, pad 0 | 1, NHWC 8-bit (C % 16 == 0) or f32 (C % 4 == 0) "
                        "tensors, no residual; low byte 0 (direct kernel) .. 2";
    case FAM_GROUP: return "grouped 3x3 kernels: INT8, group > 1 with Cg == Kg in {4, 8, 16, 32, 64}, C % 64 == 0, 3x3, dilation 1, stride 1 | 2, pad 0 | 1, "
                           "NHWC 8-bit input, NHWC s8 / u8 / f32 output, no residual; low byte 0 (direct kernel) | 1";
    }
    return "";
}

// the buffers a family reads that are made on demand (everything else is packed by set_weights)
static int sel_prepare(saber_hip_conv* op, const ConvSel& s) {
    switch (s.fam) {
    case FAM_B3: return s.ksplit ? split_prepare(op) : SABER_HIP_OK;
    case FAM_IMG1: return img_conv_prepare(op);
    case FAM_PW: return pw_prepare(op);
    default: return SABER_HIP_OK;
    }
}
// ... and what only ONE family reads, released once another is selected: the split-K partial buffers (up to 96 MB), the fragment-ordered
// bf16 planes of the FP32 halo / pointwise kernels (2 x 1.5 x the f32 weights: > 200 MB over VGG16), the fc's fragment-major copy and the
// image-resident kernel's stage. (d_w and the bf16 planes d_w3 stay: the net-level consolidation pass still switches implicit-GEMM tiles.
// A later set_tile to the released halo family reports INVALID_VALUE; the on-demand buffers of sel_prepare are packed again.)
void sel_release_unused(saber_hip_conv* op) {
    const ConvSel& s = op->sel;
    if (s.fam != FAM_B3 || !s.ksplit) {
        op->d_part.release();
        op->d_part_ctr.release();
    }
    if (s.fam != FAM_B3H) {
        op->d_w3h1.release();
        op->d_w3h2.release();
    }
    if (s.fam != FAM_PW) op->d_wpw.release();
    if (s.fam != FAM_FC_SMALL) op->d_wfc.release();
    if (s.fam != FAM_IMG1) img_conv_release(op);
}

// The one writer of op->sel. An op with fused global pooling (saber_hip_conv2d_set_global_pooling) exists only as the image-resident kernel.
int sel_set(saber_hip_conv* op, const ConvSel& s) {
    if (op->gpool && s.fam != FAM_IMG1) return fail(SABER_HIP_INVALID_VALUE, "conv + fused global pooling has a single kernel");
    if (!sel_valid(op, s)) return fail(SABER_HIP_INVALID_VALUE, sel_requirements(s.fam));
    const int rc = sel_prepare(op, s);
    if (rc) return rc;
    op->sel = s;
    sel_name(op);
    return SABER_HIP_OK;
}

// ================================================================================================
// the ABI code of saber_hip_conv2d_get_tile / set_tile: low byte | bits 8..15 | variant byte
//    0         tile | stage depth (0: keep): the family stays, its implicit-GEMM parameters change
//    1 .. 4    tile | stage depth (0: keep): implicit GEMM, register-staged / LDS-DMA ring / ring with 2 / 4 wave groups
//    5, 6      LDS-halo 3x3 kernel with 4 / 8 tile rows; tile | stage depth as get_tile reports them (stage depth 0: keep both)
//    7, 8      stem kernel on / off; 8 may carry a tile | stage depth for the implicit GEMM it returns to
//    9         small-image 3x3 kernel: output rows per slab | images per slab, bit 15: 8 waves per workgroup
//    10        small-batch fc kernel
//    11        bf16-plane implicit GEMM: tile 0..9 | stage depth (0: 1) in bits 8..11, log2 of the split-K factor in bits 12..15
//    12        image-resident kernel
//    13        bf16-plane LDS-halo kernel, variant 1..8 in the low byte
//    14        pointwise kernels: 0 = register weights, 1 .. 4 = the reduction-split variants
//    15        FP32 stem launch (a property of the fused conv + pooling op, not a selection: saber_hip_conv2d_set_tile)
//    16        depthwise 3x3: 0 = the direct kernel, 1 .. DW3X3_FORMS = the forms of conv_dw3x3.hip
//    17        INT8 grouped 3x3 (Cg == Kg): 0 = the direct kernel, 1 .. G3X3_FORMS = the forms of conv_group3x3.hip
// ================================================================================================
int sel_encode(const saber_hip_conv* op) {
    const ConvSel& s = op->sel;
    if (dw_ok(op)) return (16 << 16) | (s.fam == FAM_DW ? s.variant : 0);      // (an eligible op always answers in this encoding)
    if (group_ok(op)) return (17 << 16) | (s.fam == FAM_GROUP ? s.variant : 0);      // (likewise)
    switch (s.fam) {
    case FAM_PW: return (14 << 16) | s.variant;
    case FAM_B3H: return (13 << 16) | s.variant;
    case FAM_IMG1: return 12 << 16;
    case FAM_B3: return s.tile | ((s.ks | (s.ksplit << 4)) << 8) | (11 << 16);
    case FAM_FC_SMALL: return 10 << 16;
    case FAM_IMG: return s.img_rb | ((s.img_ib | (s.img_nw == 8 ? 0x80 : 0)) << 8) | (9 << 16);
    case FAM_STEM: return 7 << 16;
    case FAM_HALO: return s.tile | (s.ks << 8) | ((s.variant == 4 ? 5 : 6) << 16);
    case FAM_DW:
    case FAM_GROUP:
    case FAM_DIRECT:
    case FAM_IGEMM: break;
    }
    return s.tile | (s.ks << 8) | ((s.dma == 0 ? 1 : (s.dma == 1 ? 2 : (s.dma == 2 ? 3 : 4))) << 16);
}
int sel_decode(const saber_hip_conv* op, int code, ConvSel* out) {
    const ConvSel& cur = op->sel;
    const int low = code & 0xff, ks = (code >> 8) & 0xff, var = (code >> 16) & 0xff;
    const bool depth = ks == 1 || ks == 2 || ks == 4;
    if (op->gpool && var != 8 && var != 12) return fail(SABER_HIP_INVALID_VALUE, "conv + fused global pooling has a single kernel");
    ConvSel base = cur;      // the implicit-GEMM parameters the code carries, on top of the current ones
    switch (var) {
    case 0: case 1: case 2: case 3: case 4:
        if (low >= TILE_COUNT || (ks && !depth)) return fail(SABER_HIP_INVALID_VALUE, "bad tile id");
        base.tile = low;
        if (ks) base.ks = ks;
        if (var) base.dma = var == 1 ? 0 : (var == 2 ? 1 : (var == 3 ? 2 : 4));
        *out = var == 0 ? base : (op->algo <= ALGO_IGEMM_F32 ? sel_igemm(base, base.tile, base.ks, base.dma) : sel_direct(base));
        return SABER_HIP_OK;
    case 5: case 6:
        if (depth && low < TILE_COUNT) { base.tile = low; base.ks = ks; }
        *out = sel_halo(base, var == 5 ? 4 : 8);
        return SABER_HIP_OK;
    case 7: *out = sel_stem(cur); return SABER_HIP_OK;
    case 8:      // the family stays unless it is the stem kernel
        if (low < TILE_COUNT) base.tile = low;
        if (depth) base.ks = ks;
        *out = cur.fam == FAM_STEM ? sel_igemm(base, base.tile, base.ks, base.dma) : base;
        return SABER_HIP_OK;
    case 9: *out = sel_img(cur, (ks & 0x80) ? 8 : 4, ks & 0x7f, low); return SABER_HIP_OK;
    case 10: *out = sel_fc_small(cur); return SABER_HIP_OK;
    case 11: *out = sel_b3(cur, low, (ks & 15) ? (ks & 15) : 1, ks >> 4); return SABER_HIP_OK;
    case 12: *out = sel_img1(cur); return SABER_HIP_OK;
    case 13: *out = sel_b3h(cur, low); return SABER_HIP_OK;
    case 14: *out = sel_pw(cur, low); return SABER_HIP_OK;
    case 16:
        if (!dw_ok(op) || low > DW3X3_FORMS) return fail(SABER_HIP_INVALID_VALUE, sel_requirements(FAM_DW));
        *out = low ? sel_dw(cur, low) : sel_direct(cur);
        return SABER_HIP_OK;
    case 17:
        if (!group_ok(op) || low > G3X3_FORMS) return fail(SABER_HIP_INVALID_VALUE, sel_requirements(FAM_GROUP));
        *out = low ? sel_group(cur, low) : sel_direct(cur);
        return SABER_HIP_OK;
    default: return fail(SABER_HIP_INVALID_VALUE, "bad staging variant");
    }
}

int saber_hip_conv2d_set_tile(saber_hip_conv_t* op, int tile) {
    if (op->stem32) {      // FP32 stem launch: variant 15, low byte 0 = tile by launch size, 1 = 8 x 8 pooled pixels per workgroup, 2 = 4 x 8, 3 = 4 x 4
        if (((tile >> 16) & 0xff) != 15 || (tile & 0xff) > 3) return fail(SABER_HIP_INVALID_VALUE, "FP32 stem launch: (15 << 16) | 0..3");
        op->stem32 = 1 + (tile & 0xff);
        return SABER_HIP_OK;
    }
    if (op->pool_fused) return fail(SABER_HIP_INVALID_VALUE, "fused conv+pooling has a single kernel");
    ConvSel s;
    const int rc = sel_decode(op, tile, &s);
    return rc ? rc : sel_set(op, s);      // a refused code changes nothing
}
int saber_hip_conv2d_get_tile(const saber_hip_conv_t* op) { return sel_encode(op); }

// ================================================================================================
// name, kernel identity, launch
// ================================================================================================
void sel_name(saber_hip_conv* op) {
    static const char* an[] = {"igemm_i8", "igemm_i8_c4", "igemm_f32", "direct_i8", "direct_f32"};
    const ConvSel& s = op->sel;
    const saber_hip_conv_desc& d = op->d;
    const char* sum = d.res_mode == SABER_HIP_RES_SUM_INPLACE ? "+sum" : "";
    int bmk = 0, bnp = 0;      // the kernel's block: output channels x pixels (tile rows / pixel tiles for the LDS-halo forms)
    int tm = 0, thr = 0, depth = 0, wgs = 0;
    char buf[96];
    if (op->stem32) snprintf(buf, sizeof buf, "stem7x7s2_maxpool3x3s2_f32_bf16x3_nchw_in");
    else if (op->pool_fused) snprintf(buf, sizeof buf, "stem7x7s2_maxpool3x3s2_i8_4x8%s", op->pre_quant ? "_fusedquant" : "");
    else switch (s.fam) {
    case FAM_STEM: snprintf(buf, sizeof buf, "stem7x7s2_i8_8x16%s", op->pre_quant ? "_fusedquant" : ""); break;
    case FAM_FC_SMALL:
        snprintf(buf, sizeof buf, op->algo == ALGO_IGEMM_F32 ? ((op->d_fcpart.p && !op->d_wfc.p) ? "fc_f32_splitk_16xk4" : "fc_f32_small_16xk4") : "fc_i8_small_16xk4");
        break;
    case FAM_PW:
        if (s.variant) {
            (void)conv1x1_pwk_variant(s.variant, &tm, &bnp, &depth, &wgs);      // row tiles, pixel tiles, slabs in flight, workgroups per block
            snprintf(buf, sizeof buf, "pw1x1_f32_bf16x3_ksplit4_%dch_%dpx_d%d%s%s", tm * 16, bnp * 16, depth, wgs > 1 ? "_2wg" : "", sum);
        } else snprintf(buf, sizeof buf, "pw1x1_f32_bf16x3_regs_c%d_%dch_per_wave%s", op->c_eff, op->c_eff == 64 ? 64 : 32, sum);
        break;
    case FAM_B3H:
        (void)conv3x3_b3h_variant(s.variant, &bmk, &bnp, &tm, &thr);      // channels, tile rows / pixel tiles, row tiles per wave, threads
        if (s.variant >= 6) snprintf(buf, sizeof buf, "pw1x1_f32_bf16x3_%dch_%dpx_w%d", bmk, bnp * 16, thr / 64);
        else snprintf(buf, sizeof buf, "halo3x3_f32_bf16x3_%dch_%dx16_w%d%s", bmk, bnp, thr / 64, op->pool2 ? "+maxpool2x2" : "");
        break;
    case FAM_IMG1: snprintf(buf, sizeof buf, "imgres%dx%d_i8_%dch%s", d.kh, d.kw, 16 * ((d.k / 16 + 31) / 32), op->gpool ? "+gpool" : ""); break;
    case FAM_IMG: snprintf(buf, sizeof buf, "img3x3_i8_%dimg_x_%drows_k16_w%d", s.img_ib, s.img_rb, s.img_nw); break;
    case FAM_HALO: snprintf(buf, sizeof buf, "halo3x3_i8_%dx16", s.variant); break;
    case FAM_DW: snprintf(buf, sizeof buf, "dw3x3_%s_%s", op->is_i8 ? "i8" : "f32", conv_dw3x3_form_name(s.variant, !op->is_i8)); break;
    case FAM_GROUP: snprintf(buf, sizeof buf, "g3x3_i8_%s", conv_group3x3_form_name(s.variant)); break;
    case FAM_DIRECT: snprintf(buf, sizeof buf, "%s", an[op->algo]); break;
    case FAM_B3:
    case FAM_IGEMM: {
        const bool b3 = s.fam == FAM_B3;
        tile_dims(s.tile, &bmk, &bnp);
        snprintf(buf, sizeof buf, "%s_%dx%d_k%d%s%s%s%s", b3 ? "igemm_f32_bf16x3" : an[op->algo], bmk, bnp, s.ks,
                 b3 && s.tile >= TILE_W8_64x64 ? "_w8" : "",
                 b3 && s.ksplit ? (s.ksplit == 1 ? "_split2" : (s.ksplit == 2 ? "_split4" : "_split8")) : "",
                 s.dma == 0 ? "" : (s.dma == 1 ? "_dma" : (s.dma == 2 ? "_dma_wg2" : "_dma_wg4")),
                 op->pool2 ? "+maxpool2x2" : "");
        break;
    }
    }
    op->algo_name = std::string(op->pair_k2 ? "pair_" : "") + buf;
}

// one value per kernel FUNCTION a selection launches (g_used_kernels, net_consolidate_kernels): bits 0..7 the algorithm and epilogue class,
// bits 8..15 the family (5 / 6: the implicit-GEMM tile kernels), above that what the family's template is instantiated on
unsigned long long sel_kernel_key(const saber_hip_conv* op, const ConvSel& s) {
    typedef unsigned long long u64;
    const saber_hip_conv_desc& d = op->d;
    int ek = 3;   // conv_igemm.hip: epilogue_kind
    if (op->pair_k2) ek = 4;
    else if (op->algo != ALGO_IGEMM_F32 && op->epi == EPI_I8_CONV && d.res_mode != SABER_HIP_RES_SUM_INPLACE && d.k % 16 == 0)
        ek = d.res_mode == SABER_HIP_RES_ELTWISE ? 2 : (d.out_dtype == SABER_HIP_U8 ? 1 : (d.out_dtype == SABER_HIP_S8 ? 0 : 3));
    const u64 k = (u64)op->algo | ((u64)ek << 4), sum = (u64)(d.res_mode == SABER_HIP_RES_SUM_INPLACE) << 32;
    switch (s.fam) {
    case FAM_DW: return k | (11ull << 8) | ((u64)s.variant << 16) | ((u64)(d.stride_h == 2) << 24) | ((u64)(d.in_dtype == SABER_HIP_U8) << 25);
    case FAM_GROUP: {      // <CGC, U8, PT>: channel class, input type, form (and the stride, a run-time argument, as the depthwise key has it)
        const int cg = d.c / d.group;
        return k | (12ull << 8) | ((u64)s.variant << 16) | ((u64)(d.stride_h == 2) << 24) | ((u64)(d.in_dtype == SABER_HIP_U8) << 25) |
               ((u64)(cg <= 16 ? 0 : (cg == 32 ? 1 : 2)) << 26);
    }
    case FAM_PW: return s.variant ? k | (10ull << 8) | ((u64)(s.variant + 1) << 16) | sum : k | (9ull << 8) | ((u64)op->c_eff << 16) | sum;
    case FAM_B3H: return k | (8ull << 8) | ((u64)s.variant << 16);
    case FAM_IMG1: return k | (7ull << 8) | ((u64)(d.kh == 3) << 16);      // one function for all image-resident shapes
    case FAM_FC_SMALL: return k | (1ull << 8) | ((u64)((op->c_eff + 255) / 256) << 16);
    case FAM_STEM: return k | (2ull << 8);
    case FAM_IMG:   // <EK, NW, CW, NCH, GPW>: channel count and pixel groups per wave
        return k | (3ull << 8) | ((u64)op->c_eff << 16) | ((u64)((s.img_ib * s.img_rb * op->ow + 15) / 16) << 32);
    case FAM_HALO: return k | (4ull << 8) | ((u64)s.variant << 16) | ((u64)(op->c_eff % 128 == 0) << 24);
    case FAM_DIRECT:
    case FAM_IGEMM:
    case FAM_B3: break;
    }
    return k | ((s.fam == FAM_B3 ? 6ull : 5ull) << 8) | ((u64)s.tile << 16) | ((u64)s.ks << 24) | ((u64)s.dma << 32);
}

// A split-K launch of this operator found its splits on different XCDs (the kernel poisoned that output with NaN and counted
// itself in the pinned word): report it as an error status NOW and run without split-K from here on.
static int split_check(saber_hip_conv* op) {
    if (!op->h_part_err || !*(volatile unsigned*)op->h_part_err) return SABER_HIP_OK;
    *(volatile unsigned*)op->h_part_err = 0u;
    (void)sel_set(op, sel_b3(op->sel, op->sel.tile, op->sel.ks, 0));
    return fail(SABER_HIP_RUNTIME_ERROR, "FP32 split-K: in an earlier launch of this operator the splits of a tile ran on different XCDs "
                "(that output was poisoned with NaN); split-K is now off for it");
}
// enqueues the selected kernel on the filled argument block (saber_hip_conv2d_run / run_pair, after their pre-passes and early exits)
int sel_launch(saber_hip_conv* op, ConvKArgs& a, hipStream_t s) {
    const ConvSel& c = op->sel;
    const int mode = op->algo == ALGO_IGEMM_I8 ? 0 : (op->algo == ALGO_IGEMM_I8_C4 ? 1 : 2);      // conv_igemm.hip: 3 = the bf16 planes
    switch (c.fam) {
    case FAM_IGEMM:
        HIP_TRY(c.dma ? launch_conv_igemm_dma(mode, c.tile, c.ks, c.dma, a, s) : launch_conv_igemm(mode, c.tile, c.ks, a, s));
        break;
    case FAM_B3:
        if (c.ksplit && !op->d_part.p) return fail(SABER_HIP_INVALID_VALUE, "split-K selected without its buffers (saber_hip_conv2d_set_tile / autotune allocate them)");
        if (c.ksplit) {
            const int rs = split_check(op);
            if (rs) return rs;
        }
        HIP_TRY(launch_conv_igemm(3, c.tile, c.ks, a, s));
        break;
    case FAM_STEM: HIP_TRY(launch_conv_stem(0, a, s)); break;
    case FAM_HALO: HIP_TRY(launch_conv3x3_halo(c.variant, a, s)); break;
    case FAM_IMG: HIP_TRY(launch_conv3x3_img(a, c.img_nw, c.img_ib, c.img_rb, s)); break;
    case FAM_IMG1: return img_conv_run(op, a.x, a.y, a.res, nullptr, s);
    case FAM_FC_SMALL:
        if (op->algo == ALGO_IGEMM_I8) HIP_TRY(launch_fc_i8_small(a, s));
        else if (op->d_fcpart.p && !op->d_wfc.p) HIP_TRY(launch_fc_f32_splitk(a, op->d_fcpart.p, op->d_fcctr.p, nullptr, s));      // few output tiles: the reduction split over workgroups (fc_f32_splitk.hip)
        else {
            if (op->d_wfc.p) a.w = op->d_wfc.p;
            HIP_TRY(launch_fc_f32_small(a, op->d_wfc.p != nullptr, s));
        }
        break;
    case FAM_PW:
        a.w = op->d_wpw.p;
        if (c.variant) HIP_TRY(launch_conv1x1_pwk(c.variant, a, s));
        else HIP_TRY(launch_conv1x1_pw(a, s));
        break;
    case FAM_B3H: {
        int hb, ht, htm, hthr;
        (void)conv3x3_b3h_variant(c.variant, &hb, &ht, &htm, &hthr);
        a.w = htm == 1 ? op->d_w3h1.p : op->d_w3h2.p;
        HIP_TRY(launch_conv3x3_b3h(c.variant, a, s));
        break;
    }
    case FAM_DW:
        if (!dw_ok(op) || !op->d_wdw.p) return fail(SABER_HIP_INVALID_VALUE, "depthwise kernel selected on an op without its [tap][C] weights");
        a.w = op->d_wdw.p;
        HIP_TRY(launch_conv_dw3x3(c.variant, !op->is_i8, a, s));
        break;
    case FAM_GROUP:
        if (!group_ok(op) || !op->d_wg.p || (a.in_u8 && !a.comp)) return fail(SABER_HIP_INVALID_VALUE, "grouped 3x3 kernel selected on an op without its fragment-ordered weights");
        a.w = op->d_wg.p;
        HIP_TRY(launch_conv_group3x3(c.variant, a, op->d.group, s));
        break;
    case FAM_DIRECT:
        a.comp = nullptr;
        HIP_TRY(launch_conv_direct(op->is_i8 ? 0 : 1, a, op->d.group, s));
        break;
    }
    return SABER_HIP_OK;
}

// ================================================================================================
// what the autotuners time, in order (the first of equally fast candidates wins, the kernel-reuse preference walks the list in order)
// ================================================================================================
// `best` is the caller's running best selection (updated by fn): the kernels that replace the implicit GEMM for special shapes are offered
// with the fastest implicit GEMM's parameters underneath, which get_tile reports and variant 8 returns to. A sibling pair runs the
// implicit-GEMM kernels only.
void for_each_candidate(const saber_hip_conv* op, const ConvSel* best, const std::function<void(const ConvSel&)>& fn) {
    const ConvSel entry = op->sel;
    if (dw_ok(op)) {      // depthwise 3x3: the direct kernel and every form of conv_dw3x3.hip
        fn(sel_direct(entry));
        for (int f = 1; f <= DW3X3_FORMS; ++f) fn(sel_dw(entry, f));
        return;
    }
    if (group_ok(op)) {      // INT8 grouped 3x3: the direct kernel and every form of conv_group3x3.hip
        fn(sel_direct(entry));
        for (int f = 1; f <= G3X3_FORMS; ++f) fn(sel_group(entry, f));
        return;
    }
    ConvSel last = entry;
    auto offer = [&](const ConvSel& s) {
        if (!sel_valid(op, s)) return;
        last = s;
        fn(s);
    };
    for (int dma : {0, 1, 2, 4})
        for (int t = 0; t < TILE_COUNT; ++t)
            for (int ks : {1, 2, 4}) offer(sel_igemm(entry, t, ks, dma));
    // FP32 on the bf16 matrix cores: every tile (6..9: the 8-wave forms of 64x64, 128x64, 128x128 and 256x128); deep reductions on few
    // pixels also as 2 / 4 / 8 workgroups per tile (split-K inside one XCD) while the grid stays <= 2048: beyond, the unsplit grid fills the CUs
    for (int kd = 1; kd <= 2; ++kd)
        for (int t = 0; t < TILE_COUNT_B3; ++t)
            for (int sh = 0; sh <= 3; ++sh) {
                int bmk, bnp;
                tile_dims(t, &bmk, &bnp);
                const long tiles = (long)((op->d.n * op->oh * op->ow + bnp - 1) / bnp) * ((op->d.k + bmk - 1) / bmk);
                if (!sh || (tiles << sh) <= 2048) offer(sel_b3(entry, t, kd, sh));
            }
    if (op->pair_k2) return;
    last.ks = 1;
    last.dma = 0;
    for (int v = 1; v <= 8; ++v) offer(sel_b3h(last, v));      // FP32 3x3: the LDS-halo forms of the bf16-plane kernel; 1x1: its pointwise forms (6..8)
    for (int v = 0; v <= 4; ++v) offer(sel_pw(last, v));       // FP32 1x1: register weights (C = 64 / 128), the reduction split over the waves (C = 128 .. 2048)
    const ConvSel base = *best;
    offer(sel_fc_small(base));
    offer(sel_stem(base));
    offer(sel_img1(base));      // <= 64 pixels per image
    for (int rows = 4; rows <= 8; rows += 4) offer(sel_halo(base, rows));
    for (int ib : {1, 2, 4})      // small-image kernel: every feasible (images, rows) slab
        for (int rb : {1, 2, 3, 4, 7, 8, 14}) offer(sel_img(base, 4, ib, rb));
}
