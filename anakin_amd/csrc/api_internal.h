// anakin_amd/csrc/api_internal.h - what the translation units behind include/saber_hip.h share: error reporting, device
// buffers, the operator structs behind the opaque handles, the kernel-selection record, the autotuners' timing loop, and the
// op-list executor's structs. Nothing here is part of the ABI (the entry points get their C linkage from saber_hip.h).
//   api_conv.hip          convolution: create / set_weights (quantise + repack) / run, sibling pairs
//   api_select.hip        kernel selection of a convolution: eligibility, set_tile / get_tile codes, name, launch, autotune candidates
//   api_autotune.hip      per-op and per-pair autotuner (cold-L2 timing loop, kernel-reuse preference)
//   api_ops.hip           fc, INT8 / FP32 GEMM, the streaming operators' wrappers
//   api_chain.hip         conv1x1 chains (two / three convs in one launch): the table of launch forms, stream repacking, create / run
//   api_ir.hip            inverted-residual blocks (1x1 expand + depthwise 3x3 + 1x1 project in one launch): eligibility, repacking, create / run
//   api_sep.hip           separable pairs (depthwise 3x3 + pointwise 1x1 in one launch): eligibility, repacking, create / run
//   api_net.hip           op-list executor: arena, lanes, hipGraph capture / replay, in-pass timing
//   api_net_optimize.hip  executor-level fusions (saber_hip_net_optimize)
//   api_net_autotune.hip  whole-net autotuner, selection save / restore
//   api_gemm.hip          FP32 GEMM on the bf16-plane kernels (device-side plane split, per-thread plan cache)
//   api_deconv.hip        transposed convolution (FP32): create / set_weights (repack + fragment stream) / run, its forms and static rule
//   api_resize.hip        resize (FP32): create (the host index / fraction tables) / run / run_sum, its forms and static rule
//   api_detout.hip        DetectionOutput (FP32): create / run (the op's scratch), its forms and static rule
//   api_capture.hip       op-list capture: the *_run calls of a caller's own op loop recorded into a saber_hip_net
#pragma once
#include "../../include/saber_hip.h"
#include "kernels.h"

#include <cmath>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <type_traits>
#include <vector>

using namespace saber_mi355x;

namespace saber_api {

extern thread_local std::string g_err;      // defined in api_conv.hip; saber_hip_last_error reads it
inline int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
inline int hip_fail(hipError_t e, const char* where) {
    g_err = std::string(where) + ": " + hipGetErrorString(e);
    return SABER_HIP_RUNTIME_ERROR;
}
#define HIP_TRY(expr)                                    \
    do {                                                 \
        hipError_t _e = (expr);                          \
        if (_e != hipSuccess) return hip_fail(_e, #expr); \
    } while (0)

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline int conv_out(int in, int pad, int k, int dil, int stride) {
    return (in + 2 * pad - (dil * (k - 1) + 1)) / stride + 1;  // funcs_utils.h:29-53
}

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t upload(const std::vector<T>& h) {
        release();
        if (h.empty()) return hipSuccess;
        hipError_t e = hipMalloc((void**)&p, h.size() * sizeof(T));
        if (e != hipSuccess) return e;
        n = h.size();
        return hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t alloc_zero(size_t count) {
        release();
        hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e != hipSuccess) return e;
        n = count;
        e = hipMemset(p, 0, count * sizeof(T));
        return e != hipSuccess ? e : hipStreamSynchronize(nullptr);
    }
};

// 256 zero bytes in device memory per device, shared by every op created on it (padded taps of the LDS-DMA kernels).
// One page per device (an op on a second GPU must not DMA from the first one's memory), created under a lock, and
// the memset is complete before any kernel on a non-blocking stream can read it.
void* zero_page();      // api_conv.hip

enum Algo { ALGO_IGEMM_I8 = 0, ALGO_IGEMM_I8_C4 = 1, ALGO_IGEMM_F32 = 2, ALGO_DIRECT_I8 = 3, ALGO_DIRECT_F32 = 4 };

// Which kernel a convolution launches: exactly ONE family, its parameters, and the implicit-GEMM parameters underneath. Everything that
// interprets it is in api_select.hip; values are made by the sel_* constructors below and reach an op through sel_set alone.
enum ConvFamily {
    FAM_DIRECT,      // direct kernel (grouped convs, channel counts off the implicit-GEMM path)
    FAM_IGEMM,       // implicit GEMM on the i8 / f32 matrix cores: tile, ks, dma
    FAM_B3,          // FP32 implicit GEMM on three bf16 operand planes (conv_igemm_impl.h MODE 3, planes d_w3): tile 0..9, ks 1 | 2, ksplit
    FAM_STEM,        // INT8 first layer: LDS-patch stem kernel (conv_stem.h) instead of the NHWC4 implicit GEMM
    FAM_HALO,        // INT8 3x3: LDS-halo kernel (conv3x3_halo.h), variant = tile rows (4 / 8)
    FAM_IMG,         // INT8 3x3 on small images (conv3x3_img.h): img_ib images x img_rb output rows per workgroup slab, img_nw waves (4 / 8)
    FAM_IMG1,        // INT8, <= 64 pixels per image: image-resident kernel (stage_xcd.hip: img_conv_kernel), workgroup = one image x 16 NT channels
    FAM_FC_SMALL,    // small-batch fc kernel (fc_small.hip)
    FAM_B3H,         // FP32: LDS-halo bf16-plane kernel (conv3x3_b3h.hip, planes d_w3h1 / d_w3h2), variant 1..5 = 3x3 forms, 6..8 = pointwise
    FAM_PW,          // FP32 1x1 / stride 1 (planes d_wpw): variant 0 = persistent register-weights kernel (C = 64 / 128, conv1x1_pw.hip),
                     // 1 .. 4 = the reduction-split kernel's variants (C = 128 .. 2048, conv1x1_pwk.hip)
    FAM_DW,          // depthwise 3x3 (dw_ok): variant 1 .. DW3X3_FORMS = that form of conv_dw3x3.hip (weights d_wdw)
    FAM_GROUP        // INT8 grouped 3x3 with Cg == Kg (group_ok): variant 1 .. G3X3_FORMS = that form of conv_group3x3.hip (weights d_wg, d_comp)
};
struct ConvSel {
    ConvFamily fam = FAM_DIRECT;
    // the implicit-GEMM parameters. They survive while another family is selected: get_tile reports them for a halo op, set_tile variant 8
    // returns to them, the net-level consolidation pass swaps them
    int tile = TILE_64x64;
    int ks = 1;              // 64-byte k-steps per pipeline stage (1, 2, 4)
    int dma = 0;             // 0: register-staged kernel; 1/2/4: LDS-DMA ring kernel with that many wave groups
    int variant = 0;         // family-specific, see ConvFamily
    int ksplit = 0;          // FAM_B3: log2 of the split-K factor (conv_igemm_impl.h: splits of one tile share an XCD), 0: none
    int img_ib = 0, img_rb = 0, img_nw = 4;   // FAM_IMG
};
inline ConvSel sel_family(ConvSel base, ConvFamily fam, int variant = 0) {      // `base`: where the implicit-GEMM parameters come from
    base.fam = fam; base.variant = variant; base.ksplit = 0; base.img_ib = base.img_rb = 0; base.img_nw = 4;
    return base;
}
inline ConvSel sel_direct(const ConvSel& base) { return sel_family(base, FAM_DIRECT); }
inline ConvSel sel_igemm(const ConvSel& base, int tile, int ks, int dma) {
    ConvSel s = sel_family(base, FAM_IGEMM);
    s.tile = tile; s.ks = ks; s.dma = dma;
    return s;
}
inline ConvSel sel_b3(const ConvSel& base, int tile, int ks, int ksplit) {      // (register-staged, one 32-deep slab per k-step)
    ConvSel s = sel_family(base, FAM_B3);
    s.tile = tile; s.ks = ks; s.dma = 0; s.ksplit = ksplit;
    return s;
}
inline ConvSel sel_stem(const ConvSel& base) { return sel_family(base, FAM_STEM); }
inline ConvSel sel_halo(const ConvSel& base, int rows) { return sel_family(base, FAM_HALO, rows); }
inline ConvSel sel_img(const ConvSel& base, int nw, int ib, int rb) {
    ConvSel s = sel_family(base, FAM_IMG);
    s.img_nw = nw; s.img_ib = ib; s.img_rb = rb;
    return s;
}
inline ConvSel sel_img1(const ConvSel& base) { return sel_family(base, FAM_IMG1); }
inline ConvSel sel_fc_small(const ConvSel& base) { return sel_family(base, FAM_FC_SMALL); }
inline ConvSel sel_b3h(ConvSel base, int variant) { base.dma = 0; return sel_family(base, FAM_B3H, variant); }
inline ConvSel sel_pw(ConvSel base, int variant) { base.dma = 0; return sel_family(base, FAM_PW, variant); }
inline ConvSel sel_dw(const ConvSel& base, int form) { return sel_family(base, FAM_DW, form); }
inline ConvSel sel_group(const ConvSel& base, int form) { return sel_family(base, FAM_GROUP, form); }

}  // namespace saber_api
using namespace saber_api;

struct saber_hip_conv {
    saber_hip_conv_desc d;
    int oh = 0, ow = 0;
    int algo = ALGO_DIRECT_I8;
    ConvSel sel;             // the selected kernel (written by sel_set only)
    int pool_fused = 0, pool_oh = 0, pool_ow = 0;   // SaberConv2DPooling: fused stem conv + 3x3/2 max pooling
    int pool2 = 0;           // SaberConv2DPooling, FP32: relu'd implicit-GEMM conv + 2x2/2 max pooling in the epilogue
    int stem32 = 0;          // SaberConv2DPooling, FP32 stem (with pool_fused): NCHW image -> 7x7/2 conv + relu + 3x3/2 max pooling in ONE launch
                             // (conv_stem_f32.hip); d_wstem32 = its weight planes in MFMA fragment order, packed by set_pooling from w_stem_host
    DevBuf<uint8_t> d_wstem32;
    std::vector<float> w_stem_host;   // the OIHW f32 weights of a 3 -> 64 7x7 FP32 conv as handed to set_weights (9.4 K floats)
    DevBuf<uint8_t> d_w3h1, d_w3h2;   // FAM_B3H: the weight planes in MFMA fragment order for 1 / 2 row tiles per wave
    DevBuf<uint8_t> d_wpw;   // FAM_PW: the weight planes in that kernel's fragment order
    DevBuf<uint8_t> d_wdw;   // FAM_DW: the weights as [tap][C] (s8 / f32), packed by set_weights
    DevBuf<uint8_t> d_wg;    // FAM_GROUP: the weights in MFMA fragment order (group3x3_pack), packed by set_weights together with d_comp
    DevBuf<float> d_fcpart;  // FP32 fc at <= 16 rows and <= 2048 outputs: the split-K kernel's partial sums + arrival counters (fc_f32_splitk.hip;
    DevBuf<unsigned> d_fcctr; // allocated by set_weights when the shape is eligible AND SABER_HIP_FC_F32_SPLITK=1: opt-in, measured no faster - profiles/r06/fc_tail.txt)
    DevBuf<float> d_wfc;     // FP32 fc at <= 16 rows: the weights fragment-major for the streaming kernel (fc_small.hip: fc_f32_stream_kernel PACKED)
    int gpool = 0;           // the global average pooling of the output fused (saber_hip_net_optimize flag 128): pins FAM_IMG1
    struct saber_hip_stage* img_stage = nullptr;   // FAM_IMG1: the single-phase descriptor + repacked weights of that kernel (img_conv_prepare)
    bool no_placement = false;   // the op belongs to a net that does NOT own the device (saber_hip_net_optimize flag 2048): no split-K through one XCD's L2
    int epi = EPI_I8_CONV;
    bool is_i8 = false;
    int x_dtype = DT_S8;     // dtype of the tensor the conv kernel itself reads
    int c_eff = 0;           // channel count the conv kernel sees (after padding)
    bool pre_quant = false;  // f32 NCHW input quantised into the workspace first
    bool pre_pad = false;    // 8-bit C<4 input padded to NHWC4 into the workspace
    bool pre_transpose = false;  // f32 NCHW input transposed to NHWC(c_eff) into the workspace
    size_t ws_bytes = 0;
    int Kg = 0, Kg_pad = 0, kw_pad = 0;
    float in_scale = 1.f, out_scale = 1.f;
    bool weights_set = false;
    std::vector<int8_t> wq_oihw;
    std::vector<float> w_scale;
    std::vector<float> bias_host;   // the op's f32 bias as handed to set_weights (saber_hip_net_optimize re-creates ops from it)
    std::vector<float> bias_p_host, scale_host;   // INT8: the device-side bias' / scale / comp arrays (conv1x1 chain repacks them)
    std::vector<int> comp_host;
    DevBuf<uint8_t> d_w;
    DevBuf<float> d_part;    // split-K: partial accumulators [tile][split] and the tiles' arrival counters (split_prepare)
    DevBuf<unsigned> d_part_ctr;
    unsigned* h_part_err = nullptr;   // pinned, device-mapped word the split-K kernels count placement violations in (split_prepare)
    DevBuf<uint8_t> d_w3;    // FP32 convs: the repacked weights split into three bf16 planes [3][K_pad][Kg_pad] (FAM_B3; needs c_eff % 8 == 0)
    DevBuf<float> d_bias, d_scale;
    DevBuf<int> d_comp;
    DevBuf<unsigned> d_sm_ctr;   // INT8 fc + softmax in one launch (fc_small.hip): the arrival counter, zero between launches
    bool has_bias = false, has_comp = false;
    std::string algo_name;
    // sibling pair (saber_hip_conv2d_create_pair): d.k = k1 + k2, rows >= k1 belong to the second conv
    int pair_k1 = 0, pair_k2 = 0, pair_relu2 = 0, pair_dtype2 = 0;
    const saber_hip_conv* pair_src_a = nullptr;   // the two ops the pair was made of (not owned; saber_hip_net_optimize flag 512 packs
    const saber_hip_conv* pair_src_b = nullptr;   // their weights again for the stem kernel's tail)
};

// the fused stem conv + max pooling with the sibling pair of 1x1 convs reading the pooled tensor in the same launch
// (conv_stem.h: conv_stem_pool_pair_kernel); refers to the three ops, owns the pair's weights in fragment order and its constants
struct saber_hip_stem_pair {
    saber_hip_conv* stem = nullptr;
    const saber_hip_conv* a = nullptr;
    const saber_hip_conv* b = nullptr;
    DevBuf<uint8_t> d_w, d_prm;
};

// Which kernel a chain launches: the decoded meaning of a saber_hip_conv2d_chain_set_tile code FOR ONE CHAIN (the same code names different forms
// at different C). The one table from (C, kind of chain, code) to a form is chain_forms in api_chain.hip; everything else reads these fields.
enum ChainStream { CS_BASE, CS_SPLIT, CS_SPLIT8, CS_W8, CS_COOP2, CS_COOP4, CS_COUNT };      // weight-stream layouts (api_chain.hip: pack_chain_stream)
struct ChainForm {
    int code = 0;            // the public code (bits 24..27 of saber_hip_net_get_choice); 0: no such form
    int rows = 0;            // 3x3-led: rows of the 16-column pixel tile; 1x1 chain: 16-pixel fragments per workgroup
    int waves = 4;           // per workgroup (4 | 8)
    int split = 1;           // workgroups the second conv's output channels are split over (1 | 2)
    int coop = 1;            // cooperating workgroups per tile (1 | 2: conv_chain_coop.hip | 4: a one-block stage, conv_stage_coop.hip)
    ChainStream stream = CS_BASE;
    bool placement = false;  // relies on where the hardware places workgroups: never on a shared device, falls back to chain_form_plain
};

// two 1x1 INT8 convs in one launch (conv1x1_chain.hip); refers to the two ops, owns the repacked streams
struct saber_hip_chain {
    saber_hip_conv* c3 = nullptr;   // the block's 3x3 conv in front of `a` (saber_hip_conv2d_chain_create3), or null
    saber_hip_conv* a = nullptr;
    saber_hip_conv* b = nullptr;
    saber_hip_conv* b2 = nullptr;   // strided head + sibling pair (saber_hip_conv2d_chain_create3_pair): b and b2 both read a's output
    int c1 = 0, k1 = 0, k2 = 0;
    float scale_conv = 1.f;         // a's out_scale WHEN THE CHAIN WAS CREATED (the fused eltwise's first scale): copied like the weights and constants, so that
                                    // every form of the chain and every stage built from it use the value a's packed per-channel scale was made with
    std::vector<int8_t> tail_w3, tail_wa;   // strided head at C = 256 (no second 1x1 conv): c3's and a's quantised weights as they were when the chain was
                                    // created - a stage that takes the chain as its tail packs its own stream layout from them
    ChainForm form;                 // the selected form (written by chain_build, set_tile and the fall-back from a placement-dependent form)
    DevBuf<uint8_t> d_stream[CS_COUNT];   // one stream per layout that some form of this chain reads (chain_build)
    DevBuf<uint8_t> d_prm0, d_prm1, d_prm2;
    // CS_COOP2: the pairs' arrival counters, the 3x3 conv's exchange tile, the halves' XCC ids, the pinned error word; CS_COOP4: all but the streams is in `stage1`
    DevBuf<uint8_t> d_coop_xch;
    DevBuf<uint8_t> d_stream_stage1;  // C == 128 | 64, 3x3-led (stride 1) with a second 1x1 conv: per-wave streams of the one-workgroup-per-tile stage kernel
    DevBuf<unsigned long long> d_coop_ctr;
    DevBuf<unsigned> d_coop_xcc;
    unsigned* h_coop_err = nullptr;
    int coop_tiles = 0;
    struct saber_hip_chain_stage* stage1 = nullptr;
    ~saber_hip_chain();      // api_chain.hip
};

// A run of 3x3-led C = 256 chains as ONE persistent launch (conv_stage_coop.hip): the chains' own weight streams and constants, the
// hand-off counters / exchange tiles / XCC words of the launch, a pinned error word. The chains are NOT owned.
struct saber_hip_chain_stage {
    std::vector<saber_hip_chain*> chains;
    saber_hip_chain* tail = nullptr;      // the strided head behind the run (saber_hip_conv2d_stage_create_tail): d_blk[chains.size()] holds its constants
    DevBuf<uint8_t> d_tail_stream;        // ... and this its weight fragments (api_chain.hip: pack_coop4_stream without b)
    // the sibling pair in front of the run (saber_hip_conv2d_stage_create_head; not owned): d_blk[0] holds its constants (the blocks' then start at d_blk[1]), these its
    // weight fragments (api_chain.hip: pack_stage_head_stream) and the two convs' {scale, bias', comp}
    const saber_hip_conv* head_a = nullptr;
    const saber_hip_conv* head_b = nullptr;
    DevBuf<uint8_t> d_head_stream, d_head_prm1, d_head_prm2;
    DevBuf<saber_mi355x::StageBlk> d_blk;
    DevBuf<unsigned long long> d_grp_ctr, d_img_ctr;
    DevBuf<uint8_t> d_xch;
    DevBuf<unsigned> d_xcc;
    unsigned* h_err = nullptr;
    int c1 = 0, n = 0, h = 0, w = 0, tiles_x = 0, tiles_per_img = 0;
    bool per_image = false;
    ~saber_hip_chain_stage() {
        if (h_err) (void)hipHostFree(h_err);
    }
};

// a depthwise 3x3 INT8 conv and the pointwise 1x1 INT8 conv that reads it in one launch (conv_sep.hip); refers to the two ops, owns
// the depthwise weights / constants and the pointwise fragment stream / constants as they were when it was created
struct saber_hip_sep {
    saber_hip_conv* dw = nullptr;
    saber_hip_conv* pw = nullptr;
    int form = 0;                   // the selected row of conv_sep.hip's form table (its code)
    DevBuf<uint8_t> d_wdw, d_wpw, d_prm;
    DevBuf<float> d_dw_bias, d_dw_scale;
    std::string name;               // "sep_dw3x3_pw_i8_<form>" of the selected form
};

// an inverted-residual block - 1x1 expand, depthwise 3x3, 1x1 project (+ the eltwise sum with the block's input) INT8 convs - in one launch
// (conv_ir.hip); refers to the three ops, owns both fragment streams, the depthwise weights and every constant table as they were when it was
// created
struct saber_hip_ir {
    saber_hip_conv* expand = nullptr;
    saber_hip_conv* dw = nullptr;
    saber_hip_conv* project = nullptr;
    int form = 0;                   // the selected row of conv_ir.hip's form table (its code)
    float scale_conv = 1.f;         // project's out_scale when the block was created (the fused eltwise's first scale): copied like the constant tables
    DevBuf<uint8_t> d_we, d_eprm, d_wdw, d_wp, d_pprm;
    DevBuf<float> d_dw_bias, d_dw_scale;
    std::string name;               // "ir_expand_dw_project_i8_<form>" of the selected form
};

// a Fire module - a 1x1 squeeze conv, the 1x1 and the padded 3x3 expand convs that read it, and the concat of the two - in one launch
// (conv_fire.hip); refers to the three ops, owns the three fragment streams and constant tables as they were when it was created
struct saber_hip_fire {
    saber_hip_conv* squeeze = nullptr;
    saber_hip_conv* e1 = nullptr;
    saber_hip_conv* e3 = nullptr;
    int form = 0;                   // the selected row of conv_fire.hip's form table (its code)
    DevBuf<uint8_t> d_ws, d_sprm, d_w1, d_prm1, d_w3, d_prm3;
    std::string name;               // "fire_squeeze_expand_i8_<form>" of the selected form
};

// a transposed convolution (api_deconv.hip, deconv.hip): FP32 only, a type of its own - nothing of saber_hip_conv reads it
struct saber_hip_deconv {
    saber_hip_conv_desc d;
    int oh = 0, ow = 0;
    int form = 0;            // 0: deconv_direct_f32; 1 / 2: deconv_b3_f32_4x16 / _2x16 (written by deconv_set_form only)
    bool b3_ok = false;      // the bf16-plane forms exist for this descriptor
    bool weights_set = false, has_bias = false;
    std::vector<float> w_host;        // [c][k / group][kh][kw] as handed to set_weights (the fragment stream is packed from it on demand)
    DevBuf<float> d_w, d_bias;        // the direct kernel's [tap][c][k / group] repack; the bias
    DevBuf<uint8_t> d_wfrag;          // the bf16-plane forms' fragment stream (deconv_b3_pack)
    std::string algo_name;
};

// a resize (api_resize.hip, resize.hip): FP32 only, a type of its own
struct saber_hip_resize {
    saber_hip_resize_desc d;
    int oh = 0, ow = 0;
    int form = 0;            // 0: resize_direct_f32; 1: resize_rows_f32; 2: resize_x2_f32 (written by resize_set_form only)
    bool x2_ok = false;      // an integer x2 in mode 1 or 3 whose tables keep every tap within a row / column of o / 2 (form 2, with NHWC and c % 4 == 0)
    std::vector<saber_mi355x::ResizeTap> th, tw;      // per output row / column: the taps and the fraction, in the reference's float steps (create)
    DevBuf<saber_mi355x::ResizeTap> d_th, d_tw;       // ... on the device, from the first run or saber_hip_net_add_resize on
    std::string algo_name;
};

// a DetectionOutput (api_detout.hip, detout.hip): FP32 only, a type of its own
struct saber_hip_detout {
    saber_hip_detout_desc d;
    int form = 0;            // 0: detout_direct_f32; 1: detout_mask_f32 (written by detout_set_form only)
    // the kept candidates of every (image, class) between the two launches; on the device from the first run or saber_hip_net_add_detout on
    DevBuf<int> d_cnt;
    DevBuf<uint2> d_key;
    DevBuf<float4> d_box;
    std::string algo_name;
};

struct saber_hip_fc {
    saber_hip_fc_desc d;
    saber_hip_conv* conv = nullptr;
    bool pre_quant = false;
    float in_scale = 1.f;
};

namespace saber_api {
struct EventPair {   // RAII: destroyed on every exit path
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t init() {
        hipError_t e = hipEventCreate(&e0);
        return e != hipSuccess ? e : hipEventCreate(&e1);
    }
    ~EventPair() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};
// Times launches the way they run inside an op list: between repetitions a 64 MB stream through every XCD pushes the
// operands out of the L2s (the Infinity Cache keeps them), so a kernel that re-reads many weights per workgroup is not
// flattered by finding them in L2 the way a back-to-back loop of the same launch does (measured: conv3x3 + chain at
// C = 256 reads 12.9 us back to back, 16 us in the forward pass; the two launches it replaces 13.9 -> 15.3 us).
struct ColdBench {
    // 64 MB pushes the operands out of the 8 x 4 MB of L2 (the 256 MB Infinity Cache keeps them: right for a net whose whole forward
    // pass fits it, ResNet50 INT8 at batch 8 moves ~190 MB). A net whose pass moves more (VGG16 FP32 at batch 8: > 400 MB of
    // activations) finds its weights in neither cache: saber_hip_net_autotune then asks for a flush of that size (up to 512 MB) -
    // measured: with the 64 MB flush the tuner preferred the LDS-halo FP32 kernel for VGG16's 512-channel layers (90 / 169 us "cold")
    // which then ran at 120 / 227 us in the pass, where every workgroup streams its 1.7 MB of weight planes from HBM.
    size_t kBytes = (size_t)64 << 20;
    void* buf = nullptr;
    std::vector<hipEvent_t> ev;
    int reps = 0;
    hipError_t init(int r, size_t bytes = 0) {
        if (bytes) kBytes = std::min<size_t>(std::max<size_t>(bytes, (size_t)64 << 20), (size_t)512 << 20) & ~(size_t)0xfffff;
        reps = r < 3 ? 3 : (r > 32 ? 32 : r);
        hipError_t e = hipMalloc(&buf, kBytes + 256);
        if (e != hipSuccess) return e;
        e = hipMemset(buf, 1, kBytes + 256);
        if (e != hipSuccess) return e;
        ev.assign(2 * (size_t)reps, nullptr);
        for (hipEvent_t& x : ev)
            if ((e = hipEventCreate(&x)) != hipSuccess) return e;
        return hipStreamSynchronize(nullptr);
    }
    ~ColdBench() {
        for (hipEvent_t x : ev)
            if (x) (void)hipEventDestroy(x);
        if (buf) (void)hipFree(buf);
    }
    // median microseconds of fn() (which enqueues on s and returns a status); < 0 on failure
    float run(hipStream_t s, const std::function<int()>& fn) {
        if (fn() != 0) return -1.f;                  // warm-up: code, kernel arguments
        for (int r = 0; r < reps; ++r) {
            if (launch_l2_flush(buf, kBytes, (unsigned*)((char*)buf + kBytes), s) != hipSuccess) return -1.f;
            if (hipEventRecord(ev[2 * r], s) != hipSuccess) return -1.f;
            if (fn() != 0) return -1.f;
            if (hipEventRecord(ev[2 * r + 1], s) != hipSuccess) return -1.f;
        }
        if (hipEventSynchronize(ev[2 * reps - 1]) != hipSuccess) return -1.f;
        std::vector<float> t(reps);
        for (int r = 0; r < reps; ++r)
            if (hipEventElapsedTime(&t[r], ev[2 * r], ev[2 * r + 1]) != hipSuccess) return -1.f;
        std::sort(t.begin(), t.end());
        return t[reps / 2] * 1000.f;
    }
};

// One ColdBench per top-level autotune call: nested calls (saber_hip_net_autotune -> saber_hip_conv2d_autotune) share it.
// SABER_HIP_AUTOTUNE_WARM=1 in the environment restores the back-to-back timing loop (kept for A/B measurements).
extern thread_local ColdBench* g_cold;      // api_autotune.hip
// times whatever fn() enqueues on s: *t = the cold-L2 median in microseconds, or - warm loop - the milliseconds of warm_iters back-to-back
// calls after one warm-up. A status; nothing is timed when fn() fails.
int time_enqueued(hipStream_t s, const std::function<int()>& fn, int warm_iters, float* t);      // api_autotune.hip
// Kernel reuse across the ops of one net: the FIRST launch of a given kernel function in a forward pass pays for its cold
// code (0.3-0.6 us on most boxes of the pool, 3-9 us on some: profiles/r02/slow_box/ - repeats of the same function
// later in the pass run at full speed), so among candidates within g_reuse_tol of the fastest the tuner prefers a
// function another op of the net already uses. Set by saber_hip_net_autotune for the duration of its run.
extern thread_local std::vector<unsigned long long>* g_used_kernels;      // api_autotune.hip
constexpr float g_reuse_tol = 0.03f;
struct ColdScope {
    ColdBench local;
    bool owner = false;
    hipError_t enter(int reps, size_t flush_bytes = 0) {
        const char* w = std::getenv("SABER_HIP_AUTOTUNE_WARM");
        if (w && w[0] == '1') return hipSuccess;      // g_cold stays null: callers fall back to the warm loop
        if (g_cold) return hipSuccess;
        hipError_t e = local.init(reps, flush_bytes);
        if (e != hipSuccess) return e;
        g_cold = &local;
        owner = true;
        return hipSuccess;
    }
    ~ColdScope() {
        if (owner) g_cold = nullptr;
    }
};

}  // namespace saber_api

// op-list executor
namespace saber_api {
enum OpKind { OP_CONV, OP_CONV_PAIR, OP_FC, OP_QUANT, OP_DEQUANT, OP_TRANSPOSE_IN, OP_ELT_I8, OP_ELT_F32, OP_POOL_I8, OP_POOL_F32, OP_POOL_F32_I8, OP_FC_Q, OP_SOFTMAX, OP_RELU_F32, OP_ACT_F32, OP_CONCAT, OP_DECONV, OP_RESIZE, OP_DETOUT };
// What an op launches in the current selection: DERIVED from the sites' decisions by net_resolve (api_net_optimize.hip), never set elsewhere
enum Launch { LAUNCH_NONE, LAUNCH_OWN, LAUNCH_CHAIN, LAUNCH_CHAIN3, LAUNCH_STAGE, LAUNCH_STEM_PAIR, LAUNCH_SEP, LAUNCH_IR, LAUNCH_FIRE, LAUNCH_RESIZE_SUM };
// A SITE is a group of adjacent ops that can run as one launch. The op that heads a site holds the site's object and its DECISION (*_on: stored
// as asked by the net_set_* setters and read back by saber_hip_net_get_choice; a decision is never changed to express what another site
// does); what every op launches, which ops launch nothing and every conv / pair / fc / softmax op's name follow from the decisions in
// net_resolve alone.
struct NetOp {
    OpKind kind;
    std::string name;
    saber_hip_conv* conv = nullptr;
    saber_hip_fc* fc = nullptr;
    saber_hip_deconv* deconv = nullptr;      // OP_DECONV
    saber_hip_resize* resize = nullptr;      // OP_RESIZE
    saber_hip_detout* detout = nullptr;      // OP_DETOUT: ins = {loc, conf[, prior]}, out = y, out2 = count
    int in = -1, in2 = -1, out = -1, out2 = -1;
    // OP_CONCAT: EVERY input id in channel order (in = ins[0], in2 stays -1), their channel counts in elements and - u8 with rescaling - the
    // per-input multipliers (empty: a copy). Whatever asks which tensors an op reads goes through op_for_each_input / op_reads below.
    std::vector<int> ins, cat_c;
    std::vector<float> cat_m;
    // derived (net_resolve): this op's launch; LAUNCH_NONE = `skip`: ops[absorbed_by]'s launch covers it
    Launch launch = LAUNCH_OWN;
    int absorbed_by = -1;
    bool skip = false;
    std::string res_note;      // "+res/<stride>" behind the name of a conv that reads its residual strided (flag 64), until a selection is applied to the op
    // conv1x1 chain (saber_hip_net_optimize flag 16): this conv and the NEXT op (a 1x1 conv reading its output) run as one
    // launch while chain_on is set
    saber_hip_chain* chain = nullptr;
    int chain_out = -1;
    bool chain_on = false;
    // ... with the block's 3x3 conv in front (flag 32): THIS op is that 3x3 conv, the next two are the chain; while led_on
    // is set it launches all three (its own output edge is then not written)
    saber_hip_chain* chain3 = nullptr;
    int chain3_res = -1, chain3_y1 = -1, chain3_y2 = -1;
    int chain3_y3 = -1;      // strided head + sibling pair (flag 1024): the pair's second output; the launch covers the pair op (ops[i + 2]) too
    bool led_on = false;
    // ... and a RUN of such 3x3-led C = 256 chains (flag 256): THIS op is the first block's 3x3 conv; while stage_on is set it launches
    // all stage_n chains (3 * stage_n ops) as one persistent launch (saber_hip_conv2d_stage_run)
    saber_hip_chain_stage* stage = nullptr;
    int stage_n = 0;
    bool stage_on = false;
    // (names only: a stage that goes off leaves its blocks' 3x3 convs under the names they had inside the launch until a word or a chain mode
    // of their own arrives - what the executor has always reported after a fallback; kept so that every op name stays what it was)
    bool stage_name_kept = false;
    // ... with the strided head behind the run as the launch's TAIL (the stage was created with one): the two ops behind the last block -
    // ops[3 * stage_n] (its 3x3 conv, tail_of = the index of THIS op) and the 1x1 conv behind it - are covered while tail_on is set and
    // the stage is on; the strided head's own led_on stays underneath
    bool tail_on = false;
    int tail_of = -1;
    // ... and with the sibling pair in front of the run as the launch's HEAD (the stage was created with one): the OP_CONV_PAIR op ops[-1]
    // (head_of = the index of THIS op) is covered while head_on is set and the stage is on; its first output - this op's chain3_res - is
    // then not written. Switching the stage on never sets it; switching the stage off clears it
    bool head_on = false;
    int head_of = -1;
    // a block's 3x3 conv inside a C = 64 run, not the last block: the block's first output (chain3_y1) is read only by the next block of the
    // run - its eltwise and its first 1x1 conv. While the stage launch is selected that tensor stays in LDS and is not written
    bool stage_y1_private = false;
    // the fused stem conv + pooling with the sibling pair that reads the pooled tensor (flag 512): THIS op is the stem conv and always covers
    // the next op (the pair); stem_y1 / stem_y2 are the pair's outputs and this op's own output edge is not written
    saber_hip_stem_pair* stem_pair = nullptr;
    int stem_y1 = -1, stem_y2 = -1;
    // a depthwise 3x3 conv and the 1x1 conv behind it (flag 16384, SABER_HIP_NET_SEPARABLE): THIS op is the depthwise conv; while sep_on is
    // set its launch covers the pointwise op behind it, this op's own output edge is not written and sep_out is the pointwise output
    saber_hip_sep* sep = nullptr;
    int sep_out = -1;
    bool sep_on = false;
    // an inverted-residual block (flag 32768, SABER_HIP_NET_INVERTED_RESIDUAL): THIS op is the 1x1 expand conv, the next two are the depthwise
    // 3x3 and the 1x1 project conv; while ir_on is set its launch covers both, this op's and the depthwise op's output edges are not written
    // and ir_out is the project op's output
    saber_hip_ir* ir = nullptr;
    int ir_out = -1;
    bool ir_on = false;
    // a Fire module (flag 65536, SABER_HIP_NET_FIRE): THIS op is the 1x1 squeeze conv, the next three are the two expand convs and the concat;
    // while fire_on is set its launch covers all three, this op's and both expand ops' output edges are not written and fire_out is the
    // concat's output
    saber_hip_fire* fire = nullptr;
    int fire_out = -1;
    bool fire_on = false;
    // a resize and the eltwise_f32 behind it that alone reads it (flag 131072, SABER_HIP_NET_RESIZE_SUM): THIS op is the resize; while rsum_on is
    // set its launch covers the eltwise op behind it (resize + sum in one launch) and this op's own output edge is not written
    bool rsum = false, rsum_on = false;
    int lane = 0;            // 0: caller's stream, 1: the net's side stream (graph::Lane, operator_func.h:103-114)
    bool record = false;     // an op on the other lane consumes this op's output: record an event after it
    int p[16] = {0};
    float f[6] = {0};
    size_t count = 0;
};
// the tensors an op READS as operands (a concat, a detout: the whole input list; every other kind: in and in2)
template <typename F>
inline void op_for_each_input(const NetOp& o, F&& f) {
    if (o.kind == OP_CONCAT || o.kind == OP_DETOUT) {
        for (int t : o.ins) f(t);
        return;
    }
    if (o.in >= 0) f(o.in);
    if (o.in2 >= 0) f(o.in2);
}
inline int op_reads(const NetOp& o, int t) {      // how many of its operands are tensor t
    int n = 0;
    op_for_each_input(o, [&](int u) { n += u == t; });
    return n;
}
inline bool op_touches(const NetOp& o, int t) { return op_reads(o, t) || o.out == t || o.out2 == t; }
}  // namespace saber_api

struct saber_hip_net {
    std::vector<size_t> tensor_bytes;
    std::vector<size_t> tensor_off;
    std::vector<void*> tensor_ext;     // per tensor: caller-owned storage (saber_hip_net_bind_tensor) or null = a slot of the arena
    std::vector<std::pair<const void*, int>> captured_ptr;   // captured nets: caller pointer -> id of the LAST tensor seen there
    void* ptr(int id) const {
        if (id < 0) return nullptr;
        if ((size_t)id < tensor_ext.size() && tensor_ext[id]) return tensor_ext[id];
        return (void*)(arena + tensor_off[id]);
    }
    std::vector<NetOp> ops;
    char* arena = nullptr;
    size_t arena_bytes = 0, ws_off = 0, ws_bytes = 0;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    bool finalized = false;
    bool compacted = false;      // saber_hip_net_compact_arena ran: edges of disjoint lifetimes share memory (intermediate edges are not readable after a pass)
    // saber_hip_net_optimize flag 2048: other streams / processes run kernels on this device while the net does. Kernel variants whose
    // SPEED or completion depends on where the hardware places workgroups relative to each other - the persistent stage launch (needs
    // every workgroup of an image resident on its XCD at once), the cooperating-workgroup chains (tile codes 7 / 15), FP32 split-K
    // through one XCD's L2 - are then never selected: not statically, not by the autotuner, not from a restored selection.
    bool shared_device = false;
    // saber_hip_net_optimize flag 8192: FP32 ops keep their STATIC kernel selection - saber_hip_net_autotune and restored selections leave
    // them alone - so that two nets of one model answer bit-identically (the FP32 kernels differ in accumulation order; which one a
    // timing-based tuner picks depends on the box and the moment)
    bool reproducible_fp32 = false;
    bool inplace_external = false;   // captured nets: an in-place sum accumulates into a caller-owned input (api_capture.hip: readwrite)
    int coop_fallbacks = 0;   // cooperative launches that reported a failed pass (saber_hip_net_status), since the net was created
    // two-lane execution: independent branches (ResNet branch1 vs branch2a/2b) run on a side stream
    hipStream_t side = nullptr;
    hipEvent_t ev_start = nullptr, ev_join = nullptr;
    std::vector<hipEvent_t> ev_op;     // one per op that needs to publish its output to the other lane
    std::vector<int> writer;           // tensor id -> index of the op that last wrote it (-1: external)
    bool lanes_ready = false, has_side = false;
    std::vector<saber_hip_conv*> owned;   // ops created by saber_hip_net_optimize (destroyed with the net)
    std::vector<saber_hip_chain*> owned_chains;
    std::vector<saber_hip_chain_stage*> owned_stages;
    std::vector<saber_hip_stem_pair*> owned_stem_pairs;
    std::vector<saber_hip_sep*> owned_seps;
    std::vector<saber_hip_ir*> owned_irs;
    std::vector<saber_hip_fire*> owned_fires;
};

// Op-list capture (api_capture.hip; saber_hip_capture_begin / _end): while g_capture is set on the calling thread every
// capturable *_run entry point records itself into the capture's net instead of launching. Each recorder returns a status.
namespace saber_api {
struct Capture;
extern thread_local Capture* g_capture;
int capture_conv(saber_hip_conv* op, const void* x, void* y, const void* res);
int capture_fc(saber_hip_fc* fc, const void* x, float* y, bool quantised_input);
int capture_unsupported(const char* what);
int capture_deconv(saber_hip_deconv* op, const void* x, void* y);
int capture_resize(saber_hip_resize* op, const void* x, void* y);
int capture_detout(saber_hip_detout* op, const void* loc, const void* conf, const void* prior, void* y, void* count);
int capture_concat(size_t pixels, int n_inputs, const void* const* xs, const int* channels, const float* mult, int dtype, void* y);
// streaming ops: kind + the argument block of the matching saber_hip_net_add_* call; in2 / out2 may be null
int capture_stream_op(OpKind kind, const char* name, const int* p, int np, const float* f, int nf, size_t count, const void* in,
                      size_t in_bytes, const void* in2, size_t in2_bytes, void* out, size_t out_bytes, void* out2, size_t out2_bytes);
}  // namespace saber_api

// helpers one translation unit defines and another uses
// kernel selection (api_select.hip)
bool sel_valid(const saber_hip_conv* op, const saber_api::ConvSel& s);      // the family and its parameters exist for this op
int sel_set(saber_hip_conv* op, const saber_api::ConvSel& s);      // the one writer of op->sel: validates, makes the family's on-demand buffers, names
void sel_release_unused(saber_hip_conv* op);      // the buffers only a family other than the selected one reads
void sel_name(saber_hip_conv* op);      // op->algo_name of the current selection and fused-pooling properties
unsigned long long sel_kernel_key(const saber_hip_conv* op, const saber_api::ConvSel& s);
int sel_launch(saber_hip_conv* op, saber_mi355x::ConvKArgs& a, hipStream_t s);
void for_each_candidate(const saber_hip_conv* op, const saber_api::ConvSel* best, const std::function<void(const saber_api::ConvSel&)>& fn);
bool dw_ok(const saber_hip_conv* op);
bool group_ok(const saber_hip_conv* op);
bool stem_ok(const saber_hip_conv* op);
bool fc_small_ok(const saber_hip_conv* op);
bool b3_tile_ok(const saber_hip_conv* op, int tile, int ks);
int dw_static_form(const saber_hip_conv* op);      // api_conv.hip: create's choice among the depthwise forms
int group_static_form(const saber_hip_conv* op);      // api_conv.hip: create's choice among the direct kernel (0) and the grouped 3x3 forms
constexpr long DW_STRIP_MIN_LANES = 150000;     // (lanes = channel vectors x output pixels. Measured, profiles/dw3x3/README.md: at 200 704 lanes and above the strip form is the faster one for both element types, at 100 352 and below the one-pixel form)
void conv_fill_args(const saber_hip_conv* op, saber_mi355x::ConvKArgs& a, const void* x, void* y, const void* res);   // api_conv.hip
int stem_pool_args(const saber_hip_conv* op, const void* x, void* y, void* workspace, hipStream_t s, saber_mi355x::ConvKArgs* a);   // api_conv.hip
bool xcd_round_robin();      // api_conv.hip: workgroups 8 apart in a 1-D grid share an XCD on the current device (probed once)
int split_prepare(saber_hip_conv* op);      // api_conv.hip: the FP32 split-K partial buffers, arrival counters and error word
// image-resident kernel variant of an INT8 conv on <= 64-pixel images (api_stage.hip)
bool img_conv_ok(const saber_hip_conv* op);
int img_conv_prepare(saber_hip_conv* op);
int pw_prepare(saber_hip_conv* op);      // api_conv.hip: the FP32 pointwise kernels' fragment-ordered weight planes, on demand
bool pw_eligible(const saber_hip_conv* op);
int img_conv_run(saber_hip_conv* op, const void* x, void* y, const void* res, void* y_pool, hipStream_t stream);
void img_conv_release(saber_hip_conv* op);
int net_launch(saber_hip_net* net, const NetOp& o, hipStream_t s);      // api_net.hip
bool fc_softmax_ok(const saber_hip_fc* fc, bool quantised_input = false);      // api_ops.hip: the INT8 small-batch fc kernel can normalise its own logits (fc_small.hip)
int fc_run_softmax(saber_hip_fc* fc, const void* x, float* y, float* prob, void* workspace, hipStream_t s, bool quantised_input);
int fc_softmax_prepare(saber_hip_fc* fc);        // ... allocates the arrival counter (not under stream capture)
int concat_check(int n_inputs, const int* channels, const float* mult, int dtype, int* row_bytes);      // api_ops.hip: a status; row_bytes (may be null) = bytes per pixel of each input
// sites (api_net_optimize.hip): each setter stores decisions and calls net_resolve, the one place that derives launch / absorbed_by / skip and the names
void net_resolve(saber_hip_net* net);
void net_drop_graph(saber_hip_net* net);      // api_net.hip: a captured hipGraph holds the old selection / addresses
// the ops around A = ops[ia] (a 1x1 conv with the fused eltwise): 0 separate launches, 1 A + the next op chained, 2 the 3x3 conv ops[ia - 1] leads the launch
void net_set_chain_mode(saber_hip_net* net, int ia, int mode);
int net_chain_mode(const saber_hip_net* net, int ia);
// the stage headed by ops[i0] (NetOp::stage) on / off: on puts every block into its 3x3-led form and brings the tail (not the head); off takes both
void net_set_stage(saber_hip_net* net, int i0, bool on);
void net_set_head(saber_hip_net* net, int i0, bool on);    // the head of the stage headed by ops[i0]; in effect only while the stage is on
void net_set_tail(saber_hip_net* net, int i0, bool on);    // the tail of the stage headed by ops[i0]; in effect only while the stage is on
// chain forms (api_chain.hip)
ChainForm chain_form(const saber_hip_chain* ch, int code);      // the table: what `code` means for this chain, code 0 if nothing
bool chain_form_valid(const saber_hip_chain* ch, int code);      // the form exists for this chain and its stream is packed
ChainForm chain_form_default(const saber_hip_chain* ch);      // create's choice
ChainForm chain_form_plain(const saber_hip_chain* ch);      // what a placement-dependent form falls back to
std::string chain_form_name(const saber_hip_chain* ch);      // of the selected form
void for_each_chain_candidate(const saber_hip_chain* ch, bool shared_device, const std::function<void(const ChainForm&)>& fn);
// separable pairs (api_sep.hip)
bool conv_sep_ok(const saber_hip_conv* dw, const saber_hip_conv* pw, std::string* why);      // the pair is one conv_sep.hip can run
bool sep_form_valid(const saber_hip_sep* sp, int code);      // the form exists for this pair
void for_each_sep_form(const saber_hip_sep* sp, const std::function<void(int code)>& fn);      // its forms, in the autotuner's candidate order
int sep_static_form(const saber_hip_sep* sp);      // the executor's static choice: a form code, or 0 = two launches
void net_set_sep(saber_hip_net* net, int i, int code);      // api_net_optimize.hip: the site headed by ops[i] on (a valid form code) / off (0)
// inverted-residual blocks (api_ir.hip)
bool conv_ir_ok(const saber_hip_conv* expand, const saber_hip_conv* dw, const saber_hip_conv* project, std::string* why);      // a block conv_ir.hip can run
bool ir_form_valid(const saber_hip_ir* ir, int code);      // the form exists for this block
void for_each_ir_form(const saber_hip_ir* ir, const std::function<void(int code)>& fn);      // its forms, in the autotuner's candidate order
int ir_static_form(const saber_hip_ir* ir);      // the executor's static choice: a form code, or 0 = three launches
void net_set_ir(saber_hip_net* net, int i, int code);      // api_net_optimize.hip: the site headed by ops[i] on (a valid form code) / off (0)
// Fire modules (api_fire.hip)
bool conv_fire_ok(const saber_hip_conv* squeeze, const saber_hip_conv* e1, const saber_hip_conv* e3, std::string* why);      // a module conv_fire.hip can run
bool fire_form_valid(const saber_hip_fire* fr, int code);
void for_each_fire_form(const saber_hip_fire* fr, const std::function<void(int code)>& fn);
int fire_static_form(const saber_hip_fire* fr);      // the executor's static choice: a form code, or 0 = four launches
void net_set_fire(saber_hip_net* net, int i, int code);      // api_net_optimize.hip: the site headed by ops[i] on (a valid form code) / off (0)
// transposed convolutions (api_deconv.hip)
bool deconv_form_valid(const saber_hip_deconv* op, int form);      // the form exists for this op
int deconv_static_form(const saber_hip_deconv* op);      // create's choice: measured rows only (profiles/deconv/README.md), else 0
void for_each_deconv_form(const saber_hip_deconv* op, const std::function<void(int form)>& fn);      // the autotuner's candidates, form 0 first
// resizes (api_resize.hip)
bool resize_form_valid(const saber_hip_resize* op, int form);      // the form exists for this op
int resize_static_form(const saber_hip_resize* op);      // create's choice (profiles/resize/README.md)
bool resize_sum_static_on(const saber_hip_resize* op);      // the executor's static choice for a resize + sum site (flag 131072)
void for_each_resize_form(const saber_hip_resize* op, const std::function<void(int form)>& fn);      // the autotuner's candidates, form 0 first
int resize_prepare(saber_hip_resize* op);      // the tables on the device (not under stream capture)
void net_set_resize_sum(saber_hip_net* net, int i, bool on);      // api_net_optimize.hip: the site headed by ops[i] on / off
// detection outputs (api_detout.hip)
bool detout_form_valid(const saber_hip_detout* op, int form);      // the form exists for this op
int detout_static_form(const saber_hip_detout* op);      // create's choice (profiles/detout/README.md)
void for_each_detout_form(const saber_hip_detout* op, const std::function<void(int form)>& fn);      // the autotuner's candidates, form 0 first
int detout_prepare(saber_hip_detout* op);      // the scratch on the device (not under stream capture)
// api_chain.hip; y_tail: the tail's output - the tail then runs inside the launch (a stage created with one), null: the blocks only
// y_head: the second output of the stage's head - the pair then runs inside the launch (a stage created with one), x is the PAIR's input and res is not read
int stage_run(saber_hip_chain_stage* st, const void* x, const void* res, void* const* y1, void* const* y2, hipStream_t s, void* y_tail = nullptr,
              void* y_head = nullptr);
