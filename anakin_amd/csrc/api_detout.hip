// anakin_amd/csrc/api_detout.hip - DetectionOutput (saber_hip_detout_*): the reference's DetectionOutput<T, AK_FLOAT>
// (saber/funcs/detection_output.h; x86 saber_detection_output.cpp; detection_helper.cpp). FP32 only - the reference's dispatch checks
// AK_FLOAT on both inputs. A type of its own: the conv selection tables know nothing of it. Two launches (detout.hip) with a fixed-shape
// output; the op owns the scratch between them.
#include "api_internal.h"

bool detout_form_valid(const saber_hip_detout* op, int form) {
    if (form == 0) return true;
    return form == 1 && op->d.nms_eta == 1.f && detout_lds_bytes(1, op->d.nms_top_k) <= DETOUT_LDS_LIMIT;
}
void for_each_detout_form(const saber_hip_detout* op, const std::function<void(int form)>& fn) {
    for (int f = 0; f <= 1; ++f)
        if (detout_form_valid(op, f)) fn(f);
}
// The static rule (profiles/detout/README.md: MobileNet-SSD, SSD300 on 21 and 81 classes, SSD512, batch 1 and 8, warm and as the node of a
// replayed graph): detout_mask_f32 was ahead of form 0 on all 8 combinations under both protocols, by 13 % (81 classes) to 27 % (SSD300).
// Every measured row has nms_top_k = 400 and eta = 1: form 1 is named there and nowhere else - form 1's bit matrix grows with the square of
// nms_top_k, form 0's votes with nms_top_k times the kept boxes, and no row says where they cross. The autotuner times both everywhere.
constexpr int DETOUT_MASK_MEASURED_NMS_TOP_K = 400;
int detout_static_form(const saber_hip_detout* op) {
    return detout_form_valid(op, 1) && op->d.nms_top_k == DETOUT_MASK_MEASURED_NMS_TOP_K ? 1 : 0;
}
static const char* detout_form_name(int form) { return form == 1 ? "detout_mask_f32" : "detout_direct_f32"; }
static int detout_set_form(saber_hip_detout* op, int form) {      // the one writer of op->form
    if (!detout_form_valid(op, form))
        return fail(SABER_HIP_INVALID_VALUE, "detout: no such form for this op (0 direct; 1 mask: nms_eta == 1 only)");
    op->form = form;
    op->algo_name = detout_form_name(form);
    return SABER_HIP_OK;
}

int saber_hip_detout_create(const saber_hip_detout_desc* desc, saber_hip_detout_t** out) {
    if (!desc || !out) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    *out = nullptr;
    const saber_hip_detout_desc& d = *desc;
    if (d.n <= 0 || d.classes <= 0 || d.priors <= 0) return fail(SABER_HIP_INVALID_VALUE, "detout: non-positive size");
    if (d.dtype != SABER_HIP_F32) return fail(SABER_HIP_UNIMPL, "detout: FP32 only (the reference's dispatch checks AK_FLOAT on both inputs)");
    if (!d.share_location) return fail(SABER_HIP_UNIMPL, "detout: share_location = false (the two-stage path with sequence offsets) is not built");
    if (d.keep_top_k < 1) return fail(SABER_HIP_UNIMPL, "detout: keep_top_k < 1 has no fixed-shape output");
    if (d.nms_top_k < 1 || d.nms_top_k > DETOUT_MAX_NMS_TOP_K) return fail(SABER_HIP_UNIMPL, "detout: nms_top_k outside 1 .. 1024");
    if (d.code_type < 1 || d.code_type > 3) return fail(SABER_HIP_INVALID_VALUE, "detout: code_type is 1 CORNER, 2 CENTER_SIZE or 3 CORNER_SIZE");
    if (d.background_id < -1 || d.background_id >= d.classes) return fail(SABER_HIP_INVALID_VALUE, "detout: background_id outside -1 .. classes - 1");
    if (!(d.nms_eta > 0.f && d.nms_eta <= 1.f)) return fail(SABER_HIP_INVALID_VALUE, "detout: nms_eta outside (0, 1]");
    const double lim = 2147483647.0;
    if ((double)d.n * d.keep_top_k * 7 >= lim || (double)d.n * d.classes * d.nms_top_k >= lim || (double)d.n * d.priors * 4 >= lim ||
        (double)d.priors * d.classes >= lim)
        return fail(SABER_HIP_INVALID_VALUE, "detout: tensor too large (a product of the sizes passes 2^31)");
    if (!detout_keep_fits(d.classes, d.nms_top_k, d.keep_top_k))
        return fail(SABER_HIP_UNIMPL, "detout: keep_top_k in 3073 .. classes * nms_top_k - 1 (the per-image cut selects in LDS)");
    std::unique_ptr<saber_hip_detout> op(new saber_hip_detout());
    op->d = d;
    (void)detout_set_form(op.get(), detout_static_form(op.get()));
    *out = op.release();
    return SABER_HIP_OK;
}

int saber_hip_detout_out_rows(const saber_hip_detout_t* op) { return op ? op->d.n * op->d.keep_top_k : 0; }
const char* saber_hip_detout_algo(const saber_hip_detout_t* op) { return op ? op->algo_name.c_str() : ""; }
int saber_hip_detout_set_tile(saber_hip_detout_t* op, int form) {
    if (!op) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    return detout_set_form(op, form);
}
int saber_hip_detout_get_tile(const saber_hip_detout_t* op) { return op ? op->form : 0; }
void saber_hip_detout_destroy(saber_hip_detout_t* op) { delete op; }

int saber_hip_detout_read_total(const void* count, saber_hip_stream_t stream, int* total) {
    if (!count || !total) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    if (g_capture) return capture_unsupported("saber_hip_detout_read_total (a recorded pass has no host step: read count[0] after the pass)");
    HIP_TRY(hipMemcpyAsync(total, count, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return SABER_HIP_OK;
}

int detout_prepare(saber_hip_detout* op) {
    if (op->d_cnt.p && op->d_key.p && op->d_box.p) return SABER_HIP_OK;
    const size_t cls = (size_t)op->d.n * op->d.classes;
    HIP_TRY(op->d_cnt.alloc_zero(cls));
    HIP_TRY(op->d_key.alloc_zero(cls * op->d.nms_top_k));
    HIP_TRY(op->d_box.alloc_zero(cls * op->d.nms_top_k));
    return SABER_HIP_OK;
}

int saber_hip_detout_run(saber_hip_detout_t* op, const void* loc, const void* conf, const void* prior, void* y, void* count,
                         saber_hip_stream_t stream) {
    if (!op || !loc || !conf || !y || !count) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    if ((op->d.has_prior != 0) != (prior != nullptr))
        return fail(SABER_HIP_INVALID_VALUE, "detout: a prior tensor is given exactly where the op was created with has_prior");
    if (g_capture) return capture_detout(op, loc, conf, prior, y, count);
    const int rc = detout_prepare(op);
    if (rc) return rc;
    const saber_hip_detout_desc& d = op->d;
    DetoutKArgs a{};
    a.loc = (const float*)loc; a.conf = (const float*)conf; a.prior = (const float*)prior;
    a.y = (float*)y; a.count = (int*)count;
    a.cls_cnt = op->d_cnt.p; a.cls_key = op->d_key.p; a.cls_box = op->d_box.p;
    a.N = d.n; a.C = d.classes; a.P = d.priors; a.K = d.nms_top_k; a.keep = d.keep_top_k; a.bg = d.background_id;
    a.code = d.code_type; a.vit = d.variance_in_target != 0;
    a.conf_t = d.conf_thresh; a.nms_t = d.nms_thresh; a.eta = d.nms_eta;
    HIP_TRY(launch_detout_f32(op->form, a, (hipStream_t)stream));
    return SABER_HIP_OK;
}
