// anakin_amd/csrc/api_resize.hip - resize (saber_hip_resize_*): the reference's Resize<T, AK_FLOAT> (saber/funcs/resize.h; x86
// saber_resize.cpp, four ResizeType modes). FP32 only - the reference instantiates AK_FLOAT alone. A type of its own: the conv selection
// tables know nothing of it. create computes which rows / columns every output row / column reads on the HOST, in the reference's float
// steps (resize_axis_table, resize.hip); the kernels only read those tables.
#include "api_internal.h"

bool resize_form_valid(const saber_hip_resize* op, int form) {
    const bool rows = resize_rows_ok(op->d.c, op->d.in_layout == SABER_HIP_NCHW, op->d.out_layout == SABER_HIP_NCHW);
    return form == 0 || (form == 1 && rows) || (form == 2 && rows && op->x2_ok);
}
void for_each_resize_form(const saber_hip_resize* op, const std::function<void(int form)>& fn) {
    for (int f = 0; f <= 2; ++f)
        if (resize_form_valid(op, f)) fn(f);
}
// The static rule (profiles/resize/README.md, 20 row x batch combinations; cold and warm protocols, a form is named only where it is ahead
// by at least a tenth on BOTH):
//   resize_rows_f32 is ahead of form 0 on all 12 measured combinations with 1 384 448 output elements or more (by 1.4 - 3.1 x)
//   and on none of the 8 with 802 816 or fewer - there every form sits on the ~7 us floor of a launch;
//   resize_x2_f32 is ahead of form 1 on the 3 x2 combinations with 3 211 264 output elements or more (by 11 - 27 %) and on none of the 9 with
//   2 768 896 or fewer (behind form 1 on two of them, warm).
// Every measured combination agrees with a threshold between the two figures of each pair; below the first, and where the op accepts neither
// form, form 0.
constexpr double RESIZE_ROWS_MIN_ELEMS = 1.0e6, RESIZE_X2_MIN_ELEMS = 3.0e6;
int resize_static_form(const saber_hip_resize* op) {
    const double elems = (double)op->d.n * op->d.c * op->oh * op->ow;
    if (resize_form_valid(op, 2) && elems >= RESIZE_X2_MIN_ELEMS) return 2;
    return resize_form_valid(op, 1) && elems >= RESIZE_ROWS_MIN_ELEMS ? 1 : 0;
}
// ... and for a resize + sum site: on - the one launch was ahead of the two launches on every measured combination, on both protocols, with
// every form.
bool resize_sum_static_on(const saber_hip_resize*) { return true; }
static const char* resize_form_name(int form) { return form == 2 ? "resize_x2_f32" : (form == 1 ? "resize_rows_f32" : "resize_direct_f32"); }
static int resize_set_form(saber_hip_resize* op, int form) {      // the one writer of op->form
    if (!resize_form_valid(op, form))
        return fail(SABER_HIP_INVALID_VALUE, "resize: no such form for this op (0 direct; 1 rows: NHWC f32 in and out, c % 4 == 0; 2 x2: as 1, modes 1 and 3, out = 2 x in on both axes)");
    op->form = form;
    op->algo_name = resize_form_name(form);
    return SABER_HIP_OK;
}

int saber_hip_resize_create(const saber_hip_resize_desc* desc, saber_hip_resize_t** out) {
    if (!desc || !out) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    *out = nullptr;
    const saber_hip_resize_desc& d = *desc;
    if (d.n <= 0 || d.c <= 0 || d.h <= 0 || d.w <= 0) return fail(SABER_HIP_INVALID_VALUE, "resize: non-positive size");
    if (d.mode < 0 || d.mode > 3) return fail(SABER_HIP_INVALID_VALUE, "resize: mode is 0 BILINEAR_ALIGN, 1 BILINEAR_NO_ALIGN, 2 RESIZE_CUSTOM or 3 NEAREST_ALIGN");
    if (d.dtype != SABER_HIP_F32) return fail(SABER_HIP_UNIMPL, "resize: FP32 only (the reference instantiates AK_FLOAT alone)");
    if ((d.in_layout != SABER_HIP_NHWC && d.in_layout != SABER_HIP_NCHW) || (d.out_layout != SABER_HIP_NHWC && d.out_layout != SABER_HIP_NCHW))
        return fail(SABER_HIP_INVALID_VALUE, "resize: layout is NHWC or NCHW");
    // Resize::compute_output_shape: out_h / out_w where BOTH are given, else floor(in * scale) - a float product
    const bool sizes = d.out_h != -1 && d.out_w != -1;
    const bool scales = d.scale_h > 0.f && d.scale_w > 0.f;
    if (!sizes && !scales) return fail(SABER_HIP_INVALID_VALUE, "resize: neither out_h / out_w nor positive scales");
    long long oh = d.out_h, ow = d.out_w;
    if (!sizes) {
        volatile float ph = (float)d.h * d.scale_h, pw = (float)d.w * d.scale_w;
        const double fh = std::floor((double)ph), fw = std::floor((double)pw);
        oh = fh >= 1.0 && fh < 2.0e9 ? (long long)fh : 0;
        ow = fw >= 1.0 && fw < 2.0e9 ? (long long)fw : 0;
    }
    if (oh <= 0 || ow <= 0 || oh > 0x7fffffffLL || ow > 0x7fffffffLL) return fail(SABER_HIP_INVALID_VALUE, "resize: non-positive output size");
    if ((double)d.n * d.c * oh * ow >= 9.0e18 || (double)d.n * d.c * d.h * d.w >= 9.0e18) return fail(SABER_HIP_INVALID_VALUE, "resize: tensor too large");
    if ((d.mode == 0 || d.mode == 3) && (oh == 1 || ow == 1))
        return fail(SABER_HIP_INVALID_VALUE, "resize: modes 0 and 3 need more than one output row and column (the reference divides by out - 1)");
    std::unique_ptr<saber_hip_resize> op(new saber_hip_resize());
    op->d = d;
    op->oh = (int)oh;
    op->ow = (int)ow;
    if (!resize_axis_table(d.mode, d.h, op->oh, d.scale_h, sizes, op->th) || !resize_axis_table(d.mode, d.w, op->ow, d.scale_w, sizes, op->tw))
        return fail(SABER_HIP_INVALID_VALUE, "resize: an output row or column would read at or beyond the end of the input (or no positive scale)");
    op->x2_ok = (d.mode == 1 || d.mode == 3) && oh == 2LL * d.h && ow == 2LL * d.w && resize_x2_tables_ok(d.mode == 3, d.h, op->th) &&
                resize_x2_tables_ok(d.mode == 3, d.w, op->tw);
    (void)resize_set_form(op.get(), resize_static_form(op.get()));
    *out = op.release();
    return SABER_HIP_OK;
}

void saber_hip_resize_out_shape(const saber_hip_resize_t* op, int* oh, int* ow) {
    if (oh) *oh = op ? op->oh : 0;
    if (ow) *ow = op ? op->ow : 0;
}
const char* saber_hip_resize_algo(const saber_hip_resize_t* op) { return op ? op->algo_name.c_str() : ""; }
int saber_hip_resize_set_tile(saber_hip_resize_t* op, int form) {
    if (!op) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    return resize_set_form(op, form);
}
int saber_hip_resize_get_tile(const saber_hip_resize_t* op) { return op ? op->form : 0; }
void saber_hip_resize_destroy(saber_hip_resize_t* op) { delete op; }

int resize_prepare(saber_hip_resize* op) {
    if (op->d_th.p && op->d_tw.p) return SABER_HIP_OK;
    HIP_TRY(op->d_th.upload(op->th));
    HIP_TRY(op->d_tw.upload(op->tw));
    return SABER_HIP_OK;
}

static int resize_launch(saber_hip_resize* op, const void* x, const void* b, float c0, float c1, int relu, void* y, hipStream_t s) {
    int rc = resize_prepare(op);
    if (rc) return rc;
    const saber_hip_resize_desc& d = op->d;
    ResizeKArgs a{};
    a.x = (const float*)x;
    a.b = (const float*)b;
    a.y = (float*)y;
    a.th = op->d_th.p;
    a.tw = op->d_tw.p;
    a.N = d.n; a.C = d.c; a.H = d.h; a.W = d.w; a.OH = op->oh; a.OW = op->ow;
    a.nearest = d.mode == 3;
    a.in_nchw = d.in_layout == SABER_HIP_NCHW; a.out_nchw = d.out_layout == SABER_HIP_NCHW;
    a.relu = relu; a.c0 = c0; a.c1 = c1;
    HIP_TRY(launch_resize_f32(op->form, a, s));
    return SABER_HIP_OK;
}

int saber_hip_resize_run(saber_hip_resize_t* op, const void* x, void* y, saber_hip_stream_t stream) {
    if (!op || !x || !y) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    if (g_capture) return capture_resize(op, x, y);
    return resize_launch(op, x, nullptr, 0.f, 0.f, 0, y, (hipStream_t)stream);
}

int saber_hip_resize_run_sum(saber_hip_resize_t* op, const void* x, const void* b, float c0, float c1, int relu, void* y, saber_hip_stream_t stream) {
    if (!op || !x || !b || !y) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    if (g_capture) return capture_unsupported("saber_hip_resize_run_sum (record saber_hip_resize_run and saber_hip_eltwise_sum_f32; flag 131072 joins them)");
    return resize_launch(op, x, b, c0, c1, relu ? 1 : 0, y, (hipStream_t)stream);
}
