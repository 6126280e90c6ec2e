// anakin_amd/csrc/api_autotune.hip - saber_hip_conv2d_autotune, saber_hip_conv2d_autotune_pair and the timing loop they share with
// saber_hip_net_autotune.
#include "api_internal.h"

namespace saber_api {
thread_local ColdBench* g_cold = nullptr;
thread_local std::vector<unsigned long long>* g_used_kernels = nullptr;

int time_enqueued(hipStream_t s, const std::function<int()>& fn, int warm_iters, float* t) {
    if (g_cold) {   // operands cold in L2, as inside the op list
        *t = g_cold->run(s, fn);
        return *t < 0.f ? SABER_HIP_RUNTIME_ERROR : SABER_HIP_OK;
    }
    EventPair ev;
    HIP_TRY(ev.init());
    int rc = fn();   // warm-up; a variant that does not launch is skipped
    if (rc) return rc;
    HIP_TRY(hipEventRecord(ev.e0, s));
    for (int i = 0; i < warm_iters; ++i) rc |= fn();
    HIP_TRY(hipEventRecord(ev.e1, s));
    HIP_TRY(hipEventSynchronize(ev.e1));
    HIP_TRY(hipEventElapsedTime(t, ev.e0, ev.e1));
    return rc;
}
}  // namespace saber_api

// RUNTIME strategy (BaseFunc::pick_best_runtime, saber/funcs/base.h:194,205-247): time every kernel variant for_each_candidate offers
// (implicit-GEMM tiles x stage depths x stagings, stem, LDS-halo, small-image, ...) on the real tensors through `run`, which launches the
// op's CURRENT selection, and keep the fastest. A variant that fails to launch is skipped (its error is kept only if nothing works: the
// entry selection is then restored). Ends with one launch of the selected kernel.
static int tune(saber_hip_conv* op, hipStream_t s, int iters, const std::function<int()>& run) {
    const ConvSel entry = op->sel;
    ConvSel best_c = entry;
    float best = 1e30f;
    int err = SABER_HIP_OK;
    std::vector<std::pair<float, ConvSel>> cands;
    const char* log_env = std::getenv("SABER_HIP_AUTOTUNE_LOG");
    const bool log_cands = g_cold && log_env && log_env[0] == '1';      // SABER_HIP_AUTOTUNE_LOG=1: every candidate and its cold-L2 median
    for_each_candidate(op, &best_c, [&](const ConvSel& c) {
        float t = -1.f;
        int rc = sel_set(op, c);
        if (rc) return;      // (its on-demand buffers could not be made)
        rc = time_enqueued(s, run, iters, &t);
        if (log_cands)
            std::fprintf(stderr, "autotune [%dx%dx%d c%d k%d %dx%d] %-40s %8.2f us\n", op->d.n, op->d.h, op->d.w, op->d.c, op->d.k, op->d.kh,
                         op->d.kw, op->algo_name.c_str(), t);
        if (rc) { err = rc; return; }
        cands.emplace_back(t, c);
        if (t < best) {
            best = t;
            best_c = c;
        }
    });
    if (best >= 1e30f) {
        (void)sel_set(op, entry);
        return err ? err : fail(SABER_HIP_RUNTIME_ERROR, "autotune: no variant ran");
    }
    // prefer a kernel function the net already uses when it is within g_reuse_tol of the fastest (see g_used_kernels; the depthwise forms
    // have never taken part)
    if (g_used_kernels && !dw_ok(op)) {
        float reuse_best = best * (1.f + g_reuse_tol);
        for (const auto& cd : cands) {
            const unsigned long long key = sel_kernel_key(op, cd.second);
            if (cd.first <= reuse_best && std::find(g_used_kernels->begin(), g_used_kernels->end(), key) != g_used_kernels->end()) {
                reuse_best = cd.first;
                best_c = cd.second;
            }
        }
        g_used_kernels->push_back(sel_kernel_key(op, best_c));
    }
    const int rc = sel_set(op, best_c);
    if (rc) return rc;
    sel_release_unused(op);
    return run();   // the outputs hold one clean result of the selected kernel
}

// Leaves y with one clean output of the selected kernel - except for RES_SUM_INPLACE ops, whose timed launches accumulate into y (the
// caller re-initialises it).
int saber_hip_conv2d_autotune(saber_hip_conv_t* op, const void* x, void* y, const void* res, void* workspace,
                                         saber_hip_stream_t stream, int iters) {
    if ((op->algo > ALGO_IGEMM_F32 && !dw_ok(op) && !group_ok(op)) || op->pool_fused || op->gpool) return SABER_HIP_OK;   // (one fused conv+pooling kernel)
    if (op->pair_k2) return fail(SABER_HIP_INVALID_VALUE, "sibling pair: use saber_hip_conv2d_autotune_pair");
    if (op->sel.fam == FAM_FC_SMALL) return SABER_HIP_OK;   // small-batch fc: one launch at the latency floor, nothing to tune
    hipStream_t s = (hipStream_t)stream;
    ColdScope scope;
    HIP_TRY(scope.enter(7));
    return tune(op, s, iters, [&] { return saber_hip_conv2d_run(op, x, y, res, workspace, s); });
}

int saber_hip_conv2d_autotune_pair(saber_hip_conv_t* op, const void* x, void* y_a, void* y_b, saber_hip_stream_t stream,
                                   int iters) {
    if (!op || !op->pair_k2) return fail(SABER_HIP_INVALID_VALUE, "not a sibling pair");
    hipStream_t s = (hipStream_t)stream;
    ColdScope scope;
    HIP_TRY(scope.enter(7));
    return tune(op, s, iters, [&] { return saber_hip_conv2d_run_pair(op, x, y_a, y_b, s); });
}
