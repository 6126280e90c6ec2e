// tests/cpp/test_saber_detout.cpp - SaberDetectionOutput<MI355X, AK_FLOAT> through the Saber interface (init -> create -> dispatch, the
// stand-in headers of include/saber_mi355x.hpp). Inputs with exactly representable boxes (CORNER, variance in the target, multiples of
// 1 / 64) whose result is known in closed form: clusters of three boxes of which NMS keeps the best, the boxes of different clusters far
// apart. Checked: the rows and their order, both forms, the output's shape OUTSIDE an op-list capture ({1, 1, kept, 7}, and {1, 1, 1, 7}
// with a row of -1 when nothing is kept) and INSIDE one (the capacity shape, nothing launched, nothing read back; the recorded list then
// writes the rows and the -1 padding), the two-input arrangement, and the descriptors the op refuses.
// Built with the other C++ tests; run on the GPU by tests/test_gpu_detout.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "saber_mi355x.hpp"

using namespace anakin::saber;

static int g_fail = 0, g_run = 0;
static void expect(bool ok, const char* what) {
    ++g_run;
    if (!ok) { ++g_fail; printf("FAIL %s\n", what); }
}

// N images, G clusters of three priors each, C classes with class 0 the background. Cluster g sits at x = g / 4; its priors are the same box
// shifted by 0, 1 / 64 and 2 / 64 (overlap well above 0.45). In image n and class c the scores of cluster g's priors are
// 0.5 + (g + 1) / 64 + {0, 1, 2} / 1024 in an order rotated by (n + c): NMS keeps the one with the top score of each cluster.
struct Case {
    int N, G, C, keep;
    std::vector<float> loc, conf_pc, conf_cp, prior, boxes;
    std::vector<float> want;      // rows
    std::vector<int> per_image;
    Case(int n, int g, int c, int k) : N(n), G(g), C(c), keep(k) {
        const int P = 3 * G;
        loc.assign((size_t)N * P * 4, 0.f);
        prior.assign((size_t)2 * P * 4, 0.f);
        boxes.assign((size_t)N * P * 4, 0.f);
        conf_pc.assign((size_t)N * P * C, 0.f);
        conf_cp.assign((size_t)N * P * C, 0.f);
        for (int p = 0; p < P; ++p) {
            const float x0 = (p / 3) * 0.25f + (p % 3) / 64.f;
            const float b[4] = {x0, 0.25f, x0 + 0.125f, 0.5f};
            for (int k4 = 0; k4 < 4; ++k4) {
                prior[(size_t)p * 4 + k4] = b[k4] - 1.f / 64.f;
                for (int i = 0; i < N; ++i) {
                    loc[((size_t)i * P + p) * 4 + k4] = 1.f / 64.f;      // CORNER, variance in the target: box = prior + loc, exact
                    boxes[((size_t)i * P + p) * 4 + k4] = b[k4];
                }
            }
        }
        for (int i = 0; i < N; ++i) {
            std::vector<std::vector<float>> rows;      // label ascending; inside a label score descending = cluster descending
            for (int cc = 0; cc < C; ++cc)
                for (int gg = G - 1; gg >= 0; --gg)
                    for (int r = 0; r < 3; ++r) {
                        const int p = gg * 3 + r, rank = (r + i + cc) % 3;
                        const float s = 0.5f + (gg + 1) / 64.f + rank / 1024.f;
                        conf_pc[((size_t)i * P + p) * C + cc] = s;
                        conf_cp[((size_t)i * C + cc) * P + p] = s;
                        if (cc > 0 && rank == 2) rows.push_back({(float)i, (float)cc, s, boxes[((size_t)i * P + p) * 4], 0.25f, boxes[((size_t)i * P + p) * 4 + 2], 0.5f});
                    }
            // keep_top_k: score descending, then label ascending; every cluster's winner has the same score in every class
            std::vector<std::vector<float>> cut;
            if ((int)rows.size() > keep) {
                std::vector<int> taken(rows.size(), 0);
                int left = keep;
                for (int gg = G - 1; gg >= 0 && left > 0; --gg)
                    for (size_t q = 0; q < rows.size() && left > 0; ++q)
                        if (rows[q][2] == 0.5f + (gg + 1) / 64.f + 2 / 1024.f) { taken[q] = 1; --left; }
                for (size_t q = 0; q < rows.size(); ++q)
                    if (taken[q]) cut.push_back(rows[q]);
            } else {
                cut = rows;
            }
            per_image.push_back((int)cut.size());
            for (auto& r : cut) want.insert(want.end(), r.begin(), r.end());
        }
    }
    int P() const { return 3 * G; }
};

static bool rows_equal(const std::vector<float>& got, const std::vector<float>& want, size_t rows_total) {
    if (got.size() < rows_total * 7 || want.size() > got.size()) return false;
    if (std::memcmp(got.data(), want.data(), want.size() * 4) != 0) return false;
    for (size_t i = want.size(); i < rows_total * 7; ++i)
        if (got[i] != -1.f) return false;
    return true;
}

static void run_case(const Case& c, bool with_prior, float conf_thresh, Context<MI355X>& ctx) {
    const int P = c.P(), cap = c.N * c.keep;
    Tensor<MI355X> loc(Shape({c.N, P * 4, 1, 1}), AK_FLOAT), conf(with_prior ? Shape({c.N, P, c.C, 1}) : Shape({c.N, c.C, P, 1}), AK_FLOAT),
        prior(Shape({1, 2, P * 4, 1}), AK_FLOAT), out(Shape({1, 1, cap, 7}), AK_FLOAT);
    loc.copy_from_host(with_prior ? c.loc.data() : c.boxes.data());
    conf.copy_from_host(with_prior ? c.conf_pc.data() : c.conf_cp.data());
    prior.copy_from_host(c.prior.data());
    DetectionOutputParam<MI355X> dp(c.C, 0, c.keep, 50, 0.45f, conf_thresh, true, true, (int)CORNER, 1.f);
    std::vector<Tensor<MI355X>*> ins{&loc, &conf}, outs{&out};
    if (with_prior) ins.push_back(&prior);
    const bool empty = conf_thresh > 1.f;
    const std::vector<float> none;
    const std::vector<float>& want = empty ? none : c.want;
    const int total = (int)want.size() / 7;
    SaberDetectionOutput<MI355X, AK_FLOAT> op;
    expect(op.init(ins, outs, dp, ctx) == SaberSuccess, "init");
    for (int form = 0; form < 2; ++form) {
        expect(op.set_tile(form) == 0, "set_tile");
        std::vector<float> fill((size_t)cap * 7, 77.f), got((size_t)cap * 7, 0.f);
        out.reshape(Shape({1, 1, cap, 7}));
        out.copy_from_host(fill.data());
        // outside an op-list capture: the output is reshaped to the rows that were kept
        expect(op.dispatch(ins, outs, dp) == SaberSuccess, "dispatch");
        const Shape sh = out.valid_shape();
        expect(sh.size() == 4 && sh[0] == 1 && sh[1] == 1 && sh[2] == (total ? total : 1) && sh[3] == 7, "shape outside a capture");
        std::vector<int> cnt(1 + c.N, -5);
        op.count_tensor().copy_to_host(cnt.data());
        bool cnt_ok = cnt[0] == total;
        for (int i = 0; i < c.N; ++i) cnt_ok = cnt_ok && cnt[1 + i] == (empty ? 0 : c.per_image[i]);
        expect(cnt_ok, "count");
        out.reshape(Shape({1, 1, cap, 7}));
        out.copy_to_host(got.data());
        expect(rows_equal(got, want, (size_t)cap), "rows outside a capture");
        // inside one: recorded, not launched; the capacity shape stays; the recorded list writes rows and padding
        out.copy_from_host(fill.data());
        saber_hip_net_t* net = nullptr;
        expect(saber_hip_capture_begin() == SABER_HIP_OK, "capture_begin");
        expect(op.dispatch(ins, outs, dp) == SaberSuccess, "dispatch while recording");
        expect(saber_hip_capture_end(&net) == SABER_HIP_OK, "capture_end");
        (void)hipStreamSynchronize(ctx.get_compute_stream());
        const Shape sc = out.valid_shape();
        expect(sc.size() == 4 && sc[2] == cap && sc[3] == 7, "capacity shape inside a capture");
        out.copy_to_host(got.data());
        expect(got[0] == 77.f && got[(size_t)cap * 7 - 1] == 77.f, "nothing launched while recording");
        expect(net && saber_hip_net_num_ops(net) == 1, "one recorded op");
        if (net) {
            expect(saber_hip_net_bind_tensor(net, saber_hip_net_tensor_of_ptr(net, out.data()), out.mutable_data()) == SABER_HIP_OK, "bind the output");
            expect(saber_hip_net_finalize(net) == SABER_HIP_OK, "finalize");
            expect(saber_hip_net_run(net, (saber_hip_stream_t)ctx.get_compute_stream()) == SABER_HIP_OK, "run the recorded list");
            (void)hipStreamSynchronize(ctx.get_compute_stream());
            out.copy_to_host(got.data());
            expect(rows_equal(got, want, (size_t)cap), "rows of the recorded list");
            saber_hip_net_destroy(net);
        }
    }
}

int main() {
    if (!saber_hip_device_ok()) {
        printf("no gfx950 device: the MI355X Saber target has no fallback\n");
        return 2;
    }
    Context<MI355X> ctx(0, 0, 0);
    const Case small(1, 3, 3, 20), cut(3, 4, 4, 5);
    run_case(small, true, 0.3f, ctx);       // fewer rows than the capacity
    run_case(small, false, 0.3f, ctx);      // the two-input arrangement
    run_case(cut, true, 0.3f, ctx);         // every image cut to keep_top_k: all rows filled
    run_case(cut, true, 2.f, ctx);          // nothing kept: one row of -1
    {
        Tensor<MI355X> loc(Shape({1, 36, 1, 1}), AK_FLOAT), conf(Shape({1, 9, 3, 1}), AK_FLOAT), prior(Shape({1, 2, 36, 1}), AK_FLOAT), out(Shape({1, 1, 20, 7}), AK_FLOAT);
        std::vector<Tensor<MI355X>*> ins{&loc, &conf, &prior}, outs{&out};
        DetectionOutputParam<MI355X> ok(3, 0, 20, 50, 0.45f, 0.3f);
        SaberDetectionOutput<MI355X, AK_INT8> op8;
        expect(op8.init(ins, outs, ok, ctx) == SaberUnImplError, "AK_INT8 answers SaberUnImplError");
        DetectionOutputParam<MI355X> two_stage(3, 0, 20, 50, 0.45f, 0.3f, false), no_keep(3, 0, -1, 50, 0.45f, 0.3f), big_nms(3, 0, 20, 2000, 0.45f, 0.3f);
        SaberDetectionOutput<MI355X, AK_FLOAT> a, b, c2;
        expect(a.init(ins, outs, two_stage, ctx) == SaberUnImplError, "share_location = false answers SaberUnImplError");
        expect(b.init(ins, outs, no_keep, ctx) == SaberUnImplError, "keep_top_k = -1 answers SaberUnImplError");
        expect(c2.init(ins, outs, big_nms, ctx) == SaberUnImplError, "nms_top_k = 2000 answers SaberUnImplError");
        expect(a.dispatch(ins, outs, two_stage) == SaberNotInitialized, "dispatch after a refused create");
    }
    printf("%d/%d detout cases ok\n", g_run - g_fail, g_run);
    return g_fail ? 1 : 0;
}
