// anakin_amd/csrc/api_net_autotune.hip - whole-net autotuner and the kernel-selection save / restore entry points.
#include "api_internal.h"

// The kernel selection of op `index` in saber_hip_conv2d_get_tile / set_tile encoding (0 for ops without one): lets a caller
// carry an autotuned selection from one process to the next (bench.py --tune-cache: every profiling pass runs the SAME
// kernels).
static saber_hip_conv* net_op_conv(saber_hip_net* net, int index) {
    if (index < 0 || index >= (int)net->ops.size()) return nullptr;
    NetOp& o = net->ops[index];
    if (o.kind == OP_CONV || o.kind == OP_CONV_PAIR) return o.conv;
    if (o.kind == OP_FC || o.kind == OP_FC_Q) return o.fc ? o.fc->conv : nullptr;
    return nullptr;
}
// bits 0..23: saber_hip_conv2d_get_tile of the op; chain heads add bit 28 (a chain decision is recorded) and the chain's
// pixel fragments in bits 24..27 (0: run as two launches). A depthwise op never heads a chain: bits 28 AND 29 together on it say that a
// separable decision is recorded (flag 16384), bits 24..27 then hold the separable launch's form code (0: two launches).
// Bit 31 WITHOUT bit 30 on the 1x1 expand op of an inverted-residual site (flag 32768): a block decision is recorded, bits 24..27 hold the block
// launch's form code (0: three launches). No op reports that pattern otherwise: bit 31 is the tail bit of a stage head and comes only with
// bit 30, a plain 1x1 conv without residual heads no chain (bit 28), leads none (bit 29) and is no depthwise op (28 and 29) - and a word
// with bit 31 but not bit 30 changed nothing on any op before the flag existed.
int saber_hip_net_get_choice(saber_hip_net_t* net, int index) {
    if (net && index >= 0 && index < (int)net->ops.size() && net->ops[index].kind == OP_DECONV)
        return (18 << 16) | saber_hip_deconv2d_get_tile(net->ops[index].deconv);      // a deconv op: variant 18, its form code in the low byte
    if (net && index >= 0 && index < (int)net->ops.size() && net->ops[index].kind == OP_DETOUT)
        return (20 << 16) | saber_hip_detout_get_tile(net->ops[index].detout);      // a detout op: variant 20, its form code in the low byte
    if (net && index >= 0 && index < (int)net->ops.size() && net->ops[index].kind == OP_RESIZE) {      // a resize op: variant 19, its form code in the low byte; bit 8: its resize + sum site is on
        const NetOp& o = net->ops[index];
        return (19 << 16) | (o.rsum && o.rsum_on ? 1 << 8 : 0) | saber_hip_resize_get_tile(o.resize);
    }
    saber_hip_conv* c = net_op_conv(net, index);
    int choice = (c && !c->pool_fused && (c->algo <= ALGO_IGEMM_F32 || dw_ok(c) || group_ok(c))) ? saber_hip_conv2d_get_tile(c) : 0;
    if (!c) return choice;
    const NetOp& o = net->ops[index];
    if (o.chain) choice |= (1 << 28) | ((o.chain_on ? o.chain->form.code : 0) << 24);
    if (o.chain3) choice |= (1 << 29) | ((o.led_on ? o.chain3->form.code : 0) << 24);      // (a strided head reports its own decision while it runs as a tail)
    if (o.sep) choice |= (3 << 28) | ((o.sep_on ? o.sep->form : 0) << 24);
    if (o.ir) choice |= (int)0x80000000u | ((o.ir_on ? o.ir->form : 0) << 24);
    if (o.fire) choice |= (int)0x80000000u | ((o.fire_on ? o.fire->form : 0) << 24);      // (the squeeze op of a Fire site, flag 65536: the same pattern; no op heads both)
    if (o.stage && o.stage_on) choice |= 1 << 30;      // this op launches its whole stage
    if (o.stage && o.stage_on && o.tail_on) choice |= (int)0x80000000u;      // ... and the strided head behind it as the launch's tail
    // bit 29 on a sibling-pair op (which never leads a chain: bits 24..29 mean nothing else there): the pair runs as the HEAD of the stage launch behind it
    if (o.head_of >= 0 && net->ops[o.head_of].stage_on && net->ops[o.head_of].head_on) choice |= 1 << 29;
    return choice;
}
int saber_hip_net_stage_blocks(const saber_hip_net_t* net, int index) {
    if (!net || index < 0 || index >= (int)net->ops.size()) return 0;
    // (the res2 site, C = 64, reports its blocks NEGATIVE: callers that walk "every stage" - written before the site existed - pass it by, it has
    // a selector of its own)
    const NetOp& o = net->ops[index];
    return o.stage ? (o.stage->c1 == 64 ? -o.stage_n : o.stage_n) : 0;
}
int saber_hip_net_stage_head(const saber_hip_net_t* net, int index) {
    if (!net || index < 1 || index >= (int)net->ops.size() || !net->ops[index].stage) return -1;
    return net->ops[index - 1].head_of == index ? index - 1 : -1;
}
int saber_hip_net_set_choice(saber_hip_net_t* net, int index, int choice) {
    if (net && index >= 0 && index < (int)net->ops.size() && net->ops[index].kind == OP_DECONV) {
        if (net->reproducible_fp32 || ((choice >> 16) & 0xff) != 18) return SABER_HIP_OK;      // flag 8192: FP32 ops keep the static selection; a word without a deconv decision changes nothing
        const int rc = saber_hip_deconv2d_set_tile(net->ops[index].deconv, choice & 0xffff);
        if (rc) return rc;
        net_resolve(net);
        net_drop_graph(net);
        return SABER_HIP_OK;
    }
    if (net && index >= 0 && index < (int)net->ops.size() && net->ops[index].kind == OP_DETOUT) {
        if (((choice >> 16) & 0xff) != 20) return SABER_HIP_OK;      // a word without a detout decision changes nothing (flag 8192 does not hold it back: both forms compute the same bits)
        const int rc = saber_hip_detout_set_tile(net->ops[index].detout, choice & 0xff);
        if (rc) return rc;
        net_resolve(net);
        net_drop_graph(net);
        return SABER_HIP_OK;
    }
    if (net && index >= 0 && index < (int)net->ops.size() && net->ops[index].kind == OP_RESIZE) {
        if (((choice >> 16) & 0xff) != 19) return SABER_HIP_OK;      // a word without a resize decision changes nothing (flag 8192 does not hold it back: every form computes the same bits)
        const int rc = saber_hip_resize_set_tile(net->ops[index].resize, choice & 0xff);
        if (rc) return rc;
        net_set_resize_sum(net, index, (choice >> 8) & 1);      // (resolves; an op that heads no site ignores it)
        net_resolve(net);
        net_drop_graph(net);
        return SABER_HIP_OK;
    }
    saber_hip_conv* c = net_op_conv(net, index);
    // the block decision this choice carries (bit 31 without bit 30 on the expand op of a site); a code with no form for that block is refused
    // before anything changes. An expand op on the direct path (Cin % 16 == 8) has no selection of its own: the decision is all its word holds
    const bool ir_bits = c && net->ops[index].ir && ((unsigned)choice >> 30) == 2u;
    const int ir_tn = (choice >> 24) & 15;
    if (ir_bits && ir_tn && !ir_form_valid(net->ops[index].ir, ir_tn)) return saber_hip_conv2d_ir_set_tile(net->ops[index].ir, ir_tn);      // (its status and message)
    const bool fire_bits = c && net->ops[index].fire && ((unsigned)choice >> 30) == 2u;
    if (fire_bits && ir_tn && !fire_form_valid(net->ops[index].fire, ir_tn)) return saber_hip_conv2d_fire_set_tile(net->ops[index].fire, ir_tn);
    if (fire_bits && !(choice & 0xffffff)) {
        net_set_fire(net, index, ir_tn);
        net_drop_graph(net);
        return SABER_HIP_OK;
    }
    if (ir_bits && !(choice & 0xffffff)) {
        net_set_ir(net, index, ir_tn);
        net_drop_graph(net);
        return SABER_HIP_OK;
    }
    if (!c || !choice || c->pool_fused || (c->algo > ALGO_IGEMM_F32 && !dw_ok(c) && !group_ok(c))) return SABER_HIP_OK;
    if (net->reproducible_fp32 && !c->is_i8) return SABER_HIP_OK;      // flag 8192: a restored selection does not move FP32 ops either
    if (net->ops[index].kind == OP_CONV_PAIR && index > 0 && net->ops[index - 1].stem_pair) return SABER_HIP_OK;      // no kernel of its own (flag 512)
    const int chain_bits = (choice >> 24) & 63;
    const bool stage_on = ((choice >> 30) & 1) && !net->shared_device;
    const bool tail_on = stage_on && (((unsigned)choice >> 31) & 1u);      // (ignored on a stage without a tail)
    choice &= 0xffffff;
    // a selection tuned on a net that owned its device: placement-dependent variants are mapped to their plain forms (bf16-plane kernel: split-K off)
    if (net->shared_device && ((choice >> 16) & 0xff) == 11) choice &= ~(0xf << 12);
    NetOp& o = net->ops[index];
    // the chain decision this choice carries: a 3x3 head (bit 29) is restored before its chain head (bit 28, the next op): set_choices runs in
    // op order. A code with no form for that chain is refused before anything changes.
    saber_hip_chain* ch = index + 1 >= (int)net->ops.size() ? nullptr : ((o.chain3 && (chain_bits & 32)) ? o.chain3 : ((o.chain && (chain_bits & 16)) ? o.chain : nullptr));
    int tn = chain_bits & 15;      // 0: the chain off
    if (ch && net->shared_device && chain_form(ch, tn).placement) tn = chain_form_plain(ch).code;
    if (ch && tn && !chain_form_valid(ch, tn)) return saber_hip_conv2d_chain_set_tile(ch, tn);      // (its status and message)
    // ... and the separable decision (bits 28 and 29 together on the depthwise op of a site), refused likewise
    const bool sep_bits = o.sep && (chain_bits & 48) == 48;
    if (sep_bits && tn && !sep_form_valid(o.sep, tn)) return saber_hip_conv2d_sep_set_tile(o.sep, tn);      // (its status and message)
    int rc = choice ? saber_hip_conv2d_set_tile(c, choice) : SABER_HIP_OK;
    if (rc) return rc;
    o.res_note.clear();
    o.stage_name_kept = false;
    if (ch && tn) (void)saber_hip_conv2d_chain_set_tile(ch, tn);
    // (a block inside a selected stage - its head came first - stays in the 3x3-led mode the stage launch stands for, whatever form the word
    // recorded while the stage was off: its followers must not launch beside the stage. A strided head that runs as a tail is no such block:
    // its own decision is stored underneath.)
    const bool in_stage = o.chain3 && o.skip && !o.stage && o.tail_of < 0;
    const int mode = ch ? net_chain_mode(net, ch == o.chain3 ? index + 1 : index) : 0;
    if (ch && ch == o.chain3) net_set_chain_mode(net, index + 1, (tn || in_stage) ? 2 : std::min(mode, 1));
    else if (ch) net_set_chain_mode(net, index, mode == 2 ? 2 : (tn ? 1 : 0));
    // a stage head comes before its blocks and after the pair in front of it (set_choices runs in op order): a stage that was off takes the
    // head the pair's word asked for - and only then: a stage switched on by itself comes without its head
    if (o.stage) net_set_stage(net, index, stage_on);
    if (o.stage) net_set_tail(net, index, tail_on);
    if (o.head_of >= 0) net_set_head(net, o.head_of, (chain_bits & 32) && !net->shared_device);
    if (sep_bits) net_set_sep(net, index, tn);      // (a choice without the bits leaves the site as it is)
    if (ir_bits) net_set_ir(net, index, ir_tn);
    if (fire_bits) net_set_fire(net, index, ir_tn);
    net_resolve(net);      // (the names follow the kernel selection)
    net_drop_graph(net);
    return SABER_HIP_OK;
}

// End-to-end refinement after the per-op tuning: an implicit-GEMM kernel function used by exactly ONE op of the pass is a
// body of code fetched cold once per forward for one launch. For each such op try the functions other ops (of the same
// epilogue class) already run and keep a switch only if the WHOLE forward pass gets faster by >= 0.4 % against two
// measurements of the incumbent - which it does when cold code is expensive on this box (pool's slow boxes: 3-9 us per
// first use) and not when it is cheap (0.3-0.6 us).
static int net_consolidate_kernels(saber_hip_net* net, hipStream_t s) {
    if (net->has_side) return SABER_HIP_OK;
    if (const char* e = std::getenv("SABER_HIP_NO_CONSOLIDATE"))
        if (e[0] == '1') return SABER_HIP_OK;
    struct Site { int op; unsigned long long key; ConvSel choice; };
    auto conv_of = [&](const NetOp& o) -> saber_hip_conv* {
        if (o.launch != LAUNCH_OWN) return nullptr;
        if (o.kind != OP_CONV && o.kind != OP_CONV_PAIR) return nullptr;
        if (net->reproducible_fp32 && o.conv && !o.conv->is_i8) return nullptr;      // flag 8192: this pass moves no FP32 op either
        return (o.conv && !o.conv->pool_fused && o.conv->algo <= ALGO_IGEMM_F32) ? o.conv : nullptr;
    };
    auto collect = [&]() {
        std::vector<Site> v;
        for (int i = 0; i < (int)net->ops.size(); ++i)
            if (saber_hip_conv* c = conv_of(net->ops[i])) v.push_back({i, sel_kernel_key(c, c->sel), c->sel});
        return v;
    };
    EventPair ev;
    HIP_TRY(ev.init());
    auto forward_ms = [&](float* ms) -> int {   // 3 warm-up + 30 timed eager forwards
        int rc = 0;
        for (int i = 0; i < 3 && !rc; ++i) rc = saber_hip_net_run(net, s);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(ev.e0, s));
        for (int i = 0; i < 30 && !rc; ++i) rc = saber_hip_net_run(net, s);
        HIP_TRY(hipEventRecord(ev.e1, s));
        HIP_TRY(hipEventSynchronize(ev.e1));
        HIP_TRY(hipEventElapsedTime(ms, ev.e0, ev.e1));
        return rc;
    };
    std::vector<Site> sites = collect();
    for (size_t si = 0; si < sites.size(); ++si) {
        const Site cur = sites[si];
        if ((cur.key >> 8 & 0xff) != 5) continue;                      // implicit-GEMM tile kernels only
        int uses = 0;
        for (const Site& t : sites) uses += t.key == cur.key;
        if (uses != 1) continue;
        saber_hip_conv* c = conv_of(net->ops[cur.op]);
        std::vector<Site> alts;                                        // distinct functions of the same class in use elsewhere
        for (const Site& t : sites) {
            if (t.op == cur.op || (t.key & 0xff) != (cur.key & 0xff) || (t.key >> 8 & 0xff) != 5 || t.key == cur.key) continue;
            if ((net->ops[t.op].kind == OP_CONV_PAIR) != (net->ops[cur.op].kind == OP_CONV_PAIR)) continue;
            bool dup = false;
            for (const Site& a : alts) dup |= a.key == t.key;
            if (!dup) alts.push_back(t);
        }
        if (alts.empty()) continue;
        float base = 0.f, base2 = 0.f;
        int rc = forward_ms(&base);
        if (rc) return rc;
        ConvSel best_c = cur.choice;
        float best = base;
        for (const Site& a : alts) {
            const ConvSel cc = sel_igemm(cur.choice, a.choice.tile, a.choice.ks, a.choice.dma);
            float ms = 0.f;
            if (sel_set(c, cc) != SABER_HIP_OK) continue;
            if (forward_ms(&ms) != SABER_HIP_OK) { (void)hipGetLastError(); continue; }   // not launchable for this shape
            if (ms < best) { best = ms; best_c = cc; }
        }
        (void)sel_set(c, cur.choice);
        if (best < base * 0.996f) {                                    // confirm against a second look at the incumbent
            rc = forward_ms(&base2);
            if (rc) return rc;
            if (best < base2 * 0.996f) {
                (void)sel_set(c, best_c);
                net_resolve(net);
                sites = collect();
            }
        }
    }
    return saber_hip_net_run(net, s);   // every tensor holds the final selection's result
}

int saber_hip_net_autotune(saber_hip_net_t* net, saber_hip_stream_t stream, int iters) {
    if (net->inplace_external)
        return fail(SABER_HIP_INVALID_VALUE, "autotune: an in-place sum of this captured list accumulates into a tensor of the caller's that the "
                    "list itself never writes - timing passes would change it (run the pass that writes it inside the capture)");
    net_drop_graph(net);      // a captured graph holds the OLD kernel selections: the caller captures again
    auto T = [&](int id) -> void* { return net->ptr(id); };
    ColdScope scope;
    // flush size between timed repetitions: a net whose tensor arena exceeds the 256 MB Infinity Cache finds its weights in no cache
    // from one forward pass to the next - flush that much (up to 512 MB); smaller nets keep the 64 MB L2-only flush
    HIP_TRY(scope.enter(iters < 7 ? 7 : (iters > 15 ? 15 : iters), net->arena_bytes > ((size_t)256 << 20) ? net->arena_bytes : 0));
    std::vector<unsigned long long> used_kernels;
    struct UsedScope {
        UsedScope(std::vector<unsigned long long>* v) { g_used_kernels = g_cold ? v : nullptr; }
        ~UsedScope() { g_used_kernels = nullptr; }
    } used_scope(&used_kernels);
    for (NetOp& o : net->ops) {
        // a pair that runs inside the stem launch (flag 512) has no kernel of its own (one absorbed by a chain launch - flag 1024 -
        // keeps its own for the mode in which the chain is off: it is tuned like any other)
        if (o.kind == OP_CONV_PAIR && o.skip && &o != net->ops.data() && (&o)[-1].stem_pair) continue;
        if (net->reproducible_fp32 && o.conv && !o.conv->is_i8) continue;      // flag 8192: FP32 convs / pairs keep the static selection
        if (net->reproducible_fp32 && o.fc && o.fc->conv && !o.fc->conv->is_i8) continue;
        if (o.kind == OP_CONV_PAIR) {
            int rc = saber_hip_conv2d_autotune_pair(o.conv, T(o.in), T(o.out), T(o.out2), stream, iters);
            if (rc) return rc;
            continue;
        }
        saber_hip_conv* c = o.kind == OP_CONV ? o.conv : ((o.kind == OP_FC || o.kind == OP_FC_Q) ? o.fc->conv : nullptr);
        if (!c) continue;
        const void* xin = T(o.in);
        if (o.kind == OP_FC && o.fc->pre_quant) {   // the GEMM reads the quantised copy in the workspace
            int rq = net_launch(net, o, (hipStream_t)stream);
            if (rq) return rq;
            xin = net->arena + net->ws_off;
        }
        int rc = saber_hip_conv2d_autotune(c, xin, T(o.out), T(o.in2), net->arena + net->ws_off, stream, iters);
        if (rc) return rc;
        o.res_note.clear();
    }
    // deconv ops: every form the op accepts, cold L2, on the real tensors; a bf16-plane form is kept only where it is faster than form 0
    for (NetOp& o : net->ops) {
        if (o.kind != OP_DECONV || net->reproducible_fp32) continue;
        hipStream_t s = (hipStream_t)stream;
        auto run = [&]() -> int { return net_launch(net, o, s); };
        float best = 0.f;
        int best_form = -1;
        for_each_deconv_form(o.deconv, [&](int form) {
            float us = -1.f;
            if (saber_hip_deconv2d_set_tile(o.deconv, form) != SABER_HIP_OK) return;
            if (time_enqueued(s, run, 20, &us) != SABER_HIP_OK) return;
            if (best_form < 0 || us < best) { best = us; best_form = form; }
        });
        if (best_form < 0) return fail(SABER_HIP_RUNTIME_ERROR, "autotune: no form of a deconv op could be timed");
        int rc = saber_hip_deconv2d_set_tile(o.deconv, best_form);
        if (!rc) rc = run();      // the output holds the selected form's result
        if (rc) return rc;
    }
    // resize ops: every form the op accepts, cold L2, on the real tensors; where the op heads a resize + sum site (flag 131072) the one launch
    // against the two launches, the eltwise included, with every form. All candidates write the same bits: nothing here is held back by flag 8192.
    for (size_t i = 0; i < net->ops.size(); ++i) {
        NetOp& o = net->ops[i];
        if (o.kind != OP_RESIZE) continue;
        hipStream_t s = (hipStream_t)stream;
        const bool site = o.rsum && i + 1 < net->ops.size();
        auto run = [&]() -> int { return net_launch(net, net->ops[i], s) | (site ? net_launch(net, net->ops[i + 1], s) : 0); };
        float best = 0.f;
        int best_form = -1;
        bool best_on = false;
        for (int on = 0; on <= (site ? 1 : 0); ++on) {
            if (site) net_set_resize_sum(net, (int)i, on != 0);
            for_each_resize_form(o.resize, [&](int form) {
                float us = -1.f;
                if (saber_hip_resize_set_tile(o.resize, form) != SABER_HIP_OK) return;
                if (time_enqueued(s, run, 20, &us) != SABER_HIP_OK) return;
                if (best_form < 0 || us < best) { best = us; best_form = form; best_on = on != 0; }
            });
        }
        if (best_form < 0) return fail(SABER_HIP_RUNTIME_ERROR, "autotune: no form of a resize op could be timed");
        int rc = saber_hip_resize_set_tile(o.resize, best_form);
        if (site) net_set_resize_sum(net, (int)i, best_on);
        if (!rc) rc = run();      // every written output holds the selected form's result
        if (rc) return rc;
    }
    // detout ops: both forms where the op accepts both, on the real tensors. The forms write the same bits: nothing here is held back by flag 8192.
    for (size_t i = 0; i < net->ops.size(); ++i) {
        NetOp& o = net->ops[i];
        if (o.kind != OP_DETOUT) continue;
        hipStream_t s = (hipStream_t)stream;
        auto run = [&]() -> int { return net_launch(net, net->ops[i], s); };
        float best = 0.f;
        int best_form = -1;
        for_each_detout_form(o.detout, [&](int form) {
            float us = -1.f;
            if (saber_hip_detout_set_tile(o.detout, form) != SABER_HIP_OK) return;
            if (time_enqueued(s, run, 20, &us) != SABER_HIP_OK) return;
            if (best_form < 0 || us < best) { best = us; best_form = form; }
        });
        if (best_form < 0) return fail(SABER_HIP_RUNTIME_ERROR, "autotune: no form of a detout op could be timed");
        int rc = saber_hip_detout_set_tile(o.detout, best_form);
        if (!rc) rc = run();      // both outputs hold the selected form's result
        if (rc) return rc;
    }
    net_resolve(net);      // (the names of the tuned selections)
    const char* log_env = std::getenv("SABER_HIP_AUTOTUNE_LOG");
    const bool log_cands = g_cold && log_env && log_env[0] == '1';      // every timed chain / stage candidate, in the per-op tuner's format
    auto log_cand = [&](const saber_hip_conv* c, const std::string& name, float t) {
        if (log_cands) std::fprintf(stderr, "autotune [%dx%dx%d c%d k%d %dx%d] %-40s %8.2f us\n", c->d.n, c->d.h, c->d.w, c->d.c, c->d.k, c->d.kh, c->d.kw, name.c_str(), t);
    };
    // conv1x1 chains: the tuned separate launches against the chain launch (every pixel-tile size) and, where the block's
    // 3x3 conv can lead the chain, against that single launch too - on the real tensors
    for (size_t i = 0; i < net->ops.size(); ++i)
        if (net->ops[i].stage) net_set_stage(net, (int)i, false);      // (block by block first; the stages after this loop)
    for (size_t i = 0; i < net->ops.size(); ++i) {
        NetOp& A = net->ops[i];
        const int ia = (int)i;
        NetOp* H = (ia > 0 && net->ops[ia - 1].chain3) ? &net->ops[ia - 1] : nullptr;
        if (!A.chain && !H) continue;
        const int first = H ? ia - 1 : ia;
        const int last = (A.chain || (H && H->chain3->b2)) ? ia + 1 : ia;      // (a head + pair chain also replaces the pair op behind A)
        hipStream_t s = (hipStream_t)stream;
        auto run_all = [&]() -> int {
            int rc = 0;
            for (int k = first; k <= last; ++k) rc |= net_launch(net, net->ops[k], s);
            return rc;
        };
        auto timed = [&](float* t) { return time_enqueued(s, run_all, 20, t); };      // (SABER_HIP_AUTOTUNE_WARM: 20 back-to-back repetitions)
        float best = 0.f;
        int best_mode = 0, best_tn = 0;
        net_set_chain_mode(net, ia, 0);
        int rc = timed(&best);
        if (rc) return rc;
        log_cand(A.conv, "separate", best);
        for (int mode = A.chain ? 1 : 2; mode <= (H ? 2 : 1); ++mode) {
            saber_hip_chain* ch = mode == 2 ? H->chain3 : A.chain;
            for_each_chain_candidate(ch, net->shared_device, [&](const ChainForm& f) {
                float ms = -1.f;
                if (saber_hip_conv2d_chain_set_tile(ch, f.code) != SABER_HIP_OK) return;
                net_set_chain_mode(net, ia, mode);
                const int rt = timed(&ms);
                log_cand(A.conv, (mode == 2 ? H->name : A.name).substr(5), ms);
                if (rt == SABER_HIP_OK && ms < best) { best = ms; best_mode = mode; best_tn = f.code; }
            });
        }
        if (best_mode) (void)saber_hip_conv2d_chain_set_tile(best_mode == 2 ? H->chain3 : A.chain, best_tn);
        net_set_chain_mode(net, ia, best_mode);
        rc = run_all();   // every written output holds the selected form's result
        if (rc) return rc;
    }
    // stages: the blocks' tuned launches one after the other against the one persistent launch; where the strided head behind the run can be
    // the launch's tail, the head's ops are timed with them: blocks and head on their own | stage + head | stage with tail. Where the sibling
    // pair in front of the run can be the launch's head, the pair op is timed with every form, and the best stage form then runs once more
    // with the head: pair + stage | stage with head
    for (size_t i = 0; i < net->ops.size(); ++i) {
        NetOp& H0 = net->ops[i];
        if (!H0.stage || net->shared_device) continue;
        const bool has_tail = H0.stage->tail != nullptr;
        const bool has_head = saber_hip_net_stage_head(net, (int)i) >= 0;
        const int first = (int)i, last = first + 3 * H0.stage_n - 1 + (has_tail ? 2 : 0);
        hipStream_t s = (hipStream_t)stream;
        auto run_all = [&]() -> int {
            int rc = 0;
            for (int k = first - (has_head ? 1 : 0); k <= last; ++k) rc |= net_launch(net, net->ops[k], s);
            return rc;
        };
        auto timed = [&](float* t) { return time_enqueued(s, run_all, 20, t); };
        std::vector<int> modes(H0.stage_n), tns(H0.stage_n);
        for (int k = 0; k < H0.stage_n; ++k) {
            modes[k] = net_chain_mode(net, first + 3 * k + 1);
            tns[k] = net->ops[first + 3 * k].chain3->form.code;
        }
        float sep = 0.f, one = 0.f;
        int rc = timed(&sep);
        if (rc) return rc;
        log_cand(H0.conv, "separate", sep);
        net_set_stage(net, first, true);
        net_set_tail(net, first, false);
        bool ok = timed(&one) == SABER_HIP_OK && hipStreamSynchronize(s) == hipSuccess && !*(volatile unsigned*)H0.stage->h_err;
        log_cand(H0.conv, H0.name.substr(5), ok ? one : -1.f);
        if (ok && has_tail) {
            float wt = 0.f;
            net_set_tail(net, first, true);
            const bool ok_t = timed(&wt) == SABER_HIP_OK && hipStreamSynchronize(s) == hipSuccess && !*(volatile unsigned*)H0.stage->h_err;
            log_cand(H0.conv, H0.name.substr(5), ok_t ? wt : -1.f);
            if (*(volatile unsigned*)H0.stage->h_err) ok = false;      // (a launch that did not complete: the site falls back as a whole)
            else if (ok_t && wt < one) one = wt;
            else net_set_tail(net, first, false);
        }
        if (ok && one < sep && has_head) {
            float wh = 0.f;
            net_set_head(net, first, true);
            const bool ok_h = timed(&wh) == SABER_HIP_OK && hipStreamSynchronize(s) == hipSuccess && !*(volatile unsigned*)H0.stage->h_err;
            log_cand(H0.conv, H0.name.substr(5), ok_h ? wh : -1.f);
            if (*(volatile unsigned*)H0.stage->h_err) ok = false;      // (a launch that did not complete: the site falls back as a whole)
            // (kept only where it wins by more than 1 %: two cold medians of ONE form differ by up to about that - the log shows the same candidate
            // at 23.08 and 23.28 us - and a tie keeps the pair's own launch, which needs no other workgroup's arrival)
            else if (ok_h && wh < one * 0.99f) one = wh;
            else net_set_head(net, first, false);
        }
        // (the res2 stage, C = 64, is kept only where it wins by more than 1 %: what two cold medians of one form differ by)
        if (!ok || one >= sep * (H0.stage->c1 == 64 ? 0.99f : 1.f)) {
            *(volatile unsigned*)H0.stage->h_err = 0u;
            net_set_stage(net, first, false);
            for (int k = 0; k < H0.stage_n; ++k) {
                (void)saber_hip_conv2d_chain_set_tile(net->ops[first + 3 * k].chain3, tns[k]);
                net_set_chain_mode(net, first + 3 * k + 1, modes[k]);
            }
        }
        rc = run_all();   // every written output holds the selected form's result
        if (rc) return rc;
    }
    // separable sites (flag 16384): the two tuned launches against every form of the one launch, cold L2, on the real tensors
    for (size_t i = 0; i + 1 < net->ops.size(); ++i) {
        NetOp& D = net->ops[i];
        if (!D.sep) continue;
        hipStream_t s = (hipStream_t)stream;
        auto run_all = [&]() -> int { return net_launch(net, net->ops[i], s) | net_launch(net, net->ops[i + 1], s); };
        auto timed = [&](float* t) { return time_enqueued(s, run_all, 20, t); };
        float best = 0.f;
        int best_code = 0;
        net_set_sep(net, (int)i, 0);
        int rc = timed(&best);
        if (rc) return rc;
        log_cand(D.conv, "separate", best);
        for_each_sep_form(D.sep, [&](int code) {
            float us = -1.f;
            net_set_sep(net, (int)i, code);
            const int rt = timed(&us);
            log_cand(D.conv, D.name.substr(5), us);
            if (rt == SABER_HIP_OK && us < best) { best = us; best_code = code; }
        });
        net_set_sep(net, (int)i, best_code);
        rc = run_all();   // every written output holds the selected form's result
        if (rc) return rc;
    }
    // inverted-residual sites (flag 32768): the three tuned launches against every form of the one launch, cold L2, on the real tensors
    for (size_t i = 0; i + 2 < net->ops.size(); ++i) {
        NetOp& E = net->ops[i];
        if (!E.ir) continue;
        hipStream_t s = (hipStream_t)stream;
        auto run_all = [&]() -> int { return net_launch(net, net->ops[i], s) | net_launch(net, net->ops[i + 1], s) | net_launch(net, net->ops[i + 2], s); };
        auto timed = [&](float* t) { return time_enqueued(s, run_all, 20, t); };
        float best = 0.f;
        int best_code = 0;
        net_set_ir(net, (int)i, 0);
        int rc = timed(&best);
        if (rc) return rc;
        log_cand(E.conv, "separate", best);
        for_each_ir_form(E.ir, [&](int code) {
            float us = -1.f;
            net_set_ir(net, (int)i, code);
            const int rt = timed(&us);
            log_cand(E.conv, E.name.substr(5), us);
            if (rt == SABER_HIP_OK && us < best) { best = us; best_code = code; }
        });
        net_set_ir(net, (int)i, best_code);
        rc = run_all();   // every written output holds the selected form's result
        if (rc) return rc;
    }
    // Fire sites (flag 65536): the three tuned convs + the concat against every form of the one launch, cold L2, on the real tensors
    for (size_t i = 0; i + 3 < net->ops.size(); ++i) {
        NetOp& Q = net->ops[i];
        if (!Q.fire) continue;
        hipStream_t s = (hipStream_t)stream;
        auto run_all = [&]() -> int {
            int r = 0;
            for (size_t j = i; j <= i + 3; ++j) r |= net_launch(net, net->ops[j], s);
            return r;
        };
        auto timed = [&](float* t) { return time_enqueued(s, run_all, 20, t); };
        float best = 0.f;
        int best_code = 0;
        net_set_fire(net, (int)i, 0);
        int rc = timed(&best);
        if (rc) return rc;
        log_cand(Q.conv, "separate", best);
        for_each_fire_form(Q.fire, [&](int code) {
            float us = -1.f;
            net_set_fire(net, (int)i, code);
            const int rt = timed(&us);
            log_cand(Q.conv, Q.name.substr(5), us);
            if (rt == SABER_HIP_OK && us < best) { best = us; best_code = code; }
        });
        net_set_fire(net, (int)i, best_code);
        rc = run_all();   // every written output holds the selected form's result
        if (rc) return rc;
    }
    return g_cold ? net_consolidate_kernels(net, (hipStream_t)stream) : SABER_HIP_OK;
}
