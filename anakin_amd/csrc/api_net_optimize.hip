// anakin_amd/csrc/api_net_optimize.hip - saber_hip_net_optimize: executor-level fusions.
#include "api_internal.h"

// ------------------------------------------------------------------------------------------------
// Executor-level fusions, host side C++ (north star: "host side stays C++"): the reference's graph optimiser rewrites
// the operator graph before Net::init (framework/graph/llvm/fusion/fusion_op_register.cpp:45-175 is its pattern
// catalogue: Conv+Eltwise, Conv+Pooling, ...); this is the same step for an op list handed to the MI355X executor
// UNFUSED (one op per reference operator). Every rewrite keeps the bytes of every surviving edge identical:
//   1  conv (-> s8, single consumer) + INT8 eltwise sum        -> one conv with the RES_ELTWISE epilogue
//   2  two convs over the same tensor with the same geometry   -> one sibling-pair launch (saber_hip_conv2d_create_pair)
//   4  conv + max pooling (single consumer)                    -> SaberConv2DPooling where a fused kernel exists
//   8  global pooling feeding an INT8 fc that quantises on entry -> the pooling also writes the fc's s8 operand
//  16  1x1 conv with the fused eltwise epilogue + the 1x1 conv that follows it and reads its output (ResNet branch2c + sum
//      -> next branch2a) -> one conv1x1-chain launch (saber_hip_conv2d_chain_create); both ops stay in the list (the
//      second one launches nothing while the chain is selected), the autotuner keeps whichever form is faster
// New ops are re-created from the originals' quantised weights / scales / bias and owned by the net. Call before
// saber_hip_net_finalize. Returns the number of launches removed, or a negative status.
// ------------------------------------------------------------------------------------------------
// Sites: decisions in, derived state out. net_resolve is the only writer of NetOp::launch / absorbed_by / skip and - once the sites are formed -
// of every conv / pair / fc / softmax op's name. Priority: a selected stage covers its blocks, its tail and its head when those are on; below
// that a led chain covers the two ops behind it (the 1x1 chain head and its follower, or the pair); below that the 1x1 chain and the separable
// launch cover the next op. The stem pair and fc + softmax are unconditional. Called when a decision (or a kernel selection, for the names)
// changes - never per pass.
void net_resolve(saber_hip_net* net) {
    std::vector<NetOp>& ops = net->ops;
    const int n = (int)ops.size();
    enum { IN_CHAIN, IN_STAGE, IN_STEM, IN_SEP, IN_IR, IN_FIRE };
    static const char* const covered[] = {"conv:(in the chain launch)", "conv:(in the stage launch)", "conv:(in the stem launch)", "conv:(in the separable launch)",
                                          "conv:(in the inverted-residual launch)", "conv:(in the fire launch)"};
    std::vector<int> in(n, IN_CHAIN);
    for (NetOp& o : ops) {
        o.launch = LAUNCH_OWN;
        o.absorbed_by = -1;
    }
    auto absorb = [&](int j, int by, int what) {
        ops[j].launch = LAUNCH_NONE;
        ops[j].absorbed_by = by;
        in[j] = what;
    };
    for (int i = 0; i < n; ++i) {
        NetOp& o = ops[i];
        if (o.launch == LAUNCH_NONE) continue;      // (an earlier op's launch covers it, whatever it could head itself)
        if ((o.kind == OP_FC || o.kind == OP_FC_Q) && o.out2 >= 0) {
            for (int j = i + 1; j < n; ++j)
                if (ops[j].kind == OP_SOFTMAX && ops[j].out == o.out2) { absorb(j, i, IN_CHAIN); break; }
        }
        if (o.kind == OP_RESIZE && o.rsum && o.rsum_on && i + 1 < n) {      // resize + the eltwise behind it (flag 131072)
            o.launch = LAUNCH_RESIZE_SUM;
            absorb(i + 1, i, IN_CHAIN);
        }
        if (o.kind != OP_CONV || i + 1 >= n) continue;
        if (o.stage && o.stage_on) {
            o.launch = LAUNCH_STAGE;
            for (int k = 0; k < o.stage_n; ++k) {      // (a block's followers keep the name they have behind their own 3x3 conv)
                if (k) absorb(i + 3 * k, i, IN_STAGE);
                absorb(i + 3 * k + 1, i, IN_CHAIN);
                absorb(i + 3 * k + 2, i, IN_CHAIN);
            }
            if (o.tail_on)
                for (int j = i + 3 * o.stage_n; j < i + 3 * o.stage_n + 2; ++j) absorb(j, i, IN_STAGE);
            if (o.head_on) absorb(i - 1, i, IN_STAGE);
        } else if (o.stem_pair) {
            o.launch = LAUNCH_STEM_PAIR;
            absorb(i + 1, i, IN_STEM);
        } else if (o.chain3 && o.led_on) {
            o.launch = LAUNCH_CHAIN3;
            absorb(i + 1, i, IN_CHAIN);
            if (o.chain3->b || o.chain3->b2) absorb(i + 2, i, IN_CHAIN);
        } else if (o.chain && o.chain_on) {
            o.launch = LAUNCH_CHAIN;
            absorb(i + 1, i, IN_CHAIN);
        } else if (o.sep && o.sep_on) {
            o.launch = LAUNCH_SEP;
            absorb(i + 1, i, IN_SEP);
        } else if (o.ir && o.ir_on && i + 2 < n) {      // (no op of an inverted-residual site belongs to another site: formed that way)
            o.launch = LAUNCH_IR;
            absorb(i + 1, i, IN_IR);
            absorb(i + 2, i, IN_IR);
        } else if (o.fire && o.fire_on && i + 3 < n) {      // (no op of a Fire site belongs to another site: formed that way)
            o.launch = LAUNCH_FIRE;
            for (int j = i + 1; j <= i + 3; ++j) absorb(j, i, IN_FIRE);
        }
    }
    for (int i = 0; i < n; ++i) {
        NetOp& o = ops[i];
        o.skip = o.launch == LAUNCH_NONE;
        if (o.kind == OP_CONCAT) {
            o.name = "concat" + std::to_string(o.ins.size()) + (o.skip ? " (in the fire launch)" : "");
        } else if (o.kind == OP_DETOUT) {
            o.name = std::string("detout:") + o.detout->algo_name;
        } else if (o.kind == OP_DECONV) {
            o.name = std::string("deconv:") + o.deconv->algo_name;
        } else if (o.kind == OP_RESIZE) {
            o.name = std::string("resize:") + o.resize->algo_name + (o.launch == LAUNCH_RESIZE_SUM ? "+sum" : "");
        } else if (o.kind == OP_ELT_F32) {
            o.name = o.skip ? "eltwise_sum_f32 (in the resize launch)" : "eltwise_sum_f32";
        } else if (o.kind == OP_SOFTMAX) {
            o.name = o.skip ? "softmax_f32 (in the fc launch)" : "softmax_f32";
        } else if (o.kind == OP_FC || o.kind == OP_FC_Q) {
            o.name = std::string("fc:") + o.fc->conv->algo_name;
            if (o.out2 >= 0) o.name += fc_softmax_ok(o.fc, o.kind == OP_FC_Q) ? "+softmax" : " | softmax_f32";
        } else if (o.kind == OP_CONV || o.kind == OP_CONV_PAIR) {
            const std::string own = o.conv->algo_name;
            const bool kept = o.stage_name_kept && !o.skip;      // (NetOp::stage_name_kept: shown as it was inside the stage launch)
            switch (kept ? (o.stage ? LAUNCH_STAGE : LAUNCH_NONE) : o.launch) {
            case LAUNCH_NONE: o.name = covered[kept ? IN_STAGE : in[i]]; break;
            case LAUNCH_RESIZE_SUM:      // (a resize op's launch, never a conv's)
            case LAUNCH_OWN: o.name = "conv:" + own + o.res_note; break;
            case LAUNCH_CHAIN: o.name = "conv:" + chain_form_name(o.chain); break;
            case LAUNCH_CHAIN3: o.name = "conv:" + chain_form_name(o.chain3); break;
            case LAUNCH_SEP: o.name = std::string("conv:") + saber_hip_conv2d_sep_algo(o.sep); break;
            case LAUNCH_IR: o.name = std::string("conv:") + saber_hip_conv2d_ir_algo(o.ir); break;
            case LAUNCH_FIRE: o.name = std::string("conv:") + saber_hip_conv2d_fire_algo(o.fire); break;
            case LAUNCH_STEM_PAIR: o.name = "conv:" + own + "+pair1x1_" + std::to_string(o.stem_pair->a->d.k) + "+" + std::to_string(o.stem_pair->b->d.k); break;
            case LAUNCH_STAGE:
                o.name = std::string(o.head_on && !kept ? "conv:[pair1x1]+stage_c" : "conv:stage_c") + std::to_string(o.stage->c1) + "_" + std::to_string(o.stage_n) + "x[conv3x3+chain1x1]_2x16" +
                         (o.stage->c1 == 256 ? "_coop4" : "") + (o.tail_on && !kept ? "+[conv3x3/2+conv1x1]" : "");
                break;
            }
        }
    }
}
// The setters store decisions and resolve. ops[ia] = A, a 1x1 conv with the fused eltwise: mode 0 separate launches, 1 A + the next op chained,
// 2 the 3x3 conv ops[ia - 1] leads the launch. A led chain switches the 1x1 chain behind it on as well: that is what runs when it goes off again.
void net_set_chain_mode(saber_hip_net* net, int ia, int mode) {
    NetOp& A = net->ops[ia];
    NetOp* H = (ia > 0 && net->ops[ia - 1].chain3) ? &net->ops[ia - 1] : nullptr;
    if (H) H->led_on = mode == 2;
    if (H) H->stage_name_kept = false;
    A.chain_on = A.chain && mode >= 1;
    A.res_note.clear();
    net_resolve(net);
}
int net_chain_mode(const saber_hip_net* net, int ia) {
    const NetOp& A = net->ops[ia];
    return (ia > 0 && net->ops[ia - 1].chain3 && net->ops[ia - 1].led_on) ? 2 : (A.chain_on ? 1 : 0);
}
void net_set_tail(saber_hip_net* net, int i0, bool on) {
    NetOp& H0 = net->ops[i0];
    if (!H0.stage || !H0.stage->tail) return;
    H0.tail_on = on;
    net_resolve(net);
}
void net_set_head(saber_hip_net* net, int i0, bool on) {
    NetOp& H0 = net->ops[i0];
    if (!H0.stage || !H0.stage->head_a || i0 < 1 || net->ops[i0 - 1].head_of != i0) return;
    H0.head_on = on;
    net_resolve(net);
}
// On: every block goes into its 3x3-led form (and stays there when the stage goes off again) and the tail comes with the stage; the head does
// not - that takes the pair's own choice word, the autotuner or a selector. Off: tail and head go with it.
void net_set_stage(saber_hip_net* net, int i0, bool on) {
    NetOp& H0 = net->ops[i0];
    if (!H0.stage) return;
    if (on || H0.stage_on)
        for (int k = 0; k < H0.stage_n; ++k) {
            net->ops[i0 + 3 * k].led_on = true;
            net->ops[i0 + 3 * k].stage_name_kept = !on;
            net->ops[i0 + 3 * k + 1].chain_on = net->ops[i0 + 3 * k + 1].chain != nullptr;
        }
    if (on) H0.tail_on = H0.stage->tail != nullptr;
    if (!on) H0.tail_on = H0.head_on = false;
    H0.stage_on = on;
    net_resolve(net);
}
// The separable site headed by ops[i] (NetOp::sep): code = a valid form of the pair -> the one launch with that form; 0 -> the two ops launch on their own again.
void net_set_sep(saber_hip_net* net, int i, int code) {
    NetOp& D = net->ops[i];
    if (!D.sep || i + 1 >= (int)net->ops.size()) return;
    if (code && saber_hip_conv2d_sep_set_tile(D.sep, code) != SABER_HIP_OK) code = 0;
    D.sep_on = code != 0;
    net_resolve(net);
}
// The inverted-residual site headed by ops[i] (NetOp::ir): code = a valid form of the block -> the one launch with that form; 0 -> the three ops launch on
// their own again.
void net_set_ir(saber_hip_net* net, int i, int code) {
    NetOp& E = net->ops[i];
    if (!E.ir || i + 2 >= (int)net->ops.size()) return;
    if (code && saber_hip_conv2d_ir_set_tile(E.ir, code) != SABER_HIP_OK) code = 0;
    E.ir_on = code != 0;
    net_resolve(net);
}
// The Fire site headed by ops[i] (NetOp::fire): code = a valid form of the module -> the one launch with that form; 0 -> the four ops launch on
// their own again.
void net_set_fire(saber_hip_net* net, int i, int code) {
    NetOp& Q = net->ops[i];
    if (!Q.fire || i + 3 >= (int)net->ops.size()) return;
    if (code && saber_hip_conv2d_fire_set_tile(Q.fire, code) != SABER_HIP_OK) code = 0;
    Q.fire_on = code != 0;
    net_resolve(net);
}
// The resize + sum site headed by ops[i] (NetOp::rsum): on -> the resize's launch also sums; off -> the two ops launch on their own again.
void net_set_resize_sum(saber_hip_net* net, int i, bool on) {
    NetOp& R = net->ops[i];
    if (!R.rsum || i + 1 >= (int)net->ops.size()) return;
    R.rsum_on = on;
    net_resolve(net);
}
static int clone_conv_i8(const saber_hip_conv* src, const saber_hip_conv_desc& d, saber_hip_conv** out) {
    int rc = saber_hip_conv2d_create(&d, out);
    if (rc) return rc;
    rc = saber_hip_conv2d_set_weights(*out, src->wq_oihw.data(), SABER_HIP_S8, src->w_scale.data(),
                                      src->has_bias ? src->bias_host.data() : nullptr, src->in_scale, src->out_scale);
    if (rc) {
        saber_hip_conv2d_destroy(*out);
        *out = nullptr;
    }
    return rc;
}

int saber_hip_net_optimize(saber_hip_net_t* net, int flags) {
    if (!net) return fail(SABER_HIP_INVALID_VALUE, "null argument");
    if (net->finalized) return fail(SABER_HIP_INVALID_VALUE, "optimize must run before finalize");
    if (flags & 2048) {      // the net does not own the device: decided HERE, at selection time, not when a launch has failed
        net->shared_device = true;
        flags &= ~256;       // no persistent stage launch
    }
    if (net->shared_device) flags &= ~256;
    if (flags & SABER_HIP_NET_REPRODUCIBLE_FP32) net->reproducible_fp32 = true;      // sticks to the net (api_net_autotune.hip)
    std::vector<NetOp>& ops = net->ops;
    const int nt = (int)net->tensor_bytes.size();
    std::vector<char> dead(ops.size(), 0);
    int removed = 0;
    auto consumers = [&](int t) {
        int c = 0;
        for (size_t i = 0; i < ops.size(); ++i)
            if (!dead[i]) c += op_reads(ops[i], t);
        return c;
    };
    auto readers = [&](int t) {      // ... over the list as it stands (after the compaction below: every op)
        int r = 0;
        for (const NetOp& o : ops) r += op_reads(o, t);
        return r;
    };
    auto producer = [&](int t, int before) {   // last live op before `before` that writes tensor t
        for (int i = before - 1; i >= 0; --i)
            if (!dead[i] && (ops[i].out == t || ops[i].out2 == t)) return i;
        return -1;
    };
    // an op of an inverted-residual site (flag 32768 in this or an earlier call): the expand op or one of the two behind it
    auto in_ir = [&](const NetOp& o) {
        const size_t i = (size_t)(&o - ops.data());
        for (size_t b = 0; b <= 3 && b <= i && i < ops.size(); ++b)      // (... or of a Fire site, flag 65536: the squeeze op or one of the three behind it)
            if (ops[i - b].fire != nullptr) return true;
        return o.ir != nullptr || (i > 0 && i < ops.size() && ops[i - 1].ir != nullptr) || (i > 1 && i < ops.size() && ops[i - 2].ir != nullptr);
    };
    // an op of a separable site (flag 16384 in an earlier call) or of an inverted-residual site keeps its conv: the site's object was made from it
    auto in_sep = [&](const NetOp& o) {
        const size_t i = (size_t)(&o - ops.data());
        return o.sep != nullptr || (i > 0 && i < ops.size() && ops[i - 1].sep != nullptr) || in_ir(o);
    };
    auto plain_i8_conv = [&](const NetOp& o) {
        return !in_sep(o) && o.kind == OP_CONV && o.conv && o.conv->is_i8 && o.conv->weights_set && o.conv->epi == EPI_I8_CONV &&
               o.conv->d.res_mode == SABER_HIP_RES_NONE && !o.conv->pair_k2 && !o.conv->pool_fused && o.lane == 0;
    };
    // ---- 1: conv + eltwise -----------------------------------------------------------------------------------
    if (flags & 1) {
        for (size_t i = 0; i < ops.size(); ++i) {
            if (dead[i] || ops[i].kind != OP_ELT_I8) continue;
            NetOp& e = ops[i];
            for (int side = 0; side < 2; ++side) {
                const int tc = side == 0 ? e.in : e.in2, tr = side == 0 ? e.in2 : e.in;   // conv-side / residual-side tensors
                const float s_conv = e.f[side], s_res = e.f[1 - side], c_conv = e.f[2 + side], c_res = e.f[3 - side];
                const int p = producer(tc, (int)i);
                if (p < 0 || !plain_i8_conv(ops[p]) || consumers(tc) != 1 || tc == tr) continue;
                const saber_hip_conv* src = ops[p].conv;
                if (src->d.out_dtype != SABER_HIP_S8 || src->out_scale != s_conv) continue;
                if (net->tensor_bytes[tc] != net->tensor_bytes[e.out] || e.count != net->tensor_bytes[tc]) continue;
                const int pr = producer(tr, (int)i);
                if (pr >= p) continue;   // the residual must exist when the conv runs (external tensors: pr == -1)
                // the fused conv writes e.out at the CONV's position: no live op in (p, i) may read or write that tensor,
                // and it must not alias the residual or the conv's own output (in-place eltwise: e.out == tc would become the fused
                // conv's output AND the edge whose storage is freed below)
                bool clash = e.out == tr || e.out == tc;
                for (int j = p + 1; j < (int)i && !clash; ++j)
                    if (!dead[j]) clash = op_touches(ops[j], e.out);
                if (clash) continue;
                saber_hip_conv_desc d = src->d;
                d.res_mode = SABER_HIP_RES_ELTWISE;
                d.res_act = e.p[0] ? SABER_HIP_ACT_RELU : SABER_HIP_ACT_NONE;
                d.coeff_conv = c_conv; d.coeff_res = c_res; d.scale_res = s_res;
                saber_hip_conv* fused = nullptr;
                int rc = clone_conv_i8(src, d, &fused);
                if (rc) return rc;
                net->owned.push_back(fused);
                ops[p].conv = fused;
                ops[p].in2 = tr;
                ops[p].out = e.out;
                dead[i] = 1;
                net->tensor_bytes[tc] = 0;   // the conv's own output edge no longer exists
                ++removed;
                break;
            }
        }
    }
    // ---- 64: a shortcut's 1x1 / stride-s max pooling read by a fused eltwise epilogue only -> folded into that read ----
    // (the pooling graph_strategy::apply_stride_up inserts, optimize_strategy.h:213-248: one element per window, so the op is
    // a spatial subsampling; the conv then reads the pooling's SOURCE at (oy * s, ox * s): saber_hip_conv_desc::res_stride)
    if (flags & 64) {
        for (size_t i = 0; i < ops.size(); ++i) {
            if (dead[i] || ops[i].kind != OP_POOL_I8) continue;
            NetOp& q = ops[i];   // p[] = n,h,w,c,oh,ow,kh,kw,sh,sw,ph,pw,type,in_dtype,out_dtype
            if (q.p[6] != 1 || q.p[7] != 1 || q.p[8] != q.p[9] || q.p[8] < 2 || q.p[10] || q.p[11] || q.p[12] != SABER_HIP_POOL_MAX ||
                q.p[13] != SABER_HIP_S8 || q.p[14] != SABER_HIP_S8 || (q.p[1] - 1) / q.p[8] + 1 != q.p[4] ||
                (q.p[2] - 1) / q.p[8] + 1 != q.p[5] || consumers(q.out) != 1)
                continue;
            int c = -1;
            for (size_t j = i + 1; j < ops.size() && c < 0; ++j) {
                if (dead[j]) continue;
                if (ops[j].out == q.in || ops[j].out2 == q.in) break;            // the pooling's source is rewritten first
                if (ops[j].in2 == q.out && ops[j].kind == OP_CONV && ops[j].conv && !ops[j].chain && !ops[j].chain3 &&
                    ops[j].conv->d.res_mode == SABER_HIP_RES_ELTWISE && ops[j].conv->d.res_stride <= 1 && ops[j].lane == q.lane && !in_ir(ops[j]))
                    c = (int)j;
                else if (op_reads(ops[j], q.out)) break;       // some other reader
            }
            if (c < 0) continue;
            const saber_hip_conv* src = ops[c].conv;
            if (src->oh != q.p[4] || src->ow != q.p[5] || src->d.k != q.p[3] || src->d.n != q.p[0]) continue;
            saber_hip_conv_desc d = src->d;
            d.res_stride = q.p[8]; d.res_h = q.p[1]; d.res_w = q.p[2];
            saber_hip_conv* fused = nullptr;
            if (clone_conv_i8(src, d, &fused) != SABER_HIP_OK) continue;       // (the direct fallback kernel cannot: keep the op)
            net->owned.push_back(fused);
            ops[c].conv = fused;
            ops[c].in2 = q.in;
            ops[c].res_note = "+res/" + std::to_string(q.p[8]);
            dead[i] = 1;
            net->tensor_bytes[q.out] = 0;
            ++removed;
        }
    }
    // ---- 4: conv + max pooling ----------------------------------------------------------------------------------
    if (flags & 4) {
        for (size_t i = 0; i < ops.size(); ++i) {
            if (dead[i] || ops[i].kind != OP_POOL_I8) continue;
            NetOp& q = ops[i];
            const int p = producer(q.in, (int)i);
            if (p < 0 || !plain_i8_conv(ops[p]) || consumers(q.in) != 1) continue;
            {   // the pooled tensor is written at the CONV's position instead: nothing in (p, i) may read or write it, and it must
                // not be the conv's own output (an in-place pooling: the edge whose storage is freed below)
                bool clash = q.out == q.in;
                for (int j = p + 1; j < (int)i && !clash; ++j)
                    if (!dead[j]) clash = op_touches(ops[j], q.out);
                if (clash) continue;
            }
            const saber_hip_conv* src = ops[p].conv;
            saber_hip_conv* fused = nullptr;
            int rc = clone_conv_i8(src, src->d, &fused);
            if (rc) return rc;
            // p[] = n,h,w,c,oh,ow,kh,kw,sh,sw,ph,pw,type,in_dtype,out_dtype (saber_hip_net_add_pool_i8)
            const int floor_mode = saber_hip_pool_out_dim(q.p[1], q.p[10], q.p[6], q.p[8], 0) == q.p[4] ? 0 : 1;
            rc = saber_hip_conv2d_set_pooling(fused, q.p[12], q.p[6], q.p[7], q.p[8], q.p[9], q.p[10], q.p[11], floor_mode);
            int oh = 0, ow = 0;
            if (rc == SABER_HIP_OK) saber_hip_conv2d_out_shape(fused, &oh, &ow);
            if (rc != SABER_HIP_OK || oh != q.p[4] || ow != q.p[5] || q.p[13] != q.p[14]) {   // no fused kernel: keep the two ops
                saber_hip_conv2d_destroy(fused);
                continue;
            }
            net->owned.push_back(fused);
            ops[p].conv = fused;
            const int dead_t = ops[p].out;
            ops[p].out = q.out;
            dead[i] = 1;
            net->tensor_bytes[dead_t] = 0;
            ++removed;
        }
    }
    // ---- 2: sibling pairs -------------------------------------------------------------------------------------
    if (flags & 2) {
        for (size_t i = 0; i < ops.size(); ++i) {
            if (dead[i] || !plain_i8_conv(ops[i])) continue;
            for (size_t j = i + 1; j < ops.size(); ++j) {
                if (dead[j]) continue;
                if (ops[j].out == ops[i].in || ops[j].out2 == ops[i].in) break;   // the shared input is rewritten: stop
                if (!plain_i8_conv(ops[j]) || ops[j].in != ops[i].in) continue;
                {   // op j's output is written at position i instead: nothing in [i, j) may touch that tensor
                    bool clash = false;
                    for (size_t m = i; m < j && !clash; ++m)
                        if (!dead[m]) clash = op_touches(ops[m], ops[j].out);
                    if (clash) continue;
                }
                saber_hip_conv* pair = nullptr;
                bool swapped = false;
                if (saber_hip_conv2d_create_pair(ops[i].conv, ops[j].conv, &pair) != SABER_HIP_OK) {
                    // the first rows must be a multiple of the largest block tile: try the other order
                    if (saber_hip_conv2d_create_pair(ops[j].conv, ops[i].conv, &pair) != SABER_HIP_OK) continue;
                    swapped = true;
                }
                // hoisting op j to position i is safe: it only reads the shared input, and nothing between reads its output
                // before j (a consumer of j's output cannot precede j in a valid list)
                net->owned.push_back(pair);
                ops[i].kind = OP_CONV_PAIR;
                ops[i].conv = pair;
                ops[i].out2 = ops[j].out;
                if (swapped) std::swap(ops[i].out, ops[i].out2);
                dead[j] = 1;
                ++removed;
                break;
            }
        }
    }
    // ---- 8: global pooling writes the fc's quantised operand ---------------------------------------------------------
    if (flags & 8) {
        for (size_t i = 0; i < ops.size(); ++i) {
            if (dead[i] || ops[i].kind != OP_FC || !ops[i].fc->pre_quant) continue;
            const int p = producer(ops[i].in, (int)i);
            if (p < 0 || ops[p].kind != OP_POOL_F32_I8 || ops[p].out2 >= 0) continue;
            const saber_hip_fc* fc = ops[i].fc;
            // the pooled tensor must be exactly the fc's [m, k] operand
            if ((size_t)ops[p].p[0] * ops[p].p[3] * ops[p].p[4] * ops[p].p[5] != (size_t)fc->d.m * fc->d.k) continue;
            const int qt = saber_hip_net_add_tensor(net, (size_t)fc->d.m * fc->d.k);
            ops[p].out2 = qt;
            ops[p].f[1] = fc->in_scale;
            ops[p].name = "pool2d_f32_from_i8+quantize";
            ops[i].kind = OP_FC_Q;
            ops[i].in = qt;
            ++removed;   // the fc's quantise-on-entry kernel
        }
    }
    // ---- 128: conv + global average pooling (INT8): the pooling's launch disappears, both tensors are written -------
    if (flags & 128) {
        for (size_t i = 0; i < ops.size(); ++i) {
            if (dead[i] || ops[i].kind != OP_POOL_I8) continue;
            NetOp& q = ops[i];   // p[] = n,h,w,c,oh,ow,kh,kw,sh,sw,ph,pw,type,in_dtype,out_dtype
            if (q.p[4] != 1 || q.p[5] != 1 || q.p[6] != q.p[1] || q.p[7] != q.p[2] || q.p[10] || q.p[11] ||
                q.p[12] == SABER_HIP_POOL_MAX || q.p[13] != q.p[14])
                continue;
            const int p = producer(q.in, (int)i);
            if (p < 0 || ops[p].kind != OP_CONV || !ops[p].conv || ops[p].lane != q.lane || ops[p].out2 >= 0 || in_sep(ops[p])) continue;
            const saber_hip_conv* src = ops[p].conv;
            if (!src->is_i8 || src->pair_k2 || src->pool_fused || src->gpool || !img_conv_ok(src) || src->d.n != q.p[0] ||
                src->d.k != q.p[3] || src->oh != q.p[1] || src->ow != q.p[2] || src->d.out_dtype != q.p[13])
                continue;
            {   // the pooled tensor is written at the CONV's position instead: nothing in (p, i) may read or write it
                bool clash = false;
                for (int j = p + 1; j < (int)i && !clash; ++j)
                    if (!dead[j]) clash = op_touches(ops[j], q.out);
                if (clash) continue;
            }
            saber_hip_conv* fused = nullptr;
            if (clone_conv_i8(src, src->d, &fused) != SABER_HIP_OK) continue;
            if (saber_hip_conv2d_set_global_pooling(fused) != SABER_HIP_OK) {
                saber_hip_conv2d_destroy(fused);
                continue;
            }
            net->owned.push_back(fused);
            ops[p].conv = fused;
            ops[p].out2 = q.out;
            dead[i] = 1;
            ++removed;
        }
    }
    (void)nt;
    std::vector<NetOp> live;
    for (size_t i = 0; i < ops.size(); ++i)
        if (!dead[i]) live.push_back(std::move(ops[i]));
    ops.swap(live);
    // ---- 512: the fused stem conv + pooling runs the sibling pair that reads the pooled tensor (on the compacted list) --------
    bool side_lane = false;      // (like the chains: a launch that writes other ops' tensors is not ordered across lanes)
    for (const NetOp& o : ops) side_lane |= o.lane != 0;
    if ((flags & 512) && !side_lane) {
        for (size_t i = 0; i + 1 < ops.size(); ++i) {
            NetOp& S = ops[i];
            NetOp& P = ops[i + 1];
            if (S.kind != OP_CONV || !S.conv || !S.conv->pool_fused || S.lane || S.in2 >= 0 || S.out2 >= 0 || S.stem_pair) continue;
            if (P.kind != OP_CONV_PAIR || !P.conv || P.lane || P.in != S.out || !P.conv->pair_src_a || !P.conv->pair_src_b) continue;
            if (readers(S.out) != 1) continue;
            saber_hip_stem_pair* sp = nullptr;
            if (saber_hip_conv2d_stem_pair_create(S.conv, P.conv->pair_src_a, P.conv->pair_src_b, &sp) != SABER_HIP_OK) continue;
            net->owned_stem_pairs.push_back(sp);
            S.stem_pair = sp;
            S.stem_y1 = P.out;
            S.stem_y2 = P.out2;
            ++removed;
        }
        net_resolve(net);      // (the pairs now covered are no site's op below)
    }
    // A chain launch reads and writes the tensors of SEVERAL ops (chain3_res / chain_out / chain3_y1 / chain3_y2), while the
    // cross-lane event ordering of saber_hip_net_run only follows the launching op's own in / in2 / out / out2: in a
    // two-lane net a chained launch could read a residual produced on the other lane before its event. The two executor
    // options are therefore exclusive: no chains once any op sits on the side lane (and saber_hip_net_set_lane refuses
    // a lane change once chains exist).
    bool two_lanes = false;
    for (const NetOp& o : ops) two_lanes |= o.lane != 0;
    if (two_lanes) flags &= ~(16 | 32);
    // ---- 131072 (SABER_HIP_NET_RESIZE_SUM): a lane-0 resize op whose output has exactly one reader, the NEXT op, an eltwise_f32 that takes it as
    // either operand (FPN's top-down merge) -> a site: the resize's launch also sums, in + 2 x out floats instead of in + 4 x out. Both ops
    // stay; the eltwise's output keeps its bits (resize.hip rounds the resized value to float before the eltwise expression). Declined: a second
    // reader of the resized edge, an eltwise that is not the next op, a net with a side lane (the launch reads another op's operand: not ordered
    // across lanes), an eltwise whose other operand is the resize's own input tensor, an eltwise that writes in place (onto an operand or the
    // resize's input). Counted: the sites formed (each removes one launch while it is on).
    if ((flags & SABER_HIP_NET_RESIZE_SUM) && !two_lanes) {
        for (size_t i = 0; i + 1 < ops.size(); ++i) {
            NetOp& R = ops[i];
            NetOp& E = ops[i + 1];
            if (R.kind != OP_RESIZE || !R.resize || R.rsum || R.skip || R.lane || E.kind != OP_ELT_F32 || E.skip || E.lane) continue;
            if (op_reads(E, R.out) != 1 || readers(R.out) != 1) continue;
            const int other = E.in == R.out ? E.in2 : E.in;
            if (other < 0 || other == R.in || E.out == R.in || E.out == R.out || E.out == other) continue;
            const saber_hip_resize_desc& d = R.resize->d;
            if (E.count != (size_t)d.n * R.resize->oh * R.resize->ow * d.c) continue;
            R.rsum = true;
            net_set_resize_sum(net, (int)i, resize_sum_static_on(R.resize));
            ++removed;
            ++i;
        }
    }
    // ---- 65536 (SABER_HIP_NET_FIRE): four consecutive lane-0 ops - a 1x1 squeeze conv, the two convs that alone read it (1x1, then 3x3), the u8
    // concat that alone reads exactly those two, in that order, with all multipliers 1 (SqueezeNet's Fire module) - that
    // saber_hip_conv2d_fire_create accepts -> a site of the one-launch form (conv_fire.hip). All four ops stay; which sites are on is
    // fire_static_form's choice until the autotuner has timed every form against the four launches. No workgroup of that kernel depends on
    // another: allowed on a shared device. Applied BEFORE the block, separable and chain flags, which skip the ops a Fire site holds (in_ir);
    // ops another site already holds are skipped here. Counted: the sites formed (each removes three launches while a form is selected).
    if ((flags & SABER_HIP_NET_FIRE) && !two_lanes) {
        auto free_op = [&](size_t j) {
            const NetOp& o = ops[j];
            if (o.chain || o.chain3 || o.stem_pair || o.sep || o.stage || o.skip || o.lane || in_ir(o)) return false;
            if (j > 0 && (ops[j - 1].chain || ops[j - 1].chain3 || ops[j - 1].stem_pair || ops[j - 1].sep)) return false;
            return !(j > 1 && ops[j - 2].chain3 != nullptr);
        };
        for (size_t i = 0; i + 3 < ops.size(); ++i) {
            NetOp& Q = ops[i];
            NetOp& A = ops[i + 1];
            NetOp& B = ops[i + 2];
            NetOp& K = ops[i + 3];
            if (Q.kind != OP_CONV || A.kind != OP_CONV || B.kind != OP_CONV || K.kind != OP_CONCAT || !Q.conv || !A.conv || !B.conv) continue;
            if (!free_op(i) || !free_op(i + 1) || !free_op(i + 2) || !free_op(i + 3)) continue;
            if (Q.in2 >= 0 || A.in2 >= 0 || B.in2 >= 0 || Q.out2 >= 0 || A.out2 >= 0 || B.out2 >= 0 || A.in != Q.out || B.in != Q.out) continue;
            if (K.ins.size() != 2 || K.ins[0] != A.out || K.ins[1] != B.out || K.p[0] != SABER_HIP_U8) continue;
            bool copy = true;
            for (float m : K.cat_m) copy = copy && m == 1.0f;
            if (!copy || readers(Q.out) != 2 || readers(A.out) != 1 || readers(B.out) != 1) continue;
            if (K.cat_c[0] != A.conv->d.k || K.cat_c[1] != B.conv->d.k || K.count != (size_t)Q.conv->d.n * Q.conv->oh * Q.conv->ow) continue;
            saber_hip_fire* fr = nullptr;
            if (saber_hip_conv2d_fire_create(Q.conv, A.conv, B.conv, &fr) != SABER_HIP_OK) continue;      // not a module the kernel takes
            net->owned_fires.push_back(fr);
            Q.fire = fr;
            Q.fire_out = K.out;
            net_set_fire(net, (int)i, fire_static_form(fr));
            ++removed;
            i += 3;
        }
    }
    // ---- 32768 (SABER_HIP_NET_INVERTED_RESIDUAL): three consecutive lane-0 ops - a 1x1 expand conv, the depthwise 3x3 conv that alone reads it,
    // the 1x1 project conv that alone reads that (MobileNet-v2's blocks) - that saber_hip_conv2d_ir_create accepts -> a site of the one-launch
    // form (conv_ir.hip). Where the project conv carries the fused eltwise (flag 1 ran first) its residual must be the expand conv's input.
    // All three ops stay; which sites are on is ir_static_form's choice until the autotuner has timed every form against the three launches.
    // No workgroup of that kernel depends on another: allowed on a shared device. NO OP BELONGS TO TWO SITES: ops that head or follow a chain, a
    // separable or a stem site are skipped here, and the chain / separable formation below skips the ops a block site holds - so whichever flag
    // comes later finds the ops taken and counts nothing for them. Counted: the sites formed (each removes two launches while a form is selected).
    if ((flags & SABER_HIP_NET_INVERTED_RESIDUAL) && !two_lanes) {
        auto taken = [&](size_t j) {      // heads another site, or is covered by the site of an op in front of it
            const NetOp& o = ops[j];
            if (o.chain || o.chain3 || o.stem_pair || o.sep || o.stage || in_ir(o)) return true;
            if (j > 0 && (ops[j - 1].chain || ops[j - 1].chain3 || ops[j - 1].stem_pair || ops[j - 1].sep)) return true;
            return j > 1 && ops[j - 2].chain3 != nullptr;
        };
        for (size_t i = 0; i + 2 < ops.size(); ++i) {
            NetOp& E = ops[i];
            NetOp& D = ops[i + 1];
            NetOp& P = ops[i + 2];
            if (E.kind != OP_CONV || D.kind != OP_CONV || P.kind != OP_CONV || !E.conv || !D.conv || !P.conv || E.skip || D.skip || P.skip || E.lane ||
                D.lane || P.lane || E.in2 >= 0 || D.in2 >= 0 || E.out2 >= 0 || D.out2 >= 0 || P.out2 >= 0 || D.in != E.out || P.in != D.out)
                continue;
            if (taken(i) || taken(i + 1) || taken(i + 2)) continue;
            if (readers(E.out) != 1 || readers(D.out) != 1) continue;
            const bool elt = P.conv->d.res_mode == SABER_HIP_RES_ELTWISE;
            if (elt ? P.in2 != E.in : P.in2 >= 0) continue;      // the fused eltwise's residual is the block's input
            saber_hip_ir* ir = nullptr;
            if (saber_hip_conv2d_ir_create(E.conv, D.conv, P.conv, &ir) != SABER_HIP_OK) continue;      // not a block the kernel takes
            net->owned_irs.push_back(ir);
            E.ir = ir;
            E.ir_out = P.out;
            net_set_ir(net, (int)i, ir_static_form(ir));
            ++removed;
            i += 2;
        }
    }
    // ---- 16384 (SABER_HIP_NET_SEPARABLE): a depthwise 3x3 conv + the 1x1 conv that alone reads it, the NEXT op (MobileNet's separable pairs)
    // -> a site of the one-launch form (conv_sep.hip). Both ops stay; which sites are on is sep_static_form's choice until the autotuner has
    // timed every form against the two launches. No workgroup of that kernel depends on another: allowed on a shared device. Counted: the
    // sites formed (each removes one launch while a form is selected).
    if ((flags & SABER_HIP_NET_SEPARABLE) && !two_lanes) {
        for (size_t i = 0; i + 1 < ops.size(); ++i) {
            NetOp& D = ops[i];
            NetOp& P = ops[i + 1];
            if (D.kind != OP_CONV || P.kind != OP_CONV || !D.conv || !P.conv || D.sep || D.skip || P.skip || D.lane || P.lane || D.chain || D.chain3 ||
                D.stem_pair || P.chain || P.chain3 || P.stem_pair || P.sep || in_ir(D) || in_ir(P) || D.in2 >= 0 || P.in2 >= 0 || D.out2 >= 0 || P.out2 >= 0 || P.in != D.out)
                continue;
            if (!D.conv->is_i8 || !dw_ok(D.conv)) continue;
            if (readers(D.out) != 1) continue;
            saber_hip_sep* sp = nullptr;
            if (saber_hip_conv2d_sep_create(D.conv, P.conv, &sp) != SABER_HIP_OK) continue;      // not a pair the kernel takes
            net->owned_seps.push_back(sp);
            D.sep = sp;
            D.sep_out = P.out;
            net_set_sep(net, (int)i, sep_static_form(sp));
            ++removed;
        }
    }
    // ---- 16: conv1x1 chains (on the compacted list: the pair must be adjacent) --------------------------------
    if (flags & 16) {
        for (size_t i = 0; i + 1 < ops.size(); ++i) {
            NetOp& A = ops[i];
            NetOp& B = ops[i + 1];
            if (A.kind != OP_CONV || B.kind != OP_CONV || !A.conv || !B.conv || A.chain || A.skip || B.chain || A.lane || B.lane ||
                A.chain3 || B.chain3 || in_ir(A) || in_ir(B))
                continue;
            if (A.conv->d.res_mode != SABER_HIP_RES_ELTWISE || B.in != A.out || A.in2 < 0 || B.in2 >= 0) continue;
            saber_hip_chain* ch = nullptr;
            if (saber_hip_conv2d_chain_create(A.conv, B.conv, &ch) != SABER_HIP_OK) continue;   // not a chainable shape
            net->owned_chains.push_back(ch);
            A.chain = ch;
            A.chain_out = B.out;
            net_set_chain_mode(net, (int)i, ch->c1 <= 256 ? 1 : 0);      // default until the autotuner has timed both forms
            if (A.chain_on) ++removed;
        }
    }
    // ---- 32: the block's 3x3 conv in front of a chain head, when the head is its only consumer -----------------------
    if (flags & 32) {
        for (size_t i = 0; i + 2 < ops.size(); ++i) {
            NetOp& Hd = ops[i];
            NetOp& A = ops[i + 1];
            NetOp& B = ops[i + 2];
            if (!A.chain || Hd.kind != OP_CONV || !Hd.conv || Hd.chain3 || Hd.chain || Hd.skip || Hd.lane || Hd.in2 >= 0 ||
                A.in != Hd.out)
                continue;
            if (readers(Hd.out) != 1) continue;
            saber_hip_chain* ch = nullptr;
            if (saber_hip_conv2d_chain_create3(Hd.conv, A.conv, B.conv, &ch) != SABER_HIP_OK) continue;
            net->owned_chains.push_back(ch);
            Hd.chain3 = ch;
            Hd.chain3_res = A.in2; Hd.chain3_y1 = A.out; Hd.chain3_y2 = B.out;
            const bool was = A.chain_on;
            net_set_chain_mode(net, (int)i + 1, ch->c1 <= 128 ? 2 : (was ? 1 : 0));
            if (Hd.led_on) removed += was ? 1 : 2;
        }
        // ... and in front of a fused-eltwise 1x1 conv that heads no chain (the last block of a stage): conv3x3 + conv1x1
        for (size_t i = 0; i + 1 < ops.size(); ++i) {
            NetOp& Hd = ops[i];
            NetOp& A = ops[i + 1];
            if (A.chain || A.skip || A.kind != OP_CONV || !A.conv || A.conv->d.res_mode != SABER_HIP_RES_ELTWISE || A.in2 < 0 || A.lane ||
                Hd.kind != OP_CONV || !Hd.conv || Hd.chain3 || Hd.chain || Hd.skip || Hd.lane || Hd.in2 >= 0 || A.in != Hd.out || in_ir(Hd) || in_ir(A))
                continue;
            if (readers(Hd.out) != 1) continue;
            saber_hip_chain* ch = nullptr;
            // 1024: ... and the sibling pair that is the only reader of A's output (the next stage's branch1 / branch2a) joins the launch
            NetOp* P = (flags & 1024) && i + 2 < ops.size() ? &ops[i + 2] : nullptr;
            if (P && (P->kind != OP_CONV_PAIR || P->lane || P->skip || P->in != A.out || !P->conv || !P->conv->pair_src_a || !P->conv->pair_src_b)) P = nullptr;
            if (P) {
                if (readers(A.out) != 1 || saber_hip_conv2d_chain_create3_pair(Hd.conv, A.conv, const_cast<saber_hip_conv*>(P->conv->pair_src_a),
                                                                   const_cast<saber_hip_conv*>(P->conv->pair_src_b), &ch) != SABER_HIP_OK)
                    P = nullptr;
            }
            if (!P && saber_hip_conv2d_chain_create3(Hd.conv, A.conv, nullptr, &ch) != SABER_HIP_OK) continue;
            net->owned_chains.push_back(ch);
            Hd.chain3 = ch;
            Hd.chain3_res = A.in2; Hd.chain3_y1 = A.out; Hd.chain3_y2 = P ? P->out : -1; Hd.chain3_y3 = P ? P->out2 : -1;
            net_set_chain_mode(net, (int)i + 1, ch->c1 <= 128 ? 2 : 0);
            if (Hd.led_on) removed += P ? 2 : 1;
        }
    }
    // ---- 256: runs of 3x3-led C = 256 (or C = 128, or C = 64) chains whose blocks feed each other (ResNet's res4 / res3 stage) -> one persistent launch
    // NOT part of 255: the launch needs every workgroup of an image resident on its XCD at once - fine for one net on the GPU
    // (the latency path), not for several nets in flight on their own streams (two such launches can each hold half of the CUs
    // and wait for the other half: they time out, report an error and fall back; conv_stage_coop.hip)
    if ((flags & 256) && (flags & 32) && !two_lanes) {
        for (size_t i = 0; i + 2 < ops.size();) {
            auto block_ok = [&](size_t j) {
                return j + 2 < ops.size() && ops[j].chain3 && ops[j].chain3->b && !ops[j].stage && ops[j].chain3_y2 >= 0 &&
                       ((ops[j].chain3->c1 == 256 && ops[j].chain3->stage1) || ((ops[j].chain3->c1 == 128 || ops[j].chain3->c1 == 64) && ops[j].chain3->d_stream_stage1.p));
            };
            if (!block_ok(i)) { ++i; continue; }
            std::vector<saber_hip_chain*> run{ops[i].chain3};
            while ((int)run.size() < saber_mi355x::STAGE4_LONG) {
                const size_t p = i + 3 * (run.size() - 1), j = p + 3;
                if (!block_ok(j) || ops[j].chain3->c1 != run[0]->c1 || ops[j].in != ops[p].chain3_y2 || ops[j].chain3_res != ops[p].chain3_y1) break;
                run.push_back(ops[j].chain3);
            }
            if (run.size() >= 2) {
                saber_hip_chain_stage* st = nullptr;
                // the strided head behind a C = 256 run (res4f's conv3x3 / stride 2 + conv1x1 + eltwise) reads the last block's two outputs:
                // the launch's tail (conv_stage_coop.hip); where the stage does not take it, the stage without
                const size_t pl = i + 3 * (run.size() - 1), jt = pl + 3;
                saber_hip_chain* tail = nullptr;
                if (jt + 1 < ops.size() && run[0]->c1 == 256 && ops[jt].chain3 && !ops[jt].chain3->b && !ops[jt].chain3->b2 && !ops[jt].stage &&
                    ops[jt].chain3->c1 == 256 && ops[jt].chain3->c3->d.stride_h == 2 && ops[jt].in == ops[pl].chain3_y2 &&
                    ops[jt].chain3_res == ops[pl].chain3_y1 && ops[jt].chain3_y1 >= 0)
                    tail = ops[jt].chain3;
                // the sibling pair directly in front of a C = 256 run (res4a_branch1 / res4a_branch2a) whose two outputs are the first block's
                // shortcut and 3x3 input and have no other reader: the launch's head. The site is formed, the head stays OFF until the pair's
                // choice word (bit 29), the autotuner or a selector asks for it.
                const saber_hip_conv *head_a = nullptr, *head_b = nullptr;
                if (i >= 1 && run[0]->c1 == 256 && ops[i - 1].kind == OP_CONV_PAIR && !ops[i - 1].skip && !ops[i - 1].lane && ops[i - 1].conv &&
                    ops[i - 1].conv->pair_src_a && ops[i - 1].conv->pair_src_b && !(i >= 3 && ops[i - 3].chain3 && ops[i - 3].chain3->b2)) {
                    const NetOp& P = ops[i - 1];
                    const int t_res = ops[i].chain3_res, t_x = ops[i].in;
                    const bool fwd = P.out == t_res && P.out2 == t_x, rev = P.out == t_x && P.out2 == t_res;
                    if ((fwd || rev) && t_res != t_x && readers(t_res) == 1 && readers(t_x) == 1) {
                        head_a = fwd ? P.conv->pair_src_a : P.conv->pair_src_b;
                        head_b = fwd ? P.conv->pair_src_b : P.conv->pair_src_a;
                    }
                }
                if (head_a && saber_hip_conv2d_stage_create_head(run.data(), (int)run.size(), tail, head_a, head_b, &st) != SABER_HIP_OK) head_a = head_b = nullptr;
                if (!head_a && tail && saber_hip_conv2d_stage_create_tail(run.data(), (int)run.size(), tail, &st) != SABER_HIP_OK) tail = nullptr;
                if (head_a || tail || saber_hip_conv2d_stage_create(run.data(), (int)run.size(), &st) == SABER_HIP_OK) {
                    net->owned_stages.push_back(st);
                    ops[i].stage = st;
                    ops[i].stage_n = (int)run.size();
                    if (tail) ops[jt].tail_of = (int)i;
                    if (head_a) ops[i - 1].head_of = (int)i;
                    int before = 0;
                    for (size_t k = 0; k < run.size(); ++k) before += 3 - (ops[i + 3 * k].skip + ops[i + 3 * k + 1].skip + ops[i + 3 * k + 2].skip);
                    if (tail) before += 2 - (ops[jt].skip + ops[jt + 1].skip);
                    // C = 64: a block's first output that only the next block of the run reads (its eltwise and its first 1x1 conv) is not
                    // written while the one launch is selected - the tile stays in LDS
                    if (run[0]->c1 == 64)
                        for (size_t k = 0; k + 1 < run.size(); ++k) ops[i + 3 * k].stage_y1_private = readers(ops[i + 3 * k].chain3_y1) == 2;
                    // default until the autotuner has timed both forms: the res4 stage (C = 256) on from batch 4 (an image per XCD: fewer
                    // images leave XCDs idle); the res3 stage (C = 128) off - measured slower than its chain launches; the res2
                    // stage (C = 64) off: it goes on through its choice word, the autotuner or a setter only
                    const bool on = run[0]->a->d.n >= 4 && run[0]->c1 == 256;
                    net_set_stage(net, (int)i, on);
                    if (on) removed += before - 1;
                }
            }
            i += 3 * run.size();
        }
    }
    // ---- 4096: fc + the softmax over its output -> one launch (fc_small.hip: the last-arriving workgroup normalises) ----------------
    if (flags & 4096) {
        for (size_t i = 0; i + 1 < ops.size(); ++i) {
            NetOp& F = ops[i];
            if (dead[i] || (F.kind != OP_FC && F.kind != OP_FC_Q) || !F.fc || F.out2 >= 0 || F.lane) continue;
            size_t j = i + 1;
            while (j < ops.size() && dead[j]) ++j;
            if (j >= ops.size()) break;
            NetOp& S = ops[j];
            if (S.kind != OP_SOFTMAX || S.in != F.out || S.skip || S.lane || S.p[0] != F.fc->d.m || S.p[1] != F.fc->d.n) continue;
            if (F.kind == OP_FC && F.fc->pre_quant) continue;      // (a quantise-on-entry pre-pass: two launches already)
            if (!fc_softmax_ok(F.fc, F.kind == OP_FC_Q) || fc_softmax_prepare(F.fc) != SABER_HIP_OK) continue;
            F.out2 = S.out;
            ++removed;
        }
    }
    if (net->shared_device) {      // no variant that relies on workgroup placement: split-K off, cooperating chains back to one workgroup per tile
        for (NetOp& o : ops) {
            saber_hip_conv* c = (o.kind == OP_FC || o.kind == OP_FC_Q) ? (o.fc ? o.fc->conv : nullptr) : o.conv;
            if (c) {
                c->no_placement = true;
                if (c->sel.fam == FAM_B3 && c->sel.ksplit) (void)sel_set(c, sel_b3(c->sel, c->sel.tile, c->sel.ks, 0));
            }
            for (saber_hip_chain* ch : {o.chain, o.chain3})
                if (ch && ch->form.placement) ch->form = chain_form_plain(ch);
        }
    }
    net_resolve(net);
    // the shared workspace only has to cover the surviving ops
    net->ws_bytes = 0;
    for (const NetOp& o : ops) {
        size_t w = 0;
        if ((o.kind == OP_CONV) && o.conv) w = o.conv->ws_bytes;
        if (o.kind == OP_FC && o.fc) w = saber_hip_fc_workspace_bytes(o.fc);
        if (w > net->ws_bytes) net->ws_bytes = w;
    }
    return removed;
}

