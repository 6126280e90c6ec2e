"""Cases and seeded inputs of tests/test_gpu_tail.py: the classifier tail of the INT8 nets - the 1x1 conv (+ eltwise) with its fused
global average pooling (conv1x1_gpool.hip) and the fc + Softmax launch (fc_small.hip). scripts/record_fc_softmax_golden.py builds the
same fc cases to record tests/golden/fc_softmax_tail.npz, so everything here is a pure function of the case."""
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fc_softmax_tail.npz")

# ---- conv + pooling ----------------------------------------------------------------------------------------------------------------------
CIN = 512
GPOOL_IMAGES = [(7, 7), (8, 8), (5, 3), (1, 1)]      # 49 pixels (15 empty slots), every slot used, less than one fragment, one pixel
GPOOL_BATCHES = [1, 3, 8]
GPOOL_COUTS = [2048, 1936]                            # 1936: a multiple of 16, not of 64 - still four tiles per workgroup
# (name, eltwise, res_relu, relu, output dtype): eltwise s8 with and without res_relu; the plain epilogue u8 and s8
GPOOL_EPILOGUES = [("elt_relu", True, True, False, "s8"), ("elt", True, False, False, "s8"),
                   ("plain_u8", False, False, True, "u8"), ("plain_s8", False, False, False, "s8")]
GPOOL_LAUNCHES = 3
S_IN, S_OUT, S_RES = 0.03, 0.05, 0.04


def gpool_case(H, W, N, cout, epi):
    """the weights (quantised by the oracle), bias and GPOOL_LAUNCHES different (x, residual) pairs of one case"""
    from oracle import oracle as O
    name, elt, res_relu, relu, odt = epi
    seed = zlib.crc32(("gpool %d %d %d %d %s" % (H, W, N, cout, name)).encode())
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((cout, CIN, 1, 1)) * np.sqrt(2.0 / CIN)).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.5).astype(np.float32)
    ws = O.weight_scales(w)
    wq = O.quant_weights(w, ws)
    xs = [rng.integers(0, 256, (N, H, W, CIN)).astype(np.uint8) for _ in range(GPOOL_LAUNCHES)]      # (res5c_branch2c reads u8)
    rs = [rng.integers(-128, 128, (N, H, W, cout)).astype(np.int8) for _ in range(GPOOL_LAUNCHES)]
    return wq, ws, b, xs, rs


def gpool_coeff(pair):
    """the eltwise's coefficient pair: `pair` as multiples of c = 1 / S_OUT (None: the network's (c, c))"""
    c = 1.0 / S_OUT
    return (c, c) if pair is None else (float(np.float32(pair[0] * c)), float(np.float32(pair[1] * c)))


def gpool_oracle(wq, ws, b, x, res, epi, pair=None, detail=None):
    """(y, y_pool) of the oracle: conv (+ eltwise), then the INT8 pooling op's global average of those bytes;
    detail: a dict that receives the conv's own bytes (the eltwise's first operand)"""
    from oracle import oracle as O
    name, elt, res_relu, relu, odt = epi
    od = O.U8 if odt == "u8" else O.S8
    bp, sc = O.conv_i8_prepare(ws, b, S_IN, S_OUT, O.U8, od)
    y = O.conv_i8(x, wq, bp, sc, od, int(relu))
    if elt:
        c = gpool_coeff(pair)
        if detail is not None:
            detail["t1"] = y
        y = O.eltwise_i8(y, res, S_OUT, S_RES, c[0], c[1], res_relu)
    return y, O.pool_i8_nhwc(y, None, None, None, 1, global_pool=True)


def gpool_op(N, H, W, cout, wq, ws, b, epi, pair=None):
    from anakin_amd import lib as L
    from anakin_amd import saber as S
    name, elt, res_relu, relu, odt = epi
    p = S.ConvParam(wq, b, 1, (0, 0), (1, 1), (1, 1), bool(relu), ws)
    if elt:
        p.res_mode, p.res_relu, p.sum_scale, p.coeff, p.scale_res = L.RES_ELTWISE, bool(res_relu), 1.0, gpool_coeff(pair), S_RES
    conv = S.SaberConv2D(int8=True).init((N, CIN, H, W), p, L.U8, L.U8 if odt == "u8" else L.S8, S_IN, S_OUT)
    conv.set_global_pooling()
    return conv


# ---- fc + softmax ------------------------------------------------------------------------------------------------------------------------
# (M rows, K reduction, N outputs, operand dtype)
FC_CASES = [(1, 512, 37, "s8"), (8, 2048, 1000, "s8"), (8, 2048, 1000, "u8"), (9, 1024, 1001, "s8"), (16, 4096, 1024, "s8")]
FC_IN_SCALE = 0.031
FC_LAUNCHES = 12


def fc_key(case):
    return "m%d_k%d_n%d_%s" % case


def fc_case(case):
    """(wq, ws, bias, out_scale, [FC_LAUNCHES inputs]) of one case; input 0 is the one the golden file's prob belongs to"""
    from oracle import oracle as O
    M, K, N, dt = case
    rng = np.random.default_rng(zlib.crc32(("fc " + fc_key(case)).encode()))
    w = (rng.standard_normal((N, K)) * 0.02).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    ws = O.weight_scales(w)
    wq = O.quant_weights(w, ws)
    if dt == "u8":
        xs = [rng.integers(0, 256, (M, K)).astype(np.uint8) for _ in range(FC_LAUNCHES)]
    else:
        xs = [rng.integers(-128, 128, (M, K)).astype(np.int8) for _ in range(FC_LAUNCHES)]
    return wq, ws, b, (0.5 if dt == "u8" else 1.0), xs


def fc_op(case, wq, ws, b, out_scale):
    from anakin_amd import lib as L
    from anakin_amd import saber as S
    M, K, N, dt = case
    return S.SaberFc(True).init(M, N, K, wq, b, L.U8 if dt == "u8" else L.S8, FC_IN_SCALE, out_scale, w_scale=ws)


def fc_oracle(case, wq, ws, b, out_scale, x):
    from oracle import oracle as O
    return O.fc_i8(x, wq, ws, FC_IN_SCALE, b, out_scale) if case[3] == "u8" else O.fc_i8(x, wq, ws, FC_IN_SCALE, b)


def fingerprint(*arrays):
    """crc32 of the inputs' bytes: the golden file carries it, so a prob recorded for other inputs is told from a changed kernel"""
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return np.uint32(c)
