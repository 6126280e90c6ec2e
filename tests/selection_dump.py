"""Kernel-selection dump of the C ABI on a machine WITHOUT a GPU: what every selection code does to a fixed list of operators and which
candidates the autotuners visit, as text that two builds of the library can be diffed on (SABER_MI355X_LIB selects the library).

The malloc-backed mock HIP runtime (integration/mock_hip/mock_hip.cpp) is built into a temporary directory and loaded globally BEFORE the
library, so the library's weight repacking runs, kernel launches are swallowed and event times read 0 (the first autotune candidate wins).
Run in a process of its own: once loaded, the mock shadows the HIP runtime for the rest of the process.

    python tests/selection_dump.py              the dump
    python tests/selection_dump.py --roundtrip  the operator table only, each accepted code followed by what set_tile(get_tile()) does on a
                                                fresh operator of the same descriptor (tests/test_abi.py asserts on these lines)
    python tests/selection_dump.py --chains     the conv-chain section only (the last section of the dump; tests/test_abi.py asserts on it)
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_tmp = tempfile.TemporaryDirectory()
_mock = os.path.join(_tmp.name, "libmock_hip.so")
subprocess.check_call(["g++", "-O1", "-shared", "-fPIC", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                       os.path.join(ROOT, "integration", "mock_hip", "mock_hip.cpp"), "-o", _mock])
C.CDLL(_mock, mode=C.RTLD_GLOBAL)
from anakin_amd import lib as L  # noqa: E402

lib = L.load()
assert lib.saber_hip_device_ok() == 1, "the mock runtime is not in front of the library"
os.environ["SABER_HIP_AUTOTUNE_LOG"] = "1"

KS = [0, 1, 2, 4, 0x11, 0x21, 0x31, 0x81, 0x82]
CODES = [tile | (ks << 8) | (var << 16) for var in range(18) for ks in KS for tile in range(16)]
# name: n, h = w, c, k, kernel, stride, group, int8, input dtype, input layout, output dtype
TABLE = [
    ("i8_3x3_c256", 8, 14, 256, 256, 3, 1, 1, 1, L.U8, L.NHWC, L.U8),
    ("i8_1x1_c64", 8, 56, 64, 256, 1, 1, 1, 1, L.U8, L.NHWC, L.U8),
    ("i8_3x3_c64_56", 8, 56, 64, 64, 3, 1, 1, 1, L.U8, L.NHWC, L.U8),
    ("i8_1x1_7x7img", 8, 7, 512, 2048, 1, 1, 1, 1, L.U8, L.NHWC, L.U8),
    ("i8_3x3_7x7img", 8, 7, 512, 512, 3, 1, 1, 1, L.U8, L.NHWC, L.U8),
    ("i8_stem", 8, 224, 3, 64, 7, 2, 1, 1, L.F32, L.NCHW, L.U8),
    ("f32_3x3_c64", 2, 56, 64, 64, 3, 1, 1, 0, L.F32, L.NHWC, L.F32),
    ("f32_1x1_c64", 2, 56, 64, 256, 1, 1, 1, 0, L.F32, L.NHWC, L.F32),
    ("f32_1x1_c128", 2, 28, 128, 512, 1, 1, 1, 0, L.F32, L.NHWC, L.F32),
    ("f32_1x1_c512", 2, 28, 512, 128, 1, 1, 1, 0, L.F32, L.NHWC, L.F32),
    ("f32_fc", 8, 1, 2048, 1000, 1, 1, 1, 0, L.F32, L.NHWC, L.F32),
    ("dw_i8", 8, 112, 32, 32, 3, 1, 32, 1, L.U8, L.NHWC, L.U8),
    ("dw_f32_s2", 8, 56, 64, 64, 3, 2, 64, 0, L.F32, L.NHWC, L.F32),
    ("direct_g4", 8, 14, 32, 32, 3, 1, 4, 1, L.U8, L.NHWC, L.U8),
]
_keep = []      # host buffers the library may still point at


def make(n, hw, c, k, kk, stride, group, int8, in_dt, in_layout, out_dt, act=0, pad=None, **more):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.c, d.k, d.kh, d.kw = n, hw, hw, c, k, kk, kk
    d.pad_h = d.pad_w = kk // 2 if pad is None else pad
    d.stride_h = d.stride_w = stride
    d.dil_h = d.dil_w = 1
    d.group = group
    d.in_dtype, d.out_dtype, d.in_layout, d.out_layout, d.int8_weights, d.act = in_dt, out_dt, in_layout, L.NHWC, int8, act
    d.sum_scale = d.coeff_conv = d.coeff_res = d.scale_res = 1.0
    for key, v in more.items():
        setattr(d, key, v)
    h = C.c_void_p()
    assert lib.saber_hip_conv2d_create(C.byref(d), C.byref(h)) == 0, lib.saber_hip_last_error()
    w = (np.random.default_rng(0).standard_normal((k, c // group, kk, kk)) * 0.1).astype(np.float32)
    assert lib.saber_hip_conv2d_set_weights(h, w.ctypes.data, L.F32, None, None, 0.05, 0.1) == 0, lib.saber_hip_last_error()
    return h


def state(h):
    return "%s 0x%06x" % (lib.saber_hip_conv2d_algo(h).decode(), lib.saber_hip_conv2d_get_tile(h))


def buf(nbytes):
    b = (C.c_char * max(int(nbytes), 256))()
    _keep.append(b)
    return C.cast(b, C.c_void_p)


def logged(fn):
    """fn() with the C library's stderr captured: (status, [candidate names in the order the autotuner timed them])"""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            rc = fn()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        text = f.read().decode()
    cands = []
    for ln in text.splitlines():
        if ln.startswith("autotune ["):      # "autotune [shape] name   12.34 us": the time column is dropped
            cands.append(ln.split("]", 1)[1].split()[0])
    return rc, cands


def autotune(tag, h, out_bytes):
    x, y, ws = buf(1 << 16), buf(out_bytes), buf(lib.saber_hip_conv2d_workspace_bytes(h))
    rc, cands = logged(lambda: lib.saber_hip_conv2d_autotune(h, x, y, y, ws, None, 3))
    for c in cands:
        print("cand %s %s" % (tag, c))
    print("autotune %s rc=%d candidates=%d -> %s" % (tag, rc, len(cands), state(h)))


def codes(tag, h, set_tile=None, show=state, code_list=CODES):
    for code in code_list:
        rc = (set_tile or lib.saber_hip_conv2d_set_tile)(h, code)
        print("code %s 0x%06x rc=%d %s" % (tag, code, rc, show(h)))


def out_bytes(row):
    n, hw, k, stride = row[1], row[2], row[4], row[6]
    return n * (hw // stride + 1) ** 2 * k * 4


def chain_section():
    """Chains formed by saber_hip_net_optimize: per chain head every code 0..15 through saber_hip_net_set_choice (status, get_choice, the names of the
    ops of the block; codes are applied in order to ONE net, a last line switches the head's chain off again), then the candidates
    saber_hip_net_autotune times. On the mock the placement probe fails, so the cooperative forms (codes 7, 15) and the stages are refused."""
    def block(tag, c, hw, stride=1, second=True, pair=False):
        net = C.c_void_p()
        assert lib.saber_hip_net_create(C.byref(net)) == 0
        t = lambda nbytes: lib.saber_hip_net_add_tensor(net, nbytes)      # noqa: E731
        m, k1 = hw * hw, 4 * c
        elt = dict(res_mode=L.RES_ELTWISE, res_act=L.ACT_RELU)
        if stride == 2:
            elt.update(res_stride=2, res_h=2 * hw, res_w=2 * hw)
        ops = [make(1, hw * stride, c, c, 3, stride, 1, 1, L.U8, L.NHWC, L.U8, act=L.ACT_RELU),
               make(1, hw, c, k1, 1, 1, 1, 1, L.U8, L.NHWC, L.S8, **elt)]
        x, res, y0, y1 = t(m * stride * stride * c), t(m * stride * stride * k1), t(m * c), t(m * k1)
        assert lib.saber_hip_net_add_conv(net, ops[0], x, y0, -1) >= 0, lib.saber_hip_last_error()
        assert lib.saber_hip_net_add_conv(net, ops[1], y0, y1, res) >= 0, lib.saber_hip_last_error()
        if pair:      # the next stage's branch1 | branch2a: 256 -> 512 | 128
            ops += [make(1, hw, k1, 512, 1, 1, 1, 1, L.S8, L.NHWC, L.S8), make(1, hw, k1, 128, 1, 1, 1, 1, L.S8, L.NHWC, L.U8, act=L.ACT_RELU)]
            p = C.c_void_p()
            assert lib.saber_hip_conv2d_create_pair(ops[2], ops[3], C.byref(p)) == 0, lib.saber_hip_last_error()
            ops.append(p)
            assert lib.saber_hip_net_add_conv_pair(net, p, y1, t(m * 512), t(m * 128)) >= 0, lib.saber_hip_last_error()
        elif second:
            ops.append(make(1, hw, k1, c, 1, 1, 1, 1, L.S8, L.NHWC, L.U8, act=L.ACT_RELU))
            assert lib.saber_hip_net_add_conv(net, ops[2], y1, t(m * c), -1) >= 0, lib.saber_hip_last_error()
        removed = lib.saber_hip_net_optimize(net, 16 | 32 | 256 | 1024)
        assert lib.saber_hip_net_finalize(net) == 0, lib.saber_hip_last_error()
        n = lib.saber_hip_net_num_ops(net)
        names = lambda: " | ".join(lib.saber_hip_net_op_name(net, i).decode() for i in range(n))      # noqa: E731
        print("chain %s optimize=%d ops=%d %s" % (tag, removed, n, names()))
        for i in range(n):
            bit = (lib.saber_hip_net_get_choice(net, i) >> 28) & 3      # 1: heads a 1x1 chain, 2: a 3x3 conv that leads one
            if not bit:
                continue
            for code in list(range(16)) + [0]:
                rc = lib.saber_hip_net_set_choice(net, i, (bit << 28) | (code << 24))
                print("chaincode %s op%d %2d rc=%d 0x%08x %s" % (tag, i, code, rc, lib.saber_hip_net_get_choice(net, i), names()))
        rc, cands = logged(lambda: lib.saber_hip_net_autotune(net, None, 3))
        for cd in cands:
            print("cand %s %s" % (tag, cd))
        print("autotune %s rc=%d candidates=%d -> %s %s" % (tag, rc, len(cands), " ".join("0x%08x" % lib.saber_hip_net_get_choice(net, i) for i in range(n)), names()))
        lib.saber_hip_net_destroy(net)
        for h in ops:
            lib.saber_hip_conv2d_destroy(h)

    for c, hw in ((64, 9), (128, 6), (256, 5), (512, 3)):
        block("block_c%d" % c, c, hw)
    for c in (128, 256):
        block("strided_head_c%d" % c, c, 4, stride=2, second=False)
    block("strided_head_pair", 64, 4, stride=2, pair=True)


if "--chains" in sys.argv:
    chain_section()
    sys.exit(0)
roundtrip = "--roundtrip" in sys.argv
for row in TABLE:
    name = row[0]
    h = make(*row[1:])
    print("create %s %s" % (name, state(h)))
    fresh = {}      # get_tile code -> what a fresh operator makes of it
    for code in CODES:
        rc = lib.saber_hip_conv2d_set_tile(h, code)
        print("code %s 0x%06x rc=%d %s" % (name, code, rc, state(h)))
        if roundtrip and rc == 0:
            g = lib.saber_hip_conv2d_get_tile(h)
            if g not in fresh:
                h2 = make(*row[1:])
                rc2 = lib.saber_hip_conv2d_set_tile(h2, g)
                fresh[g] = "rc=%d %s" % (rc2, state(h2))
                lib.saber_hip_conv2d_destroy(h2)
            print("roundtrip %s 0x%06x %s" % (name, code, fresh[g]))
    lib.saber_hip_conv2d_destroy(h)
    h = make(*row[1:])
    autotune(name, h, out_bytes(row))
    lib.saber_hip_conv2d_destroy(h)
if roundtrip:
    sys.exit(0)

# sibling pairs: two 1x1 convs 256 -> 1024 and 256 -> 256 over one 8 x 14 x 14 tensor
for tag, int8, dt in (("pair_i8", 1, L.U8), ("pair_f32", 0, L.F32)):
    a = make(8, 14, 256, 1024, 1, 1, 1, int8, dt, L.NHWC, dt)
    b = make(8, 14, 256, 256, 1, 1, 1, int8, dt, L.NHWC, dt)
    p = C.c_void_p()
    assert lib.saber_hip_conv2d_create_pair(a, b, C.byref(p)) == 0, lib.saber_hip_last_error()
    print("create %s %s" % (tag, state(p)))
    x, ya, yb = buf(1 << 16), buf(8 * 14 * 14 * 1024 * 4), buf(8 * 14 * 14 * 256 * 4)
    rc, cands = logged(lambda: lib.saber_hip_conv2d_autotune_pair(p, x, ya, yb, None, 3))
    for c in cands:
        print("cand %s %s" % (tag, c))
    print("autotune %s rc=%d candidates=%d -> %s" % (tag, rc, len(cands), state(p)))
    codes(tag, p)
    for h in (p, a, b):
        lib.saber_hip_conv2d_destroy(h)

# fused conv + pooling: the FP32 stem launch (variant 15) and the INT8 stem (a single kernel)
POOL = (0, 3, 3, 2, 2, 0, 0, 0)
h = make(2, 224, 3, 64, 7, 2, 1, 0, L.F32, L.NCHW, L.F32, act=L.ACT_RELU)
print("set_pooling stem_f32 rc=%d %s" % (lib.saber_hip_conv2d_set_pooling(h, *POOL), state(h)))
codes("stem_f32", h, code_list=[(15 << 16) | v for v in range(5)] + [7 << 16, 8 << 16, 1 << 16, 2])
autotune("stem_f32", h, 2 * 56 * 56 * 64 * 4)
lib.saber_hip_conv2d_destroy(h)
h = make(*TABLE[5][1:])
print("set_pooling stem_i8 rc=%d %s" % (lib.saber_hip_conv2d_set_pooling(h, *POOL), state(h)))
codes("stem_i8", h, code_list=[7 << 16, 8 << 16, 1 << 16, 2, 15 << 16])
autotune("stem_i8", h, out_bytes(TABLE[5]))
lib.saber_hip_conv2d_destroy(h)

# conv + fused global average pooling: pins the image-resident kernel
h = make(*TABLE[3][1:])
print("set_global_pooling gpool rc=%d %s" % (lib.saber_hip_conv2d_set_global_pooling(h), state(h)))
codes("gpool", h)
autotune("gpool", h, out_bytes(TABLE[3]))
lib.saber_hip_conv2d_destroy(h)

# fully connected, 8 x 2048 -> 1000
lib.saber_hip_fc_algo.argtypes = [C.c_void_p]
for tag, int8, dt in (("fc_i8_f32in", 1, L.F32), ("fc_i8_s8in", 1, L.S8), ("fc_f32", 0, L.F32)):
    f = L.FcDesc()
    f.m, f.n, f.k, f.in_dtype, f.int8_weights, f.w_is_kn = 8, 1000, 2048, dt, int8, 0
    h = C.c_void_p()
    assert lib.saber_hip_fc_create(C.byref(f), C.byref(h)) == 0, lib.saber_hip_last_error()
    w = (np.random.default_rng(0).standard_normal((1000, 2048)) * 0.1).astype(np.float32)
    assert lib.saber_hip_fc_set_weights(h, w.ctypes.data, L.F32, None, None, 0.05, 0.1) == 0, lib.saber_hip_last_error()
    print("create %s %s" % (tag, lib.saber_hip_fc_algo(h).decode()))
    codes(tag, h, set_tile=lib.saber_hip_fc_set_tile, show=lambda h: lib.saber_hip_fc_algo(h).decode())
    lib.saber_hip_fc_destroy(h)

chain_section()
