"""Concat and SqueezeNet v1.1 without a GPU: the numpy restatement of the reference's u8 concat against a float64 derivation, the concat
entry points' argument checks, the squeezenet_v1_1 model entry (MACs, framework dtypes, calibration) and - against the parent commit's
recorded digests - that framework_spec emits for every earlier model exactly what it emitted before it knew concat entries."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from anakin_amd import lib as L
from anakin_amd import workloads as W
from tests import fire_util as FU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -2


# ---- the u8 concat arithmetic ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0.5, 1.5, 2.5, 3.0, 0.75, 1.2345678, 0.3333333, 1.0000001, 127.0 / 255.0, 2.0078740])
def test_u8_restatement_agrees_with_float64_except_at_ties(m):
    x = np.arange(256, dtype=np.uint8)
    got = FU.concat_u8_one(x, m)
    away, tie = FU.concat_u8_f64(x, m)
    assert np.array_equal(got[~tie], away[~tie]), (m, np.nonzero(got != away)[0])
    # at an exact tie: the even neighbour (round to nearest even), saturated
    p = (x[tie].astype(np.float64) * np.float64(np.float32(m))).astype(np.float32).astype(np.float64)
    even = np.clip(2 * np.floor(p / 2 + 0.5), 0, 255).astype(np.uint8)
    assert np.array_equal(got[tie], even), m
    if m in (0.5, 1.5, 2.5):
        assert tie.sum() == 128 and np.any(got[tie] != away[tie])      # every odd byte is a tie; half of them round the other way
    if m >= 1.5:
        assert got.max() == 255 and np.count_nonzero(got == 255) > 1      # the rail


def test_multiplier_one_is_a_copy_and_direction_is_the_references():
    x = np.arange(256, dtype=np.uint8)
    assert np.array_equal(FU.concat_u8_one(x, 1.0), x)
    mult, out_scale = FU.concat_multipliers([0.02, 0.05, 0.05])
    assert out_scale == float(np.float32(0.05)) and mult[1] == mult[2] == np.float32(1.0)
    assert mult[0] == np.float32(0.05) / np.float32(0.02)      # scale_max / scale_i, as saber_concat.cpp:198 has it
    from anakin_amd import saber as S
    cat = S.SaberConcat().init([16, 16, 16], L.U8, [0.02, 0.05, 0.05])
    assert np.array_equal(cat.mult, mult) and cat.out_scale == out_scale
    assert S.SaberConcat().init([16, 16], L.U8, [0.05, 0.05]).mult is None      # equal scales: no multipliers, a copy
    assert S.SaberConcat().init([16, 16], L.S8, [0.02, 0.05]).mult is None      # s8: a copy whatever the scales


def test_concat_cases_are_deterministic():
    for name in FU.CONCAT_CASES:
        a, b = FU.concat_inputs(name), FU.concat_inputs(name)
        assert all(np.array_equal(p, q) for p, q in zip(a, b))
        dt, pixels, chans = FU.CONCAT_CASES[name]
        y = FU.concat_ref(a, FU.CONCAT_MULTS.get(name))
        assert y.shape == (pixels, sum(chans)) and y.dtype == FU.NP_DT[dt]
    assert {c for _, _, ch in FU.CONCAT_CASES.values() for c in ch} >= {1, 3, 16, 48, 100}
    assert {len(ch) for _, _, ch in FU.CONCAT_CASES.values()} >= {1, 2, 3, 8}


# ---- the entry points' argument checks (no device) ------------------------------------------------------------------------------------
def _ints(v):
    return (C.c_int * len(v))(*v)


def _floats(v):
    return (C.c_float * len(v))(*v)


def test_concat_entry_points_validate_without_gpu():
    lib = L.load()
    ptrs = (C.c_void_p * 9)(*[4096] * 9)      # never dereferenced: every call below is refused before a launch
    y = C.c_void_p(8192)
    for n in (0, -1, 9):
        assert lib.saber_hip_concat_nhwc(4, n, ptrs, _ints([16] * 9), None, L.S8, y, None) == INVALID, n
    assert b"1 .. 8" in lib.saber_hip_last_error()
    for bad in ([16, 0], [-3, 16]):
        assert lib.saber_hip_concat_nhwc(4, 2, ptrs, _ints(bad), None, L.U8, y, None) == INVALID, bad
    for dt in (L.S8, L.F32):
        assert lib.saber_hip_concat_nhwc(4, 2, ptrs, _ints([16, 16]), _floats([1.0, 1.0]), dt, y, None) == INVALID, dt
    assert b"u8" in lib.saber_hip_last_error()
    for bad in ([1.0, 0.0], [-1.0, 1.0], [float("nan"), 1.0], [float("inf"), 1.0]):
        assert lib.saber_hip_concat_nhwc(4, 2, ptrs, _ints([16, 16]), _floats(bad), L.U8, y, None) == INVALID, bad
    assert lib.saber_hip_concat_nhwc(4, 2, ptrs, _ints([16, 16]), None, L.S32, y, None) == INVALID
    assert lib.saber_hip_concat_nhwc(4, 2, None, _ints([16, 16]), None, L.S8, y, None) == INVALID
    assert lib.saber_hip_concat_nhwc(0, 2, ptrs, _ints([16, 16]), None, L.S8, y, None) == 0      # nothing to do

    net = C.c_void_p()
    assert lib.saber_hip_net_create(C.byref(net)) == 0
    a, b, out = (lib.saber_hip_net_add_tensor(net, 4 * 16), lib.saber_hip_net_add_tensor(net, 4 * 48), lib.saber_hip_net_add_tensor(net, 4 * 64))
    for n in (0, 9):
        assert lib.saber_hip_net_add_concat(net, 4, n, _ints([a] * 9), _ints([16] * 9), None, L.S8, out) == INVALID
    assert lib.saber_hip_net_add_concat(net, 4, 2, _ints([a, b]), _ints([16, 0]), None, L.U8, out) == INVALID
    assert lib.saber_hip_net_add_concat(net, 4, 2, _ints([a, b]), _ints([16, 48]), _floats([1.0, 2.0]), L.S8, out) == INVALID
    assert lib.saber_hip_net_add_concat(net, 4, 2, _ints([a, 7]), _ints([16, 48]), None, L.S8, out) == INVALID      # no such tensor
    assert lib.saber_hip_net_add_concat(net, 4, 2, _ints([a, out]), _ints([16, 48]), None, L.S8, out) == INVALID    # in place
    assert lib.saber_hip_net_add_concat(net, 5, 2, _ints([a, b]), _ints([16, 48]), None, L.S8, out) == INVALID      # tensors too small
    assert lib.saber_hip_net_add_concat(net, 4, 2, _ints([a, b]), _ints([16, 48]), None, L.F32, out) == INVALID     # ... for f32
    assert lib.saber_hip_net_num_ops(net) == 0
    i = lib.saber_hip_net_add_concat(net, 4, 2, _ints([a, b]), _ints([16, 48]), _floats([1.5, 1.0]), L.U8, out)
    assert i == 0 and lib.saber_hip_net_op_name(net, 0) == b"concat2"
    by, fl = C.c_double(), C.c_double()
    assert lib.saber_hip_net_op_work(net, 0, C.byref(by), C.byref(fl)) == 0
    assert (by.value, fl.value) == (2.0 * 4 * 64, 0.0)      # read + written, no flops
    # a third input: the work and the op name count it
    c = lib.saber_hip_net_add_tensor(net, 4 * 3)
    out3 = lib.saber_hip_net_add_tensor(net, 4 * 67)
    assert lib.saber_hip_net_add_concat(net, 4, 3, _ints([a, c, b]), _ints([16, 3, 48]), None, L.U8, out3) == 1
    assert lib.saber_hip_net_op_name(net, 1) == b"concat3"
    assert lib.saber_hip_net_op_work(net, 1, C.byref(by), C.byref(fl)) == 0 and by.value == 2.0 * 4 * 67
    assert lib.saber_hip_net_optimize(net, 15) == 0 and lib.saber_hip_net_num_ops(net) == 2      # nothing here to fuse; the ops stay
    lib.saber_hip_net_destroy(net)


# ---- the model entry ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def squeezenet():
    return W.build_model("squeezenet_v1_1")


def test_squeezenet_macs_and_shape(squeezenet):
    spec = squeezenet["spec"]
    assert W.conv_macs(spec) == FU.squeezenet_v1_1_macs() == 349151936
    assert W.conv_macs(spec, hw=63) == FU.squeezenet_v1_1_macs(63)
    fires = [l for l in spec if l["kind"] == "concat"]
    assert [l["name"] for l in fires] == ["fire%d_concat" % i for i in range(2, 10)]
    for l in fires:
        f = l["name"][:-len("_concat")]
        assert l["srcs"] == [f + "_expand1x1", f + "_expand3x3"]
    by = {l["name"]: l for l in spec}
    assert [(by["fire%d_squeeze1x1" % i]["cout"], by["fire%d_expand1x1" % i]["cout"], by["fire%d_expand3x3" % i]["cout"]) for i in range(2, 10)] == \
        [(16, 64, 64)] * 2 + [(32, 128, 128)] * 2 + [(48, 192, 192)] * 2 + [(64, 256, 256)] * 2
    assert all(len(squeezenet["params"][l["name"]]) == 2 and squeezenet["params"][l["name"]][1] is not None for l in spec if l["kind"] == "conv")
    assert not squeezenet["raw"]      # plain biases, no BatchNorm blobs
    assert W.algorithmic_bytes_int8(squeezenet, 1) > 0


def test_squeezenet_framework_dtypes(squeezenet):
    fw = W.framework_spec(squeezenet["spec"], "int8")
    by = {l["name"]: l for l in fw}
    assert [l["name"] for l in fw] == [l["name"] for l in squeezenet["spec"]]      # nothing inserted, nothing moved
    assert by["conv1"]["odt"] == W.S8                     # cin 3: the consumer, a pooling, decides
    assert all(l["odt"] == W.U8 for l in fw if l["kind"] == "conv" and l["name"] != "conv1")
    assert "int8" not in by["pool10"]                     # feeds the softmax, not an fc: the FP32 pooling fed an 8-bit edge
    assert W.framework_spec(squeezenet["spec"], "fp32") == squeezenet["spec"]


def test_calibration_gives_concat_inputs_one_scale(squeezenet):
    x = W.make_input(1, hw=63)
    scales = W.calibrate(squeezenet, x)
    for l in squeezenet["spec"]:
        if l["kind"] == "concat":
            a, b = l["srcs"]
            assert scales[a] == scales[b] == scales[l["name"]] > 0, l["name"]
            mult, out_scale = FU.concat_multipliers([scales[a], scales[b]])
            assert np.all(mult == np.float32(1.0)) and out_scale == float(np.float32(scales[l["name"]]))
    # the walk of the framework list: fire2 reads s8 (pool1 of the s8 conv1), every later Fire module u8
    fw = W.framework_model(squeezenet, "int8")
    ref = FU.run_int8(fw, scales, x)
    assert ref["pool1"].dtype == np.int8 and all(ref["fire%d_concat" % i].dtype == np.uint8 for i in range(2, 10))
    assert ref["fire2_concat"].shape == (1, 15, 15, 128) and ref["fire9_concat"].shape == (1, 3, 3, 512) and ref["prob"].shape == (1, 1000)
    assert np.array_equal(ref["fire5_concat"][..., :128], ref["fire5_expand1x1"]) and np.array_equal(ref["fire5_concat"][..., 128:], ref["fire5_expand3x3"])


# ---- earlier models: untouched -------------------------------------------------------------------------------------------------------------
def test_framework_spec_of_every_earlier_model_is_unchanged():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "framework_spec_parent.json")))
    specs = {"resnet50": lambda: W.resnet_spec(50), "resnet101": lambda: W.resnet_spec(101), "vgg16": W.vgg16_spec,
             "mobilenet_v1": W.mobilenet_v1_spec, "mobilenet_v2": W.mobilenet_v2_spec, "resnext50_32x4d": W.resnext_spec}
    assert sorted(want) == sorted("%s/%s" % (m, p) for m in specs for p in ("int8", "fp32"))
    for key, rec in want.items():
        name, prec = key.split("/")
        fw = W.framework_spec(specs[name](), prec)
        blob = json.dumps(fw, sort_keys=True, separators=(",", ":"))
        assert len(fw) == rec["entries"] and hashlib.sha256(blob.encode()).hexdigest() == rec["sha256"], key


# ---- the Fire module as one launch: what needs no GPU --------------------------------------------------------------------------------------
def test_fire_cases_are_deterministic_and_zero_x_tells_the_halos_apart():
    a, b = FU.FireCase(FU.GEOMETRIES["f"], FU.U8, FU.BIASES[0], 5), FU.FireCase(FU.GEOMETRIES["f"], FU.U8, FU.BIASES[0], 5)
    assert np.array_equal(a.y, b.y) and np.array_equal(a.s, b.s) and a.e1_scale == b.e1_scale != a.e3_scale
    assert a.y.shape == (3, 6, 6, 128) and np.array_equal(a.y[..., :48], a.e1) and np.array_equal(a.y[..., 48:], a.e3)      # E1 != E3: the offset
    for name in ("a", "b", "g1", "g2"):
        z = FU.fire_case(name, zero_x=True)
        assert not z.x.any() and z.s.min() > 0      # squeeze(0) = relu(bias') is not zero
        alt = z.e3_with_computed_halo()
        assert not np.array_equal(alt, z.e3), name      # a computed halo stores other bytes at the border ...
        assert np.array_equal(alt[:, 1:-1, 1:-1], z.e3[:, 1:-1, 1:-1])      # ... and the same bytes inside
    for name in ("c", "f"):      # sat: saturated and unsaturated bytes on the squeeze edge and on each half
        sc = FU.fire_case(name, sat=True)
        for t in (sc.s, sc.e1, sc.e3):
            hi, mid = FU.saturation(t)
            assert hi > 10 and mid > 10, name


def _conv(lib, c, hw, k, kh=1, pad=0, in_dt=L.U8, out_dt=L.U8, relu=True, stride=1, n=1, group=1):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.c, d.k, d.kh, d.kw = n, hw, hw, c, k, kh, kh
    d.pad_h = d.pad_w = pad
    d.stride_h = d.stride_w = stride
    d.dil_h = d.dil_w = 1
    d.group = group
    d.in_dtype, d.out_dtype, d.in_layout, d.out_layout, d.int8_weights = in_dt, out_dt, L.NHWC, L.NHWC, 1
    d.act, d.res_mode, d.sum_scale = (L.ACT_RELU if relu else L.ACT_NONE), L.RES_NONE, 1.0
    h = C.c_void_p()
    assert lib.saber_hip_conv2d_create(C.byref(d), C.byref(h)) == 0, lib.saber_hip_last_error()
    return h


def test_fire_entry_points_validate_without_gpu():
    """null operands: -2; a module in range whose ops never got weights: -3 naming the weights; out-of-range descriptors: -3 about the shape"""
    lib = L.load()
    out = C.c_void_p()
    sq, a, b = _conv(lib, 64, 13, 16), _conv(lib, 16, 13, 64), _conv(lib, 16, 13, 64, kh=3, pad=1)
    for args in ((None, a, b, C.byref(out)), (sq, None, b, C.byref(out)), (sq, a, None, C.byref(out)), (sq, a, b, None)):
        assert lib.saber_hip_conv2d_fire_create(*args) == INVALID and b"null" in lib.saber_hip_last_error()
    assert lib.saber_hip_conv2d_fire_create(sq, a, b, C.byref(out)) == L.UNIMPL and not out.value and b"weights" in lib.saber_hip_last_error()
    assert lib.saber_hip_conv2d_fire_run(None, None, None, None, None) == INVALID
    assert lib.saber_hip_conv2d_fire_set_tile(None, 1) == INVALID and lib.saber_hip_conv2d_fire_get_tile(None) == 0
    assert lib.saber_hip_conv2d_fire_algo(None) == b""
    lib.saber_hip_conv2d_fire_destroy(None)

    def refused(q, x1, x3, what):
        assert lib.saber_hip_conv2d_fire_create(q, x1, x3, C.byref(out)) == L.UNIMPL and not out.value, what
        msg = lib.saber_hip_last_error()
        assert msg.startswith(b"fire:") and b"weights" not in msg, (what, msg)
    refused(_conv(lib, 64, 13, 24), _conv(lib, 24, 13, 64), _conv(lib, 24, 13, 64, kh=3, pad=1), "S = 24")
    refused(_conv(lib, 64, 13, 80), _conv(lib, 80, 13, 64), _conv(lib, 80, 13, 64, kh=3, pad=1), "S = 80")
    refused(_conv(lib, 72, 13, 16), a, b, "C % 16")
    refused(_conv(lib, 528, 13, 16), a, b, "C > 512")
    refused(sq, _conv(lib, 16, 13, 72), b, "E1 % 16")
    refused(sq, a, _conv(lib, 16, 13, 520, kh=3, pad=1), "E3 > 512")
    refused(sq, b, a, "the expand convs swapped")
    refused(sq, a, _conv(lib, 16, 13, 64, kh=3, pad=0), "3x3 without padding")
    refused(sq, a, _conv(lib, 16, 13, 64, kh=3, pad=1, stride=2), "a strided 3x3")
    refused(sq, a, _conv(lib, 16, 13, 64, kh=3, pad=1, group=2), "a grouped 3x3")
    refused(_conv(lib, 64, 13, 16, relu=False, out_dt=L.S8), a, b, "squeeze without relu")
    refused(sq, _conv(lib, 16, 13, 64, relu=False, out_dt=L.S8), b, "expand1x1 -> s8")
    refused(sq, _conv(lib, 16, 13, 64, in_dt=L.S8), b, "expand1x1 reading s8")
    refused(sq, _conv(lib, 16, 11, 64), b, "another image size")
    refused(sq, _conv(lib, 32, 13, 64), b, "expand1x1 with c != S")
    refused(_conv(lib, 64, 13, 16, n=2), a, b, "another batch")


def test_fire_form_table_walk():
    """tests/cpp/fire_geom_check.cpp (built with the other C++ tests, needs no GPU): conv_fire_geom accepts and rejects what kernels.h says"""
    import subprocess
    from anakin_amd import build as B
    exe = os.path.join(ROOT, "tests", "cpp", "fire_geom_check.bin")
    if not os.path.exists(exe) or os.path.exists("/opt/rocm/bin/hipcc"):
        B.build_cpp_tests()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fire geom ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
