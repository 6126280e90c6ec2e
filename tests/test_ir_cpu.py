"""MobileNet-v2 as a model entry and the inverted-residual block launch, host side (no GPU): the layer list and its reference-side
rewrite, the calibration scales of an existing model (unchanged by calibrate honouring an eltwise layer's `relu`), what
saber_hip_conv2d_ir_create refuses before it touches a device, and both packed weight streams walked lane by lane against the OIHW
weights (tests/cpp/ir_pack_check.cpp). (A form code without a form leaving the selection unchanged needs an object, so weights on a device:
tests/test_gpu_ir.py::test_set_tile_and_run_refusals.)"""
import ctypes as C
import json
import os
import subprocess

import pytest

from anakin_amd import build as B
from anakin_amd import lib as L
from anakin_amd import workloads as W
from tests import ir_util as IU

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the model entry ---------------------------------------------------------------------------------------------------------------------------
def test_mobilenet_v2_spec():
    model = W.build_model("mobilenet_v2")      # (KeyError before the entry existed)
    spec = model["spec"]
    convs = [l for l in spec if l["kind"] == "conv"]
    elts = [l for l in spec if l["kind"] == "eltwise"]
    assert len(convs) == 52 and len(elts) == 10 and not any(l["relu"] for l in elts)
    assert sum(1 for l in convs if l["name"].endswith("_expand")) == 16 and sum(1 for l in convs if l["name"].endswith("_dwise")) == 17
    assert all(l["relu"] for l in convs if not l["name"].endswith("_linear")) and not any(l["relu"] for l in convs if l["name"].endswith("_linear"))
    assert "ReLU6" in W.mobilenet_v2_spec.__doc__
    # the edge shapes at 224: 112 after conv1, 7 x 7 x 320 into the last 1x1 conv, 1280 into the fc
    size, chan = {"data": 224}, {"data": 3}
    for l in spec:
        if l["kind"] == "conv":
            assert chan[l["src"]] == l["cin"], l
            size[l["name"]], chan[l["name"]] = (size[l["src"]] + 2 * l["pad"] - l["k"]) // l["stride"] + 1, l["cout"]
        elif l["kind"] == "eltwise":
            assert size[l["a"]] == size[l["b"]] and chan[l["a"]] == chan[l["b"]], l
            size[l["name"]], chan[l["name"]] = size[l["a"]], chan[l["a"]]
            assert next(c for c in convs if c["name"] == l["a"])["eltwise"] == l["name"]
    assert size["conv1"] == 112 and size["conv9"] == 7 and chan["conv9"] == 1280 and chan[next(l for l in spec if l["name"] == "conv9")["src"]] == 320
    assert [l["kind"] for l in spec[-3:]] == ["gpool", "fc", "softmax"] and spec[-2]["cin"] == 1280 and spec[-2]["cout"] == 1000
    # every expanded block is inside the block launch's scope
    for l in convs:
        if l["name"].endswith("_expand"):
            assert l["cin"] % 8 == 0 and 8 <= l["cin"] <= 192 and l["cout"] % 16 == 0 and l["cout"] <= 1024, l
        if l["name"].endswith("_linear"):
            assert l["cout"] % 8 == 0 and l["cout"] <= 320, l
    assert W.conv_macs(spec) == IU.mobilenet_v2_macs()
    assert set(model["params"]) == {l["name"] for l in spec if l["kind"] in ("conv", "fc")}


def test_mobilenet_v2_framework_spec():
    """no strided 1x1 conv reads an eltwise: the stride-up pass inserts no pooling and moves no stride; u8 after expand and depthwise, s8
    after project (and the sums are s8 by the executor's rule)"""
    spec = W.build_model("mobilenet_v2")["spec"]
    for prec in ("int8", "fp32"):
        fw = W.framework_spec(spec, prec)
        assert [l["name"] for l in fw] == [l["name"] for l in spec] and not any(l["kind"] == "pool" for l in fw)
        assert [l.get("stride") for l in fw] == [l.get("stride") for l in spec]
    fw = W.framework_spec(spec, "int8")
    for l in fw:
        if l["kind"] == "conv":
            want = W.S8 if l["name"].endswith("_linear") else W.U8
            assert l["odt"] == want, l
    assert next(l for l in fw if l["kind"] == "gpool")["int8"] is True


# ---- calibration -------------------------------------------------------------------------------------------------------------------------------
def test_calibrate_scales_of_an_existing_model_are_unchanged():
    """tests/golden/calibrate_mobilenet_v1_b1.json: the scales W.calibrate gave for mobilenet_v1 at batch 1 before it honoured an eltwise
    layer's `relu` (float.hex of every edge's scale); every existing spec has relu=True on its sums"""
    with open(os.path.join(HERE, "golden", "calibrate_mobilenet_v1_b1.json")) as f:
        want = {k: float.fromhex(v) for k, v in json.load(f).items()}
    model = W.build_model("mobilenet_v1")
    got = W.calibrate(model, W.make_input(1))
    assert got == want
    for spec in (W.resnet_spec(50), W.resnet_spec(101), W.resnext_spec(), W.vgg16_spec(), W.mobilenet_v1_spec()):
        assert all(l["relu"] for l in spec if l["kind"] == "eltwise")


def test_calibrate_honours_an_eltwise_without_relu():
    import numpy as np
    model = W.build_model("mobilenet_v2")
    x = W.make_input(1, hw=32)
    s = W.calibrate(model, x)
    relu_model = dict(model, spec=[dict(l, relu=True) if l["kind"] == "eltwise" else l for l in model["spec"]])
    s_relu = W.calibrate(relu_model, x)
    assert s["conv2_1_linear"] == s_relu["conv2_1_linear"]
    assert any(s[l["name"]] != s_relu[l["name"]] for l in model["spec"] if l["kind"] == "eltwise")
    assert all(np.isfinite(v) and v > 0 for v in s.values())


# ---- the entry points ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    if not os.path.exists(L.LIB_PATH) or os.path.exists("/opt/rocm/bin/hipcc"):
        B.build()
    return L.load()


def _create(lib, c, hw, k, kh=1, stride=1, pad=0, group=1, in_dt=L.U8, out_dt=L.U8, relu=True, res_mode=L.RES_NONE, res_stride=0, dil=1, n=1):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.c, d.k, d.kh, d.kw = n, hw, hw, c, k, kh, kh
    d.pad_h = d.pad_w = pad
    d.stride_h = d.stride_w = stride
    d.dil_h = d.dil_w = dil
    d.group = group
    d.in_dtype, d.out_dtype, d.in_layout, d.out_layout, d.int8_weights = in_dt, out_dt, L.NHWC, L.NHWC, 1
    d.act = L.ACT_RELU if relu else L.ACT_NONE
    d.res_mode = res_mode
    d.sum_scale = 1.0
    d.coeff_conv = d.coeff_res = d.scale_res = 1.0
    if res_stride > 1:
        d.res_stride, d.res_h, d.res_w = res_stride, (hw - 1) * res_stride + 1, (hw - 1) * res_stride + 1
    h = C.c_void_p()
    assert lib.saber_hip_conv2d_create(C.byref(d), C.byref(h)) == 0, lib.saber_hip_last_error()
    return h


def _block(lib, cin=24, ce=144, cout=24, hw=9, stride=1, in_dt=L.S8, res=False):
    ohw = (hw - 1) // stride + 1
    return (_create(lib, cin, hw, ce, in_dt=in_dt), _create(lib, ce, hw, ce, kh=3, stride=stride, pad=1, group=ce),
            _create(lib, ce, ohw, cout, out_dt=L.S8, relu=False, res_mode=L.RES_ELTWISE if res else L.RES_NONE))


def test_entry_points_refuse_null_and_weightless_operands(built):
    """null operands: SaberInvalidValue (-2); a block inside the scope whose ops never got weights: SaberUnImplError (-3) naming the
    weights; a message each time, no object"""
    lib = built
    ex, dw, pr = _block(lib)
    out = C.c_void_p()
    for a, b, c, o in ((None, dw, pr, C.byref(out)), (ex, None, pr, C.byref(out)), (ex, dw, None, C.byref(out)), (ex, dw, pr, None), (None,) * 4):
        assert lib.saber_hip_conv2d_ir_create(a, b, c, o) == -2
        assert b"null" in lib.saber_hip_last_error()
    for res in (False, True):
        ex, dw, pr = _block(lib, res=res)
        assert lib.saber_hip_conv2d_ir_create(ex, dw, pr, C.byref(out)) == -3 and not out.value
        assert b"weights" in lib.saber_hip_last_error()
    assert lib.saber_hip_conv2d_ir_run(None, None, None, None, None, None) == -2 and b"null" in lib.saber_hip_last_error()
    assert lib.saber_hip_conv2d_ir_set_tile(None, 1) == -2 and b"null" in lib.saber_hip_last_error()
    assert lib.saber_hip_conv2d_ir_get_tile(None) == 0
    assert lib.saber_hip_conv2d_ir_algo(None) == b""
    lib.saber_hip_conv2d_ir_destroy(None)


def test_out_of_scope_descriptors_are_refused(built):
    """each out-of-scope descriptor: SaberUnImplError (-3) with a message about the SHAPE (the scope is checked before the weights are)"""
    lib = built
    out = C.c_void_p()

    def refused(ex, dw, pr, what):
        assert lib.saber_hip_conv2d_ir_create(ex, dw, pr, C.byref(out)) == -3 and not out.value, what
        msg = lib.saber_hip_last_error()
        assert msg.startswith(b"inverted residual:") and b"weights" not in msg, (what, msg)
    ex, dw, pr = _block(lib)
    # the depthwise member
    refused(ex, _create(lib, 144, 9, 144, kh=3, stride=3, pad=1, group=144), _create(lib, 144, 3, 24, out_dt=L.S8, relu=False), "stride 3")
    refused(ex, _create(lib, 144, 9, 144, kh=3, pad=0, group=144), _create(lib, 144, 7, 24, out_dt=L.S8, relu=False), "pad 0")
    refused(ex, _create(lib, 144, 9, 144, kh=3, pad=2, group=144, dil=2), pr, "dilation 2")
    refused(ex, _create(lib, 144, 9, 144, kh=3, pad=1, group=144, relu=False), pr, "no relu on the depthwise conv")
    refused(ex, _create(lib, 144, 9, 144, kh=3, pad=1, group=144, out_dt=L.S8), pr, "s8 depthwise edge")
    refused(_create(lib, 24, 9, 152, in_dt=L.S8), _create(lib, 152, 9, 152, kh=3, pad=1, group=152), _create(lib, 152, 9, 24, out_dt=L.S8, relu=False),
            "Ce % 16 != 0")
    refused(_create(lib, 24, 9, 1040, in_dt=L.S8), _create(lib, 1040, 9, 1040, kh=3, pad=1, group=1040),
            _create(lib, 1040, 9, 24, out_dt=L.S8, relu=False), "Ce > 1024")
    # the expand member
    refused(_create(lib, 24, 9, 144, in_dt=L.S8, relu=False, out_dt=L.S8), dw, pr, "relu missing on expand")
    refused(_create(lib, 24, 9, 144, in_dt=L.S8, relu=False), dw, pr, "relu missing on expand, u8")
    refused(_create(lib, 20, 9, 144, in_dt=L.S8), dw, pr, "Cin % 8 != 0")
    refused(_create(lib, 200, 9, 144, in_dt=L.S8), dw, pr, "Cin > 192")
    refused(_create(lib, 24, 9, 144, kh=3, pad=1, in_dt=L.S8), dw, pr, "a 3x3 expand conv")
    refused(_create(lib, 24, 17, 144, stride=2, in_dt=L.S8), dw, pr, "a strided expand conv")
    refused(_create(lib, 24, 9, 144, in_dt=L.S8, out_dt=L.S8, relu=False, res_mode=L.RES_ELTWISE), dw, pr, "a residual on expand")
    refused(_create(lib, 24, 9, 144, in_dt=L.S8, n=2), dw, pr, "another batch")
    # the project member
    refused(ex, dw, _create(lib, 144, 9, 28, out_dt=L.S8, relu=False), "Cout % 8 != 0")
    refused(ex, dw, _create(lib, 144, 9, 328, out_dt=L.S8, relu=False), "Cout > 320")
    refused(ex, dw, _create(lib, 144, 9, 24, out_dt=L.S8, relu=True), "s8 with relu")
    refused(ex, dw, _create(lib, 144, 9, 24, out_dt=L.U8, relu=False), "u8 without relu")
    refused(ex, dw, _create(lib, 144, 9, 24, out_dt=L.F32, relu=False), "f32 output")
    refused(ex, dw, _create(lib, 144, 9, 24, kh=3, pad=1, out_dt=L.S8, relu=False), "a 3x3 project conv")
    refused(ex, dw, _create(lib, 144, 9, 32, out_dt=L.S8, relu=False, res_mode=L.RES_ELTWISE), "residual with Cin != Cout")
    refused(ex, dw, _create(lib, 144, 9, 24, out_dt=L.S8, relu=False, res_mode=L.RES_ELTWISE, res_stride=2), "res_stride = 2")
    e2, d2, p2 = _block(lib, hw=9, stride=2, res=True)
    refused(e2, d2, p2, "residual with stride 2")
    e3, d3, p3 = _block(lib, in_dt=L.U8, res=True)
    refused(e3, d3, p3, "u8 input with residual")
    # fused pooling: the only INT8 conv + pooling op is the stem (7x7 / 2 reading the f32 image): no member of a block
    d = L.ConvDesc()
    d.n, d.h, d.w, d.c, d.k, d.kh, d.kw = 1, 30, 30, 3, 64, 7, 7
    d.pad_h = d.pad_w = 3
    d.stride_h = d.stride_w = 2
    d.dil_h = d.dil_w = d.group = 1
    d.in_dtype, d.out_dtype, d.in_layout, d.out_layout, d.int8_weights = L.F32, L.U8, L.NCHW, L.NHWC, 1
    d.act, d.res_mode, d.sum_scale = L.ACT_RELU, L.RES_NONE, 1.0
    stem = C.c_void_p()
    assert lib.saber_hip_conv2d_create(C.byref(d), C.byref(stem)) == 0
    assert lib.saber_hip_conv2d_set_pooling(stem, 0, 3, 3, 2, 2, 0, 0, 0) == 0, lib.saber_hip_last_error()
    refused(stem, _create(lib, 64, 7, 64, kh=3, pad=1, group=64), _create(lib, 64, 7, 24, out_dt=L.S8, relu=False), "fused pooling")


def test_packed_streams_against_the_oihw_weights(built):
    """tests/cpp/ir_pack_check.cpp (built with the other C++ tests, needs no GPU): the library's ir_pack walked lane by lane with the kernel's
    index arithmetic equals two plain 1x1 convolutions for (Cin, Ce, Cout) = (16, 96, 24), (24, 144, 24), (160, 960, 320) and every launch
    form; every output has one writer; every tail of both streams is zero; no walk leaves a stream, an LDS buffer or the output"""
    exe = os.path.join(HERE, "cpp", "ir_pack_check.bin")
    if not os.path.exists(exe) or os.path.exists("/opt/rocm/bin/hipcc"):
        B.build_cpp_tests()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "emulation ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
