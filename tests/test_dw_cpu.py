"""Depthwise 3x3 kernels and MobileNet-v1, host side (no GPU): which ops create() makes eligible for the depthwise kernels
(kernel selection variant 16), what set_tile accepts, and the MobileNet-v1 model in the layer vocabulary of workloads.py."""
import ctypes as C
import os

import numpy as np
import pytest

from anakin_amd import build as B
from anakin_amd import lib as L
from anakin_amd import workloads as W
from tests import dw_util as DU


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(L.LIB_PATH) or os.path.exists("/opt/rocm/bin/hipcc"):
        B.build()
    return L.load()


def _create(lib, c, hw, int8, in_dt, out_dt, k=None, kh=3, stride=1, pad=1, dil=1, group=None, in_layout=L.NHWC, out_layout=L.NHWC,
            res_mode=L.RES_NONE, n=1):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.c, d.k, d.kh, d.kw = n, hw, hw, c, c if k is None else k, kh, kh
    d.pad_h = d.pad_w = pad
    d.stride_h = d.stride_w = stride
    d.dil_h = d.dil_w = dil
    d.group = c if group is None else group
    d.in_dtype, d.out_dtype, d.in_layout, d.out_layout, d.int8_weights = in_dt, out_dt, in_layout, out_layout, int8
    d.res_mode = res_mode
    d.sum_scale = 1.0
    h = C.c_void_p()
    assert lib.saber_hip_conv2d_create(C.byref(d), C.byref(h)) == 0, lib.saber_hip_last_error()
    return h


def _eligible_cases():
    for c, hw in ((32, 112), (1024, 7)):
        for stride in (1, 2):
            yield dict(c=c, hw=hw, stride=stride, int8=1, in_dt=L.U8, out_dt=L.U8), "i8"
            yield dict(c=c, hw=hw, stride=stride, int8=1, in_dt=L.S8, out_dt=L.F32), "i8"
            yield dict(c=c, hw=hw, stride=stride, int8=0, in_dt=L.F32, out_dt=L.F32), "f32"


def _ineligible_cases():
    i8 = dict(int8=1, in_dt=L.U8, out_dt=L.U8)
    yield dict(c=32, hw=14, group=4, **i8), "direct_i8"                       # grouped, not depthwise
    yield dict(c=32, k=64, hw=14, **i8), "direct_i8"                          # channel multiplier 2
    yield dict(c=32, hw=14, dil=2, pad=2, **i8), "direct_i8"                  # dilation 2
    yield dict(c=32, hw=14, kh=5, pad=2, **i8), "direct_i8"                   # 5x5
    yield dict(c=24, hw=14, **i8), "direct_i8"                                # INT8 with C % 16 != 0
    yield dict(c=32, hw=14, int8=0, in_dt=L.F32, out_dt=L.F32, out_layout=L.NCHW), "direct_f32"      # FP32 with NCHW output
    yield dict(c=32, hw=14, int8=1, in_dt=L.U8, out_dt=L.U8, res_mode=L.RES_SUM_INPLACE), "direct_i8"    # a residual
    yield dict(c=32, hw=14, int8=0, in_dt=L.F32, out_dt=L.F32, res_mode=L.RES_SUM_INPLACE), "direct_f32"


def test_depthwise_selection_is_host_side(built):
    """create() decides eligibility from the descriptor alone: an eligible op answers get_tile in the variant-16 encoding (whatever
    form is the static choice, the direct kernel included) and takes a depthwise form's name when one is selected; grouped convs that
    are not depthwise 3x3 keep the direct kernel and its name."""
    for kw, fam in _eligible_cases():
        h = _create(built, **kw)
        assert built.saber_hip_conv2d_get_tile(h) >> 16 == 16, kw
        forms = DU.dw_forms(built, h)
        assert len(forms) >= 2, (kw, forms)
        for v in forms:
            assert built.saber_hip_conv2d_set_tile(h, (16 << 16) | v) == 0
            assert built.saber_hip_conv2d_algo(h).decode().startswith("dw3x3_%s_" % fam), (kw, v, built.saber_hip_conv2d_algo(h))
        built.saber_hip_conv2d_destroy(h)
    for kw, name in _ineligible_cases():
        h = _create(built, **kw)
        assert built.saber_hip_conv2d_algo(h).decode() == name, (kw, built.saber_hip_conv2d_algo(h))
        assert built.saber_hip_conv2d_get_tile(h) >> 16 != 16, kw
        built.saber_hip_conv2d_destroy(h)


def test_set_tile_variant_16(built):
    """(16 << 16) | v: accepted for v = 0 .. N on an eligible op and read back by get_tile; v = 0 is the direct kernel under its own
    name; refused with SaberInvalidValue (-2) for v = N + 1 and on every ineligible op."""
    for kw, fam in _eligible_cases():
        h = _create(built, **kw)
        n = len(DU.dw_forms(built, h))
        for v in range(n + 1):
            assert built.saber_hip_conv2d_set_tile(h, (16 << 16) | v) == 0, (kw, v)
            assert built.saber_hip_conv2d_get_tile(h) == (16 << 16) | v
            name = built.saber_hip_conv2d_algo(h).decode()
            assert (name == "direct_" + fam) if v == 0 else name.startswith("dw3x3_%s_" % fam), (kw, v, name)
        assert built.saber_hip_conv2d_set_tile(h, (16 << 16) | (n + 1)) == -2
        assert built.saber_hip_last_error()
        assert built.saber_hip_conv2d_get_tile(h) == (16 << 16) | n      # a refused code changes nothing
        built.saber_hip_conv2d_destroy(h)
    for kw, name in _ineligible_cases():
        h = _create(built, **kw)
        for v in (0, 1, 2):
            assert built.saber_hip_conv2d_set_tile(h, (16 << 16) | v) == -2, (kw, v)
        assert built.saber_hip_conv2d_algo(h).decode() == name
        built.saber_hip_conv2d_destroy(h)


def test_mobilenet_v1_model(orc):
    """The layer list (27 convs, 13 depthwise, 568 740 352 MACs), its INT8 edge dtypes (all u8: the tail is a u8 average pooling and an
    fc with a u8 operand), and the INT8 oracle walk picking the class a float64 torch pass picks."""
    import torch
    import torch.nn.functional as Fn
    spec = W.mobilenet_v1_spec()
    assert W.conv_macs(spec) == 568740352
    convs = [l for l in spec if l["kind"] == "conv"]
    assert len(convs) == 27
    dws = [l for l in convs if l.get("group", 1) > 1]
    assert len(dws) == 13 and all(l["group"] == l["cin"] == l["cout"] and l["k"] == 3 and l["pad"] == 1 for l in dws)
    assert [(l["stride"], l["cout"]) for l in convs if l["k"] == 1 or l.get("group", 1) > 1][:4] == [(1, 32), (1, 64), (2, 64), (1, 128)]
    model = W.build_model("mobilenet_v1")
    assert model["params"]["conv2_dw"][0].shape == (32, 1, 3, 3)
    fs = W.framework_spec(spec, "int8")
    assert all(l["odt"] == W.U8 for l in fs if l["kind"] == "conv")
    assert [l.get("int8") for l in fs if l["kind"] == "gpool"] == [True]
    x = W.make_input(2)
    scales = W.calibrate(model, x)
    t = DU.run_int8(W.framework_model(model, "int8"), scales, x)
    assert t["pool6"].dtype == np.uint8 and t["conv14_sep"].dtype == np.uint8
    for l in convs:      # not vacuous: no edge is stuck at a limit or collapsed to a few values
        e = t[l["name"]]
        assert len(np.unique(e)) >= 50, (l["name"], len(np.unique(e)))
    y = torch.from_numpy(x).double()
    for l in spec:
        if l["kind"] == "conv":
            w, b = model["params"][l["name"]]
            y = torch.relu(Fn.conv2d(y, torch.from_numpy(w).double(), torch.from_numpy(b).double(), l["stride"], l["pad"], 1, l.get("group", 1)))
        elif l["kind"] == "gpool":
            y = y.mean((2, 3))
        elif l["kind"] == "fc":
            w, b = model["params"][l["name"]]
            y = Fn.linear(y, torch.from_numpy(w).double(), torch.from_numpy(b).double())
    assert list(t["fc7"].argmax(1)) == list(y.argmax(1).numpy()), (t["fc7"].argmax(1), y.argmax(1))


def test_existing_specs_count_the_same_macs():
    """conv_macs honours `group`; the specs without one count what they always did (ResNet50 3.86 G, VGG16 15.47 G)."""
    assert W.conv_macs(W.resnet_spec(50)) == 3857973248
    assert W.conv_macs(W.vgg16_spec()) == 15470264320
    assert all("group" not in l for l in W.resnet_spec(50) + W.resnet_spec(101) + W.vgg16_spec())
