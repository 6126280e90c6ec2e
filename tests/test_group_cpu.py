"""Grouped 3x3 INT8 kernels and ResNeXt-50, host side (no GPU): which ops create() makes eligible for the grouped kernels (kernel
selection variant 17), what set_tile accepts, and the ResNeXt-50 32x4d model in the layer vocabulary of workloads.py."""
import ctypes as C
import os

import numpy as np
import pytest

from anakin_amd import build as B
from anakin_amd import lib as L
from anakin_amd import workloads as W
from tests import dw_util as DU
from tests import group_util as GU

V = GU.VARIANT


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(L.LIB_PATH) or os.path.exists("/opt/rocm/bin/hipcc"):
        B.build()
    return L.load()


def _create(lib, c, hw, int8=1, in_dt=L.U8, out_dt=L.U8, k=None, kh=3, stride=1, pad=1, dil=1, group=1, res_mode=L.RES_NONE, n=1):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.c, d.k, d.kh, d.kw = n, hw, hw, c, c if k is None else k, kh, kh
    d.pad_h = d.pad_w = pad
    d.stride_h = d.stride_w = stride
    d.dil_h = d.dil_w = dil
    d.group = group
    d.in_dtype, d.out_dtype, d.in_layout, d.out_layout, d.int8_weights = in_dt, out_dt, L.NHWC, L.NHWC, int8
    d.res_mode = res_mode
    d.sum_scale = 1.0
    h = C.c_void_p()
    assert lib.saber_hip_conv2d_create(C.byref(d), C.byref(h)) == 0, lib.saber_hip_last_error()
    return h


def _eligible_cases():
    combos = [(L.U8, L.U8), (L.S8, L.S8), (L.U8, L.F32), (L.S8, L.U8), (L.U8, L.S8), (L.S8, L.F32)]
    i = 0
    for c, hw in ((64, 9), (128, 14), (1024, 7)):
        for cg in GU.CGS:
            if cg == c:      # (one group: an ordinary convolution)
                continue
            for stride in (1, 2):
                in_dt, out_dt = combos[i % len(combos)]
                i += 1
                yield dict(c=c, hw=hw, group=c // cg, stride=stride, in_dt=in_dt, out_dt=out_dt)


def _ineligible_cases():
    yield dict(c=32, hw=14, group=4), "direct_i8"                                        # C % 64 != 0
    yield dict(c=64, k=128, hw=14, group=4), "direct_i8"                                 # Cg != Kg
    yield dict(c=64, hw=14, group=32), "direct_i8"                                       # Cg = 2
    yield dict(c=64, hw=14, group=4, kh=5, pad=2), "direct_i8"                           # 5x5
    yield dict(c=64, hw=14, group=4, dil=2, pad=2), "direct_i8"                          # dilation 2
    yield dict(c=64, hw=14, group=4, res_mode=L.RES_SUM_INPLACE), "direct_i8"            # a residual
    yield dict(c=64, hw=14, group=4, out_dt=L.S8, res_mode=L.RES_ELTWISE), "direct_i8"
    yield dict(c=64, hw=14, group=4, int8=0, in_dt=L.F32, out_dt=L.F32), "direct_f32"    # FP32 stays on the direct kernel
    yield dict(c=128, hw=14, group=32, int8=0, in_dt=L.F32, out_dt=L.F32), "direct_f32"


def test_grouped_selection_is_host_side(built):
    """create() decides eligibility from the descriptor alone: an eligible op answers get_tile in the variant-17 encoding and takes a
    g3x3_i8_ name when a form >= 1 is selected; every other grouped conv keeps the direct kernel, its name and its encoding."""
    seen = 0
    for kw in _eligible_cases():
        h = _create(built, **kw)
        assert built.saber_hip_conv2d_get_tile(h) >> 16 == V, kw
        forms = GU.group_forms(built, h)
        assert len(forms) >= 1, (kw, forms)
        for v in forms:
            assert built.saber_hip_conv2d_set_tile(h, (V << 16) | v) == 0
            assert built.saber_hip_conv2d_algo(h).decode().startswith("g3x3_i8_"), (kw, v, built.saber_hip_conv2d_algo(h))
        built.saber_hip_conv2d_destroy(h)
        seen += 1
    assert seen == (4 + 5 + 5) * 2
    for kw, name in _ineligible_cases():
        h = _create(built, **kw)
        assert built.saber_hip_conv2d_algo(h).decode() == name, (kw, built.saber_hip_conv2d_algo(h))
        assert built.saber_hip_conv2d_get_tile(h) >> 16 != V, kw
        built.saber_hip_conv2d_destroy(h)
    h = _create(built, c=64, hw=14, group=64)      # depthwise: still variant 16
    assert built.saber_hip_conv2d_get_tile(h) >> 16 == 16
    assert built.saber_hip_conv2d_set_tile(h, (V << 16) | 1) == -2
    assert built.saber_hip_conv2d_get_tile(h) >> 16 == 16
    built.saber_hip_conv2d_destroy(h)


def test_set_tile_variant_17(built):
    """(17 << 16) | v: accepted for v = 0 .. N on an eligible op and read back by get_tile; v = 0 is the direct kernel under its own
    name; refused with SaberInvalidValue (-2) for v = N + 1 and on every ineligible op, and a refused code changes nothing."""
    for kw in _eligible_cases():
        h = _create(built, **kw)
        n = len(GU.group_forms(built, h))
        for v in range(n + 1):
            assert built.saber_hip_conv2d_set_tile(h, (V << 16) | v) == 0, (kw, v)
            assert built.saber_hip_conv2d_get_tile(h) == (V << 16) | v
            name = built.saber_hip_conv2d_algo(h).decode()
            assert (name == "direct_i8") if v == 0 else name.startswith("g3x3_i8_"), (kw, v, name)
        for bad in ((V << 16) | (n + 1), (V << 16) | 255, (16 << 16) | 1):
            assert built.saber_hip_conv2d_set_tile(h, bad) == -2, (kw, bad)
            assert built.saber_hip_last_error()
            assert built.saber_hip_conv2d_get_tile(h) == (V << 16) | n      # a refused code changes nothing
        built.saber_hip_conv2d_destroy(h)
    for kw, name in _ineligible_cases():
        h = _create(built, **kw)
        before = built.saber_hip_conv2d_get_tile(h)
        for v in (0, 1, 2):
            assert built.saber_hip_conv2d_set_tile(h, (V << 16) | v) == -2, (kw, v)
        assert built.saber_hip_conv2d_algo(h).decode() == name
        assert built.saber_hip_conv2d_get_tile(h) == before
        built.saber_hip_conv2d_destroy(h)


def test_resnext50_model(orc):
    """The layer list (53 convs, 16 grouped, 4 230 479 872 MACs), where the strides sit, that the reference's optimiser leaves it alone
    (no shortcut pooling, no stride moved), and an INT8 oracle walk whose edges are not vacuous."""
    spec = W.resnext_spec()
    assert W.conv_macs(spec) == 4230479872
    convs = [l for l in spec if l["kind"] == "conv"]
    assert len(convs) == 53
    grouped = [l for l in convs if l.get("group", 1) > 1]
    assert len(grouped) == 16 and all(l["group"] == 32 and l["k"] == 3 and l["pad"] == 1 and l["cin"] == l["cout"] and
                                      l["name"].endswith("_branch2b") for l in grouped)
    assert sorted({(l["cin"], l["cin"] // 32, l["stride"]) for l in grouped}) == \
        [(128, 4, 1), (256, 8, 1), (256, 8, 2), (512, 16, 1), (512, 16, 2), (1024, 32, 1), (1024, 32, 2)]
    assert all(l["stride"] == 1 for l in convs if l["name"].endswith("_branch2a"))
    strided = sorted(l["name"] for l in convs if l["stride"] == 2)
    assert strided == sorted(["conv1"] + ["res%da_branch%s" % (s, b) for s in (3, 4, 5) for b in ("1", "2b")])
    by = {l["name"]: l for l in convs}
    assert (by["res2a_branch2a"]["cout"], by["res2a_branch2c"]["cout"], by["res5c_branch2b"]["cin"], by["res5c_branch2c"]["cout"]) == \
        (128, 256, 1024, 2048)
    model = W.build_model("resnext50_32x4d")
    assert model["params"]["res2a_branch2b"][0].shape == (128, 4, 3, 3)
    assert model["params"]["res5c_branch2b"][0].shape == (1024, 32, 3, 3)
    fs = W.framework_spec(spec, "int8")
    assert [l["name"] for l in fs if l["kind"] == "pool"] == ["pool1"]
    assert [(l["name"], l["stride"]) for l in fs if l["kind"] == "conv"] == [(l["name"], l["stride"]) for l in convs]
    assert all(l["odt"] == W.U8 for l in fs if l["kind"] == "conv" and l["name"].endswith(("_branch2a", "_branch2b")))
    x = W.make_input(2, hw=64)
    scales = W.calibrate(model, x)
    t = DU.run_int8(W.framework_model(model, "int8"), scales, x)
    for l in convs:      # not vacuous: no edge is stuck at a limit or collapsed to a few values
        e = t[l["name"]]
        assert len(np.unique(e)) >= 50, (l["name"], len(np.unique(e)))
        if l.get("group", 1) > 1:
            assert e.dtype == np.uint8 and t[l["src"]].dtype == np.uint8, l["name"]
    assert t["fc1000"].shape == (2, 1000) and np.isfinite(t["prob"]).all()


def test_existing_specs_count_their_old_macs():
    """resnet_spec shares its block builder with resnext_spec now: the old specs are what they were."""
    assert W.conv_macs(W.resnet_spec(50)) == 3857973248
    assert W.conv_macs(W.resnet_spec(101)) == 7570194432
    assert W.conv_macs(W.vgg16_spec()) == 15470264320
    assert W.conv_macs(W.mobilenet_v1_spec()) == 568740352
    assert all("group" not in l for l in W.resnet_spec(50) + W.resnet_spec(101) + W.vgg16_spec())
    r50 = {l["name"]: l for l in W.resnet_spec(50)}
    assert r50["res3a_branch2a"]["stride"] == 2 and r50["res3a_branch2b"]["stride"] == 1 and r50["res3a_branch2a"]["cout"] == 128


def test_fragment_planes_against_a_plain_grouped_convolution(built):
    """tests/cpp/group3x3_pack_check.cpp (built with the other C++ tests, needs no GPU): the library's group3x3_pack walked lane by lane
    with the kernels' index arithmetic equals a plain grouped convolution for every Cg class, input type, stride and pad, and no
    walk leaves the packed planes or the input."""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "group3x3_pack_check.bin")
    if not os.path.exists(exe) or os.path.exists("/opt/rocm/bin/hipcc"):
        B.build_cpp_tests()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "emulation ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
