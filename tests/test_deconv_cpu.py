"""The deconv op without a GPU: the expected-value rule of tests/deconv_util.py against two independent statements of a transposed
convolution, the C ABI's shape / validation / selection, a descriptor fuzz, the fragment stream of the bf16-plane kernel, and the proof that
the single-term probes separate a right kernel from a wrong one."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from anakin_amd import build as B
from anakin_amd import lib as L
from oracle import oracle as O
from tests import deconv_util as DU
from tests import fp32_probe as FP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH) or os.path.exists("/opt/rocm/bin/hipcc"):
        B.build()
    return L.load()


def _desc(cs, in_layout=L.NHWC, out_layout=L.NHWC, relu=False):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.c, d.k, d.kh, d.kw = cs["n"], cs["h"], cs["w"], cs["c"], cs["k"], cs["kh"], cs["kw"]
    (d.stride_h, d.stride_w), (d.pad_h, d.pad_w), (d.dil_h, d.dil_w) = cs["stride"], cs["pad"], cs["dil"]
    d.group = cs["group"]
    d.in_dtype = d.out_dtype = L.F32
    d.in_layout, d.out_layout = in_layout, out_layout
    d.act = L.ACT_RELU if relu else L.ACT_NONE
    return d


def _create(lib, d):
    h = C.c_void_p()
    rc = lib.saber_hip_deconv2d_create(C.byref(d), C.byref(h))
    return rc, h


@pytest.mark.parametrize("name", sorted(DU.ALL_CASES))
def test_numpy_rule_equals_torch_conv_transpose2d(name):
    """float64, 1e-12 of the largest value: groups, dilation and per-axis geometry included"""
    import torch
    cs = DU.ALL_CASES[name]
    x, w, b = DU.make(cs, np.random.default_rng(FP._seed(name)))
    want = torch.nn.functional.conv_transpose2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(),
                                                stride=cs["stride"], padding=cs["pad"], dilation=cs["dil"], groups=cs["group"]).numpy()
    got = DU.deconv_ref(x, w, b, cs)
    assert got.shape == want.shape == (cs["n"], cs["k"]) + DU.out_hw(cs)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(DU.deconv_ref(x, w, b, cs, relu=True), np.maximum(got, 0.0))


@pytest.mark.parametrize("name", sorted(DU.ALL_CASES))
def test_numpy_rule_equals_the_oracle_conv_on_the_zero_inserted_input(name):
    """the project's FP32 oracle conv (stride 1) on the input with stride - 1 zeros between pixels, weights flipped and transposed. The
    oracle accumulates in f32 over at most 96 * 16 terms of random sign: 1e-5 on the project's two criteria."""
    cs = DU.ALL_CASES[name]
    x, w, b = DU.make(cs, np.random.default_rng(FP._seed(name)))
    xz, wc, pad, dil = DU.as_conv(x, w, cs)
    got = O.conv_f32_nchw(xz, wc, b, False, pad, (1, 1), dil, cs["group"])
    DU.fp32_close(got, DU.deconv_ref(x, w, b, cs), name, rtol=1e-5)


def test_out_shape_is_the_formula(lib):
    for name, cs in DU.ALL_CASES.items():
        rc, h = _create(lib, _desc(cs))
        assert rc == 0, (name, lib.saber_hip_last_error())
        oh, ow = C.c_int(), C.c_int()
        lib.saber_hip_deconv2d_out_shape(h, C.byref(oh), C.byref(ow))
        assert (oh.value, ow.value) == DU.out_hw(cs), name
        lib.saber_hip_deconv2d_destroy(h)
    # U-Net's decoder: 2x upsampling exactly; a generator's k4 s2 p1 likewise
    for cs, want in ((DU.case(1, 28, 28, 1024, 512, 2), (56, 56)), (DU.case(1, 8, 8, 512, 256, 4, pad=(1, 1)), (16, 16)),
                     (DU.case(1, 28, 28, 256, 128, 3, pad=(1, 1)), (55, 55))):
        assert DU.out_hw(cs) == want


def test_create_accepts_and_rejects_with_a_message(lib):
    base = DU.B3_CASES["k4s2p1"]
    for il in (L.NHWC, L.NCHW):
        for ol in (L.NHWC, L.NCHW):
            rc, h = _create(lib, _desc(base, il, ol, relu=True))
            assert rc == 0
            lib.saber_hip_deconv2d_destroy(h)

    def refused(status, text, **fields):
        d = _desc(base)
        for k, v in fields.items():
            setattr(d, k, v)
        rc, h = _create(lib, d)
        assert rc == status and not h.value, (fields, rc)
        assert text in lib.saber_hip_last_error(), (fields, lib.saber_hip_last_error())

    refused(-3, b"FP32 only", int8_weights=1)
    refused(-3, b"FP32 only", in_dtype=L.U8)
    refused(-3, b"FP32 only", out_dtype=L.S8)
    refused(-2, b"no residual mode", res_mode=L.RES_ELTWISE)
    refused(-2, b"no residual mode", res_mode=L.RES_SUM_INPLACE)
    refused(-2, b"no residual mode", res_act=1)
    refused(-2, b"no residual mode", res_stride=2)
    refused(-2, b"no residual mode", res_has_dtype=1)
    refused(-2, b"negative_slope", act=L.ACT_RELU, act_negative_slope=0.1)
    refused(-2, b"negative_slope", act_negative_slope=float("nan"))
    refused(-2, b"activation", act=2)
    refused(-2, b"geometry", kh=0)
    refused(-2, b"geometry", stride_w=0)
    refused(-2, b"geometry", pad_h=-1)
    refused(-2, b"geometry", pad_h=9)          # (5 - 1) * 2 + 4 - 18 < 1: empty output
    refused(-2, b"multiples of group", group=5)
    refused(-2, b"layout", in_layout=2)
    assert lib.saber_hip_deconv2d_create(None, None) == -2
    assert lib.saber_hip_deconv2d_set_weights(None, None, None) == -2
    assert lib.saber_hip_deconv2d_run(None, None, None, None) == -2
    assert lib.saber_hip_net_add_deconv(None, None, 0, 1) == -2
    rc, h = _create(lib, _desc(base))
    assert lib.saber_hip_deconv2d_run(h, C.c_void_p(16), C.c_void_p(32), None) == -2 and b"set_weights" in lib.saber_hip_last_error()
    lib.saber_hip_deconv2d_destroy(h)


def test_selection_names_a_kernel_from_shapes_alone(lib):
    """no device: create names the direct kernel or a bf16-plane form; set_tile accepts the bf16-plane forms exactly where the header says"""
    names = [b"deconv_direct_f32", b"deconv_b3_f32_4x16", b"deconv_b3_f32_2x16"]
    for name, cs in DU.ALL_CASES.items():
        rc, h = _create(lib, _desc(cs))
        assert rc == 0
        eligible = name in DU.B3_CASES
        assert lib.saber_hip_deconv2d_algo(h) in (names if eligible else names[:1]), name
        assert lib.saber_hip_deconv2d_algo(h) == names[lib.saber_hip_deconv2d_get_tile(h)]
        for form in (1, 2, 0):
            rc = lib.saber_hip_deconv2d_set_tile(h, form)
            assert rc == (0 if eligible or form == 0 else -2), (name, form)
            if rc == 0:
                assert lib.saber_hip_deconv2d_algo(h) == names[form] and lib.saber_hip_deconv2d_get_tile(h) == form
            else:
                assert b"no such form" in lib.saber_hip_last_error()
        assert lib.saber_hip_deconv2d_set_tile(h, 3) == -2 and lib.saber_hip_deconv2d_get_tile(h) == 0
        lib.saber_hip_deconv2d_destroy(h)
    # eligible shapes lose the bf16-plane forms with an NCHW side; every measured row of the static rule is an eligible shape
    for il, ol in ((L.NCHW, L.NHWC), (L.NHWC, L.NCHW)):
        rc, h = _create(lib, _desc(DU.B3_CASES["k2s2p0"], il, ol))
        assert lib.saber_hip_deconv2d_algo(h) == names[0] and lib.saber_hip_deconv2d_set_tile(h, 1) == -2
        lib.saber_hip_deconv2d_destroy(h)
    for (c, k, hw, ks, pad) in [(1024, 512, 28, 2, 0), (512, 256, 56, 2, 0), (256, 128, 112, 2, 0), (128, 64, 224, 2, 0), (512, 256, 8, 4, 1),
                                (256, 128, 16, 4, 1), (128, 64, 32, 4, 1), (64, 32, 64, 4, 1), (256, 128, 28, 3, 1)]:
        for n in (1, 8):
            rc, h = _create(lib, _desc(DU.case(n, hw, hw, c, k, ks, pad=(pad, pad))))
            assert rc == 0 and lib.saber_hip_deconv2d_algo(h) in names
            assert lib.saber_hip_deconv2d_set_tile(h, 2) == 0
            lib.saber_hip_deconv2d_destroy(h)


def test_descriptors_and_form_codes_fuzzed_without_gpu(lib):
    """tests/fuzz_deconv_desc.py in a subprocess (a crash would take pytest with it): every call returns a status"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz_deconv_desc.py"), "11", "1500"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    created = int(r.stdout.split("plausible deconvs: created")[1].split(",")[0])
    assert created > 1000, r.stdout[-500:]


def test_fragment_stream_holds_every_weight_once_per_plane(lib):
    """tests/cpp/deconv_pack_check.cpp (built with the other C++ tests, needs no GPU)"""
    exe = os.path.join(ROOT, "tests", "cpp", "deconv_pack_check.bin")
    if not os.path.exists(exe) or os.path.exists("/opt/rocm/bin/hipcc"):
        B.build_cpp_tests()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "deconv pack ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_phase_decomposition_reaches_every_tap_once():
    """the kernel's rule - phase r = (o + pad) mod 2 uses taps a = r + 2 j on input q - j - restated in deconv_util.phase_taps, against
    the definition o = i * 2 - pad + a, for every kernel size, pad and output coordinate"""
    for k in (2, 3, 4):
        for pad in range(k):
            H = 6
            oh = (H - 1) * 2 + k - 2 * pad
            for o in range(oh):
                by_rule = {(a, i) for a, i in DU.phase_taps(k, pad, o) if 0 <= i < H}
                by_def = {(a, i) for a in range(k) for i in range(H) if i * 2 - pad + a == o}
                assert by_rule == by_def, (k, pad, o)
    assert [len([t for t in DU.stream_taps(3) if t[0] == p]) for p in range(4)] == [4, 2, 2, 1]
    assert [len([t for t in DU.stream_taps(4) if t[0] == p]) for p in range(4)] == [4, 4, 4, 4]
    assert [len([t for t in DU.stream_taps(2) if t[0] == p]) for p in range(4)] == [1, 1, 1, 1]


def _some(passes):
    return [passes[i] for i in sorted({0, len(passes) // 2, len(passes) - 1})]


@pytest.mark.parametrize("name", DU.PROBE_CASES)
def test_probes_pass_the_emulation_and_fail_injected_defects(name):
    """every pass through fp32_probe.emulate (both rounding models of the f32 accumulate) and through the float64 rule is inside 4 u with
    full coverage; with the low plane of the weights lost, the mm product skipped, or taps 0 and 1 assigned to each other's phase it is not"""
    cs = DU.B3_CASES[name]
    pr = DU.build_probes(name)
    wpasses, wcov, reach = pr["weight"]
    apasses, xcov, poscov, xread = pr["activation"]
    assert (wcov | ~reach).all() and reach.any(axis=(2, 3)).all() and poscov.all() and np.array_equal(xcov, xread)
    assert xread.all() or name == "k4s2p3"
    for p in wpasses + apasses:
        for trunc in (False, True):
            p.check(FP.emulate(p, trunc=trunc), "%s emulated, trunc=%s" % (name, trunc))
        p.check(DU.deconv_ref(p.x, p.w, p.bias, cs).astype(np.float32), name + " float64 rule")
    for fam, passes in (("weight", wpasses), ("activation", apasses)):
        for defect in ("w_no_l", "no_mm"):
            assert any(len(p.failures(FP.emulate(p, defect=defect))) for p in _some(passes)), (name, fam, defect)
        # (an activation pass whose weights all sit on taps a >= 2 does not see the swap: the first pass starts at tap (0, 0))
        assert len(passes[0].failures(FP.emulate(DU.wrong_phase(passes[0])))), (name, fam, "wrong phase")


def test_static_rule_follows_the_measured_table(lib):
    """profiles/deconv/shapes.json (scripts/bench_deconv.py shapes): create names a bf16-plane form only on a measured row where that form
    is not above form 0 by more than form 0's own spread in the cold AND the warm figures, and then the fastest such form; every shape
    that was not measured runs form 0"""
    import json
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import bench_deconv as BD
    rows = json.load(open(os.path.join(ROOT, "profiles", "deconv", "shapes.json")))
    assert {(r["c"], r["k"], r["h"], r["ks"], r["pad"]) for r in rows} == set(BD.ROWS)
    named = 0
    for r in rows:
        _, _, _, _, ok = BD._judge(r)
        within = [f for f in sorted(ok) if ok[f]]
        st = BD.static_form(r)
        assert st == (int(min(within, key=lambda f: r["us"][f])[4:]) if within else 0), r
        named += st != 0
    assert named > 0
    for name, cs in DU.B3_CASES.items():      # unmeasured shapes
        rc, h = _create(lib, _desc(cs))
        assert rc == 0 and lib.saber_hip_deconv2d_get_tile(h) == 0, name
        lib.saber_hip_deconv2d_destroy(h)
