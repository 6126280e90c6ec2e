"""The deconv op without a GPU: the expected-value rule of tests/deconv_util.py against two independent statements of a transposed
convolution, the C ABI's shape / validation / selection, a descriptor fuzz, the fragment stream of the bf16-plane kernel, the proof that
the single-term probes separate a right kernel from a wrong one, the classes of the launch that the cases and the sweep's draws reach, and
a model of the kernel's tiling that shows which injected defects only the cases with more than one column tile catch."""
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


TIE_CASES = dict(DU.ALL_CASES, **DU.STRIDE_CASES)


def _torch_ref(x, w, b, cs):
    import torch
    return torch.nn.functional.conv_transpose2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), None if b is None else torch.from_numpy(b).double(),
                                                stride=cs["stride"], padding=cs["pad"], dilation=cs["dil"], groups=cs["group"]).numpy()


@pytest.mark.parametrize("name", sorted(TIE_CASES))
def test_numpy_rule_equals_torch_conv_transpose2d(name):
    """float64, 1e-12 of the largest value: groups, dilation and per-axis geometry included"""
    import torch
    cs = TIE_CASES[name]
    x, w, b = DU.make(cs, np.random.default_rng(FP._seed(name)))
    want = torch.nn.functional.conv_transpose2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(),
                                                stride=cs["stride"], padding=cs["pad"], dilation=cs["dil"], groups=cs["group"]).numpy()
    got = DU.deconv_ref(x, w, b, cs)
    assert got.shape == want.shape == (cs["n"], cs["k"]) + DU.out_hw(cs)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(DU.deconv_ref(x, w, b, cs, relu=True), np.maximum(got, 0.0))


@pytest.mark.parametrize("name", sorted(TIE_CASES))
def test_numpy_rule_equals_the_oracle_conv_on_the_zero_inserted_input(name):
    """the project's FP32 oracle conv (stride 1) on the input with stride - 1 zeros between pixels, weights flipped and transposed. The
    oracle accumulates in f32 over at most 128 * 16 terms of random sign: 1e-5 on the project's two criteria."""
    cs = TIE_CASES[name]
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


def test_b3_cases_reach_every_class_of_the_launch():
    """the classes of launch_deconv_b3_f32 (deconv_util.b3_classes) that B3_CASES holds: one, two and three or more column tiles, a last
    column tile of exactly 1 and of exactly 16 columns, two or more tiles both ways under both forms, 1 / 2 / >= 3 slabs and channel blocks,
    both orders of unequal pads, every k and a batch across a column seam. The cases from before the seam cases had one column tile each."""
    assert DU.b3_classes(DU.B3_CASES["seam_k4p1"]) == dict(q0=(0, 0), cells=(4, 17), tiles_x=2, tiles_y={1: 1, 2: 2}, last_cols=1, nslab=1, ntile=1,
                                                           nky=1, pads_equal=True)
    cl = DU.b3_classes(DU.B3_CASES["seam_k4p2x0"])
    assert (cl["q0"], cl["cells"], cl["tiles_x"], cl["nky"], cl["ntile"], cl["pads_equal"]) == ((1, 0), (8, 21), 2, 3, 9, False)
    cl = DU.b3_classes(DU.B3_CASES["seam_k4p1_twin"])
    assert (cl["cells"], cl["tiles_x"], cl["tiles_y"], cl["nslab"], cl["nky"]) == ((17, 34), 3, {1: 5, 2: 9}, 4, 2)
    for name in ("seam_k2p0_twin", "seam_k3p1_twin"):      # the smallest H and W with two tiles both ways under the 4 x 16 form
        cl = DU.b3_classes(DU.B3_CASES[name])
        assert cl["cells"] == (5, 17) and cl["nslab"] == 3 and DU.B3_CASES[name]["n"] == 2
    for name in ("seam_k4p1_probe", "seam_k3p1_probe"):
        cl = DU.b3_classes(DU.B3_CASES[name])
        assert cl["tiles_x"] >= 2 and cl["nslab"] >= 2 and name in DU.PROBE_CASES
    old = DU.b3_coverage(DU.B3_CASES[n] for n in DU.OLD_B3)
    assert all(DU.b3_classes(DU.B3_CASES[n])["tiles_x"] == 1 and DU.b3_classes(DU.B3_CASES[n])["pads_equal"] for n in DU.OLD_B3)
    assert not DU.REQUIRED_CLASSES <= old and old & DU.REQUIRED_CLASSES == {"tiles_x 1", "nslab 1", "nslab 2", "nslab 3", "nky 1", "nky 2"}
    now = DU.b3_coverage(DU.B3_CASES.values())
    assert DU.REQUIRED_CLASSES <= now, sorted(DU.REQUIRED_CLASSES - now)
    assert all(DU.macs(cs) <= DU.MAC_BUDGET for cs in list(DU.ALL_CASES.values()) + list(DU.STRIDE_CASES.values()))
    cs = DU.STRIDE_CASES["two_grid_strides"]
    assert cs["n"] * cs["k"] * np.prod(DU.out_hw(cs)) == 4259840 > 16384 * 256


# ---- a model of the bf16-plane kernel's TILING (float64; the plane arithmetic is the emulation's business above) ----------------------------
TILING_DEFECTS = {
    "halo_zero": "the halo columns left of c0 read as zero for tx > 0",
    "c0_no_q0": "c0 computed without q0_w",
    "pad_h_twice": "pad_h used for both axes in the epilogue",
    "stray_tile": "a tile past ntile stored, not skipped (the skip compares the tile's index inside its channel block)",
    "stale_slab": "slab cc >= 2 not staged: read from the buffer's previous contents (slab cc - 2)",
    "image_zero": "the image index dropped from the staging offset for tx > 0",
}


def tiled_model(x, w, bias, cs, th, defect=None):
    """deconv_b3_f32_kernel<KS, TH> restated in numpy, workgroup after workgroup in blockIdx order (channel blocks fastest, then column
    tiles, row tiles, images): cell origins q0 / c0, a (TH + HAL) x (16 + HAL) x 32-channel patch staged per slab into one of two buffers
    (pixels outside the image are zeros), the stream's [phase][tap] order reading rows HAL - ja .. and columns HAL - jb .. of the patch, four
    16-channel tiles per block with the tile index clamped to ntile - 1, the epilogue's (oh, ow) and its skips; stores go to a flat NHWC
    array at the kernel's offsets (one outside the array is dropped). Returns NCHW float64, NaN where nothing was stored."""
    N, C, H, W = x.shape
    K, ks, (ph, pw) = cs["k"], cs["kh"], cs["pad"]
    oh, ow = DU.out_hw(cs)
    cl = DU.b3_classes(cs)
    HAL = (ks + 1) // 2 - 1
    HWID = 16 + HAL
    (q0h, q0w), tiles_x, tiles_y = cl["q0"], cl["tiles_x"], cl["tiles_y"][{4: 1, 2: 2}[th]]
    nslab, ntile, nky = cl["nslab"], cl["ntile"], cl["nky"]
    xh = np.ascontiguousarray(x.transpose(0, 2, 3, 1)).astype(np.float64)
    w64 = w.astype(np.float64)
    b64 = np.zeros(nky * 64)
    if bias is not None:
        b64[:K] = bias
    y = np.full(N * oh * ow * K, np.nan)
    taps = [(rh, rw, ja, jb) for rh in range(2) for rw in range(2) for ja in range(ks // 2 if rh else (ks + 1) // 2)
            for jb in range(ks // 2 if rw else (ks + 1) // 2)]
    assert [(2 * rh + rw, rh + 2 * ja, rw + 2 * jb) for rh, rw, ja, jb in taps] == DU.stream_taps(ks)
    for blk in range(N * tiles_y * tiles_x * nky):
        ky, b = blk % nky, blk // nky
        tx, b = b % tiles_x, b // tiles_x
        ty, n = b % tiles_y, b // tiles_y
        q0, c0 = q0h + ty * th, (0 if defect == "c0_no_q0" else q0w) + tx * 16
        n_stage = 0 if defect == "image_zero" and tx > 0 else n
        iy, ix = q0 - HAL + np.arange(th + HAL), c0 - HAL + np.arange(HWID)
        oky, okx = (iy >= 0) & (iy < H), (ix >= 0) & (ix < W)
        if defect == "halo_zero" and tx > 0:
            okx[:HAL] = False
        lds = [np.zeros((th + HAL, HWID, 32)), np.zeros((th + HAL, HWID, 32))]

        def stage(cc, buf):
            lds[buf][:] = 0.0
            lds[buf][np.ix_(oky, okx)] = xh[n_stage][np.ix_(iy[oky], ix[okx])][:, :, cc * 32:(cc + 1) * 32]
        kch = np.concatenate([min(ky * 4 + i, ntile - 1) * 16 + np.arange(16) for i in range(4)])      # the block's 64 channels, clamped
        acc = np.zeros((4, 64, th, 16))
        stage(0, 0)
        for cc in range(nslab):
            L = lds[cc & 1]
            for rh, rw, ja, jb in taps:
                acc[2 * rh + rw] += np.einsum("yxc,ck->kyx", L[HAL - ja:HAL - ja + th, HAL - jb:HAL - jb + 16],
                                              w64[cc * 32:(cc + 1) * 32, kch, rh + 2 * ja, rw + 2 * jb])
            if cc + 1 < nslab and not (defect == "stale_slab" and cc + 1 >= 2):
                stage(cc + 1, (cc & 1) ^ 1)
        for i in range(4):
            t = ky * 4 + i
            if (i if defect == "stray_tile" else t) >= ntile:
                continue
            for p in range(4):
                oy = 2 * (q0 + np.arange(th)) + (p >> 1) - ph
                ox = 2 * (c0 + np.arange(16)) + (p & 1) - (ph if defect == "pad_h_twice" else pw)
                ok = ((oy >= 0) & (oy < oh))[:, None] & ((ox >= 0) & (ox < ow))[None, :]
                off = (((n * oh + oy[:, None]) * ow + ox[None, :]) * K + t * 16)[None] + np.arange(16)[:, None, None]
                val = acc[p, i * 16:(i + 1) * 16] + b64[t * 16:(t + 1) * 16, None, None]
                ok = np.broadcast_to(ok[None], off.shape) & (off < y.size)
                assert defect == "stray_tile" or t * 16 + 16 <= K
                y[off[ok]] = val[ok]
    return y.reshape(N, oh, ow, K).transpose(0, 3, 1, 2)


def _trips(got, want):
    try:
        DU.fp32_close(got, want, "model")
    except AssertionError:
        return True
    return False


def test_tiling_model_equals_the_rule_and_every_injected_defect_needs_a_seam_case(capsys):
    """unmodified, the model is the float64 rule on every bf16-plane case under both tile heights. Each defect of TILING_DEFECTS passes the
    project's two criteria on every case from before the seam cases - or trips "ragged" alone (three slabs, a second channel block) - and
    fails at least one seam case: the seam cases see what the older ones could not"""
    data = {}
    for name, cs in DU.B3_CASES.items():
        x, w, b = DU.make(cs, np.random.default_rng(FP._seed(name)))
        want = DU.deconv_ref(x, w, b, cs)
        data[name] = (x, w, b, want)
        for th in (4, 2):
            got = tiled_model(x, w, b, cs, th)
            assert not np.isnan(got).any(), (name, th)
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (name, th)
    report = []
    for defect, text in TILING_DEFECTS.items():
        tripped = []
        for name, cs in DU.B3_CASES.items():
            x, w, b, want = data[name]
            if any(_trips(tiled_model(x, w, b, cs, th, defect), want) for th in ((4, 2) if DU.macs(cs) < 3e7 else (4,))):
                tripped.append(name)
        old, new = [n for n in tripped if n in DU.OLD_B3], [n for n in tripped if n not in DU.OLD_B3]
        report.append("%s (%s): older cases tripped %s; seam cases tripped %s" % (defect, text, old or "none", new))
        assert set(old) <= {"ragged"}, (defect, old)
        assert new, defect
    with capsys.disabled():
        print("\n" + "\n".join(report))


@pytest.mark.parametrize("seed", DU.SWEEP_SEEDS)
def test_sweep_draws_cover_the_classes_and_the_rule_equals_torch_on_each(lib, seed):
    """deconv_util.sweep_draws, for the seeds the GPU test uses: no empty output, every draw inside the reference's budget and equal to
    conv_transpose2d; over the seeds (asserted under the last one) every class of the launch, every (k, column tiles, row tiles)
    combination, every layout pair, groups, depthwise, a dilation of 2, unequal strides"""
    draws = DU.sweep_draws(seed)
    assert len(draws["direct"]) == DU.SWEEP_DIRECT and len(draws["b3"]) == DU.SWEEP_B3
    assert repr(draws) == repr(DU.sweep_draws(seed))
    for kind in ("direct", "b3"):
        for d in draws[kind]:
            cs = d["cs"]
            assert min(DU.out_hw(cs)) >= 1 and DU.macs(cs) <= DU.MAC_BUDGET, cs
            x, w, b = DU.make(cs, np.random.default_rng(seed), bias=d["bias"])
            got, want = DU.deconv_ref(x, w, b, cs), _torch_ref(x, w, b, cs)
            assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), cs
            rc, h = _create(lib, _desc(cs, L.NCHW if d.get("in_nchw") else L.NHWC, L.NCHW if d.get("out_nchw") else L.NHWC, d["relu"]))
            assert rc == 0, (cs, lib.saber_hip_last_error())
            assert lib.saber_hip_deconv2d_set_tile(h, 1) == lib.saber_hip_deconv2d_set_tile(h, 2) == (0 if kind == "b3" else -2), cs
            lib.saber_hip_deconv2d_destroy(h)
    if seed != DU.SWEEP_SEEDS[-1]:
        return
    every = [DU.sweep_draws(s) for s in DU.SWEEP_SEEDS]
    b3 = [d["cs"] for dr in every for d in dr["b3"]]
    direct = [d for dr in every for d in dr["direct"]]
    now = DU.b3_coverage(b3)
    assert DU.REQUIRED_CLASSES <= now, sorted(DU.REQUIRED_CLASSES - now)
    assert {(cs["kh"], DU.b3_classes(cs)["tiles_x"], DU.b3_classes(cs)["tiles_y"][1]) for cs in b3} == {(k, a, c) for k in (2, 3, 4) for a in (1, 2, 3) for c in (1, 2, 3)}
    assert {cs["c"] for cs in b3} == {32, 64, 96, 128} and {cs["n"] for cs in b3} == {1, 2, 3}
    assert {(d["in_nchw"], d["out_nchw"]) for d in direct} == {(a, c) for a in (False, True) for c in (False, True)}
    cases = [d["cs"] for d in direct]
    assert all(cs["kh"] != cs["kw"] for cs in cases)
    assert any(cs["group"] == 1 for cs in cases) and any(1 < cs["group"] < cs["c"] for cs in cases) and any(cs["group"] == cs["c"] == cs["k"] > 1 for cs in cases)
    assert any(cs["dil"][0] > 1 for cs in cases) and any(cs["dil"][1] > 1 for cs in cases) and any(cs["stride"][0] != cs["stride"][1] for cs in cases)
    assert any(cs["pad"][0] != cs["pad"][1] for cs in cases) and {d["bias"] for d in direct} == {d["relu"] for d in direct} == {False, True}
    assert {cs["stride"][0] for cs in cases} == {1, 2, 3} and any(cs["c"] % 2 and cs["k"] % 2 for cs in cases)


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
