"""The resize op without a GPU: tests/resize_util.resize_ref against outputs recorded from the reference's own saber_resize.cpp
(tests/golden/resize_ref.npz, scripts/record_resize_golden.py), against a float64 evaluation of the same coordinates and against
torch.nn.functional.interpolate; that axes and modes are not interchangeable in any case; the host tables saber_hip_resize_create computes,
through tests/cpp/resize_table_check.cpp, bit for bit; output shapes and refused descriptors through the C ABI."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

from anakin_amd import build as B
from anakin_amd import lib as L
from tests import resize_util as RU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = RU.geometry_cases(2, 3)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH) or os.path.exists("/opt/rocm/bin/hipcc"):
        B.build()
    return L.load()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "resize_ref.npz"))


def _desc(cs, layout=L.NHWC, dtype=L.F32):
    d = L.ResizeDesc()
    d.n, d.c, d.h, d.w, d.mode = cs["n"], cs["c"], cs["h"], cs["w"], cs["mode"]
    d.scale_h, d.scale_w, d.out_h, d.out_w = cs["scale_h"], cs["scale_w"], cs["out_h"], cs["out_w"]
    d.in_layout = d.out_layout = layout
    d.dtype = dtype
    return d


def _create(lib, d):
    h = C.c_void_p()
    rc = lib.saber_hip_resize_create(C.byref(d), C.byref(h))
    return rc, h


def test_fixture_is_small_and_holds_the_golden_cases(golden):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "resize_ref.npz")) < 200 * 1024
    assert sorted({k.split("/")[0] for k in golden.files}) == sorted(RU.GOLDEN_CASES)
    assert {cs["mode"] for cs in RU.GOLDEN_CASES.values()} == {0, 1, 2, 3}
    for name, cs in RU.GOLDEN_CASES.items():
        assert list(golden[name + "/param"]) == [cs[k] for k in ("n", "c", "h", "w", "mode", "out_h", "out_w", "scale_h", "scale_w")], name


@pytest.mark.parametrize("name", sorted(RU.GOLDEN_CASES))
def test_resize_ref_equals_the_recorded_reference(golden, name):
    """Every mode, nearest AND bilinear, bit for bit. The bound the reference's build could justify for bilinear is 8 * 2^-24 * max|x| (up to
    four contracted products and three sums on identical taps); the recording was compiled without contraction and the measured difference
    is 0 on all 23 cases, so equality is what is asserted."""
    cs = RU.GOLDEN_CASES[name]
    x, want = golden[name + "/x"], golden[name + "/y"]
    got = RU.resize_ref(x, cs)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    diff = float(np.abs(got.astype(np.float64) - want).max())
    print("%s: max |resize_ref - recorded| = %g (bound %g)" % (name, diff, 8 * 2.0 ** -24 * float(np.abs(x).max())))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, diff)


@pytest.mark.parametrize("name", sorted(CASES))
def test_resize_ref_against_float64_and_interpolate(name):
    cs = CASES[name]
    x = RU.make(cs, np.random.default_rng(RU.seed_of(name)))
    y = RU.resize_ref(x, cs)
    xmax = float(np.abs(x).max())
    assert y.shape == (cs["n"], cs["c"]) + RU.out_hw(cs)
    e64 = float(np.abs(y - RU.resize_f64(x, cs)).max())
    assert e64 <= 1e-4 * xmax, (name, e64)
    if cs["mode"] in (RU.BILINEAR_ALIGN, RU.BILINEAR_NO_ALIGN):
        t = torch.nn.functional.interpolate(torch.from_numpy(x), size=RU.out_hw(cs), mode="bilinear", align_corners=cs["mode"] == RU.BILINEAR_ALIGN).numpy()
        et = float(np.abs(y - t).max())
        assert et <= 1e-5 * xmax, (name, et)


@pytest.mark.parametrize("name", sorted(CASES))
def test_axes_and_modes_are_not_interchangeable(name):
    """a kernel that swapped the two tables, or ran another mode's arithmetic, would be caught by this case: its output differs"""
    cs = CASES[name]
    x = RU.make(cs, np.random.default_rng(RU.seed_of(name)))
    y = RU.resize_ref(x, cs)
    oh, ow = RU.out_hw(cs)
    (h0, h1, fh), (w0, w1, fw) = RU.tables(cs)
    if (cs["h"], oh) != (cs["w"], ow):      # the two axes' tables differ: a kernel that read rows by the column table would be caught
        assert oh != ow or not (np.array_equal(h0, w0) and np.array_equal(h1, w1) and np.array_equal(fh, fw)), name
    else:
        assert name.startswith(("same_7x7", "ties_2x2_3x3")), name      # the two square geometries: their axes cannot be told apart by tables
    if (cs["h"], cs["w"]) == (oh, ow) or name == "to_1x1_m1":
        return      # identity: every mode copies; one output pixel: only mode 1 exists
    given = dict(cs, out_h=oh, out_w=ow)
    others = [m for m in RU.MODES if m != cs["mode"]]
    for m in others:
        z = RU.resize_ref(x, dict(given, mode=m))
        assert z.shape == y.shape and not np.array_equal(z, y), (name, "mode %d gives the same output" % m)


def _table_check(args):
    exe = os.path.join(ROOT, "tests", "cpp", "resize_table_check.bin")
    if not os.path.exists(exe) or os.path.exists("/opt/rocm/bin/hipcc"):
        B.build_cpp_tests()
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(ROOT, "anakin_amd"), env.get("LD_LIBRARY_PATH", "")])
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)


def test_host_tables_equal_resize_ref_bit_for_bit(lib):
    """every axis of every case (and a sweep of sizes per mode) through resize_axis_table, the function saber_hip_resize_create calls"""
    axes = []
    for cs in CASES.values():
        oh, ow = RU.out_hw(cs)
        g = RU.sizes_given(cs)
        axes += [(cs["mode"], cs["h"], oh, cs["scale_h"], g), (cs["mode"], cs["w"], ow, cs["scale_w"], g)]
    for m in RU.MODES:
        for n_in in (1, 2, 3, 7, 13, 14, 28, 56, 112, 1460):
            for n_out in (2, 3, 5, 14, 27, 56, 224, 1460):
                if m == RU.RESIZE_CUSTOM and n_out > n_in * 8:
                    continue
                axes.append((m, n_in, n_out, 0.0, True))
    axes = sorted(set(axes))
    args = []
    for m, n_in, n_out, sc, g in axes:
        args += [m, n_in, n_out, "%08x" % struct.unpack("<I", struct.pack("<f", sc))[0], int(g)]
    r = _table_check(args)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")
    at = 0
    for k, (m, n_in, n_out, sc, g) in enumerate(axes):
        assert lines[at] == "table %d 1" % k, (lines[at], axes[k])
        i0, i1, fr = RU.axis_table(m, n_in, n_out, sc, g)
        assert int(i0.max()) < n_in
        want = ["%d %d %08x" % (a, b, f) for a, b, f in zip(i0, i1, fr.view(np.uint32))]
        assert lines[at + 1:at + 1 + n_out] == want, axes[k]
        at += 1 + n_out
    r = _table_check([])
    assert r.returncode == 0 and "resize tables ok" in r.stdout, (r.stdout, r.stderr)


def test_output_shapes_follow_the_reference(lib):
    for name, cs in CASES.items():
        rc, h = _create(lib, _desc(cs))
        assert rc == 0, (name, lib.saber_hip_last_error())
        oh, ow = C.c_int(), C.c_int()
        lib.saber_hip_resize_out_shape(h, C.byref(oh), C.byref(ow))
        assert (oh.value, ow.value) == RU.out_hw(cs), name
        assert lib.saber_hip_resize_algo(h) == b"resize_direct_f32"      # (small: below the static rule's thresholds)
        assert lib.saber_hip_resize_set_tile(h, 1) == -2 and lib.saber_hip_resize_get_tile(h) == 0      # c = 3: no float4 of channels
        lib.saber_hip_resize_destroy(h)
    # floor of a FLOAT product: 10 * 0.7f = 7.0000005 -> 7 ...; a given size wins only where BOTH are given
    for h_in, sc, want in ((10, 0.7, 7), (7, 2.5, 17), (3, 1.0 / 3.0, 1), (9, 0.4, 3)):
        cs = RU.case(1, 4, h_in, h_in, RU.BILINEAR_NO_ALIGN, scale_h=sc, scale_w=sc)
        rc, h = _create(lib, _desc(cs))
        assert rc == 0
        oh, ow = C.c_int(), C.c_int()
        lib.saber_hip_resize_out_shape(h, C.byref(oh), C.byref(ow))
        assert oh.value == ow.value == want == RU.out_hw(cs)[0], (h_in, sc, oh.value)
        assert lib.saber_hip_resize_set_tile(h, 1) == 0 and lib.saber_hip_resize_get_tile(h) == 1 and lib.saber_hip_resize_algo(h) == b"resize_rows_f32"
        assert lib.saber_hip_resize_set_tile(h, 2) == -2 and lib.saber_hip_resize_get_tile(h) == 1
        lib.saber_hip_resize_destroy(h)
    cs = RU.case(1, 4, 6, 6, RU.BILINEAR_NO_ALIGN, out_h=9, out_w=-1, scale_h=2.0, scale_w=2.0)
    rc, h = _create(lib, _desc(cs))
    oh, ow = C.c_int(), C.c_int()
    lib.saber_hip_resize_out_shape(h, C.byref(oh), C.byref(ow))
    assert rc == 0 and (oh.value, ow.value) == (12, 12)
    lib.saber_hip_resize_destroy(h)
    # form 2: an integer x2 in mode 1 or 3, NHWC, c % 4 == 0; the static rule names the forms by output size (profiles/resize/README.md)
    for mode, h_in, oh_want, forms, algo in ((1, 6, 12, (0, 1, 2), b"resize_direct_f32"), (3, 6, 12, (0, 1, 2), b"resize_direct_f32"), (0, 6, 12, (0, 1), b"resize_direct_f32"),
                                             (2, 6, 12, (0, 1), b"resize_direct_f32"), (1, 6, 18, (0, 1), b"resize_direct_f32"),
                                             (3, 300, 600, (0, 1, 2), b"resize_rows_f32"), (1, 500, 1000, (0, 1, 2), b"resize_x2_f32"),
                                             (0, 500, 1000, (0, 1), b"resize_rows_f32")):
        rc, h = _create(lib, _desc(RU.case(1, 4, h_in, h_in, mode, oh_want, oh_want)))
        assert rc == 0 and lib.saber_hip_resize_algo(h) == algo, (mode, h_in, lib.saber_hip_resize_algo(h))
        assert tuple(f for f in range(4) if lib.saber_hip_resize_set_tile(h, f) == 0) == forms, (mode, h_in)
        lib.saber_hip_resize_destroy(h)
    for layout in (L.NCHW,):      # forms 1 and 2 are NHWC on both sides only
        rc, h = _create(lib, _desc(RU.case(1, 4, 6, 6, 1, 9, 9), layout))
        assert rc == 0 and lib.saber_hip_resize_set_tile(h, 1) == -2 and lib.saber_hip_resize_algo(h) == b"resize_direct_f32"
        lib.saber_hip_resize_destroy(h)


def test_refused_descriptors(lib):
    ok = RU.case(2, 4, 5, 7, RU.BILINEAR_NO_ALIGN, 11, 13)
    bad = [
        dict(ok, mode=RU.BILINEAR_ALIGN, out_h=1), dict(ok, mode=RU.BILINEAR_ALIGN, out_w=1),      # the reference divides by out - 1
        dict(ok, mode=RU.NEAREST_ALIGN, out_h=1), dict(ok, mode=RU.NEAREST_ALIGN, out_w=1),
        dict(ok, n=0), dict(ok, c=0), dict(ok, h=0), dict(ok, w=-1), dict(ok, out_h=0), dict(ok, out_w=-5),      # non-positive sizes
        dict(ok, mode=RU.RESIZE_CUSTOM, out_h=-1, out_w=-1), dict(ok, mode=RU.RESIZE_CUSTOM, out_h=-1, out_w=-1, scale_h=2.0, scale_w=-1.0),
        dict(ok, out_h=-1, out_w=-1, scale_h=0.01, scale_w=0.01),      # floor(in * scale) = 0
        dict(ok, mode=4), dict(ok, mode=-1),
    ]
    for cs in bad:
        rc, h = _create(lib, _desc(cs))
        assert rc == -2 and not h, (cs, rc)
    # (a table entry with i0 >= in cannot be reached through a descriptor whose sizes follow its scale: tests/cpp/resize_table_check.cpp
    # asks resize_axis_table for one directly)
    d = L.ResizeDesc()
    d.n, d.c, d.h, d.w, d.mode, d.scale_h, d.scale_w, d.out_h, d.out_w = 1, 4, 2, 2, RU.RESIZE_CUSTOM, 1.0, 1.0, -1, -1
    d.in_layout = 7
    assert _create(lib, d)[0] == -2
    # 8-bit: the reference has none
    for dt in (L.S8, L.U8):
        rc, h = _create(lib, _desc(ok, dtype=dt))
        assert rc == -3 and not h and b"FP32 only" in lib.saber_hip_last_error()
    assert lib.saber_hip_resize_create(None, None) == -2
