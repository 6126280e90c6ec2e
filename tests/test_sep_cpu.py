"""Separable pairs (depthwise 3x3 + pointwise 1x1 INT8 in one launch), host side (no GPU): what the entry points refuse before they touch
a device, the packed pointwise weight stream walked lane by lane against the OIHW weights for every launch form, and the oracle-side
preconditions of tests/test_gpu_sep.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from anakin_amd import build as B
from anakin_amd import lib as L
from oracle import oracle as O
from tests import int8_probe as P
from tests import sep_util as SU


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(L.LIB_PATH) or os.path.exists("/opt/rocm/bin/hipcc"):
        B.build()
    return L.load()


def _create(lib, c, hw, k=None, kh=3, stride=1, pad=1, group=1, in_dt=L.U8, out_dt=L.U8):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.c, d.k, d.kh, d.kw = 1, hw, hw, c, c if k is None else k, kh, kh
    d.pad_h = d.pad_w = pad
    d.stride_h = d.stride_w = stride
    d.dil_h = d.dil_w = 1
    d.group = group
    d.in_dtype, d.out_dtype, d.in_layout, d.out_layout, d.int8_weights = in_dt, out_dt, L.NHWC, L.NHWC, 1
    d.res_mode = L.RES_NONE
    d.sum_scale = 1.0
    h = C.c_void_p()
    assert lib.saber_hip_conv2d_create(C.byref(d), C.byref(h)) == 0, lib.saber_hip_last_error()
    return h


def test_entry_points_refuse_null_and_weightless_operands(built):
    """null operands: SaberInvalidValue (-2); operands whose weights were never set: SaberUnImplError (-3); a message each time, no object"""
    lib = built
    dw = _create(lib, 64, 14, group=64)
    pw = _create(lib, 64, 14, k=128, kh=1, pad=0)
    out = C.c_void_p()
    for a, b, o in ((None, pw, C.byref(out)), (dw, None, C.byref(out)), (dw, pw, None), (None, None, None)):
        assert lib.saber_hip_conv2d_sep_create(a, b, o) == -2
        assert b"null" in lib.saber_hip_last_error()
    assert lib.saber_hip_conv2d_sep_create(dw, pw, C.byref(out)) == -3 and not out.value
    assert b"weights" in lib.saber_hip_last_error()
    assert lib.saber_hip_conv2d_sep_run(None, None, None, None, None) == -2 and b"null" in lib.saber_hip_last_error()
    assert lib.saber_hip_conv2d_sep_set_tile(None, 1) == -2 and b"null" in lib.saber_hip_last_error()
    assert lib.saber_hip_conv2d_sep_get_tile(None) == 0
    assert lib.saber_hip_conv2d_sep_algo(None) == b""
    lib.saber_hip_conv2d_sep_destroy(None)
    lib.saber_hip_conv2d_destroy(dw)
    lib.saber_hip_conv2d_destroy(pw)


def test_packed_pointwise_stream_against_the_oihw_weights(built):
    """tests/cpp/sep_pack_check.cpp (built with the other C++ tests, needs no GPU): the library's sep_pw_pack walked lane by lane with phase
    1's index arithmetic equals a plain 1x1 convolution for C = 32, 64, 96, 1024 and every launch form; every output has one writer; no
    walk leaves the stream, the LDS tile or the output; at least two forms exist and one of them splits K"""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "sep_pack_check.bin")
    if not os.path.exists(exe) or os.path.exists("/opt/rocm/bin/hipcc"):
        B.build_cpp_tests()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "emulation ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_identity_depthwise_precondition_in_the_oracle():
    """test 4 of tests/test_gpu_sep.py runs the conv/pw_k64 probes behind a depthwise conv with centre tap 1, w_scale 1 and
    in_scale == out_scale: in the oracle that conv's output IS its input, for every probe image (so the probe's bytes reach the 1x1 conv)"""
    seen = 0
    for i, o, r in P.CONV_COMBOS:
        p = P.build("conv/pw_k64/%s%s/relu%d" % (P.DT_NAME[i], P.DT_NAME[o], r))
        c = p.geo[3]
        wq, ws, bp, sc = SU.identity_dw(c, p.idt, p.in_scale)
        assert np.all(sc == np.float32(1.0)) and (bp is None or not np.any(bp)), (p.name, sc[:4], bp)
        y = O.conv_i8(p.x, wq, bp, sc, p.idt, 0, (1, 1), (1, 1), group=c)
        assert y.dtype == p.x.dtype and np.array_equal(y, p.x), p.name
        seen += 1
    assert seen == 8


def test_cases_are_what_the_gpu_tests_say_they_are():
    """the geometries keep their edge cases, and the saturation cases saturate both edges without being stuck there"""
    g = SU.GEOMETRIES
    assert len(g) == 7 and len(SU.DTYPES) == 4
    assert g[0][1] == 32 and g[0][3] < 16 and g[0][0] == 2                    # half k-step, W < 16, two images
    assert g[1][4] == 2 and g[1][2] % 2 and g[1][3] % 2                       # odd dims at stride 2
    assert g[2][5] == 0                                                        # pad 0
    assert g[3][6] % 64 and (g[3][2] - 2) * (g[3][3] - 2) == 9                 # K % 64 != 0, 9-pixel images
    assert 16 < g[4][3] < 32 and g[4][3] % 16                                  # two ragged column tiles
    assert all(n * c * h * w > 0 and c % 32 == 0 and k % 32 == 0 for n, c, h, w, s, p, k in g)
    assert {SU.BIASES[(gi + di) % 4] for gi in range(7) for di in range(4)} == set(SU.BIASES)
    for di in range(4):
        cs = SU.case(0, di, sat=True)
        idt, mdt, odt, relu_dw, relu_pw = cs.dts
        for y, dt, relu in ((cs.mid, mdt, relu_dw), (cs.out, odt, relu_pw)):
            sat, unsat = SU.saturates(y, dt, relu)
            assert sat > 0 and unsat > 0, (di, sat, unsat)
