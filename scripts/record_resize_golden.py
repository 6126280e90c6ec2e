"""Records tests/golden/resize_ref.npz from the reference's OWN resize code: the four template functions of
saber/funcs/impl/x86/saber_resize.cpp (resize_bilinear_align_kernel, resize_bilinear_no_align_kernel, resize_bilinear_custom_kernel,
resize_nearest_kernel), called through a small driver of our own that includes that file where it lies.

    python scripts/record_resize_golden.py [--ref /path/to/reference]

Needs the reference tree and g++; nothing of the reference is copied into the repository - the driver below names the file, the compiled
object lives in a temporary directory. The fixture holds, for every case of tests/resize_util.GOLDEN_CASES, the input (NCHW float32), the
parameters and the reference's output. The flags are the oracle's (oracle/Makefile REF_CXXFLAGS: -O2 -march=x86-64-v3 -ffp-contract=off)."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import resize_util as RU  # noqa: E402

DRIVER = r"""
#include "saber/funcs/impl/x86/saber_resize.cpp"
// NCHW-contiguous float tensors; the scale arguments are what SaberResize<X86>::dispatch passes: 1.f / scale with scale = out / in where the
// sizes are given, else the param's scale (saber_resize.cpp:247-284)
extern "C" int record_resize(int mode, int n, int c, int h_in, int w_in, int h_out, int w_out, float scale_h, float scale_w, int sizes_given,
                             const float* src, float* dst) {
    using namespace anakin::saber;
    float sw = sizes_given ? (float)w_out / w_in : scale_w, sh = sizes_given ? (float)h_out / h_in : scale_h;
    const int dsw = 1, dsh = w_out, dsc = w_out * h_out, dsb = dsc * c, ssw = 1, ssh = w_in, ssc = w_in * h_in, ssb = ssc * c;
    switch (mode) {
    case 0: resize_bilinear_align_kernel<float>(w_out, h_out, n, c, dsw, dsh, dsc, dsb, w_in, h_in, ssw, ssh, ssc, ssb, 1.f / sw, 1.f / sh, src, dst); break;
    case 1: resize_bilinear_no_align_kernel<float>(w_out, h_out, n, c, dsw, dsh, dsc, dsb, w_in, h_in, ssw, ssh, ssc, ssb, 1.f / sw, 1.f / sh, src, dst); break;
    case 2: resize_bilinear_custom_kernel<float>(w_out, h_out, n, c, dsw, dsh, dsc, dsb, w_in, h_in, ssw, ssh, ssc, ssb, 1.f / sw, 1.f / sh, src, dst); break;
    case 3: resize_nearest_kernel<float, true>(w_out, h_out, n, c, dsw, dsh, dsc, dsb, w_in, h_in, ssw, ssh, ssc, ssb, 1.f / sw, 1.f / sh, src, dst); break;
    default: return 1;
    }
    return 0;
}
"""


def build_driver(ref, tmp):
    src = os.path.join(tmp, "resize_driver.cpp")
    lib = os.path.join(tmp, "libresize_driver.so")
    with open(src, "w") as f:
        f.write(DRIVER)
    shim = os.path.join(ROOT, "oracle", "ref_shim")
    inc = [shim, ref] + [os.path.join(ref, d) for d in ("utils", "utils/logger", "saber", "saber/core", "saber/funcs", "framework")]
    cmd = ["g++", "-std=c++11", "-O2", "-march=x86-64-v3", "-include", "immintrin.h", "-include", "math.h", "-fopenmp", "-fPIC", "-w",
           "-ffp-contract=off", "-shared", "-o", lib, src] + ["-I" + d for d in inc]
    ref_lib = os.path.join(ROOT, "oracle", "_ref", "libanakin_x86_ref.so")      # the framework symbols SaberResize<X86>::dispatch itself refers to
    if os.path.exists(ref_lib):
        cmd += [ref_lib, "-Wl,-rpath," + os.path.dirname(ref_lib)]
    subprocess.check_call(cmd)
    return C.CDLL(lib)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "resize_ref.npz"))
    a = ap.parse_args()
    if not os.path.exists(os.path.join(a.ref, "saber", "funcs", "impl", "x86", "saber_resize.cpp")):
        sys.exit("the reference tree is not at %s" % a.ref)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_driver(a.ref, tmp)
        fp = C.POINTER(C.c_float)
        lib.record_resize.argtypes = [C.c_int] * 7 + [C.c_float, C.c_float, C.c_int, fp, fp]
        for name, cs in RU.GOLDEN_CASES.items():
            x = RU.make(cs, np.random.default_rng(RU.seed_of(name)))
            oh, ow = RU.out_hw(cs)
            y = np.full((cs["n"], cs["c"], oh, ow), np.nan, np.float32)
            rc = lib.record_resize(cs["mode"], cs["n"], cs["c"], cs["h"], cs["w"], oh, ow, cs["scale_h"], cs["scale_w"], int(RU.sizes_given(cs)),
                                   x.ctypes.data_as(fp), y.ctypes.data_as(fp))
            assert rc == 0 and not np.isnan(y).any(), name
            out[name + "/x"] = x
            out[name + "/y"] = y
            out[name + "/param"] = np.array([cs[k] for k in ("n", "c", "h", "w", "mode", "out_h", "out_w", "scale_h", "scale_w")], np.float64)
    np.savez_compressed(a.out, **out)
    print("wrote %s: %d cases, %d bytes" % (a.out, len(RU.GOLDEN_CASES), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
