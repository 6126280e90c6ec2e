"""Random deconv descriptors and form codes against the C ABI on a machine WITHOUT a GPU, in the style of tests/fuzz_desc.py
(tests/test_deconv_cpu.py runs it in a subprocess): every call returns a status, none crashes."""
import ctypes as C, os, sys, random
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from anakin_amd import lib as L
lib = L.load()
random.seed(int(sys.argv[1]) if len(sys.argv) > 1 else 1)
EDGE = [-2147483648, -7, -1, 0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 255, 256, 1000, 1 << 16, 1 << 20, (1 << 31) - 1]
SMALL = [0, 1, 2, 3, 4, 7, 8, 14, 16, 28, 56, 64, 112, 224, 256]
def val(): return random.choice(EDGE if random.random() < 0.35 else SMALL)
codes = {}
for it in range(int(sys.argv[2]) if len(sys.argv) > 2 else 3000):
    d = L.ConvDesc()
    for name, ty in d._fields_:
        if ty is C.c_int:
            setattr(d, name, val())
        else:
            setattr(d, name, random.choice([0.0, 1.0, -1.0, 1e-30, 1e30, float("inf"), float("nan"), 0.5]))
    if random.random() < 0.8:      # mostly plausible enums and no residual so that deeper validation is reached
        d.in_dtype, d.out_dtype = random.choice([0, 0, 0, 1, 2]), random.choice([0, 0, 0, 1, 2])
        d.in_layout, d.out_layout = random.choice([0, 1]), random.choice([0, 1])
        d.int8_weights = random.choice([0, 0, 1]); d.act = random.choice([0, 1, 2, 3]); d.res_mode = random.choice([0, 0, 0, 1, 2, 3]); d.group = random.choice([1, 1, 1, 2, 4, 0])
        d.res_act = d.res_stride = d.res_h = d.res_w = d.res_has_dtype = d.res_dtype = 0
        d.act_negative_slope = random.choice([0.0, 0.0, 0.0, 0.1, float("nan")])
        d.stride_h = d.stride_w = random.choice([1, 2, 0, 3]); d.dil_h = d.dil_w = random.choice([1, 1, 2, 0])
    h = C.c_void_p()
    rc = lib.saber_hip_deconv2d_create(C.byref(d), C.byref(h))
    codes[rc] = codes.get(rc, 0) + 1
    assert rc in (0, -2, -3), rc
    assert (rc == 0) == bool(h.value), (rc, h.value)
    if rc == 0:
        oh, ow = C.c_int(), C.c_int()
        lib.saber_hip_deconv2d_out_shape(h, C.byref(oh), C.byref(ow))
        assert oh.value >= 1 and ow.value >= 1
        assert lib.saber_hip_deconv2d_algo(h).startswith(b"deconv_")
        assert lib.saber_hip_deconv2d_run(h, None, None, None) == -2
        lib.saber_hip_deconv2d_destroy(h)
print("ok", codes)
ok = bad = st_ok = st_bad = 0
for it in range(2000):
    d = L.ConvDesc()
    d.n, d.h, d.w = random.choice([1, 2, 8]), random.choice([1, 7, 14, 28, 56, 224]), random.choice([1, 7, 14, 28, 56, 224])
    d.c, d.k = random.choice([3, 4, 16, 32, 64, 96, 128, 256, 512, 1024]), random.choice([8, 16, 40, 64, 128, 256, 1000])
    d.kh = d.kw = random.choice([1, 2, 2, 3, 4, 4, 5])
    d.pad_h = d.pad_w = random.choice([0, 1, 3])
    d.stride_h = d.stride_w = random.choice([1, 2, 2, 2]); d.dil_h = d.dil_w = random.choice([1, 1, 1, 2]); d.group = random.choice([1, 1, 1, 2, 4])
    d.in_dtype = d.out_dtype = L.F32
    d.in_layout, d.out_layout = random.choice([L.NHWC, L.NHWC, L.NCHW]), random.choice([L.NHWC, L.NHWC, L.NCHW])
    d.act = random.choice([0, 1])
    h = C.c_void_p()
    rc = lib.saber_hip_deconv2d_create(C.byref(d), C.byref(h))
    if rc != 0:
        assert rc == -2, rc
        bad += 1
        continue
    ok += 1
    eligible = (d.group == 1 and d.dil_h == 1 and d.stride_h == 2 and d.kh in (2, 3, 4) and d.pad_h <= d.kh - 1 and d.c % 32 == 0 and d.k % 16 == 0 and
                d.in_layout == L.NHWC and d.out_layout == L.NHWC)
    for _ in range(8):
        code = random.choice([0, 1, 2, 3, -1, 255, random.getrandbits(8), random.getrandbits(31)])
        before = (lib.saber_hip_deconv2d_get_tile(h), lib.saber_hip_deconv2d_algo(h))
        r2 = lib.saber_hip_deconv2d_set_tile(h, code)
        assert r2 == (0 if code == 0 or (eligible and code in (1, 2)) else -2), (code, r2, eligible)
        if r2 == 0:
            assert lib.saber_hip_deconv2d_get_tile(h) == code
            assert lib.saber_hip_deconv2d_algo(h) == [b"deconv_direct_f32", b"deconv_b3_f32_4x16", b"deconv_b3_f32_2x16"][code]
        else:
            assert (lib.saber_hip_deconv2d_get_tile(h), lib.saber_hip_deconv2d_algo(h)) == before, "a refused code changed the op"
        st_ok += r2 == 0
        st_bad += r2 != 0
    lib.saber_hip_deconv2d_destroy(h)
print("plausible deconvs: created %d, refused %d; set_tile accepted %d, refused %d" % (ok, bad, st_ok, st_bad))
