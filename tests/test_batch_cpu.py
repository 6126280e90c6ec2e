"""What tests/test_gpu_batch.py relies on, checked without a GPU (tests/batch_util.py): the batch sizes cross the thresholds the library
switches on (8 images / XCDs / the stage limit, 16 fc rows, the published batch 32, 65 535 images on gridDim.y), the streaming cases lie
between one and two grid strides by a ragged amount, no two images of a case expect the same output, and the numpy references of
part B equal the oracle on a slice of the same case."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import batch_util as BU


def modulo_sensitive(y, m):
    """reading image i % m instead of image i changes the expected output"""
    n = y.shape[0]
    return n > m and not np.array_equal(y, y[np.arange(n) % m])


def test_batch_sizes_cross_every_threshold():
    assert BU.BATCHES == (9, 17, 33) and BU.BATCHES_COMPOSITE == (9, 17)
    assert min(BU.BATCHES) == BU.XCDS + 1 == BU.STAGE_MAX_BATCH + 1                # the first batch beyond the XCD count and the stage limit
    assert BU.BATCHES[1] == BU.FC_SMALL_MAX_ROWS + 1 and BU.BATCHES[1] % 2         # odd, the first beyond the small-batch fc kernels
    assert BU.BATCHES[2] == BU.PUBLISHED_BATCH + 1 and BU.BATCHES[2] % 2           # odd, beyond the published batch 32
    assert BU.FC_ROWS == (9, BU.FC_SMALL_MAX_ROWS, BU.FC_SMALL_MAX_ROWS + 1, 33) and BU.FC_F32_ROWS == (17, 33) and BU.GEMM_ROWS == 17
    assert BU.GPOOL_BATCHES == (65535, 65536) and BU.GPOOL_HWC == (2, 2, 4)
    n, (h, w, c) = BU.GPOOL_BATCHES[1], BU.GPOOL_HWC
    assert n * h * w * c == 1 << 20                                                # a megabyte of input, a quarter of output
    assert BU.POOL_N == 17 and BU.POOL_HW == (9, 7)


def test_conv_tables_hold_the_families_at_their_smallest_sizes():
    t = BU.I8_CONVS
    for name, (h, w, c, k, ks, pad, stride, group, idt, odt, relu, kind) in t.items():
        assert (h, w) in ((7, 9), (5, 17), (7, 7), (30, 30)), name
        assert c % group == 0 and k % group == 0 and (odt != BU.U8 or relu or kind), name
    assert t["pw_64_256"][2:5] == (64, 256, 1) and t["c3x3_64"][2:7] == (64, 64, 3, 1, 1)
    assert t["c3x3_64_s2"][4:7] == (3, 1, 2) and t["pw_64_128_s2"][4:7] == (1, 0, 2)
    assert t["stem_f32"][:7] == t["stem_s8"][:7] == (30, 30, 3, 64, 7, 3, 2) and t["stem_f32"][8] == BU.F32 and t["stem_s8"][8] == BU.S8
    assert {t[n][6] for n in ("dw_32_s1", "dw_32_s2")} == {1, 2} and all(t[n][2] == t[n][7] == 32 for n in ("dw_32_s1", "dw_32_s2"))
    assert (t["g16_64"][2], t["g16_64"][7], t["g2_64"][7]) == (64, 16, 2)
    assert t["c3_5x5"][2] == 3 and t["c3_5x5"][4] == 5 and t["c3_5x5"][7] == 1
    c, ks, group = t["direct_g2_5x5"][2], t["direct_g2_5x5"][4], t["direct_g2_5x5"][7]
    assert (c // group, ks) == (3, 5) and group > 1        # (api_conv.hip: a grouped INT8 conv outside the depthwise / grouped 3x3 kernels is direct_i8)
    assert sorted(v[11] for v in t.values() if v[11]) == ["elt", "sub", "sum"]
    assert BU.I8_ELT_PAIR[0] != BU.I8_ELT_PAIR[1]
    assert set(BU.F32_CONVS) == {"c3x3_64", "pw_256_64", "pw_64_128", "dw_32"}


@pytest.mark.parametrize("name", sorted(BU.I8_CONVS))
def test_int8_conv_images_expect_different_outputs(name):
    for n in BU.BATCHES:
        cs = BU.i8_conv(name, n)
        assert cs.want.shape[0] == n and BU.distinct_images(cs.want), (name, n)
        assert all(modulo_sensitive(cs.want, m) for m in (8, 16, 32) if m < n), (name, n)
        if cs.kind == "sub":
            oh, ow = cs.want.shape[1:3]
            assert ((cs.res_hw[0] - 1) // 2 + 1, (cs.res_hw[1] - 1) // 2 + 1) == (oh, ow) and cs.res.shape[1:3] == cs.res_hw
        if cs.kind == "elt":
            assert cs.coeff[0] != cs.coeff[1]


@pytest.mark.parametrize("name", sorted(BU.F32_CONVS))
def test_fp32_conv_images_expect_different_outputs(name):
    for n in BU.BATCHES_COMPOSITE:
        cs = BU.f32_conv(name, n)
        assert cs.want.shape[0] == n and BU.distinct_images(cs.want), (name, n)
        assert all(modulo_sensitive(cs.want, m) for m in (8, 16) if m < n)


def test_fc_rows_expect_different_outputs():
    for m in BU.FC_ROWS:
        cs = BU.fc_case(m)
        for want in (cs.want[BU.S8], cs.want[BU.U8], cs.want_f32):
            assert want.shape == (m, BU.FC_N) and BU.distinct_images(want), m
            assert all(modulo_sensitive(want, d) for d in (8, 16, 32) if d < m)


def test_pooling_over_batch_expects_different_outputs():
    """65 536 images of four average bytes cannot all differ; what the test needs is that an image index taken modulo 8, 16, 32 or the
    gridDim.y limit changes bytes, and that the last images (the ones a y-dimension overflow would lose) are not zero."""
    for n in BU.GPOOL_BATCHES:
        for dt in (BU.S8, BU.U8):
            want = O.pool_i8_nhwc(BU.gpool_input(n, dt), None, None, None, 1, global_pool=True)
            assert want.shape == (n, 1, 1, 4)
            assert all(modulo_sensitive(want, m) for m in (8, 16, 32, 65535) if m < n), (n, dt)
            assert want[-8:].any() and len({want[i].tobytes() for i in range(n)}) > 1000
    for i, (win, st, pad, pt, c) in enumerate(BU.POOL_CASES):
        for dt in (BU.S8, BU.U8):
            want = O.pool_i8_nhwc(BU.pool_input(i, dt), win, st, pad, pt)
            assert want.shape[0] == BU.POOL_N and BU.distinct_images(want), (i, dt)
    assert {c[3] for c in BU.POOL_CASES} == {0, 1, 2} and any(c[4] % 16 == 0 for c in BU.POOL_CASES) and any(c[4] % 4 for c in BU.POOL_CASES)


# ---- part B -------------------------------------------------------------------------------------------------------------------------------------
LAUNCHERS = {"launch_quantize_nchw_to_nhwc", "launch_dequantize_nhwc_to_nchw", "launch_transpose_nchw_to_nhwc_f32", "launch_transpose_nhwc_to_nchw_f32",
             "launch_quantize_flat_s8", "launch_eltwise_sum_i8", "launch_eltwise_sum_f32", "launch_relu_f32", "launch_activation_f32", "launch_prelu_f32",
             "launch_concat_nhwc", "launch_pool2d_i8_nhwc", "launch_pool2d_f32", "launch_pool2d_f32_from_i8"}


def test_the_cap_is_the_kernels_files():
    """the constant is quoted from anakin_amd/csrc/elementwise.hip: grid_for and the three inline spellings"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "anakin_amd", "csrc", "elementwise.hip")).read()
    assert BU.GRID_CAP == 8192 * 256 == 2097152
    assert re.search(r"static unsigned grid_for\(size_t total\) \{\s*size_t b = \(total \+ 255\) / 256;\s*if \(b > 8192\) b = 8192;", src)
    assert len(re.findall(r"/ 256 > 8192 \? 8192 :", src)) == 3
    for la in LAUNCHERS:
        assert ("hipError_t %s(" % la) in src, la
    assert {cs["launcher"] for cs in BU.STREAM_CASES.values()} == LAUNCHERS


@pytest.mark.parametrize("name", sorted(BU.STREAM_CASES) + ["pad_channels_i8"])
def test_streaming_cases_lie_between_one_and_two_grid_strides(name):
    cs = BU.PAD_CHANNELS_CASE if name == "pad_channels_i8" else BU.STREAM_CASES[name]
    assert BU.GRID_CAP < cs["items"] < 2 * BU.GRID_CAP, (name, cs["items"])
    assert cs["items"] % BU.BLOCK_LANES, (name, "a whole number of blocks")
    if "count" in cs and cs["launcher"] != "launch_quantize_flat_s8":
        vec = 16 if cs["launcher"] == "launch_eltwise_sum_i8" else 4
        assert cs["count"] % vec and cs["items"] == -(-cs["count"] // vec), (name, "no scalar tail")


def test_streaming_cases_cover_every_kernel_variant():
    s = BU.STREAM_CASES
    assert s["quantize_dword"]["c_pad"] % 4 == 0 and s["quantize_bytes"]["c_pad"] % 4 != 0
    assert [s["concat_unit%d" % u]["unit"] for u in (16, 4, 1)] == [16, 4, 1]
    for u in (16, 4, 1):
        assert BU.concat_unit(s["concat_unit%d" % u]["channels"]) == u
    # launch_pool2d_i8_nhwc: the 16-byte max kernel needs type 0 and c % 16 == 0; the generic one gets an average over ragged channel groups
    assert s["pool_i8_max_vec16"]["ptype"] == 0 and s["pool_i8_max_vec16"]["shape"][3] % 16 == 0
    assert s["pool_i8_avg"]["ptype"] == 1 and s["pool_i8_avg"]["shape"][3] % 4 != 0
    # launch_pool2d_f32: NHWC with c % 4 == 0 takes the float4 kernel, everything else the generic one in either layout
    assert s["pool_f32_nhwc_vec4"]["shape"][3] % 4 == 0 and s["pool_f32_nhwc"]["shape"][3] % 4 != 0 and s["pool_f32_nchw"]["layout"] == "nchw"
    # no pooling case is a global pooling (those kernels size their grids otherwise)
    for n in ("pool_i8_avg", "pool_i8_max_vec16", "pool_f32_nchw", "pool_f32_nhwc", "pool_f32_nhwc_vec4", "pool_f32_from_i8"):
        assert min(s[n]["shape"][1:3] if s[n].get("layout") != "nchw" else s[n]["shape"][2:4]) > 2
    # the largest case holds about 170 MB on the device (two operands and the result of the f32 sum, 4 bytes each; three of the s8 sum)
    assert 3 * 4 * s["eltwise_f32"]["count"] < 110 << 20 and 3 * s["eltwise_i8"]["count"] < 110 << 20


@pytest.mark.parametrize("name", sorted(BU.STREAM_CASES))
def test_numpy_references_equal_the_oracle_on_a_slice(name):
    a = BU.stream_inputs(name, small=True)
    want = BU.stream_oracle(name, a)
    got = BU.stream_reference(name, a, small=True)
    if want is None:      # copies: the two f32 transposes undo each other, the s8 concat holds every input at its offset
        cs = BU.STREAM_CASES[name]
        if cs["launcher"] == "launch_concat_nhwc":
            off = 0
            for i, c in enumerate(cs["channels"]):
                assert np.array_equal(got[:, off:off + c], a["x%d" % i])
                off += c
            assert got.shape[1] == off
        elif cs["launcher"] == "launch_transpose_nchw_to_nhwc_f32":
            n, c, h, w = a["x"].shape
            assert got.shape == (n, h, w, cs["c_pad"]) and not got[..., c:].any()
            assert all(got[i, y, x, ch] == a["x"][i, ch, y, x] for i, ch, y, x in ((0, 0, 0, 0), (0, 2, 8, 10), (0, 1, 3, 7)))
        else:
            n, h, w, cp = a["x"].shape
            assert got.shape == (n, cs["c"], h, w)
            assert all(got[i, ch, y, x] == a["x"][i, y, x, ch] for i, ch, y, x in ((0, 0, 0, 0), (1, 2, 8, 10), (1, 1, 3, 7)))
        return
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (name, int(np.count_nonzero(got != want)))
    if name.startswith("quantize"):      # the slice holds saturated values and, where the scale is a power of two, exact ties
        t = a["x"].astype(np.float64) / BU.STREAM_CASES[name]["scale"]
        assert (np.abs(t) > 300).any() and (BU.STREAM_CASES[name].get("odt") == BU.U8 or np.count_nonzero(t - np.floor(t) == 0.5) > 3), name
