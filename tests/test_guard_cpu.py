"""The guard-band harness (tests/guard_util.py) catches what it claims to - on the CPU, without the library.

Plain numpy "kernels" for a pointwise op and a 3x3 convolution run on guarded CPU tensors. They address memory through each tensor's flat
uint8 buffer (payload at a byte offset), as a GPU kernel addresses raw pointers, so an access outside the tensor is possible and lands in
the guards. The correct versions pass the three checks of tests/test_gpu_guard.py (footprint, independence, value); each seeded defect
fails the check meant for it."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import guard_util as GU  # noqa: E402

VEC = 16


def _mem(t):
    """(flat uint8 numpy view of the whole guarded buffer, byte offset of tensor t's first element): raw memory and a pointer into it"""
    for g in _LIVE:
        if g is not None and g.t.data_ptr() == t.data_ptr():
            return g.buf.numpy(), g.lo
    raise KeyError("not a guarded tensor of this run")


_LIVE = []


@pytest.fixture(autouse=True)
def _registry(monkeypatch):
    """run_guarded hands the kernels plain tensors, as the library gets plain pointers; every Guarded made during a test is registered
    so that _mem can turn a tensor back into (memory, offset)"""
    del _LIVE[:]
    orig = GU.Guarded.__init__

    def init(self, *a, **kw):
        orig(self, *a, **kw)
        _LIVE.append(self)
    monkeypatch.setattr(GU.Guarded, "__init__", init)
    yield
    del _LIVE[:]


# ---- the models ------------------------------------------------------------------------------------------------------------------------
def relu_s8(x, y, n, defect=None):
    """y[i] = max(x[i], 0) on n s8 elements, 16 at a time with a masked tail"""
    mx, ox = _mem(x)
    my, oy = _mem(y)
    nvec = (n + VEC - 1) // VEC + (1 if defect == "store_vector_past_end" else 0)
    for v in range(nvec):
        lanes = np.arange(v * VEC, (v + 1) * VEC)
        ok = lanes < n
        src = mx[ox + np.where(ok, lanes, 0)].view(np.int8)                      # clamped load
        val = np.where(ok, np.maximum(src, 0), 0).astype(np.int8).view(np.uint8)
        if defect == "store_vector_past_end" and v == nvec - 1:
            my[oy + lanes] = val                                                  # an unmasked vector store one vector past the end
        else:
            my[oy + lanes[ok]] = val[ok]
    if defect == "store_before_start":
        my[oy - 1] = 0                                                            # one element before the start


def conv3x3(x, w, y, H, W, C, K, np_dt, defect=None):
    """NHWC 3x3 / pad 1 / stride 1 on one image, [H, W, C] -> [H, W, K], s8 (int32 accumulate, saturate) or f32; weights [K, 3, 3, C].
    Row by row: output row r reads input rows r - 1 .. r + 1; a row outside the image contributes nothing.
    defect 'row_past_end': the last output row's r + 1 row is loaded from memory instead of being masked."""
    mx, ox = _mem(x)
    my, oy = _mem(y)
    es = np.dtype(np_dt).itemsize
    acc_dt = np.int64 if np_dt == np.int8 else np.float32
    wk = w.astype(acc_dt)
    for r in range(H):
        acc = np.zeros((W, K), acc_dt)
        for kh in range(3):
            ir = r + kh - 1
            if ir < 0 or (ir >= H and defect != "row_past_end"):
                continue
            row = mx[ox + ir * W * C * es: ox + (ir + 1) * W * C * es].view(np_dt).reshape(W, C).astype(acc_dt)
            rp = np.zeros((W + 2, C), acc_dt)
            rp[1:-1] = row
            for kw in range(3):
                with np.errstate(invalid="ignore", over="ignore"):
                    acc += rp[kw:kw + W] @ wk[:, kh, kw, :].T
        out = np.clip(acc, -128, 127).astype(np.int8) if np_dt == np.int8 else acc.astype(np.float32)
        my[oy + r * W * K * es: oy + (r + 1) * W * K * es] = out.reshape(-1).view(np.uint8)


def conv3x3_ref(x, w, np_dt):
    H, W, C = x.shape
    K = w.shape[0]
    xp = np.zeros((H + 2, W + 2, C), np.float64)
    xp[1:-1, 1:-1] = x
    y = np.zeros((H, W, K), np.float64)
    for kh in range(3):
        for kw in range(3):
            y += xp[kh:kh + H, kw:kw + W] @ w[:, kh, kw, :].astype(np.float64).T
    return np.clip(y, -128, 127).astype(np.int8) if np_dt == np.int8 else y.astype(np.float32)


def channel_sum_via_workspace(x, y, ws, P, C, defect=None):
    """y[p] = sum over c of x[p, c] (s8 -> s32) through a workspace of C_pad = 4-rounded lanes per pixel: stage 1 copies the pixel's C
    channels into its lanes and zeroes the pad lanes, stage 2 sums all C_pad lanes. defect 'ws_lane': stage 1 leaves the pad lanes alone."""
    mx, ox = _mem(x)
    my, oy = _mem(y)
    mw, ow = _mem(ws)
    cp = (C + 3) // 4 * 4
    for p in range(P):
        mw[ow + p * cp: ow + p * cp + C] = mx[ox + p * C: ox + (p + 1) * C]
        if defect != "ws_lane":
            mw[ow + p * cp + C: ow + (p + 1) * cp] = 0
    for p in range(P):
        s = int(mw[ow + p * cp: ow + (p + 1) * cp].view(np.int8).astype(np.int64).sum())
        my[oy + 4 * p: oy + 4 * p + 4] = np.array([s], np.int32).view(np.uint8)


# ---- the layout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("np_dt", [np.uint8, np.int8, np.float32, np.int32])
@pytest.mark.parametrize("pattern", GU.PATTERNS)
def test_layout_alignment_abutting_guards_and_round_trip(np_dt, pattern):
    rng = np.random.default_rng(3)
    a = (rng.standard_normal((3, 5, 7)) * 50).astype(np_dt)
    g = GU.from_numpy(a, pattern, "cpu")
    assert g.t.data_ptr() % 256 == 16 and g.buf.data_ptr() % 512 == 0 and g.t.data_ptr() - g.buf.data_ptr() == GU.G + 16
    assert GU.G == 1 << 20 and g.buf.numel() == 2 * GU.G + 16 + a.nbytes               # no rounding after the payload
    assert g.t.shape == a.shape and g.t.dtype == GU.torch_dtype(np_dt) and GU.same_bytes(g.numpy(), a)
    raw = g.buf.numpy()
    assert (raw[:g.lo] == pattern).all() and (raw[g.hi:] == pattern).all() and g.hi - g.lo == a.nbytes
    assert GU.same_bytes(raw[g.lo:g.hi].view(np_dt).reshape(a.shape), a)
    assert g.intact() is None
    g.t.view(-1)[0] = g.t.view(-1)[0]                                                  # a write through the view stays inside
    g.t.mul_(1)
    assert g.intact() is None
    # the guards abut the payload: the byte before and the byte after are guard bytes, and intact() reports exactly them
    raw[g.lo - 1] ^= 0x01
    assert g.intact() == (-1, None)
    raw[g.lo - 1] ^= 0x01
    raw[g.hi] ^= 0x01
    assert g.intact() == (None, 0)
    raw[g.hi + 70000] ^= 0x80
    raw[7] ^= 0x10
    assert g.intact() == (7 - g.lo, 0)
    out = GU.guarded((4, 6), np_dt, pattern, "cpu")
    assert (out.bytes.numpy() == GU.SENTINEL).all() and out.intact() is None
    ws = GU.dirty(100, pattern, "cpu")
    assert ws.nbytes == 100 and (ws.buf.numpy() == pattern).all() and ws.t.data_ptr() % 256 == 16


def test_patterns_read_as_the_module_says():
    assert GU.SENTINEL not in GU.PATTERNS
    ff, a5 = np.full(4, 0xFF, np.uint8), np.full(4, 0x5A, np.uint8)
    assert ff.view(np.int8)[0] == -1 and np.isnan(ff.view(np.float32)[0]) and ff.view(np.int32)[0] == -1
    assert np.isfinite(a5.view(np.float32)[0]) and a5.view(np.float32)[0] > 1e16


# ---- pointwise: footprint ----------------------------------------------------------------------------------------------------------------
def _relu_case(n, defect):
    x = np.random.default_rng(n).integers(-128, 128, n).astype(np.int8)

    def launch(T, ws):
        relu_s8(T["x"], T["y"], n, defect)
    got = GU.run_guarded({"x": x}, {"y": ((n,), np.int8, None)}, launch, device="cpu", what="relu n=%d" % n)
    assert np.array_equal(got["y"], np.maximum(x, 0)), "value"


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4099])
def test_pointwise_correct_kernel_passes_all_three_checks(n):
    _relu_case(n, None)


@pytest.mark.parametrize("n", [1, 16, 17])
def test_store_one_vector_past_the_end_trips_the_footprint_check(n):
    with pytest.raises(AssertionError, match=r"tensor 'y'.*back guard, first changed byte %d past" % ((-n) % VEC)):
        _relu_case(n, "store_vector_past_end")


def test_store_one_element_before_the_start_trips_the_footprint_check():
    with pytest.raises(AssertionError, match=r"tensor 'y'.*front guard, first changed byte 1 before"):
        _relu_case(33, "store_before_start")


# ---- 3x3 conv: independence, and what the NaN pattern is for ----------------------------------------------------------------------------
H_, W_, C_, K_ = 5, 6, 8, 4


def _conv_case(np_dt, defect, zero_last_tap_row, patterns=GU.PATTERNS):
    rng = np.random.default_rng(11)
    if np_dt == np.int8:
        x = rng.integers(-128, 128, (H_, W_, C_)).astype(np.int8)
        w = rng.integers(-3, 4, (K_, 3, 3, C_)).astype(np.int8)
    else:
        x = rng.standard_normal((H_, W_, C_)).astype(np.float32)
        w = rng.integers(-3, 4, (K_, 3, 3, C_)).astype(np.float32)       # small integers: the f32 sums are exact in any order
        x = np.round(x * 8).astype(np.float32)
    if zero_last_tap_row:
        w[:, 2] = 0            # the weights that would multiply row r + 1 are zero: the only "mask" the defective kernel has
    want = conv3x3_ref(x, w, np_dt)

    def launch(T, ws):
        conv3x3(T["x"], w, T["y"], H_, W_, C_, K_, np_dt, defect)
    saved = GU.PATTERNS
    GU.PATTERNS = patterns
    try:
        got = GU.run_guarded({"x": x}, {"y": ((H_, W_, K_), np_dt, None)}, launch, device="cpu", what="conv3x3")
    finally:
        GU.PATTERNS = saved
    assert GU.same_bytes(got["y"], want), "value: the output differs from the reference"
    GU.assert_no_sentinel_run(got["y"], "conv3x3", run=16)


@pytest.mark.parametrize("np_dt", [np.int8, np.float32])
@pytest.mark.parametrize("zero_tap", [False, True])
def test_conv_correct_kernel_passes_all_three_checks(np_dt, zero_tap):
    _conv_case(np_dt, None, zero_tap)


@pytest.mark.parametrize("np_dt", [np.int8, np.float32])
def test_row_read_past_the_end_trips_the_independence_check(np_dt):
    """the over-read row meets ordinary weights: the last output row follows the guard pattern"""
    with pytest.raises(AssertionError, match="output 'y' depends on bytes outside the tensors"):
        _conv_case(np_dt, "row_past_end", False)


def test_row_read_past_the_end_under_a_zero_weight_is_exposed_on_f32_by_the_nan_pattern_only():
    """x * 0 with x from the 0xFF guard is NaN: the two patterns disagree and the value is wrong. With the finite pattern alone the same
    defect passes every check - which is why 0xFF is one of the two."""
    with pytest.raises(AssertionError, match="output 'y' depends on bytes outside the tensors"):
        _conv_case(np.float32, "row_past_end", True)
    with pytest.raises(AssertionError, match="value: the output differs"):
        _conv_case(np.float32, "row_past_end", True, patterns=(0xFF,))
    _conv_case(np.float32, "row_past_end", True, patterns=(0x5A,))          # invisible: finite * 0 == 0


def test_row_read_past_the_end_under_a_zero_weight_is_invisible_on_int8():
    """The limit of the method, stated: an integer over-read multiplied by a zero weight changes no byte under any pattern (and the load
    itself cannot be observed without faulting). The f32 forms of the same load pipeline are what exposes such a mask."""
    _conv_case(np.int8, "row_past_end", True)


# ---- workspace: independence -------------------------------------------------------------------------------------------------------------
def _ws_case(defect):
    P, C = 7, 6
    x = np.random.default_rng(5).integers(-128, 128, (P, C)).astype(np.int8)

    def launch(T, ws):
        channel_sum_via_workspace(T["x"], T["y"], ws, P, C, defect)
    got = GU.run_guarded({"x": x}, {"y": ((P,), np.int32, None)}, launch, device="cpu", ws_bytes=P * 8, what="channel sum")
    assert np.array_equal(got["y"], x.astype(np.int32).sum(1)), "value"


def test_workspace_correct_kernel_passes_all_three_checks():
    _ws_case(None)


def test_uninitialised_workspace_lane_trips_the_independence_check():
    with pytest.raises(AssertionError, match="output 'y' depends on bytes outside the tensors or on the workspace's old contents"):
        _ws_case("ws_lane")


def test_a_changed_read_only_tensor_and_a_stale_output_are_reported():
    x = np.arange(40, dtype=np.int8)

    def clobber(T, ws):
        relu_s8(T["x"], T["y"], 40)
        T["x"][3] = 9
    with pytest.raises(AssertionError, match="read-only tensor 'x' was changed"):
        GU.run_guarded({"x": x}, {"y": ((40,), np.int8, None)}, clobber, device="cpu")
    y = np.full(200, GU.SENTINEL, np.uint8)
    y[:100] = 1
    with pytest.raises(AssertionError, match="still hold the sentinel"):
        GU.assert_no_sentinel_run(y)


# ---- the out= argument of the streaming wrappers (anakin_amd/saber.py: _out) --------------------------------------------------------------
def test_out_argument_is_checked_before_any_launch():
    """a caller's out= of the wrong dtype, element count or layout is refused (no device needed: the check comes first); a right one
    comes back over the same memory in the result's shape"""
    from anakin_amd import lib as L
    from anakin_amd import saber as S
    good = torch.empty(24, dtype=torch.float32)
    y = S._out(good, (2, 3, 4), torch.float32)
    assert y.shape == (2, 3, 4) and y.data_ptr() == good.data_ptr()
    g = GU.guarded((2, 3, 4), np.int8, 0xFF, "cpu")
    assert S._out(g.t, (2, 3, 4), torch.int8).data_ptr() == g.t.data_ptr()
    for bad in (torch.empty(24, dtype=torch.int8), torch.empty(23, dtype=torch.float32), torch.empty((4, 12), dtype=torch.float32)[:, ::2]):
        with pytest.raises(L.SaberHipError, match="out= must be a contiguous"):
            S._out(bad, (2, 3, 4), torch.float32)
