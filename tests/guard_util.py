"""Tensors with guard bands, on device="cuda" and device="cpu" (tests/test_guard_cpu.py, tests/test_gpu_guard.py).

One uint8 allocation per tensor: [front guard G | LEAD 16 bytes | payload | back guard G]. The payload starts LEAD bytes past a 512-byte
boundary, so it is 16-byte aligned and no more (the alignment include/saber_hip.h asks of every tensor and workspace pointer), and the back
guard begins at the byte after the payload, with no rounding. Every guard byte holds one pattern; a launch must leave all of them alone
(footprint), its outputs must not depend on the pattern (independence), and they must be the reference's (value).

G is a condition, not a measurement: it has to exceed the farthest a mis-masked tile could reach at the shapes the tests use. The largest
pixel tile of the library is 256 rows (L.TILES goes to 128x128, the FP32 8-wave forms to 256x128; the chain / stage / halo /
image-resident kernels tile at most 256 pixels) and the largest pixel pitch the guard tests use is 2048 B (C = 2048 x 1 B in res5,
K = 512 x 4 B in pw_c128_k512): 512 KiB. A 3x3 halo adds (W + 1) pixels (< 64 at these shapes), a split-K plane or an NCHW plane of
these shapes is below 256 KiB. 1 MiB covers them twice."""
import numpy as np
import torch

G = 1 << 20                 # guard bytes on each side
LEAD = 16                   # payload address = 512-aligned base + G + LEAD: 16 (mod 256)
BASE_ALIGN = 512
SENTINEL = 77               # the suites' sentinel byte for outputs; differs from both patterns
PATTERNS = (0xFF, 0x5A)     # 0xFF: s8 -1, u8 255, f32 / s32 NaN / -1; 0x5A: finite and large as f32 (1.5e16)

_TORCH_OF_NP = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int8): torch.int8, np.dtype(np.float32): torch.float32,
                np.dtype(np.int32): torch.int32}


def torch_dtype(dt):
    return dt if isinstance(dt, torch.dtype) else _TORCH_OF_NP[np.dtype(dt)]


class Guarded:
    """.t: the payload as a tensor of the requested dtype and shape; .buf: the whole region [front | LEAD | payload | back] as uint8"""

    def __init__(self, shape, dtype, pattern, device, fill=SENTINEL):
        dtype = torch_dtype(dtype)
        shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        self.pattern, self.shape, self.dtype = int(pattern), shape, dtype
        self.nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        total = G + LEAD + self.nbytes + G
        self.raw = torch.empty(total + BASE_ALIGN, dtype=torch.uint8, device=device)      # the ONE allocation
        skip = (-self.raw.data_ptr()) % BASE_ALIGN
        self.buf = self.raw[skip:skip + total]
        self.buf.fill_(self.pattern)
        self.lo = G + LEAD                       # payload = buf[lo:hi]
        self.hi = self.lo + self.nbytes
        self.bytes = self.buf[self.lo:self.hi]
        if fill is not None:
            self.bytes.fill_(fill)
        self.t = self.bytes.view(dtype).view(shape)
        self.ptr = self.buf.data_ptr() + self.lo       # (an empty payload has no data_ptr of its own: its address is still this one)
        assert self.ptr % 256 == LEAD and (self.nbytes == 0 or self.t.data_ptr() == self.ptr)

    def set(self, a):
        """copy a numpy array / tensor of the payload's size in, bytes as they are"""
        src = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a.contiguous()
        src = src.reshape(-1).view(torch.uint8)
        assert src.numel() == self.nbytes, (src.numel(), self.nbytes)
        self.bytes.copy_(src)
        return self

    def numpy(self):
        """the payload on the host (synchronises)"""
        return self.t.cpu().numpy()

    def intact(self):
        """None when every guard byte still holds the pattern; otherwise (front, back): the offset of the first changed byte of each
        side relative to the payload (front: negative, -1 = the byte just before it; back: 0 = the byte just after it), None for a
        clean side. Compared where the buffer lives; only two flags, and on a failure two indices, cross to the host."""
        front, back = self.buf[:self.lo], self.buf[self.hi:]
        bad = torch.stack([(front != self.pattern).any(), (back != self.pattern).any()]).cpu().tolist()
        if not any(bad):
            return None
        f = int(torch.argmax((front != self.pattern).to(torch.uint8)).item()) - self.lo if bad[0] else None
        b = int(torch.argmax((back != self.pattern).to(torch.uint8)).item()) if bad[1] else None
        return (f, b)


def guarded(shape, dtype, pattern, device, fill=SENTINEL):
    return Guarded(shape, dtype, pattern, device, fill)


def from_numpy(a, pattern, device="cuda"):
    a = np.ascontiguousarray(a)
    return Guarded(a.shape, a.dtype, pattern, device, fill=None).set(a)


def dirty(nbytes, pattern, device="cuda"):
    """a workspace of exactly nbytes, guarded like a tensor and holding the pattern throughout: it may change, its guards may not"""
    return Guarded((int(nbytes),), torch.uint8, pattern, device, fill=pattern)


# ---- the three checks ------------------------------------------------------------------------------------------------------------------
def assert_footprint(tensors, what=""):
    """(a) every guard of every tensor (read-only ones and workspaces included) is intact; names tensor, side and byte offset"""
    for name, g in tensors.items():
        if g is None:
            continue
        r = g.intact()
        if r is None:
            continue
        f, b = r
        side = ("front guard, first changed byte %d before the tensor" % -f) if f is not None else \
            ("back guard, first changed byte %d past the tensor's end" % b)
        raise AssertionError("%s: tensor '%s' (%d bytes, pattern 0x%02X): write outside the tensor: %s" % (what, name, g.nbytes, g.pattern, side))


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def assert_independent(runs, what=""):
    """(b) runs: {label: {output name: ndarray}}; every output has the same bytes under every label (NaNs compared as bytes)"""
    labels = list(runs)
    for lb in labels[1:]:
        for name, a in runs[labels[0]].items():
            b = runs[lb][name]
            if not same_bytes(a, b):
                av, bv = np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8)
                i = int(np.argmax(av != bv)) if av.shape == bv.shape else -1
                raise AssertionError("%s: output '%s' depends on bytes outside the tensors or on the workspace's old contents: %s and %s "
                                     "differ in %d bytes, first at byte %d" % (what, name, labels[0], lb, int((av != bv).sum()) if i >= 0 else -1, i))


def assert_no_sentinel_run(a, what="", run=64):
    """where the op defines the whole output: no stretch of `run` consecutive sentinel bytes is left (a tile or row never stored; a single
    byte may be 77 by value)"""
    v = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    if v.size < run:
        return
    c = np.concatenate(([0], np.cumsum(v == SENTINEL)))
    full = np.nonzero(c[run:] - c[:-run] == run)[0]
    assert full.size == 0, "%s: %d consecutive output bytes from byte %d still hold the sentinel: never written" % (what, run, int(full[0]))


def label(pattern):
    return "plain" if pattern is None else "guard 0x%02X" % pattern


def run_guarded(inputs, outputs, launch, device="cuda", ws_bytes=0, plain=None, what=""):
    """One launch form under both patterns (and on ordinary tensors): asserts (a) and (b), returns the outputs of the ordinary run (of the
    first pattern when plain is None) as {name: ndarray} for the caller's value check (c).

    inputs   {name: ndarray | None}                          read-only tensors
    outputs  {name: (shape, dtype, prev ndarray | None)}     prev: the bytes an in-place mode finds there; None = the sentinel
    launch   launch(T, ws): T {name: tensor | None}, ws a uint8 tensor of ws_bytes or None; the same callable for every run, so an
             object that keeps state across launches sees them one after the other
    plain    plain(inputs, outputs, ws_bytes) -> (T, ws) on ordinary tensors; None = no ordinary run (the CPU models)"""
    runs = {}
    if plain is not None:
        T, ws = plain(inputs, outputs, ws_bytes)
        launch(T, ws)
        runs[label(None)] = {n: T[n].cpu().numpy() for n in outputs}
    for pat in PATTERNS:
        gt = {n: (None if a is None else from_numpy(a, pat, device)) for n, a in inputs.items()}
        for n, (shape, dt, prev) in outputs.items():
            gt[n] = Guarded(shape, dt, pat, device) if prev is None else Guarded(shape, dt, pat, device, fill=None).set(prev)
        ws = dirty(ws_bytes, pat, device) if ws_bytes else None
        launch({n: (None if g is None else g.t) for n, g in gt.items()}, None if ws is None else ws.t)
        runs[label(pat)] = {n: gt[n].numpy() for n in outputs}
        gt["workspace"] = ws
        assert_footprint(gt, "%s, %s" % (what, label(pat)))
        for n, a in inputs.items():
            assert a is None or same_bytes(gt[n].numpy(), a), "%s, %s: read-only tensor '%s' was changed" % (what, label(pat), n)
    assert_independent(runs, what)
    return runs[next(iter(runs))]
