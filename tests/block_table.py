"""Runs of stage blocks [conv3x3 C -> C, conv1x1 C -> 4C + eltwise, conv1x1 4C -> C] built from a PER-BLOCK TABLE, so that no two blocks of a
run share a record: per block the dtype it hands to the next block's 3x3 conv, the relu of the first 1x1 conv (before the sum), the relu on
the sum, and the coefficient pair (as multiples of c = 1 / s_sum), with scales that differ from block to block as well. A launch that applies
block 0's record to a later block, swaps the two coefficients, uses the convolution's for both or drops a sign gives other bytes - which
`conditions` asserts from the oracle alone, before anything runs on a device.

The oracle walk and the device operators (`device_ops`) read the same table. Plain numpy + the CPU oracle here: tests/test_block_table_cpu.py
checks every case's preconditions without a GPU, tests/test_gpu_stage_blocks.py runs the launches. TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import oracle as O

S8, U8, F32 = O.S8, O.U8, O.F32

# hand-over dtype, relu1, res_relu, (m0, m1): coefficient pair = (m0 * c, m1 * c)
TABLE = [(U8, 0, 1, (1.0, 1.0)), (S8, 1, 0, (1.0, -0.5)), (U8, 0, 1, (0.5, 1.0))]
UNEQUAL = [(1.0, -0.5), (0.5, 1.0)]          # (c, -c / 2) and (c / 2, c): the pairs of the single-form random cases


def rand8(rng, shape, dt):
    return rng.integers(0, 256, shape).astype(np.uint8) if dt == U8 else rng.integers(-128, 128, shape).astype(np.int8)


def _maxabs_scale(f, div):
    return max(float(np.abs(f).max()), 1e-6) / 127.0 / div


def rails(y, dt, relu):
    """(bytes on each rail the dtype and relu leave the edge, bytes strictly between the rails)"""
    hi, lo = (255, 0) if dt == U8 else (127, -128)
    on = [int(np.count_nonzero(y == hi))] + ([] if (relu or dt == U8) else [int(np.count_nonzero(y == lo))])
    return on, int(np.count_nonzero((y > lo) & (y < hi)))


def coeff_conditions(t1, r, s0, s1, c0, c1, relu, what, want=None):
    """From the oracle alone: the eltwise output under the swapped pair and under the convolution's coefficient for both each differ from
    the right output in at least a quarter of the bytes, and at least a tenth of the right output lies strictly between the rails."""
    want = O.eltwise_i8(t1, r, s0, s1, c0, c1, relu) if want is None else want
    swap = float((O.eltwise_i8(t1, r, s0, s1, c1, c0, relu) != want).mean())
    both = float((O.eltwise_i8(t1, r, s0, s1, c0, c0, relu) != want).mean())
    inside = float(((want > -128) & (want < 127)).mean())
    assert c0 != c1, what
    assert swap >= 0.25 and both >= 0.25 and inside >= 0.1, "%s: swapped pair changes %.3f, conv's for both %.3f, between the rails %.3f" % (what, swap, both, inside)
    return swap, both, inside


class Block:
    pass


class Run:
    """nblk blocks at C = c over the first inputs x (dtype first_dt) and res (s8), block k reading block k - 1's two outputs.
    sat: every scale a quarter of its edge's MAXABS scale, so the 3x3's output, the first 1x1's, the sum and the last conv's all saturate.
    .blocks[k]: weights, scales, flags, coefficients;  .wants[k] = (y1, y2) of the oracle;  .edges[k]: every edge of the block"""

    def __init__(self, rng, x, res, first_dt, c, table, sat=False):
        self.x, self.res, self.c, self.first_dt, self.sat = x, res, c, first_dt, sat
        self.N, self.H, self.W = x.shape[:3]
        k1 = 4 * c
        self.blocks, self.wants, self.edges = [], [], []
        cur_x, cur_res, idt = x, res, first_dt
        div = 4.0
        for k, (hand, relu1, res_relu, (m0, m1)) in enumerate(table):
            b = Block()
            b.hand, b.relu1, b.res_relu, b.idt, b.relu2 = hand, int(relu1), int(res_relu), idt, int(hand == U8)
            b.w0 = (rng.standard_normal((c, c, 3, 3)) * np.sqrt(2.0 / (9 * c))).astype(np.float32)
            b.b0 = (rng.standard_normal(c) * 0.5).astype(np.float32)
            b.w1 = (rng.standard_normal((k1, c, 1, 1)) * np.sqrt(2.0 / c)).astype(np.float32)
            b.b1 = (rng.standard_normal(k1) * 0.5).astype(np.float32)
            b.w2 = (rng.standard_normal((c, k1, 1, 1)) * np.sqrt(2.0 / k1)).astype(np.float32)
            b.b2 = (rng.standard_normal(c) * 0.5).astype(np.float32)
            b.s_x, b.s_in, b.s_mid, b.s_res = 0.023 + 0.001 * k, 0.02 + 0.003 * k, 0.05 - 0.004 * k, 0.043 + 0.002 * k
            b.s_sum, b.s_out = 0.06 + 0.005 * k, 0.031 + 0.002 * k
            ws0, ws1, ws2 = O.weight_scales(b.w0), O.weight_scales(b.w1), O.weight_scales(b.w2)
            q0, q1, q2 = O.quant_weights(b.w0, ws0), O.quant_weights(b.w1, ws1), O.quant_weights(b.w2, ws2)
            if sat:
                bp, sc = O.conv_i8_prepare(ws0, b.b0, b.s_x, 1.0, idt, F32)
                b.s_in = _maxabs_scale(O.conv_i8(cur_x, q0, bp, sc, F32, 1, (1, 1)), div)
            bp, sc = O.conv_i8_prepare(ws0, b.b0, b.s_x, b.s_in, idt, U8)
            t0 = O.conv_i8(cur_x, q0, bp, sc, U8, 1, (1, 1))
            if sat:
                bp, sc = O.conv_i8_prepare(ws1, b.b1, b.s_in, 1.0, U8, F32)
                b.s_mid = _maxabs_scale(O.conv_i8(t0, q1, bp, sc, F32, b.relu1), div)
            bp, sc = O.conv_i8_prepare(ws1, b.b1, b.s_in, b.s_mid, U8, S8)
            t1 = O.conv_i8(t0, q1, bp, sc, S8, b.relu1)
            if sat:
                f = m0 * t1.astype(np.float64) * b.s_mid + m1 * cur_res.astype(np.float64) * b.s_res
                b.s_sum = _maxabs_scale(np.maximum(f, 0) if res_relu else f, div)
            cf = 1.0 / b.s_sum
            b.coeff = (float(np.float32(m0 * cf)), float(np.float32(m1 * cf)))
            y1 = O.eltwise_i8(t1, cur_res, b.s_mid, b.s_res, b.coeff[0], b.coeff[1], bool(res_relu))
            if sat:
                bp, sc = O.conv_i8_prepare(ws2, b.b2, b.s_sum, 1.0, S8, F32)
                b.s_out = _maxabs_scale(O.conv_i8(y1, q2, bp, sc, F32, b.relu2), div)
            bp, sc = O.conv_i8_prepare(ws2, b.b2, b.s_sum, b.s_out, S8, hand)
            y2 = O.conv_i8(y1, q2, bp, sc, hand, b.relu2)
            self.blocks.append(b)
            self.wants.append((y1, y2))
            self.edges.append({"t0": (t0, U8, 1), "t1": (t1, S8, b.relu1), "y1": (y1, S8, b.res_relu), "y2": (y2, hand, b.relu2), "res": cur_res})
            cur_x, cur_res, idt = y2, y1, hand
        self.last_dt = idt

    def conditions(self, what):
        """asserted before any launch: no two blocks share their (hand-over dtype, relu1, res_relu, coefficient pair) record; with the
        ordinary scales the coefficient conditions on every block whose pair is unequal; with the saturating scales (which are fixed by
        the edges' MAXABS, and under which the rails and the relu hide most of what a wrong pair changes) bytes on each rail that the
        edge's dtype and relu leave it and unsaturated bytes, on all four edges of every block"""
        recs = [(b.hand, b.relu1, b.res_relu, b.coeff) for b in self.blocks]
        assert len({b.coeff for b in self.blocks}) == len(recs) and all(recs[k][:3] != recs[k - 1][:3] for k in range(1, len(recs))), (what, recs)
        assert any(b.relu1 for b in self.blocks) and any(b.coeff[1] < 0 for b in self.blocks), (what, recs)
        out = []
        for k, (b, e) in enumerate(zip(self.blocks, self.edges)):
            if b.coeff[0] != b.coeff[1] and not self.sat:
                out.append(coeff_conditions(e["t1"][0], e["res"], b.s_mid, b.s_res, b.coeff[0], b.coeff[1], bool(b.res_relu), "%s block %d" % (what, k),
                                            e["y1"][0]))
            if self.sat:
                for name in ("t0", "t1", "y1", "y2"):
                    y, dt, relu = e[name]
                    on, inside = rails(y, dt, relu)
                    assert all(v > 0 for v in on) and inside > 0, "%s block %d edge %s: on the rails %s, between them %d" % (what, k, name, on, inside)
        return out


def device_ops(run):
    """[(conv3x3, conv1x1 + eltwise, conv1x1)] library operators of a Run (needs the device library)"""
    from anakin_amd import lib as L
    from anakin_amd import saber as S
    N, H, W, c = run.N, run.H, run.W, run.c
    ops = []
    for b in run.blocks:
        c0 = S.SaberConv2D(int8=True).init((N, c, H, W), S.ConvParam(b.w0, b.b0, 1, (1, 1), (1, 1), (1, 1), True), b.idt, U8, b.s_x, b.s_in)
        pa = S.ConvParam(b.w1, b.b1, 1, (0, 0), (1, 1), (1, 1), bool(b.relu1))
        pa.res_mode, pa.res_relu, pa.sum_scale, pa.coeff, pa.scale_res = L.RES_ELTWISE, bool(b.res_relu), 1.0, b.coeff, b.s_res
        ca = S.SaberConv2D(int8=True).init((N, c, H, W), pa, U8, S8, b.s_in, b.s_mid)
        cb = S.SaberConv2D(int8=True).init((N, 4 * c, H, W), S.ConvParam(b.w2, b.b2, 1, (0, 0), (1, 1), (1, 1), bool(b.relu2)), S8, b.hand, b.s_sum, b.s_out)
        ops.append((c0, ca, cb))
    return ops


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
# name -> (C, N, H, W, blocks, saturating scales): the smallest shape of each stage kernel
CASES = {"c64": (64, 2, 7, 9, 3, False), "c128": (128, 1, 5, 13, 3, False), "c256": (256, 2, 7, 9, 3, False),
         "c64_sat": (64, 2, 7, 9, 3, True), "c128_sat": (128, 1, 5, 13, 3, True), "c256_sat": (256, 2, 7, 9, 3, True)}
_SEED = {"c64": 6401, "c128": 12801, "c256": 25601, "c64_sat": 6402, "c128_sat": 12802, "c256_sat": 25602}
_cache = {}


def case(name):
    """the Run of a name in CASES over random first inputs; cached, never modified"""
    if name not in _cache:
        c, N, H, W, nblk, sat = CASES[name]
        rng = np.random.default_rng(_SEED[name])
        x, res = rand8(rng, (N, H, W, c), U8), rand8(rng, (N, H, W, 4 * c), S8)
        _cache[name] = Run(rng, x, res, U8, c, TABLE[:nblk], sat)
    return _cache[name]
