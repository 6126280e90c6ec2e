"""The INT8 requantisation probes (tests/int8_probe.py) proven on the CPU, for every probe tests/test_gpu_int8_probe.py runs: the clean
float32 model of the epilogue and the oracle agree byte for byte (and the generator's float32 restatement of orc_conv_i8_prepare gives the
oracle's bias' and scale bit for bit); the compiled reference agrees on the outputs that do not saturate; every named defect - half-away
rounding, floor(d + 0.5), truncation, a contracted fma, a reassociated bias, wrap instead of saturate, a clamp at -127, ... - changes at
least one byte of every probe it applies to; and every class that applies (ties of both parities and signs, both rails, +-1e6, the
searched op-order accumulators) is present in two positions k % 4. This is the proof that the probes separate right from wrong."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import int8_probe as P

GROUPS = P.group_list()


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_clean_emulation_equals_the_oracle_and_classes_are_present(group):
    for name in GROUPS[group]:
        p = P.build(name)
        want, got = P.oracle_bytes(p), P.emulate(p)
        bad = np.argwhere(want != got)
        assert len(bad) == 0, (name, len(bad), bad[0], P.describe(p, bad[0]))
        if "keep" not in p.meta:
            P.assert_classes(p)
        assert int(p.acc.min()) >= -2 ** 31 and int(p.acc.max()) < 2 ** 31
    if group.startswith("stempool/"):      # pooled: the two passes of one output dtype together, and the probed bytes survive their window
        for a, b in zip(GROUPS[group][0::2], GROUPS[group][1::2]):
            P.assert_classes(P.build(a), P.build(b))
        for name in GROUPS[group]:
            p = P.build(name)
            y = P.oracle_bytes(p)
            keep = P.pooled_keep(p)
            assert np.array_equal(P.max_pool_3x3s2(y), O.pool_i8_nhwc(y, (3, 3), (2, 2), (0, 0), 0))
            assert np.array_equal(P.max_pool_3x3s2(y)[keep], y[:, 1::2, 1::2, :][keep]), name
            if p.idt == P.S8:
                assert np.array_equal(O.quant_nchw_to_nhwc(P.f32_image_of(p.x), 1.0, O.S8), p.x), name
    print(group, {n.split("/", 2)[2]: sum(v > 0 for v in P.class_counts(P.build(n)).values()) for n in GROUPS[group]})


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_every_defect_changes_a_byte_of_every_probe_it_applies_to(group):
    seen = set()
    for name in GROUPS[group]:
        p = P.build(name)
        for defect in P.DEFECTS:
            if p.applies(defect):
                seen.add(defect)
                if "keep" in p.meta:       # behind a max pooling: the changed byte must be one the pooling shows, in either pass of the pair
                    q = P.build(name[:-5] + ("bgmax" if name.endswith("bgmin") else "bgmin"))
                    n = int((p.designated(defect) & p.meta["keep"]).sum()) + int((q.designated(defect) & q.meta["keep"]).sum())
                else:
                    n = int(p.designated(defect).sum())
                assert n > 0, (name, defect, "defect not detected")
    assert seen, group
    print(group, sorted(seen))


def test_every_defect_applies_somewhere():
    seen = {d for names in GROUPS.values() for n in names for d in P.DEFECTS if P.build(n).applies(d)}
    assert seen == set(P.DEFECTS), set(P.DEFECTS) - seen


@pytest.mark.skipif(not O.ref_available(), reason="oracle/_ref is not built")
@pytest.mark.parametrize("group", sorted(g for g in GROUPS if g.startswith(("conv/", "acc24/"))))
def test_compiled_reference_agrees_where_it_does_not_saturate(group):
    """The reference's GEMM path casts without saturating (tests/test_oracle_vs_ref.py): compared where d is inside the output range."""
    n = 0
    for name in GROUPS[group]:
        p = P.build(name)
        pad, st = (p.geo[6],) * 2, (p.geo[7],) * 2
        got = O.ref_conv_i8(p.x, p.wq, p.w_scale, p.bias, p.in_scale, p.out_scale, p.odt, int(p.relu), pad, st)
        lo, hi = P.RANGE[p.odt]
        r = np.rint(np.maximum(p.d(), P.F(0)) if p.relu else p.d())
        ok = (r >= lo) & (r <= hi)
        want = P.oracle_bytes(p)
        bad = np.argwhere((got != want) & ok)
        assert len(bad) == 0, (name, len(bad), bad[0], int(got[tuple(bad[0])]), int(want[tuple(bad[0])]), P.describe(p, bad[0]))
        n += int(ok.sum())
    assert n > 0


def test_relu_round_and_saturate_commute_on_one_monotone_chain():
    """Why "relu after the round" and "saturate before the relu" are not defects of a plain convolution (int8_probe's docstring): on every
    d a probe holds, and for both roundings, the three orders give one byte."""
    for name in GROUPS["conv/pw_k64"]:
        p = P.build(name)
        d = p.d()
        lo, hi = P.RANGE[p.odt]
        for rnd in (P._rne, P._roundf):
            a = np.clip(rnd(np.maximum(d, P.F(0))), lo, hi)
            b = np.clip(np.maximum(rnd(d), 0), lo, hi)
            c = np.maximum(np.clip(rnd(d), lo, hi), 0)
            assert np.array_equal(a, b) and np.array_equal(a, c), name


def test_describe_names_the_class():
    p = P.build("conv/pw_k64/s8s8/relu0")
    idx = np.argwhere(p.classes()["s8_rail_127.5"])[0]
    assert "s8_rail_127.5" in P.describe(p, idx) and "d 127.5" in P.describe(p, idx)


# ---- the streaming ops' probes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(P.ELT_SETS))
def test_eltwise_grid_model_equals_the_oracle_and_its_defects_show(mode):
    c, s0, s1 = P.ELT_SETS[mode]
    a, b = P.eltwise_grid()
    detects = {"half": ("elt_rne",), "sum": ("wrap", "clamp_m127"), "order": ("elt_assoc", "elt_fma", "elt_premul"),
               "below_half": ("half_identity_05",), "uneq": ("coeff_swap", "coeff_conv_for_both"), "neg": P.COEFF_DEFECTS,
               "zero_res": ("coeff_swap", "coeff_conv_for_both")}[mode]
    assert (c[0] != c[1]) == (mode in P.COEFF_MODES)
    for relu in (False, True):
        want = O.eltwise_i8(a, b, s0, s1, c[0], c[1], relu)
        assert np.array_equal(P.eltwise_model(a, b, c, s0, s1, relu), want), (mode, relu)
        for defect in detects:
            if defect == "clamp_m127" and relu:
                continue
            assert (P.eltwise_model(a, b, c, s0, s1, relu, defect) != want).any(), (mode, relu, defect)


NEW_ELT_PROBES = [n for g in sorted(GROUPS) if g.startswith("elt/") for n in GROUPS[g] if n.rsplit("/", 1)[1] in P.COEFF_MODES]


def test_unequal_coefficient_probes_model_equals_the_oracle_and_every_coefficient_defect_shows():
    """The three modes with c0 != c1 on every fused geometry: products exact in float32 (t is a multiple of one half), the clean model is
    the oracle byte for byte, and a swapped pair, the conv's coefficient used for both and (mode neg) a dropped sign each change bytes
    of every probe - in two lane positions k % 4 (assert_classes)."""
    assert len(NEW_ELT_PROBES) == len(P.FUSED_GEOMETRIES) * 2 * 3 * len(P.COEFF_MODES)
    n_def = 0
    for name in NEW_ELT_PROBES:
        p = P.build(name)
        (c0, c1), s0, s1 = P.ELT_COEFFS[p.meta["elt_mode"]]
        assert c0 != c1 and p.elt[2] == (c0, c1) and (p.out_scale, p.elt[3]) == (s0, s1) == (0.5, 0.5)
        t2 = 2.0 * p.t().astype(np.float64)
        assert np.array_equal(t2, np.rint(t2)), name
        assert np.array_equal(P.emulate(p), P.oracle_bytes(p)), name
        P.assert_classes(p)
        for defect in P.COEFF_DEFECTS:
            assert p.applies(defect) == (defect != "coeff_sign_dropped" or p.meta["elt_mode"] == "neg")
            if p.applies(defect):
                assert (P.emulate(p, defect) != P.oracle_bytes(p)).any(), (name, defect)
                n_def += 1
    assert n_def == len(NEW_ELT_PROBES) // 3 * 7


@pytest.mark.parametrize("shape", P.STAGE_PROBE_SHAPES)
def test_stage_probe_shapes_build_and_hold_every_class(shape):
    """the probes of the stage launch's first block at its own shapes (two images, ragged tiles; C = 64 among them): they build, hold
    every class in two lane positions, the model is the oracle, and every coefficient defect shows where it applies"""
    probes = P.stage_block_probes(shape)
    assert len(probes) == 3 + 2 * len(P.ELT_MODES)
    for which, name, geo in probes:
        p = P.build(name, geo)
        assert p.acc.shape[:3] == (shape[1], shape[2], shape[3])
        P.assert_classes(p)
        assert np.array_equal(P.emulate(p), P.oracle_bytes(p)), (shape, name)
        for defect in P.COEFF_DEFECTS:
            assert not p.applies(defect) or p.designated(defect).any(), (shape, name, defect)
    c64 = [s for s in P.STAGE_PROBE_SHAPES if s[0] == 64]      # tiles of 2 rows x 16 columns
    assert all(-(-s[2] // 2) >= 3 and s[2] % 2 for s in c64), "at least three tile rows with a ragged last row"
    assert any(-(-s[3] // 16) == 2 and s[3] % 16 for s in c64) and any(s[1] == 2 for s in c64), "two column tiles with a ragged one; two images"


def test_the_four_earlier_coefficient_sets_are_unchanged():
    assert P.ELT_MODES[:4] == ("half", "sum", "order", "below_half")
    assert [P.ELT_COEFFS[m] for m in P.ELT_MODES[:4]] == [((1.0, 1.0), 0.5, 0.5), ((2.0, 2.0), 0.5, 0.5), ((float(P.F(1.0 / 0.06)),) * 2, 0.05, 0.043),
                                                          ((1.0, 1.0), float(P.HALF_LO), float(P.HALF_LO))]
    for m in P.ELT_MODES[:4]:
        assert not any(P.build("elt/pw_k64/s8/relu0_res0/" + m).applies(d) for d in P.COEFF_DEFECTS)


@pytest.mark.parametrize("odt", [P.S8, P.U8])
def test_quantiser_values_model_equals_the_oracle_and_its_defects_show(odt):
    x, scale = P.quant_values(odt)
    want = O.quant_nchw_to_nhwc(x, scale, odt)
    assert np.array_equal(P.quant_model(x, odt).transpose(0, 2, 3, 1), want)
    for defect in ("elt_rne", "half_identity_05", "wrap") + (("clamp_m127",) if odt == P.S8 else ("u8_no_lower_clamp",)):
        assert (P.quant_model(x, odt, defect).transpose(0, 2, 3, 1) != want).any(), defect
    if odt == P.S8:
        assert np.array_equal(O.quant_flat_s8(x.reshape(4, -1), 1.0), P.quant_model(x, odt).reshape(4, -1))


@pytest.mark.parametrize("dt", [P.S8, P.U8])
def test_pooling_image_model_equals_the_oracle_and_its_defects_show(dt):
    x = P.pool_image(dt)
    seen = {"half_away": 0, "pool_divide": 0}
    cases = [(x, w, s, p_, t, False) for w, s, p_, t in P.POOL_WINDOWS] + [(P.pool_image(dt, *hw), None, None, None, 1, True) for hw in ((8, 8), (4, 4), (7, 7), (2, 3))]
    for xi, win, st, pad, pt, glob in cases:
        want = O.pool_i8_nhwc(xi, win, st, pad, pt, global_pool=glob)
        assert np.array_equal(P.pool_model(xi, win, st, pad, pt, want.shape[1:3], global_pool=glob), want), (win, st, pad, pt, glob)
        for defect in seen:
            seen[defect] += int((P.pool_model(xi, win, st, pad, pt, want.shape[1:3], global_pool=glob, defect=defect) != want).sum())
    assert all(seen.values()), seen


@pytest.mark.parametrize("name", P.GPOOL_NAMES)
def test_global_pooling_probe_sums_are_exact_ties(name):
    p = P.build(name)
    y = P.oracle_bytes(p)
    assert np.array_equal(y, P.emulate(p))
    tot = y.astype(np.int64).sum(axis=(1, 2))
    tie = tot % 16 == 8
    assert tie.sum() >= 4 and len({int(k) % 4 for k in np.nonzero(tie[0])[0]}) >= 2
    assert {int(v) % 2 for v in (tot[tie] // 16)} == {0, 1}, "pooled ties of both parities"
    want = O.pool_i8_nhwc(y, None, None, None, 1, global_pool=True)
    assert np.array_equal(P.pool_model(y, None, None, None, 1, None, global_pool=True), want)
    assert (P.pool_model(y, None, None, None, 1, None, global_pool=True, defect="half_away") != want).any()


@pytest.mark.parametrize("M", [1, 8])
@pytest.mark.parametrize("idt", [P.S8, P.U8])
def test_fc_probe_model_equals_the_oracle_and_its_defect_shows(M, idt):
    x, wq, ws, b, s_in, s_out = P.fc_probe(M, 512, 24, idt)
    want = O.fc_i8(x, wq, ws, s_in, b, s_out) if idt == P.U8 else O.fc_i8(x, wq, ws, s_in, b)
    assert np.array_equal(P.fc_model(x, wq, ws, b, s_in, s_out), want)
    assert len(np.unique(x.astype(np.int64) @ wq.astype(np.int64).T)) == 2 * M
    bad = P.fc_model(x, wq, ws, b, s_in, s_out, "fma" if idt == P.S8 else "bias_float") != want
    assert bad.any(), "the contracted / reassociated epilogue gives the same bits on this probe"
