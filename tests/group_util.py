"""Grouped 3x3 INT8 kernels (conv_group3x3.hip; kernel selection variant 17) and ResNeXt-50: what the CPU and the GPU tests share.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

from tests import int8_probe as P

VARIANT = 17
# (C, Cg, input H, stride) of the seven distinct grouped layers of ResNeXt-50 32x4d at 224 x 224
RESNEXT_GROUP_SHAPES = [(128, 4, 56, 1), (256, 8, 56, 2), (256, 8, 28, 1), (512, 16, 28, 2), (512, 16, 14, 1), (1024, 32, 14, 2),
                        (1024, 32, 7, 1)]
CGS = (4, 8, 16, 32, 64)


def group_forms(lib, h):
    """The form numbers v >= 1 that saber_hip_conv2d_set_tile accepts as (17 << 16) | v on the op `h` (restores the op's selection)."""
    keep = lib.saber_hip_conv2d_get_tile(h)
    forms, v = [], 1
    while v < 256 and lib.saber_hip_conv2d_set_tile(h, (VARIANT << 16) | v) == 0:
        forms.append(v)
        v += 1
    assert lib.saber_hip_conv2d_set_tile(h, keep) == 0
    return forms


def group_probe(name, geo, cg, idt, odt, relu):
    """tests/int8_probe.py:dw_probe generalised to Cg > 1: output channel k has ONE weight sigma, on the centre tap of input channel
    k % Cg of its own group, the row's other weights are zero; every channel of the pixel under the centre tap holds the accumulator t
    itself (t <= 127). Returns (probe, wq [K, Cg, 3, 3]): the probe carries the same weights dense ([K, C, 3, 3], zero outside the
    group) for its own integer model and class masks."""
    N, H, W, C, K, k, pad, stride = geo
    assert C == K and k == 3 and pad == 1 and C % cg == 0
    s_i, s_o = P._io_scales(idt, odt)
    order, extra = P.op_order_search(idt, odt, relu, t_max=127)
    chans = [(s, 0.5, bp / 2.0) for s, bp in P._pow2_channels(odt)] + order + order[:1]
    sig, ws, b = P._channel_params(K, chans)
    oh, ow = P.out_hw(geo)
    tvals = P.T_BASE + extra
    tv = np.asarray(tvals)[np.arange(N * oh * ow) % len(tvals)].reshape(N, oh, ow)
    x = np.zeros((N, H, W, C), np.int64)
    x[:, (np.arange(oh) * stride)[:, None], (np.arange(ow) * stride)[None, :], :] = tv[..., None]
    kk = np.arange(K)
    wq = np.zeros((K, cg, 3, 3), np.int8)
    wq[kk, kk % cg, 1, 1] = sig
    dense = np.zeros((K, C, 3, 3), np.int8)
    dense[kk, (kk // cg) * cg + kk % cg, 1, 1] = sig
    p = P.Probe(name, geo, idt, odt, relu, x.astype(P.NP_DT[idt]), dense, ws, b, s_i, s_o,
                meta={"t": tvals, "order_channels": order, "acc24": "out of reach: one tap"})
    return p, wq
