"""Oracle walks for models with grouped convolutions (MobileNet-v1): oracle/net_oracle.py:run_int8 / run_fp32 restated with the
layer's `group` handed to O.conv_i8 / O.conv_f32_nchw (net_oracle.py does not pass it; oracle/oracle.py takes it), and with the fc
reading a u8 operand as it is (MobileNet's tail is u8: every conv has relu). TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import net_oracle as NO
from oracle import oracle as O

F32, S8, U8 = O.F32, O.S8, O.U8

# (C, H, stride) of the nine distinct depthwise layers of MobileNet-v1 at 224 x 224
MOBILENET_DW_SHAPES = [(32, 112, 1), (64, 112, 2), (128, 56, 1), (128, 56, 2), (256, 28, 1), (256, 28, 2), (512, 14, 1), (512, 14, 2),
                       (1024, 7, 1)]


def run_int8(model, scales, x, prep=None):
    """x: f32 NCHW batch -> {edge name: numpy tensor} (8-bit edges NHWC), one oracle op per layer of model["spec"]."""
    scales = dict(scales)
    prep = prep if prep is not None else NO.prepare_int8(model)
    t, dt = {"data": x}, {"data": F32}
    for l in model["spec"]:
        kd, nm = l["kind"], l["name"]
        if kd == "conv":
            w, b = model["params"][nm]
            src = t[l["src"]]
            if dt[l["src"]] == F32:      # quantise on entry
                src, in_dt = O.quant_nchw_to_nhwc(src, scales[l["src"]], S8), S8
            else:
                in_dt = dt[l["src"]]
            odt = l.get("odt", U8 if l["relu"] else S8)
            ws, wq = prep[nm]
            bp, sc = O.conv_i8_prepare(ws, b, scales[l["src"]], scales[nm], in_dt, odt)
            t[nm] = O.conv_i8(src, wq, bp, sc, odt, l["relu"], (l["pad"],) * 2, (l["stride"],) * 2, group=l.get("group", 1))
            dt[nm] = odt
        elif kd == "pool":
            t[nm] = O.pool_i8_nhwc(t[l["src"]], (l["win"],) * 2, (l["stride"],) * 2, (l["pad"],) * 2, l["type"],
                                   floor_mode=l.get("floor", False))
            dt[nm], scales[nm] = dt[l["src"]], scales[l["src"]]
        elif kd == "eltwise":
            c = np.float32(1.0 / scales[nm])
            t[nm] = O.eltwise_i8(t[l["a"]], t[l["b"]], scales[l["a"]], scales[l["b"]], c, c, l["relu"])
            dt[nm] = S8
        elif kd == "gpool" and l.get("int8"):
            t[nm] = O.pool_i8_nhwc(t[l["src"]], None, None, None, 1, global_pool=True)
            dt[nm], scales[nm] = dt[l["src"]], scales[l["src"]]
        elif kd == "gpool":
            t[nm] = O.pool_f32_nchw(O.dequant_nhwc_to_nchw(t[l["src"]], scales[l["src"]]), None, None, None, 1, global_pool=True)
            dt[nm] = F32
        elif kd == "fc":
            w, b = model["params"][nm]
            ws, wq = prep[nm]
            xin = t[l["src"]].reshape(t[l["src"]].shape[0], -1)
            xq = xin if dt[l["src"]] in (S8, U8) else O.quant_flat_s8(xin, scales[l["src"]])
            t[nm] = O.fc_i8(xq, wq, ws, scales[l["src"]], b)
            dt[nm] = F32
        elif kd == "softmax":
            t[nm] = O.softmax_f32(t[l["src"]])
            dt[nm] = F32
    return t


def run_fp32(model, x):
    """FP32 forward, NCHW."""
    t = {"data": x}
    for l in model["spec"]:
        kd, nm = l["kind"], l["name"]
        if kd == "conv":
            w, b = model["params"][nm]
            t[nm] = O.conv_f32_nchw(t[l["src"]], w, b, l["relu"], (l["pad"],) * 2, (l["stride"],) * 2, group=l.get("group", 1))
        elif kd == "pool":
            t[nm] = O.pool_f32_nchw(t[l["src"]], (l["win"],) * 2, (l["stride"],) * 2, (l["pad"],) * 2, l["type"],
                                    floor_mode=l.get("floor", False))
        elif kd == "eltwise":
            t[nm] = O.eltwise_f32(t[l["a"]], t[l["b"]], 1.0, 1.0, l["relu"])
        elif kd == "gpool":
            t[nm] = O.pool_f32_nchw(t[l["src"]], None, None, None, 1, global_pool=True)
        elif kd == "fc":
            w, b = model["params"][nm]
            y = O.fc_f32(t[l["src"]].reshape(t[l["src"]].shape[0], -1), w, b)
            t[nm] = np.maximum(y, 0) if l.get("relu") else y
        elif kd == "softmax":
            t[nm] = O.softmax_f32(t[l["src"]])
    return t


def dw_forms(lib, h):
    """The depthwise form numbers v >= 1 that saber_hip_conv2d_set_tile accepts on the op `h` (restores the op's selection)."""
    keep = lib.saber_hip_conv2d_get_tile(h)
    forms, v = [], 1
    while v < 256 and lib.saber_hip_conv2d_set_tile(h, (16 << 16) | v) == 0:
        forms.append(v)
        v += 1
    assert lib.saber_hip_conv2d_set_tile(h, keep) == 0
    return forms
