"""numpy reference of the output formats beside 8-bit 4:2:0 (include/uav_hip.h `uav_clip_window_to_yuv`): 8-bit 4:4:4 and 10-bit
4:2:0 / 4:4:4, on int64, written from the formulas of the C ABI's documentation; the 8-bit pieces come from tests/yuv_ref.py.
Shared by the CPU and GPU tests of `--out-format`."""
import numpy as np

import yuv_ref

# name -> (chroma444, depth, Y4M tag)
FORMATS = {"444": (True, 8, "C444"), "420p10": (False, 10, "C420p10"), "444p10": (True, 10, "C444p10")}


def table10(matrix, full_range):
    """round(k * S / 4095 * 65536): S = 1023, yo = 0 for full range; S = 876 (luma) / 896 (chroma), yo = 64 for limited range."""
    kr, kb = yuv_ref.KR_KB[matrix]
    kg = 1 - kr - kb
    ys, yo, cs = (1023, 0, 1023) if full_range else (876, 64, 896)

    def r(x, s):
        return round(x * s / 4095 * 65536)
    return dict(yo=yo, fy=[r(kr, ys), r(kg, ys), r(kb, ys)],
                fcb=[r(-kr / (2 * (1 - kb)), cs), r(-kg / (2 * (1 - kb)), cs), r(0.5, cs)],
                fcr=[r(0.5, cs), r(-kg / (2 * (1 - kr)), cs), r(-kb / (2 * (1 - kr)), cs)])


def rgb_u8(frames):
    """(T,3,H,W) fp32 -> (T,H,W,3) uint8 as uav_clip_to_frames_u8 forms it: clamp(x/2 + 0.5, 0, 1) * 255 in fp32, truncated."""
    x = np.asarray(frames, dtype=np.float32)
    v = np.clip(x / np.float32(2) + np.float32(0.5), np.float32(0), np.float32(1)) * np.float32(255)
    return v.astype(np.int64).astype(np.uint8).transpose(0, 2, 3, 1)


def rgb_q12(frames):
    """(T,3,H,W) fp32 -> (T,H,W,3) int64 12-bit RGB: v = clamp(x/2 + 0.5, 0, 1) in fp32, (int)(v * 4095.0f + 0.5f)."""
    x = np.asarray(frames, dtype=np.float32)
    v = np.clip(x / np.float32(2) + np.float32(0.5), np.float32(0), np.float32(1))
    return (v * np.float32(4095) + np.float32(0.5)).astype(np.int64).transpose(0, 2, 3, 1)


def encode(frames, fmt, matrix, full_range, peak=None):
    """(T,3,H,W) fp32 frames -> planes (y, cb, cr) of format `fmt`: uint8 for '444', uint16 for the 10-bit formats; Cb, Cr
    (T,H,W) for 4:4:4, (T,H/2,W/2) for 4:2:0 (H and W even).  `peak`: a list that receives the largest absolute intermediate."""
    chroma444, depth, _ = FORMATS[fmt]
    if depth == 8:
        k, v, centre, vmax, dtype = yuv_ref.table(matrix, full_range), rgb_u8(frames).astype(np.int64), 128, 255, np.uint8
    else:
        k, v, centre, vmax, dtype = table10(matrix, full_range), rgb_q12(frames), 512, 1023, np.uint16
    t, h, w, _ = v.shape
    ysum = (v * np.array(k["fy"], dtype=np.int64)).sum(-1) + 32768
    y = np.clip((ysum >> 16) + k["yo"], 0, vmax)

    def chroma(f):
        s = (v * np.array(f, dtype=np.int64)).sum(-1)
        if chroma444:
            s = s + 32768
            return s, np.clip((s >> 16) + centre, 0, vmax)
        assert h % 2 == 0 and w % 2 == 0
        s = s.reshape(t, h // 2, 2, w // 2, 2).sum(axis=(2, 4)) + (1 << 17)
        return s, np.clip((s >> 18) + centre, 0, vmax)
    sb, cb = chroma(k["fcb"])
    sr, cr = chroma(k["fcr"])
    if peak is not None:
        peak.append(int(max(np.abs(ysum).max(), np.abs(sb).max(), np.abs(sr).max())))
    return y.astype(dtype), cb.astype(dtype), cr.astype(dtype)


def exact(frames, fmt, matrix, full_range):
    """The float64 conversion of the same fp32 values, unrounded and unclamped at the output: planes in steps of the format."""
    chroma444, depth, _ = FORMATS[fmt]
    kr, kb = yuv_ref.KR_KB[matrix]
    kg = 1 - kr - kb
    one = (1 << depth) - 1
    ys, yo, cs = (one, 0, one) if full_range else (219 << (depth - 8), 16 << (depth - 8), 224 << (depth - 8))
    v = np.clip(np.asarray(frames, dtype=np.float32).astype(np.float64) / 2 + 0.5, 0, 1)
    r, g, b = v[:, 0], v[:, 1], v[:, 2]
    luma = kr * r + kg * g + kb * b
    y = luma * ys + yo
    cb = (b - luma) / (2 * (1 - kb)) * cs + (one + 1) // 2
    cr = (r - luma) / (2 * (1 - kr)) * cs + (one + 1) // 2
    if not chroma444:
        t, h, w = y.shape
        cb, cr = (c.reshape(t, h // 2, 2, w // 2, 2).mean(axis=(2, 4)) for c in (cb, cr))
    return y, cb, cr


def file_bytes(planes, header):
    """The Y4M file of `planes`: `header`, then per frame 'FRAME\\n' and the three planes, 16-bit samples little-endian."""
    y, cb, cr = (np.ascontiguousarray(p).astype("<u2") if p.dtype.itemsize == 2 else np.ascontiguousarray(p) for p in planes)
    out = [header]
    for i in range(len(y)):
        out += [b"FRAME\n", y[i].tobytes(), cb[i].tobytes(), cr[i].tobytes()]
    return b"".join(out)
