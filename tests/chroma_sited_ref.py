"""numpy reference of the two siting-aware 4:2:0 conversions (include/uav_hip.h `uav_yuv420_sited_to_clip_f32` /
`uav_clip_to_yuv420_sited`), on int64, written from the formulas of the C ABI's documentation; tables and quantisation come from
tests/yuv_ref.py and tests/yuv_fmt_ref.py.  Shared by the CPU and GPU tests of `--chroma sited`."""
import numpy as np

import yuv_fmt_ref
import yuv_ref

# (centre_h, centre_v) per input tag
SITINGS = {"C420jpeg": (True, True), "C420mpeg2": (False, True), "C420paldv": (False, False)}
LEFT = (False, True)                                                           # the siting of the tags written: C420mpeg2, C420p10


def taps(n_luma, n_chroma, centre):
    """Per luma index x of one axis: the two chroma indices (clamped to the plane) and their weights in quarters."""
    x = np.arange(n_luma)
    i, odd = x >> 1, (x & 1).astype(bool)
    ia = np.where(odd, i, np.maximum(i - 1, 0))
    ib = np.where(odd, np.minimum(i + 1, n_chroma - 1), i)
    if centre:
        wa, wb = np.where(odd, 3, 1), np.where(odd, 1, 3)
    else:
        wa, wb = np.where(odd, 2, 0), np.where(odd, 2, 4)
    return ia, ib, wa.astype(np.int64), wb.astype(np.int64)


def upsample16(c, h, w, siting):
    """A chroma plane stack (T,ceil(h/2),ceil(w/2)) -> (T,h,w) int64 in SIXTEENTHS of a step (the two axes' quarters multiplied)."""
    centre_h, centre_v = siting
    c = c.astype(np.int64)
    ja, jb, va, vb = taps(h, c.shape[1], centre_v)
    ia, ib, ha, hb = taps(w, c.shape[2], centre_h)
    rows = va[None, :, None] * c[:, ja] + vb[None, :, None] * c[:, jb]          # (T,h,cw)
    return ha * rows[:, :, ia] + hb * rows[:, :, ib]


def decode(y, cb, cr, matrix, full_range, siting, peak=None):
    """Y (T,H,W), Cb, Cr (T,ceil(H/2),ceil(W/2)) uint8 -> (T,H,W,3) uint8 RGB, chroma up-sampled bilinearly at `siting`, one
    rounding.  `peak`: a list that receives the largest absolute intermediate value."""
    k = yuv_ref.table(matrix, full_range)
    t, h, w = y.shape
    assert cb.shape == cr.shape == (t, (h + 1) // 2, (w + 1) // 2)
    yy = 16 * (y.astype(np.int64) - k["yo"]) * k["iy"]
    u16, v16 = upsample16(cb, h, w, siting) - 2048, upsample16(cr, h, w, siting) - 2048
    half = 1 << 19
    sums = [yy + k["rcr"] * v16 + half, yy + k["gcb"] * u16 + k["gcr"] * v16 + half, yy + k["bcb"] * u16 + half]
    if peak is not None:
        peak.append(int(max(np.abs(s).max() for s in sums)))
    return np.stack([np.clip(s >> 20, 0, 255) for s in sums], axis=-1).astype(np.uint8)


def decode_exact(y, cb, cr, matrix, full_range, siting):
    """The float64 conversion of the same up-sampled chroma, unrounded and unclamped: (T,H,W,3) in 8-bit steps."""
    kr, kb = yuv_ref.KR_KB[matrix]
    kg = 1 - kr - kb
    ys, yo, cs = (255, 0, 255) if full_range else (219, 16, 224)
    t, h, w = y.shape
    yy = (y.astype(np.float64) - yo) * 255 / ys
    u = (upsample16(cb, h, w, siting) / 16.0 - 128) * 255 / cs
    v = (upsample16(cr, h, w, siting) / 16.0 - 128) * 255 / cs
    r = yy + 2 * (1 - kr) * v
    b = yy + 2 * (1 - kb) * u
    g = yy - 2 * kb * (1 - kb) / kg * u - 2 * kr * (1 - kr) / kg * v
    return np.stack([r, g, b], axis=-1)


def clip_of(rgb):
    """(T,H,W,3) uint8 -> the clip (3,T,H,W) fp32 `(v/255. - 0.5) * 2`, in fp32 like the kernel."""
    v = rgb.astype(np.float32).transpose(3, 0, 1, 2)
    return (v / np.float32(255.0) - np.float32(0.5)) * np.float32(2.0)


def encode_q(q, depth, matrix, full_range, peak=None):
    """(T,H,W,3) integer RGB `q` of `depth` (8: the uint8 value, 10: the 12-bit value), H and W even -> planes Y (T,H,W), Cb, Cr
    (T,H/2,W/2), uint8 / uint16: today's luma, chroma (1,2,1) around the even column over both rows of a block, one rounding."""
    assert depth in (8, 10)
    k, centre, vmax, dtype = ((yuv_ref.table(matrix, full_range), 128, 255, np.uint8) if depth == 8 else
                              (yuv_fmt_ref.table10(matrix, full_range), 512, 1023, np.uint16))
    v = np.asarray(q).astype(np.int64)
    t, h, w, _ = v.shape
    assert h % 2 == 0 and w % 2 == 0
    ysum = (v * np.array(k["fy"], dtype=np.int64)).sum(-1) + 32768
    y = np.clip((ysum >> 16) + k["yo"], 0, vmax)
    even = np.arange(0, w, 2)
    s = v[:, :, np.maximum(even - 1, 0)] + 2 * v[:, :, even] + v[:, :, even + 1]          # (T,H,W/2,3); even + 1 <= w - 1
    s = s.reshape(t, h // 2, 2, w // 2, 3).sum(axis=2)

    def chroma(f):
        acc = (s * np.array(f, dtype=np.int64)).sum(-1) + (1 << 18)
        return acc, np.clip((acc >> 19) + centre, 0, vmax)
    sb, cb = chroma(k["fcb"])
    sr, cr = chroma(k["fcr"])
    if peak is not None:
        peak.append(int(max(np.abs(ysum).max(), np.abs(sb).max(), np.abs(sr).max())))
    return y.astype(dtype), cb.astype(dtype), cr.astype(dtype)


def encode(frames, depth, matrix, full_range, peak=None):
    """(T,3,H,W) fp32 frames -> the planes of `encode_q` on the RGB value the existing kernels form for that depth."""
    q = yuv_fmt_ref.rgb_u8(frames) if depth == 8 else yuv_fmt_ref.rgb_q12(frames)
    return encode_q(q, depth, matrix, full_range, peak)
