"""numpy reference of the two Y'CbCr conversions (csrc/yuv_io.hip K13, include/uav_hip.h), on int64, written from the
formulas of the C ABI's documentation: shared by the CPU and GPU tests of the Y4M front end."""
import numpy as np

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
PAIRS = [(m, f) for m in ("bt601", "bt709") for f in (True, False)]


def table(matrix, full_range):
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    ys, yo, cs = (255, 0, 255) if full_range else (219, 16, 224)

    def r(x):
        return round(x * 65536)
    return dict(yo=yo,
                fy=[r(kr * ys / 255), r(kg * ys / 255), r(kb * ys / 255)],
                fcb=[r(-kr / (2 * (1 - kb)) * cs / 255), r(-kg / (2 * (1 - kb)) * cs / 255), r(0.5 * cs / 255)],
                fcr=[r(0.5 * cs / 255), r(-kg / (2 * (1 - kr)) * cs / 255), r(-kb / (2 * (1 - kr)) * cs / 255)],
                iy=r(255 / ys), rcr=r(2 * (1 - kr) * 255 / cs), bcb=r(2 * (1 - kb) * 255 / cs),
                gcb=r(-2 * kb * (1 - kb) / kg * 255 / cs), gcr=r(-2 * kr * (1 - kr) / kg * 255 / cs))


def encode(rgb, matrix, full_range, peak=None):
    """(T,H,W,3) uint8 RGB, H and W even -> Y (T,H,W), Cb, Cr (T,H/2,W/2) uint8.  `peak`: a list that receives the largest
    absolute intermediate value."""
    k = table(matrix, full_range)
    t, h, w, _ = rgb.shape
    assert h % 2 == 0 and w % 2 == 0
    v = rgb.astype(np.int64)
    ysum = (v * np.array(k["fy"], dtype=np.int64)).sum(-1) + 32768
    y = np.clip((ysum >> 16) + k["yo"], 0, 255)

    def chroma(f):
        s = (v * np.array(f, dtype=np.int64)).sum(-1).reshape(t, h // 2, 2, w // 2, 2).sum(axis=(2, 4)) + (1 << 17)
        return s, np.clip((s >> 18) + 128, 0, 255)
    sb, cb = chroma(k["fcb"])
    sr, cr = chroma(k["fcr"])
    if peak is not None:
        peak.append(int(max(np.abs(ysum).max(), np.abs(sb).max(), np.abs(sr).max())))
    return y.astype(np.uint8), cb.astype(np.uint8), cr.astype(np.uint8)


def decode(y, cb, cr, matrix, full_range, chroma444=False, peak=None):
    """Y (T,H,W), Cb, Cr (T,ceil(H/2),ceil(W/2)) [chroma444: (T,H,W)] uint8 -> (T,H,W,3) uint8 RGB; chroma replicated over 2x2."""
    k = table(matrix, full_range)
    t, h, w = y.shape
    if not chroma444:
        cb = cb.repeat(2, axis=1).repeat(2, axis=2)[:, :h, :w]
        cr = cr.repeat(2, axis=1).repeat(2, axis=2)[:, :h, :w]
    yy = (y.astype(np.int64) - k["yo"]) * k["iy"]
    u, v = cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    sums = [yy + k["rcr"] * v + 32768, yy + k["gcb"] * u + k["gcr"] * v + 32768, yy + k["bcb"] * u + 32768]
    if peak is not None:
        peak.append(int(max(np.abs(s).max() for s in sums)))
    return np.stack([np.clip(s >> 16, 0, 255) for s in sums], axis=-1).astype(np.uint8)
