"""numpy reference of the scene statistics (csrc/scene_stats.hip, `uav_clip_scene_stats`) on int64 and a float64 restatement of
the cut decision (`uav.video_io.scene_cuts`), written from include/uav_hip.h and the docstring; and the synthetic scenes the
tests of `--scenes auto` share.  The uint8 luma is tests/yuv_ref.py's."""
import numpy as np

import yuv_ref

BINS = 64


def luma(clip):
    """(3,T,h,w) fp32 in [-1,1] -> (T,h,w) int64: the uint8 RGB value of the kernels (fp32 clamp, truncation), then the BT.601
    full-range luma of `yuv_ref.encode` (a frame with an odd side is padded for it; luma is per pixel)."""
    x = np.asarray(clip, dtype=np.float32)
    v = np.clip(x / np.float32(2.0) + np.float32(0.5), np.float32(0.0), np.float32(1.0)) * np.float32(255.0)
    rgb = np.moveaxis(v.astype(np.uint8), 0, -1)                                # (T,h,w,3), truncated
    t, h, w, _ = rgb.shape
    padded = np.pad(rgb, ((0, 0), (0, h % 2), (0, w % 2), (0, 0)), mode="edge")
    return yuv_ref.encode(padded, "bt601", True)[0][:, :h, :w].astype(np.int64)


def stats(clip):
    """-> hist (T,64) int32, sad (T,) int64."""
    y = luma(clip)
    t = y.shape[0]
    hist = np.stack([np.bincount((f >> 2).reshape(-1), minlength=BINS) for f in y]).astype(np.int32)
    sad = np.zeros(t, dtype=np.int64)
    sad[1:] = np.abs(np.diff(y, axis=0)).sum(axis=(1, 2))
    return hist, sad


def measures(sad, hist, pixels):
    """mad (T,), hd (T,) in float64; index 0 is 0."""
    sad, hist = np.asarray(sad, dtype=np.int64), np.asarray(hist, dtype=np.int64)
    mad, hd = np.zeros(len(sad)), np.zeros(len(sad))
    mad[1:] = sad[1:] / float(pixels)
    hd[1:] = np.abs(hist[1:] - hist[:-1]).sum(axis=1) / (2.0 * pixels)
    return mad, hd


def cuts(sad, hist, pixels, threshold=(24.0, 0.30), min_len=8, max_len=0):
    """The whole form of the decision, frame by frame."""
    mad, hd = measures(sad, hist, pixels)
    total, start, out = len(mad), 0, []
    for t in range(1, total):
        candidate = mad[t] >= threshold[0] and hd[t] >= threshold[1] and t - start >= min_len
        forced = max_len > 0 and t == start + max_len
        if (candidate or forced) and total - t >= min_len:
            out.append(t)
            start = t
    return out


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
MEANS = [(70, 90, 60), (170, 150, 190), (40, 120, 200)]


def scene_u8(index, frames, h, w, seed=0):
    """Scene `index` of the fixture: (frames,h,w,3) uint8 RGB — a drifting sine pattern around the scene's mean colour plus
    integer noise in [-2, 2]."""
    rng = np.random.default_rng(1000 * seed + index)
    mean = MEANS[index % len(MEANS)]
    amp, period = 25 + 2.5 * (index % 3), 11 + 2.5 * (index % 3)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((frames, h, w, 3))
    for i in range(frames):
        for c in range(3):
            phase = 0.9 * c + 0.4 * index
            out[i, ..., c] = mean[c] + amp * np.sin(2 * np.pi * (x + i) / period + phase) * np.cos(2 * np.pi * y / (1.5 * period))
    out += rng.integers(-2, 3, out.shape)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def scenes_u8(lengths, h, w, seed=0):
    return np.concatenate([scene_u8(i, n, h, w, seed) for i, n in enumerate(lengths)])


def clip_of(rgb):
    """(T,h,w,3) uint8 -> (3,T,h,w) fp32 in [-1,1], the normalisation of `frames_to_clip_f32`."""
    return ((np.moveaxis(rgb, -1, 0).astype(np.float32) / np.float32(255.0) - np.float32(0.5)) * np.float32(2.0))


def assert_fixture(clip, lengths):
    """The margins every test that relies on the fixture asserts first, from this reference: pairs inside a scene stay below
    half the default thresholds (MAD < 12, distance < 0.15), pairs across a cut above twice them (MAD > 48, distance > 0.6)."""
    hist, sad = stats(clip)
    mad, hd = measures(sad, hist, clip.shape[-2] * clip.shape[-1])
    starts = set(np.cumsum(lengths)[:-1].tolist())
    for t in range(1, clip.shape[1]):
        if t in starts:
            assert mad[t] > 48 and hd[t] > 0.6, f"fixture: cut at {t} has MAD {mad[t]:.1f}, distance {hd[t]:.2f}"
        else:
            assert mad[t] < 12 and hd[t] < 0.15, f"fixture: frame {t} inside a scene has MAD {mad[t]:.1f}, distance {hd[t]:.2f}"
    return sorted(starts)
