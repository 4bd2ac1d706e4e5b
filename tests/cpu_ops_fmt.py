"""Torch stand-in on the CPU for `uav.ops.clip_window_to_yuv` (K13, the output formats beside 8-bit 4:2:0), installed beside
`cpu_ops` / `cpu_ops_io` so that the upscaling program runs `--out-format 444|420p10|444p10` end to end without a GPU.  Same
arithmetic as the kernel: fp32 for the clamp and the quantisation, int32 16.16 fixed point for the colour conversion."""
import torch

_SAVED = {}


def clip_window_to_yuv(window, y, cb, cr, coefs, *, chroma444, depth, frames_first=False):
    assert depth in (8, 10) and getattr(coefs, "depth", 8) == depth and (chroma444 or depth == 10)
    frames = (window if frames_first else window.permute(1, 0, 2, 3)).float()                  # (T,3,h,w)
    t, _, h, w = frames.shape
    v = (frames / 2.0 + 0.5).clamp(0.0, 1.0)
    q = (v * 255.0).to(torch.int32) if depth == 8 else (v * 4095.0 + 0.5).to(torch.int32)  # truncation
    f = coefs.forward
    centre, vmax = (128, 255) if depth == 8 else (512, 1023)
    y.copy_(((f[0] * q[:, 0] + f[1] * q[:, 1] + f[2] * q[:, 2] + 32768 >> 16) + f[9]).clamp(0, vmax))
    if chroma444:
        cshape, s, half, shift = (t, h, w), q, 32768, 16
    else:
        assert h % 2 == 0 and w % 2 == 0
        cshape, s, half, shift = (t, h // 2, w // 2), q.reshape(t, 3, h // 2, 2, w // 2, 2).sum(dim=(3, 5)), 1 << 17, 18
    assert tuple(cb.shape) == tuple(cr.shape) == cshape and tuple(y.shape) == (t, h, w)
    cb.copy_(((f[3] * s[:, 0] + f[4] * s[:, 1] + f[5] * s[:, 2] + half >> shift) + centre).clamp(0, vmax))
    cr.copy_(((f[6] * s[:, 0] + f[7] * s[:, 1] + f[8] * s[:, 2] + half >> shift) + centre).clamp(0, vmax))


def install():
    """Swap uav.ops.clip_window_to_yuv for the stand-in (beside cpu_ops.install() and cpu_ops_io.install()).  Not re-entrant."""
    from uav import ops
    assert not _SAVED, "cpu_ops_fmt.install() is already active"
    _SAVED["clip_window_to_yuv"] = ops.clip_window_to_yuv
    ops.clip_window_to_yuv = clip_window_to_yuv


def restore():
    from uav import ops
    if _SAVED:
        ops.clip_window_to_yuv = _SAVED.pop("clip_window_to_yuv")
