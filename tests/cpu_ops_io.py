"""Torch stand-ins on the CPU for the frame I/O entry points of uav.ops (K13): `frames_to_clip_f32`, `clip_to_frames_u8`
and the two Y'CbCr conversions, so that the upscaling program (uav/cli.py) runs end to end without a GPU next to
`cpu_ops.install()`.  Same arithmetic as the kernels: fp32 for the normalisation, int32 16.16 fixed point for the colour
conversion."""
import torch

_SAVED = {}


def frames_to_clip_f32(frames):
    return ((frames.float() / 255.0 - 0.5) * 2.0).permute(1, 0, 2, 3).contiguous()


def _to_u8(frames):
    return ((frames / 2.0 + 0.5).clamp(0.0, 1.0) * 255.0).to(torch.int32)                  # truncation, like numpy's astype


def clip_to_frames_u8(frames):
    return _to_u8(frames).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def yuv420_to_clip_f32(y, cb, cr, coefs, chroma444=False):
    yo, iy, rcr, gcb, gcr, bcb = coefs.inverse
    t, h, w = y.shape
    if not chroma444:
        cb = cb.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)[:, :h, :w]
        cr = cr.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)[:, :h, :w]
    yy, u, v = (y.to(torch.int32) - yo) * iy, cb.to(torch.int32) - 128, cr.to(torch.int32) - 128
    rgb = torch.stack([(yy + rcr * v + 32768) >> 16, (yy + gcb * u + gcr * v + 32768) >> 16, (yy + bcb * u + 32768) >> 16])
    return (rgb.clamp(0, 255).float() / 255.0 - 0.5) * 2.0                                 # (3,T,H,W)


def clip_to_yuv420_u8(frames, coefs):
    f = coefs.forward
    t, _, h, w = frames.shape
    assert h % 2 == 0 and w % 2 == 0
    rgb = _to_u8(frames)
    y = (((f[0] * rgb[:, 0] + f[1] * rgb[:, 1] + f[2] * rgb[:, 2] + 32768) >> 16) + f[9]).clamp(0, 255)
    s4 = rgb.reshape(t, 3, h // 2, 2, w // 2, 2).sum(dim=(3, 5))
    cb = (((f[3] * s4[:, 0] + f[4] * s4[:, 1] + f[5] * s4[:, 2] + (1 << 17)) >> 18) + 128).clamp(0, 255)
    cr = (((f[6] * s4[:, 0] + f[7] * s4[:, 1] + f[8] * s4[:, 2] + (1 << 17)) >> 18) + 128).clamp(0, 255)
    return y.to(torch.uint8), cb.to(torch.uint8), cr.to(torch.uint8)


_OPS = ("frames_to_clip_f32", "clip_to_frames_u8", "yuv420_to_clip_f32", "clip_to_yuv420_u8")


def install():
    """Swap the four uav.ops entry points for the stand-ins (beside cpu_ops.install()).  Not re-entrant."""
    from uav import ops
    assert not _SAVED, "cpu_ops_io.install() is already active"
    for name in _OPS:
        _SAVED[name] = getattr(ops, name)
        setattr(ops, name, globals()[name])


def restore():
    from uav import ops
    for name in _OPS:
        if name in _SAVED:
            setattr(ops, name, _SAVED.pop(name))
