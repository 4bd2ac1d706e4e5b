"""Torch stand-ins on the CPU for `uav.ops.yuv420_sited_to_clip_f32` and `uav.ops.clip_to_yuv420_sited` (K13, siting-aware
4:2:0), installed beside `cpu_ops` / `cpu_ops_io` / `cpu_ops_fmt` so that the upscaling program runs `--chroma sited` end to end
without a GPU.  Same arithmetic as the kernels: fp32 for the clamp and the quantisation, int32 fixed point for the rest."""
import torch

_SAVED = {}


def _taps(n_luma, n_chroma, centre):
    x = torch.arange(n_luma)
    i, odd = x >> 1, (x & 1).bool()
    ia = torch.where(odd, i, (i - 1).clamp(min=0))
    ib = torch.where(odd, (i + 1).clamp(max=n_chroma - 1), i)
    one = torch.ones_like(x, dtype=torch.int32)
    if centre:
        return ia, ib, torch.where(odd, 3 * one, one), torch.where(odd, one, 3 * one)
    return ia, ib, torch.where(odd, 2 * one, 0 * one), torch.where(odd, 2 * one, 4 * one)


def _up16(c, h, w, siting):
    centre_h, centre_v = siting
    c = c.to(torch.int32)
    ja, jb, va, vb = _taps(h, c.shape[1], centre_v)
    ia, ib, ha, hb = _taps(w, c.shape[2], centre_h)
    rows = va[None, :, None] * c[:, ja] + vb[None, :, None] * c[:, jb]
    return ha * rows[:, :, ia] + hb * rows[:, :, ib]


def yuv420_sited_to_clip_f32(y, cb, cr, coefs, siting):
    yo, iy, rcr, gcb, gcr, bcb = coefs.inverse
    t, h, w = y.shape
    assert tuple(cb.shape) == tuple(cr.shape) == (t, (h + 1) // 2, (w + 1) // 2) and len(siting) == 2
    yy = (y.to(torch.int32) - yo) * iy * 16
    u, v = _up16(cb, h, w, siting) - 2048, _up16(cr, h, w, siting) - 2048
    half = 1 << 19
    rgb = torch.stack([(yy + rcr * v + half) >> 20, (yy + gcb * u + gcr * v + half) >> 20, (yy + bcb * u + half) >> 20])
    return (rgb.clamp(0, 255).float() / 255.0 - 0.5) * 2.0                                 # (3,T,H,W)


def clip_to_yuv420_sited(frames, coefs, depth=8):
    assert depth in (8, 10) and getattr(coefs, "depth", 8) == depth
    t, _, h, w = frames.shape
    assert h % 2 == 0 and w % 2 == 0
    v = (frames.float() / 2.0 + 0.5).clamp(0.0, 1.0)
    q = (v * 255.0).to(torch.int32) if depth == 8 else (v * 4095.0 + 0.5).to(torch.int32)  # truncation
    f = coefs.forward
    centre, vmax, dtype = (128, 255, torch.uint8) if depth == 8 else (512, 1023, torch.int16)
    y = (((f[0] * q[:, 0] + f[1] * q[:, 1] + f[2] * q[:, 2] + 32768) >> 16) + f[9]).clamp(0, vmax)
    even = torch.arange(0, w, 2)
    s = q[..., (even - 1).clamp(min=0)] + 2 * q[..., even] + q[..., even + 1]              # (T,3,H,W/2)
    s = s.reshape(t, 3, h // 2, 2, w // 2).sum(dim=3)
    cb = (((f[3] * s[:, 0] + f[4] * s[:, 1] + f[5] * s[:, 2] + (1 << 18)) >> 19) + centre).clamp(0, vmax)
    cr = (((f[6] * s[:, 0] + f[7] * s[:, 1] + f[8] * s[:, 2] + (1 << 18)) >> 19) + centre).clamp(0, vmax)
    return y.to(dtype), cb.to(dtype), cr.to(dtype)


_OPS = ("yuv420_sited_to_clip_f32", "clip_to_yuv420_sited")


def install():
    """Swap the two uav.ops entry points for the stand-ins (beside the other cpu_ops*.install()).  Not re-entrant."""
    from uav import ops
    assert not _SAVED, "cpu_ops_chroma.install() is already active"
    for name in _OPS:
        _SAVED[name] = getattr(ops, name)
        setattr(ops, name, globals()[name])


def restore():
    from uav import ops
    for name in _OPS:
        if name in _SAVED:
            setattr(ops, name, _SAVED.pop(name))
