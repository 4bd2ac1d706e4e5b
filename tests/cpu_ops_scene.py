"""Torch stand-in on the CPU for `uav.ops.clip_scene_stats` (csrc/scene_stats.hip), installed beside the other `cpu_ops*` so that
`--scenes auto` runs end to end without a GPU.  Same arithmetic as the kernel: fp32 for the clamp and the quantisation, integers
for the luma, the histogram and the sum of absolute differences."""
import torch

_SAVED = {}


def clip_scene_stats(clip, coefs):
    assert clip.dim() == 4 and clip.shape[0] == 3 and clip.dtype == torch.float32 and getattr(coefs, "depth", 8) == 8
    f = coefs.forward
    q = ((clip / 2.0 + 0.5).clamp(0.0, 1.0) * 255.0).to(torch.int32)                       # truncation
    y = (((f[0] * q[0] + f[1] * q[1] + f[2] * q[2] + 32768) >> 16) + f[9]).clamp(0, 255)   # (T,h,w)
    t = y.shape[0]
    bins = (y >> 2).reshape(t, -1).to(torch.int64)
    hist = torch.zeros(t, 64, dtype=torch.int64).scatter_add_(1, bins, torch.ones_like(bins)).to(torch.int32)
    sad = torch.zeros(t, dtype=torch.int64)
    sad[1:] = (y[1:] - y[:-1]).abs().sum(dim=(1, 2), dtype=torch.int64)
    return hist, sad


_OPS = ("clip_scene_stats",)


def install():
    """Swap the uav.ops entry point for the stand-in (beside the other cpu_ops*.install()).  Not re-entrant."""
    from uav import ops
    assert not _SAVED, "cpu_ops_scene.install() is already active"
    for name in _OPS:
        _SAVED[name] = getattr(ops, name)
        setattr(ops, name, globals()[name])


def restore():
    from uav import ops
    for name in _OPS:
        if name in _SAVED:
            setattr(ops, name, _SAVED.pop(name))
