"""Torch stand-in on the CPU for `uav.ops.resize_aa_f32` (csrc/resize_aa.hip, `--out-size` / `--out-scale`), installed beside
`cpu_ops` / `cpu_ops_io` / `cpu_ops_fmt` so that the upscaling program resizes its chunks end to end without a GPU: torch's own
antialiased bicubic, the filter the kernel is defined by (its positions are fp32 where the kernel's are exact)."""
import torch
import torch.nn.functional as F

_SAVED = {}


def resize_aa_f32(x, ho, wo):
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() >= 2
    lead, (h, w) = x.shape[:-2], x.shape[-2:]
    out = F.interpolate(x.reshape(1, -1, h, w), size=(int(ho), int(wo)), mode="bicubic", antialias=True, align_corners=False)
    return out.reshape(*lead, int(ho), int(wo)).contiguous()


def install():
    """Swap uav.ops.resize_aa_f32 for the stand-in (beside the other cpu_ops*.install()).  Not re-entrant."""
    from uav import ops
    assert not _SAVED, "cpu_ops_resize.install() is already active"
    _SAVED["resize_aa_f32"] = ops.resize_aa_f32
    ops.resize_aa_f32 = resize_aa_f32


def restore():
    from uav import ops
    if _SAVED:
        ops.resize_aa_f32 = _SAVED.pop("resize_aa_f32")
