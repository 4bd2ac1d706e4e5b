"""Torch stand-in on the CPU for `uav.ops.frame_axpby_f32` (csrc/frame_axpby.hip), installed beside the other `cpu_ops*` so that
`--scene-overlap` runs end to end without a GPU.  Same arithmetic as the kernel: each product rounded to fp32, then the sum."""
import torch

_SAVED = {}


def frame_axpby_f32(a, b, wa, wb, out=None):
    assert a.dtype == b.dtype == wa.dtype == wb.dtype == torch.float32 and a.shape == b.shape and a.is_contiguous() and b.is_contiguous()
    t = a.shape[0]
    assert tuple(wa.shape) == tuple(wb.shape) == (t,)
    shape = (t,) + (1,) * (a.dim() - 1)
    pa, pb = wa.reshape(shape) * a, wb.reshape(shape) * b                     # two tensors: nothing fuses the products into the sum
    if out is None:
        return pa + pb
    assert out.shape == a.shape and out.dtype == torch.float32 and out.is_contiguous()
    return torch.add(pa, pb, out=out)


_OPS = ("frame_axpby_f32",)


def install():
    """Swap the uav.ops entry point for the stand-in (beside the other cpu_ops*.install()).  Not re-entrant."""
    from uav import ops
    assert not _SAVED, "cpu_ops_seam.install() is already active"
    for name in _OPS:
        _SAVED[name] = getattr(ops, name)
        setattr(ops, name, globals()[name])


def restore():
    from uav import ops
    for name in _OPS:
        if name in _SAVED:
            setattr(ops, name, _SAVED.pop(name))
