"""numpy float64 reference of the antialiased separable cubic resize (include/uav_hip.h `uav_resize_aa_f32`), written from the
formulas of the C ABI's documentation: per axis a dense weight matrix (n_out, n_in) whose rows are the normalised taps, positions
from integer arithmetic, horizontal pass first.  Shared by the CPU and GPU tests of `--out-size` and by tools/bench_out_size.py,
with the shapes the kernel is held to (`SHAPES`) and their inputs (`case`)."""
import functools
from fractions import Fraction

import numpy as np

A = -0.5

# (hi, wi, ho, wo), planes — and what each shape reaches in csrc/resize_aa.hip
SHAPES = [((64, 96, 36, 54), 3),            # 16/9 on both axes, 8 taps; 16-byte loads, 4-byte stores (wo % 4 != 0)
          ((64, 96, 27, 41), 2),            # odd sizes, 10 taps
          ((40, 56, 40, 21), 4),            # identity on one axis
          ((33, 47, 17, 19), 5),            # odd input: scalar loads, rows and row groups that end early
          ((48, 64, 48, 64), 6),            # identity: a copy
          ((32, 32, 50, 44), 3),            # enlarging: 4 taps; 16-byte vertical pass
          ((256, 256, 255, 257), 2),        # a ratio next to 1, shrinking and enlarging; two blocks per row
          ((16, 16, 1, 1), 4),              # one result sample of 16 x 16 taps
          ((64, 64, 5, 7), 2),              # 52 taps: the border samples lose most of them
          ((2, 4096, 2, 4095), 2),          # 16 blocks per row, large indices
          ((2, 4096, 3, 2160), 3),          # ... shrinking, and enlarging 2 rows to 3
          ((320, 448, 180, 252), 3),        # the program's own kind of frame: 16-byte accesses in both passes
          ((3, 6000, 2, 700), 2),           # 60 / 7: 35 taps, a block's source span is staged through LDS in three chunks
          # the streamed horizontal pass of real frame sizes (2048 blocks or more): 513 row groups x 3 column segments, a block
          # streams 4 row groups with the next one's loads in flight; the last block holds 1 group and the last group 2 rows
          ((2050, 900, 1100, 520), 6),
          ((2050, 900, 1100, 520), 3)]      # ... half the planes: 2 row groups per block, the last block 1


def cubic(x):
    x = abs(x)
    if x < 1:
        return ((A + 2) * x - (A + 3)) * x * x + 1
    if x < 2:
        return A * (((x - 5) * x + 8) * x - 4)
    return 0.0


def taps(n_in, n_out, i):
    """(lo, weights) of result sample `i`: s = n_in / n_out, c = s (i + 0.5), support = 2 s if s >= 1 else 2, taps j in
    [max(0, floor(c - support + 0.5)), min(n_in, floor(c + support + 0.5))), k_j = cubic((j + 0.5 - c) * (1/s if s >= 1 else 1)),
    normalised.  Positions are exact rationals; the quotient alone is rounded (to float64 here)."""
    s = Fraction(n_in, n_out)
    c = s * Fraction(2 * i + 1, 2)
    support = 2 * s if s >= 1 else Fraction(2)
    inv = 1 / s if s >= 1 else Fraction(1)
    half = Fraction(1, 2)
    lo = max(0, (c - support + half).__floor__())
    hi = min(n_in, (c + support + half).__floor__())
    k = np.array([cubic(float((j + half - c) * inv)) for j in range(lo, hi)], dtype=np.float64)
    return lo, k / k.sum()


@functools.lru_cache(maxsize=None)
def weight_matrix(n_in, n_out):
    """(n_out, n_in) float64: row i holds the weights of result sample i at its taps, zero elsewhere — and the tap counts.
    Cached: callers do not write into the result."""
    m = np.zeros((n_out, n_in), dtype=np.float64)
    counts = []
    for i in range(n_out):
        lo, w = taps(n_in, n_out, i)
        m[i, lo:lo + len(w)] = w
        counts.append(len(w))
    return m, counts


def resize(x, ho, wo):
    """(..., hi, wi) -> (..., ho, wo) float64: horizontal pass, then vertical."""
    x = np.asarray(x, dtype=np.float64)
    hi, wi = x.shape[-2:]
    mx, _ = weight_matrix(wi, wo)
    my, _ = weight_matrix(hi, ho)
    return np.matmul(my, np.matmul(x, mx.T))


@functools.lru_cache(maxsize=None)
def case(shape, planes):
    """Input (planes, hi, wi) fp32 torch tensor — noise of deviation 0.8 with the edge values of the front end's tests in front,
    clipped to +-1.5, its last plane constant — and the reference's result as float64 numpy, made once."""
    import torch
    hi, wi, ho, wo = shape
    g = torch.Generator().manual_seed(sum(shape) + planes)
    x = torch.randn((planes, hi, wi), generator=g) * 0.8
    x.view(-1)[:8] = torch.tensor([-1.0, 1.0, -1.5, 1.5, 0.0, 0.999999, -0.999999, 0.5])
    x = x.clamp(-1.5, 1.5)
    x[-1] = 0.7315
    return x, resize(x.numpy(), ho, wo)
