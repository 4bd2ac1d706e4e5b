"""The access-mode pickers of the Y'CbCr kernels (csrc/yuv_mode.h: `yuv_encode_mode`, `yuv_decode_mode`) against the four
spellings they replaced, restated here from the source of the commit before them: `yuv_mode`, the downgrade ladder of
`uav_clip_window_to_yuv420_u8`, and the `planes_ok` lambdas of `uav_clip_window_to_yuv` and `uav_clip_to_yuv420_sited`.  A wrong
pick still writes the right bytes, only slower (or, too high, with misaligned vector accesses), so the byte-exact GPU tests cannot see
it.  The header is plain C++: tests/yuv_mode_main.cpp is compiled with the system compiler and fed the grid on stdin."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
BASE = 1 << 20                                                                # a 64-aligned address
OFFSETS = (0, 1, 2, 4, 8, 16)
KIND, W, SRC, Y, CB, CR, SC, ST, SR, YP, YF, CP, CF, SB, C444 = range(15)


# ---- the parent's pickers, on numpy arrays ---------------------------------------------------------------------------------
def _aligned(p, a):
    return (p & (a - 1)) == 0


def _pick(ok2, ok1):
    return np.where(ok2, 2, np.where(ok1, 1, 0))


def parent_yuv_mode(w, f32, y, cb, cr, c444):
    c = np.where(c444, 4, 2)
    return np.where(~_aligned(f32, 16), 0, _pick((w % 8 == 0) & _aligned(y, 8) & _aligned(cb, 4) & _aligned(cr, 4),
                                                 (w % 4 == 0) & _aligned(y, 4) & _aligned(cb, c) & _aligned(cr, c)))


def parent_window420_u8(g):
    """uav_clip_window_to_yuv420_u8: yuv_mode() when the source strides keep the alignment, then the downgrade ladder."""
    mode = np.where((g[SC] | g[ST] | g[SR]) % 4 == 0, parent_yuv_mode(g[W], g[SRC], g[Y], g[CB], g[CR], False), 0)
    mode = np.where((mode == 2) & (((g[YP] | g[YF]) % 8 != 0) | ((g[CP] | g[CF]) % 4 != 0)), 1, mode)
    return np.where((mode == 1) & (((g[YP] | g[YF]) % 4 != 0) | ((g[CP] | g[CF]) % 2 != 0)), 0, mode)


def parent_window(g):
    """uav_clip_window_to_yuv for the other three formats: its `planes_ok` lambda."""
    def planes_ok(a):
        c = np.where(g[C444] != 0, a, a // 2)
        return ((g[W] % a == 0) & _aligned(g[Y], a * g[SB]) & ((g[YP] | g[YF]) % a == 0) & _aligned(g[CB], c * g[SB])
                & _aligned(g[CR], c * g[SB]) & ((g[CP] | g[CF]) % c == 0))
    return np.where(((g[SC] | g[ST] | g[SR]) % 4 == 0) & _aligned(g[SRC], 16), _pick(planes_ok(8), planes_ok(4)), 0)


def parent_sited(g):
    """uav_clip_to_yuv420_sited, contiguous: its `planes_ok` lambda."""
    def planes_ok(a):
        return (g[W] % a == 0) & _aligned(g[Y], a * g[SB]) & _aligned(g[CB], a // 2 * g[SB]) & _aligned(g[CR], a // 2 * g[SB])
    return np.where(~_aligned(g[SRC], 16), 0, _pick(planes_ok(8), planes_ok(4)))


# ---- the grid ----------------------------------------------------------------------------------------------------------------
def _cross(*axes):
    """Every combination of the axes' entries; an axis is a list of scalars or of equal-length tuples.  Returns the columns."""
    axes = [np.array(a, dtype=np.int64).reshape(len(a), -1) for a in axes]
    idx = np.meshgrid(*[np.arange(len(a)) for a in axes], indexing="ij")
    return np.concatenate([a[i.reshape(-1)] for a, i in zip(axes, idx)], axis=1).T


def _records(kind, w, src, y, cb, cr, sc=0, st=0, sr=0, yp=0, yf=0, cp=0, cf=0, sb=1, c444=0):
    n = len(w)
    cols = [kind, w, BASE + src, BASE + y, BASE + cb, BASE + cr, sc, st, sr, yp, yf, cp, cf, sb, c444]
    return np.stack([np.broadcast_to(np.asarray(c, dtype=np.int64), (n,)) for c in cols])


def _grid():
    """(records (15, N), the parent's mode (N,), group (N,)): the group names the (direction, sb, c444) a record belongs to."""
    widths = list(range(1, 41))
    formats = [(1, 0), (1, 1), (2, 0), (2, 1)]                                # (sb, c444)
    parts = []
    # decode: every width, every address at every offset, both chroma layouts
    w, a0, a1, a2, a3, c444 = _cross(widths, OFFSETS, OFFSETS, OFFSETS, OFFSETS, [0, 1])
    g = _records(0, w, a0, a1, a2, a3, c444=c444)
    parts.append((g, parent_yuv_mode(g[W], g[SRC], g[Y], g[CB], g[CR], g[C444] != 0)))
    # encode, window entries: the addresses, with strides and pitches that keep every alignment
    w, a0, a1, a2, a3, sb, c444 = _cross(widths, OFFSETS, OFFSETS, OFFSETS, OFFSETS, formats)
    parts.append((_records(1, w, a0, a1, a2, a3, 4096, 3 * 4096, 64, 64, 4096, 64, 4096, sb, c444), None))
    # ... pitches w .. w + 9 (chroma from its own width), frame strides that are and are not multiples of 8, 4 and 2, source
    # strides that are multiples of 4 and one of each that is not, at aligned and at half-aligned bases
    pitch = [(i, i) for i in range(10)] + [(i, 0) for i in range(1, 10)] + [(0, j) for j in range(1, 10)]
    frame = [(0, 0), (4, 0), (2, 0), (1, 0), (0, 4), (0, 2), (0, 1)]
    source = [(4096, 12288, 64), (4096, 12288, 62), (4098, 12288, 64), (4096, 12289, 64)]
    bases = [(0, 0, 0, 0), (0, 4, 2, 2)]
    w, pi, pj, fi, fj, sc, st, sr, a0, a1, a2, a3, sb, c444 = _cross(widths, pitch, frame, source, bases, formats)
    cw = np.where(c444 != 0, w, (w + 1) // 2)
    parts.append((_records(1, w, a0, a1, a2, a3, sc, st, sr, w + pi, 4096 + fi, cw + pj, 4096 + fj, sb, c444), None))
    # the contiguous entries: frames (T,3,h,w) and planes Y (T,h,w), Cb / Cr (T,h/2,w/2), every even h <= 8 and even w
    w, h, a0, a1, a2, a3 = _cross(widths[1::2], [2, 4, 6, 8], OFFSETS, OFFSETS, OFFSETS, OFFSETS)
    for sb, parent in ((1, lambda g: parent_yuv_mode(g[W], g[SRC], g[Y], g[CB], g[CR], False)), (1, parent_sited), (2, parent_sited)):
        g = _records(1, w, a0, a1, a2, a3, h * w, 3 * h * w, w, w, h * w, w // 2, h * w // 4, sb, 0)
        parts.append((g, parent(g)))
    out, expect = [], []
    for g, e in parts:
        if e is None:                                                         # 8-bit 4:2:0 took the ladder, the rest the lambda
            e = np.where((g[SB] == 1) & (g[C444] == 0), parent_window420_u8(g), parent_window(g))
        out.append(g); expect.append(e)
    g = np.concatenate(out, axis=1)
    return g, np.concatenate(expect), g[KIND] * 100 + g[SB] * 10 + g[C444]


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_mode_pickers_return_what_the_four_spellings_returned(tmp_path):
    exe = str(tmp_path / "yuv_mode_main")
    subprocess.run([CXX, "-std=c++17", "-O1", "-o", exe, os.path.join(HERE, "yuv_mode_main.cpp")], check=True)
    g, expect, group = _grid()
    r = subprocess.run([exe], input=np.ascontiguousarray(g.T).astype("<i8").tobytes(), capture_output=True, check=True)
    got = np.frombuffer(r.stdout, dtype=np.uint8).astype(np.int64) - ord("0")
    assert got.shape == expect.shape
    for key in np.unique(group):
        sel = group == key
        assert set(np.unique(expect[sel])) == {0, 1, 2}, f"group {key}: the grid does not reach every mode"
    bad = np.flatnonzero(got != expect)
    assert bad.size == 0, f"{bad.size} of {got.size} picks differ, the first: record {g[:, bad[0]].tolist()} -> {got[bad[0]]}, parent {expect[bad[0]]}"
