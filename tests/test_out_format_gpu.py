"""The output formats beside 8-bit 4:2:0 on the device: `uav_clip_window_to_yuv` (csrc/yuv_io.hip) against
tests/yuv_fmt_ref.py, sample for sample, in every access mode and on every tail, with the bytes around the box and around the
planes untouched; its refusals; and the program's files for `--out-format` against the reference's planes of
`upscale_clip`'s fp32 frames."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
import yuv_fmt_ref  # noqa: E402
import yuv_ref  # noqa: E402
from test_stream_gpu import _Guarded, _values  # noqa: E402

pytestmark = pytest.mark.gpu
NEW = ("444", "420p10", "444p10")


def _coefs(matrix, full_range, depth):
    import ctypes
    from uav import video_io
    return (ctypes.c_int32 * 10)(*video_io.yuv_coefficients(matrix, full_range, depth=depth).forward)


def _convert_window(dev, full, frames_first, box, plane_hw, at, shift, fmt, matrix, full_range):
    """Window `box` = (y0, x0, h, w) of the tensor `full` ((3,T,H,W), or (T,3,H,W) with `frames_first`) through the C entry point
    into planes of `plane_hw` at offset `at` = (row, column), their bases `shift` SAMPLES past an aligned address, and everything
    the test asks of the result.  Returns the planes' boxes."""
    from uav import _lib
    lib = _lib.load()
    chroma444, depth, _ = yuv_fmt_ref.FORMATS[fmt]
    sb = 2 if depth == 10 else 1
    y0, x0, h, w = box
    view = full[:, :, y0:y0 + h, x0:x0 + w]
    c_dim, t_dim = (1, 0) if frames_first else (0, 1)
    t = view.shape[t_dim]
    ph, pw = plane_hw
    oy, ox = at
    s = 1 if chroma444 else 2                                                   # chroma sub-sampling
    cph, cpw = ph // s, pw // s
    planes = [_Guarded(t * ph * pw * sb, dev, shift * sb)] + [_Guarded(t * cph * cpw * sb, dev, shift * sb) for _ in range(2)]
    rc = lib.uav_clip_window_to_yuv(view.data_ptr(), view.stride(c_dim), view.stride(t_dim), view.stride(2),
                                    planes[0].ptr + (oy * pw + ox) * sb, pw, ph * pw,
                                    planes[1].ptr + ((oy // s) * cpw + ox // s) * sb, planes[2].ptr + ((oy // s) * cpw + ox // s) * sb,
                                    cpw, cph * cpw, t, h, w, int(chroma444), depth, _coefs(matrix, full_range, depth), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert all(p.intact() for p in planes), "a guard around the planes was written"
    frames = (view if frames_first else view.permute(1, 0, 2, 3)).contiguous().cpu().numpy()   # the materialised window (T,3,h,w)
    ref = yuv_fmt_ref.encode(frames, fmt, matrix, full_range)
    fill = 0xA5A5 if depth == 10 else 0xA5
    out = []
    for k, (p, r) in enumerate(zip(planes, ref)):
        d = 1 if k == 0 else s
        got = p.body().view("<u2" if depth == 10 else np.uint8).reshape(t, ph // d, pw // d)
        expect = np.full_like(got, fill)
        assert r.shape == (t, -(-h // d), -(-w // d))
        expect[:, oy // d:oy // d + r.shape[1], ox // d:ox // d + r.shape[2]] = r
        assert np.array_equal(got, expect), f"{fmt} plane {k}: window or its surroundings differ"
        out.append(r)
    return out


# (tensor H, W), window (y0, x0, h, w), planes (H, W), offset of the box in the planes — and the access mode each one reaches
WINDOWS = [((6, 8), (2, 4, 2, 2), (8, 12), (4, 6)),                 # (2,2): one thread, scalar
           ((10, 20), (2, 4, 6, 10), (12, 24), (4, 8)),             # (6,10): even, w % 4 != 0: scalar with a 2-pixel tail
           ((8, 24), (2, 4, 4, 12), (8, 32), (2, 8)),               # (4,12): w % 4 == 0: half-width stores and a scalar 4-pixel tail
           ((8, 32), (2, 4, 6, 24), (8, 48), (2, 16)),              # (6,24): w % 8 == 0: 16-byte loads, full-width stores
           ((8, 32), (2, 2, 6, 24), (8, 48), (2, 16)),              # ... from a crop at column 2: misaligned fp32 rows, scalar
           ((8, 32), (2, 4, 6, 24), (8, 44), (2, 12)),              # ... into a box at column 12 of pitch 44: the half-width mode
           ((8, 32), (2, 4, 6, 24), (8, 38), (2, 10)),              # ... pitches that are no multiple of 4: scalar
           ((68, 80), (2, 4, 64, 72), (72, 96), (4, 16))]           # (64,72): 288 threads, more than one block
WINDOWS_444 = [((6, 12), (1, 4, 3, 5), (6, 8), (2, 2)),             # odd h and w: a one-row run and an odd tail
               ((4, 8), (2, 4, 1, 1), (4, 6), (1, 3)),              # one pixel
               ((8, 24), (1, 4, 5, 20), (8, 32), (1, 8)),           # odd h with vector-friendly rows: the last run has one row
               ((8, 24), (1, 4, 3, 16), (8, 32), (3, 8))]


@pytest.mark.parametrize("matrix,full_range", yuv_ref.PAIRS)
@pytest.mark.parametrize("fmt", NEW)
def test_window_kernel_equals_the_reference_in_every_mode(dev, fmt, matrix, full_range):
    windows = WINDOWS + (WINDOWS_444 if yuv_fmt_ref.FORMATS[fmt][0] else [])
    for shape, box, plane_hw, at in windows:
        for t, frames_first in ((3, False), (1, True), (3, True), (1, False)):
            full = _values((t, 3) + shape if frames_first else (3, t) + shape, seed=sum(shape) + sum(box) + t).to(dev)
            _convert_window(dev, full, frames_first, box, plane_hw, at, 0, fmt, matrix, full_range)


@pytest.mark.parametrize("fmt", NEW)
def test_window_kernel_with_plane_bases_shifted_by_one_sample(dev, fmt):
    """Vector-friendly widths whose planes start one sample past an aligned address: the scalar mode, same samples."""
    windows = WINDOWS[:4] + WINDOWS[7:] + (WINDOWS_444[2:] if yuv_fmt_ref.FORMATS[fmt][0] else [])
    for shape, box, plane_hw, at in windows:
        full = _values((3, 2) + shape, seed=11).to(dev)
        _convert_window(dev, full, False, box, plane_hw, at, 1, fmt, "bt709", False)


@pytest.mark.parametrize("fmt", NEW)
def test_window_kernel_on_a_whole_decoder_chunk(dev, fmt):
    """(1,3,3,1280,1280), the decoder's layout, whole: what the untiled program converts per chunk."""
    full = _values((3, 3, 1280, 1280), seed=1280).to(dev)
    _convert_window(dev, full, False, (0, 0, 1280, 1280), (1280, 1280), (0, 0), 0, fmt, "bt709", False)


@pytest.mark.parametrize("matrix,full_range", yuv_ref.PAIRS)
def test_444_luma_is_the_420_kernels_luma_and_depth_8_420_is_that_kernel(dev, matrix, full_range):
    from uav import ops, video_io
    coefs = video_io.yuv_coefficients(matrix, full_range)
    dec = _values((3, 3, 40, 56), seed=9).to(dev)
    for window in (dec, dec[:, :, 2:38, 4:52], dec[:, :, 2:12, 2:20]):
        t, h, w = window.shape[1:]
        old = [torch.zeros((t, h, w), dtype=torch.uint8, device=dev)] + [torch.zeros((t, h // 2, w // 2), dtype=torch.uint8, device=dev) for _ in range(2)]
        ops.clip_window_to_yuv420_u8(window, *old, coefs)
        new = [torch.zeros((t, h, w), dtype=torch.uint8, device=dev) for _ in range(3)]
        ops.clip_window_to_yuv(window, *new, coefs, chroma444=True, depth=8)
        assert torch.equal(new[0], old[0])
        same = [torch.zeros_like(p) for p in old]
        ops.clip_window_to_yuv(window, *same, coefs, chroma444=False, depth=8)
        assert all(torch.equal(a, b) for a, b in zip(same, old))


def test_every_420_entry_point_shares_one_core(dev):
    """Contiguous (T,3,H,W) frames at one thread scalar, a 2-pixel tail, the half-width mode with its scalar 4-pixel tail, and the
    full-width mode: `uav_clip_to_yuv420_u8`, `uav_clip_window_to_yuv420_u8` and `uav_clip_window_to_yuv(0, 8)` write the same
    planes, and the luma of `uav_clip_to_yuv420_sited` is the luma of the unsited entry of its depth."""
    from uav import _lib, ops, video_io
    lib = _lib.load()
    for t, h, w in ((2, 2, 2), (1, 6, 10), (2, 4, 12), (1, 6, 24)):
        frames = _values((t, 3, h, w), seed=t + h + w).to(dev)
        for depth in (8, 10):
            coefs = video_io.yuv_coefficients("bt709", False, depth=depth)
            k = _coefs("bt709", False, depth)
            dtype = torch.uint8 if depth == 8 else torch.int16

            def planes():
                return [torch.zeros((t, h, w), dtype=dtype, device=dev)] + [torch.zeros((t, h // 2, w // 2), dtype=dtype, device=dev) for _ in range(2)]

            def geometry(p):                                                  # the contiguous tensors as a window
                return (frames.data_ptr(), h * w, 3 * h * w, w, p[0].data_ptr(), w, h * w, p[1].data_ptr(), p[2].data_ptr(), w // 2, h * w // 4, t, h, w)
            unsited = planes()
            assert lib.uav_clip_window_to_yuv(*geometry(unsited), 0, depth, k, None) == 0
            if depth == 8:
                window = planes()
                assert lib.uav_clip_window_to_yuv420_u8(*geometry(window), k, None) == 0
                torch.cuda.synchronize()
                contiguous = ops.clip_to_yuv420_u8(frames, coefs)
                for a, b, c in zip(contiguous, window, unsited):
                    assert torch.equal(a, c) and torch.equal(b, c), f"{(t, h, w)}: the 8-bit 4:2:0 entry points differ"
            torch.cuda.synchronize()
            sited = ops.clip_to_yuv420_sited(frames, coefs, depth=depth)
            assert torch.equal(sited[0], unsited[0]), f"{(t, h, w)} depth {depth}: sited luma is not the unsited entry's"


def test_ops_wrapper_takes_views_and_copies_nothing(dev):
    from uav import _lib, ops, video_io
    dec = _values((1, 3, 3, 48, 64), seed=5).to(dev)                          # decoder output
    window = dec[0, :, :, 8:40, 4:60]                                         # (3,3,32,56), a tile's crop
    frames = window.permute(1, 0, 2, 3).contiguous().cpu().numpy()
    for fmt in NEW:
        chroma444, depth, _ = yuv_fmt_ref.FORMATS[fmt]
        coefs = video_io.yuv_coefficients("bt601", True, depth=depth)
        dtype, fill = (torch.uint8, 0xA5) if depth == 8 else (torch.int16, 0x25A5)
        s = 1 if chroma444 else 2
        planes = [torch.full((3, 96, 128), fill, dtype=dtype, device=dev)] + [torch.full((3, 96 // s, 128 // s), fill, dtype=dtype, device=dev)
                                                                               for _ in range(2)]
        where = [(16, 48, 32, 88)] + [(16 // s, 48 // s, 32 // s, 88 // s)] * 2
        boxes = [p[:, a:b, c:d] for p, (a, b, c, d) in zip(planes, where)]
        assert ops.clip_window_to_yuv(window, *boxes, coefs, chroma444=chroma444, depth=depth) is None
        ref = yuv_fmt_ref.encode(frames, fmt, "bt601", True)
        again = video_io.postprocess_planes(window.permute(1, 0, 2, 3), coefs, fmt)          # (T,3,h,w) frames, frames_first inside
        for plane, box, (a, b, c, d), r, g in zip(planes, boxes, where, ref, again):
            assert np.array_equal(box.cpu().numpy().astype(r.dtype), r) and np.array_equal(g.cpu().numpy().astype(r.dtype), r)
            assert g.dtype == dtype
            mask = torch.ones_like(plane, dtype=torch.bool)
            mask[:, a:b, c:d] = False
            assert bool((plane[mask] == fill).all())
        bad = [(window[..., ::2], boxes), (window.double(), boxes), (window.cpu(), boxes), (window[:, :, :30], boxes),
               (window, [boxes[0], boxes[1], boxes[2].float()]), (window, [boxes[0][..., ::2]] + boxes[1:]),
               (window, [b.to(torch.int16 if depth == 8 else torch.uint8) for b in boxes])]
        if not chroma444:
            bad.append((window[:, :, :31], [boxes[0][:, :31], boxes[1], boxes[2]]))
        for w_, b_ in bad:
            with pytest.raises(_lib.UavError):
                ops.clip_window_to_yuv(w_, *b_, coefs, chroma444=chroma444, depth=depth)
        with pytest.raises(_lib.UavError):                                     # coefficients of the other depth
            ops.clip_window_to_yuv(window, *boxes, video_io.yuv_coefficients("bt601", True, depth=18 - depth), chroma444=chroma444, depth=depth)
        with pytest.raises(_lib.UavError):
            ops.clip_window_to_yuv(window, *boxes, coefs, chroma444=chroma444, depth=12)


def test_window_kernel_refuses_bad_arguments_before_any_launch(dev):
    from uav import _lib
    lib = _lib.load()
    src = torch.zeros(3, 1, 6, 6, device=dev)
    planes = [torch.full((128,), 0xA5, dtype=torch.uint8, device=dev) for _ in range(3)]
    p = [t.data_ptr() for t in planes]
    k8, k10 = _coefs("bt601", True, 8), _coefs("bt601", True, 10)

    def call(h, w, c444, depth, t_len=1, ptrs=None, coefs=None, strides=(36, 36, 6), pitches=None):
        s, y, cb, cr = ptrs or [src.data_ptr()] + p
        pitches = pitches or ((6, 36, 6, 36) if c444 else (6, 36, 3, 9))
        coefs = coefs if coefs is not None else (k10 if depth == 10 else k8)
        return lib.uav_clip_window_to_yuv(s, *strides, y, pitches[0], pitches[1], cb, cr, pitches[2], pitches[3], t_len, h, w, c444, depth, coefs, None)
    for c444, depth in ((1, 8), (0, 10), (1, 10), (0, 8)):
        assert call(6, 6, c444, depth) == 0                                   # the arguments the refusals below vary
    assert call(3, 5, 1, 8) == 0 and call(1, 1, 1, 10) == 0                   # 4:4:4 takes any h, w >= 1
    torch.cuda.synchronize()
    for t in planes:
        t.fill_(0xA5)
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    for c444, depth in ((1, 8), (0, 10), (1, 10)):
        for hole in range(4):                                                  # null pointers
            ptrs = [src.data_ptr()] + p
            ptrs[hole] = None
            assert call(6, 6, c444, depth, ptrs=ptrs) == EINVAL
        assert lib.uav_clip_window_to_yuv(src.data_ptr(), 36, 36, 6, p[0], 6, 36, p[1], p[2], 6, 36, 1, 6, 6, c444, depth, None, None) == EINVAL
        for h, w in ((0, 6), (6, 0), (-2, 6)):                                 # empty window
            assert call(h, w, c444, depth) == ESHAPE
        assert call(6, 6, c444, depth, t_len=0) == ESHAPE and call(2, 2, c444, depth, t_len=70000) == ESHAPE
        assert call(6, 6, c444, depth, strides=(36, 36, -6)) == ESHAPE
        cw = 6 if c444 else 3
        assert call(6, 6, c444, depth, pitches=(4, 36, cw, 36)) == ESHAPE and call(6, 6, c444, depth, pitches=(6, 36, cw - 1, 36)) == ESHAPE
        assert call(6, 6, c444, depth, t_len=2, pitches=(6, 30, cw, 36)) == ESHAPE       # frames of a plane would overlap
        assert call(6, 6, c444, depth, t_len=2, pitches=(6, 36, cw, (6 if c444 else 3) * cw - 1)) == ESHAPE
    for depth in (0, 9, 12, 16, -8):
        assert call(6, 6, 1, depth, coefs=k8) == EINVAL
    for c444 in (2, -1):
        assert call(6, 6, c444, 10) == EINVAL
    for h, w in ((3, 6), (6, 5), (1, 1)):                                      # odd sizes with 4:2:0
        assert call(h, w, 0, 10) == ESHAPE and call(h, w, 0, 8) == ESHAPE
    for hole in (1, 2, 3):                                                     # a 16-bit plane at an odd address
        ptrs = [src.data_ptr()] + p
        ptrs[hole] += 1
        assert call(6, 6, 1, 10, ptrs=ptrs) == EALIGN and call(6, 6, 0, 10, ptrs=ptrs) == EALIGN
        assert call(2, 2, 1, 8, ptrs=ptrs) == 0                               # ... which an 8-bit plane may have
    torch.cuda.synchronize()
    for t in planes:
        body = t.cpu().numpy()
        assert (body[16:] == 0xA5).all()                                       # only the three 2x2 8-bit calls wrote, into their boxes
        t.fill_(0xA5)


def test_program_writes_the_formats_on_the_device(dev, tmp_path):
    """One fresh process on the tiny seeded checkpoints (see `_child`)."""
    r = subprocess.run([sys.executable, "-X", "faulthandler", os.path.abspath(__file__), str(tmp_path)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, f"exit status {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    print(r.stdout[-3000:])


# ---- child ---------------------------------------------------------------------------------------------------------------
def _child(tmp):
    import time
    from test_cli_dropin_cpu import _clip_u8, _write_pretrained
    from uav import cli, video_io
    start = time.time()
    dev = torch.device("cuda:0")
    base = _write_pretrained(tmp)
    os.chdir(tmp)
    rgb = _clip_u8(5, 64, 96, 71).permute(0, 2, 3, 1).contiguous().numpy()
    video_io.write_y4m("in5.y4m", *yuv_ref.encode(rgb, "bt601", True), "30000/1001", True)
    clip = video_io.preprocess_planes(video_io.read_y4m("in5.y4m"), dev, "auto")
    pipe, _ = cli.load_pipeline(base, device=dev)
    common = ["-i", "in5.y4m", "-s", "2", "--pretrained", base, "--device", "cuda:0"]
    opts = dict(prompt="best quality, extremely detailed", negative_prompt="blur, worst quality", steps=2, guidance_scale=6, noise_level=120)
    header = b"YUV4MPEG2 W384 H256 F30000:1001 Ip A1:1 C444p10 XCOLORRANGE=FULL\n"
    # 64 rows are no more than the tiles' overlap, so `--tile_size 64` leaves this clip NO tile (tiling.tile_grid, the reference
    # program's rule): black frames from both paths.  The 68x160 clip has two tiles, whose crops start at columns that are
    # multiples of 4 and land in boxes of the chunk's planes.
    rgb = _clip_u8(4, 68, 160, 72).permute(0, 2, 3, 1).contiguous().numpy()
    video_io.write_y4m("tiled4.y4m", *yuv_ref.encode(rgb, "bt601", True), "30000/1001", True)
    tiled = video_io.preprocess_planes(video_io.read_y4m("tiled4.y4m"), dev, "auto")
    tile = (["--perform_tile", "--tile_size", "64"], dict(perform_tile=True, tile_size=64))
    jobs = (("in5", clip, [], {}, True), ("in5", clip) + tile + (False,), ("in5", clip, ["--color_fix", "Wavelet"], dict(color_fix="Wavelet"), True),
            ("tiled4", tiled) + tile + (True,))
    for k, (name, source, extra, kw, textured) in enumerate(jobs):
        assert cli.main(["-i", name + ".y4m"] + common[2:] + ["-o", f"o{k}", "--out-format", "444p10"] + extra) == 0
        got = open(f"o{k}/video/{name}_n120_g6_s2.y4m", "rb").read()
        frames = video_io.upscale_clip(pipe, source, generator=torch.Generator(device=dev).manual_seed(10), **opts, **kw)
        t, (h, w) = source.shape[2], source.shape[-2:]
        assert frames.shape == (t, 3, 4 * h, 4 * w) and frames.dtype == torch.float32
        head = header.replace(b"W384 H256", f"W{4 * w} H{4 * h}".encode())
        expect = yuv_fmt_ref.file_bytes(yuv_fmt_ref.encode(frames.cpu().numpy(), "444p10", "bt601", True), head)
        assert len(got) == len(expect) == len(head) + t * (6 + 3 * 16 * h * w * 2)
        assert got == expect, f"444p10 {name} {extra}: the file is not the reference's planes of upscale_clip's frames"
        assert (np.frombuffer(got, dtype="<u2", count=16 * h * w, offset=len(head) + 6).std() > 20) == textured
        print(f"444p10 {name} {' '.join(extra)}: {len(got)} bytes ok at {time.time() - start:.1f} s", flush=True)
    assert cli.main(common + ["-o", "plain"]) == 0
    assert cli.main(common + ["-o", "flag", "--out-format", "420"]) == 0
    plain = open("plain/video/in5_n120_g6_s2.y4m", "rb").read()
    assert plain == open("flag/video/in5_n120_g6_s2.y4m", "rb").read() and plain.startswith(b"YUV4MPEG2 W384 H256 F30000:1001 Ip A1:1 C420jpeg ")
    print(f"child total {time.time() - start:.1f} s", flush=True)


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "upscale-a-video_amd")]
    torch.set_num_threads(min(16, os.cpu_count() or 1))                         # as tests/conftest.py
    _child(sys.argv[1])
