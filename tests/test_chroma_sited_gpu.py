"""`--chroma sited` on the device: the two siting-aware 4:2:0 kernels (csrc/yuv_io.hip K13: uav_yuv420_sited_to_clip_f32 /
uav_clip_to_yuv420_sited) against the numpy reference of tests/chroma_sited_ref.py — bit for bit, inside 4 KiB guards, at every
alignment —, their argument checks, `preprocess_planes` / `postprocess_planes` against the direct ops, and the upscaling program
(uav/cli.py) end to end."""
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
import chroma_sited_ref as ref  # noqa: E402
import yuv_fmt_ref  # noqa: E402
import yuv_ref  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 4096
DECODER_SHAPES = [(3, 40, 56), (2, 37, 51), (1, 1, 1), (1, 2, 3), (2, 6, 12), (1, 5, 12), (2, 7, 16), (1, 3, 20)]
ENCODER_SHAPES = [(2, 2, 2), (1, 6, 10), (2, 4, 12), (1, 6, 24), (2, 10, 20), (3, 44, 72)]


def _planes(t, h, w, seed):
    rng = np.random.default_rng(seed)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    y = rng.integers(0, 256, (t, h, w), dtype=np.uint8)
    cb = rng.integers(0, 256, (t, ch, cw), dtype=np.uint8)
    cr = rng.integers(0, 256, (t, ch, cw), dtype=np.uint8)
    y.reshape(-1)[:4] = [0, 255, 16, 235][:y.size]                             # range ends: every clamp is exercised
    return y, cb, cr


def _frames(t, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    out = torch.randn(t, 3, h, w, generator=g) * 0.8
    edge = torch.tensor([-1.0, 1.0, -1.5, 1.5, 0.0, 0.999999, -0.999999, 0.5])
    flat = out.view(-1)
    flat[:min(8, flat.numel())] = edge[:min(8, flat.numel())]
    return out


class _Guarded:
    """`nbytes` of device memory with GUARD bytes of 0xA5 in front and behind (and `shift` bytes of misalignment)."""

    def __init__(self, nbytes, dev, shift=0, fill=None):
        self.buf = torch.full((GUARD + shift + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.lo, self.n = GUARD + shift, nbytes
        if fill is not None:
            self.buf[self.lo:self.lo + nbytes] = torch.from_numpy(np.ascontiguousarray(fill).reshape(-1).view(np.uint8)).to(dev)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.lo

    def body(self):
        return self.buf[self.lo:self.lo + self.n].cpu().numpy()

    def intact(self):
        return bool((self.buf[:self.lo] == 0xA5).all()) and bool((self.buf[self.lo + self.n:] == 0xA5).all())


_DECODED = {}


def _decoded(shape, tag, matrix, full):
    """The reference clip of a case, computed once: the planes and (3,T,H,W) fp32."""
    key = (shape, tag, matrix, full)
    if key not in _DECODED:
        y, cb, cr = _planes(*shape, seed=3 * sum(shape))
        _DECODED[key] = (y, cb, cr, ref.clip_of(ref.decode(y, cb, cr, matrix, full, ref.SITINGS[tag])))
    return _DECODED[key]


@pytest.mark.parametrize("matrix,full", yuv_ref.PAIRS)
@pytest.mark.parametrize("tag", sorted(ref.SITINGS))
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("shape", DECODER_SHAPES)
def test_sited_decoder_equals_the_reference_inside_its_guards(dev, shape, shift, tag, matrix, full):
    """The three MODEs (W % 8 == 0, W % 4 == 0 with its 4-pixel tail, any W; misaligned planes: the scalar kernel), odd sizes,
    single-sample chroma planes and every clamped border: the clip is the reference's, the 4 KiB of 0xA5 around all four buffers
    are untouched."""
    import ctypes
    from uav import _lib, video_io
    lib = _lib.load()
    t, h, w = shape
    y, cb, cr, want = _decoded(shape, tag, matrix, full)
    src = [_Guarded(p.size, dev, shift, fill=p) for p in (y, cb, cr)]
    out = _Guarded(3 * t * h * w * 4, dev)
    inv = (ctypes.c_int32 * 6)(*video_io.yuv_coefficients(matrix, full).inverse)
    centre_h, centre_v = ref.SITINGS[tag]
    rc = lib.uav_yuv420_sited_to_clip_f32(src[0].ptr, src[1].ptr, src[2].ptr, out.ptr, t, h, w, int(centre_h), int(centre_v), inv, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert out.intact() and all(s.intact() for s in src)
    assert np.array_equal(out.body().view(np.float32).reshape(3, t, h, w), want)


@pytest.mark.parametrize("matrix,full", yuv_ref.PAIRS)
@pytest.mark.parametrize("depth,shift", [(8, 0), (8, 1), (8, 2), (10, 0), (10, 2)])      # 16-bit planes: even shifts (odd: UAV_EALIGN, below)
@pytest.mark.parametrize("shape", ENCODER_SHAPES)
def test_sited_encoder_equals_the_reference_inside_its_guards(dev, shape, depth, shift, matrix, full):
    """Uint8 / int16 planes at byte offsets 0, 1 and 2 (the 8-, 4- and 2-byte stores of the MODEs and the scalar kernel), one
    chroma sample per row, W % 8 == 4 tails, more than one thread per row: the planes are the reference's, the guards untouched."""
    import ctypes
    from uav import _lib, video_io
    lib = _lib.load()
    t, h, w = shape
    frames = _frames(t, h, w, seed=5 * sum(shape))
    sb = depth // 8 + (depth % 8 > 0)
    outs = [_Guarded(n * sb, dev, shift) for n in (t * h * w, t * h * w // 4, t * h * w // 4)]
    fwd = (ctypes.c_int32 * 10)(*video_io.yuv_coefficients(matrix, full, depth).forward)
    dev_frames = frames.to(dev)
    assert lib.uav_clip_to_yuv420_sited(dev_frames.data_ptr(), outs[0].ptr, outs[1].ptr, outs[2].ptr, t, h, w, depth, fwd, None) == 0
    torch.cuda.synchronize()
    assert all(o.intact() for o in outs)
    for o, r in zip(outs, ref.encode(frames.numpy(), depth, matrix, full)):
        assert np.array_equal(o.body().view(r.dtype), r.reshape(-1))


def test_bad_arguments_are_refused_with_nothing_written(dev):
    import ctypes
    from uav import _lib, ops, video_io
    lib = _lib.load()
    k8, k10 = video_io.yuv_coefficients("bt601", False), video_io.yuv_coefficients("bt601", False, depth=10)
    fwd = (ctypes.c_int32 * 10)(*k8.forward)
    inv = (ctypes.c_int32 * 6)(*k8.inverse)
    src = torch.zeros(1, 3, 6, 6, device=dev)
    planes = [torch.full((128,), 0xA5, dtype=torch.uint8, device=dev) for _ in range(3)]
    clip = torch.full((3 * 36,), 7.0, device=dev)
    p = [t.data_ptr() for t in planes]
    enc, dec = lib.uav_clip_to_yuv420_sited, lib.uav_yuv420_sited_to_clip_f32
    for h, w in ((3, 6), (6, 5), (1, 1), (0, 6), (6, 0)):                       # odd or empty sides
        assert enc(src.data_ptr(), p[0], p[1], p[2], 1, h, w, 8, fwd, None) == -3                             # UAV_ESHAPE
    assert enc(src.data_ptr(), p[0], p[1], p[2], 0, 6, 6, 8, fwd, None) == -3
    assert enc(src.data_ptr(), p[0], p[1], p[2], 70000, 2, 2, 10, fwd, None) == -3
    for depth in (0, 9, 12, 16):
        assert enc(src.data_ptr(), p[0], p[1], p[2], 1, 6, 6, depth, fwd, None) == -1                         # UAV_EINVAL
    for hole in range(4):                                                      # null pointers
        args = [src.data_ptr()] + p
        args[hole] = None
        assert enc(*args, 1, 6, 6, 8, fwd, None) == -1
    assert enc(src.data_ptr(), p[0], p[1], p[2], 1, 6, 6, 8, None, None) == -1
    for odd in range(3):                                                       # a 16-bit plane at an odd address
        args = list(p)
        args[odd] += 1
        assert enc(src.data_ptr(), *args, 1, 6, 6, 10, fwd, None) == -2                                       # UAV_EALIGN
    for hole in range(4):
        args = p + [clip.data_ptr()]
        args[hole] = None
        assert dec(*args, 1, 6, 6, 0, 1, inv, None) == -1
    assert dec(p[0], p[1], p[2], clip.data_ptr(), 1, 6, 6, 0, 1, None, None) == -1
    for ch, cv in ((2, 1), (0, 2), (-1, 0), (1, -1)):                            # a siting is 0 or 1 per axis
        assert dec(p[0], p[1], p[2], clip.data_ptr(), 1, 6, 6, ch, cv, inv, None) == -1
    assert dec(p[0], p[1], p[2], clip.data_ptr(), 1, 0, 6, 0, 1, inv, None) == -3
    assert dec(p[0], p[1], p[2], clip.data_ptr(), 1, 6, 0, 0, 1, inv, None) == -3
    assert dec(p[0], p[1], p[2], clip.data_ptr(), 0, 6, 6, 0, 1, inv, None) == -3
    assert dec(p[0], p[1], p[2], clip.data_ptr(), 70000, 6, 6, 0, 1, inv, None) == -3
    torch.cuda.synchronize()
    assert all(bool((t == 0xA5).all()) for t in planes) and bool((clip == 7.0).all()) and bool((src == 0).all())
    # the ops refuse host tensors and bad shapes before the library is asked
    good = [torch.zeros(1, 4, 4, dtype=torch.uint8, device=dev), torch.zeros(1, 2, 2, dtype=torch.uint8, device=dev),
            torch.zeros(1, 2, 2, dtype=torch.uint8, device=dev)]
    assert tuple(ops.yuv420_sited_to_clip_f32(*good, k8, (False, True)).shape) == (3, 1, 4, 4)
    for bad in ([g.cpu() for g in good], [good[0], good[1], good[2][:, :1]], [good[0], good[0], good[0]], [good[0].float(), good[1], good[2]]):
        with pytest.raises(_lib.UavError):
            ops.yuv420_sited_to_clip_f32(*bad, k8, (False, True))
    for siting in ((2, 1), None, (True,), "left"):
        with pytest.raises(_lib.UavError):
            ops.yuv420_sited_to_clip_f32(*good, k8, siting)
    for frames, coefs, depth in ((torch.zeros(1, 3, 4, 4), k8, 8), (torch.zeros(1, 3, 3, 4, device=dev), k8, 8),
                                 (torch.zeros(1, 3, 4, 6, device=dev)[..., :5], k8, 8), (torch.zeros(1, 4, 4, 4, device=dev), k8, 8),
                                 (torch.zeros(1, 3, 4, 4, device=dev), k8, 12), (torch.zeros(1, 3, 4, 4, device=dev), k8, 10),
                                 (torch.zeros(1, 3, 4, 4, device=dev), k10, 8), (torch.zeros(1, 3, 4, 4, device=dev).half(), k8, 8)):
        with pytest.raises(_lib.UavError):
            ops.clip_to_yuv420_sited(frames, coefs, depth)


@pytest.mark.parametrize("matrix,full", yuv_ref.PAIRS)
def test_pre_and_postprocess_planes_equal_the_direct_ops(dev, matrix, full):
    from uav import ops, video_io
    shape = (2, 37, 51)
    y, cb, cr = _planes(*shape, seed=19)
    k8 = video_io.yuv_coefficients(matrix, full)
    on_dev = [torch.from_numpy(p).to(dev) for p in (y, cb, cr)]
    for tag in ("C420jpeg", "C420mpeg2", "C420", "", "C420paldv"):
        clip = video_io.Y4MClip(y, cb, cr, None, shape[1:], tag, full)
        got = video_io.preprocess_planes(clip, dev, matrix, chroma="sited")
        assert torch.equal(got, ops.yuv420_sited_to_clip_f32(*on_dev, k8, video_io.chroma_siting(tag)).unsqueeze(0))
        assert np.array_equal(got[0].cpu().numpy(), ref.clip_of(ref.decode(y, cb, cr, matrix, full, video_io.chroma_siting(tag))))
        today = ops.yuv420_to_clip_f32(*on_dev, k8).unsqueeze(0)
        assert torch.equal(video_io.preprocess_planes(clip, dev, matrix), today) and not torch.equal(got, today)
        assert torch.equal(video_io.preprocess_planes(clip, dev, matrix, chroma="replicate"), today)
    # 4:4:4 input has nothing to up-sample
    y4, cb4, cr4 = y, np.ascontiguousarray(y[:, ::-1]), np.ascontiguousarray(y[:, :, ::-1])
    clip = video_io.Y4MClip(y4, cb4, cr4, None, shape[1:], "C444", full)
    assert torch.equal(video_io.preprocess_planes(clip, dev, matrix, chroma="sited"), video_io.preprocess_planes(clip, dev, matrix))
    frames = _frames(2, 10, 20, seed=23).to(dev)
    for fmt in ("420", "420p10"):
        depth = video_io.OUT_FORMATS[fmt].depth
        coefs = video_io.yuv_coefficients(matrix, full, depth)
        got = video_io.postprocess_planes(frames, coefs, fmt, siting=(False, True))
        direct = ops.clip_to_yuv420_sited(frames, coefs, depth)
        want = ref.encode(frames.cpu().numpy(), depth, matrix, full)
        today = video_io.postprocess_planes(frames, coefs, fmt)
        for g, d, w, o in zip(got, direct, want, today):
            assert g.dtype == (torch.uint8 if depth == 8 else torch.int16) and torch.equal(g, d)
            assert np.array_equal(g.cpu().numpy().view(w.dtype), w)
        assert torch.equal(got[0], today[0]) and not torch.equal(got[1], today[1])            # the luma is today's, the chroma is not
        for same in (None, (True, True)):                                      # centre / centre IS the block mean
            assert all(torch.equal(a, b) for a, b in zip(video_io.postprocess_planes(frames, coefs, fmt, siting=same), today))
    for fmt in ("444", "444p10"):                                              # no output filter
        coefs = video_io.yuv_coefficients(matrix, full, video_io.OUT_FORMATS[fmt].depth)
        assert all(torch.equal(a, b) for a, b in zip(video_io.postprocess_planes(frames, coefs, fmt, siting=(False, True)),
                                                     video_io.postprocess_planes(frames, coefs, fmt)))


def test_program_end_to_end_on_the_device(dev, tmp_path):
    """uav/cli.py with `--chroma sited` on tiny seeded checkpoints, in one fresh process: the planes of the written files equal
    the reference encoder applied to upscale_clip(...) of the sited-preprocessed clip, and a second run writes the same bytes."""
    r = subprocess.run([sys.executable, "-X", "faulthandler", os.path.abspath(__file__), str(tmp_path)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, f"exit status {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    print(r.stdout[-1500:])


def _child(tmp):
    import time
    from test_cli_dropin_cpu import _clip_u8, _write_pretrained
    from uav import cli, video_io
    start = time.time()
    dev = torch.device("cuda:0")
    base = _write_pretrained(tmp)
    os.chdir(tmp)

    def write_input(name, t, h, w, seed):
        rgb = _clip_u8(t, h, w, seed).permute(0, 2, 3, 1).contiguous().numpy()
        video_io.write_y4m(name, *yuv_ref.encode(rgb, "bt601", False), "30000/1001", False)

    write_input("plain.y4m", 3, 64, 96, 41)
    write_input("tiled.y4m", 2, 68, 160, 42)
    jobs = (("plain", [], {}, (3, 256, 384)),
            ("tiled", ["--perform_tile", "--tile_size", "64"], dict(perform_tile=True, tile_size=64), (2, 272, 640)))
    pipe, _ = cli.load_pipeline(base, device=dev)
    for name, extra, kw, shape in jobs:
        source = video_io.read_y4m(name + ".y4m")
        assert source.colorspace == "C420mpeg2" and source.full_range is False
        clip = video_io.preprocess_planes(source, dev, "auto", chroma="sited")
        assert not torch.equal(clip, video_io.preprocess_planes(source, dev, "auto"))
        frames = video_io.upscale_clip(pipe, clip, prompt="best quality, extremely detailed", negative_prompt="blur, worst quality", steps=2,
                                       guidance_scale=6, noise_level=120, generator=torch.Generator(device=dev).manual_seed(10), **kw)
        want = ref.encode(frames.cpu().numpy(), 8, video_io.auto_matrix(frames.shape[-2]), False)
        argv = ["-i", name + ".y4m", "-s", "2", "--pretrained", base, "--device", "cuda:0", "--chroma", "sited"] + extra
        assert cli.main(argv + ["-o", "run1"]) == 0
        assert cli.main(argv + ["-o", "run2"]) == 0
        out = f"run1/video/{name}_n120_g6_s2.y4m"
        first = open(out, "rb").read()
        assert first == open(out.replace("run1", "run2"), "rb").read(), f"{name}: two runs of the program differ"
        assert first.startswith(f"YUV4MPEG2 W{shape[2]} H{shape[1]} F30000:1001 Ip A1:1 C420mpeg2 XCOLORRANGE=LIMITED\nFRAME\n".encode())
        got = video_io.read_y4m(out)
        assert got.y.shape == shape and got.y.std() > 5
        assert all(np.array_equal(g, w) for g, w in zip((got.y, got.cb, got.cr), want)), f"{name}: file != reference of the direct call"
        print(f"{name}: {shape} ok at {time.time() - start:.1f} s", flush=True)


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "upscale-a-video_amd")]
    torch.set_num_threads(min(16, os.cpu_count() or 1))                         # as tests/conftest.py
    _child(sys.argv[1])
