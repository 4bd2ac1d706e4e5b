"""The Y4M front end on the device: the two Y'CbCr kernels (csrc/yuv_io.hip K13: uav_yuv420_to_clip_f32 /
uav_yuv444_to_clip_f32 / uav_clip_to_yuv420_u8) against the numpy reference of tests/yuv_ref.py composed with the existing
pre/post-processing — bit for bit —, their bounds behaviour, and the upscaling program (uav/cli.py) end to end."""
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
import yuv_ref  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 4096


def _planes(t, h, w, seed, chroma444=False):
    rng = np.random.default_rng(seed)
    ch, cw = (h, w) if chroma444 else ((h + 1) // 2, (w + 1) // 2)
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


@pytest.mark.parametrize("matrix,full", yuv_ref.PAIRS)
@pytest.mark.parametrize("shape,chroma444", [((3, 40, 56), False), ((2, 37, 51), False), ((1, 1, 1), False), ((2, 6, 12), False),
                                             ((3, 40, 56), True), ((2, 37, 51), True), ((1, 5, 12), True)])
def test_yuv_to_clip_equals_preprocess_of_decoded_rgb(dev, shape, chroma444, matrix, full):
    from uav import ops, video_io
    y, cb, cr = _planes(*shape, seed=sum(shape), chroma444=chroma444)
    rgb = yuv_ref.decode(y, cb, cr, matrix, full, chroma444=chroma444)
    ref = video_io.preprocess_frames(torch.from_numpy(rgb).permute(0, 3, 1, 2).contiguous().to(dev))
    coefs = video_io.yuv_coefficients(matrix, full)
    out = ops.yuv420_to_clip_f32(*(torch.from_numpy(p).to(dev) for p in (y, cb, cr)), coefs, chroma444=chroma444)
    assert out.dtype == torch.float32 and tuple(out.shape) == (3,) + shape
    assert torch.equal(out.unsqueeze(0), ref)
    clip = video_io.Y4MClip(y, cb, cr, None, shape[1:], "C444" if chroma444 else "C420mpeg2", full)
    assert torch.equal(video_io.preprocess_planes(clip, dev, matrix), ref)


@pytest.mark.parametrize("matrix,full", yuv_ref.PAIRS)
def test_large_y4m_through_read_frames_is_area_pooled(dev, tmp_path, matrix, full):
    """(2,1280,1284): file -> read_frames -> preprocess_planes, the >= 1280-px area pooling included (2e-6 absolute, the bound
    tests/test_video_io_gpu.py allows for the pooling's 16-term fp32 means)."""
    from uav import video_io
    y, cb, cr = _planes(2, 1280, 1284, seed=11)
    path = tmp_path / "big.y4m"
    video_io.write_y4m(path, y, cb, cr, 24, full)
    clip, fps = video_io.read_frames(str(path))
    assert fps == 24 and clip.full_range is full
    rgb = yuv_ref.decode(y, cb, cr, matrix, full)
    ref = video_io.preprocess_frames(torch.from_numpy(rgb).permute(0, 3, 1, 2).contiguous().to(dev))
    out = video_io.preprocess_planes(clip, dev, matrix)
    assert tuple(out.shape) == (1, 3, 2, 320, 321) == tuple(ref.shape)
    assert (out - ref).abs().max().item() < 2e-6
    if matrix == "bt709":                                                      # 1280 rows: what `auto` picks
        assert torch.equal(video_io.preprocess_planes(clip, dev, "auto"), out)


@pytest.mark.parametrize("matrix,full", yuv_ref.PAIRS)
@pytest.mark.parametrize("shape", [(3, 44, 72), (2, 2, 2), (1, 6, 10), (2, 4, 12), (2, 1280, 1280)])
def test_clip_to_yuv420_equals_encoder_of_postprocessed_frames(dev, shape, matrix, full):
    from uav import video_io
    frames = _frames(*shape, seed=sum(shape)).to(dev)
    rgb = video_io.postprocess_frames(frames).cpu().numpy()
    ry, rcb, rcr = yuv_ref.encode(rgb, matrix, full)
    y, cb, cr = video_io.postprocess_planes(frames, video_io.yuv_coefficients(matrix, full))
    assert y.dtype == cb.dtype == cr.dtype == torch.uint8
    assert np.array_equal(y.cpu().numpy(), ry) and np.array_equal(cb.cpu().numpy(), rcb) and np.array_equal(cr.cpu().numpy(), rcr)


def test_bad_arguments_are_refused_before_any_launch(dev):
    import ctypes
    from uav import _lib, ops, video_io
    lib = _lib.load()
    fwd = (ctypes.c_int32 * 10)(*video_io.yuv_coefficients("bt601", True).forward)
    inv = (ctypes.c_int32 * 6)(*video_io.yuv_coefficients("bt601", True).inverse)
    src = torch.zeros(1, 3, 6, 6, device=dev)
    planes = [torch.full((64,), 0xA5, dtype=torch.uint8, device=dev) for _ in range(3)]
    clip = torch.full((3 * 36,), 7.0, device=dev)
    p = [t.data_ptr() for t in planes]
    for h, w in ((3, 6), (6, 5), (1, 1)):                                       # odd height / width
        assert lib.uav_clip_to_yuv420_u8(src.data_ptr(), p[0], p[1], p[2], 1, h, w, fwd, None) == -3          # UAV_ESHAPE
    assert lib.uav_clip_to_yuv420_u8(src.data_ptr(), p[0], p[1], p[2], 0, 6, 6, fwd, None) == -3
    assert lib.uav_clip_to_yuv420_u8(src.data_ptr(), p[0], p[1], p[2], 70000, 2, 2, fwd, None) == -3
    for hole in range(4):                                                      # null pointers
        args = [src.data_ptr()] + p
        args[hole] = None
        assert lib.uav_clip_to_yuv420_u8(*args, 1, 6, 6, fwd, None) == -1                                     # UAV_EINVAL
    assert lib.uav_clip_to_yuv420_u8(src.data_ptr(), p[0], p[1], p[2], 1, 6, 6, None, None) == -1
    for fn in (lib.uav_yuv420_to_clip_f32, lib.uav_yuv444_to_clip_f32):
        for hole in range(4):
            args = p + [clip.data_ptr()]
            args[hole] = None
            assert fn(*args, 1, 6, 6, inv, None) == -1
        assert fn(p[0], p[1], p[2], clip.data_ptr(), 1, 6, 6, None, None) == -1
        assert fn(p[0], p[1], p[2], clip.data_ptr(), 1, 0, 6, inv, None) == -3
        assert fn(p[0], p[1], p[2], clip.data_ptr(), 0, 6, 6, inv, None) == -3
    torch.cuda.synchronize()
    assert all(bool((t == 0xA5).all()) for t in planes) and bool((clip == 7.0).all())                         # nothing was launched
    with pytest.raises(_lib.UavError):
        ops.clip_to_yuv420_u8(torch.zeros(1, 3, 3, 4, device=dev), video_io.yuv_coefficients("bt601", True))
    with pytest.raises(_lib.UavError):
        ops.clip_to_yuv420_u8(torch.zeros(1, 3, 4, 4), video_io.yuv_coefficients("bt601", True))               # CPU tensor


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


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("shape,chroma444", [((2, 37, 51), False), ((1, 5, 12), False), ((1, 1, 1), False), ((2, 7, 16), False),
                                             ((1, 3, 20), False), ((2, 37, 51), True), ((1, 5, 12), True)])
def test_yuv_to_clip_writes_inside_its_output_only(dev, shape, chroma444, shift):
    """Odd sizes, the 4-pixel tail of a W % 8 == 4 row, a single pixel and misaligned planes (the scalar kernel): the clip is
    right and the 4 KiB of 0xA5 around it are untouched."""
    import ctypes
    from uav import _lib, video_io
    lib = _lib.load()
    t, h, w = shape
    y, cb, cr = _planes(t, h, w, seed=3 * sum(shape), chroma444=chroma444)
    src = [_Guarded(p.size, dev, shift, fill=p) for p in (y, cb, cr)]
    out = _Guarded(3 * t * h * w * 4, dev)
    inv = (ctypes.c_int32 * 6)(*video_io.yuv_coefficients("bt601", False).inverse)
    fn = lib.uav_yuv444_to_clip_f32 if chroma444 else lib.uav_yuv420_to_clip_f32
    assert fn(src[0].ptr, src[1].ptr, src[2].ptr, out.ptr, t, h, w, inv, None) == 0
    torch.cuda.synchronize()
    assert out.intact() and all(s.intact() for s in src)
    rgb = yuv_ref.decode(y, cb, cr, "bt601", False, chroma444=chroma444).astype(np.float32)
    ref = ((torch.from_numpy(rgb) / 255. - 0.5) * 2).permute(3, 0, 1, 2).contiguous().numpy()
    assert np.array_equal(out.body().view(np.float32).reshape(3, t, h, w), ref)


@pytest.mark.parametrize("shift", [0, 1, 2])
@pytest.mark.parametrize("shape", [(1, 6, 10), (2, 4, 12), (2, 2, 2), (1, 6, 24), (2, 10, 20)])
def test_clip_to_yuv420_writes_inside_its_planes_only(dev, shape, shift):
    import ctypes
    from uav import _lib, video_io
    lib = _lib.load()
    t, h, w = shape
    frames = _frames(t, h, w, seed=5 * sum(shape)).to(dev)
    outs = [_Guarded(n, dev, shift) for n in (t * h * w, t * h * w // 4, t * h * w // 4)]
    fwd = (ctypes.c_int32 * 10)(*video_io.yuv_coefficients("bt709", False).forward)
    assert lib.uav_clip_to_yuv420_u8(frames.data_ptr(), outs[0].ptr, outs[1].ptr, outs[2].ptr, t, h, w, fwd, None) == 0
    torch.cuda.synchronize()
    assert all(o.intact() for o in outs)
    ref = yuv_ref.encode(video_io.postprocess_frames(frames).cpu().numpy(), "bt709", False)
    for o, r in zip(outs, ref):
        assert np.array_equal(o.body(), r.reshape(-1))


def test_program_end_to_end_on_the_device(dev, tmp_path):
    """uav/cli.py on tiny seeded checkpoints, in one fresh process: the planes of the written files equal the numpy encoder
    of postprocess_frames(upscale_clip(...)) called directly, a second run writes the same bytes, and upscale_clip's flow
    branch equals the same calls made by hand."""
    r = subprocess.run([sys.executable, "-X", "faulthandler", os.path.abspath(__file__), str(tmp_path)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, f"exit status {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    print(r.stdout[-1500:])


def _child(tmp):
    import time
    import synth
    from test_cli_dropin_cpu import _clip_u8, _write_pretrained
    from uav import cli, video_io
    start = time.time()
    dev = torch.device("cuda:0")
    base = _write_pretrained(tmp)
    os.chdir(tmp)

    def write_input(name, t, h, w, seed):
        rgb = _clip_u8(t, h, w, seed).permute(0, 2, 3, 1).contiguous().numpy()
        video_io.write_y4m(name, *yuv_ref.encode(rgb, "bt601", True), "30000/1001", True)

    def direct(pipe, path, **kw):
        clip = video_io.preprocess_planes(video_io.read_y4m(path), dev, "auto")
        out = video_io.upscale_clip(pipe, clip, prompt="best quality, extremely detailed", negative_prompt="blur, worst quality", steps=2,
                                    guidance_scale=6, noise_level=120, generator=torch.Generator(device=dev).manual_seed(10), **kw)
        return yuv_ref.encode(video_io.postprocess_frames(out).cpu().numpy(), video_io.auto_matrix(out.shape[-2]), True)

    write_input("plain.y4m", 3, 64, 96, 41)
    write_input("tiled.y4m", 2, 68, 160, 42)
    jobs = (("plain", ["--color_fix", "Wavelet"], dict(color_fix="Wavelet"), (3, 256, 384)),
            ("tiled", ["--perform_tile", "--tile_size", "64"], dict(perform_tile=True, tile_size=64), (2, 272, 640)))
    pipe, _ = cli.load_pipeline(base, device=dev)
    for name, extra, kw, shape in jobs:
        argv = ["-i", name + ".y4m", "-s", "2", "--pretrained", base, "--device", "cuda:0"] + extra
        assert cli.main(argv + ["-o", "run1"]) == 0
        assert cli.main(argv + ["-o", "run2"]) == 0
        out = f"run1/video/{name}_n120_g6_s2.y4m"
        first = open(out, "rb").read()
        assert first == open(out.replace("run1", "run2"), "rb").read(), f"{name}: two runs of the program differ"
        assert first.startswith(f"YUV4MPEG2 W{shape[2]} H{shape[1]} F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=FULL\nFRAME\n".encode())
        got = video_io.read_y4m(out)
        y, cb, cr = direct(pipe, name + ".y4m", **kw)
        assert got.y.shape == shape and got.y.std() > 5
        assert np.array_equal(got.y, y) and np.array_equal(got.cb, cb) and np.array_equal(got.cr, cr), f"{name}: file != direct call"
        print(f"{name}: {shape} ok at {time.time() - start:.1f} s", flush=True)

    # the flow branch: RAFT flows of the whole clip -> pipeline(..., flows_bi=[forward, backward], propagation_steps=[1])
    from models_video.RAFT.raft_bi import RAFT_bi
    from models_video.propagation_module import Propagation
    raft = RAFT_bi(model_path=None, device="cpu")
    raft.fix_raft.load_state_dict(synth.synth_state_dict(raft.fix_raft.state_dict(), seed=777))
    raft = raft.to(dev)
    pipe.propagator = Propagation(4, learnable=False).to(dev)
    clip = synth.synth_clip(1, 3, 128, 160, seed=5, motion=(2, 1)).to(dev)
    common = dict(num_inference_steps=2, guidance_scale=6, noise_level=120, negative_prompt="n", propagation_steps=[1])
    seen = []                                                                  # flows the propagator was called with
    pipe.propagator.register_forward_hook(lambda module, args, output: seen.append((args[1].clone(), args[2].clone())))
    mine = video_io.upscale_clip(pipe, clip, prompt="p", negative_prompt="n", raft=raft, propagation_steps=[1], steps=2, guidance_scale=6,
                                 noise_level=120, generator=torch.Generator(device=dev).manual_seed(10))
    with torch.no_grad():
        ff, fb = raft.forward_slicing(clip)
        hand = pipe("p", image=clip, flows_bi=[ff, fb], generator=torch.Generator(device=dev).manual_seed(10), **common).images
    hand = hand.squeeze(0).permute(1, 0, 2, 3).contiguous().float()
    assert tuple(mine.shape) == (3, 3, 512, 640) and torch.equal(mine, hand)
    # one propagation per call, and upscale_clip handed the pipeline the forward flows first, the backward flows second
    assert len(seen) == 2 and tuple(ff.shape) == (1, 2, 2, 128, 160) and not torch.equal(ff, fb)
    for got_f, got_b in seen:
        assert torch.equal(got_f.float(), ff.to(got_f.dtype).float()) and torch.equal(got_b.float(), fb.to(got_b.dtype).float())
    print(f"flow branch ok; child total {time.time() - start:.1f} s", flush=True)


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "upscale-a-video_amd")]
    torch.set_num_threads(min(16, os.cpu_count() or 1))                         # as tests/conftest.py
    _child(sys.argv[1])
