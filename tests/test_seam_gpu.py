"""`--scene-overlap` on the device: the cross-fade kernel (csrc/frame_axpby.hip, `uav_frame_axpby_f32`) against numpy's float32
expression — bit for bit, through the raw C ABI, inside 4 KiB guards, with 16-byte and scalar accesses, out of place and in place —,
its refusals, the `ops` wrapper, and the upscaling program (uav/cli.py) end to end in one child process."""
import functools
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
import scene_ref  # noqa: E402
import yuv_ref  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 4096
# (t_len, frame_elems): one element; odd sizes and sizes % 4 != 0 (scalar whatever the alignment); one vector; more than one block
# of 2048 elements with a short last one; a frame of the program's input size; more frames than weights in the table below
SHAPES = [(1, 1), (2, 3), (3, 4), (2, 7), (3, 189), (4, 1024), (3, 4097), (2, 3 * 64 * 96), (65, 5)]
# (wa, wb): 0 and 1, the (K-j)/(K+1) pairs of K = 3, and those of K = 2, which no float32 holds exactly
WEIGHTS = [(0.0, 1.0), (1.0, 0.0), (3 / 4, 1 / 4), (2 / 4, 2 / 4), (1 / 4, 3 / 4), (2 / 3, 1 / 3), (1 / 3, 2 / 3), (0.0, 0.0), (1.0, 1.0)]


class _Guarded:
    """`nbytes` of device memory, every byte 0xA5, with GUARD bytes in front and behind (and `shift` bytes of misalignment)."""

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


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Seeded frames in [-1.3, 1.3] with signed zeros among them, the weights, and numpy's float32 result, computed once."""
    t, n = shape
    g = torch.Generator().manual_seed(31 * t + n)
    a, b = ((torch.rand(t, n, generator=g) * 2.6 - 1.3).numpy() for _ in range(2))
    for i, (za, zb) in enumerate([(-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0), (0.0, 0.0)][:n]):
        a[:, i], b[:, i] = za, zb
    pairs = [WEIGHTS[i % len(WEIGHTS)] for i in range(t)]
    wa, wb = (np.array([p[i] for p in pairs], dtype=np.float64).astype(np.float32) for i in (0, 1))
    want = np.stack([np.float32(wa[i]) * a[i] + np.float32(wb[i]) * b[i] for i in range(t)])
    assert want.dtype == np.float32
    return a, b, wa, wb, want


def _bits(x):
    return np.ascontiguousarray(x).reshape(-1).view(np.uint32)


def _run(shape, dev, shift, into=None):
    """The case through the raw entry point, every buffer guarded and `shift` bytes off a 16-byte boundary; `into` = 'a' / 'b'
    writes over that input.  Returns the bits of the output."""
    from uav import _lib
    lib = _lib.load()
    t, n = shape
    a, b, wa, wb, _ = _case(shape)
    ga, gb = _Guarded(a.size * 4, dev, shift, fill=a), _Guarded(b.size * 4, dev, shift, fill=b)
    gwa, gwb = _Guarded(t * 4, dev, shift, fill=wa), _Guarded(t * 4, dev, shift, fill=wb)
    out = {"a": ga, "b": gb}.get(into) or _Guarded(a.size * 4, dev, shift)
    assert ga.ptr % 16 == gb.ptr % 16 == out.ptr % 16 == shift
    assert lib.uav_frame_axpby_f32(ga.ptr, gb.ptr, out.ptr, gwa.ptr, gwb.ptr, t, n, None) == 0
    torch.cuda.synchronize()
    assert all(g.intact() for g in (ga, gb, gwa, gwb, out))
    for g, src in ((ga, a), (gb, b), (gwa, wa), (gwb, wb)):
        assert g is out or np.array_equal(g.body().view(np.uint32), _bits(src))          # the inputs are unchanged
    return out.body().view(np.uint32)


@pytest.mark.parametrize("shift", [0, 4], ids=["aligned", "one_float_in"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_numpy_float32_bit_for_bit(dev, shape, shift):
    """`shift` = 4: every base is one float past a 16-byte boundary, so every access is scalar whatever frame_elems is."""
    assert np.array_equal(_run(shape, dev, shift), _bits(_case(shape)[4]))


@pytest.mark.parametrize("shift", [0, 4], ids=["aligned", "one_float_in"])
@pytest.mark.parametrize("into", ["a", "b"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_in_place(dev, shape, into, shift):
    assert np.array_equal(_run(shape, dev, shift, into), _bits(_case(shape)[4]))


def test_bad_arguments_are_refused_with_nothing_written(dev):
    from uav import _lib
    fn = _lib.load().uav_frame_axpby_f32
    a, b = torch.ones(2, 8, device=dev), torch.ones(2, 8, device=dev)
    wa, wb = torch.ones(2, device=dev), torch.ones(2, device=dev)
    out = torch.full((2, 8), 7.0, device=dev)
    good = [a.data_ptr(), b.data_ptr(), out.data_ptr(), wa.data_ptr(), wb.data_ptr(), 2, 8, None]
    for hole in range(5):                                                       # null pointers
        args = list(good)
        args[hole] = None
        assert fn(*args) == -1                                                  # UAV_EINVAL
    for t, n in ((0, 8), (-1, 8), (65536, 8), (2, 0), (2, -8), (2, 2 ** 36), (2, 2 ** 62)):
        assert fn(*good[:5], t, n, None) == -3                                  # UAV_ESHAPE; the last two: a grid beyond the launch limits
    for hole in range(5):                                                       # pointers off a 4-byte boundary
        for off in (1, 2, 3):
            args = list(good)
            args[hole] += off
            assert fn(*args) == -2                                              # UAV_EALIGN
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((a == 1.0).all()) and bool((b == 1.0).all())
    assert fn(*good) == 0
    torch.cuda.synchronize()
    assert bool((out == 2.0).all())


def test_the_op_takes_views_returns_out_and_refuses_host_tensors(dev):
    from uav import _lib, ops
    a, b, wa, wb, want = _case((3, 189))
    big_a, big_b, big_out = (torch.full((5, 3, 7, 9), 9.0, device=dev) for _ in range(3))
    big_a[1:4], big_b[1:4] = (torch.from_numpy(x).to(dev).view(3, 3, 7, 9) for x in (a, b))
    wa, wb = torch.from_numpy(wa).to(dev), torch.from_numpy(wb).to(dev)
    out = big_out[1:4]
    assert ops.frame_axpby_f32(big_a[1:4], big_b[1:4], wa, wb, out=out) is out
    assert np.array_equal(_bits(big_out[1:4].cpu().numpy()), _bits(want)) and bool((big_out[0] == 9.0).all()) and bool((big_out[4] == 9.0).all())
    fresh = ops.frame_axpby_f32(big_a[1:4], big_b[1:4], wa, wb)
    assert fresh.shape == (3, 3, 7, 9) and fresh.device == big_a.device and np.array_equal(_bits(fresh.cpu().numpy()), _bits(want))
    view = big_a[1:4]
    assert ops.frame_axpby_f32(view, big_b[1:4], wa, wb, out=view) is view      # in place, inside a larger tensor
    assert np.array_equal(_bits(big_a[1:4].cpu().numpy()), _bits(want)) and bool((big_a[0] == 9.0).all()) and bool((big_a[4] == 9.0).all())
    x = torch.zeros(3, 4, device=dev)
    for bad in ((x.cpu(), x, wa, wb), (x, x.cpu(), wa, wb), (x, x, wa.cpu(), wb), (x, x, wa, wb.cpu()), (x.half(), x.half(), wa, wb),
                (x, torch.zeros(3, 5, device=dev), wa, wb), (x, x, wa[:2], wb), (x, x, wa.double(), wb),
                (torch.zeros(3, 8, device=dev)[:, ::2], x, wa, wb)):
        with pytest.raises(_lib.UavError):
            ops.frame_axpby_f32(*bad)
    with pytest.raises(_lib.UavError):
        ops.frame_axpby_f32(x, x, wa, wb, out=x.cpu())


# ---- the program, in one child process -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _program(tmp):
    return subprocess.run([sys.executable, "-X", "faulthandler", os.path.abspath(__file__), tmp], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def program(dev, tmp_path_factory):
    r = _program(str(tmp_path_factory.mktemp("seam")))
    assert r.returncode == 0, f"exit status {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    print(r.stdout[-1500:])
    return r.stdout


def test_program_cross_fades_forced_splits_on_the_device(program):
    """uav/cli.py `-s 2 --scenes auto --scene-max 8 --scene-overlap 3` on tiny seeded checkpoints and 26 frames of 64x96 without a
    cut: exit status 0, 26 frames of 256x384, and the planes of the file equal `postprocess_planes` of the composition restated by
    hand — `upscale_clip` on [0,11), [8,19), [16,26) with one generator, blended with `ops.frame_axpby_f32`."""
    assert "cross-fade: ok" in program


def test_program_cross_fades_the_same_way_on_tiles(program):
    """The same with `--perform_tile --tile_size 48`: the tile-by-tile window conversion and the seam's fp32 frames meet."""
    assert "cross-fade on tiles: ok" in program


def test_program_writes_the_same_bytes_with_an_overlap_of_zero(program):
    assert "overlap 0: ok" in program


def _child(tmp):
    import contextlib
    import io
    import time
    from test_cli_dropin_cpu import _write_pretrained
    from uav import cli, ops, video_io
    start = time.time()
    dev = torch.device("cuda:0")
    base = _write_pretrained(tmp)
    os.chdir(tmp)

    def write_input(name, frames):
        rgb = scene_ref.scenes_u8([frames], 64, 96)
        video_io.write_y4m(name, *yuv_ref.encode(rgb, "bt601", True), "24", True)
        clip = video_io.preprocess_planes(video_io.read_y4m(name), dev, "auto")
        assert scene_ref.assert_fixture(clip[0].cpu().numpy(), [frames]) == []
        return clip

    clip = write_input("take.y4m", 26)
    write_input("short.y4m", 16)
    common = ["-s", "2", "--pretrained", base, "--device", "cuda:0", "--scenes", "auto", "--scene-max", "8"]
    pipe, _ = cli.load_pipeline(base, device=dev)
    coefs = video_io.yuv_coefficients("bt601", True)
    k = 3
    wa = torch.tensor([(k - j) / (k + 1) for j in range(k)], dtype=torch.float32).to(dev)
    wb = torch.tensor([(j + 1) / (k + 1) for j in range(k)], dtype=torch.float32).to(dev)
    for label, folder, extra, kw in (("cross-fade", "fade", [], {}),
                                     ("cross-fade on tiles", "tiles", ["--perform_tile", "--tile_size", "48"], dict(perform_tile=True, tile_size=48))):
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            assert cli.main(["-i", "take.y4m", "-o", folder, "--scene-overlap", "3"] + extra + common) == 0
        lines = [ln for ln in out.getvalue().splitlines() if ln.startswith("[")]
        assert len(lines) == 1 and ("take: 26 frames 64x96 -> 256x384, 1 tile(s), 3 scene(s) (cuts at 8, 16), 3-frame overlap at 2 split(s), "
                                    in lines[0]), lines
        got = video_io.read_y4m(f"{folder}/video/take_n120_g6_s2.y4m")
        assert got.y.shape == (26, 256, 384) and got.y.std() > 5
        generator = torch.Generator(device=dev).manual_seed(10)
        one, two, three = (video_io.upscale_clip(pipe, clip[:, :, a:b].contiguous(), prompt="best quality, extremely detailed",
                                                 negative_prompt="blur, worst quality", steps=2, guidance_scale=6, noise_level=120,
                                                 generator=generator, **kw) for a, b in ((0, 11), (8, 19), (16, 26)))
        frames = torch.cat([one[:8], ops.frame_axpby_f32(one[8:11], two[:3], wa, wb), two[3:8],
                            ops.frame_axpby_f32(two[8:11], three[:3], wa, wb), three[3:]])
        assert frames.shape[0] == 26
        want = [p.cpu().numpy() for p in video_io.postprocess_planes(frames, coefs)]
        assert all(np.array_equal(g, w) for g, w in zip((got.y, got.cb, got.cr), want)), f"{label}: the file != the composition"
        hard = [p.cpu().numpy() for p in video_io.postprocess_planes(torch.cat([one[8:11], two[8:11]]), coefs)]
        assert not np.array_equal(hard[0], np.concatenate([want[0][8:11], want[0][16:19]]))        # the blend is not a no-op
        del one, two, three, frames
        print(f"{label}: ok at {time.time() - start:.1f} s", flush=True)
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(["-i", "short.y4m", "-o", "zero", "--scene-overlap", "0"] + common) == 0
        assert cli.main(["-i", "short.y4m", "-o", "none"] + common) == 0
    zero = open("zero/video/short_n120_g6_s2.y4m", "rb").read()
    assert zero.count(b"FRAME\n") >= 16 and zero == open("none/video/short_n120_g6_s2.y4m", "rb").read(), "overlap 0 != no option"
    print(f"overlap 0: ok at {time.time() - start:.1f} s", flush=True)


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "upscale-a-video_amd")]
    torch.set_num_threads(min(16, os.cpu_count() or 1))                         # as tests/conftest.py
    _child(sys.argv[1])
