"""Same-process timing of the siting-aware 4:2:0 kernels of the Y4M front end (csrc/yuv_io.hip K13, `--chroma sited`) against the
kernels they stand beside, in the style of tools/bench_out_format.py.  The algorithmic bytes of each pair are equal:
  decode, planes (8,H,W) for 320x320 and 1280x1280:   uav_yuv420_sited_to_clip_f32  vs  uav_yuv420_to_clip_f32   (1.5 B read + 12 B written per pixel)
  encode 8-bit, frames (8,3,1280,1280):               uav_clip_to_yuv420_sited (8)  vs  uav_clip_to_yuv420_u8    (12 + 1.5)
  encode 8-bit, frames (8,3,1280,1284), W % 8 == 4:   the same pair in the half-width mode (4-byte luma, 2-byte chroma stores)
  encode 10-bit, the same frames:                     uav_clip_to_yuv420_sited (10) vs  uav_clip_window_to_yuv 420p10 on contiguous frames (12 + 3)
Per kernel: ROUNDS rounds, interleaved between all kernels, of 20 warm launches between two HIP events; the launches rotate over NBUF
input tensors (4 x 157 MB of frames, more than the 256 MiB Infinity Cache; the 1280x1280 decoder writes 4 x 157 MB); the encoders'
planes are allocated once for both sides of a pair.  One JSON line per kernel: median and min of the rounds' mean launch time in us,
GB/s of the algorithmic bytes at the median, that figure as a fraction of its yardstick's, and the min-vs-median spread.
With --end-to-end: the tests' tiny seeded checkpoints and a 12-frame 68x160 `C420mpeg2` clip are written to a temporary directory and
the program runs `--perform_tile --tile_size 64` with `--chroma replicate` and `sited`, twice each, a fresh process per run.
usage: python tools/bench_chroma_sited.py [--out FILE] [--end-to-end [--steps N]]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "upscale-a-video_amd"))
from uav import ops, video_io  # noqa: E402

LAUNCHES, ROUNDS, NBUF = 20, 7, 4


def time_round(fn, bufs):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(LAUNCHES):
        fn(bufs[i % len(bufs)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / LAUNCHES                                 # us per launch


def end_to_end(steps):
    """Per-video seconds of `upscale.py` on one tiled job per chroma mode, a fresh process each (the first run of all also warms the box)."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
    import yuv_ref
    from test_cli_dropin_cpu import _clip_u8, _write_pretrained
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        base = _write_pretrained(tmp)
        clip = os.path.join(tmp, "tiled12.y4m")
        rgb = _clip_u8(12, 68, 160, 42).permute(0, 2, 3, 1).contiguous().numpy()
        video_io.write_y4m(clip, *yuv_ref.encode(rgb, "bt601", False), 24, False)
        for mode in ("replicate", "sited", "replicate", "sited"):
            start = time.time()
            r = subprocess.run([sys.executable, os.path.join(ROOT, "upscale.py"), "-i", clip, "-o", os.path.join(tmp, mode), "-s", str(steps),
                                "--pretrained", base, "--perform_tile", "--tile_size", "64", "--chroma", mode],
                               capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-3000:]
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("[1/1]")][0]
            out.setdefault(mode, []).append(dict(wall_s=round(time.time() - start, 2), video_s=float(line.split(" s -> ")[0].split()[-1])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--end-to-end", dest="end_to_end", action="store_true")
    ap.add_argument("--steps", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    t, h, w = 8, 1280, 1280
    k8, k10 = video_io.yuv_coefficients("bt709", False), video_io.yuv_coefficients("bt709", False, depth=10)
    frames = [(torch.randn(t, 3, h, w, generator=g) * 0.8).to(dev) for _ in range(NBUF)]
    p10 = video_io._new_planes(frames[0], t, h, w, video_io.OUT_FORMATS["420p10"])
    # (pair, kernel, role, shape, fn, buffers, bytes per pixel)
    cases = [("encode8", "uav_clip_to_yuv420_u8", "yardstick", (t, 3, h, w), lambda f: ops.clip_to_yuv420_u8(f, k8), frames, 13.5),
             ("encode8", "uav_clip_to_yuv420_sited", "sited", (t, 3, h, w), lambda f: ops.clip_to_yuv420_sited(f, k8, 8), frames, 13.5),
             ("encode10", "uav_clip_window_to_yuv", "yardstick", (t, 3, h, w),
              lambda f: ops.clip_window_to_yuv(f, *p10, k10, chroma444=False, depth=10, frames_first=True), frames, 15.0),
             ("encode10", "uav_clip_to_yuv420_sited", "sited", (t, 3, h, w), lambda f: ops.clip_to_yuv420_sited(f, k10, 10), frames, 15.0)]
    # W % 8 == 4: the half-width mode (4-byte luma and 2-byte chroma stores), which no 1280-wide frame takes
    w4 = w + 4
    frames4 = [(torch.randn(t, 3, h, w4, generator=g) * 0.8).to(dev) for _ in range(NBUF)]
    cases += [("encode8_w1284", "uav_clip_to_yuv420_u8", "yardstick", (t, 3, h, w4), lambda f: ops.clip_to_yuv420_u8(f, k8), frames4, 13.5),
              ("encode8_w1284", "uav_clip_to_yuv420_sited", "sited", (t, 3, h, w4), lambda f: ops.clip_to_yuv420_sited(f, k8, 8), frames4, 13.5)]
    for side in (320, 1280):
        planes = [tuple(torch.randint(0, 256, s, generator=g, dtype=torch.uint8).to(dev)
                        for s in ((t, side, side), (t, side // 2, side // 2), (t, side // 2, side // 2))) for _ in range(NBUF)]
        cases += [(f"decode{side}", "uav_yuv420_to_clip_f32", "yardstick", (t, side, side), lambda p: ops.yuv420_to_clip_f32(*p, k8), planes, 13.5),
                  (f"decode{side}", "uav_yuv420_sited_to_clip_f32", "sited", (t, side, side),
                   lambda p: ops.yuv420_sited_to_clip_f32(*p, k8, (False, True)), planes, 13.5)]
    for *_, fn, bufs, _ in cases:                                               # warm-up: code objects, allocator
        for b in bufs:
            fn(b)
    torch.cuda.synchronize()
    times = [[] for _ in cases]
    for _ in range(ROUNDS):
        for k, (*_, fn, bufs, _) in enumerate(cases):
            times[k].append(time_round(fn, bufs))
    lines, yard = [], {}
    for (pair, kernel, role, shape, _, _, per_pixel), ts in zip(cases, times):
        med, best = statistics.median(ts), min(ts)
        gbps = per_pixel * shape[0] * shape[-2] * shape[-1] / med / 1e3
        if role == "yardstick":
            yard[pair] = gbps
        lines.append(json.dumps(dict(pair=pair, kernel=kernel, role=role, shape=list(shape), launches_per_round=LAUNCHES, rounds=ROUNDS,
                                     input_buffers=NBUF, us_median=round(med, 2), us_min=round(best, 2), bytes_per_pixel=per_pixel,
                                     gbps_at_median=round(gbps, 1), gbps_vs_yardstick=round(gbps / yard[pair], 3),
                                     spread_min_vs_median=round(1 - best / med, 3), device=torch.cuda.get_device_name(0))))
    del frames, frames4, cases, p10
    torch.cuda.empty_cache()
    if args.end_to_end:
        for mode, runs in end_to_end(args.steps).items():
            lines.append(json.dumps(dict(end_to_end="upscale.py --perform_tile --tile_size 64", clip="12 frames 68x160 C420mpeg2", steps=args.steps,
                                         out_format="420", chroma=mode, runs=runs)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
