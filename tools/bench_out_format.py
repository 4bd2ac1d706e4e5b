"""Same-process timing of the output-format kernels of the Y4M front end (csrc/yuv_io.hip K13, `uav_clip_window_to_yuv`) against the
8-bit 4:2:0 kernel they stand beside, in the style of tools/bench_yuv_io.py.
  frames (8,3,1280,1280) fp32, 12 B read per pixel; written per pixel: uav_clip_to_yuv420_u8 1.5 B (the yardstick), the window
  kernel for 420 1.5 B, 444 3 B, 420p10 3 B, 444p10 6 B.
Per kernel: ROUNDS rounds, interleaved between the kernels, of 20 warm launches between two HIP events; the launches rotate over NBUF
input tensors (4 x 157 MB, more than the 256 MiB Infinity Cache) so that every launch reads from HBM; the planes are allocated once.
One JSON line per kernel: median and min of the rounds' mean launch time in us, GB/s of the algorithmic bytes at the median, and that
figure as a fraction of the yardstick's.  With --pretrained DIR (the tiny seeded checkpoints of the tests will do) and --clip FILE.y4m:
one end-to-end pair, the wall time of the same job of the program with `--out-format 420` and with `444p10`, each in a fresh process.
usage: python tools/bench_out_format.py [--out FILE] [--pretrained DIR --clip FILE.y4m [--steps N]]"""
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


def end_to_end(pretrained, clip, steps):
    """Wall time of `upscale.py` on `clip` per format, a fresh process each (checkpoint loading and warm-up included in both)."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for fmt in ("420", "444p10", "420", "444p10"):
            start = time.time()
            r = subprocess.run([sys.executable, os.path.join(ROOT, "upscale.py"), "-i", clip, "-o", os.path.join(tmp, fmt), "-s", str(steps),
                                "--pretrained", pretrained, "--out-format", fmt], capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-3000:]
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("[1/1]")][0]
            out.setdefault(fmt, []).append(dict(wall_s=round(time.time() - start, 2), video_s=float(line.split(" s -> ")[0].split()[-1])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pretrained", default=None)
    ap.add_argument("--clip", default=None)
    ap.add_argument("--steps", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    t, h, w = 8, 1280, 1280
    frames = [(torch.randn(t, 3, h, w, generator=g) * 0.8).to(dev) for _ in range(NBUF)]
    cases = [("uav_clip_to_yuv420_u8", "420", lambda f, k=video_io.yuv_coefficients("bt709", True): ops.clip_to_yuv420_u8(f, k), 13.5)]
    for name, extra in (("420", 1.5), ("444", 3.0), ("420p10", 3.0), ("444p10", 6.0)):
        fmt = video_io.OUT_FORMATS[name]
        coefs = video_io.yuv_coefficients("bt709", True, depth=fmt.depth)
        planes = video_io._new_planes(frames[0], t, h, w, fmt)

        def run(f, fmt=fmt, coefs=coefs, planes=planes):
            ops.clip_window_to_yuv(f, *planes, coefs, chroma444=fmt.chroma444, depth=fmt.depth, frames_first=True)
        cases.append(("uav_clip_window_to_yuv", name, run, 12.0 + extra))
    for _, _, fn, _ in cases:                                                   # warm-up: code objects, allocator
        for b in frames:
            fn(b)
    torch.cuda.synchronize()
    times = [[] for _ in cases]
    for _ in range(ROUNDS):
        for k, (_, _, fn, _) in enumerate(cases):
            times[k].append(time_round(fn, frames))
    lines, yard = [], None
    for (kernel, fmt, _, per_pixel), ts in zip(cases, times):
        med, best, nbytes = statistics.median(ts), min(ts), per_pixel * t * h * w
        gbps = nbytes / med / 1e3
        yard = yard or gbps
        lines.append(json.dumps(dict(kernel=kernel, format=fmt, shape=[t, 3, h, w], launches_per_round=LAUNCHES, rounds=ROUNDS,
                                     input_buffers=NBUF, us_median=round(med, 2), us_min=round(best, 2), bytes_per_pixel=per_pixel,
                                     gbps_at_median=round(gbps, 1), gbps_vs_yardstick=round(gbps / yard, 3),
                                     spread_min_vs_median=round(1 - best / med, 3), device=torch.cuda.get_device_name(0))))
    del frames, cases
    torch.cuda.empty_cache()
    if args.pretrained and args.clip:
        for fmt, runs in end_to_end(args.pretrained, args.clip, args.steps).items():
            lines.append(json.dumps(dict(end_to_end="upscale.py", clip=os.path.basename(args.clip), steps=args.steps, format=fmt, runs=runs)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
