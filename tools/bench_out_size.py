"""Same-process timing of the antialiased resize behind `--out-size` / `--out-scale` (csrc/resize_aa.hip, `uav_resize_aa_f32`) against
the colour-conversion kernel it stands in front of, in the style of tools/bench_out_format.py.
  uav_resize_aa_f32 on one chunk of the program, (3*3, 1280, 1280) -> 720 x 720 and (3*3, 2160, 3840) -> (1080, 1920); algorithmic
  bytes per plane 4 * (hi*wi + 2*hi*wo + ho*wo): the source read, the intermediate written and read, the result written (the tap
  tables and the set-up launch are inside the timed call and outside the bytes).
  uav_clip_to_yuv420_u8 on (8,3,1280,1280), 13.5 B per pixel: the yardstick of profiles/out_format_kernels.txt.
Per case: ROUNDS rounds, interleaved between the cases, of LAUNCHES warm calls between two HIP events; the calls rotate over input
tensors that together exceed the 256 MiB Infinity Cache, so that every call reads its source from HBM (the resize's intermediate,
37 MB and 149 MB, is written and read back inside one call and may stay in that cache: that is how the program runs it too).
One JSON line per case: median and min of the rounds' mean call time in us, GB/s of the algorithmic bytes at the median, and that
figure as a fraction of the yardstick's.  Then the worst absolute error of the kernel on the shapes of tests/test_out_size_gpu.py
against the float64 reference.  With --pretrained DIR (the tiny seeded checkpoints of the tests will do) and --clip FILE.y4m: the
program's own per-video seconds on that clip without a size option and with `--out-size WxH` (--size), a fresh process each.
usage: python tools/bench_out_size.py [--out FILE] [--pretrained DIR --clip FILE.y4m --size WxH [--steps N]]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from uav import ops, video_io  # noqa: E402

LAUNCHES, ROUNDS = 20, 7
RESIZES = (((9, 1280, 1280), (720, 720), 6), ((9, 2160, 3840), (1080, 1920), 2))       # source, result, rotating source tensors


def time_round(fn, bufs):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(LAUNCHES):
        fn(bufs[i % len(bufs)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / LAUNCHES                                 # us per call


def kernel_error(dev):
    """Worst max-abs error of the kernel over the shapes of the GPU test (tests/resize_aa_ref.py SHAPES), against that reference."""
    from resize_aa_ref import SHAPES, case as _case
    worst = (0.0, None)
    for shape, planes in SHAPES:
        x, ref = _case(shape, planes)
        got = ops.resize_aa_f32(x.to(dev), *shape[2:]).cpu().numpy()
        err = float(abs(got - ref).max())
        if err > worst[0]:
            worst = (err, list(shape))
    return dict(kernel="uav_resize_aa_f32", worst_abs_error=worst[0], at_shape=worst[1], shapes=len(SHAPES), reference="tests/resize_aa_ref.py (float64)")


def end_to_end(pretrained, clip, size, steps):
    """The program's per-video seconds on `clip` without and with `--out-size`, a fresh process each, alternating."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, extra in enumerate(([], ["--out-size", size], [], ["--out-size", size])):
            start = time.time()
            r = subprocess.run([sys.executable, os.path.join(ROOT, "upscale.py"), "-i", clip, "-o", os.path.join(tmp, str(k)), "-s", str(steps),
                                "--pretrained", pretrained] + extra, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-3000:]
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("[1/1]")][0]
            out.setdefault(" ".join(extra) or "4x", []).append(dict(wall_s=round(time.time() - start, 2), video_s=float(line.split(" s -> ")[0].split()[-1]),
                                                                    frames=line.split(": ")[1].split(",")[0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pretrained", default=None)
    ap.add_argument("--clip", default=None)
    ap.add_argument("--size", default=None)
    ap.add_argument("--steps", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    lines = []

    def measure(cases):
        """cases: (dict describing the case, fn, buffers, algorithmic bytes per call) -> [(dict, GB/s at the median)]"""
        for _, fn, bufs, _ in cases:                                            # warm-up: code objects, allocator
            for b in bufs:
                fn(b)
        torch.cuda.synchronize()
        times = [[] for _ in cases]
        for _ in range(ROUNDS):
            for k, (_, fn, bufs, _) in enumerate(cases):
                times[k].append(time_round(fn, bufs))
        out = []
        for (what, _, bufs, nbytes), ts in zip(cases, times):
            med, best = statistics.median(ts), min(ts)
            out.append((dict(what, launches_per_round=LAUNCHES, rounds=ROUNDS, input_buffers=len(bufs), us_median=round(med, 2), us_min=round(best, 2),
                             algorithmic_mb=round(nbytes / 1e6, 1), gbps_at_median=round(nbytes / med / 1e3, 1),
                             spread_min_vs_median=round(1 - best / med, 3)), nbytes / med / 1e3))
        return out

    t, h, w = 8, 1280, 1280
    frames = [(torch.randn(t, 3, h, w, generator=g) * 0.8).to(dev) for _ in range(4)]
    coefs = video_io.yuv_coefficients("bt709", True)
    yard_case = (dict(kernel="uav_clip_to_yuv420_u8", shape=[t, 3, h, w]), lambda f: ops.clip_to_yuv420_u8(f, coefs), frames, 13.5 * t * h * w)
    # the yardstick is timed in the same rounds as each resize (one resize shape at a time: the sources of both do not fit together)
    for (planes, hi, wi), (ho, wo), nbuf in RESIZES:
        srcs = [(torch.randn(planes, hi, wi, generator=g) * 0.8).to(dev) for _ in range(nbuf)]
        nbytes = 4 * planes * (hi * wi + 2 * hi * wo + ho * wo)
        case = (dict(kernel="uav_resize_aa_f32", shape=[planes, hi, wi], result=[ho, wo]), lambda s, ho=ho, wo=wo: ops.resize_aa_f32(s, ho, wo), srcs, nbytes)
        (yard, yard_gbps), (mine, gbps) = measure([yard_case, case])
        mine["gbps_vs_yardstick"] = round(gbps / yard_gbps, 3)
        lines += [json.dumps(dict(yard, device=torch.cuda.get_device_name(0))), json.dumps(dict(mine, device=torch.cuda.get_device_name(0)))]
        del srcs, case
        torch.cuda.empty_cache()
    del frames, yard_case
    torch.cuda.empty_cache()
    lines.append(json.dumps(kernel_error(dev)))
    if args.pretrained and args.clip and args.size:
        for opt, runs in end_to_end(args.pretrained, args.clip, args.size, args.steps).items():
            lines.append(json.dumps(dict(end_to_end="upscale.py", clip=os.path.basename(args.clip), steps=args.steps, option=opt, runs=runs)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
