"""The engine's own upscaling program: video files in, 4x video files out (or any size from 1x to 4x), on one MI355X.

    ffmpeg -i in.mp4 in.y4m                                                   # on the user's side: any container -> YUV4MPEG2
    python upscale.py -i in.y4m -o results --pretrained pretrained_models/upscale_a_video
    ffmpeg -i results/video/in_n120_g6_s30.y4m out.mp4

or, with no file in between (`-i -` reads one Y4M stream from standard input, `--y4m-out -` writes it to standard output):

    ffmpeg -i in.mp4 -f yuv4mpegpipe - | python upscale.py -i - --y4m-out - --pretrained DIR | ffmpeg -i - out.mp4

(`python -m uav.cli` with `upscale-a-video_amd` on the path is the same program.) It takes the options of the reference
project's `inference_upscale_a_video.py` and does per video what that program does — `video_io.upscale_clip_chunks` — 3 output
frames at a time: the input is read whole unless `--scenes auto` is given (the DDIM loop needs all of a clip, at 1/16 of the
output's size), the 4x frames go to the file chunk by chunk and never exist as one clip. It reads and writes by itself:
YUV4MPEG2 (`.y4m`, 8-bit 4:2:0 / 4:4:4, progressive), `.npy` arrays of (T,H,W,3) uint8 RGB and directories of images in; `.y4m`
out — `--out-format 420` (8-bit 4:2:0, the default), `444`, `420p10` or `444p10`; the 10-bit formats are made from the fp32
frames with no 8-bit step in between and ffmpeg reads all four through the same pipe —, the colour conversion on the GPU on both
sides (`uav_yuv420_to_clip_f32`, `uav_clip_to_yuv420_u8`, `uav_clip_window_to_yuv`). Input stays 8-bit. `--out-size WxH` (or
`W:H`) or `--out-scale S` (1 to 4) write another size than 4x, from the network's input size up to 4x of it: 480p material at
1080p is `--out-scale 2.25`. Each chunk's fp32 frames are resized on the GPU with an antialiased cubic filter
(`uav_resize_aa_f32`: the filter of `F.interpolate(mode='bicubic', antialias=True)`, after the colour fix and before the colour
conversion), so only frames of the delivery size reach the host; `--matrix auto` goes by the rows written. `--chroma sited`
filters 4:2:0 chroma at the position the tags declare instead of replicating samples on the way in and writing block means on
the way out: bilinear up-sampling at the input tag's siting (`uav_yuv420_sited_to_clip_f32`) and, for the left-sited tags
written (`C420mpeg2`, `C420p10`), a (1,2,1) filter around the even column (`uav_clip_to_yuv420_sited`); the default,
`replicate`, keeps every file's bytes as they were. `--scenes auto` splits a video at its cuts: `uav_clip_scene_stats` makes per
frame a luma histogram and the absolute difference to the frame before on the GPU, `video_io.scene_cuts` decides on the host
(`--scene-threshold MAD:HIST`, `--scene-min N`, `--scene-max N`; the defaults are conventional starting values, NOT validated on
real footage; `--scene-overlap K` runs both sides of a split that `--scene-max` forced over K shared frames and cross-fades them
with `uav_frame_axpby_f32` — a linear dissolve between two independent renderings, which softens detail over K frames and does
not remove their difference, judged on no real footage; detected cuts stay hard), and every scene goes through
`video_io.upscale_clip_chunks` as a clip of its own, one after the other into the one output file, so that no temporal window, attention or flow crosses a cut; a `.y4m` input, file or pipe, is then read 48
frames at a time and only as far as the scene at hand needs (`video_io.Y4MReader`), which bounds the memory by the longest scene
or `--scene-max` instead of the video. Without it (`--scenes off`, the default) the input is read whole and the video is one
clip, byte for byte as before. `-i` may also be a directory whose `.y4m` / `.npy` files and image sub-directories are one video
each. Not there: compressed containers and codecs (use ffmpeg as above) and the LLaVA captioner — `--prompt` takes the caption
text, default none.

`--pretrained DIR` is the released checkpoint layout: vae/{vae_3d,vae_video}{_config.json,.bin},
unet/unet_video{_config.json,.bin}, scheduler/, low_res_scheduler/, text_encoder/, tokenizer/ and, for `-p`,
propagator/raft-things.pth.  There is no random-weight mode: bench.py is the tool for running without checkpoints.
"""
import argparse
import os
import sys
import time
from fractions import Fraction

import torch


PIECE_FRAMES = 48           # `--scenes auto` reads and analyses the input this many frames at a time


class UserError(Exception):
    """A problem with the command line or the files it names: reported as one line, exit status 2."""


def _int_list(text):
    return [int(v) for v in text.split(",") if v.strip() != ""]


def _fps(text):
    try:
        value = Fraction(text.replace(":", "/"))
    except (ValueError, ZeroDivisionError):
        raise argparse.ArgumentTypeError(f"not a frame rate: {text!r} (e.g. 24, 29.97, 30000/1001)") from None
    if value <= 0:
        raise argparse.ArgumentTypeError("the frame rate must be positive")
    return value


def build_parser():
    p = argparse.ArgumentParser(prog="upscale.py", description="Upscale-A-Video on an MI355X: 4x video super-resolution, Y4M in and out.")
    p.add_argument("-i", "--input_path", required=True,
                   help="a .y4m / .npy file, a directory of images, a directory of those, or - for one Y4M stream on standard input")
    p.add_argument("-o", "--output_path", default="./results", help="output folder (videos go to <out>/video)")
    p.add_argument("--pretrained", required=True, metavar="DIR", help="released checkpoint directory (pretrained_models/upscale_a_video)")
    p.add_argument("-n", "--noise_level", type=int, default=120, help="noise level [0, 200] applied to the input video")
    p.add_argument("-g", "--guidance_scale", type=int, default=6, help="classifier-free guidance scale")
    p.add_argument("-s", "--inference_steps", type=int, default=30, help="number of denoising steps")
    p.add_argument("-p", "--propagation_steps", type=_int_list, default=[], help="comma list of steps after which latents are propagated")
    p.add_argument("--prompt", default="", help="caption of the video (there is no captioner); --a_prompt is appended")
    p.add_argument("--a_prompt", default="best quality, extremely detailed")
    p.add_argument("--n_prompt", default="blur, worst quality")
    p.add_argument("--use_video_vae", action="store_true")
    p.add_argument("--color_fix", default="None", choices=["None", "AdaIn", "Wavelet"])
    p.add_argument("--perform_tile", action="store_true")
    p.add_argument("--tile_size", type=int, default=256)
    p.add_argument("--y4m-out", dest="y4m_out", metavar="FILE|-", default=None,
                   help="write the one output video to FILE, or to standard output with - (the per-video line then goes to standard error)")
    p.add_argument("--save_image", action="store_true", help="also write PNG frames to <out>/frame/<name> (needs PIL)")
    p.add_argument("--save_suffix", default="")
    p.add_argument("--matrix", default="auto", choices=["auto", "bt601", "bt709"],
                   help="Y'CbCr matrix; auto = BT.709 from 720 rows up, else BT.601, decided separately for input and output size")
    p.add_argument("--out-format", dest="out_format", default="420", choices=["420", "444", "420p10", "444p10"],
                   help="Y4M output: 8-bit 4:2:0 (default), 8-bit 4:4:4, or 10-bit 4:2:0 / 4:4:4 (16-bit little-endian samples)")
    p.add_argument("--out-size", dest="out_size", metavar="WxH", default=None,
                   help="size of the frames written (also W:H), from the network's input size up to 4x of it; default 4x")
    p.add_argument("--out-scale", dest="out_scale", metavar="S", default=None,
                   help="the same as a factor of the network's input size, 1 to 4 (2.25: 480p -> 1080p); sides are rounded to even")
    p.add_argument("--chroma", default="replicate", choices=["replicate", "sited"],
                   help="4:2:0 chroma: replicate = samples replicated on input, block means on output (default, the files' bytes as "
                        "ever); sited = filtered at the position the Y4M tags declare, on both sides")
    p.add_argument("--scenes", default="off", choices=["off", "auto"],
                   help="auto = find the cuts on the GPU, run every scene as a clip of its own (nothing temporal crosses a cut) and "
                        "read the input only as far as the scene at hand needs; off (default) = the whole video is one clip")
    p.add_argument("--scene-threshold", dest="scene_threshold", metavar="MAD:HIST", default="24:0.30",
                   help="with --scenes auto: a cut needs a mean absolute luma difference >= MAD (8-bit steps) AND a 64-bin histogram "
                        "distance >= HIST (0 to 1) to the frame before; the defaults are conventional starting values and have NOT "
                        "been validated on real footage")
    p.add_argument("--scene-min", dest="scene_min", metavar="N", default="8",
                   help="with --scenes auto: no scene shorter than N frames (default 8, the network's temporal window); the three "
                        "--scene-* values are checked whether or not --scenes auto is given")
    p.add_argument("--scene-max", dest="scene_max", metavar="N", default="0",
                   help="with --scenes auto: split a scene after N frames even without a cut, which bounds the memory; 0 (default) = never")
    p.add_argument("--scene-overlap", dest="scene_overlap", metavar="K", default="0",
                   help="with --scenes auto and --scene-max: run both sides of a forced split over K shared frames and cross-fade them "
                        "(a linear dissolve between two renderings, NOT judged on real footage); at most --scene-min; 0 (default) = "
                        "hard splits, the files' bytes as ever; detected cuts always stay hard")
    p.add_argument("--seed", type=int, default=10)
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--fps", type=_fps, default=None, help="frame rate of the output (default: the input's, 24 when it has none)")
    p.add_argument("--dump-rgb", dest="dump_rgb", metavar="FILE", default=None,
                   help="write the uint8 RGB frames (T,H,W,3) of the last video as .npy (tests, A/B runs)")
    return p


def _out_size_options(args):
    """`--out-size` / `--out-scale` as `video_io.output_size` takes them: ((W, H) or None, S or None)."""
    if args.out_size is not None and args.out_scale is not None:
        raise UserError("--out-size and --out-scale exclude each other")
    size = scale = None
    if args.out_size is not None:
        parts = args.out_size.lower().replace(":", "x").split("x")
        if len(parts) != 2 or not all(v.isascii() and v.isdigit() for v in parts) or not all(int(v) > 0 for v in parts):
            raise UserError(f"--out-size: not a size: {args.out_size!r} (e.g. 1920x1080 or 1920:1080)")
        size = (int(parts[0]), int(parts[1]))
    if args.out_scale is not None:
        try:
            scale = float(args.out_scale)
        except ValueError:
            scale = float("nan")
        if not 1.0 <= scale <= 4.0:
            raise UserError(f"--out-scale: a factor from 1 to 4 expected, got {args.out_scale!r}")
    return size, scale


def _scene_options(args):
    """`--scene-threshold` / `--scene-min` / `--scene-max` / `--scene-overlap` as `video_io.upscale_scenes_chunks` takes them:
    (((MAD, HIST), min, max), overlap)."""
    import math
    parts = args.scene_threshold.split(":")
    try:
        mad, dist = (float(v) for v in parts) if len(parts) == 2 else (math.nan, math.nan)
    except ValueError:
        mad = dist = math.nan
    if not (math.isfinite(mad) and mad >= 0.0 and 0.0 <= dist <= 1.0):
        raise UserError(f"--scene-threshold: MAD:HIST with MAD >= 0 and HIST from 0 to 1 expected (e.g. 24:0.30), got {args.scene_threshold!r}")
    counts = []
    for option, text in (("--scene-min", args.scene_min), ("--scene-max", args.scene_max)):
        if not (text.isascii() and text.isdigit()):
            raise UserError(f"{option}: a number of frames expected, got {text!r}")
        counts.append(int(text))
    if counts[0] < 1:
        raise UserError(f"--scene-min: at least 1 frame expected, got {args.scene_min!r}")
    if 0 < counts[1] < counts[0]:
        raise UserError(f"--scene-max: 0 (never force a split) or at least --scene-min = {counts[0]} expected, got {args.scene_max!r}")
    text = args.scene_overlap
    if not (text.isascii() and text.isdigit()):
        raise UserError(f"--scene-overlap: a number of frames expected, got {text!r}")
    if int(text) > counts[0]:
        raise UserError(f"--scene-overlap: at most --scene-min = {counts[0]} frames expected, got {text!r}")
    return ((mad, dist), counts[0], counts[1]), int(text)


class _Pieces:
    """One video of `--scenes auto`, read as far as it has been asked for: `size` (H, W) of the input, `fps`, `full_range`, and
    `clips(device, matrix, chroma)`, the (1,3,n,h,w) clips of `PIECE_FRAMES` frames each.  A `.y4m` input (file or standard input)
    is a `Y4MReader` whose header and first piece are read here, up front; `.npy` arrays and image directories are read whole,
    as ever, and sliced."""

    def __init__(self, path):
        from . import video_io
        self._reader = self._frames = None
        try:
            if path == "-" or (os.path.isfile(path) and str(path).lower().endswith(".y4m")):
                self._reader = video_io.Y4MReader(sys.stdin.buffer if path == "-" else path)
                self._first = self._reader.read(PIECE_FRAMES)
                self.size, self.fps, self.full_range = self._reader.size, self._reader.fps, self._reader.full_range
            else:
                self._frames, self.fps = video_io.read_frames(path)
                self.size, self.full_range = tuple(int(v) for v in self._frames.shape[1:3]), True
        except (ValueError, OSError) as e:
            raise UserError(str(e)) from None

    def clips(self, device, matrix, chroma):
        from . import video_io
        if self._reader is None:
            for i in range(0, len(self._frames), PIECE_FRAMES):
                frames = torch.from_numpy(self._frames[i:i + PIECE_FRAMES]).permute(0, 3, 1, 2).contiguous()
                yield video_io.preprocess_frames(frames.to(device))
            return
        try:
            piece, self._first = self._first, None
            while piece is not None:
                yield video_io.preprocess_planes(piece, device, matrix, chroma=chroma)
                piece = self._reader.read(PIECE_FRAMES)
        except (ValueError, OSError) as e:
            raise UserError(str(e)) from None
        finally:
            self._reader.close()


def _output_size(source, size, scale, fmt):
    """(H, W) to write for one video read by `_read`; a size outside the video's range is a UserError."""
    from . import video_io
    in_h, in_w = source.size if isinstance(source, (video_io.Y4MClip, _Pieces)) else source.shape[1:3]
    h, w = video_io.pooled_size(int(in_h), int(in_w))
    try:
        return video_io.output_size(4 * h, 4 * w, out_size=size, out_scale=scale, fmt=fmt)
    except ValueError as e:
        raise UserError(f"--out-size: {e}" if size is not None else f"--out-scale: {e}") from None


def _need(path, what):
    if not os.path.exists(path):
        raise UserError(f"{what} not found: {path}")
    return path


def load_pipeline(base, *, use_video_vae=False, with_propagator=False, device="cuda:0"):
    """The released checkpoint directory -> (pipeline, raft or None): VAE fp32 and UNet `.half()` with strict=True, DDIM
    scheduler, then low_res_scheduler / text encoder / tokenizer; RAFT and the propagator only when asked for."""
    from models_video.autoencoder_kl_cond_video import AutoencoderKLVideo
    from models_video.pipeline_upscale_a_video import VideoUpscalePipeline
    from models_video.scheduling_ddim import DDIMScheduler
    from models_video.unet_video import UNetVideoModel
    if not os.path.isdir(base):
        raise UserError(f"--pretrained: {base} is not a directory")
    name = "vae_video" if use_video_vae else "vae_3d"
    vae = AutoencoderKLVideo.from_config(_need(os.path.join(base, "vae", name + "_config.json"), "VAE config"))
    vae.load_state_dict(torch.load(_need(os.path.join(base, "vae", name + ".bin"), "VAE weights"), map_location="cpu"), strict=True)
    unet = UNetVideoModel.from_config(_need(os.path.join(base, "unet", "unet_video_config.json"), "UNet config"))
    unet.load_state_dict(torch.load(_need(os.path.join(base, "unet", "unet_video.bin"), "UNet weights"), map_location="cpu"), strict=True)
    unet = unet.half().eval()
    scheduler = DDIMScheduler.from_config(_need(os.path.join(base, "scheduler", "scheduler_config.json"), "scheduler config"))
    for sub in ("low_res_scheduler", "text_encoder", "tokenizer"):
        _need(os.path.join(base, sub), f"{sub}/")
    pipeline = VideoUpscalePipeline.from_pretrained(base, torch_dtype=torch.float16)
    pipeline.vae, pipeline.unet, pipeline.scheduler = vae, unet, scheduler
    raft = propagator = None
    if with_propagator:
        from models_video.RAFT.raft_bi import RAFT_bi
        from models_video.propagation_module import Propagation
        raft = RAFT_bi(_need(os.path.join(base, "propagator", "raft-things.pth"), "RAFT weights (needed by -p)"), device=device)
        propagator = Propagation(4, learnable=False)
    pipeline.propagator = propagator
    return pipeline.to(device), raft


def list_videos(path):
    """`-i`: one file, one directory of images, or a directory whose .y4m / .npy files and image sub-directories are one
    video each (sorted by name)."""
    from .video_io import IMAGE_EXTENSIONS
    if os.path.isfile(path):
        return [path]
    if not os.path.isdir(path):
        raise UserError(f"input not found: {path}")
    videos = []
    for n in sorted(os.listdir(path)):
        full = os.path.join(path, n)
        if os.path.isfile(full) and n.lower().endswith((".y4m", ".npy")):
            videos.append(full)
        elif os.path.isdir(full) and any(m.lower().endswith(IMAGE_EXTENSIONS) for m in os.listdir(full)):
            videos.append(full)
    if not videos and any(n.lower().endswith(IMAGE_EXTENSIONS) for n in os.listdir(path)):
        return [path]
    if not videos:
        raise UserError(f"no .y4m / .npy files or image directories in {path}")
    return videos


def _save_png(frames_u8, folder, first=0):
    try:
        from PIL import Image
    except ImportError:
        raise UserError("--save_image needs the PIL package (Pillow)") from None
    os.makedirs(folder, exist_ok=True)
    for i, frame in enumerate(frames_u8, first):
        Image.fromarray(frame).save(os.path.join(folder, f"{i:04d}.png"))


def _read(path):
    from . import video_io
    try:
        if path == "-":
            clip = video_io.read_y4m(sys.stdin.buffer)
            return clip, clip.fps
        return video_io.read_frames(path)
    except (ValueError, OSError) as e:
        raise UserError(str(e)) from None


def run(args):
    from . import tiling, video_io
    size, scale = _out_size_options(args)
    scene, overlap = _scene_options(args)
    auto = args.scenes == "auto"
    videos = ["-"] if args.input_path == "-" else list_videos(args.input_path)
    if args.y4m_out is not None and len(videos) > 1:
        raise UserError(f"--y4m-out takes one video, {args.input_path} holds {len(videos)}")
    device = torch.device(args.device)
    if device.type == "cuda" and not torch.cuda.is_available():
        raise UserError(f"--device {args.device}: no GPU is visible")
    first = (_Pieces(videos[0]), None) if auto else _read(videos[0])                # before the checkpoints are loaded: an unreadable input fails at once
    fmt = video_io.out_format(args.out_format)
    _output_size(first[0], size, scale, fmt)                # ... and so does a size the first video cannot have
    pipeline, raft = load_pipeline(args.pretrained, use_video_vae=args.use_video_vae, with_propagator=bool(args.propagation_steps),
                                   device=device)
    prompt = args.prompt + args.a_prompt
    out_path = None
    for index, path in enumerate(videos):
        source, fps = first if index == 0 else ((_Pieces(path), None) if auto else _read(path))
        first = None
        out_h, out_w = _output_size(source, size, scale, fmt)
        name = "stdin" if path == "-" else os.path.splitext(os.path.basename(os.path.normpath(path)))[0]
        if auto:
            clip, fps, in_size = None, source.fps, source.size
        elif isinstance(source, video_io.Y4MClip):
            clip = video_io.preprocess_planes(source, device, args.matrix, chroma=args.chroma)
            in_size = source.size
        else:
            frames = torch.from_numpy(source).permute(0, 3, 1, 2).contiguous()
            clip = video_io.preprocess_frames(frames.to(device))
            in_size = tuple(source.shape[1:3])
        t, (h, w) = (None, video_io.pooled_size(*in_size)) if auto else (clip.shape[2], clip.shape[-2:])
        tiles = len(tiling.tile_grid(h, w, args.tile_size)) if tiling.needs_tiling(h, w, args.perform_tile) else 1
        generator = torch.Generator(device=device).manual_seed(args.seed)
        full_range = source.full_range if isinstance(source, (video_io.Y4MClip, _Pieces)) else True
        coefs = video_io.yuv_coefficients(video_io.auto_matrix(out_h) if args.matrix == "auto" else args.matrix, full_range,
                                          depth=fmt.depth)
        prop = "_p" + "_".join(map(str, args.propagation_steps)) if args.propagation_steps else ""
        suffix = "_" + args.save_suffix if args.save_suffix else ""
        save_name = f"{name}_n{args.noise_level}_g{args.guidance_scale}_s{args.inference_steps}{prop}{suffix}"
        if args.y4m_out is None:
            os.makedirs(os.path.join(args.output_path, "video"), exist_ok=True)
            out_path = os.path.join(args.output_path, "video", save_name + ".y4m")
        else:
            out_path = args.y4m_out
        dump = [] if args.dump_rgb and index == len(videos) - 1 else None
        need_frames = args.save_image or dump is not None       # the uint8 RGB frames are made from the fp32 chunk, like the planes
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        start = time.time()
        options = dict(prompt=prompt, negative_prompt=args.n_prompt, raft=raft, propagation_steps=args.propagation_steps,
                       steps=args.inference_steps, guidance_scale=args.guidance_scale, noise_level=args.noise_level,
                       tile_size=args.tile_size, perform_tile=args.perform_tile, color_fix=args.color_fix, generator=generator,
                       coefs=None if need_frames else coefs, fmt=fmt,
                       out_size=None if (out_h, out_w) == (4 * h, 4 * w) else (out_h, out_w), chroma=args.chroma)
        if auto:        # scene by scene, the input read piece by piece as the scenes need it
            chunks = video_io.upscale_scenes_chunks(pipeline, source.clips(device, args.matrix, args.chroma), scene=scene, overlap=overlap,
                                                    **options)
        else:
            chunks = video_io.upscale_clip_chunks(pipeline, clip, **options)
        with video_io.Y4MWriter(sys.stdout.buffer if out_path == "-" else out_path, out_w, out_h, args.fps or fps or 24, full_range,
                                fmt) as out:
            for chunk in chunks:                                # one chunk is alive: decoded, converted and written before the next
                if need_frames:
                    rgb = video_io.postprocess_frames(chunk).cpu().numpy()
                    if args.save_image:
                        _save_png(rgb, os.path.join(args.output_path, "frame", save_name), first=out.frames)
                    if dump is not None:
                        dump.append(rgb)
                    chunk = video_io.postprocess_planes(chunk, coefs, fmt, video_io.output_siting(fmt, full_range, args.chroma))
                out.write(*chunk)
                del chunk                                       # before the generator decodes the next one
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        seconds = time.time() - start
        if dump is not None:
            import numpy as np
            with open(args.dump_rgb, "wb") as fh:
                np.save(fh, np.concatenate(dump))
        scenes = ""
        if auto:
            t, starts = chunks.frames, [a for a, _ in chunks.scenes[1:]]
            scenes = f", {len(chunks.scenes)} scene(s)"
            if starts:
                scenes += " (cuts at " + ", ".join(map(str, starts[:12])) + (", …" if len(starts) > 12 else "") + ")"
            if chunks.seams:
                scenes += f", {overlap}-frame overlap at {len(chunks.seams)} split(s)"
        print(f"[{index + 1}/{len(videos)}] {name}: {t} frames {in_size[0]}x{in_size[1]} -> {out_h}x{out_w}, {tiles} tile(s){scenes}, "
              f"{seconds:.2f} s -> {out_path}", file=sys.stderr if out_path == "-" else sys.stdout, flush=True)
    return out_path


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    try:
        run(args)
    except UserError as e:
        print(f"upscale.py: error: {e}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
