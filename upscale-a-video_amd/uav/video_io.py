"""Frame I/O around `pipeline(...)`: the device-side conversions, a YUV4MPEG2 reader / writer and the
per-video body of the upscaling program (`uav/cli.py`).

Two kernel passes mirror what the reference CLI does with chains of eager tensor ops over the whole clip
(`inference_upscale_a_video.py:180-187,357-359`; 4K output: 5 passes over 3.2 GB):

    clip = preprocess_frames(frames)        # (T,C,H,W) 0..255 -> (1,C,T,h,w) fp32 in [-1,1], >= 1280-px inputs area-pooled /4
    video = postprocess_frames(output)      # (T,C,H,W) in [-1,1] -> (T,H,W,C) uint8, ready for imageio.mimwrite

and two more take the place of a decoder / encoder's colour conversion for the one container the engine reads and writes
itself, YUV4MPEG2 (`.y4m`: uncompressed planar Y'CbCr, what `ffmpeg -i in.mp4 in.y4m` / `ffmpeg -i out.y4m out.mp4`
produce and eat), in 16.16 fixed point so that every byte is defined (csrc/yuv_io.hip, K13):

    clip = preprocess_planes(read_y4m(path), device)        # planes -> (1,3,T,h,w), same normalisation and pooling
    y, cb, cr = postprocess_planes(output, coefs)           # (T,3,H,W) in [-1,1] -> 4:2:0 planes; write_y4m(path, y, cb, cr, ...)

Input is 8-bit (4:2:0 or 4:4:4).  Output is one of `OUT_FORMATS`: '420' (8-bit 4:2:0, the default), '444', '420p10', '444p10' —
the 10-bit ones from 12-bit RGB with no 8-bit intermediate, 16-bit little-endian samples in the file (`uav_clip_window_to_yuv`).

Output size: the network's result is 4x its input; `output_size` turns the program's `--out-size WxH` / `--out-scale S` into any
(H, W) between 1x and 4x, and `upscale_clip_chunks(..., out_size=(H, W))` resizes every chunk's fp32 frames on the device with the
antialiased cubic filter of `ops.resize_aa_f32` (csrc/resize_aa.hip) before they are converted, so nothing larger than the
delivery size crosses to the host.

Chroma siting: by default (`chroma="replicate"`) a 4:2:0 chroma sample is replicated over its 2x2 block on the way in and is the
block's mean on the way out, whatever the tag says — the bytes of the program's files are pinned by tests, so that stays the
default.  `chroma="sited"` (`--chroma sited`) filters at the position the tags declare: bilinear up-sampling at `chroma_siting(tag)`
on the way in (`uav_yuv420_sited_to_clip_f32`) and, for the left-sited tags written (`C420mpeg2`, `C420p10`), the (1,2,1) filter
around the even column on the way out (`uav_clip_to_yuv420_sited`).

Scenes (`--scenes auto`): `upscale_scenes_chunks` takes a video as an iterator of pieces — `Y4MReader` reads a `.y4m` file or
pipe that way, with `read_y4m`'s header parser and refusals —, gets each piece's integer statistics from `ops.clip_scene_stats`
(per frame a 64-bin luma histogram and the sum of absolute luma differences to the frame before, csrc/scene_stats.hip), lets
`SceneCutter`, the streaming form of the pure function `scene_cuts`, find the cuts, and runs `upscale_clip_chunks` on every
scene as a clip of its own with one shared generator; nothing temporal crosses a cut and no more input is held than the open
scene needs. The detector's defaults (`SCENE_THRESHOLD`, `SCENE_MIN_LEN`) are conventional starting values that have not been
validated on real footage. Without it a video is one clip and is read whole.  `overlap=K` (`--scene-overlap`) cross-fades the
splits that `max_len` forces in the middle of a shot: the scene before such a split runs K frames on, those K fp32 frames are
held at the delivery size and blended with the next scene's first K by `ops.frame_axpby_f32` (csrc/frame_axpby.hip, every bit
defined); detected cuts stay hard.  A linear dissolve between two independent renderings: it softens detail over K frames and
does not remove their difference, and nobody has judged it on real footage.

Compressed containers and codecs are not read or written, and there is no captioner (the reference's LLaVA step).
"""
import os
from collections import namedtuple
from fractions import Fraction

import torch

from . import engine as E
from . import ops

# integer colour-conversion table: `forward` = fy[3], fcb[3], fcr[3], yo (RGB -> Y'CbCr), `inverse` = yo, iy, rcr, gcb, gcr, bcb
YuvCoefs = namedtuple("YuvCoefs", "matrix full_range forward inverse")
# a decoded .y4m file: uint8 numpy planes y (T,H,W), cb / cr (T,ceil(H/2),ceil(W/2)) [colorspace 'C444': (T,H,W)], fps a Fraction
# or None, size (H, W), the file's colour-space tag ('' when it has none) and its range
Y4MClip = namedtuple("Y4MClip", "y cb cr fps size colorspace full_range")
# an output format: its name, chroma layout, bits per sample, the Y4M `C` tag (None: 'C420jpeg' / 'C420mpeg2' by range, as ever)
# and the bytes of one sample in the file
OutFormat = namedtuple("OutFormat", "name chroma444 depth tag sample_bytes")
OUT_FORMATS = {f.name: f for f in (OutFormat("420", False, 8, None, 1), OutFormat("444", True, 8, "C444", 1),
                                   OutFormat("420p10", False, 10, "C420p10", 2), OutFormat("444p10", True, 10, "C444p10", 2))}


class YuvCoefs10(YuvCoefs):
    """The forward table of the 10-bit formats, same layout as the 8-bit one (`inverse` is None: input is 8-bit)."""
    __slots__ = ()
    depth = 10


def out_format(fmt) -> OutFormat:
    if isinstance(fmt, OutFormat):
        return fmt
    if fmt not in OUT_FORMATS:
        raise ValueError(f"output format must be one of {sorted(OUT_FORMATS)}, got {fmt!r}")
    return OUT_FORMATS[fmt]


def _plane_dtype(fmt: OutFormat):
    return torch.uint8 if fmt.depth == 8 else torch.int16     # 0..1023 fit; the writer reinterprets them as unsigned

_KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
_CHROMA_420 = ("C420jpeg", "C420mpeg2", "C420paldv", "C420")
CHROMA_MODES = ("replicate", "sited")
# (centre_h, centre_v) per 4:2:0 tag: True when the chroma sample lies between its two luma samples on that axis, False when it
# lies on the even one.  'C420paldv' is top-left, as ffmpeg maps it; 'C420p10' is what this program writes for 10 bits.
_SITING = {"C420jpeg": (True, True), "C420mpeg2": (False, True), "C420": (False, True), "": (False, True), "C420p10": (False, True),
           "C420paldv": (False, False)}
IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".webp")


def preprocess_frames(frames: torch.Tensor) -> torch.Tensor:
    """`vframes = (vframes/255. - 0.5) * 2`; `if h >= 1280 and w >= 1280: F.interpolate(vframes, (h//4, w//4), mode='area')`;
    `unsqueeze(0)` + `rearrange('b t c h w -> b c t h w')` (inference_upscale_a_video.py:180-187)."""
    with E.device_guard(frames):
        clip = ops.frames_to_clip_f32(frames.contiguous())                      # (C,T,H,W)
        return _pool_large(clip).unsqueeze(0)


def pooled_size(h: int, w: int):
    """The size the network sees for frames of h x w: those of 1280 pixels and more on both sides are area-pooled by 4."""
    return (h // 4, w // 4) if h >= 1280 and w >= 1280 else (h, w)


def _pool_large(clip):
    h, w = (int(v) for v in clip.shape[-2:])
    if pooled_size(h, w) != (h, w):
        clip = ops.resize_area_f32(clip, *pooled_size(h, w))
    return clip


def postprocess_frames(output: torch.Tensor) -> torch.Tensor:
    """`(output / 2 + 0.5).clamp(0, 1) * 255`, `rearrange('t c h w -> t h w c')`, `.astype(np.uint8)` (:357-359); the result
    stays on the device — `.cpu().numpy()` is the caller's (one 1-byte-per-value copy instead of an fp32 one)."""
    with E.device_guard(output):
        return ops.clip_to_frames_u8(output.float().contiguous())


# ------------------------------------------------------------------------------------------------
# Y'CbCr: integer coefficients, the two device passes
def yuv_coefficients(matrix: str, full_range: bool, depth: int = 8) -> YuvCoefs:
    """16.16 fixed-point tables of both directions for `matrix` in 'bt601' / 'bt709'.  With Kg = 1-Kr-Kb and (ys, yo, cs) =
    (255, 0, 255) for full range, (219, 16, 224) for limited range, every entry is round(x * 65536) of the textbook value.
    `depth=10`: the forward table only (a `YuvCoefs10`), from 12-bit RGB to 10-bit samples — (ys, yo, cs) = (1023, 0, 1023) for
    full range, (876, 64, 896) for limited range, entries round(x * s / 4095 * 65536); same layout fy[3], fcb[3], fcr[3], yo."""
    if matrix not in _KR_KB:
        raise ValueError(f"matrix must be one of {sorted(_KR_KB)}, got {matrix!r}")
    if depth not in (8, 10):
        raise ValueError(f"depth must be 8 or 10, got {depth!r}")
    kr, kb = _KR_KB[matrix]
    kg = 1.0 - kr - kb
    if depth == 10:
        ys, yo, cs = (1023, 0, 1023) if full_range else (876, 64, 896)

        def r12(x):
            return int(round(x / 4095 * 65536))
        fy = [r12(kr * ys), r12(kg * ys), r12(kb * ys)]
        fcb = [r12(-kr / (2 * (1 - kb)) * cs), r12(-kg / (2 * (1 - kb)) * cs), r12(0.5 * cs)]
        fcr = [r12(0.5 * cs), r12(-kg / (2 * (1 - kr)) * cs), r12(-kb / (2 * (1 - kr)) * cs)]
        return YuvCoefs10(matrix, bool(full_range), tuple(fy + fcb + fcr + [yo]), None)
    ys, yo, cs = (255, 0, 255) if full_range else (219, 16, 224)

    def r(x):
        return int(round(x * 65536))
    fy = [r(kr * ys / 255), r(kg * ys / 255), r(kb * ys / 255)]
    fcb = [r(-kr / (2 * (1 - kb)) * cs / 255), r(-kg / (2 * (1 - kb)) * cs / 255), r(0.5 * cs / 255)]
    fcr = [r(0.5 * cs / 255), r(-kg / (2 * (1 - kr)) * cs / 255), r(-kb / (2 * (1 - kr)) * cs / 255)]
    iy, rcr, bcb = r(255 / ys), r(2 * (1 - kr) * 255 / cs), r(2 * (1 - kb) * 255 / cs)
    gcb, gcr = r(-2 * kb * (1 - kb) / kg * 255 / cs), r(-2 * kr * (1 - kr) / kg * 255 / cs)
    return YuvCoefs(matrix, bool(full_range), tuple(fy + fcb + fcr + [yo]), (yo, iy, rcr, gcb, gcr, bcb))


def auto_matrix(rows: int) -> str:
    """The usual convention for untagged material: BT.709 from 720 rows up, BT.601 below."""
    return "bt709" if rows >= 720 else "bt601"


def output_size(h4: int, w4: int, *, out_size=None, out_scale=None, fmt):
    """The (H, W) of the frames to write for a network result of h4 x w4 (4x its input).  At most one of: `out_size` = (W, H),
    taken as given — ValueError unless h4/4 <= H <= h4 and w4/4 <= W <= w4, and for an odd side with a 4:2:0 format `fmt`;
    `out_scale` = S in [1, 4] — each side 2*floor(S*side/2 + 0.5) of the network's input side (h4/4, w4/4), clipped to the even
    sizes of that range, so it suits every format.  Neither: (h4, w4)."""
    fmt = out_format(fmt)
    if out_size is not None and out_scale is not None:
        raise ValueError("give an output size or an output scale, not both")
    h1, w1 = -(-h4 // 4), -(-w4 // 4)
    span = f"{w1}x{h1} to {w4}x{h4}"
    if out_size is not None:
        w, h = (int(v) for v in out_size)
        if not (h1 <= h <= h4 and w1 <= w <= w4):
            raise ValueError(f"output size {w}x{h} is outside {span} (1x to 4x of the network's input)")
        if not fmt.chroma444 and (h % 2 or w % 2):
            raise ValueError(f"output size {w}x{h}: the 4:2:0 format {fmt.name} needs even sides ({span}, even)")
        return h, w
    if out_scale is not None:
        scale = float(out_scale)
        if not 1.0 <= scale <= 4.0:
            raise ValueError(f"output scale {out_scale} is outside 1 to 4 ({span})")

        def side(n1, n4):
            return min(max(2 * int(scale * n1 / 2 + 0.5), n1 + n1 % 2), n4 - n4 % 2)
        return side(h1, h4), side(w1, w4)
    return h4, w4


def chroma_siting(tag: str):
    """(centre_h, centre_v) of the chroma samples of a 4:2:0 Y4M colour-space tag ('' = no `C` tag): 'C420jpeg' centre / centre,
    'C420mpeg2', 'C420' and no tag co-sited horizontally and centred vertically, 'C420paldv' co-sited on both axes (top-left, as
    ffmpeg maps it); also 'C420p10', which is written left-sited like 'C420mpeg2'.  ValueError for any other tag."""
    if tag not in _SITING:
        raise ValueError(f"no 4:2:0 chroma siting is known for the tag {tag!r}")
    return _SITING[tag]


def _chroma_mode(chroma):
    if chroma not in CHROMA_MODES:
        raise ValueError(f"chroma must be one of {list(CHROMA_MODES)}, got {chroma!r}")
    return chroma


def output_siting(fmt, full_range: bool, chroma: str = "replicate"):
    """The siting `postprocess_planes` is to filter for, given the tag `y4m_header` writes for `fmt` and the range: None — the
    block-mean kernels, as ever — with `chroma="replicate"`, for the 4:4:4 formats (no filter) and for 'C420jpeg' (centre /
    centre IS the block mean); `chroma_siting(tag)` = (False, True) for 'C420mpeg2' and 'C420p10'."""
    fmt = out_format(fmt)
    if _chroma_mode(chroma) == "replicate" or fmt.chroma444:
        return None
    siting = chroma_siting(fmt.tag or ("C420jpeg" if full_range else "C420mpeg2"))
    return None if siting == (True, True) else siting


def preprocess_planes(clip: Y4MClip, device, matrix: str = "auto", chroma: str = "replicate") -> torch.Tensor:
    """A decoded .y4m clip -> (1,3,T,h,w) fp32 in [-1,1] on `device`: what `preprocess_frames` returns for the uint8 RGB
    frames a decoder with the fixed-point arithmetic of `uav_yuv420_to_clip_f32` would have produced (colour conversion
    and normalisation are one pass over 1.5 bytes per pixel; the >= 1280-px area pooling follows as there).
    `chroma="sited"`: 4:2:0 chroma is up-sampled bilinearly at `chroma_siting(clip.colorspace)` in the same pass
    (`ops.yuv420_sited_to_clip_f32`) instead of being replicated; 'C444' input has nothing to up-sample and ignores the option."""
    coefs = yuv_coefficients(auto_matrix(clip.size[0]) if matrix == "auto" else matrix, clip.full_range)
    sited = _chroma_mode(chroma) == "sited" and clip.colorspace != "C444"
    y, cb, cr = (torch.from_numpy(p).to(device) for p in (clip.y, clip.cb, clip.cr))
    with E.device_guard(y):
        if sited:
            out = ops.yuv420_sited_to_clip_f32(y, cb, cr, coefs, chroma_siting(clip.colorspace))
        else:
            out = ops.yuv420_to_clip_f32(y, cb, cr, coefs, chroma444=clip.colorspace == "C444")
        return _pool_large(out).unsqueeze(0)


def postprocess_planes(output: torch.Tensor, coefs: YuvCoefs, fmt="420", siting=None):
    """(T,3,H,W) in [-1,1] -> uint8 planes Y (T,H,W), Cb, Cr (T,H/2,W/2) on the device: `postprocess_frames`' uint8 RGB value,
    converted and 2x2-averaged in the same pass (reads the fp32 frames once, writes 1.5 bytes per pixel).  With another `fmt`
    of `OUT_FORMATS`: the planes of that format — Cb, Cr (T,H,W) for 4:4:4, int16 holding 0..1023 for 10 bits — in one pass too;
    `coefs` must be of the format's depth.  `siting` = (centre_h, centre_v) of the chroma samples to make (`output_siting`): None
    or (True, True) is the block mean above; (False, True), for a 4:2:0 format, is `ops.clip_to_yuv420_sited` — same luma,
    chroma filtered around the even column; a 4:4:4 format has no chroma filter and ignores it."""
    fmt = out_format(fmt)
    if siting is not None and tuple(siting) not in ((True, True), (False, True)):
        raise ValueError(f"output chroma is written centre / centre or left-sited (False, True), got siting {siting!r}")
    with E.device_guard(output):
        frames = output.float().contiguous()
        if siting is not None and tuple(siting) == (False, True) and not fmt.chroma444:
            return ops.clip_to_yuv420_sited(frames, coefs, fmt.depth)
        if fmt.name == "420":
            return ops.clip_to_yuv420_u8(frames, coefs)
        t, _, h, w = frames.shape
        planes = _new_planes(frames, t, h, w, fmt)
        ops.clip_window_to_yuv(frames, *planes, coefs, chroma444=fmt.chroma444, depth=fmt.depth, frames_first=True)
        return planes


def _new_planes(like, t, h, w, fmt: OutFormat):
    """Uninitialised planes of `t` frames of h x w pixels in `fmt` on the device of `like`."""
    if not fmt.chroma444 and (h % 2 or w % 2):
        raise ValueError(f"4:2:0 planes need even H and W, got {h}x{w}")
    ch, cw = (h, w) if fmt.chroma444 else (h // 2, w // 2)
    dtype = _plane_dtype(fmt)
    return (like.new_empty((t, h, w), dtype=dtype), like.new_empty((t, ch, cw), dtype=dtype), like.new_empty((t, ch, cw), dtype=dtype))


# ------------------------------------------------------------------------------------------------
# YUV4MPEG2
def _parse_y4m_header(data: bytes, end: int, path):
    """The stream header of a YUV4MPEG2 file — `data` from its first byte, `end` the index of the first newline (-1: none) — as
    (w, h, fps, colorspace, full_range); every refusal of `read_y4m` and `Y4MReader` about the header is raised here."""
    if not data.startswith(b"YUV4MPEG2") or end < 0 or (end > 9 and data[9:10] != b" "):
        raise ValueError(f"{path}: not a YUV4MPEG2 file (no 'YUV4MPEG2' signature line)")
    w = h = None
    fps, colorspace, full_range = None, "", None
    for tag in data[10:end].decode("ascii", "replace").split():
        key, val = tag[0], tag[1:]
        try:
            if key == "W":
                w = int(val)
            elif key == "H":
                h = int(val)
            elif key == "F":
                num, den = (int(v) for v in val.split(":"))
                fps = Fraction(num, den) if num > 0 and den > 0 else None
        except ValueError:
            raise ValueError(f"{path}: malformed header tag {tag!r}") from None
        if key == "I" and val not in ("p", "?"):
            raise ValueError(f"{path}: interlaced material is not supported (tag {tag!r})")
        if key == "C":
            if tag not in _CHROMA_420 + ("C444",):
                raise ValueError(f"{path}: unsupported colour space {tag!r} (8-bit 4:2:0 and 4:4:4 only)")
            colorspace = tag
        if tag.startswith("XCOLORRANGE="):
            if val[len("COLORRANGE="):] not in ("FULL", "LIMITED"):
                raise ValueError(f"{path}: unsupported range tag {tag!r}")
            full_range = val.endswith("=FULL")
    if not w or not h or w < 0 or h < 0:
        raise ValueError(f"{path}: the header has no valid W / H tags")
    if full_range is None:
        full_range = colorspace == "C420jpeg"
    return w, h, fps, colorspace, full_range


def read_y4m(path) -> Y4MClip:
    """Read a progressive 8-bit YUV4MPEG2 file — `path`, or an open binary stream such as a pipe, named by its `.name` in
    messages — whole.  Chroma `C420jpeg`, `C420mpeg2`, `C420paldv`, `C420` or no `C` tag
    (= 4:2:0, as the format defines) and `C444`.  Chroma SITING is not applied here: the tag is kept in `colorspace`, and
    `preprocess_planes` replicates a sample over its 2x2 block by default or, with `chroma="sited"`, filters at `chroma_siting(tag)`.  Range: `XCOLORRANGE=FULL|LIMITED` when present, else full for `C420jpeg` and limited for the
    rest.  Anything else (4:2:2, mono, more than 8 bits, interlaced, a truncated frame) raises ValueError naming the tag."""
    import numpy as np
    if hasattr(path, "read"):
        data, path = path.read(), getattr(path, "name", "<stream>")
    else:
        with open(path, "rb") as fh:
            data = fh.read()
    end = data.find(b"\n")
    w, h, fps, colorspace, full_range = _parse_y4m_header(data, end, path)
    ch, cw = (h, w) if colorspace == "C444" else ((h + 1) // 2, (w + 1) // 2)
    ysz, csz = h * w, ch * cw
    pos, offsets = end + 1, []
    while pos < len(data):
        nl = data.find(b"\n", pos)
        if not data.startswith(b"FRAME", pos) or nl < 0:
            raise ValueError(f"{path}: 'FRAME' expected at byte {pos}")
        pos = nl + 1                                                    # parameters on the FRAME line are skipped
        if pos + ysz + 2 * csz > len(data):
            raise ValueError(f"{path}: frame {len(offsets)} is truncated ('FRAME' with {len(data) - pos} of {ysz + 2 * csz} bytes)")
        offsets.append(pos)
        pos += ysz + 2 * csz
    if not offsets:
        raise ValueError(f"{path}: no 'FRAME' in the file")
    buf = np.frombuffer(data, dtype=np.uint8)
    y = np.stack([buf[o:o + ysz].reshape(h, w) for o in offsets])
    cb = np.stack([buf[o + ysz:o + ysz + csz].reshape(ch, cw) for o in offsets])
    cr = np.stack([buf[o + ysz + csz:o + ysz + 2 * csz].reshape(ch, cw) for o in offsets])
    return Y4MClip(y, cb, cr, fps, (h, w), colorspace, full_range)


class Y4MReader:
    """`read_y4m` in pieces: the header is parsed on construction by the same code (every refusal and message is `read_y4m`'s),
    then `read(n)` returns the next up to `n` frames as a `Y4MClip`, or None at the end of the input.  `path_or_stream`: a path,
    or an open binary stream such as a pipe — nothing seeks and nothing is read past the frames asked for (Python's own
    buffering aside).  `fps`, `size` = (H, W), `colorspace` and `full_range` are the header's; `frames_read` counts the frames
    returned so far.  A frame cut short and a missing 'FRAME' raise `read_y4m`'s ValueError with the same frame index / byte offset."""
    _LINE = 1 << 16                                    # longest header / FRAME line looked at

    def __init__(self, path_or_stream):
        self._own = not hasattr(path_or_stream, "read")
        self.name = os.fspath(path_or_stream) if self._own else getattr(path_or_stream, "name", "<stream>")
        self._fh = open(path_or_stream, "rb") if self._own else path_or_stream
        try:
            line = self._fh.readline(self._LINE)
            w, h, self.fps, self.colorspace, self.full_range = _parse_y4m_header(line, line.find(b"\n"), self.name)
        except BaseException:
            self.close()
            raise
        self.size, self.frames_read, self._pos = (h, w), 0, len(line)
        ch, cw = (h, w) if self.colorspace == "C444" else ((h + 1) // 2, (w + 1) // 2)
        self._cshape, self._ysz, self._csz = (ch, cw), h * w, ch * cw

    def _read_exact(self, n):
        parts, got = [], 0
        while got < n:
            part = self._fh.read(n - got)
            if not part:
                break
            parts.append(part)
            got += len(part)
        return parts[0] if len(parts) == 1 else b"".join(parts)

    def read(self, n: int):
        import numpy as np
        if n < 1:
            raise ValueError(f"Y4MReader.read: a positive number of frames expected, got {n}")
        size, frames = self._ysz + 2 * self._csz, []
        while len(frames) < n and self._fh is not None:
            line = self._fh.readline(self._LINE)
            if not line:
                break
            if not line.startswith(b"FRAME") or not line.endswith(b"\n"):
                raise ValueError(f"{self.name}: 'FRAME' expected at byte {self._pos}")
            self._pos += len(line)                                         # parameters on the FRAME line are skipped
            data = self._read_exact(size)
            if len(data) < size:
                raise ValueError(f"{self.name}: frame {self.frames_read + len(frames)} is truncated ('FRAME' with {len(data)} of "
                                 f"{size} bytes)")
            self._pos += size
            frames.append(data)
        if not frames:
            if self.frames_read == 0:
                raise ValueError(f"{self.name}: no 'FRAME' in the file")
            return None
        self.frames_read += len(frames)
        buf = np.frombuffer(b"".join(frames), dtype=np.uint8).reshape(len(frames), size)
        (h, w), (ch, cw), ysz, csz = self.size, self._cshape, self._ysz, self._csz
        y = buf[:, :ysz].reshape(-1, h, w).copy()
        cb = buf[:, ysz:ysz + csz].reshape(-1, ch, cw).copy()
        cr = buf[:, ysz + csz:].reshape(-1, ch, cw).copy()
        return Y4MClip(y, cb, cr, self.fps, self.size, self.colorspace, self.full_range)

    def close(self) -> None:
        fh, self._fh = getattr(self, "_fh", None), None
        if fh is not None and self._own:
            fh.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def y4m_header(w: int, h: int, fps, full_range: bool, fmt="420") -> bytes:
    fps = Fraction(str(fps)) if isinstance(fps, float) else Fraction(fps)
    tag = out_format(fmt).tag or ("C420jpeg" if full_range else "C420mpeg2")
    return (f"YUV4MPEG2 W{w} H{h} F{fps.numerator}:{fps.denominator} Ip A1:1 {tag} "
            f"XCOLORRANGE={'FULL' if full_range else 'LIMITED'}\n").encode("ascii")


class Y4MWriter:
    """A progressive YUV4MPEG2 stream written chunk by chunk: the header once, then `write(y, cb, cr)` appends the frames
    of planes Y (n,H,W), Cb, Cr (n,ceil(H/2),ceil(W/2)) — uint8 tensors on any device, or numpy arrays.  Device planes are
    gathered frame by frame on the device and cross to the host as ONE copy per call.  `path_or_file`: an open binary stream
    (a pipe will do: nothing seeks), or a path — then the bytes go to `<path>.part`, which takes the name only on a clean exit:
    a Y4M file has no frame count, so a file cut short by a failure would look complete.  `fmt`, one of `OUT_FORMATS`: 4:4:4
    takes Cb, Cr (n,H,W); the 10-bit formats take int16 tensors (or int16 / uint16 numpy arrays) holding 0..1023 and write
    every sample as 16 bits, little-endian."""

    def __init__(self, path_or_file, w: int, h: int, fps, full_range: bool, fmt="420"):
        self.w, self.h, self.frames, self.fmt = int(w), int(h), 0, out_format(fmt)
        self._path = None if hasattr(path_or_file, "write") else os.fspath(path_or_file)
        self._fh = path_or_file if self._path is None else open(self._path + ".part", "wb")
        try:
            self._fh.write(y4m_header(self.w, self.h, fps, full_range, self.fmt))
        except BaseException:
            self.close(False)
            raise

    def write(self, y, cb, cr) -> None:
        import numpy as np
        if len(y.shape) != 3 or tuple(y.shape[1:]) != (self.h, self.w):
            raise ValueError(f"Y4MWriter: luma planes {tuple(y.shape)}, expected (n, {self.h}, {self.w})")
        t = y.shape[0]
        cshape = (t, self.h, self.w) if self.fmt.chroma444 else (t, (self.h + 1) // 2, (self.w + 1) // 2)
        if tuple(cb.shape) != cshape or tuple(cr.shape) != cshape:
            raise ValueError(f"Y4MWriter: chroma planes {tuple(cb.shape)} / {tuple(cr.shape)}, expected {cshape} for "
                             f"{'4:4:4' if self.fmt.chroma444 else '4:2:0'}")
        if isinstance(y, torch.Tensor):
            if not y.dtype == cb.dtype == cr.dtype == _plane_dtype(self.fmt):
                raise ValueError(f"Y4MWriter: {'uint8' if self.fmt.depth == 8 else 'int16'} planes expected")
            frames = torch.cat([p.reshape(t, -1) for p in (y, cb, cr)], dim=1).cpu().numpy()       # (n, samples of one frame)
        else:
            if not all(p.dtype in ((np.uint8,) if self.fmt.depth == 8 else (np.int16, np.uint16)) for p in (y, cb, cr)):
                raise ValueError(f"Y4MWriter: {'uint8' if self.fmt.depth == 8 else 'int16 / uint16'} planes expected")
            frames = np.concatenate([np.ascontiguousarray(p).reshape(t, -1) for p in (y, cb, cr)], axis=1)
        if self.fmt.depth != 8:
            frames = frames.view(np.uint16).astype("<u2", copy=False)                               # little-endian in the file
        for i in range(t):
            self._fh.write(b"FRAME\n")
            self._fh.write(frames[i].tobytes())
        self._fh.flush()                                  # a reader on the other end of a pipe gets every chunk as it is made
        self.frames += t

    def close(self, complete: bool = True) -> None:
        """Flush; a file opened by path is closed and, when `complete`, renamed from `<path>.part` (else removed)."""
        fh, self._fh = self._fh, None
        if fh is None:
            return
        if self._path is None:
            fh.flush()
            return
        fh.close()
        if complete:
            os.replace(self._path + ".part", self._path)
        else:
            os.remove(self._path + ".part")

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self.close(exc_type is None)
        return False


def write_y4m(path, y, cb, cr, fps, full_range: bool, fmt="420") -> None:
    """Write 4:2:0 planes Y (T,H,W), Cb, Cr (T,ceil(H/2),ceil(W/2)) (uint8 tensors on any device, or numpy arrays) as a
    progressive YUV4MPEG2 file: one `Y4MWriter.write`.  `fmt`: the planes of another of `OUT_FORMATS`, as `Y4MWriter` takes them."""
    fmt = out_format(fmt)
    t, h, w = y.shape
    cshape = (t, h, w) if fmt.chroma444 else (t, (h + 1) // 2, (w + 1) // 2)
    if tuple(cb.shape) != cshape or tuple(cr.shape) != cshape:
        raise ValueError(f"write_y4m: chroma planes {tuple(cb.shape)} / {tuple(cr.shape)}, expected {cshape} for "
                         f"{'4:4:4' if fmt.chroma444 else '4:2:0'}")
    with Y4MWriter(path, w, h, fps, full_range, fmt) as out:
        out.write(y, cb, cr)


def read_frames(path):
    """One video from `path`: a `.y4m` file -> (Y4MClip, fps); a `.npy` file of (T,H,W,3) uint8 RGB or a directory of images
    (sorted names, decoded with PIL) -> ((T,H,W,3) uint8 numpy array, None)."""
    import numpy as np
    if os.path.isdir(path):
        names = sorted(n for n in os.listdir(path) if n.lower().endswith(IMAGE_EXTENSIONS))
        if not names:
            raise ValueError(f"{path}: no image files in the directory")
        try:
            from PIL import Image
        except ImportError:
            raise ValueError(f"{path}: reading image files needs the PIL package (Pillow)") from None
        frames = [np.asarray(Image.open(os.path.join(path, n)).convert("RGB")) for n in names]
        if len({f.shape for f in frames}) != 1:
            raise ValueError(f"{path}: the images differ in size")
        return np.stack(frames), None
    low = str(path).lower()
    if low.endswith(".y4m"):
        clip = read_y4m(path)
        return clip, clip.fps
    if low.endswith(".npy"):
        frames = np.load(path, allow_pickle=False)
        if frames.ndim != 4 or frames.shape[-1] != 3 or frames.dtype != np.uint8:
            raise ValueError(f"{path}: a (T,H,W,3) uint8 array expected, got {frames.dtype} {frames.shape}")
        return frames, None
    raise ValueError(f"{path}: unsupported input ('.y4m', '.npy' or a directory of images; convert other containers with "
                     "`ffmpeg -i in.mp4 in.y4m`)")


# ------------------------------------------------------------------------------------------------
def _window_to_planes(window, planes, dst, coefs, fmt=OUT_FORMATS["420"]):
    """One piece of a chunk — `window` (3,n,dy,dx), a view of decoder output — converted into the box `dst` = (y0, y1, x0, x1)
    of the chunk's planes Y (n,H,W), Cb, Cr (n,H/2,W/2).  On the device this is ONE kernel that reads the view in place and
    writes the box (`ops.clip_window_to_yuv420_u8`).  The only place that decides about host tensors: `uav.ops` has no CPU
    path — every op raises `UavError` for a host tensor, and so does this one in production — but the CPU tests swap
    `ops.clip_to_yuv420_u8` for a torch stand-in (tests/cpu_ops_io.py) and know nothing of newer symbols, so a host window
    goes through that entry point on a contiguous copy and is placed with torch indexing.  The other formats of `OUT_FORMATS`
    are `ops.clip_window_to_yuv` for every window (the CPU tests swap that one op: tests/cpu_ops_fmt.py)."""
    y0, y1, x0, x1 = dst
    cbox = (y0, y1, x0, x1) if fmt.chroma444 else (y0 // 2, y1 // 2, x0 // 2, x1 // 2)
    boxes = [p[:, a:b, c:d] for p, (a, b, c, d) in zip(planes, ((y0, y1, x0, x1), cbox, cbox))]
    if fmt.name != "420":
        ops.clip_window_to_yuv(window, *boxes, coefs, chroma444=fmt.chroma444, depth=fmt.depth)
    elif window.is_cuda:
        ops.clip_window_to_yuv420_u8(window, *boxes, coefs)
    else:
        for box, plane in zip(boxes, ops.clip_to_yuv420_u8(window.permute(1, 0, 2, 3).contiguous(), coefs)):
            box.copy_(plane)


def upscale_clip_chunks(pipeline, clip: torch.Tensor, *, prompt, negative_prompt, raft=None, propagation_steps=(), steps, guidance_scale,
                        noise_level, tile_size=256, perform_tile=False, color_fix="None", generator, coefs: YuvCoefs = None, fmt="420",
                        out_size=None, chroma="replicate", seam=None):
    """What the upscaling program does with one video between reading and writing it, in its order, 3 output frames at a time:
    bidirectional flows of the whole clip when propagation steps are asked for, then the DDIM loop of the whole clip — of
    every tile (`tiling.needs_tiling`: asked for, or h*w >= 384*384), or of the one pipeline call — whose results live at the
    input resolution, then per chunk the decode and the optional colour fix against the bicubically up-sampled input frames
    of that chunk (statistics, blur and resize are per frame).  `clip`: (1,3,T,h,w) in [-1,1] (preprocess_frames /
    preprocess_planes).  A generator of the chunks' frames (n,3,4h,4w) fp32, n <= 3 — or, with `coefs`, of their 4:2:0 planes
    (y, cb, cr) as `postprocess_planes` returns them, in the output format `fmt` (`coefs` of its depth); without a colour fix those
    are converted straight from the decoder's output, tile by tile, and no fp32 frame of the 4x clip is assembled at all.

    `out_size` = (H, W) other than (4h, 4w), within `output_size`'s range: every chunk is assembled as fp32 frames at 4x (the
    colour fix's branch; resampling crosses tile borders, so the tile-by-tile conversion cannot serve), colour-fixed at 4x when
    asked, resized to (n,3,H,W) with `ops.resize_aa_f32` and converted then.  That costs, per chunk of 3 frames and beside the
    decoder's output, the fp32 frames at 4x (3*3*4h*4w*4 bytes), the resizer's intermediate (3*3*4h*W*4) and its result
    (3*3*H*W*4).  `None` or (4h, 4w): today's path, unchanged.

    `chroma="sited"` with `coefs` of a left-sited 4:2:0 output (`output_siting(fmt, coefs.full_range, chroma)`): the 3-tap
    chroma filter crosses tile borders, so a chunk is assembled as fp32 frames too (the same branch) and converted by
    `postprocess_planes(..., siting=...)`.  Every other case — 'replicate', 4:4:4, full-range 8-bit 4:2:0 — is unchanged.

    `seam` = (head, tail), for `SceneChunks`' cross-fade of forced splits: a chunk that holds one of the clip's first `head` or last
    `tail` frames is yielded as fp32 frames (n,3,H,W) at the delivery size — assembled, colour-fixed and resized as above, NOT
    converted — even when `coefs` is given; the caller blends and converts them.  Every other chunk, and every chunk when `seam` is
    None, takes the path and gives the bytes described above."""
    from models_video import color_correction
    from . import tiling
    if color_fix not in ("None", "AdaIn", "Wavelet"):
        raise ValueError(f"color_fix must be 'None', 'AdaIn' or 'Wavelet', got {color_fix!r}")
    fmt = out_format(fmt)
    _chroma_mode(chroma)
    siting = output_siting(fmt, coefs.full_range, chroma) if coefs is not None else None      # fp32 frames have no chroma planes
    propagation_steps = list(propagation_steps)
    if propagation_steps and raft is None:
        raise ValueError("propagation steps need a flow estimator (raft=...)")
    h, w = clip.shape[-2:]
    head, tail = (0, 0) if seam is None else (int(v) for v in seam)
    if head < 0 or tail < 0 or head + tail > clip.shape[2]:
        raise ValueError(f"seam = (head, tail) must lie within the clip's {clip.shape[2]} frames without overlapping, got {seam!r}")
    if out_size is not None:
        out_h, out_w = output_size(4 * h, 4 * w, out_size=(out_size[1], out_size[0]), fmt=fmt if coefs is not None else "444")
        out_size = None if (out_h, out_w) == (4 * h, 4 * w) else (out_h, out_w)
    kwargs = dict(num_inference_steps=steps, guidance_scale=guidance_scale, noise_level=noise_level,
                  negative_prompt=negative_prompt, propagation_steps=propagation_steps)
    with torch.no_grad(), E.device_guard(clip):          # (no guard is held across a `yield`: the caller's current device is its own)
        flows_bi = list(raft.forward_slicing(clip)) if propagation_steps else None
    if tiling.needs_tiling(h, w, perform_tile):
        chunks = tiling.upscale_tiled_chunks(pipeline, prompt, clip, flows_bi, generator, tile_size=tile_size, **kwargs)
    else:
        denoised = pipeline.denoise(prompt, image=clip, flows_bi=flows_bi, generator=generator, **kwargs)
        whole = (0, 4 * h, 0, 4 * w)
        chunks = ((s, f.shape[2], [(whole, f[0])]) for s, f in pipeline.decode_chunks(denoised))
    for start, n, pieces in chunks:
        with torch.no_grad(), E.device_guard(clip):
            window = None
            at_seam = start < head or start + n > clip.shape[2] - tail
            if coefs is not None and color_fix == "None" and out_size is None and siting is None and not at_seam:
                out = _new_planes(clip, n, 4 * h, 4 * w, fmt)
                for dst, window in pieces:
                    _window_to_planes(window, out, dst, coefs, fmt)
                if window is None:          # no tile at all (`tile_grid` drops the only row or column of a frame no larger than
                    # the overlap): the planes of the black canvas the other path starts with
                    out = postprocess_planes(clip.new_zeros((n, clip.shape[1], 4 * h, 4 * w), dtype=torch.float32), coefs, fmt)
            else:
                out = clip.new_zeros((n, clip.shape[1], 4 * h, 4 * w), dtype=torch.float32)     # "start with black image"
                for (y0, y1, x0, x1), window in pieces:
                    out[:, :, y0:y1, x0:x1] = window.permute(1, 0, 2, 3)
                if color_fix != "None":
                    source = color_correction.upsample_bicubic4(clip[0, :, start:start + n].permute(1, 0, 2, 3).contiguous())
                    fix = color_correction.adain_color_fix if color_fix == "AdaIn" else color_correction.wavelet_color_fix
                    out = fix(out, source).float()
                if out_size is not None:
                    out = ops.resize_aa_f32(out.contiguous(), *out_size)
                if coefs is not None and not at_seam:
                    out = postprocess_planes(out, coefs, fmt, siting)
            del pieces, window                                  # views of the decoder's output: let it go before the next decode
        yield out
        del out


def upscale_clip(pipeline, clip: torch.Tensor, *, prompt, negative_prompt, raft=None, propagation_steps=(), steps, guidance_scale,
                 noise_level, tile_size=256, perform_tile=False, color_fix="None", generator, out_size=None) -> torch.Tensor:
    """`upscale_clip_chunks` with the frames of all chunks in one tensor (T,3,4h,4w) fp32: the whole 4x clip on the device —
    (T,3,H,W) with `out_size` = (H, W)."""
    return torch.cat(list(upscale_clip_chunks(
        pipeline, clip, prompt=prompt, negative_prompt=negative_prompt, raft=raft, propagation_steps=propagation_steps, steps=steps,
        guidance_scale=guidance_scale, noise_level=noise_level, tile_size=tile_size, perform_tile=perform_tile, color_fix=color_fix,
        generator=generator, out_size=out_size)))


# ------------------------------------------------------------------------------------------------
# scenes: cuts from the integer statistics of `ops.clip_scene_stats`, one clip per scene
SCENE_THRESHOLD = (24.0, 0.30)          # (MAD in 8-bit luma steps, histogram distance in [0, 1]): conventional starting values of
#                                         content detectors, NOT validated on real footage
SCENE_MIN_LEN = 8                       # the temporal window of the network: a shorter scene stays with its neighbour
SCENE_BINS = 64


class SceneCutter:
    """The decision of `scene_cuts`, fed piece by piece: `push(sad, hist)` takes the statistics of the next frames (sad[i] against
    the frame before, whichever piece that was in; the very first frame's is ignored) and returns the cuts that are certain by
    now, as absolute frame indices; `finish()` returns those the end of the input decides.  All cuts, in order, are in `.cuts`:
    the same list as one `scene_cuts(..., final=True)` call on the whole arrays, however the input was cut into pieces.  `.forced`
    is the sub-list of the cuts that `max_len` produced: a split in the middle of a shot, where `--scene-overlap` cross-fades.  A
    cut that is also a detected candidate — the earliest one falling on start + max_len — counts as detected."""

    def __init__(self, pixels: int, *, threshold=SCENE_THRESHOLD, min_len=SCENE_MIN_LEN, max_len=0):
        self.mad_min, self.hist_min = (float(v) for v in threshold)
        self.pixels, self.min_len, self.max_len = int(pixels), int(min_len), int(max_len)
        if self.pixels < 1 or self.min_len < 1 or self.mad_min < 0 or not 0.0 <= self.hist_min <= 1.0:
            raise ValueError(f"scene detection needs pixels >= 1, min_len >= 1, MAD >= 0 and a histogram distance in [0, 1], got "
                             f"{pixels!r}, {min_len!r}, {threshold!r}")
        if self.max_len < 0 or 0 < self.max_len < self.min_len:
            raise ValueError(f"max_len must be 0 (never force a split) or at least min_len = {self.min_len}, got {max_len!r}")
        self.frames, self.cuts, self.forced = 0, [], []
        self._start, self._pending, self._last_hist = 0, [], None

    def push(self, sad, hist):
        import numpy as np
        sad, hist = np.asarray(sad, dtype=np.int64).reshape(-1), np.asarray(hist, dtype=np.int64)
        if hist.shape != (len(sad), SCENE_BINS):
            raise ValueError(f"scene statistics: sad (n,) and hist (n, {SCENE_BINS}) expected, got {sad.shape} and {hist.shape}")
        if len(sad) == 0:
            return []
        before = hist[:1] if self._last_hist is None else self._last_hist[None]
        mad = sad.astype(np.float64) / self.pixels
        hd = np.abs(np.diff(np.concatenate([before, hist]), axis=0)).sum(axis=1).astype(np.float64) / (2.0 * self.pixels)
        hit = (mad >= self.mad_min) & (hd >= self.hist_min)
        if self.frames == 0:
            hit[0] = False                              # no frame before the first
        self._pending.extend(int(i) + self.frames for i in np.nonzero(hit)[0])
        self._last_hist, self.frames = hist[-1].copy(), self.frames + len(sad)
        return self._scan()

    def finish(self):
        """The end of the input: a cut needs min_len known frames after it whether more may follow or not, so what the last
        `push` left open stays one scene and nothing is added."""
        return self._scan()

    def _scan(self):
        new = []
        while True:
            # a candidate nearer than min_len to the scene's start stays inside the scene
            self._pending = [t for t in self._pending if t - self._start >= self.min_len]
            events = self._pending[:1] + ([self._start + self.max_len] if self.max_len > 0 else [])
            t = min(events, default=self.frames)
            if t >= self.frames or self.frames - t < self.min_len:
                # not seen yet, or too near the end of what is known: more frames decide — and when none come, this one and
                # every later one is too near the end
                break
            new.append(t)
            if self._pending[:1] != [t]:
                self.forced.append(t)                   # no candidate here: max_len alone made this cut
            self._start = t
        self.cuts.extend(new)
        return new


def scene_cuts(sad, hist, pixels, *, threshold=SCENE_THRESHOLD, min_len=SCENE_MIN_LEN, max_len=0, final=True, forced=False):
    """The first frames of the scenes 2, 3, ... of a clip of T frames, from `ops.clip_scene_stats`' integers `sad` (T,) and `hist`
    (T,64) and `pixels` = h*w.  For t >= 1, in float64: mad[t] = sad[t] / pixels (8-bit luma steps) and hd[t] = sum_b |hist[t][b] -
    hist[t-1][b]| / (2 pixels) in [0, 1]; frame t is a candidate iff mad[t] >= M AND hd[t] >= D, `threshold` = (M, D) — fast motion
    moves the MAD but not the histogram, a fade the histogram but hardly the MAD of neighbouring frames.  Candidates are taken in
    ascending order, s the current scene's start: t is a cut iff t - s >= min_len and T - t >= min_len, so flashes and stubs stay
    with a neighbour.  `max_len` = N > 0 forces a split at s + N when no cut fell in (s, s + N], under the same rule for the tail.
    `final=False`: T is what has been seen so far and more may follow — only the cuts that min_len known further frames make
    certain are returned, which is the same rule for the tail: both forms give one list for the same arrays, and a longer
    input only appends to it (`SceneCutter` is this form with a memory).  `forced=True`: the pair (cuts, forced cuts) instead — the
    second list holds those of the first that `max_len` alone produced (`SceneCutter.forced`).  The defaults are conventional
    starting values and have NOT been validated on real footage."""
    cutter = SceneCutter(pixels, threshold=threshold, min_len=min_len, max_len=max_len)
    cutter.push(sad, hist)
    if final:
        cutter.finish()
    return (list(cutter.cuts), list(cutter.forced)) if forced else list(cutter.cuts)


class SceneChunks:
    """The iterator `upscale_scenes_chunks` returns: the chunks of scene after scene; `.scenes` is the list of (start, end) frame
    ranges of the scenes begun so far — the nominal ranges [c_i, c_i+1) between the cuts, whatever `overlap` is —, `.seams` the
    forced cuts that have been cross-faded so far and `.frames` the number of input frames pulled."""

    def __init__(self, pipeline, pieces, scene, kwargs, overlap=0):
        threshold, min_len, max_len = scene
        self.scenes, self.seams, self.frames = [], [], 0
        self._scene = dict(threshold=threshold, min_len=min_len, max_len=max_len)
        SceneCutter(1, **self._scene)                                       # bad options raise here, not at the first chunk
        if isinstance(overlap, bool) or not isinstance(overlap, int) or not 0 <= overlap <= int(min_len):
            raise ValueError(f"overlap must be a number of frames from 0 to min_len = {int(min_len)}, got {overlap!r}")
        self._overlap = overlap
        self._gen = self._run(pipeline, iter(pieces), kwargs)

    def __iter__(self):
        return self

    def __next__(self):
        return next(self._gen)

    def close(self):
        self._gen.close()

    def _run(self, pipeline, pieces, kwargs):
        coefs = yuv_coefficients("bt601", True)         # the detector's luma: one table for every input, like its thresholds
        held, base, last, cutter = [], 0, None, None    # frames [base, self.frames) wait in `held`; `last`: the newest frame
        tail = None                                     # the open seam: the scene before's rendering of this scene's first frames

        def scene_clip(end, extra=0):
            """Take the frames [base, end) out of `held` as one contiguous clip.  The pieces are copied into it one by one and
            let go as they are, so the scene and one piece exist at a time, not the scene twice.  `extra`: the clip also gets a
            copy of the frames [end, end + extra), which stay in `held` for the next scene."""
            nonlocal base
            n = end - base
            self.scenes.append((base, end))
            base = end
            if extra == 0 and len(held) == 1 and held[0].shape[2] == n and held[0].is_contiguous():
                return held.pop()
            clip = held[0].new_empty(held[0].shape[:2] + (n + extra,) + held[0].shape[3:])
            done = 0
            while done < n:
                piece = held.pop(0)
                take = min(piece.shape[2], n - done)
                clip[:, :, done:done + take] = piece[:, :, :take]
                if take < piece.shape[2]:
                    held.insert(0, piece[:, :, take:].clone())              # the next scene's first frames: less than a piece
                done += take
                del piece
            for piece in held:                                              # known already: a cut has min_len >= extra frames behind it
                take = min(piece.shape[2], n + extra - done)
                clip[:, :, done:done + take] = piece[:, :, :take]
                done += take
                if done == n + extra:
                    break
            assert done == n + extra, "a forced cut without its look-ahead"
            return clip

        def scene_chunks(end):
            """The chunks of the scene [base, end).  After a forced cut its first `overlap` frames are the cross-fade of the scene
            before's tail and this scene's head; before one, the clip runs `overlap` frames on and those are held, not emitted."""
            nonlocal tail
            extra = self._overlap if end in cutter.forced else 0
            before, tail = tail, None
            head = 0 if before is None else self._overlap
            if head == 0 and extra == 0:
                yield from upscale_clip_chunks(pipeline, scene_clip(end), **kwargs)
                return
            seam_at, total = base, end + extra - base
            out_coefs, fmt, chroma = kwargs.get("coefs"), kwargs.get("fmt", "420"), kwargs.get("chroma", "replicate")
            siting = output_siting(fmt, out_coefs.full_range, chroma) if out_coefs is not None else None
            pos = got = kept = 0                        # frames of the clip seen, of the head gathered, of the tail kept
            mine = after = None
            for chunk in upscale_clip_chunks(pipeline, scene_clip(end, extra), seam=(head, extra), **kwargs):
                fp32 = isinstance(chunk, torch.Tensor)
                n = chunk.shape[0] if fp32 else chunk[0].shape[0]
                h_n = max(0, min(pos + n, head) - pos)                      # [0, h_n) of the chunk: head; [t_0, n): tail
                t_0 = min(n, max(0, total - extra - pos))
                if h_n:
                    if mine is None:
                        mine = chunk.new_empty((head,) + chunk.shape[1:])
                    mine[got:got + h_n] = chunk[:h_n]
                    got += h_n
                    if got == head:
                        k = head
                        with torch.no_grad(), E.device_guard(before):
                            wa = torch.tensor([(k - j) / (k + 1) for j in range(k)], dtype=torch.float32).to(before.device)
                            wb = torch.tensor([(j + 1) / (k + 1) for j in range(k)], dtype=torch.float32).to(before.device)
                            blended = ops.frame_axpby_f32(before, mine, wa, wb, out=before)
                            if out_coefs is not None:
                                blended = postprocess_planes(blended, out_coefs, fmt, siting)
                        self.seams.append(seam_at)
                        before = mine = None
                        for i in range(0, k, 3):
                            yield blended[i:i + 3] if out_coefs is None else tuple(p[i:i + 3] for p in blended)
                        del blended
                if t_0 > h_n:
                    part = chunk if (h_n, t_0) == (0, n) else chunk[h_n:t_0]
                    yield postprocess_planes(part, out_coefs, fmt, siting) if fp32 and out_coefs is not None else part
                    del part
                if t_0 < n:
                    if after is None:
                        after = chunk.new_empty((extra,) + chunk.shape[1:])
                    after[kept:kept + n - t_0] = chunk[t_0:]
                    kept += n - t_0
                pos += n
                del chunk
            assert pos == total and got == head and kept == extra, "a scene's chunks do not add up to its clip"
            tail = after

        for piece in pieces:
            if piece.dim() != 5 or piece.shape[0] != 1 or piece.shape[1] != 3 or piece.shape[2] < 1:
                raise ValueError(f"upscale_scenes_chunks: pieces of shape (1,3,n,h,w) expected, got {tuple(piece.shape)}")
            if cutter is None:
                cutter = SceneCutter(int(piece.shape[-2]) * int(piece.shape[-1]), **self._scene)
            elif piece.shape[-2:] != last.shape[-2:]:
                raise ValueError("upscale_scenes_chunks: the pieces differ in size")
            with torch.no_grad(), E.device_guard(piece):
                frames = piece[0].float() if last is None else torch.cat([last, piece[0].float()], dim=1)
                hist, sad = ops.clip_scene_stats(frames.contiguous(), coefs)
                skip = 0 if last is None else 1                             # the row of the frame carried over is not new
                sad, hist = sad[skip:].cpu().numpy(), hist[skip:].cpu().numpy()
                last = piece[0, :, -1:].float().clone()
            del frames
            held.append(piece)
            self.frames += piece.shape[2]
            del piece
            for cut in cutter.push(sad, hist):
                yield from scene_chunks(cut)
        if cutter is None:
            raise ValueError("upscale_scenes_chunks: no frames")
        for cut in cutter.finish() + [self.frames]:
            if cut > base:
                yield from scene_chunks(cut)


def upscale_scenes_chunks(pipeline, pieces, *, scene=(SCENE_THRESHOLD, SCENE_MIN_LEN, 0), overlap=0, **kwargs) -> SceneChunks:
    """`upscale_clip_chunks`, scene by scene (`--scenes auto`).  `pieces`: an iterator of (1,3,n,h,w) clips on the device, in
    order — a video read as far as it is needed; `scene` = (threshold, min_len, max_len) of `scene_cuts`; every other keyword is
    `upscale_clip_chunks`' and goes to it unchanged.  Each piece's statistics (`ops.clip_scene_stats`, with the last frame of the
    piece before in front) go to a `SceneCutter`; once a scene's end is certain, or the input ends, its frames are concatenated
    and `upscale_clip_chunks` runs on them as on a clip of its own — flows, DDIM loop and tiles per scene, nothing temporal
    crosses a cut — with the ONE `generator`, which carries on from scene to scene as it does from tile to tile; the scene's
    frames are dropped before more input is pulled.  Yields exactly what `upscale_clip_chunks` yields, scene after scene: a clip
    without a cut gives the chunks of `upscale_clip_chunks` on the whole clip bit for bit.  Held at once: the frames of the
    scene that is open (at most `max_len` when given) plus the piece that closed it and the min_len frames of look-ahead.
    The result iterates and records `.scenes` / `.frames` (`SceneChunks`).

    `overlap` = K > 0 (`--scene-overlap`) cross-fades the FORCED splits, those `max_len` makes in the middle of a shot
    (`SceneCutter.forced`); 0, the default, is the path above, bit for bit.  A scene [s, c) that ends at a forced cut c runs as ONE
    clip of the frames [s, c + K); its output for [c, c + K), the tail, is not emitted but held as fp32 frames at the delivery
    size (after the colour fix and `out_size`, before the colour conversion).  The next scene starts at c as ever, and its first K
    output frames, the head, taken at the same stage, are blended with the tail in one `ops.frame_axpby_f32` call:
        out[c + j] = wa_j * tail[j] + wb_j * head[j],  wb_j = float32((j + 1) / (K + 1)),  wa_j = float32((K - j) / (K + 1)),
    j = 0 .. K-1, every weight computed in double precision and rounded once, both products rounded to fp32 before the sum; with
    `coefs` the result goes through `postprocess_planes` like a colour-fixed chunk.  A scene that ends at a detected cut or at the
    end of the input is not extended: a detected cut stays hard.
      - Both sides of a cross-fade are renderings of the same input frame; no content from across a real cut is ever mixed in.
      - K <= min_len, else ValueError here, where bad scene options raise: a cut needs min_len known frames after it, so the K
        frames behind a forced cut are already held when it is reported, the next scene has at least K frames, and a scene's head
        and tail never overlap.
      - The one `generator` is used in the order of the scenes, extended clips included.
      - The result does not depend on how the input was cut into pieces.
      - `.scenes` keeps the nominal ranges [c_i, c_i+1); `.seams` lists the forced cuts that were cross-faded.
      - Every yielded chunk holds 1 to 3 frames, and the chunks add up to exactly the input's frames: a chunk that straddles a
        seam comes out as its blended, plain and (withheld) tail parts.
      - Chunks wholly outside a head or a tail keep their path (with `coefs`, the tile-by-tile conversion with no fp32 canvas);
        one that holds a head or tail frame is assembled as fp32 frames whole (`upscale_clip_chunks(..., seam=(head, tail))`).
    Held beside the above: K more input frames per open scene and K fp32 frames at the delivery size between two scenes (K*3*H*W*4
    bytes: 100 MB per frame at 3840x2160), twice that while a head is gathered.  Each forced split sends K more frames through the
    whole network, about K / max_len more work by the frame count (not measured).  The cross-fade is a linear dissolve between two
    independent renderings: it spreads the change of the invented detail over K frames and softens detail there, it does not
    remove the difference — and nobody has judged it on real footage."""
    return SceneChunks(pipeline, pieces, scene, kwargs, overlap)
