"""Video preprocessing on the device: decoded uint8 frames -> the feature extractor's input.

What the reference's data loader does on the CPU with the ``video_transforms_test`` list of ``configs/generate_*.yaml``
(generate_vgg.yaml:53-65) and ``GenerateMultipleSegments`` + permute (models/data/vggsound_dataset.py:233, 273-275):

    Resize(256, antialias=True) -> CenterCrop([224, 224]) -> ToFloat32DType -> Normalize(0.5, 0.5) -> segments of 16 frames

runs here as one launch of ``vaura_video_preprocess`` (csrc/preproc.hip) per source geometry.

Arithmetic.  For tensors ``torchvision.transforms.v2.Resize`` is ``torch.nn.functional.interpolate(mode="bilinear", antialias=True)``,
and on uint8 torch resamples in fixed point: per axis, float64 triangle-filter taps normalised to sum 1, scaled by ``2^prec`` (the
largest ``prec`` <= 22 whose largest tap stays below 2^15) and rounded to int16; a pixel is
``clamp((2^(prec-1) + sum(tap * src)) >> prec, 0, 255)``; the horizontal pass comes first and its result is uint8 again before the
vertical pass.  ``tap_table`` restates that; ``reference_u8`` applies it on the CPU; the kernel applies the same tables.  On every
geometry the tests use, ``reference_u8`` equals torch's uint8 path on every pixel.

Segments (video_transforms.py:146-156, 205-236, ``is_start_random=False``, video only): ``stride = int(step_size_seg * F)``,
``S = floor((T - F) / stride) + 1`` (or ``n_segments``), and the run of segments is CENTRED in the clip: it starts at frame
``(T - int((S * step + 1 - step) * F)) // 2``; segment ``s`` holds frames ``start + s * stride .. + F``.  Frames outside are dropped.

Decoder surfaces.  No decoder produces RGB: hardware decode hands over NV12 surfaces in device memory, software decode planar
yuv420p.  With ``input_format="nv12"`` / ``"i420"`` the input is 8-bit 4:2:0 (1.5 bytes per pixel over the link) and one launch of
``vaura_video_preprocess_yuv420`` computes ``yuv -> RGB uint8 -> the transforms above``.  The colour step is an integer formula the host
defines (``yuv_coefficients``: 2^14-scaled BT.601 / BT.709 coefficients, limited or full range, chroma replicated over its 2 x 2 luma
block) and the kernel only applies; ``yuv420_to_rgb_u8`` restates it on the CPU.  The reference does not pin it: its loader gets RGB
from torchvision / PyAV (swscale); what pins it is a float64 evaluation of the same real coefficients (tests/test_preprocess_yuv_host.py).

Frame rate.  Everything behind this stage counts in 25 fps frames (a 16-frame segment is 0.64 s), and the reference got its videos
there offline (scripts/reencode_videos.py:71: ``ffmpeg -vf fps=25``).  With ``src_fps=`` or ``pts=`` / ``time_base=`` the frames are
selected here: ``fps_plan`` / ``FpsClock`` restate ffmpeg's ``fps`` filter at its defaults in exact rationals (frames dropped and
repeated, nothing blended; parity unpinned by the reference — ffmpeg is not run, tests/preprocess_fps_reference.py walks the filter's
queue literally), the segments are cut from the selected sequence, and ``vaura_video_preprocess_frames`` /
``vaura_video_preprocess_yuv420_frames`` read every output frame's source frame from a device table: bit for bit the existing
launch on ``video[:, table]``.  ``VideoFrameStream`` does the same for frames that arrive a few at a time and hands out complete
segments, which ``LiveSession.push(frames=)`` takes.
"""
from __future__ import annotations

import functools
import math
from fractions import Fraction
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib as L

MAX_TAPS = 32                       # VAURA_PREPROC_MAX_TAPS (include/vaura_hip.h)
_LDS_TARGET = 48 * 1024             # tile_rows is the largest power of two <= 32 whose workgroup stays below this
_LDS_LIMIT = 64 * 1024

_RESIZE = "torchvision.transforms.v2.Resize"
_CROP = "torchvision.transforms.v2.CenterCrop"
_NORM = "torchvision.transforms.v2.Normalize"
# ToFloat32DType (video_transforms.py:68-78) is v2.ConvertDtype(float32) or, on newer torchvision, v2.ToDtype(float32, scale=True)
_TOFLOAT = ("models.data.transforms.video_transforms.ToFloat32DType", "vaura_amd.preprocess.ToFloat32DType",
            "torchvision.transforms.v2.ConvertDtype", "torchvision.transforms.v2.ConvertImageDtype", "torchvision.transforms.v2.ToDtype")


class ToFloat32DType:
    """Name holder: ``target: vaura_amd.preprocess.ToFloat32DType`` is accepted where the reference's class is named."""


def resized_size(H: int, W: int, resize: int) -> Tuple[int, int]:
    """torchvision's Resize(int): the short side to ``resize``, the long side to ``int(resize * long / short)``."""
    short, long = (W, H) if W <= H else (H, W)
    new_long = int(resize * long / short)
    return (new_long, resize) if W <= H else (resize, new_long)


def crop_offset(size: int, crop: int) -> int:
    """torchvision's center_crop: ``int(round((size - crop) / 2.0))`` (Python's round: half to even)."""
    return int(round((size - crop) / 2.0))


def tap_table(in_size: int, out_size: int, lo: int = 0, n: Optional[int] = None) -> dict:
    """Fixed-point taps of torch's antialiased bilinear resample of one axis, for output indices ``lo .. lo + n``.

    Returns ``start`` (n,) int32, ``length`` (n,) int32, ``weights`` (n, taps) int16, ``weights_f64`` (n, taps), ``taps``, ``prec``.
    The precision is decided by the largest tap over the WHOLE axis (as torch does), not over the kept range.  Rows near the border
    are shifted so that ``start + taps <= in_size`` for every row (zero taps fill the front); ``start + length`` is where the last
    non-zero tap may sit.  ``in_size == out_size`` (no resize on this axis) is the identity: one tap of 2^14.
    """
    n = out_size - lo if n is None else n
    if in_size == out_size:
        idx = np.arange(lo, lo + n, dtype=np.int32)
        return {"start": idx, "length": np.ones(n, np.int32), "weights": np.full((n, 1), 1 << 14, np.int16),
                "weights_f64": np.ones((n, 1)), "taps": 1, "prec": 14}
    scale = in_size / out_size
    support = scale if scale >= 1.0 else 1.0
    invscale = 1.0 / scale if scale >= 1.0 else 1.0
    K = int(math.ceil(np.float32(support))) * 2 + 1
    w = np.zeros((out_size, K))
    start = np.zeros(out_size, np.int64)
    length = np.zeros(out_size, np.int64)
    for i in range(out_size):
        center = scale * (i + 0.5)
        xmin = max(int(center - support + 0.5), 0)
        xsize = min(max(min(int(center + support + 0.5), in_size) - xmin, 0), K)
        total = 0.0
        for j in range(xsize):
            d = abs((j + xmin - center + 0.5) * invscale)
            w[i, j] = 1.0 - d if d < 1.0 else 0.0
            total += w[i, j]
        if total != 0.0:
            w[i, :xsize] /= total
        start[i], length[i] = xmin, xsize
    wmax = float(w.max())
    prec = 0
    while prec < 22 and int(0.5 + wmax * (1 << (prec + 1))) < (1 << 15):
        prec += 1
    wi = np.trunc(w * (1 << prec) + 0.5).astype(np.int64)            # bilinear taps are never negative
    # keep the asked range, then make every row read exactly `taps` source elements inside [0, in_size)
    w, wi, start, length = w[lo:lo + n], wi[lo:lo + n], start[lo:lo + n], length[lo:lo + n]
    taps = min(K, in_size)
    new_start = np.minimum(start, in_size - taps)
    shift = start - new_start
    wf2, wi2 = np.zeros((n, taps)), np.zeros((n, taps), np.int64)
    for i in range(n):
        m = min(int(length[i]), taps - int(shift[i]))
        wf2[i, shift[i]:shift[i] + m] = w[i, :m]
        wi2[i, shift[i]:shift[i] + m] = wi[i, :m]
    return {"start": new_start.astype(np.int32), "length": (length + shift).astype(np.int32), "weights": wi2.astype(np.int16),
            "weights_f64": wf2, "taps": int(taps), "prec": int(prec)}


def segment_starts(T: int, F: int, step_size_seg: float = 1.0, n_segments: Optional[int] = None) -> Tuple[int, int, int]:
    """(S, first frame, stride) of GenerateMultipleSegments with ``is_start_random=False`` (see the module docstring)."""
    stride = int(step_size_seg * F)
    if F < 1 or stride < 1:
        raise L.VauraHipError(f"segments of {F} frames with step {step_size_seg}: the stride must be at least one frame")
    if T < F:
        raise L.VauraHipError(f"a clip of {T} frames is shorter than one segment of {F} frames")
    s_max = math.floor((T - F) / stride) + 1
    S = s_max if n_segments is None else int(n_segments)
    if S < 1 or S > s_max:
        raise L.VauraHipError(f"cannot make {S} segments of {F} frames (stride {stride}) from {T} frames: at most {s_max}")
    seq = int((S * step_size_seg + (1 - step_size_seg)) * F)
    return S, (T - seq) // 2, stride


# ---- video at its own frame rate: which source frame every 25 fps tick shows (exact rationals, host only)
MODEL_FPS = 25
MAP_KEEP, MAP_CARRY = -1, -2                                          # frame_map values of the table launches (include/vaura_hip.h)


def as_rate(x) -> Fraction:
    """A frame rate or a time base as an exact rational: int, Fraction, ``(num, den)`` or float (through ``Fraction(str(x))``, so
    29.97 is 2997/100 and not its binary neighbour; NTSC rates are ``(30000, 1001)``)."""
    if isinstance(x, bool):
        raise L.VauraHipError(f"a rate is an int, a Fraction, (num, den) or a float; got {x!r}")
    if isinstance(x, Fraction):
        r = x
    elif isinstance(x, (int, np.integer)):
        r = Fraction(int(x))
    elif isinstance(x, tuple) and len(x) == 2 and all(isinstance(v, (int, np.integer)) for v in x) and x[1] != 0:
        r = Fraction(int(x[0]), int(x[1]))
    elif isinstance(x, float) and math.isfinite(x):
        r = Fraction(str(x))
    else:
        raise L.VauraHipError(f"a rate is an int, a Fraction, (num, den) or a float; got {x!r}")
    if r <= 0:
        raise L.VauraHipError(f"a rate must be positive; got {x!r}")
    return r


def _rnd(x: Fraction) -> int:
    """Nearest integer, halves away from zero."""
    n, d = x.numerator, x.denominator
    q = (2 * abs(n) + d) // (2 * d)
    return q if n >= 0 else -q


def _pts_list(pts) -> List[int]:
    vals = pts.tolist() if hasattr(pts, "tolist") else list(pts)
    if any(isinstance(p, bool) or not isinstance(p, (int, np.integer)) for p in vals):
        raise L.VauraHipError("pts are integers in units of time_base")
    return [int(p) for p in vals]


class FpsPlan:
    """``table`` (n_out,) int32: the source frame tick ``first_tick + m`` shows; ``n_out``; ``first_tick`` (r_0)."""

    def __init__(self, table: np.ndarray, first_tick: int):
        self.table, self.n_out, self.first_tick = table, int(len(table)), int(first_tick)


class FpsClock:
    """ffmpeg's ``fps`` filter at its defaults (``round=near``, ``eof_action=round``) as a rule on integers, applied frame by frame.
    Parity unpinned by the reference: it is restated from the filter's algorithm, ffmpeg itself is not run.

    Source frame i has time t_i (``i / src_fps``, or ``pts_i * time_base``) and reaches the output at tick
    ``r_i = rnd(t_i * dst_fps)`` (nearest, halves away from zero).  Tick m shows ``max{i : r_i <= m}``: a frame whose successor has
    also reached the tick is dropped, a frame whose successor lies beyond it is shown again.  A tick is decided once a frame with
    ``r_i > m`` has arrived; the end of the video (``close``) decides the ticks up to ``r_end = rnd(t_end * dst_fps)``."""

    def __init__(self, src_fps=None, *, time_base=None, dst_fps=MODEL_FPS):
        if (src_fps is None) == (time_base is None):
            raise L.VauraHipError("FpsClock takes src_fps (constant rate) or time_base (timestamped frames), not both and not neither")
        self.src_fps = None if src_fps is None else as_rate(src_fps)
        self.time_base = None if time_base is None else as_rate(time_base)
        self.dst_fps = as_rate(dst_fps)
        self.n = 0                                                      # frames received
        self.first_tick: Optional[int] = None                           # r_0
        self.next_tick: Optional[int] = None                            # the first tick not decided yet (r of the last frame)
        self._t: List[Fraction] = []                                     # the times of the last two frames
        self.closed = False

    def _times(self, frames) -> List[Fraction]:
        if self.src_fps is not None:
            if isinstance(frames, bool) or not isinstance(frames, (int, np.integer)) or frames < 0:
                raise L.VauraHipError(f"a constant-rate clock is pushed a number of frames; got {frames!r}")
            return [Fraction(self.n + i) / self.src_fps for i in range(int(frames))]
        if isinstance(frames, (int, np.integer)):
            raise L.VauraHipError("a timestamped clock is pushed the pts of its frames, not a count")
        ts = [p * self.time_base for p in _pts_list(frames)]
        prev = self._t[-1] if self._t else None
        for t in ts:
            if prev is not None and t <= prev:
                raise L.VauraHipError("pts must be strictly increasing")
            prev = t
        return ts

    def push(self, frames) -> List[Tuple[int, int]]:
        """``frames``: a count (constant rate) or the pts of the new frames -> [(tick, source frame), ...] that became decided."""
        if self.closed:
            raise L.VauraHipError("FpsClock.push after close")
        out = []
        for t in self._times(frames):
            r = _rnd(t * self.dst_fps)
            if self.n == 0:
                self.first_tick = self.next_tick = r
            else:
                out += [(m, self.n - 1) for m in range(self.next_tick, r)]
                self.next_tick = r
            self._t = (self._t + [t])[-2:]
            self.n += 1
        return out

    def close(self, end=None) -> List[Tuple[int, int]]:
        """The ticks the end of the video decides.  Constant rate: t_end = n / src_fps.  With pts: ``end`` (in time_base units, behind
        the last frame) or, without it, the last frame lasts as long as the one before it (a single frame: one output tick)."""
        if self.closed:
            raise L.VauraHipError("FpsClock.close called twice")
        if self.n == 0:
            self.closed = True
            return []
        if self.src_fps is not None:
            if end is not None:
                raise L.VauraHipError("end is a pts; a constant-rate video ends at n / src_fps")
            t_end = Fraction(self.n) / self.src_fps
        elif end is not None:
            t_end = _pts_list([end])[0] * self.time_base
            if t_end <= self._t[-1]:
                raise L.VauraHipError("end must lie behind the pts of the last frame")
        else:
            t_end = 2 * self._t[-1] - self._t[-2] if self.n >= 2 else self._t[-1] + 1 / self.dst_fps
        r_end = _rnd(t_end * self.dst_fps)
        out = [(m, self.n - 1) for m in range(self.next_tick, r_end)]
        self.next_tick = max(self.next_tick, r_end)
        self.closed = True
        return out


def fps_plan(n_frames: Optional[int] = None, src_fps=None, *, pts=None, time_base=None, end=None, dst_fps=MODEL_FPS) -> FpsPlan:
    """The whole selection at once, in closed form (``FpsClock`` is the same rule frame by frame): exactly one of
    ``(n_frames, src_fps)`` and ``(pts, time_base)``.  N_out = max(r_end - r_0, 0)."""
    const, stamped = n_frames is not None or src_fps is not None, pts is not None or time_base is not None
    if const == stamped or (const and (n_frames is None or src_fps is None)) or (stamped and (pts is None or time_base is None)):
        raise L.VauraHipError("fps_plan takes (n_frames, src_fps) or (pts, time_base), not both and not neither")
    dst = as_rate(dst_fps)
    if const:
        if end is not None:
            raise L.VauraHipError("end is a pts; a constant-rate video ends at n / src_fps")
        if isinstance(n_frames, bool) or not isinstance(n_frames, (int, np.integer)) or n_frames < 0:
            raise L.VauraHipError(f"n_frames must be a non-negative int; got {n_frames!r}")
        return _constant_plan(int(n_frames), as_rate(src_fps), dst)
    tb = as_rate(time_base)
    ts = [p * tb for p in _pts_list(pts)]
    if any(b <= a for a, b in zip(ts, ts[1:])):
        raise L.VauraHipError("pts must be strictly increasing")
    if not ts:
        return FpsPlan(np.zeros(0, np.int32), 0)
    if end is not None:
        t_end = _pts_list([end])[0] * tb
        if t_end <= ts[-1]:
            raise L.VauraHipError("end must lie behind the pts of the last frame")
    else:
        t_end = 2 * ts[-1] - ts[-2] if len(ts) >= 2 else ts[0] + 1 / dst
    return _plan_of_times(ts, t_end, dst)


def _plan_of_times(ts: List[Fraction], t_end: Fraction, dst: Fraction) -> FpsPlan:
    r = np.array([_rnd(t * dst) for t in ts], dtype=np.int64)
    r_end = _rnd(t_end * dst)
    ticks = np.arange(int(r[0]), max(r_end, int(r[0])), dtype=np.int64)
    table = (np.searchsorted(r, ticks, side="right") - 1).astype(np.int32)
    table.setflags(write=False)
    return FpsPlan(table, int(r[0]))


@functools.lru_cache(maxsize=256)
def _constant_plan(n: int, src: Fraction, dst: Fraction) -> FpsPlan:
    """Kept per (n, rates): the rationals of a few hundred frames cost more host time than the launch they plan."""
    if n == 0:
        return FpsPlan(np.zeros(0, np.int32), 0)
    return _plan_of_times([Fraction(i) / src for i in range(n)], Fraction(n) / src, dst)


INPUT_FORMATS = ("rgb", "nv12", "i420")
_YUV_LAYOUT = {"nv12": 0, "i420": 1}                                  # VAURA_YUV_NV12 / VAURA_YUV_I420 (include/vaura_hip.h)
_COLOR_MATRIX = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}   # (Kr, Kb)
_COLOR_RANGE = {"limited": (16, 255 / 219, 255 / 224), "full": (0, 1.0, 1.0)}   # (y_off, luma scale, chroma scale)
YUV_PREC = 14


def yuv_coefficients_f64(color_matrix: str = "bt601", color_range: str = "limited") -> Tuple[int, Tuple[float, ...]]:
    """(y_off, (cy, crv, cgu, cgv, cbu)) as real numbers: R = cy (Y - y_off) + crv (V - 128), G = .. + cgu (U - 128) + cgv (V - 128),
    B = .. + cbu (U - 128)."""
    if color_matrix not in _COLOR_MATRIX:
        raise L.VauraHipError(f"color_matrix {color_matrix!r} is not built; one of {sorted(_COLOR_MATRIX)}")
    if color_range not in _COLOR_RANGE:
        raise L.VauraHipError(f"color_range {color_range!r} is not built; one of {sorted(_COLOR_RANGE)}")
    kr, kb = _COLOR_MATRIX[color_matrix]
    kg = 1 - kr - kb
    y_off, sy, sc = _COLOR_RANGE[color_range]
    return y_off, (sy, 2 * sc * (1 - kr), -2 * sc * kb * (1 - kb) / kg, -2 * sc * kr * (1 - kr) / kg, 2 * sc * (1 - kb))


def yuv_coefficients(color_matrix: str = "bt601", color_range: str = "limited") -> Tuple[int, int, int, int, int, int]:
    """(y_off, cy, crv, cgu, cgv, cbu): the integers the kernel applies, ``int(round(c * 2^14))``."""
    y_off, cs = yuv_coefficients_f64(color_matrix, color_range)
    return (y_off, *[int(round(c * (1 << YUV_PREC))) for c in cs])


def yuv_surface(frames: torch.Tensor, layout: str, size: Optional[Tuple[int, int]] = None,
                chroma_row: Optional[int] = None) -> Tuple[int, int, int, int, int]:
    """(.., R, P) uint8 surfaces -> (H, W, R, P, chroma_row), with every refusal about the surface.  ``size=None``: tight frames,
    R = 3H/2 and P = W; else P >= W is the pitch, luma sits in rows [0, H), the chroma plane starts at row ``chroma_row`` (default H)
    and R >= chroma_row + H/2."""
    if layout not in _YUV_LAYOUT:
        raise L.VauraHipError(f"input_format {layout!r} is not a 4:2:0 layout; one of {sorted(_YUV_LAYOUT)}")
    R, P = int(frames.shape[-2]), int(frames.shape[-1])
    if size is None:
        if R % 3:
            raise L.VauraHipError(f"tight {layout} frames have R = 3H/2 rows; R = {R} is no multiple of 3 (pass size=(H, W) for a padded "
                                  "surface)")
        if chroma_row is not None:
            raise L.VauraHipError("chroma_row needs size=(H, W)")
        H, W = 2 * R // 3, P
    else:
        H, W = int(size[0]), int(size[1])
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise L.VauraHipError(f"a 4:2:0 frame has even height and width; got H = {H}, W = {W}")
    crow = H if chroma_row is None else int(chroma_row)
    if P < W:
        raise L.VauraHipError(f"pitch P = {P} is shorter than a row of W = {W} pixels")
    if layout == "i420" and P % 2:
        raise L.VauraHipError(f"i420 with an odd pitch P = {P}: the chroma planes have pitch P / 2")
    if crow < H:
        raise L.VauraHipError(f"chroma_row = {crow} lies inside the luma plane of H = {H} rows")
    if R < crow + H // 2:
        raise L.VauraHipError(f"R = {R} rows do not hold the chroma plane: chroma_row + H / 2 = {crow + H // 2}")
    if frames.stride(-1) != 1 or frames.stride(-2) != P:
        raise L.VauraHipError(f"the last two dims of a {layout} input must be contiguous; strides are {tuple(frames.stride())}")
    return H, W, R, P, crow


def yuv420_planes(frames: torch.Tensor, layout: str, size: Optional[Tuple[int, int]] = None, chroma_row: Optional[int] = None):
    """(.., R, P) uint8 surfaces (``yuv_surface``) -> ``(y (.., H, W), u (.., H/2, W/2), v (.., H/2, W/2))``."""
    H, W, R, P, crow = yuv_surface(frames, layout, size, chroma_row)
    lead = tuple(frames.shape[:-2])
    y = frames[..., :H, :W]
    c = frames[..., crow:crow + H // 2, :].reshape(*lead, -1)          # the chroma plane(s) as bytes
    if layout == "nv12":
        c = c.reshape(*lead, H // 2, P)[..., :W].reshape(*lead, H // 2, W // 2, 2)
        return y, c[..., 0], c[..., 1]
    c = c.reshape(*lead, 2, H // 2, P // 2)[..., :W // 2]
    return y, c[..., 0, :, :], c[..., 1, :, :]


def yuv420_to_rgb_u8(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, color_matrix: str = "bt601",
                     color_range: str = "limited") -> torch.Tensor:
    """The kernel's colour step on the CPU (torch int32): y (.., H, W), u and v (.., H/2, W/2) uint8 -> RGB uint8 (.., 3, H, W).
    ``level = clamp((cy (Y - y_off) + cu (U - 128) + cv (V - 128) + 2^13) >> 14, 0, 255)``, arithmetic shift; the chroma sample at
    ``(y >> 1, x >> 1)`` serves its 2 x 2 luma block."""
    y_off, cy, crv, cgu, cgv, cbu = yuv_coefficients(color_matrix, color_range)
    H, W = y.shape[-2:]
    if tuple(u.shape[-2:]) != (H // 2, W // 2) or u.shape != v.shape or H % 2 or W % 2:
        raise L.VauraHipError(f"4:2:0 planes: y {tuple(y.shape)} needs u, v of (.., {H // 2}, {W // 2}); got {tuple(u.shape)}, {tuple(v.shape)}")
    up = lambda c: (c.cpu().to(torch.int32) - 128).repeat_interleave(2, -2).repeat_interleave(2, -1)  # noqa: E731
    yy = (y.cpu().to(torch.int32) - y_off) * cy + (1 << (YUV_PREC - 1))
    uu, vv = up(u), up(v)
    rgb = torch.stack([yy + crv * vv, yy + cgu * uu + cgv * vv, yy + cbu * uu], dim=-3)
    return (rgb >> YUV_PREC).clamp_(0, 255).to(torch.uint8)


class _Geometry:
    """Tables of one (H, W, resize, crop): host copies, and device copies per device."""

    def __init__(self, H: int, W: int, resize: int, crop: Tuple[int, int]):
        self.H, self.W, self.resize, self.crop = H, W, resize, crop
        ch, cw = crop
        oh, ow = resized_size(H, W, resize)
        if ch > oh or cw > ow:
            raise L.VauraHipError(f"crop {crop} is larger than the resized image {(oh, ow)} of a {H} x {W} source")
        if cw % 4:
            raise L.VauraHipError(f"crop width {cw}: the kernel writes 4 columns per store (multiples of 4 only)")
        self.out_hw = (oh, ow)
        self.top, self.left = crop_offset(oh, ch), crop_offset(ow, cw)
        self.h = tap_table(W, ow, self.left, cw)
        self.v = tap_table(H, oh, self.top, ch)
        if self.h["taps"] > MAX_TAPS or self.v["taps"] > MAX_TAPS:
            raise L.VauraHipError(f"{H} x {W} -> {oh} x {ow} needs {max(self.h['taps'], self.v['taps'])} taps per pixel; the kernel "
                                  f"is compiled for at most {MAX_TAPS}")
        self.x0 = int(self.h["start"].min())
        self.span = int(self.h["start"].max()) + self.h["taps"] - self.x0
        self.h_rel = (self.h["start"] - self.x0).astype(np.int32)
        self._dev: Dict[str, tuple] = {}
        self._tiles: Dict[object, Tuple[int, int]] = {}

    def tile_src_rows(self, tile_rows: int) -> int:
        st, ch, k = self.v["start"], self.crop[0], self.v["taps"]
        return max(int(st[min(r0 + tile_rows, ch) - 1]) + k - int(st[r0]) for r0 in range(0, ch, tile_rows))

    def tiles(self, channels_last: bool, yuv_layout: Optional[str] = None) -> Tuple[int, int]:
        """(tile_rows, tile_src_rows): the largest power of two <= 32 output rows whose workgroup stays below the LDS target.
        ``yuv_layout`` ("nv12" / "i420"): for the launch from 4:2:0 surfaces, whose row slabs are larger."""
        key = channels_last if yuv_layout is None else yuv_layout
        if key not in self._tiles:
            lib = L.lib()
            pick = None
            for tr in (32, 16, 8, 4, 2, 1):
                rows = self.tile_src_rows(tr)
                if yuv_layout is None:
                    need = lib.vaura_video_preprocess_lds_bytes(int(channels_last), self.crop[1], self.h["taps"], self.span, rows)
                else:
                    need = lib.vaura_video_preprocess_yuv420_lds_bytes(_YUV_LAYOUT[yuv_layout], self.crop[1], self.h["taps"], self.span, rows)
                if need <= _LDS_TARGET or (tr == 1 and need <= _LDS_LIMIT):
                    pick = (tr, rows)
                    break
            if pick is None:
                raise L.VauraHipError(f"a {self.H} x {self.W} source does not fit the kernel's {_LDS_LIMIT // 1024} KiB of LDS at one "
                                      "output row per workgroup")
            self._tiles[key] = pick
        return self._tiles[key]

    def device_tables(self, dev: torch.device):
        key = str(dev)
        if key not in self._dev:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
            self._dev[key] = (up(self.h_rel), up(self.h["weights"]), up(self.v["start"]), up(self.v["weights"]))
        return self._dev[key]


def _resample_axis(x: torch.Tensor, tab: dict, axis: int) -> torch.Tensor:
    """x int32; one pass of the fixed-point resample along ``axis`` for the rows of ``tab``."""
    x = x.movedim(axis, -1)
    start = torch.from_numpy(tab["start"].astype(np.int64))
    w = torch.from_numpy(tab["weights"].astype(np.int32))
    acc = torch.full(x.shape[:-1] + (len(start),), 1 << (tab["prec"] - 1), dtype=torch.int32)
    for k in range(tab["taps"]):
        acc += x.index_select(-1, start + k) * w[:, k]
    return (acc >> tab["prec"]).clamp_(0, 255).movedim(-1, axis)


class VideoPreprocessor:
    def __init__(self, resize: int = 256, crop: Sequence[int] = (224, 224), mean: Sequence[float] = (0.5, 0.5, 0.5),
                 std: Sequence[float] = (0.5, 0.5, 0.5), segment_size_vframes: int = 16, n_segments: Optional[int] = None,
                 step_size_seg: float = 1.0, channels_last: bool = False, device: Union[str, torch.device, None] = None,
                 input_format: str = "rgb", color_matrix: str = "bt601", color_range: str = "limited", src_fps=None,
                 dst_fps=MODEL_FPS):
        """``src_fps``: the frame rate of the input (``as_rate``; a list: one rate per clip of a call), None = it is ``dst_fps``
        already.  Any other rate is converted to ``dst_fps`` by dropping and repeating frames (``fps_plan``) in the same launch;
        timestamped input passes ``pts`` / ``time_base`` to the call instead."""
        self.dst_fps = as_rate(dst_fps)
        self.src_fps = self._rates(src_fps)
        if input_format not in INPUT_FORMATS:
            raise L.VauraHipError(f"input_format {input_format!r} is not built; one of {list(INPUT_FORMATS)}")
        self.input_format, self.color_matrix, self.color_range = input_format, color_matrix, color_range
        self.yuv = yuv_coefficients(color_matrix, color_range)          # refuses an unknown matrix / range
        if input_format != "rgb" and channels_last:
            raise L.VauraHipError(f"channels_last=True with input_format={input_format!r}: a 4:2:0 surface has planes, not channels")
        if isinstance(crop, int):
            crop = (crop, crop)
        if isinstance(resize, (list, tuple)):
            if len(resize) != 1:
                raise L.VauraHipError(f"Resize(size={list(resize)}): only the int form (short side) is built")
            resize = resize[0]
        self.resize, self.crop = int(resize), (int(crop[0]), int(crop[1]))
        mean = [float(mean)] * 3 if isinstance(mean, (int, float)) else [float(m) for m in mean]
        std = [float(std)] * 3 if isinstance(std, (int, float)) else [float(s) for s in std]
        if len(mean) != 3 or len(std) != 3 or any(s == 0 for s in std):
            raise L.VauraHipError(f"Normalize(mean={mean}, std={std}): three values each, std non-zero")
        self.mean, self.std = tuple(mean), tuple(std)
        self.segment_size_vframes, self.n_segments, self.step_size_seg = int(segment_size_vframes), n_segments, float(step_size_seg)
        self.channels_last = bool(channels_last)
        self.device = None if device is None else torch.device(device)
        self._geo: Dict[Tuple[int, int], _Geometry] = {}
        self._lut_dev: Dict[str, torch.Tensor] = {}
        self._map_dev: Dict[tuple, torch.Tensor] = {}
        # lut[c, level] = ((level / 255) - mean[c]) / std[c], in fp32, in that order
        lv = torch.arange(256, dtype=torch.float32) / 255
        self.lut = torch.stack([(lv - torch.tensor(m, dtype=torch.float32)) / torch.tensor(s, dtype=torch.float32)
                                for m, s in zip(self.mean, self.std)]).contiguous()

    # ---- configuration
    @classmethod
    def from_transforms_config(cls, transforms: Sequence[dict], **segment_kw) -> "VideoPreprocessor":
        """From the reference's ``video_transforms_test`` list (configs/generate_vgg.yaml:53-65) as plain data."""
        kw: dict = {}
        seen: List[str] = []
        for entry in transforms:
            target = entry.get("target") if hasattr(entry, "get") else None
            params = dict(entry.get("params", None) or {}) if target is not None else {}
            if target == _RESIZE:
                if not params.get("antialias", False):
                    raise L.VauraHipError(f"{_RESIZE} without antialias=true is not built (the kernel is the antialiased filter)")
                interp = str(params.get("interpolation", "bilinear")).lower()
                if interp not in ("bilinear", "interpolationmode.bilinear", "2"):
                    raise L.VauraHipError(f"{_RESIZE}: interpolation {params['interpolation']!r} is not built (bilinear only)")
                if params.get("max_size") is not None:
                    raise L.VauraHipError(f"{_RESIZE}: max_size is not built")
                kw["resize"] = params["size"]
            elif target == _CROP:
                kw["crop"] = params["size"]
            elif target in _TOFLOAT:
                if str(params.get("dtype", "float32")).replace("torch.", "") != "float32":
                    raise L.VauraHipError(f"{target}: dtype {params['dtype']!r} is not built (float32 only)")
                if target.endswith(".ToDtype") and not params.get("scale", False):
                    raise L.VauraHipError(f"{target} without scale=true leaves levels 0..255; the kernel scales by 1/255")
            elif target == _NORM:
                kw["mean"], kw["std"] = params["mean"], params["std"]
            else:
                raise L.VauraHipError(f"video transform {target!r} is not built; VideoPreprocessor takes {_RESIZE}, {_CROP}, "
                                      f"ToFloat32DType and {_NORM}")
            seen.append(_TOFLOAT[0] if target in _TOFLOAT else target)
        if seen != [_RESIZE, _CROP, _TOFLOAT[0], _NORM]:
            raise L.VauraHipError("video transforms must be Resize -> CenterCrop -> ToFloat32DType -> Normalize, in that order; got "
                                  f"{[str(t).rsplit('.', 1)[-1] for t in seen]}")
        return cls(**kw, **segment_kw)

    def geometry(self, H: int, W: int) -> _Geometry:
        if (H, W) not in self._geo:
            self._geo[(H, W)] = _Geometry(H, W, self.resize, self.crop)
        return self._geo[(H, W)]

    # ---- input handling
    def _clips(self, video) -> List[torch.Tensor]:
        """-> list of (b, T, C, H, W) / (b, T, H, W, C) uint8 tensors ((b, T, R, P) surfaces for a 4:2:0 format), one per clip or
        batch of one shape."""
        items = list(video) if isinstance(video, (list, tuple)) else [video]
        if not items:
            raise L.VauraHipError("VideoPreprocessor: no clips")
        yuv = self.input_format != "rgb"
        nd = 3 if yuv else 4                                               # dims of one clip
        out = []
        for v in items:
            if not torch.is_tensor(v):
                raise L.VauraHipError(f"VideoPreprocessor takes uint8 tensors, got {type(v).__name__}")
            if v.dtype != torch.uint8:
                if yuv:
                    raise L.VauraHipError(f"input_format={self.input_format!r} takes 8-bit surfaces (uint8); {v.dtype} (10-bit P010 and "
                                          "the like) is not built")
                raise L.VauraHipError(f"VideoPreprocessor takes decoded uint8 frames; a {v.dtype} input has been transformed already")
            if isinstance(video, (list, tuple)):
                if v.dim() != nd:
                    raise L.VauraHipError(f"clips of a list are {'(T, R, P) surfaces' if yuv else '(T, C, H, W) or (T, H, W, C)'}; "
                                          f"got {tuple(v.shape)}")
                v = v[None]
            elif v.dim() == nd:
                v = v[None]
            elif v.dim() != nd + 1:
                if yuv:
                    raise L.VauraHipError(f"{self.input_format} video must be (B, T, R, P) or (T, R, P) surfaces; got {tuple(v.shape)}")
                raise L.VauraHipError(f"video must be (B, T, C, H, W) or (T, C, H, W) (channels last: (.., H, W, C)); got {tuple(v.shape)}")
            out.append(v)
        return out

    def _dims(self, v: torch.Tensor) -> Tuple[int, int, int, int, int]:
        b, T = v.shape[:2]
        C, H, W = (v.shape[4], v.shape[2], v.shape[3]) if self.channels_last else tuple(v.shape[2:])
        if C != 3:
            raise L.VauraHipError(f"video has {C} channels ({'last' if self.channels_last else 'first'} layout expected); 3 are needed")
        return b, T, C, H, W

    # ---- the frame rate
    @staticmethod
    def _rates(src_fps):
        """None, one rate, or a list of per-clip rates (a tuple is ``(num, den)``)."""
        if src_fps is None:
            return None
        return [as_rate(r) for r in src_fps] if isinstance(src_fps, list) else as_rate(src_fps)

    def _plans(self, clips: List[torch.Tensor], src_fps, pts, time_base, end) -> Optional[List[FpsPlan]]:
        """One ``fps_plan`` per clip of the call (the rows of ``clips`` in order), or None where the frames are at ``dst_fps``
        already and the launch is the one without a table."""
        rows = [int(v.shape[1]) for v in clips for _ in range(v.shape[0])]
        rates = self.src_fps if src_fps is None else self._rates(src_fps)
        if pts is None:
            if time_base is not None or end is not None:
                raise L.VauraHipError("time_base / end describe pts; pass pts")
            if isinstance(rates, list):
                if len(rates) != len(rows):
                    raise L.VauraHipError(f"{len(rates)} rates for {len(rows)} clips")
            else:
                rates = [rates] * len(rows)
            if all(r is None or r == self.dst_fps for r in rates):
                return None
            return [fps_plan(T, self.dst_fps if r is None else r, dst_fps=self.dst_fps) for T, r in zip(rows, rates)]
        if rates is not None:
            raise L.VauraHipError("pts and src_fps both describe the frames' times; pass one of them")
        if time_base is None:
            raise L.VauraHipError("pts are in units of time_base; pass time_base")
        per_clip = len(pts) > 0 and not isinstance(pts[0], (int, np.integer)) and not (torch.is_tensor(pts[0]) and pts[0].dim() == 0)
        pts = list(pts) if per_clip else [pts] * len(rows)
        ends = list(end) if isinstance(end, (list, tuple)) else [end] * len(rows)
        if len(pts) != len(rows) or len(ends) != len(rows):
            raise L.VauraHipError(f"{len(pts)} pts lists and {len(ends)} ends for {len(rows)} clips")
        for T, p in zip(rows, pts):
            if len(p) != T:
                raise L.VauraHipError(f"{len(p)} pts for a clip of {T} frames")
        return [fps_plan(pts=p, time_base=time_base, end=e, dst_fps=self.dst_fps) for p, e in zip(pts, ends)]

    def _frame_maps(self, plans: List[FpsPlan]) -> Tuple[int, List[np.ndarray]]:
        """(S, per clip the (S * F,) source frames of its output frames): the segments are cut from the CONVERTED sequence of
        ``n_out`` frames, output (s, f) takes ``table[first + s * stride + f]``."""
        F = self.segment_size_vframes
        maps, Ss, done = [], [], {}
        for p in plans:
            if id(p) not in done:                                           # the clips of a batch mostly share one plan
                S, first, stride = segment_starts(p.n_out, F, self.step_size_seg, self.n_segments)
                idx = first + stride * np.arange(S)[:, None] + np.arange(F)[None, :]
                done[id(p)] = (S, p.table[idx.reshape(-1)].astype(np.int32))
            Ss.append(done[id(p)][0])
            maps.append(done[id(p)][1])
        if len(set(Ss)) != 1:
            raise L.VauraHipError(f"clips of one call must give the same number of segments; at {float(self.dst_fps):g} fps they give {Ss}")
        return Ss[0], maps

    # ---- CPU restatement
    def reference_u8(self, video, size: Optional[Tuple[int, int]] = None, chroma_row: Optional[int] = None, src_fps=None, pts=None,
                     time_base=None, end=None) -> torch.Tensor:
        """The kernel's integer arithmetic on the CPU with the same tap tables: uint8 levels (B, S, C, F, h, w) before the scaling.
        A 4:2:0 input goes through ``yuv420_to_rgb_u8`` first (``size`` / ``chroma_row`` as in ``__call__``).  With a frame rate
        (``src_fps`` / ``pts``, as in ``__call__``) every clip is ``video[table]`` first."""
        outs = []
        clips = self._clips(video)
        plans = self._plans(clips, src_fps, pts, time_base, end)
        if plans is not None:
            rows = [v[i:i + 1] for v in clips for i in range(v.shape[0])]
            clips = [r.cpu().index_select(1, torch.from_numpy(p.table.astype(np.int64))) for r, p in zip(rows, plans)]
        for v in clips:
            if self.input_format != "rgb":
                v = yuv420_to_rgb_u8(*yuv420_planes(v.cpu(), self.input_format, size, chroma_row), self.color_matrix, self.color_range)
            b, T, C, H, W = self._dims(v)
            g = self.geometry(H, W)
            S, first, stride = segment_starts(T, self.segment_size_vframes, self.step_size_seg, self.n_segments)
            x = v.cpu()
            if self.channels_last:
                x = x.permute(0, 1, 4, 2, 3)
            # rows the kept output rows need, then both passes (horizontal first, uint8 in between)
            y0, y1 = int(g.v["start"].min()), int(g.v["start"].max()) + g.v["taps"]
            x = x[..., y0:y1, :].to(torch.int32)
            x = _resample_axis(x, g.h, -1)
            vt = dict(g.v, start=g.v["start"] - y0)
            x = _resample_axis(x, vt, -2).to(torch.uint8)                   # (b, T, C, h, w)
            F = self.segment_size_vframes
            seg = torch.stack([x[:, first + s * stride: first + s * stride + F] for s in range(S)], dim=1)   # (b, S, F, C, h, w)
            outs.append(seg.permute(0, 1, 3, 2, 4, 5).contiguous())
        return self._cat(outs)

    def scale_normalize(self, u8: torch.Tensor) -> torch.Tensor:
        """uint8 levels (B, S, C, F, h, w) -> ``((u8 / 255) - mean) / std`` in fp32, in that order (CPU)."""
        x = u8.cpu().to(torch.float32) / 255
        m = torch.tensor(self.mean, dtype=torch.float32).view(1, 1, 3, 1, 1, 1)
        s = torch.tensor(self.std, dtype=torch.float32).view(1, 1, 3, 1, 1, 1)
        return (x - m) / s

    @staticmethod
    def _cat(outs: List[torch.Tensor]) -> torch.Tensor:
        if len({tuple(o.shape[1:]) for o in outs}) != 1:
            raise L.VauraHipError(f"clips of one call must give the same number of segments; got shapes {[tuple(o.shape) for o in outs]}")
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)

    # ---- device path
    def _check_map(self, fmap: np.ndarray, b: int, T: int, S: int, carry) -> bool:
        """Every refusal about a (b, S * F) frame map, on the host; -> whether it names the carried frame."""
        if fmap.dtype != np.int32 or fmap.shape != (b, S * self.segment_size_vframes):
            raise L.VauraHipError(f"a frame map is int32 (clips, S * F) = {(b, S * self.segment_size_vframes)}; got {fmap.dtype} {fmap.shape}")
        if fmap.size and (int(fmap.min()) < MAP_CARRY or int(fmap.max()) >= T):
            raise L.VauraHipError(f"a frame map names source frames 0 .. {T - 1}, -1 (keep) or -2 (the carried frame); got "
                                  f"{int(fmap.min())} .. {int(fmap.max())}")
        uses = bool((fmap == MAP_CARRY).any())
        if uses and carry is None:
            raise L.VauraHipError("the frame map names the carried frame (-2) and there is none")
        return uses

    def _device_map(self, fmap: np.ndarray, dev: torch.device) -> torch.Tensor:
        """The map on the device.  Kept per content: a constant rate gives the same few maps call after call and push after push,
        and the upload (a synchronous copy of a few hundred bytes) costs as much host time as the launch."""
        key = (str(dev), fmap.shape, fmap.tobytes())
        if key not in self._map_dev:
            if len(self._map_dev) >= 256:
                self._map_dev.clear()
            self._map_dev[key] = torch.from_numpy(np.ascontiguousarray(fmap)).to(dev)
        return self._map_dev[key]

    def _launch(self, v: torch.Tensor, out: torch.Tensor, dev: torch.device, fmap: Optional[np.ndarray] = None,
                carry: Optional[torch.Tensor] = None) -> None:
        b, T, C, H, W = self._dims(v)
        g = self.geometry(H, W)
        if fmap is not None:                                               # the table launch: the map has the segments applied
            S = out.shape[1]
            uses = self._check_map(fmap, b, T, S, carry)
            if tuple(out.shape) != (b, S, 3, self.segment_size_vframes, *self.crop) or not out.is_contiguous():
                raise L.VauraHipError(f"the output of {b} clips is (b, S, 3, F, h, w) and contiguous; got {tuple(out.shape)}")
            if carry is not None and (tuple(carry.shape) != (b, *v.shape[2:]) or not carry.is_contiguous() or carry.dtype != torch.uint8):
                raise L.VauraHipError(f"the carried frames are uint8 {(b, *v.shape[2:])}; got {carry.dtype} {tuple(carry.shape)}")
            tile_rows, tile_src = g.tiles(self.channels_last)
            h_rel, h_w, v_start, v_w = g.device_tables(dev)
            key = str(dev)
            if key not in self._lut_dev:
                self._lut_dev[key] = self.lut.to(dev)
            dmap = self._device_map(fmap, dev)
            L.check(L.lib().vaura_video_preprocess_frames(
                L.ptr(v), int(self.channels_last), b, T, C, H, W, self.resize, self.crop[0], self.crop[1], self.segment_size_vframes, S,
                L.ptr(h_rel), L.ptr(h_w), g.h["taps"], g.h["prec"], L.ptr(v_start), L.ptr(v_w), g.v["taps"], g.v["prec"], g.x0, g.span,
                tile_rows, tile_src, L.ptr(self._lut_dev[key]), L.ptr(out), L.ptr(dmap), L.ptr(carry), int(uses),
                L.current_stream(dev)), "vaura_video_preprocess_frames")
            return
        S, first, stride = segment_starts(T, self.segment_size_vframes, self.step_size_seg, self.n_segments)
        if tuple(out.shape) != (b, S, 3, self.segment_size_vframes, *self.crop):
            raise L.VauraHipError(f"clips of one call must give the same number of segments; this group gives {S}, the first {out.shape[1]}")
        tile_rows, tile_src = g.tiles(self.channels_last)
        h_rel, h_w, v_start, v_w = g.device_tables(dev)
        key = str(dev)
        if key not in self._lut_dev:
            self._lut_dev[key] = self.lut.to(dev)
        L.check(L.lib().vaura_video_preprocess(
            L.ptr(v), int(self.channels_last), b, T, C, H, W, self.resize, self.crop[0], self.crop[1], self.segment_size_vframes, S,
            first, stride, L.ptr(h_rel), L.ptr(h_w), g.h["taps"], g.h["prec"], L.ptr(v_start), L.ptr(v_w), g.v["taps"], g.v["prec"],
            g.x0, g.span, tile_rows, tile_src, L.ptr(self._lut_dev[key]), L.ptr(out), L.current_stream(dev)), "vaura_video_preprocess")

    def _launch_yuv(self, v: torch.Tensor, out: torch.Tensor, dev: torch.device, size, chroma_row, fmap: Optional[np.ndarray] = None,
                    carry: Optional[torch.Tensor] = None) -> None:
        b, T = v.shape[:2]
        H, W, R, P, crow = yuv_surface(v, self.input_format, size, chroma_row)
        # frame n = clip * T + t sits at byte n * frame_stride: true of a contiguous batch and of the usual views of one
        fs = v.stride(1) if T > 1 else (v.stride(0) if b > 1 else R * P)
        if fs < R * P or (b > 1 and T > 1 and v.stride(0) != T * fs) or (carry is not None and fs != R * P):
            v = v.contiguous()
            fs = R * P
        g = self.geometry(H, W)
        if fmap is not None:                                               # the table launch: the map has the segments applied
            S = out.shape[1]
            uses = self._check_map(fmap, b, T, S, carry)
            if tuple(out.shape) != (b, S, 3, self.segment_size_vframes, *self.crop) or not out.is_contiguous():
                raise L.VauraHipError(f"the output of {b} clips is (b, S, 3, F, h, w) and contiguous; got {tuple(out.shape)}")
            if carry is not None and (tuple(carry.shape) != (b, R, P) or not carry.is_contiguous() or carry.dtype != torch.uint8):
                raise L.VauraHipError(f"the carried surfaces are uint8 {(b, R, P)}; got {carry.dtype} {tuple(carry.shape)}")
            tile_rows, tile_src = g.tiles(False, self.input_format)
            h_rel, h_w, v_start, v_w = g.device_tables(dev)
            key = str(dev)
            if key not in self._lut_dev:
                self._lut_dev[key] = self.lut.to(dev)
            dmap = self._device_map(fmap, dev)
            L.check(L.lib().vaura_video_preprocess_yuv420_frames(
                L.ptr(v), (b * T - 1) * fs + R * P, _YUV_LAYOUT[self.input_format], P, crow * P, fs, b, T, H, W, *self.yuv, self.resize,
                self.crop[0], self.crop[1], self.segment_size_vframes, S, L.ptr(h_rel), L.ptr(h_w), g.h["taps"], g.h["prec"],
                L.ptr(v_start), L.ptr(v_w), g.v["taps"], g.v["prec"], g.x0, g.span, tile_rows, tile_src, L.ptr(self._lut_dev[key]),
                L.ptr(out), L.ptr(dmap), L.ptr(carry), int(uses), L.current_stream(dev)), "vaura_video_preprocess_yuv420_frames")
            return
        S, first, stride = segment_starts(T, self.segment_size_vframes, self.step_size_seg, self.n_segments)
        if tuple(out.shape) != (b, S, 3, self.segment_size_vframes, *self.crop):
            raise L.VauraHipError(f"clips of one call must give the same number of segments; this group gives {S}, the first {out.shape[1]}")
        tile_rows, tile_src = g.tiles(False, self.input_format)
        h_rel, h_w, v_start, v_w = g.device_tables(dev)
        key = str(dev)
        if key not in self._lut_dev:
            self._lut_dev[key] = self.lut.to(dev)
        L.check(L.lib().vaura_video_preprocess_yuv420(
            L.ptr(v), (b * T - 1) * fs + R * P, _YUV_LAYOUT[self.input_format], P, crow * P, fs, b, T, H, W, *self.yuv, self.resize,
            self.crop[0], self.crop[1], self.segment_size_vframes, S, first, stride, L.ptr(h_rel), L.ptr(h_w), g.h["taps"], g.h["prec"],
            L.ptr(v_start), L.ptr(v_w), g.v["taps"], g.v["prec"], g.x0, g.span, tile_rows, tile_src, L.ptr(self._lut_dev[key]),
            L.ptr(out), L.current_stream(dev)), "vaura_video_preprocess_yuv420")

    @torch.no_grad()
    def __call__(self, video, size: Optional[Tuple[int, int]] = None, chroma_row: Optional[int] = None, *, src_fps=None, pts=None,
                 time_base=None, end=None) -> torch.Tensor:
        """uint8 (B, T, C, H, W), (T, C, H, W) or a list of per-clip (T, C, H, W) tensors whose H, W may differ (channels last:
        (.., H, W, C)) -> fp32 (B, S, C, F, crop_h, crop_w) on the device.  Host tensors are copied once, as uint8.

        ``input_format`` "nv12" / "i420": uint8 (B, T, R, P), (T, R, P) or a list of per-clip (T, R, P) surfaces.  Tight frames have
        R = 3H/2 rows of P = W bytes (H rows of luma, then the chroma plane).  A padded decoder surface passes ``size=(H, W)``: P >= W
        is the pitch, luma sits in rows [0, H), the chroma plane starts at row ``chroma_row`` (default H) and R >= chroma_row + H/2;
        bytes outside the planes never reach the result.  Host surfaces are copied once, as they are (1.5 bytes per pixel).

        Video that is not at ``dst_fps``: the preprocessor's ``src_fps`` (or ``src_fps=`` here; a list: one rate per clip), or
        ``pts`` (integers in units of ``time_base``, strictly increasing; one list for all clips or one per clip) with an optional
        ``end``.  The frames are selected by ``fps_plan`` and the segments are cut from the selected sequence, in the same single
        launch per geometry (``vaura_video_preprocess_frames``); of a host input only the selected frames are copied."""
        yuv = self.input_format != "rgb"
        if not yuv and (size is not None or chroma_row is not None):
            raise L.VauraHipError("size / chroma_row describe a 4:2:0 surface; input_format is 'rgb'")
        clips = self._clips(video)
        plans = self._plans(clips, src_fps, pts, time_base, end)
        if plans is not None:
            return self._call_fps(clips, plans, size, chroma_row)
        # one launch per run of consecutive clips of one geometry (the output keeps the clips' order)
        groups: List[List[torch.Tensor]] = []
        for v in clips:
            if groups and tuple(groups[-1][0].shape[1:]) == tuple(v.shape[1:]):
                groups[-1].append(v)
            else:
                groups.append([v])
        for grp in groups:                                                   # every refusal before any device work
            if yuv:
                T = grp[0].shape[1]
                for v in grp:
                    H, W = yuv_surface(v, self.input_format, size, chroma_row)[:2]
            else:
                _, T, _, H, W = self._dims(grp[0])
            self.geometry(H, W)
            segment_starts(T, self.segment_size_vframes, self.step_size_seg, self.n_segments)
        dev = self._device_for(clips)
        S = segment_starts(clips[0].shape[1], self.segment_size_vframes, self.step_size_seg, self.n_segments)[0]
        B = sum(v.shape[0] for v in clips)
        with torch.cuda.device(dev):
            out = torch.empty(B, S, 3, self.segment_size_vframes, *self.crop, dtype=torch.float32, device=dev)
            b0 = 0
            for grp in groups:
                grp = [v.to(dev, non_blocking=True) for v in grp]               # uint8 over the link, once
                if yuv:
                    v = grp[0] if len(grp) == 1 else torch.cat(grp, dim=0)      # a single surface stays the view it is
                    self._launch_yuv(v, out[b0:b0 + v.shape[0]], dev, size, chroma_row)
                else:
                    v = (grp[0] if len(grp) == 1 else torch.cat(grp, dim=0)).contiguous()
                    self._launch(v, out[b0:b0 + v.shape[0]], dev)              # same stream as the copy: v may be freed after it
                b0 += v.shape[0]
        return out

    def _device_for(self, clips: Sequence[torch.Tensor]) -> torch.device:
        dev = self.device
        if dev is None:
            dev = next((v.device for v in clips if v.device.type == "cuda"), None)
            if dev is None:
                if not torch.cuda.is_available():
                    raise L.VauraHipError("VideoPreprocessor runs on a HIP device only (reference_u8 is the CPU restatement)")
                dev = torch.device("cuda", torch.cuda.current_device())
        return dev

    @staticmethod
    def _upload_named(v: torch.Tensor, used: np.ndarray, dev: torch.device) -> torch.Tensor:
        """The frames ``used`` (sorted) of the host clips ``v`` (b, T, ..) on the device, (b, len(used), ..): one copy per clip and run
        of consecutive frames, straight from where they lie (a gather on the host first would cost more than the link saves)."""
        dst = torch.empty(v.shape[0], len(used), *v.shape[2:], dtype=v.dtype, device=dev)
        cuts = np.flatnonzero(np.diff(used) != 1) + 1
        at = 0
        for run in np.split(used, cuts):
            for i in range(v.shape[0]):
                dst[i, at:at + len(run)].copy_(v[i, int(run[0]):int(run[-1]) + 1], non_blocking=True)
            at += len(run)
        return dst

    def _call_fps(self, clips: List[torch.Tensor], plans: List[FpsPlan], size, chroma_row) -> torch.Tensor:
        """``__call__`` for video at its own frame rate: one table launch per run of consecutive clips of one geometry."""
        yuv = self.input_format != "rgb"
        F = self.segment_size_vframes
        S, maps = self._frame_maps(plans)                                    # refuses clips too short for a segment at dst_fps
        items, r0 = [], 0                                                     # (frames, (b, S * F) map) per input tensor
        for v in clips:
            b = v.shape[0]
            fmap = np.stack(maps[r0:r0 + b])
            r0 += b
            if yuv:
                H, W = yuv_surface(v, self.input_format, size, chroma_row)[:2]
            else:
                H, W = self._dims(v)[3:]
            self.geometry(H, W)
            if v.device.type != "cuda":                                      # only the frames the table names cross the link
                used = np.unique(fmap)
                fmap = np.searchsorted(used, fmap).astype(np.int32)
            else:
                used = None
            items.append((v, fmap, used))
        shape_of = lambda it: (it[0].shape[1] if it[2] is None else len(it[2]), *it[0].shape[2:])  # noqa: E731  (frames on the device, ..)
        groups: List[list] = []
        for it in items:
            if groups and shape_of(groups[-1][0]) == shape_of(it):
                groups[-1].append(it)
            else:
                groups.append([it])
        dev = self._device_for(clips)
        B = sum(v.shape[0] for v in clips)
        with torch.cuda.device(dev):
            out = torch.empty(B, S, 3, F, *self.crop, dtype=torch.float32, device=dev)
            b0 = 0
            for grp in groups:
                vs = [v.to(dev, non_blocking=True) if used is None else self._upload_named(v, used, dev) for v, _, used in grp]
                fmap = np.concatenate([m for _, m, _ in grp])
                if yuv:
                    v = vs[0] if len(vs) == 1 else torch.cat(vs, dim=0)
                    self._launch_yuv(v, out[b0:b0 + v.shape[0]], dev, size, chroma_row, fmap=fmap)
                else:
                    v = (vs[0] if len(vs) == 1 else torch.cat(vs, dim=0)).contiguous()
                    self._launch(v, out[b0:b0 + v.shape[0]], dev, fmap=fmap)
                b0 += v.shape[0]
        return out

    def open_stream(self, batch: int, *, src_fps=None, time_base=None, size=None, chroma_row=None) -> "VideoFrameStream":
        """A ``VideoFrameStream`` of ``batch`` clips on this preprocessor: ``src_fps`` (default: the preprocessor's) or ``time_base``."""
        if src_fps is None and time_base is None:
            src_fps = self.src_fps if self.src_fps is not None else self.dst_fps
        return VideoFrameStream(self, batch, src_fps=src_fps, time_base=time_base, size=size, chroma_row=chroma_row)


class VideoFrameStream:
    """Decoded frames at their own rate in, complete 25 fps segments out: what ``LiveSession.push(frames=)`` takes.

        vs = pre.open_stream(batch, src_fps=30)            # or time_base=(1, 90000) and pts with every push
        for seg in vs.push(frames, pts): ...                # frames (B, n, ..) uint8, any n >= 0; seg (B, 1, 3, F, h, w) fp32
        for seg in vs.close(): ...                          # what the end of the video completes; vs.dropped_ticks = the cut tail

    The selection is ``FpsClock`` (all clips of a stream share their frame times); segment s holds the ticks
    ``[r_0 + s F, r_0 + (s + 1) F)``, so the segments are those of the one-pass call on the whole video with ``step_size_seg == 1``
    (anything else is refused).  Device state: the pending segment and, per clip, the last frame received — it may still be shown
    at later ticks.  A push launches once per segment it touches, into the pending segment itself: map value -1 keeps the ticks
    filled earlier, -2 names the carried frame, so old and new frames are never concatenated."""

    def __init__(self, pre: VideoPreprocessor, batch: int, *, src_fps=None, time_base=None, size=None, chroma_row=None):
        if pre.step_size_seg != 1.0 or pre.n_segments is not None:
            raise L.VauraHipError("a frame stream makes back-to-back segments: step_size_seg == 1.0 and n_segments None; got "
                                  f"{pre.step_size_seg} and {pre.n_segments}")
        if isinstance(src_fps, list):
            raise L.VauraHipError("the clips of a stream share one clock: one src_fps, not a list")
        if batch < 1:
            raise L.VauraHipError(f"a stream of {batch} clips")
        if pre.input_format == "rgb" and (size is not None or chroma_row is not None):
            raise L.VauraHipError("size / chroma_row describe a 4:2:0 surface; input_format is 'rgb'")
        self.pre, self.batch, self.size, self.chroma_row = pre, int(batch), size, chroma_row
        self.clock = FpsClock(src_fps, time_base=time_base, dst_fps=pre.dst_fps)
        self.segments, self.dropped_ticks, self.closed = 0, 0, False
        self._filled = 0                                                 # ticks of the pending segment that are written
        self._frame_shape: Optional[Tuple[int, ...]] = None
        self._pending: Optional[torch.Tensor] = None
        self._carry: Optional[torch.Tensor] = None
        self._dev: Optional[torch.device] = None

    def _check(self, frames, pts) -> torch.Tensor:
        pre = self.pre
        nd = 2 if pre.input_format != "rgb" else 3                        # dims of one frame
        if not torch.is_tensor(frames) or frames.dtype != torch.uint8:
            raise L.VauraHipError("a frame stream takes decoded uint8 frames")
        if frames.dim() == nd + 1 and self.batch == 1:
            frames = frames[None]
        if frames.dim() != nd + 2 or frames.shape[0] != self.batch:
            raise L.VauraHipError(f"a push is (B = {self.batch}, n, ..) frames in the preprocessor's input layout; got {tuple(frames.shape)}")
        if self._frame_shape is not None and tuple(frames.shape[2:]) != self._frame_shape:
            raise L.VauraHipError(f"a stream has one geometry: frames of {self._frame_shape}, then {tuple(frames.shape[2:])}")
        if self.clock.src_fps is not None:
            if pts is not None:
                raise L.VauraHipError("a constant-rate stream takes no pts (open it with time_base= for timestamped frames)")
        elif pts is None or len(pts) != frames.shape[1]:
            raise L.VauraHipError(f"a timestamped stream takes one pts per frame; {frames.shape[1]} frames, "
                                  f"{'no' if pts is None else len(pts)} pts")
        return frames

    def _emit(self, decided: List[Tuple[int, int]], base: int, v: torch.Tensor) -> List[torch.Tensor]:
        """Write the decided ticks: source frame ``i`` is ``v[:, i - base]``, or the carried frame for ``i == base - 1``."""
        pre, F, out = self.pre, self.pre.segment_size_vframes, []
        at = 0
        while at < len(decided):
            n = min(F - self._filled, len(decided) - at)                  # the ticks of this launch: up to the segment's end
            row = np.full(F, MAP_KEEP, np.int32)
            for j, (tick, i) in enumerate(decided[at:at + n]):
                assert (tick - self.clock.first_tick) % F == self._filled + j and i >= base - 1
                row[self._filled + j] = i - base if i >= base else MAP_CARRY
            fmap = np.tile(row, (self.batch, 1))
            if pre.input_format != "rgb":
                pre._launch_yuv(v, self._pending, self._dev, self.size, self.chroma_row, fmap=fmap, carry=self._carry)
            else:
                pre._launch(v, self._pending, self._dev, fmap=fmap, carry=self._carry)
            self._filled += n
            at += n
            if self._filled == F:                                         # complete: handed over, a new buffer takes its place
                out.append(self._pending)
                self._pending = torch.empty_like(self._pending)
                self._filled = 0
                self.segments += 1
        return out

    @torch.no_grad()
    def push(self, frames: torch.Tensor, pts=None) -> List[torch.Tensor]:
        """``frames``: uint8 (B, n, C, H, W) / (B, n, H, W, C) / (B, n, R, P) surfaces, n >= 0 ((n, ..) with B == 1); ``pts``: their n
        timestamps on a ``time_base`` stream.  -> the segments (B, 1, 3, F, h, w) fp32 this push completed, oldest first."""
        if self.closed:
            raise L.VauraHipError("VideoFrameStream.push after close")
        frames = self._check(frames, pts)
        pre = self.pre
        if self._frame_shape is None:                                     # every refusal about the geometry, before any state
            if pre.input_format != "rgb":
                H, W = yuv_surface(frames, pre.input_format, self.size, self.chroma_row)[:2]
            else:
                H, W = pre._dims(frames)[3:]
            pre.geometry(H, W)
        n = int(frames.shape[1])
        base = self.clock.n
        decided = self.clock.push(n if self.clock.src_fps is not None else pts)
        if n == 0:
            return []
        if self._frame_shape is None:
            self._frame_shape = tuple(frames.shape[2:])
            self._dev = pre._device_for([frames])
            with torch.cuda.device(self._dev):
                self._pending = torch.empty(self.batch, 1, 3, pre.segment_size_vframes, *pre.crop, dtype=torch.float32, device=self._dev)
                self._carry = torch.empty(self.batch, *self._frame_shape, dtype=torch.uint8, device=self._dev)
        with torch.cuda.device(self._dev):
            v = frames.to(self._dev, non_blocking=True).contiguous()
            out = self._emit(decided, base, v)
            self._carry.copy_(v[:, -1])                                   # behind the launches that read the frame carried so far
        return out

    @torch.no_grad()
    def close(self, end=None) -> List[torch.Tensor]:
        """The segments the end of the video completes (``end``: its pts on a ``time_base`` stream, see ``FpsClock.close``).  A
        trailing incomplete segment is dropped; ``dropped_ticks`` says how many ticks it held."""
        if self.closed:
            raise L.VauraHipError("VideoFrameStream.close called twice")
        decided = self.clock.close(end)
        self.closed = True
        out = []
        if self._carry is not None:
            with torch.cuda.device(self._dev):
                out = self._emit(decided, self.clock.n, self._carry[:, None])   # every remaining tick shows the last frame
        self.dropped_ticks = self._filled
        self._pending = self._carry = None
        return out
