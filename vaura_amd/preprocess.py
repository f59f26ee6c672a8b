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
"""
from __future__ import annotations

import math
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
                 input_format: str = "rgb", color_matrix: str = "bt601", color_range: str = "limited"):
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

    # ---- CPU restatement
    def reference_u8(self, video, size: Optional[Tuple[int, int]] = None, chroma_row: Optional[int] = None) -> torch.Tensor:
        """The kernel's integer arithmetic on the CPU with the same tap tables: uint8 levels (B, S, C, F, h, w) before the scaling.
        A 4:2:0 input goes through ``yuv420_to_rgb_u8`` first (``size`` / ``chroma_row`` as in ``__call__``)."""
        outs = []
        for v in self._clips(video):
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
    def _launch(self, v: torch.Tensor, out: torch.Tensor, dev: torch.device) -> None:
        b, T, C, H, W = self._dims(v)
        g = self.geometry(H, W)
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

    def _launch_yuv(self, v: torch.Tensor, out: torch.Tensor, dev: torch.device, size, chroma_row) -> None:
        b, T = v.shape[:2]
        H, W, R, P, crow = yuv_surface(v, self.input_format, size, chroma_row)
        # frame n = clip * T + t sits at byte n * frame_stride: true of a contiguous batch and of the usual views of one
        fs = v.stride(1) if T > 1 else (v.stride(0) if b > 1 else R * P)
        if fs < R * P or (b > 1 and T > 1 and v.stride(0) != T * fs):
            v = v.contiguous()
            fs = R * P
        g = self.geometry(H, W)
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
    def __call__(self, video, size: Optional[Tuple[int, int]] = None, chroma_row: Optional[int] = None) -> torch.Tensor:
        """uint8 (B, T, C, H, W), (T, C, H, W) or a list of per-clip (T, C, H, W) tensors whose H, W may differ (channels last:
        (.., H, W, C)) -> fp32 (B, S, C, F, crop_h, crop_w) on the device.  Host tensors are copied once, as uint8.

        ``input_format`` "nv12" / "i420": uint8 (B, T, R, P), (T, R, P) or a list of per-clip (T, R, P) surfaces.  Tight frames have
        R = 3H/2 rows of P = W bytes (H rows of luma, then the chroma plane).  A padded decoder surface passes ``size=(H, W)``: P >= W
        is the pitch, luma sits in rows [0, H), the chroma plane starts at row ``chroma_row`` (default H) and R >= chroma_row + H/2;
        bytes outside the planes never reach the result.  Host surfaces are copied once, as they are (1.5 bytes per pixel)."""
        yuv = self.input_format != "rgb"
        if not yuv and (size is not None or chroma_row is not None):
            raise L.VauraHipError("size / chroma_row describe a 4:2:0 surface; input_format is 'rgb'")
        clips = self._clips(video)
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
        dev = self.device
        if dev is None:
            dev = next((v.device for v in clips if v.device.type == "cuda"), None)
            if dev is None:
                if not torch.cuda.is_available():
                    raise L.VauraHipError("VideoPreprocessor runs on a HIP device only (reference_u8 is the CPU restatement)")
                dev = torch.device("cuda", torch.cuda.current_device())
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
