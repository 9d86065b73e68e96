"""EvalSession — the reference's primary entry (src/eval/session.rs:281-497), batched for the device.

Same names, argument meaning and error behaviour as the reference; what differs is the schedule:
the reference scores one (codec, quality) cell at a time on the calling thread (session.rs:375-410),
here every cell of an image — or of a whole corpus — is encoded/decoded first, then all decoded
images go to the device as ONE batch per shape (reference uploaded once per image, decoder output
converted to RGB8 on the device), and the scores are filled into the same `CodecResult` rows in the
reference's loop order.  Report types and writers are in `reports.py`.
"""
from __future__ import annotations

import os
import time
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import (ColourDescription, GainMap, HlgDescription, DEEP_DEPTHS, PIXEL_RGB_F32, PIXEL_RGB8, PIXEL_RGB16, PIXEL_RGBA8, PIXEL_RGBA16, Batch, CodecEvalError, ColorTable, Context, IccLutProfile, IccProfile, icc_describe, icc_lut_describe, DimensionMismatch, MetricCalculation,
               MetricConfig, MetricResult, _error_obj, estimate_batch_bytes, CE_ERR_BACKEND)
from . import RESAMPLE_LANCZOS3
from . import CHROMA_TRIANGLE, MEM_HOST, YUV_400, YUV_420, YUV_444, YUV_BT601, YUV_FULL, YUV_PLANAR, YUV_SEMIPLANAR, YuvImage, yuv_coefficients
from . import QUANT_NEAREST_EVEN, TensorImage, quantise_tensor
from . import ALPHA_BLACK_WHITE, ALPHA_BLEND_LINEAR, MAX_BACKGROUNDS, PIXEL_RGBA_F32, composite_over, scale_background, srgb_table
from . import reports as R
from .viewing import SimulationMode, ViewingCondition

__all__ = ["ImageData", "EncodeRequest", "EvalConfig", "EvalConfigBuilder", "EvalSession", "ALPHA_BLACK_WHITE", "ALPHA_BLEND_LINEAR"]


Colour = Union[ColourDescription, HlgDescription]  # what colour= takes: H.273 code points, or BT.2100 HLG with its display


def _gain_map_for(gain_map: Optional[GainMap], colour: Optional["Colour"], width: int, height: int) -> Optional[GainMap]:
    """A constructor's gain_map=: a GainMap no larger than the image, whose base a ColourDescription (or none: sRGB) reads."""
    if gain_map is None:
        return None
    if not isinstance(gain_map, GainMap):
        raise TypeError("gain_map= takes a GainMap")
    if isinstance(colour, HlgDescription):
        raise ValueError("a gain map's base image is read by a ColourDescription, not an HlgDescription")
    gh, gw = gain_map.samples.shape[:2]
    if not (1 <= gw <= int(width) and 1 <= gh <= int(height)):
        raise ValueError(f"a gain map of {gw} x {gh} for an image of {width} x {height}: it must be 1 x 1 at least and the image's size at most")
    return gain_map


def _colour_at(colour: Optional[Colour], depth: int) -> Optional[Colour]:
    """A constructor's colour= at the image's own depth (a preset names primaries and transfer; the samples say the depth)."""
    return None if colour is None else colour.with_depth(int(depth))


@dataclass
class ImageData:
    """session.rs:25-149.  `RgbSlice`, `RgbaSlice`, `RgbSliceWithIcc` (the imgref variants carry the same bytes)."""
    data: np.ndarray  # packed u8, RGB or RGBA (depth 0); packed u16 of `depth` bits per sample for a deep image
    width: int
    height: int
    channels: int = 3
    icc_profile: Optional[bytes] = None
    depth: int = 0  # 0: 8-bit samples in u8; 8, 10, 12 or 16: a deep image (rgb16 / rgba16), scored at its own precision
    yuv_image: Optional[YuvImage] = None  # a decode still in its Y'CbCr planes (ImageData.yuv); `data` is then empty
    # How the code values are to be read (H.273 primaries / transfer; its depth is this image's): None = sRGB, as ever.  A
    # decode with a non-sRGB description is scored in linear light through a linear batch.
    colour: Optional[Colour] = None
    linear: bool = False  # `data` is packed float32 RGB, linear light with sRGB primaries (ImageData.linear_f32)
    # `data` is the SDR base of a gain-map image (Ultra HDR JPEG, gain-map AVIF / HEIC / JPEG XL) and this its map with the
    # metadata: the HDR rendition is scored, in linear light.  Not with an HlgDescription.
    gain_map: Optional[GainMap] = None
    premultiplied: bool = False  # a linear RGBA image whose colour samples already hold colour * coverage
    tensor_image: Optional[TensorImage] = None  # a framework's tensor as it is (ImageData.tensor); `data` is then empty

    @staticmethod
    def rgb(data, width: int, height: int, colour: Optional[Colour] = None, gain_map: Optional[GainMap] = None) -> "ImageData":
        return ImageData(np.ascontiguousarray(data, dtype=np.uint8).reshape(-1), int(width), int(height), 3, colour=_colour_at(colour, 8),
                         gain_map=_gain_map_for(gain_map, colour, width, height))

    @staticmethod
    def rgba(data, width: int, height: int, colour: Optional[Colour] = None, gain_map: Optional[GainMap] = None) -> "ImageData":
        return ImageData(np.ascontiguousarray(data, dtype=np.uint8).reshape(-1), int(width), int(height), 4, colour=_colour_at(colour, 8),
                         gain_map=_gain_map_for(gain_map, colour, width, height))

    @staticmethod
    def linear_f32(data, width: int, height: int, channels: int = 3, premultiplied: bool = False) -> "ImageData":
        """Packed float32 RGB in linear light with BT.709 / sRGB primaries, 1.0 = the white an 8-bit 255 maps to; values
        below 0 and above 1 are scored.  A session scores it through a linear batch.  channels = 4: float RGBA, straight
        or `premultiplied` alpha in [0, 1], which a session with alpha_blend blends over its alpha_backgrounds."""
        if channels not in (3, 4):
            raise ValueError(f"a linear image has 3 or 4 channels, got {channels}")
        if premultiplied and channels != 4:
            raise ValueError("premultiplied= is for a linear image with alpha (channels = 4)")
        a = np.ascontiguousarray(data, dtype=np.float32).reshape(-1)
        if a.size != int(width) * int(height) * channels:
            raise ValueError(f"a linear image is width * height * {channels} floats, got {a.size}")
        return ImageData(a, int(width), int(height), int(channels), linear=True, premultiplied=bool(premultiplied))

    @staticmethod
    def rgb_with_icc(data, width: int, height: int, icc_profile: bytes) -> "ImageData":
        return ImageData(np.ascontiguousarray(data, dtype=np.uint8).reshape(-1), int(width), int(height), 3, bytes(icc_profile))

    @staticmethod
    def rgb16(data, width: int, height: int, depth: int, colour: Optional[Colour] = None, gain_map: Optional[GainMap] = None,
              icc_profile: Optional[bytes] = None) -> "ImageData":
        """A decoder's PixelData::Rgb16 (crates/codec-iter/src/avif_config.rs:122-170) kept as it is: packed uint16
        samples of `depth` bits, each meaning the sRGB value v / (2^depth - 1).  A session scores it through a deep batch.
        icc_profile: the decode's matrix/TRC profile, applied on the device by a session without a cms."""
        if depth not in DEEP_DEPTHS:
            raise ValueError(f"depth must be one of {DEEP_DEPTHS}, got {depth}")
        return ImageData(np.ascontiguousarray(data, dtype=np.uint16).reshape(-1), int(width), int(height), 3,
                         None if icc_profile is None else bytes(icc_profile), int(depth),
                         colour=_colour_at(colour, depth), gain_map=_gain_map_for(gain_map, colour, width, height))

    @staticmethod
    def rgba16(data, width: int, height: int, depth: int, colour: Optional[Colour] = None, gain_map: Optional[GainMap] = None) -> "ImageData":
        if depth not in DEEP_DEPTHS:
            raise ValueError(f"depth must be one of {DEEP_DEPTHS}, got {depth}")
        return ImageData(np.ascontiguousarray(data, dtype=np.uint16).reshape(-1), int(width), int(height), 4, None, int(depth),
                         colour=_colour_at(colour, depth), gain_map=_gain_map_for(gain_map, colour, width, height))

    @staticmethod
    def yuv(planes, width: int, height: int, subsampling: int = YUV_420, layout: int = YUV_PLANAR, matrix: int = YUV_BT601,
            range: int = YUV_FULL, upsample: int = CHROMA_TRIANGLE, *, depth: int = 8, msb_aligned: bool = False,
            colour: Optional[Colour] = None, icc_profile: Optional[bytes] = None) -> "ImageData":
        """A decoder's Y'CbCr planes in host memory (a JPEG decoder in raw mode, dav1d: 2-D arrays, Y, Cb, Cr or Y,
        interleaved CbCr; uint8 at depth 8, uint16 at 10 and 12, low- or MSB-aligned as P010 is) as they are: the session
        upsamples and converts them on the device, straight into the batch slot (Batch.set_*_yuv, the definition of
        include/ce_metrics.h), and scores the result as RGB8; the multi-device session converts them on the host with
        to_rgb8_vec, the same definition.  With a `colour` other than sRGB's (an HDR10 frame: BT2020_PQ) the image is
        scored in linear light, its planes going through Batch.set_*_yuv_cicp, or through
        Batch.set_*_yuv_hlg for an HlgDescription (section 18).
        icc_profile: the decode's embedded profile (a phone's JPEG or HEIC: Display P3).  A session without a cms applies a
        profile the library takes (matrix/TRC or LUT-based) on the device in the same launch that converts the planes
        (Batch.set_*_yuv_icc); a session with a cms, and the multi-device session, convert on the host
        (to_rgb8_srgb) and upload RGB8.  As with packed images, the source image's own profile stays unapplied."""
        if depth not in (8, 10, 12):
            raise ValueError(f"Y'CbCr samples are 8, 10 or 12 bits, got {depth}")
        img = YuvImage([np.asarray(p) for p in planes], subsampling, layout, matrix, range, upsample, int(depth), bool(msb_aligned), MEM_HOST)
        want = np.uint8 if depth == 8 else np.uint16
        for p in img.planes:
            if p.dtype != want or p.ndim != 2:
                raise TypeError("ImageData.yuv takes 2-D uint8 planes" if depth == 8 else f"ImageData.yuv at depth {depth} takes 2-D uint16 planes")
        return ImageData(np.empty(0, np.uint8), int(width), int(height), 3, None if icc_profile is None else bytes(icc_profile), 0, img,
                         colour=_colour_at(colour, depth))

    @staticmethod
    def tensor(obj, layout: str = "CHW", depth: int = 0, linear: bool = False, quantise: int = QUANT_NEAREST_EVEN) -> "ImageData":
        """One image as a framework holds it - a learned codec's float tensor in [0, 1], a GPU decoder's uint8 planes; a numpy
        array or a torch tensor, on the host or the device, any strides (TensorImage.from_array) - as it is: the session reads
        it through its strides on the device, straight into the batch slot (Batch.set_*_tensor, the definition of
        include/ce_metrics.h).  depth = 0: scored as RGB8, a float tensor quantised to 8 bits by
        `quantise`; depth 8, 10, 12 or 16: scored through a deep batch at that depth; linear=True: a float tensor of linear
        light with sRGB primaries, scored through a linear batch.  The multi-device session and to_rgb8_vec quantise on the
        host with quantise_tensor, the same definition.  A device tensor must stay alive and unchanged until the scores are in."""
        if depth and depth not in DEEP_DEPTHS:
            raise ValueError(f"depth must be 0 or one of {DEEP_DEPTHS}, got {depth}")
        if linear and depth:
            raise ValueError("a tensor is scored at an integer depth or in linear light, not both")
        t = obj if isinstance(obj, TensorImage) else TensorImage.from_array(obj, layout, quantise)
        if t.count != 1:
            raise ValueError(f"ImageData.tensor holds one image, the tensor has {t.count}")
        return ImageData(np.empty(0, np.uint8), t.width, t.height, 3, None, int(depth), linear=bool(linear), tensor_image=t)

    def _tensor_to_host(self, depth: int) -> np.ndarray:
        """The device's conversion of the tensor restated on the host: packed samples of `depth` bits."""
        t = self.tensor_image
        a = t.host_elements()[0]
        if a.dtype in (np.uint8, np.uint16):  # integer code values: clamped as deep ingest clamps
            return np.minimum(a, (1 << depth) - 1).astype(np.uint8 if a.dtype == np.uint8 and depth == 8 else np.uint16).reshape(-1)
        return quantise_tensor(a, depth, t.quantise).reshape(-1)

    def _yuv_to_rgb8_host(self) -> np.ndarray:
        """The device's conversion restated on the host for to_rgb8_vec (int64, the definition of include/ce_metrics.h)."""
        y, w, h = self.yuv_image, self.width, self.height
        ky, krv, kgu, kgv, kbu, y0, c0 = yuv_coefficients(y.matrix, y.range, y.depth, 8)
        shift, maxv = (16 - y.depth if y.msb_aligned else 0), (1 << y.depth) - 1
        sample = lambda p: np.minimum(p.astype(np.int64) >> shift, maxv)
        luma = sample(y.planes[0])[:h, :w]
        if y.subsampling == YUV_400:
            cb = cr = np.full((h, w), c0, np.int64)
        else:
            if y.layout == YUV_SEMIPLANAR:
                cb, cr = sample(y.planes[1][:, 0::2]), sample(y.planes[1][:, 1::2])
            else:
                cb, cr = sample(y.planes[1]), sample(y.planes[2])
            cb, cr = (self._upsample_chroma(c, y.subsampling, y.upsample == CHROMA_TRIANGLE)[:h, :w] for c in (cb, cr))
        yy = ky * (luma - y0) + 32768
        rgb = np.stack([(yy + krv * (cr - c0)) >> 16, (yy - kgu * (cb - c0) - kgv * (cr - c0)) >> 16, (yy + kbu * (cb - c0)) >> 16], -1)
        return np.clip(rgb, 0, 255).astype(np.uint8).reshape(-1)

    @staticmethod
    def _upsample_chroma(c: np.ndarray, subsampling: int, triangle: bool) -> np.ndarray:
        if subsampling == YUV_444:
            return c
        shift = lambda a, k, axis: np.take(a, np.clip(np.arange(a.shape[axis]) + k, 0, a.shape[axis] - 1), axis=axis)
        nb = (lambda a, k, axis: shift(a, k, axis)) if triangle else (lambda a, k, axis: a)
        if subsampling == YUV_420:
            t = np.empty((2 * c.shape[0], c.shape[1]), np.int64)
            t[0::2], t[1::2] = 3 * c + nb(c, -1, 0), 3 * c + nb(c, 1, 0)
            even, odd, sh = 8, 7, 4
        else:
            t, even, odd, sh = c, 1, 2, 2
        out = np.empty((t.shape[0], 2 * t.shape[1]), np.int64)
        out[:, 0::2], out[:, 1::2] = (3 * t + nb(t, -1, 1) + even) >> sh, (3 * t + nb(t, 1, 1) + odd) >> sh
        return out

    def to_rgb8_vec(self) -> np.ndarray:  # session.rs:98-117 (host copy; the session itself strips alpha on the device)
        if self.gain_map is not None:  # its RGB8 form would be the base alone, which scores a damaged gain map as identical
            raise MetricCalculation(CE_ERR_BACKEND, "Metric calculation failed: an image with a gain map is scored in linear light and has no RGB8 form")
        if self.in_linear_light:  # no reference rule turns HDR or wide-gamut content into sRGB bytes: it is scored in linear light
            raise MetricCalculation(CE_ERR_BACKEND, "Metric calculation failed: an image in linear light or with a non-sRGB colour description has no RGB8 form")
        if self.yuv_image is not None:
            return self._yuv_to_rgb8_host()
        if self.tensor_image is not None and not self.depth:
            return self._tensor_to_host(8).astype(np.uint8)
        if self.tensor_image is not None:
            data = self._tensor_to_host(self.depth)
        else:
            data = self.data if self.channels == 3 else np.ascontiguousarray(self.data.reshape(-1, 4)[:, :3]).reshape(-1)
        if self.depth:  # to_8bit's rule for any depth: what the reference does to a 10-bit decode before it measures
            maxv = (1 << self.depth) - 1
            return np.minimum((np.minimum(data, maxv).astype(np.uint64) * 255 + maxv // 2) // maxv, 255).astype(np.uint8)
        return data

    @property
    def in_linear_light(self) -> bool:
        """Scored through a linear batch: linear float32, code values with a description other than sRGB's, or a base image
        with a gain map."""
        return self.linear or self.gain_map is not None or (self.colour is not None and not self.colour.is_srgb)

    @property
    def has_alpha(self) -> bool:
        return self.channels == 4 and self.yuv_image is None

    def composited_rgb8_vec(self, background: Sequence[int]) -> np.ndarray:
        """to_rgb8_vec of this image seen over the opaque 8-bit colour `background` (EvalConfig.alpha_backgrounds), on the
        host: composite_over at the image's own depth, then to_8bit's rule.  An image without alpha is to_rgb8_vec."""
        if not self.has_alpha:
            return self.to_rgb8_vec()
        d = self.depth or 8
        rgb = composite_over(self.data.reshape(-1, 4), scale_background(background, d), d).reshape(-1)
        if self.depth:
            maxv = (1 << d) - 1
            return np.minimum((rgb.astype(np.uint64) * 255 + maxv // 2) // maxv, 255).astype(np.uint8)
        return rgb

    def to_rgb8_srgb(self, cms: Optional[Callable[[bytes, np.ndarray], np.ndarray]] = None) -> np.ndarray:
        """session.rs:143-147 -> transform_to_srgb, metrics/icc.rs:69-113: on the HOST (the session itself applies the
        profile on the device through a colour table).  `cms(profile_bytes, rgb_nx3_u8) -> rgb_nx3_u8` is the colour
        management to use (the reference's is moxcms); without one a tagged image fails like a build without `icc`."""
        rgb = self.to_rgb8_vec()
        if self.icc_profile is None:
            return rgb
        if cms is None:
            self._check_profile()
        return np.ascontiguousarray(cms(self.icc_profile, rgb.reshape(-1, 3)), dtype=np.uint8).reshape(-1)

    def _check_profile(self):
        if self.icc_profile is not None:
            # the reference built without its `icc` feature (icc.rs:105-113): no colour management available
            raise MetricCalculation(CE_ERR_BACKEND, "Metric calculation failed: ICC: ICC profile support requires the 'icc' feature")

    @property
    def pixel_format(self) -> int:
        if self.linear:
            return PIXEL_RGB_F32 if self.channels == 3 else PIXEL_RGBA_F32
        if self.depth:
            return PIXEL_RGB16 if self.channels == 3 else PIXEL_RGBA16
        return PIXEL_RGB8 if self.channels == 3 else PIXEL_RGBA8


@dataclass
class EncodeRequest:  # session.rs:151-177
    quality: float
    params: Dict[str, str] = field(default_factory=dict)

    def with_param(self, key: str, value: str) -> "EncodeRequest":
        self.params[str(key)] = str(value)
        return self


EncodeFn = Callable[[ImageData, EncodeRequest], bytes]
DecodeFn = Callable[[bytes], ImageData]


@dataclass
class EvalConfig:  # session.rs:188-279
    report_dir: str
    cache_dir: Optional[str] = None
    viewing: Optional[ViewingCondition] = None  # carried; no metric reads it (dssim.rs:43 ignores it too) unless simulate_viewing is set
    metrics: MetricConfig = field(default_factory=MetricConfig.all)
    quality_levels: List[float] = field(default_factory=lambda: [50.0, 60.0, 70.0, 80.0, 85.0, 90.0, 95.0])
    # Not in the reference, whose simulation_params (src/viewing.rs:244-301) nothing consumes.  None: every score is what it
    # always was.  A SimulationMode: each decode and its source are resampled on the device to the size `viewing` displays
    # them at (SimulationParams.displayed_size, viewing.py) and scored there; 8-bit decodes only.
    simulate_viewing: Optional[SimulationMode] = None
    resample_filter: int = RESAMPLE_LANCZOS3
    # Not in the reference, which drops alpha (session.rs:98-117).  None: every score and every upload is what it always was.
    # A sequence of 8-bit (r, g, b) colours (ALPHA_BLACK_WHITE: black and white): a pair whose source or decode has alpha is
    # composited over each on the device (Batch.set_*_over) and scored over each; the row carries the
    # worst value per metric and the report keeps the per-background scores (ImageReport.alpha_scores).
    alpha_backgrounds: Optional[Sequence[Tuple[int, int, int]]] = None
    # None: a pair scored in linear light (a colour description, HLG, float32, an ICC profile into a linear group) whose
    # source or decode has alpha is refused under alpha_backgrounds, as ever.  ALPHA_BLEND_LINEAR: such a pair is blended
    # over each background in linear light, after the pixel's own conversion (Batch.set_*_cicp_over / _hlg_over /
    # _icc_over / _linear_over), and reported like a composited 8-bit pair.
    alpha_blend: Optional[str] = None

    @staticmethod
    def builder() -> "EvalConfigBuilder":
        return EvalConfigBuilder()


class EvalConfigBuilder:
    def __init__(self):
        self._report_dir = self._cache_dir = self._viewing = self._metrics = self._levels = self._simulate = None
        self._alpha = self._alpha_blend = None

    def report_dir(self, path):
        self._report_dir = str(path)
        return self

    def cache_dir(self, path):
        self._cache_dir = str(path)
        return self

    def viewing(self, viewing):
        self._viewing = viewing
        return self

    def simulate_viewing(self, mode: Optional[SimulationMode]):
        self._simulate = mode
        return self

    def metrics(self, metrics: MetricConfig):
        self._metrics = metrics
        return self

    def alpha_backgrounds(self, backgrounds: Optional[Sequence[Tuple[int, int, int]]]):
        """8-bit (r, g, b) colours to composite transparent images over (ALPHA_BLACK_WHITE); None: alpha is dropped"""
        if backgrounds is not None:
            backgrounds = tuple(tuple(int(v) for v in bg) for bg in backgrounds)
            if not 1 <= len(backgrounds) <= MAX_BACKGROUNDS or any(len(bg) != 3 or min(bg) < 0 or max(bg) > 255 for bg in backgrounds):
                raise ValueError(f"alpha_backgrounds: 1 to {MAX_BACKGROUNDS} colours of three 8-bit values")
        self._alpha = backgrounds
        return self

    def alpha_blend(self, mode: Optional[str]):
        """ALPHA_BLEND_LINEAR: blend transparent images that are scored in linear light over alpha_backgrounds there; None:
        such pairs stay refused"""
        if mode not in (None, ALPHA_BLEND_LINEAR):
            raise ValueError(f"alpha_blend: None or ALPHA_BLEND_LINEAR, got {mode!r}")
        self._alpha_blend = mode
        return self

    def quality_levels(self, levels: Sequence[float]):
        self._levels = [float(q) for q in levels]
        return self

    def build(self) -> EvalConfig:
        if self._report_dir is None:
            raise ValueError("report_dir is required")  # session.rs:269 `.expect("report_dir is required")`
        cfg = EvalConfig(self._report_dir, self._cache_dir, self._viewing)
        if self._metrics is not None:
            cfg.metrics = self._metrics
        if self._levels is not None:
            cfg.quality_levels = self._levels
        cfg.simulate_viewing = self._simulate
        cfg.alpha_backgrounds = self._alpha
        cfg.alpha_blend = self._alpha_blend
        return cfg


def worst_over_backgrounds(per_bg: Sequence[MetricResult]) -> MetricResult:
    """One pair's scores over each background -> the worst value per metric: max DSSIM, max Butteraugli, min SSIMULACRA2,
    min PSNR.  A single entry is returned as it is."""
    if len(per_bg) == 1:
        return per_bg[0]
    pick = lambda vals, f: None if any(v is None for v in vals) else f(vals)
    return MetricResult(dssim=pick([m.dssim for m in per_bg], max), ssimulacra2=pick([m.ssimulacra2 for m in per_bg], min),
                        butteraugli=pick([m.butteraugli for m in per_bg], max), psnr=pick([m.psnr for m in per_bg], min))


@dataclass
class _CodecEntry:
    id: str
    version: str
    encode: EncodeFn
    decode: Optional[DecodeFn]


class EvalSession:
    """session.rs:309-497.  One session = one device context; `evaluate_image` may be called for any shape."""

    def __init__(self, config: EvalConfig, ctx: Optional[Context] = None, device: int = 0,
                 cms: Optional[Callable[[bytes, np.ndarray], np.ndarray]] = None):
        """cms(profile_bytes, rgb (n, 3) uint8) -> (n, 3) uint8: the host's ICC -> sRGB transform (the reference's default
        build uses moxcms, icc.rs:69-103).  It is evaluated ONCE per distinct profile on the identity colour cube; the
        resulting 2^24-entry table lives on the device and is applied to every decoded image tagged with that profile
        (session.rs:394: only DECODED images go through to_rgb8_srgb, the source image does not).  Without a cms a decoded
        image tagged with a matrix/TRC profile (icc_describe(profile).kind == 0) has it applied on the device by the library
        itself (IccProfile), in RGB8, deep and linear groups alike; one tagged with any other profile
        raises what a build without the `icc` feature raises."""
        self.config = config
        self.ctx = ctx or Context(device)
        self._own_ctx = ctx is None
        self._codecs: List[_CodecEntry] = []
        self._cms = cms
        self._tables: Dict[bytes, ColorTable] = {}
        self._profiles: Dict[bytes, Optional[IccProfile]] = {}

    def close(self):
        for t in self._tables.values():
            t.close()
        self._tables.clear()
        for p in self._profiles.values():
            if p is not None:
                p.close()
        self._profiles.clear()
        if self._own_ctx:
            self.ctx.close()

    def _profile_for(self, image: ImageData) -> Optional[IccProfile]:
        """The device profile of a decoded image tagged with a matrix/TRC profile or with a LUT-based one that
        icc_lut_describe supports (its A2B0 tag, trilinear interpolation), in a session without a cms; None for
        an untagged image, a session with a cms (which applies every profile) and any other profile.  A profile is parsed
        once per session: the handle, or None for a profile the library does not take, is kept by the profile's bytes."""
        if image.icc_profile is None or self._cms is not None:
            return None
        key = bytes(image.icc_profile)
        if key not in self._profiles:
            if icc_describe(key).kind == 0:
                self._profiles[key] = IccProfile(self.ctx, key)
            elif icc_lut_describe(key).kind == 0:  # a LUT-based profile the library evaluates itself
                self._profiles[key] = IccLutProfile(self.ctx, key)
            else:
                self._profiles[key] = None
        return self._profiles[key]

    def _table_for(self, image: ImageData) -> Optional[ColorTable]:
        """The device colour table of a decoded image's profile (None for untagged = sRGB images, icc.rs:73)."""
        if image.icc_profile is None:
            return None
        if self._cms is None:
            if self._profile_for(image) is not None:
                return None  # applied by set_*_icc instead
            image._check_profile()
        key = bytes(image.icc_profile)
        t = self._tables.get(key)
        if t is None:
            out = np.asarray(self._cms(key, ColorTable.identity_cube()), dtype=np.uint8)
            if out.shape != (1 << 24, 3):
                raise MetricCalculation(CE_ERR_BACKEND, f"Metric calculation failed: ICC: Failed to apply ICC transform: the cms returned shape {out.shape}")
            t = self._tables[key] = ColorTable(self.ctx, out)
        return t

    def add_codec(self, id: str, version: str, encode: EncodeFn) -> "EvalSession":  # :325-334
        self._codecs.append(_CodecEntry(id, version, encode, None))
        return self

    def add_codec_with_decode(self, id: str, version: str, encode: EncodeFn, decode: DecodeFn) -> "EvalSession":  # :336-351
        self._codecs.append(_CodecEntry(id, version, encode, decode))
        return self

    def codec_count(self) -> int:
        return len(self._codecs)

    # -- the sweep -------------------------------------------------------------------------------
    def _sweep(self, name: str, image: ImageData):
        """Encode/decode every (codec, quality) cell of one image (session.rs:375-428 minus the metrics).
        Returns the report with metric-less rows and the list of (row index, decoded ImageData)."""
        width, height = image.width, image.height
        report = R.ImageReport(name, width, height)
        pending: List[Tuple[int, ImageData]] = []
        for codec in self._codecs:
            for quality in self.config.quality_levels:
                request = EncodeRequest(float(quality))
                t0 = time.perf_counter()
                encoded = codec.encode(image, request)
                encode_ms = int((time.perf_counter() - t0) * 1000)
                row = R.CodecResult(codec.id, codec.version, float(quality), len(encoded),
                                    (len(encoded) * 8) / (float(width) * float(height)), encode_ms,
                                    codec_params=dict(request.params))
                if codec.decode is not None:
                    t0 = time.perf_counter()
                    decoded = codec.decode(encoded)
                    row.decode_time_ms = int((time.perf_counter() - t0) * 1000)
                    if self._cms is None and self._profile_for(decoded) is None:
                        decoded._check_profile()  # to_rgb8_srgb's failure mode without colour management, before anything reaches the device
                    pending.append((len(report.results), decoded))
                report.results.append(row)
        return report, pending

    def _displayed(self, w: int, h: int) -> Tuple[int, int]:
        """The size a w x h image is scored at: its own, unless config.simulate_viewing asks for the displayed one."""
        if self.config.simulate_viewing is None:
            return w, h
        cond = self.config.viewing or ViewingCondition.default()
        return cond.simulation_params(w, h, self.config.simulate_viewing).displayed_size(w, h)

    def _score(self, jobs: List[Tuple[ImageData, R.ImageReport, List[Tuple[int, ImageData]]]]):
        """All cells of all images, one device batch per shape; references uploaded once per image."""
        cfg = self.config.metrics
        buckets: Dict[Tuple[int, int], list] = {}
        for image, report, pending in jobs:
            if pending:
                buckets.setdefault((image.width, image.height), []).append((image, report, pending))
        for (w, h), group in buckets.items():
            # a shape's cells go through device batches that fit the device: whole images while they fit, an image with
            # more cells than one batch holds is split (its reference is uploaded once per part)
            free, _total = self.ctx.memory_info()
            budget = int(os.environ.get("CE_SESSION_BATCH_BYTES", 0)) or int(free * 0.6)
            sw, sh = self._displayed(w, h)  # the metrics' working set is the displayed shape's; the source slabs come on top
            in_linear = any(image.in_linear_light or any(d.in_linear_light for _, d in pending) for image, _, pending in group)
            extra = (12 if in_linear else 3) * w * h if (sw, sh) != (w, h) else 0  # a linear source slab holds 12 bytes a pixel
            fixed = estimate_batch_bytes(sw, sh, 0, 0, cfg)
            per_ref = estimate_batch_bytes(sw, sh, 1, 0, cfg) - fixed + extra
            per_pair = estimate_batch_bytes(sw, sh, 0, 1, cfg) - fixed + extra
            # with alpha_backgrounds a pair may take one slot per background on either side: budget for that
            fan = len(self.config.alpha_backgrounds) if self.config.alpha_backgrounds else 1
            per_ref, per_pair = per_ref * fan, per_pair * fan
            max_pairs = max(1, (budget - fixed - per_ref) // max(per_pair, 1))
            parts: List[list] = [[]]  # each part: [(image, report, cells)]
            used = fixed
            for image, report, pending in group:
                for o in range(0, len(pending), max_pairs):
                    cells = pending[o:o + max_pairs]
                    need = per_ref + per_pair * len(cells)
                    if parts[-1] and used + need > budget:
                        parts.append([])
                        used = fixed
                    parts[-1].append((image, report, cells))
                    used += need
            for part in parts:
                self._score_part(w, h, part, cfg)

    def _score_part(self, w: int, h: int, group, cfg: MetricConfig):
        """Cells whose decode is 8-bit go through an RGB8 batch as ever; the cells of deep decodes (ImageData.rgb16 /
        rgba16) through one deep batch per (source depth, decode depth), the 8-bit source as depth 8, neither side rescaled."""
        kinds: Dict[Tuple[int, int], list] = {}
        linear_group = []
        for image, report, pending in group:
            by_depth: Dict[int, list] = {}
            lin = [cell for cell in pending if image.in_linear_light or cell[1].in_linear_light]
            if lin:
                linear_group.append((image, report, lin))
                pending = [cell for cell in pending if not (image.in_linear_light or cell[1].in_linear_light)]
            for cell in pending:
                by_depth.setdefault(cell[1].depth, []).append(cell)
            for d, cells in by_depth.items():
                kinds.setdefault((image.depth or 8, d) if (d or image.depth) else (0, 0), []).append((image, report, cells))
        for depths, sub in kinds.items():
            self._score_cells(w, h, sub, cfg, None if depths == (0, 0) else (depths[0], depths[1] or 8))
        if linear_group:
            self._score_cells_linear(w, h, linear_group, cfg)

    def _set_linear(self, batch: Batch, image: ImageData, ref_index: int, pair_index: Optional[int]):
        """One image into a slot of a linear batch: float32 as it is, code values through the CICP ingest - by their own
        description, an untagged image as sRGB (1, 13) at its own depth - and Y'CbCr planes through the fused ingest; an
        HlgDescription takes the HLG calls of the same shape, an image with a gain map the gain-map calls."""
        def refuse(what):
            raise MetricCalculation(CE_ERR_BACKEND, f"Metric calculation failed: linear-light scoring: {what}")
        if image.yuv_image is not None:  # the planes' own tag, an untagged image as sRGB; depth 16 keeps what the matrix gives between code points
            if image.colour is not None and image.icc_profile is not None:
                refuse("an image with both a colour description and an ICC profile is not supported")
            if image.icc_profile is not None and pair_index is not None:  # a decode's profile; the source's own is not applied, as ever
                profile = self._profile_for(image)
                if profile is None:
                    refuse("an ICC profile is not applied in linear light")
                return batch.set_test_yuv_icc(pair_index, ref_index, image.yuv_image, 16, profile)  # the library's own transform, planes and profile in one launch
            colour = (image.colour or ColourDescription.SRGB).with_depth(16)
            if isinstance(colour, HlgDescription):
                if pair_index is None:
                    return batch.set_reference_yuv_hlg(ref_index, image.yuv_image, colour)
                return batch.set_test_yuv_hlg(pair_index, ref_index, image.yuv_image, colour)
            if pair_index is None:
                return batch.set_reference_yuv_cicp(ref_index, image.yuv_image, colour)
            return batch.set_test_yuv_cicp(pair_index, ref_index, image.yuv_image, colour)
        if image.tensor_image is not None:  # a float tensor of linear light, read in place
            if pair_index is None:
                return batch.set_reference_tensor(ref_index, image.tensor_image)
            return batch.set_test_tensor(pair_index, [ref_index], image.tensor_image)
        if image.colour is not None and image.icc_profile is not None:
            refuse("an image with both a colour description and an ICC profile is not supported")
        profile = self._profile_for(image) if pair_index is not None and not image.linear and image.gain_map is None else None
        if image.icc_profile is not None and pair_index is not None and profile is None:  # the source's own profile is not applied, as ever
            refuse("an ICC profile is not applied in linear light")
        if image.has_alpha and self.config.alpha_backgrounds:
            refuse("alpha_backgrounds with a colour description is not supported")
        if image.linear and image.channels == 4:
            refuse("a float RGBA image is blended over alpha_backgrounds: it needs both alpha_backgrounds and alpha_blend")
        if profile is not None:  # a matrix/TRC profile, no cms: the library's own transform, into linear light
            return batch.set_test_icc(pair_index, ref_index, image.data.reshape(image.height, image.width, image.channels), image.depth or 8, profile)
        if image.linear:
            return batch.set_reference(ref_index, image.data) if pair_index is None else batch.set_test(pair_index, ref_index, image.data)
        colour = image.colour or ColourDescription.SRGB.with_depth(image.depth or 8)
        px = image.data.reshape(image.height, image.width, image.channels)
        if image.gain_map is not None:
            if pair_index is None:
                batch.set_reference_gainmap(ref_index, px, colour, image.gain_map)
            else:
                batch.set_test_gainmap(pair_index, ref_index, px, colour, image.gain_map)
        elif isinstance(colour, HlgDescription):
            if pair_index is None:
                batch.set_reference_hlg(ref_index, px, colour)
            else:
                batch.set_test_hlg(pair_index, ref_index, px, colour)
        elif pair_index is None:
            batch.set_reference_cicp(ref_index, px, colour)
        else:
            batch.set_test_cicp(pair_index, ref_index, px, colour)

    def _set_linear_over(self, batch: Batch, image: ImageData, first: int, ref_of: Optional[List[int]], bgs: np.ndarray):
        """One image with alpha into len(bgs) consecutive slots of a linear batch from `first` on (the test slots bound to
        ref_of), turned into linear light by _set_linear's route and blended there over each of bgs (alpha_blend)."""
        def refuse(what):
            raise MetricCalculation(CE_ERR_BACKEND, f"Metric calculation failed: linear-light scoring: {what}")
        test = ref_of is not None
        if image.gain_map is not None:
            refuse("a gain-map image with alpha is not supported by alpha_blend")
        if image.colour is not None and image.icc_profile is not None:
            refuse("an image with both a colour description and an ICC profile is not supported")
        profile = self._profile_for(image) if test and not image.linear else None
        if image.icc_profile is not None and test and profile is None:  # the source's own profile is not applied, as ever
            refuse("an ICC profile is not applied in linear light")
        if image.linear:
            px = image.data.reshape(image.height, image.width, 4)
            if test:
                return batch.set_test_linear_over(first, ref_of, px, bgs, premultiplied=image.premultiplied)
            return batch.set_reference_linear_over(first, px, bgs, premultiplied=image.premultiplied)
        px = image.data.reshape(image.height, image.width, image.channels)
        if profile is not None:
            return batch.set_test_icc_over(first, ref_of, px, image.depth or 8, profile, bgs)
        colour = image.colour or ColourDescription.SRGB.with_depth(image.depth or 8)
        if isinstance(colour, HlgDescription):
            return batch.set_test_hlg_over(first, ref_of, px, colour, bgs) if test else batch.set_reference_hlg_over(first, px, colour, bgs)
        return batch.set_test_cicp_over(first, ref_of, px, colour, bgs) if test else batch.set_reference_cicp_over(first, px, colour, bgs)

    def _score_cells_linear(self, w: int, h: int, group, cfg: MetricConfig):
        """The cells scored in linear light: one linear batch, a reference slot per image, a test slot
        per cell; PSNR is not defined there and stays None.  With simulate_viewing they are scored at the displayed size: the
        batch of the uploads is resampled in linear light into a linear batch of that shape."""
        if cfg.flags & 1:  # CE_FLAG_XYB_ROUNDTRIP
            raise MetricCalculation(CE_ERR_BACKEND, "Metric calculation failed: linear-light scoring: xyb_roundtrip is an 8-bit quantisation")
        # with alpha_blend a pair whose source or decode has alpha is fanned over alpha_backgrounds exactly as _score_cells
        # does it, the blend done in linear light; each 8-bit background goes through the sRGB curve once
        bgs = (self.config.alpha_backgrounds or ()) if self.config.alpha_blend == ALPHA_BLEND_LINEAR else ()
        bgs_lin = srgb_table(8, 0)[np.asarray(bgs, np.int64).reshape(-1, 3)] if bgs else None
        fan = lambda image, decoded: len(bgs) if bgs and (image.has_alpha or decoded.has_alpha) else 1
        n_refs = sum(len(bgs) if bgs and image.has_alpha else 1 for image, _, _ in group)
        n_pairs = sum(fan(image, decoded) for image, _, p in group for _, decoded in p)
        batch = Batch(self.ctx, w, h, n_refs, n_pairs, linear=True)
        try:
            rows = []
            k = ri = 0
            for image, report, pending in group:
                if bgs and image.has_alpha:
                    self._set_linear_over(batch, image, ri, None, bgs_lin)
                    ref_of = list(range(ri, ri + len(bgs)))
                else:
                    self._set_linear(batch, image, ri, None)
                    ref_of = [ri] * max(len(bgs), 1)
                ri = ref_of[-1] + 1
                for row_index, decoded in pending:
                    if (decoded.width, decoded.height) != (w, h):
                        raise DimensionMismatch(1, f"Dimension mismatch: expected ({w}, {h}), got ({decoded.width}, {decoded.height})")
                    n = fan(image, decoded)
                    if bgs and decoded.has_alpha:
                        self._set_linear_over(batch, decoded, k, ref_of, bgs_lin)
                    else:
                        for j in range(n):  # an opaque decode against a source with alpha: the same image over every background
                            self._set_linear(batch, decoded, ref_of[j], k + j)
                    rows.append((report, row_index, k, n))
                    k += n
            shown = self._displayed(w, h)
            if shown != (w, h):
                dst = Batch(self.ctx, shown[0], shown[1], n_refs, n_pairs, linear=True)
                try:
                    batch.resample_pairs_into(dst, n_refs, n_pairs, self.config.resample_filter)
                    scores = dst.run(n_pairs, cfg)
                finally:
                    dst.close()
            else:
                scores = batch.run(n_pairs, cfg)
        finally:
            batch.close()
        for report, row_index, first, n in rows:
            per_bg = []
            for s in scores[first:first + n]:
                if s.status != 0:
                    raise _error_obj(s.status, self.ctx._err())
                per_bg.append(MetricResult.from_c(s))
            m = worst_over_backgrounds(per_bg)
            row = report.results[row_index]
            row.dssim, row.ssimulacra2, row.butteraugli, row.psnr = m.dssim, m.ssimulacra2, m.butteraugli, m.psnr
            row.perception = m.perception_level()
            if n > 1:
                report.alpha_scores[row_index] = per_bg

    def _score_cells(self, w: int, h: int, group, cfg: MetricConfig, depths: Optional[Tuple[int, int]]):
        # a pair whose source or decode has alpha takes one test slot per background (config.alpha_backgrounds); a source
        # with alpha takes one reference slot per background, an opaque one a single slot that all of them read
        bgs = self.config.alpha_backgrounds or ()
        fan = lambda image, decoded: len(bgs) if bgs and (image.has_alpha or decoded.has_alpha) else 1
        n_refs = sum(len(bgs) if bgs and image.has_alpha else 1 for image, _, _ in group)
        n_pairs = sum(fan(image, decoded) for image, _, p in group for _, decoded in p)
        bg_side = [[scale_background(bg, d or 8) for bg in bgs] for d in (depths or (8, 8))]  # at each side's depth
        batch = Batch(self.ctx, w, h, n_refs, n_pairs, depths=depths)
        try:
            rows = []
            k = ri = 0
            for image, report, pending in group:
                if bgs and image.has_alpha:
                    batch.set_reference_over(ri, image.data, image.pixel_format, bg_side[0])
                    ref_of = list(range(ri, ri + len(bgs)))
                else:
                    if image.yuv_image is not None:
                        batch.set_reference_yuv(ri, image.yuv_image)
                    elif image.tensor_image is not None:  # a framework's tensor: read through its strides on the device, into the slot
                        batch.set_reference_tensor(ri, image.tensor_image)
                    else:
                        batch.set_reference_fmt(ri, image.data, image.pixel_format)
                    ref_of = [ri] * max(len(bgs), 1)
                ri = ref_of[-1] + 1
                for row_index, decoded in pending:
                    if (decoded.width, decoded.height) != (w, h):  # calculate_metrics' length check, ssimulacra2.rs:65-70
                        raise DimensionMismatch(1, f"Dimension mismatch: expected ({w}, {h}), got ({decoded.width}, {decoded.height})")
                    n = fan(image, decoded)
                    profile = self._profile_for(decoded)  # a matrix/TRC profile in a session without a cms, else None
                    if bgs and decoded.has_alpha:
                        if profile is not None or self._table_for(decoded) is not None:
                            raise MetricCalculation(CE_ERR_BACKEND, "Metric calculation failed: alpha_backgrounds: a decode with alpha and an ICC profile is not supported")
                        batch.set_test_over(k, ref_of, decoded.data, decoded.pixel_format, bg_side[1])
                    else:
                        for j in range(n):  # an opaque decode against a source with alpha: the same image over every background
                            if decoded.tensor_image is not None:
                                batch.set_test_tensor(k + j, [ref_of[j]], decoded.tensor_image)
                            elif decoded.yuv_image is not None and profile is not None:  # planes with a profile the library takes: one launch, at the planes' own depth
                                batch.set_test_yuv_icc(k + j, ref_of[j], decoded.yuv_image, decoded.yuv_image.depth, profile)
                            elif decoded.yuv_image is not None and decoded.icc_profile is not None:  # a session with a cms: to_rgb8_srgb on the host
                                batch.set_test(k + j, ref_of[j], decoded.to_rgb8_srgb(self._cms))
                            elif decoded.yuv_image is not None:  # a decoder's Y'CbCr planes: upsampled and converted on the device, into the slot
                                batch.set_test_yuv(k + j, ref_of[j], decoded.yuv_image)
                            elif profile is not None:  # to_rgb8_srgb by the library's own transform
                                batch.set_test_icc(k + j, ref_of[j], decoded.data.reshape(decoded.height, decoded.width, decoded.channels),
                                                   decoded.depth or 8, profile)
                            else:
                                batch.set_test_lut(k + j, ref_of[j], decoded.data, decoded.pixel_format, self._table_for(decoded))  # to_rgb8_srgb, session.rs:394
                    rows.append((report, row_index, k, n))
                    k += n
            shown = self._displayed(w, h)
            if shown != (w, h):
                dst = Batch(self.ctx, shown[0], shown[1], n_refs, n_pairs)
                try:
                    batch.resample_pairs_into(dst, n_refs, n_pairs, self.config.resample_filter)
                    scores = dst.run(n_pairs, cfg)
                finally:
                    dst.close()
            else:
                scores = batch.run(n_pairs, cfg)
        finally:
            batch.close()
        for report, row_index, first, n in rows:
            per_bg = []
            for s in scores[first:first + n]:
                if s.status != 0:
                    raise _error_obj(s.status, self.ctx._err())
                per_bg.append(MetricResult.from_c(s))
            m = worst_over_backgrounds(per_bg)
            row = report.results[row_index]
            row.dssim, row.ssimulacra2, row.butteraugli, row.psnr = m.dssim, m.ssimulacra2, m.butteraugli, m.psnr
            row.perception = m.perception_level()  # session.rs:407
            if n > 1:
                report.alpha_scores[row_index] = per_bg

    def evaluate_image(self, name: str, image: ImageData) -> R.ImageReport:  # session.rs:368-434
        # the source image enters as to_rgb8_vec() (session.rs:373): its own profile, if any, is NOT applied
        report, pending = self._sweep(name, image)
        self._score([(image, report, pending)])
        return report

    def evaluate_corpus(self, name: str, images: Sequence[Tuple[str, ImageData]], rank: int = 0, world: int = 1) -> R.CorpusReport:
        """Every image of a corpus in one pass (the loop a caller of evaluate_image writes, e.g. examples/ and
        crates/codec-compare): all cells of all images of a shape share one device batch.  With world > 1 the
        images are partitioned by reference (sharding.assign_references) and this rank scores its own."""
        from .sharding import assign_references

        corpus = R.CorpusReport(name, config_summary=f"metrics: {self.config.metrics}")
        mine = list(range(len(images)))
        if world > 1:
            mine = assign_references([im.width * im.height for _, im in images], world)[rank]
        jobs = []
        for i in mine:
            img_name, image = images[i]
            report, pending = self._sweep(img_name, image)
            jobs.append((image, report, pending))
            corpus.images.append(report)
        self._score(jobs)
        return corpus

    # -- writers (session.rs:500-584) ---------------------------------------------------------------
    def write_image_report(self, report: R.ImageReport) -> str:
        return R.write_image_report(self.config.report_dir, report)

    def write_corpus_report(self, report: R.CorpusReport):
        return R.write_corpus_report(self.config.report_dir, report)
