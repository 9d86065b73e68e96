"""Viewing conditions — src/viewing.rs mirrored, plus what the reference leaves out: scoring at the displayed size.

`ViewingCondition`, `SimulationMode`, `SimulationParams`, `REFERENCE_PPD` and `presets` follow src/viewing.rs item for
item: every formula is f64 and `round()` rounds half away from zero, as Rust's `f64::round`.  The reference stops at the
parameters - it has no resampler and its metrics ignore the condition (src/metrics/dssim.rs:43).  `score_under` goes on:
it resamples a resident batch on the device (`Batch.resample_pairs_into`) to the size each condition displays it at and
scores it there.

`SimulationParams.target_width` is kept as the reference computes it, `round(w * ratio)`; its own tests pin 1000 -> 2000
for a 2x image on a 1x display that the same struct flags `requires_downscale`.  A browser divides: that image covers
`w / ratio` device pixels.  `SimulationParams.displayed_size` is that size, and it is what gets resampled (DESIGN.md
section 12).
"""
from __future__ import annotations

import enum
import math
import os
from dataclasses import dataclass, replace
from typing import List, Optional, Sequence, Tuple

__all__ = ["ViewingCondition", "SimulationMode", "SimulationParams", "REFERENCE_PPD", "presets", "ConditionScores", "score_under",
           "rust_round"]

REFERENCE_PPD = 40.0  # src/viewing.rs:337


def rust_round(x: float) -> int:
    """f64::round: half away from zero (Python's round() rounds half to even)."""
    return int(math.floor(x + 0.5)) if x >= 0.0 else -int(math.floor(-x + 0.5))


def _round_u32(x: float) -> int:
    """`x.round() as u32`: the cast saturates."""
    if x != x:
        return 0
    return min(max(rust_round(x), 0), 0xFFFFFFFF)


class SimulationMode(enum.Enum):  # src/viewing.rs:33-53
    Accurate = 0
    DownsampleOnly = 1


@dataclass(frozen=True)
class SimulationParams:  # src/viewing.rs:308-331
    scale_factor: float
    target_width: int
    target_height: int
    adjusted_ppd: float
    requires_upscale: bool
    requires_downscale: bool

    def requires_scaling(self) -> bool:  # :342
        return self.requires_upscale or self.requires_downscale

    def downscale_only_factor(self) -> float:  # :348
        return min(self.scale_factor, 1.0)

    def threshold_multiplier(self) -> float:  # :381
        return self.adjusted_ppd / REFERENCE_PPD

    def adjust_dssim_threshold(self, base_threshold: float) -> float:  # :406
        return base_threshold * self.threshold_multiplier()

    def adjust_butteraugli_threshold(self, base_threshold: float) -> float:  # :418
        return base_threshold * self.threshold_multiplier()

    def adjust_ssimulacra2_threshold(self, base_threshold: float) -> float:  # :431-445
        multiplier = self.threshold_multiplier()
        if multiplier >= 1.0:
            v = base_threshold - (100.0 - base_threshold) * (1.0 - 1.0 / multiplier)
        else:
            v = base_threshold + (100.0 - base_threshold) * (1.0 / multiplier - 1.0)
        return min(max(v, 0.0), 100.0)

    def dssim_acceptable(self, dssim: float, base_threshold: float) -> bool:  # :454
        return dssim < self.adjust_dssim_threshold(base_threshold)

    def butteraugli_acceptable(self, butteraugli: float, base_threshold: float) -> bool:  # :460
        return butteraugli < self.adjust_butteraugli_threshold(base_threshold)

    def ssimulacra2_acceptable(self, ssimulacra2: float, base_threshold: float) -> bool:  # :466
        return ssimulacra2 > self.adjust_ssimulacra2_threshold(base_threshold)

    def displayed_size(self, width: int, height: int) -> Tuple[int, int]:
        """Not in the reference: the device pixels a `width` x `height` image occupies, `round(n / scale_factor)` per side
        and at least 1 - the size it is resampled to.  `(width, height)` when scale_factor is 1."""
        if self.scale_factor == 1.0:
            return int(width), int(height)
        return max(1, _round_u32(width / self.scale_factor)), max(1, _round_u32(height / self.scale_factor))


@dataclass(frozen=True)
class ViewingCondition:  # src/viewing.rs:74-104
    acuity_ppd: float
    browser_dppx: Optional[float] = None
    image_intrinsic_dppx: Optional[float] = None
    ppd: Optional[float] = None

    @staticmethod
    def new(acuity_ppd: float) -> "ViewingCondition":  # :113
        return ViewingCondition(float(acuity_ppd))

    @staticmethod
    def desktop() -> "ViewingCondition":  # :127
        return ViewingCondition.new(40.0)

    @staticmethod
    def laptop() -> "ViewingCondition":  # :136
        return ViewingCondition.new(60.0)

    @staticmethod
    def smartphone() -> "ViewingCondition":  # :145
        return ViewingCondition.new(90.0)

    @staticmethod
    def default() -> "ViewingCondition":  # :471-475
        return ViewingCondition.desktop()

    def with_browser_dppx(self, dppx: float) -> "ViewingCondition":  # :155
        return replace(self, browser_dppx=float(dppx))

    def with_image_intrinsic_dppx(self, dppx: float) -> "ViewingCondition":  # :166
        return replace(self, image_intrinsic_dppx=float(dppx))

    def with_ppd_override(self, ppd: float) -> "ViewingCondition":  # :177
        return replace(self, ppd=float(ppd))

    def effective_ppd(self) -> float:  # :194-206
        if self.ppd is not None:
            return self.ppd
        return self.acuity_ppd * self.srcset_ratio()

    def srcset_ratio(self) -> float:  # :214-218
        browser = 1.0 if self.browser_dppx is None else self.browser_dppx
        intrinsic = 1.0 if self.image_intrinsic_dppx is None else self.image_intrinsic_dppx
        return intrinsic / browser

    def simulation_params(self, image_width: int, image_height: int, mode: SimulationMode = SimulationMode.Accurate) -> SimulationParams:
        """src/viewing.rs:244-301."""
        ratio = self.srcset_ratio()
        if mode == SimulationMode.Accurate or ratio >= 1.0:
            return SimulationParams(ratio, _round_u32(image_width * ratio), _round_u32(image_height * ratio), self.effective_ppd(),
                                    ratio < 1.0 if mode == SimulationMode.Accurate else False, ratio > 1.0)
        # DownsampleOnly, undersized: the image stays as it is and the PPD carries the missing upscale
        return SimulationParams(1.0, int(image_width), int(image_height), self.acuity_ppd * ratio, False, False)


class presets:  # src/viewing.rs:495-656
    @staticmethod
    def native_desktop() -> ViewingCondition:
        return ViewingCondition.new(40.0).with_browser_dppx(1.0).with_image_intrinsic_dppx(1.0)

    @staticmethod
    def native_laptop() -> ViewingCondition:
        return ViewingCondition.new(70.0).with_browser_dppx(2.0).with_image_intrinsic_dppx(2.0)

    @staticmethod
    def native_phone() -> ViewingCondition:
        return ViewingCondition.new(95.0).with_browser_dppx(3.0).with_image_intrinsic_dppx(3.0)

    @staticmethod
    def srcset_1x_on_phone() -> ViewingCondition:
        return ViewingCondition.new(95.0).with_browser_dppx(3.0).with_image_intrinsic_dppx(1.0)

    @staticmethod
    def srcset_1x_on_laptop() -> ViewingCondition:
        return ViewingCondition.new(70.0).with_browser_dppx(2.0).with_image_intrinsic_dppx(1.0)

    @staticmethod
    def srcset_2x_on_phone() -> ViewingCondition:
        return ViewingCondition.new(95.0).with_browser_dppx(3.0).with_image_intrinsic_dppx(2.0)

    @staticmethod
    def srcset_2x_on_desktop() -> ViewingCondition:
        return ViewingCondition.new(40.0).with_browser_dppx(1.0).with_image_intrinsic_dppx(2.0)

    @staticmethod
    def srcset_2x_on_laptop_1_5x() -> ViewingCondition:
        return ViewingCondition.new(70.0).with_browser_dppx(1.5).with_image_intrinsic_dppx(2.0)

    @staticmethod
    def srcset_3x_on_phone() -> ViewingCondition:
        return presets.native_phone()

    @staticmethod
    def all() -> List[ViewingCondition]:  # most demanding first
        p = presets
        return [p.srcset_1x_on_phone(), p.srcset_1x_on_laptop(), p.native_desktop(), p.srcset_2x_on_phone(), p.native_laptop(),
                p.srcset_2x_on_desktop(), p.srcset_2x_on_laptop_1_5x(), p.native_phone()]

    @staticmethod
    def key() -> List[ViewingCondition]:
        return [presets.native_desktop(), presets.native_laptop(), presets.native_phone()]

    @staticmethod
    def baseline() -> ViewingCondition:
        return presets.native_laptop()

    @staticmethod
    def demanding() -> ViewingCondition:
        return presets.native_desktop()


# ---- scoring at the displayed size ---------------------------------------------------------------------------------
# the reference's "imperceptible" thresholds at REFERENCE_PPD (src/metrics/mod.rs:189-235; the examples of
# src/viewing.rs:391, 416, 429), which ConditionScores carries adjusted to the condition
BASE_DSSIM_THRESHOLD, BASE_BUTTERAUGLI_THRESHOLD, BASE_SSIMULACRA2_THRESHOLD = 0.0003, 1.0, 90.0


@dataclass
class ConditionScores:
    """One condition's share of `score_under`."""
    condition: ViewingCondition
    params: SimulationParams
    displayed_size: Tuple[int, int]
    results: list  # MetricResult per pair
    dssim_threshold: float
    butteraugli_threshold: float
    ssimulacra2_threshold: float


def score_under(ctx, batch, n_refs: int, n_pairs: int, conditions: Sequence[ViewingCondition],
                mode: SimulationMode = SimulationMode.Accurate, config=None, filter: Optional[int] = None) -> List[ConditionScores]:
    """Score the resident RGB8 or linear `batch` (references [0, n_refs), pairs [0, n_pairs)) under every condition, each
    at the size that condition displays the images: one device-side resample and one launch per distinct displayed shape,
    no upload.  A linear batch is resampled in linear light into linear batches.  A shape's
    destination batch is sized with estimate_batch_bytes (_linear for a linear batch) against a third of the free device memory;
    when the whole grid does not fit, the pairs go through it in chunks (every chunk carries all n_refs references).
    Conditions that display the images as they are score `batch` itself."""
    from . import (RESAMPLE_LANCZOS3, Batch, MetricConfig, MetricResult, _error_obj, estimate_batch_bytes, estimate_batch_bytes_linear)

    config = config or MetricConfig.all()
    filter = RESAMPLE_LANCZOS3 if filter is None else filter
    w, h = batch.width, batch.height
    linear = bool(getattr(batch, "linear", False))
    estimate = estimate_batch_bytes_linear if linear else estimate_batch_bytes
    params = [c.simulation_params(w, h, mode) for c in conditions]
    by_shape = {}

    def collect(scores):
        out = []
        for s in scores:
            if s.status != 0:
                raise _error_obj(s.status, ctx._err())
            out.append(MetricResult.from_c(s))
        return out

    for p in params:
        shape = p.displayed_size(w, h)
        if shape in by_shape:
            continue
        if shape == (w, h):
            by_shape[shape] = collect(batch.run(n_pairs, config))
            continue
        ow, oh = shape
        free, _total = ctx.memory_info()
        budget = int(os.environ.get("CE_VIEWING_BATCH_BYTES", 0)) or free // 3
        fixed = estimate(ow, oh, n_refs, 0, config)
        per_pair = max(estimate(ow, oh, n_refs, 1, config) - fixed, 1)
        chunk = int(min(n_pairs, max(1, (budget - fixed) // per_pair)))
        results = []
        if chunk >= n_pairs:
            dst = Batch(ctx, ow, oh, n_refs, n_pairs, linear=linear)
            try:
                batch.resample_pairs_into(dst, n_refs, n_pairs, filter)
                results = collect(dst.run(n_pairs, config))
            finally:
                dst.close()
        else:
            # every pair is resampled once into `shown`, a batch that is never launched and so holds its slabs only; its
            # tests then go chunk by chunk (device copies on the context's stream) through `dst`, which holds the references
            shown = Batch(ctx, ow, oh, n_refs, n_pairs, linear=linear)
            dst = Batch(ctx, ow, oh, n_refs, chunk, linear=linear)
            try:
                batch.resample_into(dst, 0, n_refs, False, filter)
                batch.resample_into(shown, 0, n_pairs, True, filter)
                img = ow * oh * (12 if linear else 3)
                for o in range(0, n_pairs, chunk):
                    m = min(chunk, n_pairs - o)
                    ctx.copy_device(dst.test_slab, shown.test_slab + o * img, m * img)
                    for i in range(m):
                        dst.bind_pair(i, batch.pair_reference(o + i))
                    results += collect(dst.run(m, config))
            finally:
                shown.close()
                dst.close()
        by_shape[shape] = results
    return [ConditionScores(c, p, p.displayed_size(w, h), by_shape[p.displayed_size(w, h)],
                            p.adjust_dssim_threshold(BASE_DSSIM_THRESHOLD), p.adjust_butteraugli_threshold(BASE_BUTTERAUGLI_THRESHOLD),
                            p.adjust_ssimulacra2_threshold(BASE_SSIMULACRA2_THRESHOLD))
            for c, p in zip(conditions, params)]
