"""The precision margin guard's host side: the report ``MarconetPipeline.calibrate`` returns and the logic that fills it from the records of
``ops.compare_stats`` (mnet_compare_stats).  Pure Python — no device, no torch: the decision logic is tested on hand-made records."""
import math
from dataclasses import dataclass, field
from typing import List, Optional

STAGES = ("style_w", "prior64", "prior32", "feat32_fused", "feat64_fused", "sr")       # in forward order
_RANK = {"fp16": 0, "fp16x2": 1, "fp16x3": 2, "fp32": 3}                                # by accuracy
REFERENCES = ("fp16x3", "fp32")
RECORD_FIELDS = ("max_abs_diff", "max_abs_ref", "max_abs_mode", "argmax_index", "sum_sq_diff", "sum_sq_ref", "nonfinite_mode", "nonfinite_ref")


class PrecisionMarginError(ArithmeticError):
    """``PrecisionReport.raise_if_failed``: the configured precision mode deviates from the reference mode by more than the tolerance (or
    produced a non-finite element) on the calibration strips"""


def check_reference(modes, reference):
    """``modes``: the precision modes of the pipeline and its three nets.  "fp32" is a reference for any mode (for the fp32 mode itself the
    comparison is a self-check that reports zeros); "fp16x3" only for runs whose every net is in "fp16x2" or "fp16" — a reference that is not
    more accurate than the mode says nothing about the mode's margin: ValueError."""
    if reference not in REFERENCES:
        raise ValueError("calibrate: reference must be one of %s, got %r" % (", ".join(REFERENCES), reference))
    for m in modes:
        if m not in _RANK:
            raise ValueError("calibrate: unknown precision mode %r" % (m,))
    if reference != "fp32" and any(_RANK[m] >= _RANK[reference] for m in modes):
        raise ValueError("calibrate: reference %r is not more accurate than the configured mode (%s) — use reference='fp32'"
                         % (reference, ", ".join(sorted(set(modes), key=_RANK.get))))


@dataclass
class StageReport:
    name: str
    max_abs_diff: float           # max |mode - reference| over all strips (finite pairs)
    ref_abs_max: float            # max |reference|
    rel: float                    # max_abs_diff / max(1, ref_abs_max)
    rms: float                    # sqrt(sum (mode - reference)^2 / elements)
    nonfinite_mode: int
    nonfinite_ref: int
    worst_strip: int              # the strip that holds max_abs_diff (-1: nothing compared)
    worst_index: int              # element index inside the worst GROUP (a strip's map, a glyph's prior): pixel * C + channel
    per_strip: List[float] = field(default_factory=list)      # max |mode - reference| per strip
    records: List[tuple] = field(default_factory=list)        # the device records as they came, one tuple per group in RECORD_FIELDS order


def stage_from_records(name, records, group_to_strip, n_strips, elems_per_group):
    """``records``: one mnet_cmp_stats-like object per group (attributes max_abs_diff, max_abs_ref, argmax_index, sum_sq_diff, nonfinite_mode,
    nonfinite_ref); ``group_to_strip[g]``: the strip group g belongs to (a strip's own map: g; a glyph's prior: the glyph's strip)."""
    if len(records) != len(group_to_strip):
        raise ValueError("%s: %d records for %d groups" % (name, len(records), len(group_to_strip)))
    per_strip = [0.0] * n_strips
    worst, worst_g = -1.0, -1
    for g, r in enumerate(records):
        d = float(r.max_abs_diff)
        s = group_to_strip[g]
        per_strip[s] = max(per_strip[s], d)
        if d > worst:                                    # (strictly: the first group — lowest strip — that attains the maximum)
            worst, worst_g = d, g
    n = max(1, len(records) * int(elems_per_group))
    dmax = max(worst, 0.0)
    rmax = max([float(r.max_abs_ref) for r in records] + [0.0])
    return StageReport(name=name, max_abs_diff=dmax, ref_abs_max=rmax, rel=dmax / max(1.0, rmax),
                       rms=math.sqrt(sum(float(r.sum_sq_diff) for r in records) / n),
                       nonfinite_mode=sum(int(r.nonfinite_mode) for r in records), nonfinite_ref=sum(int(r.nonfinite_ref) for r in records),
                       worst_strip=group_to_strip[worst_g] if worst_g >= 0 else -1,
                       worst_index=int(records[worst_g].argmax_index) if worst_g >= 0 else -1, per_strip=per_strip,
                       records=[tuple(getattr(r, f) for f in RECORD_FIELDS) for r in records])


def glyph_to_strip(counts):
    """glyph counts per strip → the strip of every glyph, in glyph order"""
    return [s for s, c in enumerate(counts) for _ in range(int(c))]


@dataclass
class PrecisionReport:
    """What ``MarconetPipeline.calibrate`` found.  A stage the run did not have (the priors of strips without glyphs) is None."""
    mode: str                     # the configured mode, e.g. "fp16x2" or "fp16x2 (sr scale branches: fp16)"
    reference: str
    tol: float
    strips: int
    style_w: Optional[StageReport] = None
    prior64: Optional[StageReport] = None
    prior32: Optional[StageReport] = None
    feat32_fused: Optional[StageReport] = None
    feat64_fused: Optional[StageReport] = None
    sr: Optional[StageReport] = None
    applied: bool = False

    def stages(self):
        return [getattr(self, n) for n in STAGES if getattr(self, n) is not None]

    @property
    def nonfinite(self):
        return sum(s.nonfinite_mode + s.nonfinite_ref for s in self.stages())

    @property
    def ok(self):
        """no non-finite element in any stage of either run, and the SR outputs of the two runs within ``tol`` of each other"""
        return self.sr is not None and self.nonfinite == 0 and self.sr.max_abs_diff <= self.tol

    @property
    def first_stage_over(self):
        """the first stage, in forward order, whose ``rel`` exceeds ``tol`` (None: none) — where the deviation enters; diagnostic, not part of ``ok``"""
        for s in self.stages():
            if s.rel > self.tol:
                return s.name
        return None

    def raise_if_failed(self):
        if not self.ok:
            raise PrecisionMarginError(str(self))
        return self

    def __str__(self):
        lines = ["precision margin: mode %s against reference %s on %d strip%s, tol %.3g: %s%s" %
                 (self.mode, self.reference, self.strips, "" if self.strips == 1 else "s", self.tol, "OK" if self.ok else "FAILED",
                  " (reference mode applied)" if self.applied else ""),
                 "  %-13s %11s %11s %11s %11s %9s %6s" % ("stage", "max|d|", "max|ref|", "rel", "rms", "nonfinite", "strip")]
        for s in self.stages():
            lines.append("  %-13s %11.3e %11.3e %11.3e %11.3e %9d %6d%s" % (s.name, s.max_abs_diff, s.ref_abs_max, s.rel, s.rms,
                                                                             s.nonfinite_mode + s.nonfinite_ref, s.worst_strip,
                                                                             "  > tol" if s.rel > self.tol else ""))
        if self.nonfinite:
            lines.append("  non-finite elements: %d (activations beyond the fp16 range 65504?)" % self.nonfinite)
        if self.first_stage_over is not None:
            lines.append("  the deviation first exceeds tol (relative to max(1, |ref|)) at stage %s" % self.first_stage_over)
        return "\n".join(lines)
