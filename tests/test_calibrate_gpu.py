"""-m gpu: MarconetPipeline.calibrate — the precision margin guard end to end.

  * the report against a hand run: sr / prior64 / prior32 max |mode - reference| equal, bit for bit, what two ordinary runs in the two modes give on the host;
  * state: apply=False leaves the pipeline and every module as they were (the following forward_batch returns the same bytes), apply=True on a failing case
    leaves what a pipeline constructed at the reference mode computes;
  * agreement with the CPU oracle wherever the oracle can decide.  With e_m = |mode - oracle|, e_r = |reference - oracle| and d = |mode - reference| (all max-abs
    on the SR output), e_m - e_r <= d <= e_m + e_r: the guard must trip when e_m - e_r > tol and pass when e_m + e_r <= tol; nothing is asserted in between.
    Measured on the MI355X (tol 5e-4, reference fp16x3; precision_guard.json in the report directory holds every row):
        must pass  trained_like x full16, fp16x2                   e_m 4.0e-5  e_r 1.9e-6  d 4.1e-5
        must pass  tame x edges, fp16x2                            e_m 2.4e-4  e_r 2.8e-5  d 2.4e-4
        must trip  tame x edges, fp16x2 + scale branches in fp16   e_m 9.6e-4  e_r 2.8e-5  d 9.7e-4
        must trip  tame x grid, fp16                               e_m 1.3e-2  e_r 2.6e-5  d 1.3e-2
    and the planted-outlier nets of tests/test_stress_gpu.py, recorded on a device for the first time (consistency is all that is asserted of them):
        x100, fp16x2                                               e_m 3.4e-4  e_r 4.6e-5  d 3.1e-4   passes
        x1000_trunk_gn, fp16x2                                     e_m 2.8e-4  e_r 4.6e-5  d 2.9e-4   passes
        x1000_fuse64_gn, fp16x2                                    e_m 1.6e-3  e_r 3.2e-4  d 1.5e-3   trips
  * localisation: a gain planted in conv_64_fuse.0.norm2 changes the records of feat64_fused and sr and of no stage before them.
Inputs are those of tests/test_stress_gpu.py::_outlier_case (lq seed 77, labels seed 78, 8 glyphs) and tests/golden/cases.py: the session's oracle memo is shared."""
import json
import os

import pytest
import torch

from oracle import marconet_oracle as O
from oracle import synth
from tests.golden import cases
from tests.test_stress_gpu import OUTLIERS, _outlier_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 5e-4
ROWS = {}
CLASSES = {"must_pass": [], "must_trip": []}


@pytest.fixture(scope="module", autouse=True)
def _dump_rows(report_dir):
    yield
    with open(os.path.join(report_dir, "precision_guard.json"), "w") as f:
        json.dump({"tol": TOL, "reference": "fp16x3", "rows": ROWS, "classes": CLASSES}, f, indent=1, sort_keys=True)


_PIPES = {}


def _pipe(key, sde, sdg, sds):
    """one pipeline per weight set for the module (weights are packed once per precision mode)"""
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    if key not in _PIPES:
        _PIPES[key] = MarconetPipeline(*checkpoints.build_networks(sde, sdg, sds, DEV), precision="fp32")
    return _PIPES[key]


def _configure(pipe, mode, plan=None):
    pipe.set_precision(mode)
    pipe.sr.scale_branch_precision = plan
    return pipe


def _outlier_input():
    n = 8
    return synth.make_lq(77, 1, [512]), [synth.make_labels(78, n)], synth.make_locs([n], [512])


def _state(pipe):
    return (pipe.precision, pipe.encoder.precision, pipe.encoder.resnet.precision, pipe.gan.precision, pipe.gan.TextGenerator.precision,
            pipe.sr.precision, pipe.sr.scale_branch_precision, pipe.prior_image_precision, pipe.check_finite)


def _maxabs(a, b):
    return (a - b).abs().max().item()


# ================================================================================================================ the report against a hand run
def test_report_equals_two_ordinary_runs_bit_for_bit(ckpts):
    from marconet_amd import ops
    pipe = _configure(_pipe("tame", *ckpts), "fp16x2")
    lq, labels, locs = _outlier_input()
    lqd = lq.to(DEV)
    report = pipe.calibrate(lqd, labels, locs)
    print(report)
    assert report.mode == "fp16x2" and report.reference == "fp16x3" and report.tol == TOL and report.strips == 1 and not report.applied
    y, pri = {}, {}
    for mode in ("fp16x2", "fp16x3"):
        pipe.set_precision(mode)
        y[mode] = pipe.forward_batch(lqd, labels, locs).cpu()
        w = pipe.encoder(lqd)[2]
        lab = labels[0].to(DEV)
        _, p64, p32 = pipe.gan.TextGenerator.forward_nhwc(w, lab, need_image=False, style_index=torch.zeros(lab.shape[0], dtype=torch.int64, device=DEV),
                                                          precision=mode)
        pri[mode] = (w.cpu(), ops.convert(p64, torch.float32).cpu(), ops.convert(p32, torch.float32).cpu())
    pipe.set_precision("fp16x2")
    assert report.sr.max_abs_diff == _maxabs(y["fp16x2"], y["fp16x3"]) > 0
    assert report.prior64.max_abs_diff == _maxabs(pri["fp16x2"][1], pri["fp16x3"][1]) > 0
    assert report.prior32.max_abs_diff == _maxabs(pri["fp16x2"][2], pri["fp16x3"][2]) > 0
    assert report.prior64.ref_abs_max == pri["fp16x3"][1].abs().max().item() and report.sr.ref_abs_max == y["fp16x3"].abs().max().item()
    assert report.style_w.max_abs_diff == _maxabs(pri["fp16x2"][0], pri["fp16x3"][0])          # (0: the fp16x2 mode runs the encoder's ResNet in fp16x3)
    # the worst element is where the host finds it: glyph-major for the priors, NCHW for the SR output
    d = (y["fp16x2"] - y["fp16x3"]).abs().reshape(-1)
    assert report.sr.worst_index == int((d == d.max()).nonzero()[0]) and report.sr.worst_strip == 0
    assert len(report.prior64.records) == 8 and len(report.sr.records) == 1 and report.prior64.per_strip == [report.prior64.max_abs_diff]
    assert report.nonfinite == 0 and report.ok and report.sr.rel == report.sr.max_abs_diff
    rms = ((y["fp16x2"] - y["fp16x3"]).double() ** 2).mean().sqrt().item()
    assert abs(report.sr.rms - rms) <= 1e-9 * rms


# ================================================================================================================ state
def test_apply_false_changes_nothing_and_apply_true_leaves_the_reference_pipeline(ckpts):
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    pipe = _configure(_pipe("tame", *ckpts), "fp16", plan=None)
    lq, labels, locs = _outlier_input()
    lqd = lq.to(DEV)
    before, y0 = _state(pipe), pipe.forward_batch(lqd, labels, locs)
    report = pipe.calibrate(lqd, labels, locs)                            # plain fp16 is at 1e-2: fails, nothing applied
    assert not report.ok and not report.applied and _state(pipe) == before
    assert torch.equal(pipe.forward_batch(lqd, labels, locs), y0)
    with pytest.raises(ArithmeticError):
        report.raise_if_failed()
    # the same with the per-layer plan set: it belongs to the mode run, and it is still there afterwards
    _configure(pipe, "fp16x2", plan="fp16")
    before, y1 = _state(pipe), pipe.forward_batch(lqd, labels, locs)
    r2 = pipe.calibrate(lqd, labels, locs)
    assert _state(pipe) == before and torch.equal(pipe.forward_batch(lqd, labels, locs), y1) and "scale branches fp16" in r2.mode
    # a passing check with apply=True applies nothing
    _configure(pipe, "fp16x2")
    before = _state(pipe)
    r3 = pipe.calibrate(lqd, labels, locs, apply=True)
    assert r3.ok and not r3.applied and _state(pipe) == before
    # a failing one: what follows is a pipeline constructed at the reference mode, byte for byte
    _configure(pipe, "fp16", plan="fp16")
    r4 = pipe.calibrate(lqd, labels, locs, apply=True)
    assert not r4.ok and r4.applied and pipe.precision == "fp16x3" and pipe.sr.scale_branch_precision is None
    fresh = MarconetPipeline(*checkpoints.build_networks(*ckpts, DEV), precision="fp16x3")
    assert _state(pipe) == _state(fresh)
    assert torch.equal(pipe.forward_batch(lqd, labels, locs), fresh.forward_batch(lqd, labels, locs))
    with pytest.raises(ValueError):
        pipe.calibrate(lqd, labels, locs)                                 # fp16x3 against fp16x3
    assert pipe.calibrate(lqd, labels, locs, reference="fp32").ok


# ================================================================================================================ agreement with the oracle
def _case_weights(weights, ckpts, harness_weights):
    if weights == "tame":
        return ckpts
    if weights == "trained_like":
        return harness_weights["trained_like"][:3]
    sdg, sds = _outlier_case(weights)
    return ckpts[0], sdg, sds


# name: (class or None = record only, weights, input, mode, scale-branch plan)
ORACLE_CASES = {
    "trained_like.full16.fp16x2": ("must_pass", "trained_like", "full16", "fp16x2", None),
    "tame.edges.fp16x2": ("must_pass", "tame", "edges", "fp16x2", None),
    "tame.edges.fp16x2+scale_fp16": ("must_trip", "tame", "edges", "fp16x2", "fp16"),
    "tame.grid.fp16": ("must_trip", "tame", "grid", "fp16", None),
    "x100.fp16x2": (None, "x100", "outlier", "fp16x2", None),
    "x1000_trunk_gn.fp16x2": (None, "x1000_trunk_gn", "outlier", "fp16x2", None),
    "x1000_fuse64_gn.fp16x2": (None, "x1000_fuse64_gn", "outlier", "fp16x2", None),
}
assert {c[1] for c in ORACLE_CASES.values()} >= set(OUTLIERS)


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_guard_agrees_with_the_oracle_where_the_oracle_can_decide(name, ckpts, harness_weights):
    cls, weights, inp, mode, plan = ORACLE_CASES[name]
    sde, sdg, sds = _case_weights(weights, ckpts, harness_weights)
    lq, locs, labels = cases.sr_input(inp) if inp != "outlier" else (lambda a, b, c: (a, c, b))(*_outlier_input())
    ref = O.end_to_end(sde, sdg, sds, lq, labels, locs)["sr"]
    pipe = _pipe(weights, sde, sdg, sds)
    lqd = lq.to(DEV)
    y_r = _configure(pipe, "fp16x3").forward_batch(lqd, labels, locs).cpu()
    y_m = _configure(pipe, mode, plan).forward_batch(lqd, labels, locs).cpu()
    e_m, e_r = _maxabs(y_m, ref), _maxabs(y_r, ref)
    report = pipe.calibrate(lqd, labels, locs)
    d = report.sr.max_abs_diff
    row = {"class": cls, "e_m": e_m, "e_r": e_r, "d": d, "ok": report.ok, "first_stage_over": report.first_stage_over, "mode": report.mode,
           "rel": {s.name: s.rel for s in report.stages()}, "worst_strip": report.sr.worst_strip}
    ROWS[name] = row
    print("%-32s e_m %.3e  e_r %.3e  d %.3e  %s  first over: %s" % (name, e_m, e_r, d, "ok" if report.ok else "TRIPPED", report.first_stage_over))
    print(report)
    assert report.nonfinite == 0 and d == _maxabs(y_m, y_r)
    if e_m - e_r > TOL:
        assert not report.ok, row
        row["decided"] = "must_trip"
    elif e_m + e_r <= TOL:
        assert report.ok, row
        row["decided"] = "must_pass"
    else:
        row["decided"] = None                     # between the two: the oracle cannot decide, recorded only
    if row["decided"]:
        CLASSES[row["decided"]].append(name)
    if cls is not None:
        assert row["decided"] == cls, "%s is no member of its class any more: %r" % (name, row)


def test_each_class_has_its_member():
    """(runs after the cases above) neither branch of the oracle agreement passed vacuously"""
    assert CLASSES["must_pass"] and CLASSES["must_trip"], CLASSES


# ================================================================================================================ localisation
def test_a_gain_planted_in_conv_64_fuse_shows_from_feat64_fused_on(ckpts):
    sdg, sds = _outlier_case("x1000_fuse64_gn")
    lq, labels, locs = _outlier_input()
    lqd = lq.to(DEV)
    planted = _configure(_pipe("x1000_fuse64_gn", ckpts[0], sdg, sds), "fp16x2").calibrate(lqd, labels, locs)
    plain = _configure(_pipe("fuse64_unplanted", ckpts[0], sdg, ckpts[2]), "fp16x2").calibrate(lqd, labels, locs)
    for stage in ("style_w", "prior64", "prior32", "feat32_fused"):       # nothing upstream of conv_64_fuse reads the planted gain
        assert getattr(planted, stage) == getattr(plain, stage), stage
    assert planted.feat64_fused.records != plain.feat64_fused.records and planted.sr.records != plain.sr.records
    ROWS["localisation.x1000_fuse64_gn"] = {"planted": {s.name: s.rel for s in planted.stages()}, "unplanted": {s.name: s.rel for s in plain.stages()},
                                            "first_stage_over": planted.first_stage_over}
