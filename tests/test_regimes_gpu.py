"""-m gpu: the parity harness on weights that are NOT the friendly synthetic ones.

Two weight sets go through the same oracle-vs-HIP comparison as tests/test_modules_gpu.py, on the four SR cases of tests/golden/cases.py:
  * "trained_like": marconet_amd/synthetic.py regime="trained" — heavy-tailed conv weights, a per-channel modulation spread of 10^3,
    spectral-norm convs stored at sigma in [0.1, 10], log-normal GroupNorm gains (oracle output spans the tanh range);
  * "real_checkpoints": the reference's own files (checkpoints/download_github.py:4-6, loaded as test_sr.py:43-51 does) when
    MARCONET_CKPT_DIR holds them — absent in this build (no network), then skipped.
Bar (BASELINE.json north_star): SR max-abs <= 1e-3 against the CPU oracle on the same weights, character indices bit-exact — for every
mode that claims the bar (fp32, fp16x3, fp16x2).  The margins are written to gpurun_out/regime_parity.json."""
import json
import os

import pytest
import torch

from oracle import marconet_oracle as O
from tests.golden import cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3
REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_report(report_dir):
    yield
    with open(os.path.join(report_dir, "regime_parity.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def regime_pipes(harness_weights):
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    pipes = {}
    for name, (sde, sdg, sds, source) in harness_weights.items():
        pipes[name] = (MarconetPipeline(*checkpoints.build_networks(sde, sdg, sds, DEV), precision="fp32"), (sde, sdg, sds), source)
    return pipes


@pytest.mark.parametrize("weights", ["trained_like", "real_checkpoints"])
@pytest.mark.parametrize("name", sorted(cases.SR_CASES))
def test_whole_chain_meets_the_bar_on_other_weight_regimes(name, weights, regime_pipes):
    if weights not in regime_pipes:
        pytest.skip("MARCONET_CKPT_DIR not set: the reference's real checkpoints are not in this build (no network)")
    pipe, (sde, sdg, sds), source = regime_pipes[weights]
    lq, locs, labels = cases.sr_input(name)
    ref = O.end_to_end(sde, sdg, sds, lq, labels, locs)
    ref_sr, ref_arg = ref["sr"], ref["logits"].argmax(-1)
    top = ref["logits"].topk(2, -1).values
    # the regime must be a real test: finite, tanh not saturated, output of ordinary size
    assert torch.isfinite(ref_sr).all() and float(ref_sr.abs().max()) > 0.3 and float((ref_sr.abs() > 0.999).float().mean()) < 0.05
    row = {"weights": source, "oracle_sr_abs_max": float(ref_sr.abs().max()), "min_top2_logit_gap": float((top[..., 0] - top[..., 1]).min())}
    for prec in ("fp32", "fp16x3", "fp16x2"):
        pipe.set_precision(prec)
        y = pipe.forward_batch(lq.to(DEV), labels, locs)
        lg = pipe.encoder(lq.to(DEV))[0]
        err = (y.cpu() - ref_sr).abs().max().item()
        same = bool(torch.equal(lg.argmax(-1).cpu(), ref_arg))
        row["sr_max_abs_%s" % prec] = err
        row["margin_%s" % prec] = TOL / max(err, 1e-12)
        row["indices_exact_%s" % prec] = same
        print("%-16s %-10s %-7s sr max-abs %.3e (margin %.1fx)  indices exact: %s" % (weights, name, prec, err, TOL / max(err, 1e-12), same))
        assert err <= TOL, "%s / %s / %s: %.3e" % (weights, name, prec, err)
        assert same
    pipe.set_precision("fp32")
    REPORT["%s.%s" % (weights, name)] = row


def test_generator_priors_on_the_trained_like_regime(regime_pipes):
    """TSPGAN alone (test_w.py path) with a per-channel modulation spread of 10^3: image and both priors against the oracle"""
    pipe, (sde, sdg, sds), _ = regime_pipes["trained_like"]
    from marconet_amd import synthetic
    styles, labels = synthetic.make_styles(91, 6), synthetic.make_labels(92, 6)
    ref = O.tspgan_forward(sdg, styles, labels)
    # (round 6: the fp16x2 bars are the north star's — 1e-3 absolute on the image, 1e-3 x max(1, |p|) on the priors; the image's own level runs in fp16x3 when the
    #  image is returned: networks.returned_image_precision)
    # (the "fp16x2" row calls the MODULE, which runs the whole generator in fp16x3 arithmetic in that mode — TextGenerator.module_call_fp16x3; the mode's own
    #  arithmetic, fold included, is test_generator_fp16x2_arithmetic_on_the_trained_like_regime below)
    for prec, bars in (("fp32", (1e-3, 1e-3, 1e-3)), ("fp16x3", (1e-3, 1e-3, 1e-3)), ("fp16x2", (1e-3, 1e-3, 1e-3))):
        pipe.gan.set_precision(prec)
        out = pipe.gan(styles=styles.to(DEV), labels=labels.to(DEV), noise=None)
        errs = [(o.cpu() - r).abs().max().item() for o, r in zip(out, ref)]
        REPORT["trained_like.gan.%s" % prec] = {"image": errs[0], "prior64": errs[1], "prior32": errs[2],
                                                "oracle_prior64_abs_max": float(ref[1].abs().max()), "oracle_prior32_abs_max": float(ref[2].abs().max())}
        print("trained_like gan %-7s image %.3e prior64 %.3e prior32 %.3e (|p64| max %.2f)" % (prec, errs[0], errs[1], errs[2], float(ref[1].abs().max())))
        # the image is a tanh output (absolute bar); the priors are unbounded features (|p| up to ~10): bar relative to their size
        assert errs[0] <= bars[0]
        assert errs[1] <= bars[1] * max(1.0, float(ref[1].abs().max())) and errs[2] <= bars[2] * max(1.0, float(ref[2].abs().max()))
    pipe.gan.set_precision("fp32")


# ---------------------------------------------------------------------------------------------------------------- the generator's own fp16x2 arithmetic
BAR_FP16X2_PRIORS = 1e-3      # the north star's bar: the measured errors pass it (table in the test's docstring)
K_FOLD = 1.038 + 0.25         # the largest fold / two-launch ratio of the table + 0.25 for the unmeasured seeds, as K_END_TO_END of tests/test_upfold_gpu.py


def fp16x2_prior_errors(tg, sdg, seed, monkeypatch):
    """forward_nhwc(need_image=False, precision="fp16x2") on make_styles(seed, 6) / make_labels(seed + 1, 6), as shipped ("fold") and with networks._NO_UPFOLD
    ("two_launch") → {form: (fold launches, prior64 error, prior32 error)}, (max |prior64|, max |prior32|) of the oracle; errors are max-abs against the oracle"""
    from marconet_amd import networks, ops, synthetic
    styles, labels = synthetic.make_styles(seed, 6), synthetic.make_labels(seed + 1, 6)
    ref = O.tspgan_forward(sdg, styles, labels)
    sd, ld = styles.to(DEV).float().contiguous(), labels.to(DEV).long().contiguous()
    out = {}
    for form, knob in (("fold", False), ("two_launch", True)):
        calls = [0]
        fold = ops.upfold3x3
        with monkeypatch.context() as m:
            m.setattr(ops, "upfold3x3", lambda *a, **k: (calls.__setitem__(0, calls[0] + 1), fold(*a, **k))[1])
            m.setattr(networks, "_NO_UPFOLD", knob)
            with torch.no_grad(), ops.on_device(sd):
                img, p64, p32 = tg.forward_nhwc(sd, ld, need_image=False, precision="fp16x2")
                p64, p32 = ops.nhwc_to_nchw(p64), ops.nhwc_to_nchw(p32)
            torch.cuda.synchronize()
        assert img is None
        out[form] = (calls[0], (p64.cpu() - ref[1]).abs().max().item(), (p32.cpu() - ref[2]).abs().max().item())
    return out, (float(ref[1].abs().max()), float(ref[2].abs().max()))


def test_generator_fp16x2_arithmetic_on_the_trained_like_regime(regime_pipes, monkeypatch):
    """The "fp16x2" row of test_generator_priors_on_the_trained_like_regime goes through the module call, which runs fp16x3 (TextGenerator.module_call_fp16x3).
    This one runs forward_nhwc in the mode's OWN arithmetic — the only one that takes the tap-conv + fold form of the 16→32 and 32→64 up-convs — as shipped and
    with the fold switched off, and compares both priors with the oracle (never with each other).

    Max-abs errors against the oracle measured on an MI355X, trained-like weights, 6 glyphs, styles / labels seeds s / s + 1 (max |prior64| 6.6 ... 7.1,
    max |prior32| 6.1 ... 8.0):
        seed   prior64 fold  two-launch  ratio    prior32 fold  two-launch  ratio
        91     2.208e-4      2.127e-4    1.038    2.190e-4      2.251e-4    0.973
        92     2.470e-4      2.489e-4    0.992    2.187e-4      2.110e-4    1.037
        93     2.736e-4      2.857e-4    0.958    2.763e-4      2.684e-4    1.030
    Absolute bar: 1e-3 x max(1, max |p|), the north star's — every measured error is below 1e-3 even without the factor max |p| (at most 4.1e-5 x max |p|), so the
    documented claim for the fp16x2 priors stands as it is.  K_FOLD = 1.038 + 0.25.  The test runs seed 91."""
    pipe, (sde, sdg, sds), _ = regime_pipes["trained_like"]
    errs, (m64, m32) = fp16x2_prior_errors(pipe.gan.TextGenerator, sdg, 91, monkeypatch)
    REPORT["trained_like.gan.fp16x2_own_arithmetic"] = {"fold": errs["fold"], "two_launch": errs["two_launch"], "oracle_prior64_abs_max": m64,
                                                        "oracle_prior32_abs_max": m32, "bar": BAR_FP16X2_PRIORS, "K": K_FOLD}
    for form in ("fold", "two_launch"):
        print("trained_like gan fp16x2 own arithmetic %-10s fold launches %d  prior64 %.3e (|p| max %.2f)  prior32 %.3e (|p| max %.2f)"
              % ((form,) + errs[form][:2] + (m64, errs[form][2], m32)))
    assert errs["fold"][0] == 2 and errs["two_launch"][0] == 0                    # 16→32 and 32→64 take the fold; the knob takes it away
    for form in ("fold", "two_launch"):
        assert errs[form][1] <= BAR_FP16X2_PRIORS * max(1.0, m64), (form, errs[form])
        assert errs[form][2] <= BAR_FP16X2_PRIORS * max(1.0, m32), (form, errs[form])
    assert errs["two_launch"][1] > 0.0 and errs["two_launch"][2] > 0.0
    assert errs["fold"][1] <= K_FOLD * errs["two_launch"][1] and errs["fold"][2] <= K_FOLD * errs["two_launch"][2]
