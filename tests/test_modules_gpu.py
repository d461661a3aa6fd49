"""-m gpu: module-level parity of the HIP path (through the C-ABI) against the CPU oracle on the same seeded
checkpoints and inputs, and directly against the golden vectors generated from the real reference.

Bars (BASELINE.json north_star): fp32 mode ≤ 1e-3 max-abs on every output, argmax(logits) bit-exact.
The fp16 throughput mode's deviation is *reported* (gpurun_out/parity_r1.json) and only loosely bounded."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import marconet_oracle as O
from oracle import synth
from tests.golden import cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3
REPORT = {}


def _err(a, b):
    return (a.detach().float().cpu() - b).abs().max().item()


def _note(key, val):
    REPORT[key] = val
    print("%-48s %s" % (key, ("%.3e" % val) if isinstance(val, float) else val))


@pytest.fixture(scope="module")
def nets(ckpts):
    from marconet_amd import networks
    enc, gan, sr = networks.TextContextEncoderV2(), networks.TSPGAN(), networks.TSPSRNet()
    enc.load_state_dict(ckpts[0], strict=True)
    gan.load_state_dict(ckpts[1], strict=True)
    sr.load_state_dict(ckpts[2], strict=True)
    return [m.eval().to(DEV).set_precision("fp32") for m in (enc, gan, sr)]


@pytest.fixture(scope="module", autouse=True)
def _dump_report(report_dir):
    yield
    with open(os.path.join(report_dir, "parity_r1.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


def test_native_library_is_the_one_running():
    from marconet_amd import _lib
    _lib.load()
    maps = open("/proc/self/maps").read()
    assert "libmarconet_hip.so" in maps


def test_encoder_parity_fp32(nets, ckpts, golden):
    lq = cases.encoder_input()
    with torch.no_grad():
        ref = O.encoder_forward(ckpts[0], lq)
    logits, locs, w = nets[0](lq.to(DEV))
    assert logits.shape == (2, 64, 6736) and locs.shape == (2, 32) and w.shape == (2, 512)
    assert logits.dtype == torch.float32 and logits.is_cuda
    for name, a, b in (("logits", logits, ref[0]), ("locs", locs, ref[1]), ("w", w, ref[2])):
        e = _err(a, b)
        _note("enc.fp32.%s.maxabs" % name, e)
        assert e <= TOL
    am = logits.argmax(-1).cpu()
    assert torch.equal(am, ref[0].argmax(-1)), "predicted character indices must be bit-exact"
    assert np.array_equal(am.numpy(), golden["enc.argmax"])
    assert np.abs(w.cpu().numpy() - golden["enc.w"]).max() <= TOL
    # device-side argmax kernel == torch.max(...,1)[1] of test_w.py:36
    from marconet_amd import ops
    assert torch.equal(ops.argmax_rows(logits.reshape(-1, 6736)).cpu().reshape(2, 64), ref[0].argmax(-1))


def test_resnet_and_textvit_module_signatures(nets, ckpts):
    """models/resnet.py ResNet.forward and models/textvit_arch.py TextViT.forward keep their NCHW signatures"""
    lq = cases.encoder_input()[:1]
    with torch.no_grad():
        f_ref = O.resnet45_forward(ckpts[0], lq)
        t_ref = O.textvit_forward(ckpts[0], f_ref)
    f = nets[0].resnet(lq.to(DEV))
    assert f.shape == (1, 512, 8, 512)
    e = _err(f, f_ref)
    _note("enc.fp32.resnet_feat.maxabs", e)
    assert e <= TOL
    out = nets[0].transformer(f_ref.to(DEV))
    for a, b in zip(out, t_ref):
        assert _err(a, b) <= TOL


def test_gan_parity_fp32(nets, ckpts, golden):
    styles, labels = cases.gan_input()
    with torch.no_grad():
        ref = O.tspgan_forward(ckpts[1], styles, labels)
    out = nets[1](styles=styles.to(DEV), labels=labels, noise=None)         # keyword call form of test_sr.py:183
    assert out[0].shape == (3, 3, 128, 128) and out[1].shape == (3, 256, 64, 64) and out[2].shape == (3, 512, 32, 32)
    for name, a, b in zip(("image", "prior64", "prior32"), out, ref):
        e = _err(a, b)
        _note("gan.fp32.%s.maxabs" % name, e)
        assert e <= TOL
    for k, t in (("img", out[0]), ("p64", out[1]), ("p32", out[2])):
        assert np.abs(cases.sample_map(t.cpu(), k).numpy() - golden["gan.%s_s" % k]).max() <= TOL


def test_gan_two_chars_per_sample(nets, ckpts):
    """SelectText concatenates c characters along W (networks.py:205-215): labels [N,2] → width 2·128"""
    styles = synth.make_styles(31, 2)
    labels = synth.make_labels(32, 4).reshape(2, 2)
    with torch.no_grad():
        ref = O.tspgan_forward(ckpts[1], styles, labels)
    out = nets[1](styles=styles.to(DEV), labels=labels.to(DEV), noise=None)
    assert out[0].shape == (2, 3, 128, 256)
    assert out[1].shape == (2, 512, 32, 64) and out[2].shape == (2, 512, 16, 32)     # levels picked by absolute width (:155,158)
    for a, b in zip(out, ref):
        assert _err(a, b) <= TOL


@pytest.mark.parametrize("name", list(cases.SR_CASES))
def test_sr_parity_fp32(name, nets, ckpts, golden):
    lq, locs, labels = cases.sr_input(name)
    r = O.end_to_end(ckpts[0], ckpts[1], ckpts[2], lq, labels, locs)
    # SR in isolation: oracle priors in, NCHW fp32 lists exactly like test_sr.py:197
    y = nets[2](lq.to(DEV), [p.to(DEV) for p in r["p64"]], [p.to(DEV) for p in r["p32"]], locs.to(DEV))
    assert y.shape == (lq.shape[0], 3, 128, 2048) and y.dtype == torch.float32
    e = _err(y, r["sr"])
    _note("sr.fp32.%s.isolated.maxabs" % name, e)
    assert e <= TOL
    # full HIP chain: encoder → per-image TSPGAN with the image's single w → SR (NHWC hand-over between modules)
    _, _, w = nets[0](lq.to(DEV))
    p64, p32 = [], []
    for b, lab in enumerate(labels):
        _, a, c = nets[1](styles=w[b:b + 1].repeat(lab.shape[0], 1), labels=lab, noise=None)
        p64.append(a)
        p32.append(c)
    y2 = nets[2](lq.to(DEV), p64, p32, locs.to(DEV))
    e2 = _err(y2, r["sr"])
    _note("sr.fp32.%s.chain.maxabs" % name, e2)
    assert e2 <= TOL
    g = np.abs(cases.sample_map(y2.cpu(), "sr").numpy() - golden["sr.%s.out_s" % name]).max()
    _note("sr.fp32.%s.chain.vs_golden" % name, float(g))
    assert g <= TOL


def test_batch_invariance_and_missing_priors(nets, ckpts):
    """image b of a batch == the same image run alone, bit for bit (needed for 1-vs-N GPU equality);
    an image without priors gets the plain trunk (reference: loop body skipped)."""
    lq, locs, labels = cases.sr_input("grid")
    r = O.end_to_end(ckpts[0], ckpts[1], ckpts[2], lq, labels, locs)
    p64 = [p.to(DEV) for p in r["p64"]]
    p32 = [p.to(DEV) for p in r["p32"]]
    both = nets[2](lq.to(DEV), p64, p32, locs.to(DEV))
    one = nets[2](lq[1:2].to(DEV), p64[1:], p32[1:], locs[1:2].to(DEV))
    assert torch.equal(both[1:2], one)
    a = nets[0](lq.to(DEV))
    b = nets[0](lq[:1].to(DEV))
    assert torch.equal(a[0][:1], b[0]) and torch.equal(a[2][:1], b[2])
    # only the first image has priors
    y = nets[2](lq.to(DEV), p64[:1], p32[:1], locs.to(DEV))
    with torch.no_grad():
        ref = O.tspsr_forward(ckpts[2], lq, r["p64"][:1], r["p32"][:1], locs)
    assert _err(y, ref) <= TOL


def test_fp16_throughput_mode_deviation(nets, ckpts):
    """fp16 storage / fp32 accumulate: report the measured deviation next to the fp32 numbers."""
    lq, locs, labels = cases.sr_input("grid")
    r = O.end_to_end(ckpts[0], ckpts[1], ckpts[2], lq, labels, locs)
    try:
        for m in nets:
            m.set_precision("fp16")
        logits, elocs, w = nets[0](lq.to(DEV))
        _note("enc.fp16.logits.maxabs", _err(logits, r["logits"]))
        _note("enc.fp16.w.maxabs", _err(w, r["w"]))
        _note("enc.fp16.argmax_match", float((logits.argmax(-1).cpu() == r["logits"].argmax(-1)).float().mean()))
        p64, p32 = [], []
        for b, lab in enumerate(labels):
            img, a, c = nets[1](styles=w[b:b + 1].repeat(lab.shape[0], 1), labels=lab, noise=None)
            p64.append(a)
            p32.append(c)
            if b == 0:
                _note("gan.fp16.image.maxabs", _err(img, r["prior_images"][0]))
                _note("gan.fp16.prior64.maxabs", _err(a, r["p64"][0]))
        y = nets[2](lq.to(DEV), p64, p32, locs.to(DEV))
        e = _err(y, r["sr"])
        _note("sr.fp16.grid.chain.maxabs", e)
        _note("sr.fp16.grid.chain.meanabs", (y.cpu() - r["sr"]).abs().mean().item())
        assert torch.isfinite(y).all()
        assert e <= 2.5e-2          # plain fp16 storage measures 1.1e-2 - 1.2e-2 here: a 2x regression fails
    finally:
        for m in nets:
            m.set_precision("fp32")


@pytest.mark.parametrize("prec", ["fp16x3", "fp16x2"])
@pytest.mark.parametrize("name", ["grid", "full16", "edges"])
def test_fp16x3_mode_meets_the_parity_bar(name, prec, nets, ckpts, golden):
    """the split-half (three fp16 MFMA products per multiply) and fp16+8 (f16 MFMA + one block-scaled fp8 MFMA) throughput modes
    against the north-star bar itself:
    SR <= 1e-3 max-abs vs the CPU oracle AND vs the real reference's golden samples, character indices bit-exact"""
    lq, locs, labels = cases.sr_input(name)
    r = O.end_to_end(ckpts[0], ckpts[1], ckpts[2], lq, labels, locs)
    try:
        for m in nets:
            m.set_precision(prec)
        logits, elocs, w = nets[0](lq.to(DEV))
        assert torch.equal(logits.argmax(-1).cpu(), r["logits"].argmax(-1))
        _note("enc." + prec + ".%s.logits.maxabs" % name, _err(logits, r["logits"]))
        _note("enc." + prec + ".%s.w.maxabs" % name, _err(w, r["w"]))
        assert _err(logits, r["logits"]) <= TOL and _err(w, r["w"]) <= TOL and _err(elocs, r["enc_locs"]) <= TOL
        p64, p32 = [], []
        for b, lab in enumerate(labels):
            img, a, c = nets[1](styles=w[b:b + 1].repeat(lab.shape[0], 1), labels=lab, noise=None)
            p64.append(a)
            p32.append(c)
            if b == 0:
                _note("gan." + prec + ".%s.image.maxabs" % name, _err(img, r["prior_images"][0]))
                _note("gan." + prec + ".%s.prior64.maxabs" % name, _err(a, r["p64"][0]))
                assert _err(img, r["prior_images"][0]) <= TOL and _err(a, r["p64"][0]) <= TOL
        y = nets[2](lq.to(DEV), p64, p32, locs.to(DEV))
        e = _err(y, r["sr"])
        _note("sr." + prec + ".%s.chain.maxabs" % name, e)
        assert torch.isfinite(y).all() and e <= TOL
        assert np.abs(cases.sample_map(y.cpu(), "sr").numpy() - golden["sr.%s.out_s" % name]).max() <= TOL
    finally:
        for m in nets:
            m.set_precision("fp32")


@pytest.mark.parametrize("prec", ["fp16x3", "fp16x2"])
def test_fp16x3_batched_driver_and_batch_invariance(prec, nets, ckpts):
    """forward_batch in the fp16x3 mode on bench-shaped strips vs the oracle, and a batch == its halves bit for bit"""
    from marconet_amd.pipeline import MarconetPipeline
    counts, widths = [16, 7, 16, 12], [512, 512, 400, 512]
    lq = synth.make_lq(151, 4, widths)
    labels = [synth.make_labels(160 + b, c) for b, c in enumerate(counts)]
    locs = synth.make_locs(counts, widths, max_glyphs=16)
    pipe = MarconetPipeline(*nets, precision=prec)
    try:
        y = pipe.forward_batch(lq.to(DEV), labels, locs)
        worst = 0.0
        for b in range(4):
            r = O.end_to_end(ckpts[0], ckpts[1], ckpts[2], lq[b:b + 1], [labels[b]], locs[b:b + 1])
            worst = max(worst, _err(y[b:b + 1], r["sr"]))
        _note("sr." + prec + ".forward_batch.bench_shape.maxabs", worst)
        assert worst <= TOL
        lo = pipe.forward_batch(lq[:2].to(DEV), labels[:2], locs[:2])
        hi = pipe.forward_batch(lq[2:].to(DEV), labels[2:], locs[2:])
        assert torch.equal(y[:2], lo) and torch.equal(y[2:], hi)
        u8 = pipe.forward_batch(lq.to(DEV), labels, locs, output="u8_bgr")
        assert u8.dtype == torch.uint8 and u8.shape == (4, 128, 2048, 3)
    finally:
        pipe.set_precision("fp32")


@pytest.mark.parametrize("prec", ["fp16x3", "fp16x2"])
def test_fp16x3_mixed_widths_and_reference_call_form(prec, nets, ckpts):
    """configs[4] in the split-half / fp16+8 modes: bucketed widths (row gathers of blocked-storage priors) against the oracle at the bucket width"""
    from marconet_amd.pipeline import MarconetPipeline
    widths, counts = [130, 512, 250], [2, 4, 3]
    lq = synth.make_lq(171, len(widths), widths)
    labels = [synth.make_labels(180 + i, c) for i, c in enumerate(counts)]
    locs = synth.make_locs(counts, widths)
    pipe = MarconetPipeline(*nets, precision=prec)
    try:
        outs = pipe.forward_mixed_widths(lq.to(DEV), widths, labels, locs)          # labels / locs on the host
        worst = 0.0
        with torch.no_grad():
            _, _, w = O.encoder_forward(ckpts[0], lq)
            for b, wd in enumerate(widths):
                wb = (wd + 63) // 64 * 64
                _, a, c = O.tspgan_forward(ckpts[1], w[b:b + 1].repeat(counts[b], 1), labels[b])
                # (the integer centres of the padded run, see test_config5_mixed_widths_bucketed)
                c64 = torch.trunc(locs[b:b + 1] * 1024.0)
                ref = O.tspsr_forward(ckpts[2], lq[b:b + 1, :, :, :wb], [a], [c], (c64 + 0.5) / (2.0 * wb))
                worst = max(worst, _err(outs[b], ref[0]))
        _note("sr.cfg5." + prec + ".bucketed.maxabs", worst)
        assert worst <= TOL
    finally:
        pipe.set_precision("fp32")


def test_style_normalisation_is_exact_and_removes_the_half_precision_hazard(nets, ckpts):
    """The generator normalises every style row by a power of two (mnet_style_rows) and lets the demodulation / ToRGB scale absorb it.
    (1) fp32: bit-identical to the un-normalised evaluation; (2) with modulation weights 3e4 times larger — styles no half can
    carry once multiplied into an activation — the fp16x3 priors still match the CPU oracle, while the un-normalised path overflows."""
    from marconet_amd import networks
    styles, labels = synth.make_styles(191, 3), synth.make_labels(192, 3)
    gan = nets[1]
    try:
        a = gan(styles=styles.to(DEV), labels=labels.to(DEV), noise=None)
        networks._STYLE_NORM = False
        b = gan(styles=styles.to(DEV), labels=labels.to(DEV), noise=None)
        networks._STYLE_NORM = True
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        big = {k: (v * 3e4 if ".modulation." in k else v) for k, v in ckpts[1].items()}
        g2 = networks.TSPGAN()
        g2.load_state_dict(big, strict=True)
        g2 = g2.eval().to(DEV).set_precision("fp16x3")          # (the fp16+8 mode shares the hi half and its range)
        with torch.no_grad():
            ref = O.tspgan_forward(big, styles, labels)
        out = g2(styles=styles.to(DEV), labels=labels.to(DEV), noise=None)
        assert all(bool(torch.isfinite(t).all()) for t in out)
        e64, e32 = _err(out[1], ref[1]), _err(out[2], ref[2])
        _note("gan.fp16x3.big_styles.prior64.maxabs", e64)
        assert e64 <= TOL and e32 <= TOL          # (the image is tanh(3e4 * ...): saturated, its zero crossings amplify any rounding — not compared)
        networks._STYLE_NORM = False
        bad = g2(styles=styles.to(DEV), labels=labels.to(DEV), noise=None)
        networks._STYLE_NORM = True
        # x * s leaves the half range without the normalisation: non-finite values, or (where a saturated value meets a zero) plain wrong ones
        assert (not bool(torch.isfinite(bad[1]).all())) or _err(bad[1], ref[1]) > 100 * TOL
    finally:
        networks._STYLE_NORM = True


def test_error_behaviour(nets):
    """errors surface as Python exceptions so test_sr.py's try/except…continue (:181-190) keeps working"""
    styles = synth.make_styles(1, 2).to(DEV)
    with pytest.raises(RuntimeError):
        nets[1](styles=styles, labels=torch.tensor([[3], [-1]]), noise=None)     # alphabet.find() == -1
    lq, locs, labels = cases.sr_input("edges")
    bad = locs.clone()
    bad[0, 0] = 1.2                                                             # centre-16 > 512 → empty window
    p64 = [torch.zeros(6, 256, 64, 64, device=DEV), torch.zeros(1, 256, 64, 64, device=DEV)]
    p32 = [torch.zeros(6, 512, 32, 32, device=DEV), torch.zeros(1, 512, 32, 32, device=DEV)]
    with pytest.raises(ValueError):
        nets[2](lq.to(DEV), p64, p32, bad.to(DEV))
    with pytest.raises(RuntimeError):
        nets[0](lq)                                                             # CPU tensor: no CPU path


def test_fused_act_provider_is_hip():
    """`from basicsr.ops.fused_act import fused_leaky_relu, FusedLeakyReLU` served by the HIP op"""
    from marconet_amd.fused_act import FusedLeakyReLU, fused_leaky_relu
    x, b = torch.randn(2, 7, 5, 3), torch.randn(7)
    y = fused_leaky_relu(x.to(DEV), b.to(DEV))
    assert _err(y, O.fused_leaky_relu(x, b)) <= 1e-6
    m = FusedLeakyReLU(7).to(DEV)
    with torch.no_grad():
        m.bias.copy_(b)
    assert _err(m(x.to(DEV)), O.fused_leaky_relu(x, b)) <= 1e-6


def test_pipeline_without_prior_image_gives_identical_sr(nets, ckpts):
    """the opt-in need_prior_image=False driver mode (secondary bench figure) must not change a single SR bit"""
    from marconet_amd.pipeline import MarconetPipeline
    lq = synth.make_lq(31, 2, [512, 300]).to(DEV)
    labels = [synth.make_labels(32, 5).to(DEV), synth.make_labels(33, 3).to(DEV)]
    locs = synth.make_locs([5, 3], [512, 300]).to(DEV)
    pipe = MarconetPipeline(*nets, precision="fp16")
    y1 = pipe.forward_batch(lq, labels, locs)
    pipe.need_prior_image = False
    y0 = pipe.forward_batch(lq, labels, locs)
    pipe.set_precision("fp32")
    assert torch.equal(y0, y1) and torch.isfinite(y1).all()


def test_config4_gan_only_large_batch(nets, ckpts):
    """BASELINE configs[3] (test_w.py path): TSPGAN alone on a large glyph batch, one style per 16-glyph group
    (test_w.py:104-108).  fp32 parity on a subset against the oracle; the fp16 run of the full 256 x 16 batch must be
    finite, tanh-bounded and equal (bit for bit) to the same glyphs run in a small batch (batch invariance)."""
    gan = nets[1]
    groups, n = 256, 16
    styles = synth.make_styles(41, groups).repeat_interleave(n, dim=0)
    labels = synth.make_labels(42, groups * n)
    with torch.no_grad():
        ref = O.tspgan_forward(ckpts[1], styles[:2 * n], labels[:2 * n])
    gan.set_precision("fp32")
    img, p64, p32 = gan(styles=styles[:2 * n].to(DEV), labels=labels[:2 * n].to(DEV), noise=None)
    for name, got, want in (("image", img, ref[0]), ("prior64", p64, ref[1]), ("prior32", p32, ref[2])):
        e = _err(got, want)
        _note("gan.cfg4.fp32.%s.maxabs" % name, e)
        assert e <= TOL
    gan.set_precision("fp16")
    tg = gan.TextGenerator
    big = tg.forward_nhwc(styles.to(DEV), labels.to(DEV))
    small = tg.forward_nhwc(styles[:n].to(DEV).contiguous(), labels[:n].to(DEV).contiguous())
    torch.cuda.synchronize()
    assert big[0].shape == (groups * n, 128, 128, 4) and big[0].dtype == torch.float32 and torch.isfinite(big[0]).all() and float(big[0].abs().max()) <= 1.0
    for b_, s_ in zip(big, small):
        assert torch.equal(b_[:n], s_)
    gan.set_precision("fp32")


def test_config5_mixed_widths_bucketed(nets, ckpts):
    """BASELINE configs[4]: variable-width strips bucketed by padded width.  Oracle: the reference
    TSPSRNet at the SAME bucket width W' with the glyph centres of the 512-padded run — the integer centres trunc(loc * 512) /
    trunc(loc * 1024) the locs were normalised for (re-normalising in fp32, loc * 512 / W' * W', can move a centre by one pixel);
    encoder and TSPGAN see the 512-padded strip."""
    from marconet_amd.pipeline import MarconetPipeline
    widths = [130, 200, 512, 250, 128]
    counts = [2, 3, 4, 0, 1]
    lq = synth.make_lq(51, len(widths), widths)
    labels = [synth.make_labels(60 + i, c) for i, c in enumerate(counts)]
    locs = synth.make_locs(counts, widths)
    # image 0 (bucket 192): a glyph whose window [169, 201) straddles the bucket edge, and a centre where the fp32 re-normalisation
    # loc * (512 / 192) * 192 truncates differently from loc * 512
    locs[0, 0] = 185.3 / 512.0
    locs[0, 2] = 0.1601562350988388          # just below 82 / 512: trunc(loc * 512) = 81, trunc(fp32(loc * 512 / 192) * 192) = 82
    assert int(torch.trunc(locs[0, 2] * 512.0)) == 81 and int(torch.trunc((locs[0, 2] * (512.0 / 192)) * 192.0)) == 82
    pipe = MarconetPipeline(*nets, precision="fp32")
    outs = pipe.forward_mixed_widths(lq.to(DEV), widths, [l.to(DEV) for l in labels], locs.to(DEV))
    worst = 0.0
    with torch.no_grad():
        _, _, w = O.encoder_forward(ckpts[0], lq)
        for b, wd in enumerate(widths):
            wb = (wd + 63) // 64 * 64
            if counts[b]:
                _, a, c = O.tspgan_forward(ckpts[1], w[b:b + 1].repeat(counts[b], 1), labels[b])
            else:
                a, c = torch.zeros(0, 256, 64, 64), torch.zeros(0, 512, 32, 32)
            # the oracle (the reference's arithmetic at width W') is handed locs that reproduce the integer centres of the padded run:
            # (c64 + 0.5) / (2 W') → trunc(. * 2 W') = c64 = trunc(loc * 1024) and trunc(. * W') = c64 >> 1 = trunc(loc * 512)
            c64 = torch.trunc(locs[b:b + 1] * 1024.0)
            ref = O.tspsr_forward(ckpts[2], lq[b:b + 1, :, :, :wb], [a], [c], (c64 + 0.5) / (2.0 * wb))
            assert outs[b].shape == (3, 128, 4 * wb)
            worst = max(worst, _err(outs[b], ref[0]))
    _note("sr.cfg5.fp32.bucketed.maxabs", worst)
    assert worst <= TOL
    with pytest.raises(ValueError):
        pipe.forward_mixed_widths(lq.to(DEV), [640] + widths[1:], [l.to(DEV) for l in labels], locs.to(DEV))


def test_clear_labels_locs_and_w_interpolation(nets, ckpts):
    """test_w.py path: argmax + collapse on our logits == the oracle's clear_labels on its logits (bit-exact indices),
    (left,right)→(centre,half-width), and the batched w-interpolation == one generator call per step."""
    from marconet_amd.pipeline import clear_labels_batch, locs_from_left_right, w_interpolation
    lq = synth.make_lq(71, 2, [290, 255])
    with torch.no_grad():
        ref_logits, ref_locs, ref_w = O.encoder_forward(ckpts[0], lq)
    logits, locs_lr, w = nets[0](lq.to(DEV))
    got = clear_labels_batch(logits)
    for b in range(2):
        assert got[b].reshape(-1).tolist() == O.clear_labels(ref_logits[b])
    conv = locs_from_left_right(locs_lr).cpu()
    assert torch.allclose(conv[:, 0::2], (ref_locs[:, 1::2] + ref_locs[:, 0::2]) / 2, atol=1e-5)
    assert torch.allclose(conv[:, 1::2], (ref_locs[:, 1::2] - ref_locs[:, 0::2]) / 2, atol=1e-5)
    labels = got[0][:3] if got[0].shape[0] >= 1 else synth.make_labels(72, 3)
    imgs = w_interpolation(nets[1], w[:1], w[1:2], labels, steps=3)
    for i in range(3):
        s_ = i / 2
        with torch.no_grad():
            ref = O.tspgan_forward(ckpts[1], (ref_w[:1] * s_ + ref_w[1:2] * (1 - s_)).repeat(labels.shape[0], 1), labels)[0]
        assert _err(imgs[i], ref) <= TOL


def test_forward_blind_vs_oracle(nets, ckpts):
    """the self-contained pass (labels = clear_labels(logits), test_w.py:34-40; locs = (left, right) → (centre, half-width),
    Train/tspgan/models/tspgan_model.py:331-336) against the same chain built from the oracle: identical labels, locs and SR <= 1e-3"""
    from marconet_amd.pipeline import MarconetPipeline
    pipe = MarconetPipeline(*nets, precision="fp32")
    lq = synth.make_lq(81, 2, [400, 512])
    sr, labels, locs = pipe.forward_blind(lq.to(DEV))
    assert sr.shape == (2, 3, 128, 2048) and torch.isfinite(sr).all() and len(labels) == 2 and locs.shape == (2, 32)
    with torch.no_grad():
        logits, enc_locs, w = O.encoder_forward(ckpts[0], lq)
        l, r = enc_locs[:, 0::2], enc_locs[:, 1::2]
        locs_ref = torch.stack(((r + l) / 2.0, (r - l) / 2.0), dim=2).reshape(2, 32)
        assert _err(locs, locs_ref) <= 1e-5
        p64, p32 = [], []
        for b in range(2):
            lab = [int(v) for v in O.clear_labels(logits[b])][:16]
            assert labels[b].flatten().tolist() == lab
            if lab:
                _, a, c = O.tspgan_forward(ckpts[1], w[b:b + 1].repeat(len(lab), 1), torch.tensor(lab).reshape(-1, 1))
            else:
                a, c = torch.zeros(0, 256, 64, 64), torch.zeros(0, 512, 32, 32)
            p64.append(a)
            p32.append(c)
        ref = O.tspsr_forward(ckpts[2], lq, p64, p32, locs_ref)
    e = _err(sr, ref)
    _note("sr.fp32.forward_blind.maxabs", e)
    assert e <= TOL


@pytest.mark.parametrize("precision", ["fp16", "fp16x3", "fp16x2"])
def test_full_size_batch_properties_fp16(nets, precision):
    """BASELINE configs[1] at full size (64 strips x 16 glyphs, fp16 throughput mode), checked through size-independent
    properties instead of the (hours-long) CPU oracle: the batch equals its two halves run separately bit for bit (what
    makes an N-GPU data-parallel run equal the 1-GPU run), images are processed independently (a permuted
    batch gives permuted outputs), and the output is finite and tanh-bounded."""
    from marconet_amd.pipeline import MarconetPipeline
    B, n = 64, 16
    lq = synth.make_lq(91, B, [512] * B).to(DEV)
    labels = [synth.make_labels(100 + b, n).to(DEV) for b in range(B)]
    locs = synth.make_locs([n] * B, [512] * B).to(DEV)
    pipe = MarconetPipeline(*nets, precision=precision)
    try:
        full = pipe.forward_batch(lq, labels, locs)
        assert full.shape == (B, 3, 128, 2048) and torch.isfinite(full).all() and float(full.abs().max()) <= 1.0
        h = B // 2
        lo = pipe.forward_batch(lq[:h].contiguous(), labels[:h], locs[:h].contiguous())
        hi = pipe.forward_batch(lq[h:].contiguous(), labels[h:], locs[h:].contiguous())
        assert torch.equal(full[:h], lo) and torch.equal(full[h:], hi)
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(7)).tolist()
        pt = torch.tensor(perm, device=DEV)
        shuffled = pipe.forward_batch(lq.index_select(0, pt), [labels[i] for i in perm], locs.index_select(0, pt))
        assert torch.equal(shuffled, full.index_select(0, pt))
    finally:
        pipe.set_precision("fp32")


@pytest.mark.parametrize("precision", ["fp16x2", "fp16x3"])
def test_full_size_batch_sampled_against_the_oracle(nets, ckpts, precision):
    """the full-size batch (64 strips x 16 glyphs, what bench.py runs per --batch 64) in the parity-meeting throughput modes, with THREE of
    its strips — spread over the batch, i.e. over different pixel / glyph tiles of every big launch — recomputed by the CPU oracle one
    at a time like test_sr.py:77: <= 1e-3 each (the full-size test was property-only)"""
    from marconet_amd.pipeline import MarconetPipeline
    B, n = 64, 16
    lq = synth.make_lq(91, B, [512] * B)
    labels = [synth.make_labels(100 + b, n) for b in range(B)]
    locs = synth.make_locs([n] * B, [512] * B)
    pipe = MarconetPipeline(*nets, precision=precision)
    try:
        y = pipe.forward_batch(lq.to(DEV), labels, locs).cpu()
        worst = 0.0
        for b in (0, 27, 63):
            r = O.end_to_end(ckpts[0], ckpts[1], ckpts[2], lq[b:b + 1], [labels[b]], locs[b:b + 1])
            worst = max(worst, (y[b:b + 1] - r["sr"]).abs().max().item())
        _note("sr.%s.full_batch_64x16.sampled3.maxabs" % precision, worst)
        assert worst <= TOL
    finally:
        pipe.set_precision("fp32")


@pytest.mark.parametrize("precision", ["fp16x2", "fp16x3"])
def test_generator_chunks_are_bit_exact_and_meet_the_bar(nets, ckpts, precision):
    """bench.py's batch-256 step is the only place where MarconetPipeline._core runs its glyph loop more than once
    (4096 glyphs / glyph_chunk 1024).  Here 8 strips x 16 glyphs with glyph_chunk 48 → chunks of 48, 48 and 32 glyphs that start and end
    in the middle of images: the SR output must equal the single-chunk run BIT FOR BIT (every conv gives the same bits whichever tile its
    launch size selects; the priors land in slices of the all-glyph buffers), in the default configuration and without the prior
    image (that variant in fp16x2), and three strips are recomputed by the oracle: <= 1e-3"""
    from marconet_amd.pipeline import MarconetPipeline
    B, n = 8, 16
    lq = synth.make_lq(171, B, [512] * B)
    labels = [synth.make_labels(180 + b, n) for b in range(B)]
    locs = synth.make_locs([n] * B, [512] * B)
    pipe = MarconetPipeline(*nets, precision=precision)
    try:
        whole = pipe.forward_batch(lq.to(DEV), labels, locs)
        pipe.glyph_chunk = 48
        chunked = pipe.forward_batch(lq.to(DEV), labels, locs)
        pipe.need_prior_image = False
        chunked_noimg = pipe.forward_batch(lq.to(DEV), labels, locs)
        pipe.glyph_chunk = 1024
        whole_noimg = pipe.forward_batch(lq.to(DEV), labels, locs)
        assert torch.equal(whole, chunked) and torch.equal(whole, chunked_noimg) and torch.equal(whole, whole_noimg)
        worst = 0.0
        for b in (0, 2, 7):                     # strip 2 straddles chunks 0 / 1 (glyphs 32-47 | 48-63), strip 7 is in the short last chunk
            r = O.end_to_end(ckpts[0], ckpts[1], ckpts[2], lq[b:b + 1], [labels[b]], locs[b:b + 1])
            worst = max(worst, _err(chunked_noimg[b:b + 1], r["sr"]))
        _note("sr.%s.chunked_generator_8x16_chunk48.sampled3.maxabs" % precision, worst)
        assert worst <= TOL
    finally:
        pipe.set_precision("fp32")


@pytest.mark.parametrize("precision", ["fp32", "fp16x2", "fp16x3", "fp16"])
def test_conv1_modulation_in_the_gather_equals_the_prologue_form(nets, ckpts, precision):
    """round 4: the first StyledConv's style multiply rides in the SelectText gather (mnet_embed_gather_scaled) instead of the conv prologue.
    fp32: the same fp32 product feeds the same MFMA sequence — priors bit-identical; the half-range modes round x*s to their storage once in
    either form but conv1 then runs on a different kernel (LDS-DMA instead of register-staged: other summation order): both forms within the
    mode's bar of the oracle, and of each other"""
    from marconet_amd import networks
    gan = nets[1]
    n = 6
    styles = torch.randn(n, 512, generator=torch.Generator().manual_seed(201)).to(DEV)
    labels = synth.make_labels(202, n).reshape(n, 1).to(DEV)
    gan.set_precision(precision)
    old = networks._FUSE_CONV1_MOD
    try:
        networks._FUSE_CONV1_MOD = True
        a = [t.float().cpu() for t in gan(styles, labels, None)]
        networks._FUSE_CONV1_MOD = False
        b = [t.float().cpu() for t in gan(styles, labels, None)]
    finally:
        networks._FUSE_CONV1_MOD = old
        gan.set_precision("fp32")
    with torch.no_grad():
        ref = O.tspgan_forward(ckpts[1], styles.cpu(), labels.cpu())
    tol = {"fp32": 1e-4, "fp16": 5e-2}.get(precision, TOL)
    for name, x, y, r in zip(("image", "prior64", "prior32"), a, b, ref):
        if precision == "fp32":
            assert torch.equal(x, y), name
        assert _err(x, r) <= tol and _err(y, r) <= tol, (name, _err(x, r), _err(y, r))
        _note("gan.%s.%s.conv1_modulation_gather_vs_prologue.maxabs" % (precision, name), _err(x, y))


@pytest.mark.parametrize("precision", ["fp16x2", "fp16x3"])
def test_prior_image_precision_leaves_sr_bits_unchanged(nets, ckpts, precision):
    """the batched driver runs the generator levels behind the two prior levels (they feed only the structure image it never returns,
    models/networks.py:161-164) in plain fp16: priors and SR output must not change by a bit; the image itself stays a finite,
    loosely bounded picture (reported), and TSPGAN.forward — the reference call form that RETURNS the image — keeps the mode's arithmetic"""
    from marconet_amd.pipeline import MarconetPipeline
    counts = [5, 3, 16]
    lq = synth.make_lq(191, 3, [512, 300, 512])
    labels = [synth.make_labels(192 + b, c) for b, c in enumerate(counts)]
    locs = synth.make_locs(counts, [512, 300, 512], max_glyphs=16)
    pipe = MarconetPipeline(*nets, precision=precision)
    try:
        assert pipe._image_precision() == "fp16"
        y_auto = pipe.forward_batch(lq.to(DEV), labels, locs)
        pipe.prior_image_precision = None
        assert pipe._image_precision() is None
        y_mode = pipe.forward_batch(lq.to(DEV), labels, locs)
        assert torch.equal(y_auto, y_mode) and torch.isfinite(y_auto).all()
        tg = nets[1].TextGenerator
        tg.precision = precision
        w = nets[0](lq.to(DEV))[2]
        lab = labels[2].to(DEV)
        st = w[2:3].repeat(lab.shape[0], 1).contiguous()
        img16, a16, c16 = tg.forward_nhwc(st, lab, image_precision="fp16")
        img, a, c = tg.forward_nhwc(st, lab)
        from marconet_amd import ops
        assert torch.equal(ops.convert(a16, torch.float32), ops.convert(a, torch.float32)) and torch.equal(ops.convert(c16, torch.float32), ops.convert(c, torch.float32))
        with torch.no_grad():
            ref = O.tspgan_forward(ckpts[1], O.encoder_forward(ckpts[0], lq[2:3])[2].repeat(lab.shape[0], 1), labels[2])[0]
        e_mode, e16 = _err(ops.nhwc_to_nchw(img, c=3), ref), _err(ops.nhwc_to_nchw(img16, c=3), ref)
        _note("gan.%s.image.maxabs" % precision, e_mode)
        _note("gan.%s.image_levels_in_fp16.image.maxabs" % precision, e16)
        assert e_mode <= TOL and e16 <= 2.5e-2 and torch.isfinite(img16).all()
    finally:
        pipe.set_precision("fp32")


@pytest.mark.parametrize("precision", ["fp16x2", "fp32"])
def test_forward_batch_returns_the_structure_images(nets, ckpts, precision):
    """forward_batch(return_prior=True) → (SR, prior_cha [ΣN,3,128,128]) — the generator's first return value (models/networks.py:164,
    test_sr.py:183) for every glyph of the batch, in strip order, in the MODE's arithmetic (not the plain-fp16 form a dropped image gets);
    the SR output is the same bits as without it; a pipeline that stops the generator at the 64-px level refuses"""
    from marconet_amd.pipeline import MarconetPipeline
    counts = [5, 0, 3, 16]
    widths = [512, 512, 300, 512]
    lq = synth.make_lq(391, 4, widths)
    labels = [synth.make_labels(392 + b, c) for b, c in enumerate(counts)]
    locs = synth.make_locs(counts, widths, max_glyphs=16)
    pipe = MarconetPipeline(*nets, precision=precision, glyph_chunk=7)           # chunks that straddle strips (24 glyphs = 7+7+7+3)
    try:
        y0 = pipe.forward_batch(lq.to(DEV), labels, locs)
        y, prior = pipe.forward_batch(lq.to(DEV), labels, locs, return_prior=True)
        assert torch.equal(y, y0)
        assert prior.shape == (sum(counts), 3, 128, 128) and prior.dtype == torch.float32
        with torch.no_grad():
            w = O.encoder_forward(ckpts[0], lq)[2]
            ref = torch.cat([O.tspgan_forward(ckpts[1], w[b:b + 1].repeat(c, 1), labels[b])[0] for b, c in enumerate(counts) if c])
        e = _err(prior, ref)
        _note("pipeline.%s.prior_cha.maxabs" % precision, e)
        assert e <= TOL
        pipe.need_prior_image = False
        with pytest.raises(ValueError, match="need_prior_image"):
            pipe.forward_batch(lq.to(DEV), labels, locs, return_prior=True)
    finally:
        pipe.set_precision("fp32")


def test_scale_branch_precision_plan_is_opt_in(nets, ckpts):
    """VERDICT r3 item 3 (per-layer precision plan; DESIGN.md §4, tools/precision_plan.py): the conv_32_scale / conv_64_scale branches in plain
    fp16 are the cheapest demotion on regular strips (emulated 2.5e-4 against 1.7e-4) — and still NOT the default, because the reference's
    edge-window case leaves the bar with it.  Both facts are measured here: three bench-shaped strips (plan on / off, both inside the bar)
    and the 'edges' case of tests/golden/cases.py (reported; the default must hold the bar on it)"""
    from marconet_amd.pipeline import MarconetPipeline
    B, n = 3, 16
    lq = synth.make_lq(211, B, [512] * B)
    labels = [synth.make_labels(220 + b, n) for b in range(B)]
    locs = synth.make_locs([n] * B, [512] * B)
    refs = torch.cat([O.end_to_end(ckpts[0], ckpts[1], ckpts[2], lq[b:b + 1], [labels[b]], locs[b:b + 1])["sr"] for b in range(B)])
    lq_e, locs_e, labels_e = cases.sr_input("edges")
    ref_e = O.end_to_end(ckpts[0], ckpts[1], ckpts[2], lq_e, labels_e, locs_e)["sr"]
    pipe = MarconetPipeline(*nets, precision="fp16x2")
    sr = nets[2]
    try:
        assert sr.scale_branch_precision is None and sr._scale_branch_pack() is None
        e_mode = _err(pipe.forward_batch(lq.to(DEV), labels, locs), refs)
        e_mode_edges = _err(pipe.forward_batch(lq_e.to(DEV), labels_e, locs_e), ref_e)
        sr.scale_branch_precision = "fp16"
        assert sr._scale_branch_pack() is not None
        e_plan = _err(pipe.forward_batch(lq.to(DEV), labels, locs), refs)
        e_plan_edges = _err(pipe.forward_batch(lq_e.to(DEV), labels_e, locs_e), ref_e)
        _note("sr.fp16x2.default.bench_strips.maxabs", e_mode)
        _note("sr.fp16x2.default.edges.maxabs", e_mode_edges)
        _note("sr.fp16x2.scale_branches_fp16.bench_strips.maxabs", e_plan)
        _note("sr.fp16x2.scale_branches_fp16.edges.maxabs", e_plan_edges)
        assert e_mode <= TOL and e_mode_edges <= TOL and e_plan <= TOL and e_plan_edges <= 5 * TOL
    finally:
        sr.scale_branch_precision = None
        pipe.set_precision("fp32")


def test_forward_batch_vs_oracle_on_bench_shaped_strips(nets, ckpts):
    """the batched driver (what bench.py times) against the CPU oracle on 4 strips of the bench shape — full 512-px width,
    ragged glyph counts up to the bench's 16 per image — in the fp32 parity mode: <= 1e-3, indices bit-exact"""
    from marconet_amd.pipeline import MarconetPipeline
    counts = [16, 9, 1, 13]
    widths = [512, 512, 512, 470]
    lq = synth.make_lq(131, 4, widths)
    labels = [synth.make_labels(140 + b, c) for b, c in enumerate(counts)]
    locs = synth.make_locs(counts, widths, max_glyphs=16)
    pipe = MarconetPipeline(*nets, precision="fp32")
    y = pipe.forward_batch(lq.to(DEV), labels, locs)                      # labels / locs on the host, like bench.py
    logits = nets[0](lq.to(DEV))[0]
    worst = 0.0
    for b in range(4):
        r = O.end_to_end(ckpts[0], ckpts[1], ckpts[2], lq[b:b + 1], [labels[b]], locs[b:b + 1])      # batch 1, like test_sr.py:77
        worst = max(worst, _err(y[b:b + 1], r["sr"]))
        assert torch.equal(logits[b:b + 1].argmax(-1).cpu(), r["logits"].argmax(-1))
    _note("sr.fp32.forward_batch.bench_shape.maxabs", worst)
    assert worst <= TOL


def test_generator_distinct_styles_equal_expanded(nets):
    """style_index (distinct styles + glyph→style map, what the batched driver passes) == one style row per glyph, bit for bit"""
    tg = nets[1].TextGenerator
    for prec in ("fp32", "fp16"):
        nets[1].set_precision(prec)
        tg.precision = prec
        w = synth.make_styles(111, 3).to(DEV)
        idx = torch.tensor([0, 0, 1, 2, 2, 2, 1], device=DEV)
        lab = synth.make_labels(112, 7).to(DEV)
        a = tg.forward_nhwc(w, lab, style_index=idx)
        b = tg.forward_nhwc(w.index_select(0, idx).contiguous(), lab)
        torch.cuda.synchronize()
        for u, v in zip(a, b):
            assert torch.equal(u, v)
    nets[1].set_precision("fp32")


@pytest.mark.parametrize("precision", ["fp16", "fp16x3", "fp16x2", "fp32"])
@pytest.mark.parametrize("output", ["nchw_f32", "u8_bgr"])
def test_hip_graph_replay_equals_eager(nets, output, precision):
    """GraphedForward (the whole forward of one batch signature captured in a HIP graph) gives the eager driver's bits, also
    when replayed on new LQ / labels / locations; a different glyph-count signature is refused"""
    from marconet_amd.pipeline import GraphedForward, MarconetPipeline
    pipe = MarconetPipeline(*nets, precision=precision)
    try:
        counts = [5, 0, 3]
        gf = GraphedForward(pipe, 3, counts, output=output)
        for seed in (41, 42):
            lq = synth.make_lq(seed, 3, [512, 512, 300]).to(DEV)
            labels = [synth.make_labels(seed * 10 + b, n) for b, n in enumerate(counts)]
            locs = synth.make_locs(counts, [512, 512, 300])
            want = pipe.forward_batch(lq, labels, locs, output=output)
            got = gf(lq, labels, locs).clone()
            assert got.dtype == want.dtype and torch.equal(got, want), seed
        with pytest.raises(ValueError):
            gf(lq, [labels[0], labels[2], labels[2]], locs)
        # the documented latency pattern — replay with check=False, test when the output is consumed — in every mode (the fp32 mode
        # captures no flag, overflow being impossible there, and must return quietly)
        gf(lq, labels, locs, check=False)
        gf.raise_if_not_finite()
        assert gf.has_flag == (precision != "fp32")
    finally:
        pipe.set_precision("fp32")


@pytest.mark.parametrize("precision", ["fp16", "fp16x3", "fp16x2"])
def test_packed_blob_drives_the_same_forward(nets, ckpts, tmp_path, precision):
    """SURVEY §8(f) NEXT-3: modules that attach an offline packed-weights blob (packing.save_packed / load_packed) instead of
    packing at first use give the same bits"""
    from marconet_amd import networks
    from marconet_amd.packing import load_packed, save_packed
    from marconet_amd.pipeline import MarconetPipeline
    lq = synth.make_lq(51, 2, [512, 300]).to(DEV)
    labels = [synth.make_labels(52, 4), synth.make_labels(53, 2)]
    locs = synth.make_locs([4, 2], [512, 300])
    pipe = MarconetPipeline(*nets, precision=precision)
    try:
        want = pipe.forward_batch(lq, labels, locs)
        path = str(tmp_path / "marconet.packed.safetensors")
        keys = save_packed(path, encoder=nets[0], gan=nets[1], sr=nets[2])
        fresh = [networks.TextContextEncoderV2(), networks.TSPGAN(), networks.TSPSRNet()]
        for m, sd in zip(fresh, ckpts):
            m.load_state_dict(sd, strict=True)
            m.eval().to(DEV).set_precision(precision)
        assert sorted(load_packed(path, encoder=fresh[0], gan=fresh[1], sr=fresh[2])) == keys
        for _, h in [x for m in fresh for x in __import__("marconet_amd.packing", fromlist=["_holders"])._holders(m)]:
            h._build = None                                   # any attempt to re-pack would now raise
        got = MarconetPipeline(*fresh, precision=precision).forward_batch(lq, labels, locs)
        assert torch.equal(got, want)
    finally:
        pipe.set_precision("fp32")


# ------------------------------------------------------------------------------------------------ the precision mode is an argument
# The smallest shapes the nets accept: one 32x512 strip with two glyphs.
def _small_problem():
    lq = synth.make_lq(611, 1, [512]).to(DEV)
    labels = synth.make_labels(612, 2)
    return lq, labels, synth.make_locs([2], [512]), synth.make_styles(613, 2).to(DEV)


def _f32(t):
    from marconet_amd import ops
    return t if t.dtype == torch.float32 else ops.convert(t, torch.float32)


def _same_bits(a, b):
    return len(a) == len(b) and all(u.shape == v.shape and torch.equal(_f32(u), _f32(v)) for u, v in zip(a, b))


def _module_state(nets):
    """attribute names and precision mode of every module of the three nets"""
    return {"%d.%s" % (i, name): (tuple(m.__dict__), getattr(m, "precision", None))
            for i, net in enumerate(nets) for name, m in net.named_modules()}


@pytest.mark.parametrize("precision", ["fp16x2", "fp32"])
def test_a_forward_leaves_the_modules_as_it_found_them(nets, precision):
    """no call form — module calls, the batched driver with and without the returned image, mixed widths, a HIP-graph capture and
    replay, a forward that raises — assigns an attribute of a module (its ``precision`` least of all) or leaves a new one behind"""
    from marconet_amd import networks, resnet
    from marconet_amd.pipeline import GraphedForward, MarconetPipeline
    enc, gan, sr = nets
    lq, labels, locs, styles = _small_problem()
    lab = labels.to(DEV)
    pipe = MarconetPipeline(*nets, precision=precision)

    def every_form(graph):
        enc(lq)
        _, p64, p32 = gan(styles, lab, None)
        sr(lq, [p64], [p32], locs.to(DEV))
        pipe.forward_batch(lq, [labels], locs)
        pipe.forward_batch(lq, [labels], locs, return_prior=True)
        pipe.forward_mixed_widths(lq, [512], [labels], locs)
        if graph:
            GraphedForward(pipe, 1, [2])(lq, [labels], locs)

    try:
        every_form(graph=False)                                    # warm-up: the packing for this mode is done
        before, writes = _module_state(nets), []
        with pytest.MonkeyPatch.context() as mp:
            for cls in (networks.TextContextEncoderV2, resnet.ResNet, networks.TSPGAN, networks.TextGenerator, networks.TSPSRNet):
                def record(self, name, value):
                    writes.append((type(self).__name__, name))
                    torch.nn.Module.__setattr__(self, name, value)
                mp.setattr(cls, "__setattr__", record, raising=False)
            every_form(graph=True)
            assert writes == [] and _module_state(nets) == before
            with pytest.raises(RuntimeError, match="out of range"):
                gan(styles, torch.tensor([[3], [gan.TextGenerator.class_num]], device=DEV), None)
            assert writes == [] and _module_state(nets) == before
        assert not hasattr(pipe, "_finite")
    finally:
        pipe.set_precision("fp32")


def test_precision_argument_and_attribute_mean_the_same(nets):
    """TextGenerator.forward_nhwc(precision=m) gives the bits of the same call on a generator whose mode IS m; the fp16x2 module call
    is that fp16x3 result (``module_call_fp16x3``), or the mode's own with the switch off — and the attribute reads fp16x2 throughout"""
    from marconet_amd import ops
    gan, tg = nets[1], nets[1].TextGenerator
    _, labels, _, styles = _small_problem()
    lab = labels.to(DEV)
    nchw = lambda r: (ops.nhwc_to_nchw(r[0], c=3), ops.nhwc_to_nchw(r[1]), ops.nhwc_to_nchw(r[2]))
    try:
        for mode in ("fp16x3", "fp16x2"):                           # warm-up, one forward per mode
            tg.forward_nhwc(styles, lab, precision=mode)
        gan.set_precision("fp16x3")
        want = tg.forward_nhwc(styles, lab)
        gan.set_precision("fp16x2")
        assert tg.precision == "fp16x2"
        assert _same_bits(tg.forward_nhwc(styles, lab, precision="fp16x3"), want) and tg.precision == "fp16x2"
        own = tg.forward_nhwc(styles, lab)
        assert tg.module_call_fp16x3
        assert _same_bits(gan(styles, lab, None), nchw(want)) and tg.precision == "fp16x2"
        tg.module_call_fp16x3 = False
        assert _same_bits(gan(styles, lab, None), nchw(own)) and tg.precision == "fp16x2"
    finally:
        tg.module_call_fp16x3 = True
        gan.set_precision("fp32")


def test_pipeline_mode_reaches_the_generator_without_touching_it(nets):
    """tools/precision_probe.py's form — the three nets switched one by one, ``pipe.precision`` naming the generator's mode: the
    generator runs in the pipeline's mode, and still holds what its owner set"""
    from marconet_amd.pipeline import MarconetPipeline
    enc, gan, sr = nets
    lq, labels, locs, _ = _small_problem()
    pipe = MarconetPipeline(*nets, precision="fp16x3")
    try:
        pipe.forward_batch(lq, [labels], locs, return_prior=True)                  # warm-up
        gan.set_precision("fp32")
        pipe.precision = "fp16x3"
        got = pipe.forward_batch(lq, [labels], locs, return_prior=True)
        assert gan.TextGenerator.precision == "fp32" and gan.precision == "fp32"
        pipe.set_precision("fp16x3")
        want = pipe.forward_batch(lq, [labels], locs, return_prior=True)
        assert _same_bits(got, want)
    finally:
        pipe.set_precision("fp32")


def test_encoder_resnet_mode_is_set_without_a_forward(nets, monkeypatch):
    """the encoder's ResNet keeps the three-product arithmetic in the fp16x2 mode (TextContextEncoderV2.resnet_precision) from the
    constructor and from set_precision on, not from the first forward on; the encoder's fp16x2 output is its fp16x3 output"""
    from marconet_amd import networks
    fresh = networks.TextContextEncoderV2().set_precision("fp16x2")
    assert fresh.precision == "fp16x2" and fresh.resnet.precision == "fp16x3"
    monkeypatch.setenv("MARCONET_PRECISION", "fp16x2")
    built = networks.TextContextEncoderV2()
    assert built.precision == "fp16x2" and built.resnet.precision == "fp16x3"
    enc = nets[0]
    lq = _small_problem()[0]
    try:
        for mode in ("fp16x3", "fp16x2"):                           # warm-up
            enc.set_precision(mode)(lq)
        a = enc.set_precision("fp16x2")(lq)
        b = enc.set_precision("fp16x3")(lq)
        assert _same_bits(a, b)
    finally:
        enc.set_precision("fp32")


def test_finiteness_flags_belong_to_their_call(nets):
    """a GraphedForward reads the flag its own graph refreshes, whatever the pipe has run since its capture"""
    from marconet_amd.pipeline import GraphedForward, MarconetPipeline
    lq, labels, locs, _ = _small_problem()
    pipe = MarconetPipeline(*nets, precision="fp16x2")
    try:
        pipe.forward_batch(lq, [labels], locs)                                     # warm-up
        gf = GraphedForward(pipe, 1, [2])
        gf(lq, [labels], locs, check=False)
        pipe.forward_batch(lq, [labels], locs)
        pipe.forward_mixed_widths(lq, [512], [labels], locs)
        assert gf.has_flag and gf._flag.numel() == 1
        gf.raise_if_not_finite()
        assert not hasattr(pipe, "_finite")
    finally:
        pipe.set_precision("fp32")
