"""-m gpu: conv3x3 ∘ bilinear×2 in polyphase form in the fp16+8 mode (MNET_CONV_ALGO_FLAG_SHUFFLE2 + ring fix-up: ops.upconv3x3_polyphase) against the
two-launch form (ops.upsample2x + ops.conv2d) and an fp64 reference built from the same stored inputs.

Bounds.  Ring pixels (hi-res rows / columns {0, 1, last two}) are the two-launch form's own bytes.  On the interior the polyphase form multiplies the
stored input by weights combined in fp64 and rounded once, where the two-launch form rounds the up-sampled activations to storage and multiplies them
by the once-rounded weights: max-abs error against fp64 <= 1.5 x the two-launch form's on the same inputs (the margin is for the one extra rounding of
the combined weights; no activation rounding is added).  GroupNorm affine: the bound of tests/test_mx_gpu.py's gn_partial test (6e-5 of the
normalised output's range)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 1 << 16            # guard elements (4 bytes each) on either side of y

# N, low-res H x W, Cin, C
CASES = {"small_tiles": (2, 8, 32, 64, 64), "odd_width_all_sides_meet": (3, 4, 96, 64, 32), "one_wave_tile": (1, 64, 1024, 64, 64),
         "conv_final_3_channels": (2, 4, 64, 128, 64)}
_MEMO = {}


def _ops():
    from marconet_amd import ops
    return ops


def _P():
    from marconet_amd import packing
    return packing


def _rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _run(name):
    """both forms and the fp64 reference of one case, computed once per session"""
    if name in _MEMO:
        return _MEMO[name]
    ops, P = _ops(), _P()
    n, h, w, cin, c = CASES[name]
    x = _rnd((n, cin, h, w), 11)
    wt = _rnd((c, cin, 3, 3), 12, 1.0 / math.sqrt(cin * 9))
    bias = _rnd((c,), 13, 0.3)
    xd = ops.convert(x.permute(0, 2, 3, 1).contiguous().to(DEV), P.MX_DTYPE)
    xs = ops.convert(xd, torch.float32).cpu().permute(0, 3, 1, 2).double()                    # the STORED input
    wq = P.pack_conv_weight(wt, P.MX_DTYPE).to(DEV)
    wpoly = P.pack_polyphase_conv_weight(wt.permute(0, 2, 3, 1).contiguous(), P.MX_DTYPE).to(DEV)
    bd, bpoly = bias.to(DEV), bias.repeat(4).to(DEV)
    two = ops.conv2d(ops.upsample2x(xd), wq, c, 3, 3, (1, 1), (1, 1), bias=bd, act=ops.ACT_LRELU)
    numel = n * 2 * h * 2 * w * c
    buf = torch.empty((numel + 2 * GUARD,), dtype=P.MX_DTYPE, device=DEV)
    buf.view(torch.uint8).fill_(0xA5)
    y = P.tag(buf[GUARD:GUARD + numel].reshape(n, 2 * h, 2 * w, c))
    plan = ops.polyphase_plan(xd, c, ops.ACT_LRELU)
    assert plan >= 0, "the planner refuses the polyphase launch of case %s" % name
    yy, part, ring = ops.upconv3x3_polyphase(xd, wpoly, bpoly, wq, bd, c, ops.ACT_LRELU, out=y)
    torch.cuda.synchronize()
    assert yy.data_ptr() == y.data_ptr()
    ref = F.leaky_relu(F.conv2d(F.interpolate(xs, scale_factor=2, mode="bilinear", align_corners=False), wt.double(), bias.double(), padding=1), 0.2)
    dec = lambda t: ops.convert(t, torch.float32).cpu().permute(0, 3, 1, 2).double()
    r = dict(plan=plan, xd=xd, two=two, y=y, buf=buf, part=part, ring=ring, ref=ref, two_f=dec(two), y_f=dec(y), shape=(n, h, w, cin, c))
    _MEMO[name] = r
    return r


def _ring_mask(h2, w2):
    m = torch.zeros((h2, w2), dtype=torch.bool)
    m[:2] = m[-2:] = True
    m[:, :2] = m[:, -2:] = True
    return m


@pytest.mark.parametrize("name", list(CASES))
def test_polyphase_equals_the_two_launch_form_on_the_ring_and_beats_its_bound_inside(name):
    r = _run(name)
    n, h, w, cin, c = r["shape"]
    ring = _ring_mask(2 * h, 2 * w)
    yb, tb = r["y"].cpu().view(torch.uint8).reshape(n, 2 * h, 2 * w, c * 4), r["two"].cpu().view(torch.uint8).reshape(n, 2 * h, 2 * w, c * 4)
    assert torch.equal(yb[:, ring], tb[:, ring]), "ring pixels must be the two-launch form's bytes"
    inner = ~ring
    e_poly = (r["y_f"] - r["ref"]).abs()[:, :, inner].max().item()
    e_two = (r["two_f"] - r["ref"]).abs()[:, :, inner].max().item()
    print("%-28s interior max|d| vs fp64: polyphase %.3e  two-launch %.3e  (ratio %.2f)" % (name, e_poly, e_two, e_poly / e_two))
    assert e_poly <= 1.5 * e_two
    g = r["buf"].view(torch.uint8)
    assert bool((g[:GUARD * 4] == 0xA5).all()) and bool((g[-GUARD * 4:] == 0xA5).all()), "bytes outside y were written"


def test_the_one_wave_tile_takes_the_big_launch_and_pinned_tiles_give_the_same_bytes():
    from marconet_amd import _lib
    ops = _ops()
    r = _run("one_wave_tile")
    assert r["plan"] == _lib.ALGO_DMA_CFG16, "cout' 256 on 65536 pixels: the one-wave-per-SIMD tile (id 16) when not steered away"
    n, h, w, cin, c = r["shape"]
    assert ops.polyphase_plan(r["xd"], c, ops.ACT_LRELU, algo=_lib.ALGO_DMA_CFG0 + 15) == _lib.ALGO_DMA_CFG0 + 15
    # the same launch on the 8-wave software-pipelined tile (conv_final.3's routing) and on the small-launch tile: the same bytes, the same sums
    P = _P()
    wt = _rnd((c, cin, 3, 3), 12, 1.0 / math.sqrt(cin * 9))
    wpoly = P.pack_polyphase_conv_weight(wt.permute(0, 2, 3, 1).contiguous(), P.MX_DTYPE).to(DEV)
    bpoly = _rnd((c,), 13, 0.3).repeat(4).to(DEV)
    outs = []
    for algo in (_lib.ALGO_DMA_CFG16, _lib.ALGO_DMA_CFG0 + 15, _lib.ALGO_DMA_CFG0 + 10):
        part = ops.gn_partial_buffer(n, h, w, 4 * c, DEV)
        y = ops.conv2d(r["xd"], wpoly, 4 * c, 3, 3, (1, 1), (1, 1), bias=bpoly, act=ops.ACT_LRELU, gn_partial=part, algo=algo, shuffle2=True)
        outs.append((y.cpu().view(torch.uint8), part.cpu()))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
    y_nogn = ops.conv2d(r["xd"], wpoly, 4 * c, 3, 3, (1, 1), (1, 1), bias=bpoly, act=ops.ACT_LRELU, algo=_lib.ALGO_DMA_CFG0 + 15, shuffle2=True)
    assert torch.equal(y_nogn.cpu().view(torch.uint8), outs[0][0])


@pytest.mark.parametrize("name", list(CASES))
def test_groupnorm_affine_from_masked_partials_and_ring_sums(name):
    ops = _ops()
    r = _run(name)
    n, h, w, cin, c = r["shape"]
    gamma, beta = _rnd((c,), 14).abs() + 0.5, _rnd((c,), 15, 0.2)
    sc, sh = ops.groupnorm_affine_from_partial_ring(r["part"], r["ring"], n, 2 * h, 2 * w, c, gamma.to(DEV), beta.to(DEV), 1e-6)
    torch.cuda.synchronize()
    yf = r["y_f"]                                                        # fp64 statistics of the STORED output
    ref = F.group_norm(yf, c // 32, gamma.double(), beta.double(), 1e-6)
    got = yf * sc.cpu().double()[:, :, None, None] + sh.cpu().double()[:, :, None, None]
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    print("%-28s GroupNorm affine max|d| %.3e of %.3e" % (name, err, scale))
    assert err <= 6e-5 * scale


def test_a_launch_the_planner_refuses_enqueues_nothing_and_the_layer_falls_back():
    from marconet_amd import _lib
    from marconet_amd._lib import MarconetHipError
    ops, P = _ops(), _P()
    r = _run("small_tiles")
    n, h, w, cin, c = r["shape"]
    wt = _rnd((c, cin, 3, 3), 12, 1.0 / math.sqrt(cin * 9))
    wpoly = P.pack_polyphase_conv_weight(wt.permute(0, 2, 3, 1).contiguous(), P.MX_DTYPE).to(DEV)
    # a tile without a build of the mode, the strip kernel, the register-staged kernel: refused by the planner ...
    for algo in (_lib.ALGO_DMA_CFG0 + 6, _lib.ALGO_STRIP_CFG0 + 1, _lib.ALGO_REG_STAGED):
        assert ops.polyphase_plan(r["xd"], c, ops.ACT_LRELU, algo=algo) < 0
    # ... as are a width that is no multiple of 32, a residual and valid_w
    xodd = ops.convert(_rnd((1, 8, 24, cin), 16).to(DEV), P.MX_DTYPE)
    assert ops.polyphase_plan(xodd, c, ops.ACT_LRELU) < 0
    assert ops.conv_plan(r["xd"], 4 * c, 3, 3, (1, 1), (1, 1), residual=True, algo=_lib.ALGO_FLAG_SHUFFLE2) < 0
    # ... and the launch itself writes nothing
    y = P.new_tensor((n, 2 * h, 2 * w, c), P.MX_DTYPE, DEV)
    y.view(torch.uint8).fill_(0x5A)
    with pytest.raises(MarconetHipError):
        ops.conv2d(r["xd"], wpoly, 4 * c, 3, 3, (1, 1), (1, 1), act=ops.ACT_LRELU, algo=_lib.ALGO_DMA_CFG0 + 6, shuffle2=True, out=y)
    torch.cuda.synchronize()
    assert bool((y.view(torch.uint8) == 0x5A).all())
    # other storages never take the form
    assert ops.polyphase_plan(torch.zeros((1, 8, 32, 64), dtype=torch.float16, device=DEV), 64) < 0


# ------------------------------------------------------------------------------------------------------------------ end to end (fp16x2, seeded synthetic weights)
@pytest.fixture(scope="module")
def pipe(ckpts):
    from marconet_amd import networks
    from marconet_amd.pipeline import MarconetPipeline
    enc, gan, sr = networks.TextContextEncoderV2(), networks.TSPGAN(), networks.TSPSRNet()
    enc.load_state_dict(ckpts[0], strict=True)
    gan.load_state_dict(ckpts[1], strict=True)
    sr.load_state_dict(ckpts[2], strict=True)
    return MarconetPipeline(*[m.eval().to(DEV) for m in (enc, gan, sr)], precision="fp16x2")


def test_the_sr_net_takes_the_polyphase_form_in_the_fp16x2_mode_only(pipe):
    from marconet_amd import networks
    sr = pipe.sr
    pk = sr._cache.get(sr, "fp16x2", sr._build)
    # conv_final.3 by default; conv_up.1 only under its A/B knob (its ring strips cost what the saved up-sample pass gains)
    assert "poly" in pk["conv_final.3"] and ("poly" in pk["conv_up.1"]) == networks._POLYPHASE_CONV_UP and not networks._NO_POLYPHASE
    assert "poly" not in sr._cache.get(sr, "fp16", sr._build)["conv_up.1"]


def test_one_strip_alone_equals_the_same_strip_in_a_batch_of_three(pipe):
    from oracle import synth
    counts, widths = [5, 9, 3], [512, 512, 512]
    lq = synth.make_lq(301, 3, widths)
    labels = [synth.make_labels(310 + b, k) for b, k in enumerate(counts)]
    locs = synth.make_locs(counts, widths, max_glyphs=16)
    y3 = pipe.forward_batch(lq.to(DEV), labels, locs)
    for b in range(3):
        y1 = pipe.forward_batch(lq[b:b + 1].to(DEV), labels[b:b + 1], locs[b:b + 1])
        assert torch.equal(y3[b:b + 1], y1), "strip %d" % b


def test_mixed_widths_against_the_oracle_and_the_on_off_difference(pipe, ckpts, monkeypatch):
    from marconet_amd import networks
    from oracle import marconet_oracle as O
    from oracle import synth
    widths, counts = [128, 192, 320], [2, 3, 4]
    lq = synth.make_lq(321, len(widths), widths)
    labels = [synth.make_labels(330 + i, k) for i, k in enumerate(counts)]
    locs = synth.make_locs(counts, widths)
    outs = pipe.forward_mixed_widths(lq.to(DEV), widths, labels, locs)
    worst = 0.0
    with torch.no_grad():
        _, _, w = O.encoder_forward(ckpts[0], lq)
        for b, wd in enumerate(widths):
            _, a, c = O.tspgan_forward(ckpts[1], w[b:b + 1].repeat(counts[b], 1), labels[b])
            c64 = torch.trunc(locs[b:b + 1] * 1024.0)
            ref = O.tspsr_forward(ckpts[2], lq[b:b + 1, :, :, :wd], [a], [c], (c64 + 0.5) / (2.0 * wd))
            worst = max(worst, (outs[b].detach().float().cpu() - ref[0]).abs().max().item())
    monkeypatch.setattr(networks, "_NO_POLYPHASE", True)
    off = pipe.forward_mixed_widths(lq.to(DEV), widths, labels, locs)
    diff = max((a.float() - b.float()).abs().max().item() for a, b in zip(outs, off))
    print("fp16x2 mixed widths %s: max|d| vs oracle %.3e; polyphase on / off max|d| %.3e" % (widths, worst, diff))
    assert worst <= 1e-3
