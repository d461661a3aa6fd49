"""-m gpu: the epilogue contract of mnet_conv2d_nhwc on every kernel build, against an fp64 evaluation of the header formula (marconet_hip.h):

    y = post_scale[n,o] * act( out_scale[n,o] * conv(W, X') + bias[o] + residual[n, pix % res_mod or pix, o] )
    X' = f(X * in_scale + in_shift) or X;  columns >= valid_w[n] read as zero;  X = concat(x0, x1) or the x1_center fold
    gn_partial = (sum, sum of squares) of that y before storage rounding, over valid columns only

Every (storage type, requested kernel) runs the all-pairs table of its kernel family (tests/conv_contract.py) plus the forced rows and the probes on a
few small shapes that reach the tiles' tails (and the >= 65536-pixel maps for the kernels made for them), and checks per row:
  * the planner's answer for the full descriptor: a refused launch raises MarconetHipError and leaves `out` bit for bit as it was;
  * (a) the value against the fp64 formula on the STORED operands (per-type bounds of the existing files, relative to the output scale);
  * (b) the same bytes as a launch pinned at the kernel the planner named;
  * (c) the same bytes as the other kernels of the storage type the header promises identical bits for (signed zeros included);
  * (d) the GroupNorm sums against fp64 per (32 pixels, group) over valid columns, and the same bytes across kernels.
mnet_conv2d_splitk is checked with the same reference.  Margins (error / bound) go to conv_epilogue_contract.json in the report_dir fixture's directory."""
import ctypes
import itertools
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests import conv_contract as C
from tests.test_kernels_gpu import MX, SPLIT, _nhwc, _pack_w, _q, _rnd
from tests.test_mx_gpu import _emulate, _wdec

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f32": torch.float32, "f16": torch.float16, "split": SPLIT, "mx": MX}
REPORT = {}
_CACHE = {}          # (storage, shape) inputs and fp64 convolutions, and the byte-identity anchors


@pytest.fixture(scope="module", autouse=True)
def _dump_report(report_dir):
    yield
    with open(os.path.join(report_dir, "conv_epilogue_contract.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


def _ops():
    from marconet_amd import ops
    return ops


def _act(v, act):
    return {0: lambda t: t, 1: F.relu, 2: lambda t: F.leaky_relu(t, 0.2), 3: lambda t: F.leaky_relu(t, 0.2) * 2 ** 0.5,
            4: torch.tanh, 5: F.gelu, 6: torch.sigmoid}[act](v)


def _split_q(t):
    """round through the split-half representation (hi = f16(v), lo = f16(v - hi))"""
    hi = t.to(torch.float16)
    return hi.float() + (t - hi.float()).to(torch.float16).float()


def _signed(shape, seed):
    """a per-(image, channel) scale with exact zeros and one all-negative column"""
    s = _rnd(shape, seed) + 0.1
    s.view(-1)[::7] = 0.0
    s[:, 5] = -(s[:, 5].abs() + 0.5)
    return s


class Inputs:
    """everything one (storage, shape) pair launches with: stored operands on the device and their decoded values on the host"""

    def __init__(self, storage, sname):
        shape = C.SHAPES[sname]
        n, h, w, c0, c1, cout, k, stride, pad, vws, big = shape
        dt = DTYPES[storage]
        self.storage, self.sname, self.shape, self.dt = storage, sname, shape, dt
        self.ho, self.wo = C.out_size(shape)
        ho, wo = self.ho, self.wo
        seed = 1000 + 17 * list(C.SHAPES).index(sname)
        self.x = _q(_rnd((n, c0 + c1, h, w), seed), dt)                       # decoded stored activations (x0 | x1)
        self.wt = _rnd((cout, c0 + c1, k, k), seed + 1, 1.0 / math.sqrt((c0 + c1) * k * k))
        if dt == torch.float16:
            self.wt = self.wt.half().float()
        self.x0d, self.x1d = _nhwc(self.x[:, :c0].contiguous(), dt), _nhwc(self.x[:, c0:].contiguous(), dt)
        self.wpd = {"none": _pack_w(self.wt[:, :c0].contiguous(), dt), "two": _pack_w(self.wt, dt)}
        self.terms = {
            "out_scale": {"pos": _rnd((n, cout), seed + 2).abs() + 0.5, "signed": _signed((n, cout), seed + 3)},
            "post_scale": {"pos": _rnd((n, cout), seed + 4).abs() + 0.5, "signed": _signed((n, cout), seed + 5)},
            "bias": {"yes": _rnd((cout,), seed + 6, 0.3)},
        }
        self.res = {"full": _q(_rnd((n, cout, ho, wo), seed + 7), dt),
                    "mod_img": _q(_rnd((1, cout, 1, ho * wo), seed + 8), dt), "mod_div": _q(_rnd((1, cout, 1, wo), seed + 9), dt)}
        # the res_mod residuals sit in front of other values (a buffer of n*ho*wo pixels): a kernel that ignores res_mod reads wrong values, never past the buffer
        pad_px = lambda v: n * ho * wo - v.shape[0] * v.shape[2] * v.shape[3]
        self.resd = {kk: _nhwc(v if pad_px(v) == 0 else torch.cat([v, _q(_rnd((1, cout, 1, pad_px(v)), seed + 12), dt)], dim=3), dt)
                     for kk, v in self.res.items()}
        self.res_rows = {kk: v.permute(0, 2, 3, 1).reshape(-1, cout).double() for kk, v in self.res.items()}   # [pixel or pixel % res_mod, cout]
        self.in_scale = _rnd((n, c0 + c1), seed + 10).abs() + 0.5
        self.in_shift = _rnd((n, c0 + c1), seed + 11, 0.2)
        self.vw = torch.tensor(vws, dtype=torch.int32)
        self.dev = {(grp, lv): t.to(DEV) for grp, lvs in self.terms.items() for lv, t in lvs.items()}
        for cu in (c0, c0 + c1):            # [n][cin] of the launch: cin = c0 with one source, c0 + c1 with two
            self.dev[("in_scale", cu)], self.dev[("in_shift", cu)] = self.in_scale[:, :cu].contiguous().to(DEV), self.in_shift[:, :cu].contiguous().to(DEV)
        self.dev["valid_w"] = self.vw.to(DEV)
        # output rows the fp64 reference covers: all of them, or a band of border rows on the big maps
        self.rows = list(range(ho)) if not big else [0, 1, ho - 2, ho - 1]
        self.convs = {}

    def xprime(self, row):
        """X' of the row: the input transform (rounded to the storage as the kernel stages it) and the valid-width mask"""
        c_used = self.shape[3] + (self.shape[4] if row["src2"] != "none" else 0)
        x = self.x[:, :c_used]
        if row["xform"] != "none":
            x = x * self.in_scale[:, :c_used, None, None] + self.in_shift[:, :c_used, None, None]
            if row["xform"] == "swish":
                x = x * torch.sigmoid(x)
            x = x if self.storage == "f32" else x.half().float() if self.storage == "f16" else _split_q(x)
        if row["valid_w"] != "none":
            x = x.clone()
            for i, v in enumerate(self.vw.tolist()):
                x[i, :, :, v:] = 0
        return x

    def weights(self, row, kind):
        """kind 'dec': the values the kernel multiplies with; 'true': the unrounded weights (the fp16+8 LDS-DMA kernels vs fp64 and _emulate)"""
        c0 = self.shape[3]
        w = self.wt if row["src2"] != "none" else self.wt[:, :c0].contiguous()
        if kind == "dec":
            w = {"split": lambda t: _split_q(t * 256.0) / 256.0, "mx": _wdec}.get(self.storage, lambda t: t)(w)
        if row["src2"] == "center":              # x1 enters at the centre tap only
            k = self.shape[6]
            m = torch.zeros_like(w)
            m[:, :c0] = 1.0
            m[:, c0:, k // 2, k // 2] = 1.0
            w = w * m
        return w

    def conv(self, row, kind):
        """fp64 (kind 'emu': the fp16+8 three-product emulation) convolution of X' over the reference rows: [n, cout, len(rows), wo]"""
        key = (row["src2"], row["xform"], row["valid_w"], kind)
        if key not in self.convs:
            n, h, w, c0, c1, cout, k, stride, pad, vws, big = self.shape
            x = self.xprime(row)
            wt = self.weights(row, "true" if kind == "emu" else kind)
            if kind == "emu":
                f = lambda xx: _emulate(xx, wt, stride=stride, padding=pad).double()
            else:
                f = lambda xx: F.conv2d(xx.double(), wt.double(), stride=stride, padding=pad)
            if not big:
                y = f(x)
            else:                                # 3x3 / stride 1 / pad 1: output rows 0, 1 from input rows 0..2; rows h-2, h-1 from h-3..h-1
                y = torch.cat([f(x[:, :, 0:3])[:, :, 0:2], f(x[:, :, h - 3:h])[:, :, 1:3]], dim=2)
            self.convs[key] = y
        return self.convs[key]

    def reference(self, row, kind):
        """the header formula in fp64 over the reference rows"""
        n = self.shape[0]
        v = self.conv(row, kind)
        if row["out_scale"] != "none":
            v = v * self.terms["out_scale"][row["out_scale"]].double()[:, :, None, None]
        if row["bias"] != "none":
            v = v + self.terms["bias"]["yes"].double()[None, :, None, None]
        if row["residual"] != "none":
            pix = (torch.arange(n)[:, None, None] * self.ho * self.wo + torch.tensor(self.rows)[None, :, None] * self.wo
                   + torch.arange(self.wo)[None, None, :])
            rr = self.res_rows[row["residual"]]
            v = v + rr[pix % rr.shape[0]].permute(0, 3, 1, 2)
        v = _act(v, row["act"])
        if row["post_scale"] != "none":
            v = v * self.terms["post_scale"][row["post_scale"]].double()[:, :, None, None]
        return v


def _inputs(storage, sname):
    key = ("in", storage, sname)
    if key not in _CACHE:
        _CACHE[key] = Inputs(storage, sname)
    return _CACHE[key]


def _launch_args(inp, row):
    two = row["src2"] != "none"
    d = inp.dev
    kw = dict(x1=inp.x1d if two else None, x1_center=row["src2"] == "center", act=row["act"], res_mod=C.res_mod(row, inp.shape),
              out_scale=d.get(("out_scale", row["out_scale"])), post_scale=d.get(("post_scale", row["post_scale"])), bias=d.get(("bias", row["bias"])),
              residual=inp.resd.get(row["residual"]), valid_w=d["valid_w"] if row["valid_w"] != "none" else None)
    if row["xform"] != "none":
        cu = inp.shape[3] + (inp.shape[4] if two else 0)
        kw.update(in_scale=d[("in_scale", cu)], in_shift=d[("in_shift", cu)], in_swish=row["xform"] == "swish")
    return kw, inp.wpd["two" if two else "none"]


def _prepare(inp, row, algo):
    """buffers of one launch of the row (output and GroupNorm buffer pre-filled with NaN) and mnet_conv2d_plan's answer for its FULL descriptor
    (every buffer the launch passes, at its real address)"""
    from marconet_amd import _lib, packing
    ops = _ops()
    n, h, w, c0, c1, cout, k, stride, pad, vws, big = inp.shape
    kw, wp = _launch_args(inp, row)
    out = packing.new_tensor((n, inp.ho, inp.wo, cout), inp.x0d.dtype, DEV)
    out.view(torch.uint8).fill_(0xFF)                   # all-ones bytes: NaN in every storage type
    gn = None
    if row["gn"] == "on":
        gn = torch.full(((n * inp.ho * inp.wo) // 32, cout // 32, 2), float("nan"), device=DEV)
    a = lambda t: None if t is None else t.data_ptr()
    d = ops._conv_desc(inp.x0d, kw["x1"], cout, k, k, stride, (pad, pad), wgt=wp.data_ptr(), y=out.data_ptr(), in_scale=a(kw.get("in_scale")),
                       in_shift=a(kw.get("in_shift")), in_swish=kw.get("in_swish", False), valid_w=a(kw["valid_w"]), out_scale=a(kw["out_scale"]),
                       bias=a(kw["bias"]), residual=a(kw["residual"]), res_mod=kw["res_mod"], act=kw["act"], post_scale=a(kw["post_scale"]), gn_partial=a(gn))
    plan = int(_lib.load().mnet_conv2d_plan(ctypes.byref(d), algo | (C.FLAG_X1_CENTER if kw["x1_center"] else 0)))
    launch = lambda a_: ops.conv2d(inp.x0d, wp, cout, k, k, stride, (pad, pad), out=out, gn_partial=gn, algo=a_, **kw)
    return plan, out, gn, launch


def _bytes(t):
    return t.view(torch.uint8)


def _decode(inp, y):
    """stored output -> fp64 NCHW on the host over the reference rows (device converter for the blocked types: byte-exact with the host decoders)"""
    f = y.float() if y.dtype in (torch.float32, torch.float16) else _ops().convert(y, torch.float32)
    return f[:, inp.rows].permute(0, 3, 1, 2).double().cpu()


def _tolerances(storage, k, row):
    """[(reference kind, bound relative to the output scale)]: the per-type bounds of the existing files"""
    trans = row["act"] >= 4
    xf = row["xform"] != "none"
    if storage == "f32":
        return [("dec", 2e-5 * (4 if xf else 2 if trans else 1))]
    if storage == "f16":
        return [("dec", 2.5e-3 * (4 if xf else 2))]
    if storage == "split":
        return [("dec", 2e-5 if row["xform"] == "swish" else 8e-6 if (trans or xf) else 6e-6)]
    if C.is_dma(k) or C.is_strip(k):                  # fp16+8 LDS-DMA / strip: the three-product emulation, and fp64 of the true weights
        return ([] if row["src2"] == "center" else [("emu", 2e-5)]) + [("true", 4e-5)]
    return [("dec", 3e-5 if xf else 2e-5)]           # fp16+8 register-staged: fp64 of the decoded operands


_ANCHOR = {"f16": C.dma(0), "mx": C.dma(6)}          # the kernel every byte-identical kernel of the storage type is compared with


def _anchor(inp, rname, row):
    """(kernel, output bytes, GroupNorm buffer) of the storage type's anchor on this row (cached), or None when the planner refuses it"""
    key = ("anchor", inp.storage, inp.sname, tuple(sorted(row.items())))
    if key not in _CACHE:
        k, out, gn, launch = _prepare(inp, row, _ANCHOR[inp.storage])
        if k < 0:
            _CACHE[key] = None
        else:
            launch(_ANCHOR[inp.storage])
            torch.cuda.synchronize()
            _CACHE[key] = (k, _bytes(out).clone(), gn)
    return _CACHE[key]


def _gn_margin(inp, row, ref, err_v, part):
    """(d) GroupNorm partial sums against fp64 (sum, sum of squares) of the reference y per (32 pixels, 32 channels), valid columns only.  Bound: the
    output's own error err_v per value, plus 1e-5 of sum |y| / sum y^2 (fp32 summation) — relative to those, not to the sum, which can cancel"""
    n, cout = inp.shape[0], inp.shape[5]
    y = ref.permute(0, 2, 3, 1).clone()                                    # [n, rows, wo, cout]
    if row["valid_w"] != "none":
        for i, v in enumerate(inp.vw.tolist()):
            y[i, :, v:] = 0
    pix = (torch.arange(n)[:, None, None] * inp.ho * inp.wo + torch.tensor(inp.rows)[None, :, None] * inp.wo + torch.arange(inp.wo)[None, None, :])
    frag = (pix // 32).reshape(-1)
    ids = torch.unique(frag)
    pos = torch.searchsorted(ids, frag)
    yb = y.reshape(-1, cout // 32, 32)
    s1 = torch.zeros(len(ids), cout // 32, dtype=torch.float64)
    a1, s2 = torch.zeros_like(s1), torch.zeros_like(s1)
    s1.index_add_(0, pos, yb.sum(-1))
    a1.index_add_(0, pos, yb.abs().sum(-1))
    s2.index_add_(0, pos, (yb * yb).sum(-1))
    got = part.cpu().double()[ids]
    b1 = 1e-5 * a1 + 1024 * err_v + 1e-30
    b2 = 1e-5 * s2 + 2 * err_v * a1 + 1024 * err_v ** 2 + 1e-30
    return max(float(((got[..., 0] - s1).abs() / b1).max()), float(((got[..., 1] - s2).abs() / b2).max()))


def _check_row(inp, req, algo, rname, row, fails, rep):
    from marconet_amd._lib import MarconetHipError
    storage = inp.storage
    tag = "%s %s %s %s" % (storage, req, inp.sname, rname)
    key = rname + "@" + inp.sname
    kp, out, gn, launch = _prepare(inp, row, algo)
    if kp < 0:                                            # refused: the launch raises and enqueues nothing
        before = _bytes(out).clone()
        try:
            launch(algo)
            fails.append("%s: the planner refuses it (%d) but the launch ran" % (tag, kp))
        except MarconetHipError:
            pass
        torch.cuda.synchronize()
        if not torch.equal(_bytes(out), before):
            fails.append("%s: a refused launch wrote to out" % tag)
        rep[key] = {"plan": kp}
        return
    launch(algo)
    torch.cuda.synchronize()
    got = _decode(inp, out)
    entry = {"plan": kp}
    err_v = 0.0
    for kind, tol in _tolerances(storage, kp, row):       # (a) value against the header formula
        ref = inp.reference(row, kind)
        scale = max(float(ref.abs().max()), 1e-6)
        err = float((got - ref).abs().max())
        entry["margin_" + kind] = err / (tol * scale)
        if not err <= tol * scale:
            fails.append("%s: kernel %d vs %s reference: err %.3e > %.1e x scale %.3e" % (tag, kp, kind, err, tol, scale))
        if kind != "emu":
            err_v = err
    if kp != algo:                                        # (b) the kernel the planner named, pinned, gives the same bytes
        kp2, out2, gn2, launch2 = _prepare(inp, row, kp)
        launch2(kp)
        torch.cuda.synchronize()
        if kp2 != kp or not torch.equal(_bytes(out2), _bytes(out)) or (gn is not None and not torch.equal(_bytes(gn2), _bytes(gn))):
            fails.append("%s: the planner names kernel %d (pinned: %d) but a launch pinned there gives other bytes" % (tag, kp, kp2))
    ids = C.BYTE_IDENTICAL.get(storage, ())
    if kp in ids:                                         # (c) the bytes the header promises identical across kernels, -0 vs +0 included
        anc = _anchor(inp, rname, row)
        if anc is not None and anc[0] in ids:
            if not torch.equal(anc[1], _bytes(out)):
                nd = int((anc[1] != _bytes(out)).sum())
                fails.append("%s: kernel %d stores other bytes than kernel %d (%d bytes differ)" % (tag, kp, anc[0], nd))
            if gn is not None and not torch.equal(_bytes(anc[2]), _bytes(gn)):
                fails.append("%s: kernel %d writes other GroupNorm sums than kernel %d" % (tag, kp, anc[0]))
    if gn is not None:                                    # (d) GroupNorm sums
        if not bool(torch.isfinite(gn).all()):
            fails.append("%s: GroupNorm fragments left unwritten" % tag)
        else:
            m = _gn_margin(inp, row, inp.reference(row, _tolerances(storage, kp, row)[-1][0]), err_v, gn)
            entry["margin_gn"] = m
            if not m <= 1.0:
                fails.append("%s: GroupNorm sums off by %.2f x the bound" % (tag, m))
    rep[key] = entry


_CASES = [(s, r) for s in ("f32", "f16", "split", "mx") for r in sorted(C.requests(s))]


@pytest.mark.parametrize("storage,req", _CASES, ids=["%s-%s" % c for c in _CASES])
def test_epilogue_terms_on_every_kernel(storage, req):
    """every row of the kernel family's table on every shape the request is made for; all failures collected, one assertion"""
    algo, family = C.requests(storage)[req]
    fails, rep = [], {}
    for sname in C.SHAPES:
        if not C.uses_shape(req, sname) or (storage == "f32" and C.SHAPES[sname][-1]):
            continue
        inp = _inputs(storage, sname)
        for rname, row in C.table(family):
            _check_row(inp, req, algo, rname, row, fails, rep)
    REPORT["%s/%s" % (storage, req)] = rep
    assert not fails, "%d failures:\n%s" % (len(fails), "\n".join(fails[:60]))


def test_splitk_epilogue_terms():
    """mnet_conv2d_splitk (patchify, fp32): every combination of bias / residual / res_mod / act against the same fp64 formula"""
    ops = _ops()
    n, h, w, c, k, cout, ksplit = 3, 8, 64, 32, 8, 36, 8
    ho, wo = h // k, w // k
    x = _rnd((n, c, h, w), 301)
    wt = _rnd((cout, c, k, k), 302, 1.0 / math.sqrt(c * k * k))
    bias = _rnd((cout,), 303, 0.3)
    res = {"full": _rnd((n, cout, ho, wo), 304), "mod_img": _rnd((1, cout, 1, ho * wo), 305), "mod_div": _rnd((1, cout, 1, wo), 306)}
    resm = {"none": 0, "full": 0, "mod_img": ho * wo, "mod_div": wo}
    conv = F.conv2d(x.double(), wt.double(), stride=k)
    x0, wp = _nhwc(x, torch.float32), _pack_w(wt, torch.float32)
    fails, rep = [], {}
    for b, r, act in itertools.product(("none", "yes"), ("none", "full", "mod_img", "mod_div"), range(7)):
        v = conv + (bias.double()[None, :, None, None] if b == "yes" else 0.0)
        if r != "none":
            rr = res[r].permute(0, 2, 3, 1).reshape(-1, cout).double()
            v = v + rr[torch.arange(n * ho * wo) % rr.shape[0]].reshape(n, ho, wo, cout).permute(0, 3, 1, 2)
        ref = _act(v, act)
        y = ops.conv2d(x0, wp, cout, k, k, (k, k), (0, 0), splitk=ksplit, bias=bias.to(DEV) if b == "yes" else None,
                       residual=None if r == "none" else _nhwc(res[r], torch.float32), res_mod=resm[r], act=act)
        torch.cuda.synchronize()
        got = y.cpu().permute(0, 3, 1, 2).double()
        scale = max(float(ref.abs().max()), 1e-6)
        err = float((got - ref).abs().max())
        tol = 2e-5 * (2 if act >= 4 else 1)
        rep["%s/%s/%d" % (b, r, act)] = err / (tol * scale)
        if not err <= tol * scale:
            fails.append("split-K bias=%s residual=%s act=%d: err %.3e > %.1e x %.3e" % (b, r, act, err, tol, scale))
    REPORT["f32/splitk"] = rep
    assert not fails, "\n".join(fails)
