"""-m gpu: the geometry contract of mnet_conv2d_nhwc on every kernel build — the header's one formula for any kh, kw, stride and padding
(include/marconet_hip.h) against an fp64 reference built from the definition with explicit zero padding (tests/conv_geometry.py):

    y[n,oh,ow,o] = post_scale * act( out_scale * sum_{r,s,i} W[o,r,s,i] * X'[n, oh*sh - ph + r, ow*sw - pw + s, i] + bias + residual )
    out-of-image taps (and INPUT columns >= valid_w[n]) are zero

Every (storage type, requested kernel) runs every row of the geometry table (1x1 ... 8x4 filters, strides (1,2), 2 and 3, paddings from none to far beyond
the filter, one-row and one-column maps, two >= 65536-pixel maps) in the launch variants of a seeded all-pairs cover, and checks per launch:
  * the planner's answer for the full descriptor at its real addresses equals what the header's rules give (conv_geometry.expected, pinned on the CPU
    tier): a refused launch raises MarconetHipError and leaves `out` byte for byte as it was, an accepted one runs — no row is skipped;
  * (a) the value against the fp64 reference on the STORED operands, within the per-type bounds of the epilogue contract (unchanged), relative to the
    output scale; outputs whose window holds no live tap equal the epilogue of an exact zero (a bare launch stores zero);
  * (b) the same bytes as a launch pinned at the kernel the planner named;
  * (c) the same bytes as the storage type's anchor kernel for the ids the header promises identical bits for;
  * (d) the GroupNorm sums against fp64, and the same sum bytes across kernels.
x0, x1 and y are 128-byte aligned slices of larger buffers whose other bytes are 0xFF (NaN in every storage type): a padding tap that reads its linear
neighbour shows as NaN, a tap that reads the previous image's last row as a wrong value, and the bytes around y must be intact afterwards.
mnet_conv2d_splitk gets three patchify geometries with unused last rows / columns.  Margins (error / bound per launch, plan ids) go to
conv_geometry_contract.json in the report_dir fixture's directory."""
import ctypes
import json
import os

import pytest
import torch

from tests import conv_contract as C
from tests import conv_geometry as G
from tests.test_conv_epilogue_contract_gpu import _ANCHOR, _bytes, _decode, _gn_margin, _tolerances
from tests.test_kernels_gpu import _nhwc, _pack_w, _rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPORT = {}
_CACHE = {}          # device operands per (storage, row, channels), anchors' bytes


@pytest.fixture(scope="module", autouse=True)
def _dump_report(report_dir):
    yield
    with open(os.path.join(report_dir, "conv_geometry_contract.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


def _ops():
    from marconet_amd import ops
    return ops


def _guarded(t, guard_bytes):
    """(whole buffer, a copy of t inside it as a view of t's dtype and shape, its byte offset): a 128-byte aligned slice with at least
    guard_bytes of 0xFF on either side"""
    from marconet_amd import packing
    raw = packing.untag(t).contiguous().view(torch.uint8).reshape(-1)
    g = (guard_bytes + 127) // 128 * 128
    buf = torch.full((g + raw.numel() + g + 128,), 0xFF, dtype=torch.uint8, device=DEV)
    off = (-buf.data_ptr()) % 128 + g
    core = buf[off:off + raw.numel()]
    core.copy_(raw)
    return buf, packing.tag(core.view(t.dtype).reshape(t.shape)), off


class Device:
    """the stored operands of one (storage, row, channels) on the device; x0 / x1 between 0xFF guards of at least ph*w + pw + kw pixels"""

    def __init__(self, storage, rname, chans):
        self.op = op = G.operands(storage, rname, chans)
        self.storage, self.rname, self.chans = storage, rname, chans
        n, h, w, kh, kw, (sh, sw), (ph, pw) = op.geo[:7]
        c0, c1, cout = chans
        dt = op.dt
        self.ho, self.wo, self.rows = op.ho, op.wo, op.rows
        self.shape = (n, h, w, c0, c1, cout)                                   # (what _gn_margin reads: n and cout)
        self.vw = torch.tensor(op.vws, dtype=torch.int32)
        gpix = ph * w + pw + kw + 16
        x0, x1 = _nhwc(op.x_raw[:, :c0].contiguous(), dt), _nhwc(op.x_raw[:, c0:].contiguous(), dt)
        self.x0buf, self.x0d, _ = _guarded(x0, gpix * c0 * x0.element_size())
        self.x1buf, self.x1d, _ = _guarded(x1, gpix * c1 * x1.element_size())
        self.wpd = {"none": _pack_w(op.wt[:, :c0].contiguous(), dt), "two": _pack_w(op.wt, dt)}
        self.out_scale, self.bias = op.out_scale.to(DEV), op.bias.to(DEV)
        self.resd = None
        self.valid_w = self.vw.to(DEV)
        self.xf = {cu: (op.in_scale[:, :cu].contiguous().to(DEV), op.in_shift[:, :cu].contiguous().to(DEV)) for cu in (c0, c0 + c1)}

    def residual(self):
        if self.resd is None:
            self.resd = _nhwc(self.op.res_raw, self.op.dt)
        return self.resd


def _device(storage, rname, chans):
    key = ("dev", storage, rname, chans)
    if key not in _CACHE:
        if G.flag(rname, "big"):                       # one big map at a time
            for k in [k for k in _CACHE if G.flag(k[2], "big")]:
                del _CACHE[k]
        _CACHE[key] = Device(storage, rname, chans)
    return _CACHE[key]


def _prepare(dev, row, algo):
    """the buffers of one launch (y a 0xFF-filled slice between 0xFF guards, the GroupNorm buffer NaN) and mnet_conv2d_plan's answer for the FULL
    descriptor, every buffer at its real address"""
    from marconet_amd import _lib
    ops = _ops()
    n, h, w, kh, kw, stride, pad = dev.op.geo[:7]
    c0, c1, cout = dev.chans
    two = row["src2"] != "none"
    kw_ = dict(x1=dev.x1d if two else None, x1_center=row["src2"] == "center", act=row["act"], out_scale=dev.out_scale if row["out_scale"] != "none" else None,
               bias=dev.bias if row["bias"] != "none" else None, residual=dev.residual() if row["residual"] != "none" else None,
               valid_w=dev.valid_w if row["valid_w"] != "none" else None)
    if row["xform"] != "none":
        sc, shf = dev.xf[c0 + (c1 if two else 0)]
        kw_.update(in_scale=sc, in_shift=shf, in_swish=row["xform"] == "swish")
    wp = dev.wpd["two" if two else "none"]
    ybuf, out, yoff = _guarded_out((n, dev.ho, dev.wo, cout), dev.x0d.dtype, cout)
    gn = None
    if row["gn"] == "on":
        gn = torch.full(((n * dev.ho * dev.wo) // 32, cout // 32, 2), float("nan"), device=DEV)
    a = lambda t: None if t is None else t.data_ptr()
    d = ops._conv_desc(dev.x0d, kw_["x1"], cout, kh, kw, stride, pad, wgt=wp.data_ptr(), y=out.data_ptr(), in_scale=a(kw_.get("in_scale")),
                       in_shift=a(kw_.get("in_shift")), in_swish=kw_.get("in_swish", False), valid_w=a(kw_["valid_w"]), out_scale=a(kw_["out_scale"]),
                       bias=a(kw_["bias"]), residual=a(kw_["residual"]), res_mod=0, act=kw_["act"], post_scale=None, gn_partial=a(gn))
    plan = int(_lib.load().mnet_conv2d_plan(ctypes.byref(d), algo | (C.FLAG_X1_CENTER if kw_["x1_center"] else 0)))
    launch = lambda a_: ops.conv2d(dev.x0d, wp, cout, kh, kw, stride, pad, out=out, gn_partial=gn, algo=a_, **kw_)
    return plan, ybuf, out, yoff, gn, launch


def _guarded_out(shape, dtype, cout):
    """an output tensor of 0xFF bytes between 0xFF guards of 512 pixels"""
    from marconet_amd import packing
    esz = torch.empty((), dtype=dtype).element_size()
    nbytes = shape[0] * shape[1] * shape[2] * shape[3] * esz
    g = 512 * cout * esz
    buf = torch.full((g + nbytes + g + 128,), 0xFF, dtype=torch.uint8, device=DEV)
    off = (-buf.data_ptr()) % 128 + g
    return buf, packing.tag(buf[off:off + nbytes].view(dtype).reshape(shape)), off


def _guards_intact(ybuf, out, yoff):
    nbytes = out.numel() * out.element_size()
    return bool((ybuf[:yoff] == 0xFF).all()) and bool((ybuf[yoff + nbytes:] == 0xFF).all())


def _anchor(dev, vname, row):
    """(kernel, output bytes, GroupNorm buffer) of the storage type's anchor kernel on this launch (cached), or None when the planner refuses it"""
    key = ("anchor", dev.storage, dev.rname, dev.chans, tuple(sorted(row.items())))
    if key not in _CACHE:
        algo = _ANCHOR[dev.storage]
        k, ybuf, out, yoff, gn, launch = _prepare(dev, row, algo)
        if k < 0:
            _CACHE[key] = None
        else:
            launch(algo)
            torch.cuda.synchronize()
            _CACHE[key] = (k, _bytes(out).clone(), gn)
    return _CACHE[key]


def _check_launch(dev, req, algo, vname, row, fails, rep):
    from marconet_amd._lib import MarconetHipError
    storage, op = dev.storage, dev.op
    key = "%s/%dx%dx%d/%s" % ((dev.rname,) + dev.chans + (vname,))
    tag = "%s %s %s" % (storage, req, key)
    exp = G.expected(storage, req, dev.rname, dev.chans, row)
    kp, ybuf, out, yoff, gn, launch = _prepare(dev, row, algo)
    msg = G.plan_mismatch(storage, exp, kp, dev.rname)
    if msg:
        fails.append("%s: %s" % (tag, msg))
    if kp < 0:                                            # refused: the launch raises and enqueues nothing
        try:
            launch(algo)
            fails.append("%s: the planner refuses it (%d) but the launch ran" % (tag, kp))
        except MarconetHipError:
            pass
        torch.cuda.synchronize()
        if not bool((ybuf == 0xFF).all()):
            fails.append("%s: a refused launch wrote to out" % tag)
        rep[key] = {"plan": kp}
        return False
    launch(algo)
    torch.cuda.synchronize()
    if not _guards_intact(ybuf, out, yoff):
        fails.append("%s: kernel %d wrote outside y" % (tag, kp))
    got = _decode(dev, out)
    entry = {"plan": kp}
    err_v = 0.0
    for kind, tol in _tolerances(storage, kp, row):       # (a) value against the definition
        ref = op.reference(row, kind)
        scale = max(float(ref.abs().max()), 1e-6)
        err = float((got - ref).abs().max())              # (a NaN — a tap read from a guard — gives err = nan and fails the comparison below)
        entry["margin_" + kind] = err / (tol * scale)
        if not err <= tol * scale:
            fails.append("%s: kernel %d vs %s reference: err %.3e > %.1e x scale %.3e" % (tag, kp, kind, err, tol, scale))
        if kind != "emu":
            err_v = err
    dead = ~G.live_mask(op.geo, op.vws if row["valid_w"] != "none" else None)[:, dev.rows]
    if bool(dead.any()):                                  # windows without a live tap: the epilogue of an EXACT zero
        sel = dead[:, None].expand_as(got)
        zero = op.epilogue(row, torch.zeros_like(got))
        if row["bias"] == "none" and row["residual"] == "none":
            if not bool((got[sel] == 0).all()):
                fails.append("%s: kernel %d stores a non-zero where no tap is live" % (tag, kp))
        else:
            # no accumulation error is left: three fp32 roundings of the epilogue (the add, the two factors of LRELU_SQRT2: 1.8e-7) plus the storage
            # rounding of the output — f16 2^-11 = 4.9e-4, split half 2^-22 = 2.4e-7, fp16+8 2^-11 (the half) x 2^-4 (the e4m3 byte) = 3.1e-5
            tol0 = {"f32": 1e-6, "f16": 5.5e-4, "split": 1e-6, "mx": 4e-5}[storage]
            e0 = float((got[sel] - zero[sel]).abs().max())
            entry["margin_dead"] = e0 / (tol0 * max(float(zero.abs().max()), 1e-6))
            if not e0 <= tol0 * max(float(zero.abs().max()), 1e-6):
                fails.append("%s: kernel %d: outputs without a live tap are off the epilogue of zero by %.3e" % (tag, kp, e0))
    if kp != algo:                                        # (b) the kernel the planner named, pinned, gives the same bytes
        kp2, ybuf2, out2, yoff2, gn2, launch2 = _prepare(dev, row, kp)
        if kp2 != kp:
            fails.append("%s: the planner names kernel %d, pinned there it names %d" % (tag, kp, kp2))
        else:
            launch2(kp)
            torch.cuda.synchronize()
            if not torch.equal(_bytes(out2), _bytes(out)) or (gn is not None and not torch.equal(_bytes(gn2), _bytes(gn))):
                fails.append("%s: the planner names kernel %d but a launch pinned there gives other bytes" % (tag, kp))
    ids = C.BYTE_IDENTICAL.get(storage, ())
    if kp in ids:                                         # (c) the bytes the header promises identical across kernels
        anc = _anchor(dev, vname, row)
        if anc is not None and anc[0] in ids:
            if not torch.equal(anc[1], _bytes(out)):
                fails.append("%s: kernel %d stores other bytes than kernel %d (%d bytes differ)" % (tag, kp, anc[0], int((anc[1] != _bytes(out)).sum())))
            if gn is not None and not torch.equal(_bytes(anc[2]), _bytes(gn)):
                fails.append("%s: kernel %d writes other GroupNorm sums than kernel %d" % (tag, kp, anc[0]))
    if gn is not None:                                    # (d) GroupNorm sums
        if not bool(torch.isfinite(gn).all()):
            fails.append("%s: GroupNorm fragments left unwritten" % tag)
        else:
            m = _gn_margin(dev, row, op.reference(row, _tolerances(storage, kp, row)[-1][0]), err_v, gn)
            entry["margin_gn"] = m
            if not m <= 1.0:
                fails.append("%s: GroupNorm sums off by %.2f x the bound" % (tag, m))
    rep[key] = entry
    return True


_CASES = [(s, r) for s in ("f32", "f16", "split", "mx") for r in sorted(C.requests(s))]


@pytest.mark.parametrize("storage,req", _CASES, ids=["%s-%s" % c for c in _CASES])
def test_geometry_on_every_kernel(storage, req):
    """every row of the geometry table in every variant on the requested kernel; all failures collected, one assertion.  The launches that must RUN are
    the ones the header's rules accept (conv_geometry.expected, checked against the planner without a device in test_conv_geometry_table.py)"""
    algo, family = C.requests(storage)[req]
    fails, rep = [], {}
    todo = G.launches(storage, req)
    want = sum(G.expected(storage, req, rname, ch, row)[0] != "refused" for rname, ch, vname, row in todo)
    ran = 0
    for rname, ch, vname, row in todo:
        ran += _check_launch(_device(storage, rname, ch), req, algo, vname, row, fails, rep)
    REPORT["%s/%s" % (storage, req)] = rep
    if ran != want:
        fails.append("%s %s launch-count: %d launches ran, the header's rules accept %d" % (storage, req, ran, want))
    rows = sorted({f.split()[2].split("/")[0] for f in fails})
    assert not fails, "%d failures on rows %s:\n%s" % (len(fails), ", ".join(rows), "\n".join(fails[:60]))


@pytest.mark.parametrize("name", sorted(G.SPLITK))
def test_splitk_patchify_geometries(name):
    """mnet_conv2d_splitk (fp32) on non-square patchify filters whose map leaves an unused last row / column: against the same explicit-padding fp64
    reference and against the register-staged launch, both within the f32 bound, at two ksplit values the header allows"""
    import torch.nn.functional as F
    ops = _ops()
    h, w, c, kh, kw, cout, ksplits = G.SPLITK[name]
    n = 3
    geo = (n, h, w, kh, kw, (kh, kw), (0, 0))
    ho, wo = G.out_size(geo)
    assert (h - kh) % kh or (w - kw) % kw
    seed = 7100 + 10 * sorted(G.SPLITK).index(name)
    x, wt, bias = _rnd((n, c, h, w), seed), _rnd((cout, c, kh, kw), seed + 1, (c * kh * kw) ** -0.5), _rnd((cout,), seed + 2, 0.3)
    conv = G.explicit_conv(x, geo, None, list(range(ho)), lambda xp, stride: F.conv2d(xp.double(), wt.double(), stride=stride))
    ref = F.leaky_relu(conv + bias.double()[None, :, None, None], 0.2)
    scale = max(float(ref.abs().max()), 1e-6)
    xbuf, x0, _ = _guarded(_nhwc(x, torch.float32), (w + kw + 16) * c * 4)
    wp = _pack_w(wt, torch.float32)
    reg = ops.conv2d(x0, wp, cout, kh, kw, (kh, kw), (0, 0), bias=bias.to(DEV), act=2, algo=C.ALGO_REG).cpu().permute(0, 3, 1, 2).double()
    fails, rep = [], {}
    for ks in ksplits:
        ybuf, out, yoff = _guarded_out((n, ho, wo, cout), torch.float32, cout)
        ops.conv2d(x0, wp, cout, kh, kw, (kh, kw), (0, 0), bias=bias.to(DEV), act=2, splitk=ks, out=out)
        torch.cuda.synchronize()
        got = out.cpu().permute(0, 3, 1, 2).double()
        e_ref, e_reg = float((got - ref).abs().max()), float((got - reg).abs().max())
        rep["ksplit%d" % ks] = {"margin_dec": e_ref / (2e-5 * scale), "margin_reg": e_reg / (2e-5 * scale)}
        if not e_ref <= 2e-5 * scale:
            fails.append("split-K %s ksplit %d vs fp64: err %.3e > 2e-5 x %.3e" % (name, ks, e_ref, scale))
        if not e_reg <= 2e-5 * scale:
            fails.append("split-K %s ksplit %d vs the register-staged kernel: %.3e > 2e-5 x %.3e" % (name, ks, e_reg, scale))
        if not _guards_intact(ybuf, out, yoff):
            fails.append("split-K %s ksplit %d wrote outside y" % (name, ks))
    REPORT["f32/splitk/" + name] = rep
    assert not fails, "\n".join(fails)


def test_splitk_refuses_what_the_header_does_not_allow():
    """a ksplit whose slices are not whole 16-float steps (4x8, cin 8, ksplit 32: 8-float slices) and a launch with padding: MarconetHipError, out untouched"""
    from marconet_amd._lib import MarconetHipError
    ops = _ops()
    name, ks = G.SPLITK_REFUSED_KSPLIT
    h, w, c, kh, kw, cout, ksplits = G.SPLITK[name]
    n = 3
    x0 = _nhwc(_rnd((n, c, h, w), 7200), torch.float32)
    wp = _pack_w(_rnd((cout, c, kh, kw), 7201, 0.1), torch.float32)
    for ksplit, pad in ((ks, (0, 0)), (ksplits[0], (kh, kw))):
        geo = (n, h, w, kh, kw, (kh, kw), pad)
        ho, wo = G.out_size(geo)
        ybuf, out, yoff = _guarded_out((n, ho, wo, cout), torch.float32, cout)
        with pytest.raises(MarconetHipError):
            ops.conv2d(x0, wp, cout, kh, kw, (kh, kw), pad, splitk=ksplit, out=out)
        torch.cuda.synchronize()
        assert bool((ybuf == 0xFF).all()), "a refused split-K launch (ksplit %d, pad %s) wrote to out" % (ksplit, pad)
