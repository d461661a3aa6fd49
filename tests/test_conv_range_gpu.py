"""-m gpu: the operand-range contract of mnet_conv2d_nhwc (include/marconet_hip.h, "operand range") on every kernel build — the conv kernels as READERS of
the storages' edge blocks.  The scene of tests/conv_range.py (fp16-subnormal blocks at the floor E = 105, E = 0 blocks, blocks 2^6 apart inside a pixel and
between neighbours, weight rows 2^10 apart, a coherent image whose rounding residuals share a sign) is put on the device from HOST-encoded bytes, every
launch runs a bare epilogue (no bias, ACT_NONE), and every output is judged alone against the fp64 reference of the kernel family that ran:

    |got - ref|(o) <= gamma * A_o + f_o + r_o,    exactly 0 where no product of the window is non-zero          (tests/conv_range.py)

Per launch: the planner's answer is the pinned request or its documented hand-over, the bound holds on every output of the reference rows, exact zeros are
exact, and the kernels the header promises identical bytes for give the bytes of the set's anchor.  The worst error / bound per (storage, request, shape,
class) goes to conv_range_contract.json in the report directory."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import conv_contract as C
from tests import conv_range as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPORT = {}
_DEVICE = {}          # (storage, shape, two sources) -> operands on the device; one big map at a time
_ANCHORS = {}
_ANCHOR = {"f16": C.dma(0), "mx": C.dma(6)}
FLAG_SHUFFLE2, FLAG_F32_OUT = 1024, 2048
BIG_REQUESTS = ("auto", "dma5", "dma6", "dma8", "dma9", "dma11", "dma13", "dma15", "dma16")


@pytest.fixture(scope="module", autouse=True)
def _dump_report(report_dir):
    yield
    with open(os.path.join(report_dir, "conv_range_contract.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


def _pk():
    from marconet_amd import packing
    return packing


def _dtype(storage):
    pk = _pk()
    return {"mx": pk.MX_DTYPE, "split": pk.SPLIT_DTYPE, "f16": torch.float16, "f32": torch.float32}[storage]


def _upload(raw, shape, storage):
    """host-encoded bytes -> a device tensor of logical ``shape`` (no device writer between the scene and the kernel under test)"""
    t = torch.from_numpy(np.ascontiguousarray(raw).reshape(-1)).to(DEV).view(_dtype(storage)).reshape(shape)
    assert t.data_ptr() % 128 == 0
    return _pk().tag(t)


def _operands(c):
    key = (c.storage, c.sname, c.raw1 is not None)
    if key not in _DEVICE:
        if R.SHAPES[c.sname][-1]:                      # a big map comes in: drop the others
            for k in [k for k in _DEVICE if R.SHAPES[k[1]][-1]]:
                del _DEVICE[k]
            for k in [k for k in _ANCHORS if R.SHAPES[k[1]][-1] and k[:2] != key[:2]]:
                del _ANCHORS[k]
            torch.cuda.empty_cache()
        n, h, w, c0, c1 = R.SHAPES[c.sname][:5]
        _DEVICE[key] = (_upload(c.raw0, (n, h, w, c0), c.storage), None if c.raw1 is None else _upload(c.raw1, (n, h, w, c1), c.storage),
                        c.wpacked.to(DEV))
    return _DEVICE[key]


def _launch(c, algo, shuffle2=False, out_f32=False, in_scale=None):
    """(the planner's answer for the full descriptor, the output or None when it refuses — then the launch must raise and write nothing)"""
    from marconet_amd import _lib, ops
    from marconet_amd._lib import MarconetHipError
    x0d, x1d, wpd = _operands(c)
    n, h, w = x0d.shape[:3]
    k, pad, cout = c.k, c.pad, c.cout
    ho, wo = h + 2 * pad - k + 1, w + 2 * pad - k + 1
    oshape = (n, 2 * ho, 2 * wo, cout // 4) if shuffle2 else (n, ho, wo, cout)
    out = _pk().new_tensor(oshape, torch.float32 if out_f32 else _dtype(c.storage), DEV)
    out.view(torch.uint8).fill_(0xFF)                   # NaN in every storage type
    center = c.src2 == "center"
    d = ops._conv_desc(x0d, x1d, cout, k, k, (1, 1), (pad, pad), wgt=wpd.data_ptr(), y=out.data_ptr(), in_scale=None if in_scale is None else in_scale.data_ptr())
    flags = (C.FLAG_X1_CENTER if center else 0) | (FLAG_SHUFFLE2 if shuffle2 else 0) | (FLAG_F32_OUT if out_f32 else 0)
    plan = int(_lib.load().mnet_conv2d_plan(ctypes.byref(d), algo | flags))
    run = lambda: ops.conv2d(x0d, wpd, cout, k, k, (1, 1), (pad, pad), x1=x1d, x1_center=center, out=out, algo=algo, shuffle2=shuffle2, out_f32=out_f32, in_scale=in_scale)
    if plan < 0:
        with pytest.raises(MarconetHipError):
            run()
        torch.cuda.synchronize()
        assert bool((out.view(torch.uint8) == 0xFF).all()), "a refused launch wrote to out"
        return plan, None
    run()
    torch.cuda.synchronize()
    return plan, out


def _values(c, out, shuffle2=False, out_f32=False):
    """the stored output over the reference rows, exact, [P, cout] fp64 (parsed from its bytes on the host: no device reader in between)"""
    raw = _pk().untag(out).contiguous().view(torch.uint8)
    if shuffle2:                                        # [n, 2h, 2w, 32]: block (2 py + px) of low-res pixel (i, j) sits at hi-res pixel (2 i + py, 2 j + px)
        n, h2, w2, nb = raw.shape
        assert nb == 128
        raw = raw.reshape(n, h2 // 2, 2, w2 // 2, 2, nb).permute(0, 1, 3, 2, 4, 5).reshape(n, h2 // 2, w2 // 2, 4 * nb)
    raw = raw[:, c.rows].contiguous().cpu().numpy()
    return R.stored_value(raw.reshape(-1, raw.shape[-1]), "f32" if out_f32 else c.storage)


def _judge(c, got, tag, fails, out_f32=False):
    """every output against its own bound; -> {class: worst error / bound}"""
    ref, A, b = c.ref(), c.A(), c.bound(out_f32)
    if not np.isfinite(got).all():
        fails.append("%s: %d outputs unwritten or non-finite" % (tag, int((~np.isfinite(got)).sum())))
        got = np.where(np.isfinite(got), got, 0.0)
    zero = A == 0
    if (got[zero] != 0).any():
        fails.append("%s: %d outputs whose window holds no non-zero product are not 0 (largest %.3e)" % (tag, int((got[zero] != 0).sum()), float(np.abs(got[zero]).max())))
    err = np.abs(got - ref)
    ratio = np.where(zero, 0.0, err / np.maximum(b, 1e-300))
    bands, rows, imgs = c.out_bands(), c.row_classes(), c.out_images()
    margin = {}
    for bi in range(-1, len(R.BANDS)):
        for img in (0, 1):
            m = (bands == bi) & (imgs == img)
            if m.any():
                margin["%s/img%d" % ("edge" if bi < 0 else R.BANDS[bi], img)] = float(ratio[m].max())
    for wi, name in enumerate(R.WCLASSES):
        margin["w:" + name] = float(ratio[:, rows == wi].max())
    if (err > b).any():
        p, o = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        fails.append("%s: %d of %d outputs beyond their bound; worst %.2f x at output %d channel %d (band %s, image %d, row class %s): got %.9e ref %.9e bound %.3e A %.3e"
                     % (tag, int((err > b).sum()), err.size, float(ratio[p, o]), p, o, "edge" if bands[p] < 0 else R.BANDS[bands[p]], int(imgs[p]),
                        R.WCLASSES[rows[o]], got[p, o], ref[p, o], b[p, o], A[p, o]))
    return margin


def _family(storage, k):
    if storage != "mx":
        return storage
    return "mx_dma" if C.is_dma(k) or C.is_strip(k) else "mx_reg"


def _allowed(storage, algo):
    """what a pinned request may resolve to: itself, or the hand-over the header documents (mnet_conv2d_plan)"""
    ok = {algo}
    if storage == "mx" and algo == C.dma(16):
        ok.add(C.dma(15))
    if storage == "mx" and algo == C.dma(9):
        ok.add(C.dma(8))
    return ok


def _row(src2):
    r = {f: C.FACTORS[f][0] for f in C.NAMES}
    r["src2"] = src2
    return r


def _run(storage, req, algo, sname, src2, fails, rep, **kw):
    tag = "%s %s %s %s" % (storage, req, sname, src2)
    probe = R.case(storage, sname, src2)                # (the stored operands do not depend on the family)
    k, out = _launch(probe, algo, **{a: b for a, b in kw.items() if a in ("shuffle2", "out_f32")})
    entry = {"plan": k}
    rep["%s/%s" % (sname, src2)] = entry
    shape = R.SHAPES[sname][:5] + (probe.cout,) + R.SHAPES[sname][6:]
    bad = C.header_violations(storage, shape, _row(src2), algo, k)
    if k >= 0 and req not in ("auto",) and k not in _allowed(storage, algo) and not (req == "reg" and k == C.ALGO_SKINNY):
        bad.append("pinned request %d resolved to kernel %d" % (algo, k))
    fails += ["%s: %s" % (tag, b) for b in bad]
    if out is None:
        return False
    c = R.case(storage, sname, src2, family=_family(storage, k))
    entry["family"] = c.fam
    entry["margin"] = _judge(c, _values(c, out, **{a: b for a, b in kw.items() if a in ("shuffle2", "out_f32")}), tag, fails, out_f32=kw.get("out_f32", False))
    ids = C.BYTE_IDENTICAL.get(storage, ())
    if k in ids and not kw:                             # the bytes the header promises identical across kernels
        akey = (storage, sname, src2)
        if akey not in _ANCHORS:
            ka, oa = _launch(probe, _ANCHOR[storage])
            _ANCHORS[akey] = None if oa is None or ka not in ids else (ka, oa.view(torch.uint8).clone())
        if _ANCHORS[akey] is not None and not torch.equal(_ANCHORS[akey][1], out.view(torch.uint8)):
            fails.append("%s: kernel %d stores other bytes than kernel %d (%d bytes differ)" % (tag, k, _ANCHORS[akey][0], int((_ANCHORS[akey][1] != out.view(torch.uint8)).sum())))
    return True


def _launches(storage, req, family):
    """(shape, second source) of a request: the small shapes with one and two sources (the folded skip on the LDS-DMA ids), the big maps for the kernels made for them"""
    out = []
    if req == "skinny":
        return [("a1", "none")]
    if not req.startswith("strip"):
        for sname in ("a", "b"):
            out.append((sname, "none"))
            if "concat" in C.family_levels(family)["src2"]:
                out.append((sname, "concat"))
        if req.startswith("dma"):
            out.append(("b", "center"))
    if storage != "f32" and (req.startswith("strip") or req in BIG_REQUESTS):
        out += [("c64", "none"), ("c256", "none")]
    return out


_CASES = [(s, r) for s in ("f32", "f16", "split", "mx") for r in sorted(C.requests(s))]


@pytest.mark.parametrize("storage,req", _CASES, ids=["%s-%s" % c for c in _CASES])
def test_operand_range_on_every_kernel(storage, req):
    algo, family = C.requests(storage)[req]
    fails, rep, ran = [], {}, 0
    for sname, src2 in _launches(storage, req, family):
        ran += _run(storage, req, algo, sname, src2, fails, rep)
    REPORT["%s/%s" % (storage, req)] = rep
    assert ran, "the planner refused every launch of %s %s: %s" % (storage, req, rep)
    assert not fails, "%d failures:\n%s" % (len(fails), "\n".join(fails[:40]))


@pytest.mark.parametrize("id_", [10, 15, 16])
def test_operand_range_shuffle2_builds(id_):
    """the pixel-shuffle output mode of the fp16+8 builds that carry it, on the polyphase shape (one block per pixel: neighbours 2^6 apart)"""
    fails, rep = [], {}
    assert _run("mx", "dma%d" % id_, C.dma(id_), "d", "none", fails, rep, shuffle2=True), rep
    REPORT["mx/shuffle2/dma%d" % id_] = rep
    assert not fails, "\n".join(fails)


def test_operand_range_fp32_output_of_the_one_wave_tile():
    """MNET_CONV_ALGO_FLAG_F32_OUT on fp16+8 id 16: the value before the storage's rounding — r_o = 0"""
    fails, rep = [], {}
    for sname, src2 in (("a", "none"), ("b", "none"), ("b", "concat")):
        assert _run("mx", "dma16", C.dma(16), sname, src2, fails, rep, out_f32=True), rep
    REPORT["mx/out_f32/dma16"] = rep
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("storage", ["f32", "f16", "split", "mx"])
def test_operand_range_in_scale_moves_the_unit_band_into_the_subnormal_band(storage):
    """register-staged, in_scale = 2^-19 on every channel: X' = X * 2^-19 staged in the storage's form (the reference rounds it through the spec codec)"""
    fails = []
    c = R.case(storage, "b", "concat", family=_family(storage, C.ALGO_REG), in_scale=True)
    n, cin = R.SHAPES["b"][0], c.cin
    sc = torch.full((n, cin), 2.0 ** R.IN_POW, dtype=torch.float32, device=DEV)
    k, out = _launch(c, C.ALGO_REG, in_scale=sc)
    assert k == C.ALGO_REG and out is not None, k
    tag = "%s reg b concat in_scale" % storage
    REPORT["%s/in_scale/reg" % storage] = {"b/concat": {"plan": k, "family": c.fam, "margin": _judge(c, _values(c, out), tag, fails)}}
    assert not fails, "\n".join(fails)
