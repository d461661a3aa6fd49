"""-m gpu: where in memory an element lies.  Every launch of tests/large_tensors.py runs ONCE on tensors of more than 2^31 elements and more than 2^32
bytes (685 images of 3 * 2^20 elements: 8.03 GiB in the 4-byte storages, 4.01 GiB in f16; the many-small-images rows 174 800 images of 12 x 16 x 64),
so that every hand-written address product — (size_t)pix * cout * 4, the per-tile 64-bit bases n_first * img0 of the LDS-DMA kernels, the hi-res indices of
the pixel-shuffle store, the grid-stride counters — is formed beyond each wrap point: byte offset 2^31 (W1), byte offset 2^32 (W2), element offset 2^31 (W3).

One method for every row.  The big tensors are allocated with torch.empty; every image slot is filled with one seeded filler image F (a device broadcast
copy of the stored bytes of one image, encoded once with ops.convert); the probe slots — image 0, the image that holds each wrap point of each tensor with its
two neighbours, the last image — are overwritten with distinct seeded probe images P_k; the kernel is launched once.  Then
  (a) out[slot] of every probe slot is BYTE-IDENTICAL to the same kernel, pinned at the id the planner named for the big launch, run on P_k alone (n = 1; the
      strip kernels, which take >= 65536 pixels only, run on two copies of P_k);
  (b) every other slot is byte-identical to the kernel run on F alone (compared on the device in chunks of images): a store that wrapped into another image,
      or a load that wrapped, shows here;
  (c) for one probe per row the n = 1 result is inside the bound of the existing contract tests against the fp64 reference (a band of rows on the big maps):
      no new tolerance.
(a) and (b) are equalities the project already promises ("the same bits for every launch size"; the GroupNorm fold order does not depend on the batch).

Section 4: the largest maps the LDS-DMA kernels take — n = 2, h * w the largest the header's address-range conditions accept and no multiple of 512 (a tile
straddles the two images), x and y about 2 GiB each.

Left out: the ViT and style row kernels (their operands stay far below 2^28 elements at any batch the pipeline forms); the four uint8 image kernels (their
`too large` guards are already tested); element offsets >= 2^32, which would need 16 GiB per tensor.

Per-test durations and the margins of (c) and of section 4 go to large_tensors.json in the report_dir fixture's directory."""
import ctypes
import gc
import json
import math
import os
import time
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import large_tensors as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPORT = {"durations": {}, "margins": {}, "plans": {}}


@pytest.fixture(scope="module", autouse=True)
def _dump_report(report_dir):
    yield
    with open(os.path.join(report_dir, "large_tensors.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


@pytest.fixture(autouse=True)
def _timed_and_freed(request):
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    REPORT["durations"][request.node.name] = round(time.time() - t0, 3)
    gc.collect()
    torch.cuda.empty_cache()


def _ops():
    from marconet_amd import ops
    return ops


def _P():
    from marconet_amd import packing
    return packing


def _tdt(storage):
    P = _P()
    return {"f32": torch.float32, "f16": torch.float16, "split": P.SPLIT_DTYPE, "mx": P.MX_DTYPE}[storage]


def _key(storage):
    """the dtype key of tests/test_kernels_gpu.py's helpers (_tol, _check, _pack_w)"""
    return {"f32": torch.float32, "f16": torch.float16, "split": "split", "mx": "mx"}[storage]


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def _need(name, nbytes):
    free = torch.cuda.mem_get_info()[0]
    if free < 1.25 * nbytes:
        pytest.skip("%s needs %d bytes (x 1.25 = %d), the device has %d free" % (name, nbytes, int(1.25 * nbytes), free))


def _iv(t):
    """[n, ...] tensor of any storage -> its bytes as an integer view [n, words per image]"""
    r = _P().untag(t)
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[r.element_size()]
    return r.view(it).reshape(r.shape[0], -1)


def _enc(shape, dt, seed, scale=1.0, shift=0.0):
    """a seeded image on the device, in storage dt through ops.convert"""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    v = torch.randn(shape, generator=g, device=DEV) * scale + shift
    return v if dt == torch.float32 else _ops().convert(v, dt)


def _host(t):
    """stored tensor -> fp32 host values (the host decoders)"""
    return _P().to_float(_P().untag(t).cpu())


def _take_rows(t, rows_):
    """t[:, rows_] of an NHWC tensor of any storage (indexed through an integer view: the blocked dtypes have no index kernel)"""
    P = _P()
    r = P.untag(t)
    it = {2: torch.int16, 4: torch.int32}[r.element_size()]
    return P.tag(r.view(it)[:, rows_].contiguous().view(r.dtype))


def _big(n, img, probes):
    """n slots of the filler image `img` [1, ...], the probe slots overwritten"""
    P = _P()
    t = P.new_tensor((n,) + tuple(img.shape[1:]), img.dtype, DEV)
    v = _iv(t)
    v[:] = _iv(img)
    for k, p in probes.items():
        v[k] = _iv(p)[0]
    return t


def _rep(img, m):
    P = _P()
    return img if m == 1 else P.tag(P.untag(img).expand((m,) + tuple(img.shape[1:])).contiguous())


def _differs(big, one):
    """bool [n] on the device: slot i of `big` is not byte-identical to `one` [1, ...]"""
    b, o = _iv(big), _iv(one)
    step = max(1, (1 << 28) // b.shape[1])
    return torch.cat([(b[i:i + step] != o).any(dim=1) for i in range(0, b.shape[0], step)])


def run_batched(name, n, ins, rows, launch, alone_m=1, tweak=None):
    """the method of the module docstring.  ins: {tensor name: (image shape, torch dtype, scale, shift)}; rows: {name: fn(seed) -> [1, ...] per-image parameter};
    launch(tensors, rows, m) -> tuple of outputs [m, ...]; tweak(slot or "F", tensors) may edit an image before it is used.
    Returns (probe slots, probe inputs, probe rows, alone outputs) for the truth check."""
    slots = L.probe_slots(L.rows()[name])
    assert slots[0] == 0 and slots[-1] == n - 1

    def mk(who):
        tensors = {k: _enc((1,) + tuple(s), dt, _seed(name, k, who), sc, sh) for k, (s, dt, sc, sh) in ins.items()}
        if tweak is not None:
            tweak(who, tensors)
        return tensors, {k: fn(_seed(name, k, who)) for k, fn in rows.items()}
    f_in, f_row = mk("F")
    p_in, p_row = {}, {}
    for s in slots:
        p_in[s], p_row[s] = mk(s)
    alone = lambda tin, trow: tuple(o[:1] for o in launch({k: _rep(v, alone_m) for k, v in tin.items()}, {k: _rep(v, alone_m) for k, v in trow.items()}, alone_m))
    f_out = alone(f_in, f_row)
    p_out = {s: alone(p_in[s], p_row[s]) for s in slots}
    big_in = {k: _big(n, f_in[k], {s: p_in[s][k] for s in slots}) for k in ins}
    big_row = {k: _big(n, f_row[k], {s: p_row[s][k] for s in slots}) for k in rows}
    out = launch(big_in, big_row, n)
    torch.cuda.synchronize()
    fails = []
    is_probe = torch.zeros(n, dtype=torch.bool)
    is_probe[slots] = True
    for j, o in enumerate(out):
        assert o.shape[0] == n
        diff = _differs(o, f_out[j]).cpu()
        wrong = (diff & ~is_probe).nonzero().reshape(-1).tolist()
        if wrong:                                                      # (b)
            fails.append("%s output %d: %d filler slots differ from the kernel run on the filler alone, first %s" % (name, j, len(wrong), wrong[:8]))
        same = [s for s in slots if not bool(diff[s])]
        if same:                                                       # (the probes must be told apart from the filler, or (a) proves nothing)
            fails.append("%s output %d: probe slots %s hold the filler's result" % (name, j, same))
        for s in slots:                                                # (a)
            if not torch.equal(_iv(o)[s], _iv(p_out[s][j])[0]):
                nb = int((_iv(o)[s] != _iv(p_out[s][j])[0]).sum())
                fails.append("%s output %d: slot %d differs from the kernel run on its image alone (%d words)" % (name, j, s, nb))
    assert not fails, "\n".join(fails[:40])
    return slots, p_in, p_row, p_out


# ====================================================================================================================== conv rows
def _conv_plan(dtype_id, n, h, w, c0, c1, cout, algo, residual, bias, gn, k=3):
    from marconet_amd import _lib
    d = _lib.ConvDesc()
    d.dtype = dtype_id
    d.x0 = d.wgt = d.y = 1 << 20
    d.n, d.h, d.w, d.ho, d.wo = n, h, w, h, w
    d.c0, d.cout, d.kh, d.kw = c0, cout, k, k
    if c1:
        d.x1, d.c1 = 1 << 20, c1
    d.stride_h = d.stride_w = 1
    d.pad_h = d.pad_w = k // 2
    d.residual = (1 << 20) if residual else None
    d.bias = (1 << 20) if bias else None
    d.gn_partial = (1 << 20) if gn else None
    d.act = 3 if bias else 0
    return int(_lib.load().mnet_conv2d_plan(ctypes.byref(d), algo))


def _req_algo(req):
    from tests import conv_contract as C
    if req == "reg":
        return C.ALGO_REG
    if req == "auto":
        return C.ALGO_AUTO
    return C.strip(int(req[5:])) if req.startswith("strip") else C.dma(int(req[3:]))


def _band(h, small):
    return list(range(h)) if small else [0, 1, h // 2 - 1, h // 2, h - 2, h - 1]


def _conv_truth(name, storage, k, wt, bias, x_nchw, res_nchw, got_nchw, rows_, extra, c0):
    """(c): the n = 1 result against fp64 over the output rows `rows_` (all columns), bounds of tests/test_conv_epilogue_contract_gpu.py::_tolerances"""
    from tests import conv_geometry as G
    from tests.test_conv_epilogue_contract_gpu import _tolerances
    row = {"act": 3 if bias is not None else 0, "xform": "none", "src2": {"two": "concat", "center": "center"}.get(extra, "none")}
    xp = F.pad(x_nchw, (1, 1, 1, 1))
    out = {}
    for kind, tol in _tolerances(storage, k, row):
        w = wt if kind in ("true", "emu") else {"split": lambda t: G.H.split_q(t * 256.0) / 256.0, "mx": G.H.wdec}.get(storage, lambda t: t)(wt)
        if extra == "center":
            m = torch.zeros_like(w)
            m[:, :c0] = 1.0
            m[:, c0:, 1, 1] = 1.0
            w = w * m
        if kind == "emu":
            conv = lambda xs: G.H.emulate(xs, w, stride=1, padding=0).double()
        else:
            conv = lambda xs: F.conv2d(xs.double(), w.double())
        v = torch.cat([conv(xp[:, :, r:r + 3]) for r in rows_], dim=2)
        if bias is not None:
            v = v + bias.double()[None, :, None, None]
        if res_nchw is not None:
            v = v + res_nchw[:, :, rows_].double()
        ref = G.H.act(v, row["act"])
        if extra == "shuffle2":                                         # channel (2 py + px) C + c of low-res (i, j) is channel c of hi-res (2 i + py, 2 j + px)
            c = ref.shape[1] // 4
            r5 = ref.reshape(1, 2, 2, c, len(rows_), ref.shape[3])       # [1, py, px, c, i, j]
            ref = r5.permute(0, 3, 4, 1, 5, 2).reshape(1, c, 2 * len(rows_), 2 * ref.shape[3])
        scale = max(float(ref.abs().max()), 1e-6)
        err = float((got_nchw.double() - ref).abs().max())
        out["margin_" + kind] = err / (tol * scale)
        assert err <= tol * scale, "%s: kernel %d vs the %s reference: err %.3e > %.1e x scale %.3e" % (name, k, kind, err, tol, scale)
    return out


@pytest.mark.parametrize("name", sorted(L.CONV))
def test_conv_past_the_wrap_points(name):
    from tests import conv_contract as C
    from tests.test_kernels_gpu import _pack_w, _rnd
    ops = _ops()
    r = L.CONV[name]
    storage, extra = r["storage"], r.get("extra")
    row = "conv/" + name
    _need(row, L.need_bytes(L.rows()[row]))
    n, h, w, c0, c1, cout, yshape = L.conv_geometry(name)
    dt, dtype_id = _tdt(storage), L.STORAGES.index(storage)
    plain = extra in ("shuffle2", "f32out")
    with_bias = extra != "f32out"
    gn = extra == "gn"
    flags = {"shuffle2": 1024, "f32out": 2048, "center": 512}.get(extra, 0)
    k = _conv_plan(dtype_id, n, h, w, c0, c1, cout, _req_algo(r["req"]) | flags, not plain, with_bias, gn)
    assert k >= 0, "the planner refuses the big launch: %d" % k
    if r["req"].startswith(("dma", "strip")):
        assert k == _req_algo(r["req"]), "pinned %s, the planner names %d" % (r["req"], k)     # no hand-over on these rows: the id under test runs
    REPORT["plans"][name] = k
    alone_m = 2 if C.is_strip(k) else 1
    k1 = _conv_plan(dtype_id, alone_m, h, w, c0, c1, cout, k | flags, not plain, with_bias, gn)
    assert k1 == k, "pinned at kernel %d, the launch on one image resolves to %d" % (k, k1)
    seed = _seed(name, "w")
    wt = _rnd((cout, c0 + c1, 3, 3), seed, 1.0 / math.sqrt((c0 + c1) * 9))
    if storage == "f16":
        wt = wt.half().float()
    wp = _pack_w(wt, _key(storage))
    bias = _rnd((cout,), seed + 1, 0.3) if with_bias else None
    bias_d = None if bias is None else bias.to(DEV)
    ins = {"x0": ((h, w, c0), dt, 1.0, 0.0)}
    if c1:
        ins["x1"] = ((h, w, c1), dt, 1.0, 0.0)
    if not plain:
        ins["residual"] = (yshape, dt, 1.0, 0.0)

    def launch(t, rows, m):
        P = _P()
        y = P.new_tensor((m,) + yshape, torch.float32 if extra == "f32out" else dt, DEV)
        _iv(y).fill_(-1)
        g = torch.full(((m * h * w) // 32, cout // 32, 2), float("nan"), device=DEV) if gn else None
        ops.conv2d(t["x0"], wp, cout, 3, 3, (1, 1), (1, 1), x1=t.get("x1"), bias=bias_d, residual=t.get("residual"), act=3 if with_bias else 0, out=y,
                   algo=k, x1_center=extra == "center", gn_partial=g, shuffle2=extra == "shuffle2", out_f32=extra == "f32out")
        return (y, g.view(m, -1)) if gn else (y,)

    slots, p_in, _, p_out = run_batched(row, n, ins, {}, launch, alone_m)
    # (c) one probe: the image that holds the last wrap point of y
    s = slots[-3]
    pin = p_in[s]
    small = extra == "small"
    rows_ = _band(h, small)
    x = torch.cat([_host(pin[kk]) for kk in ("x0", "x1") if kk in pin], dim=3).permute(0, 3, 1, 2).contiguous()
    res = None if plain else _host(pin["residual"]).permute(0, 3, 1, 2).contiguous()
    y1 = p_out[s][0]
    got = (y1 if y1.dtype in (torch.float32, torch.float16) else ops.convert(y1, torch.float32)).float().cpu().permute(0, 3, 1, 2)
    yrows = rows_ if extra != "shuffle2" else [2 * i + d for i in rows_ for d in (0, 1)]
    REPORT["margins"][row] = _conv_truth(row, storage, k, wt, bias, x, res, got[:, :, yrows], rows_, extra, c0)
    if gn:
        assert bool(torch.isfinite(p_out[s][1]).all())


# ====================================================================================================================== streaming rows
def _check(name, got, ref, key):
    from tests.test_kernels_gpu import _check as chk, _tol
    chk(name, got, ref, key)
    scale = max(ref.abs().max().item(), 1e-6)
    REPORT["margins"][name] = {"margin": (got - ref).abs().max().item() / (_tol(key) * scale)}


def _frow(shape, scale=1.0, shift=0.0, absolute=False):
    def fn(seed):
        g = torch.Generator().manual_seed(seed)
        v = torch.randn((1,) + tuple(shape), generator=g) * scale
        return ((v.abs() if absolute else v) + shift).to(DEV)
    return fn


IMG = L.SHAPES[64]
QUARTER = (IMG[0] // 2, IMG[1] // 2, IMG[2])
STREAM_STORAGES = L.STORAGES


@pytest.mark.parametrize("direction", ["from", "to"])
@pytest.mark.parametrize("storage", ["f16", "split", "mx"])
def test_convert_past_the_wrap_points(storage, direction):
    ops, P = _ops(), _P()
    name = "stream/convert-%s-%s" % (direction, storage)
    _need(name, L.need_bytes(L.rows()[name]))
    src, dst = (_tdt(storage), torch.float32) if direction == "from" else (torch.float32, _tdt(storage))
    slots, p_in, _, p_out = run_batched(name, L.N, {"src": (IMG, src, 1.5, 0.0)}, {}, lambda t, rows, m: (ops.convert(t["src"], dst),))
    s = slots[-3]
    if direction == "from":                                              # the host decoder, exactly
        assert torch.equal(p_out[s][0].cpu(), _host(p_in[s]["src"]))
    else:                                                               # the host packer, byte for byte (finite input)
        want = P.from_float(p_in[s]["src"].cpu(), dst)
        assert torch.equal(_iv(p_out[s][0]).cpu(), _iv(want))


UPS = [(st, form) for st in STREAM_STORAGES for form in ("plain", "scale")] + [("split", "tof16"), ("mx", "tof16")]


@pytest.mark.parametrize("storage,form", UPS, ids=["%s-%s" % u for u in UPS])
def test_upsample2x_past_the_wrap_points(storage, form):
    ops = _ops()
    name = "stream/upsample2x-%s%s" % ({"plain": "", "scale": "scale-", "tof16": "tof16-"}[form], storage)
    _need(name, L.need_bytes(L.rows()[name]))
    rows = {"scale": _frow((IMG[2],), 1.0, 0.5, True)} if form == "scale" else {}
    odt = torch.float16 if form == "tof16" else None
    slots, p_in, p_row, p_out = run_batched(name, L.N, {"src": (QUARTER, _tdt(storage), 1.5, 0.0)}, rows,
                                            lambda t, rw, m: (ops.upsample2x(t["src"], scale=rw.get("scale"), out_dtype=odt),))
    s = slots[-3]
    ref = F.interpolate(_host(p_in[s]["src"]).permute(0, 3, 1, 2).double(), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    if form == "scale":
        ref = ref * p_row[s]["scale"].cpu().double()[:, None, None, :]
    _check(name, _host(p_out[s][0]).double(), ref, _key("f16" if form == "tof16" else storage))


@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("storage", STREAM_STORAGES)
def test_affine_act_past_the_wrap_points(storage, inplace):
    ops, P = _ops(), _P()
    name = "stream/affine_act-%s%s" % ("inplace-" if inplace else "", storage)
    _need(name, L.need_bytes(L.rows()[name]))

    def launch(t, rw, m):
        x = t["x"]
        if inplace:
            x = x if m == L.N else P.tag(P.untag(x).clone())             # (the probe images are read again below)
            return (ops.affine_act(x, rw["scale"], rw["shift"], swish=True, out=x),)
        return (ops.affine_act(x, rw["scale"], rw["shift"], swish=True),)

    slots, p_in, p_row, p_out = run_batched(name, L.N, {"x": (IMG, _tdt(storage), 2.0, 0.3)}, {"scale": _frow((IMG[2],), 1.0, 1.0), "shift": _frow((IMG[2],), 0.3)}, launch)
    s = slots[-3]
    t = _host(p_in[s]["x"]).double() * p_row[s]["scale"].cpu().double()[:, None, None, :] + p_row[s]["shift"].cpu().double()[:, None, None, :]
    _check(name, _host(p_out[s][0]).double(), t * torch.sigmoid(t), _key(storage))


@pytest.mark.parametrize("storage", STREAM_STORAGES)
def test_groupnorm_affine_past_the_wrap_points(storage):
    """ragged valid_w; the scale and shift rows of the probe images equal the n = 1 rows bit for bit (and every other row the filler's)"""
    from tests.test_kernels_gpu import _rnd
    from tests.test_tail_kernels_gpu import _gn_reference
    ops = _ops()
    name = "stream/groupnorm_affine-" + storage
    _need(name, L.need_bytes(L.rows()[name]))
    h, w, c = IMG
    gamma, beta = 1 + 0.1 * _rnd((c,), 402), 0.1 * _rnd((c,), 403)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    vw = lambda seed: torch.tensor([[(1, w, 301, w // 2 + 1, 17)[seed % 5]]], dtype=torch.int32, device=DEV)
    slots, p_in, p_row, p_out = run_batched(name, L.N, {"x": (IMG, _tdt(storage), 0.5, 3.0)}, {"valid_w": vw},
                                            lambda t, rw, m: ops.groupnorm_affine(t["x"], gd, bd, 1e-6, rw["valid_w"].reshape(-1)))
    s = slots[-3]
    v = int(p_row[s]["valid_w"].item())
    rsc, rsh = _gn_reference(_host(p_in[s]["x"]).permute(0, 3, 1, 2), 0, v, gamma, beta)
    esc, esh = (p_out[s][0][0].cpu().double() - rsc).abs().max().item(), (p_out[s][1][0].cpu().double() - rsh).abs().max().item()
    REPORT["margins"][name] = {"margin_scale": esc / (2e-6 * rsc.abs().max().item()), "margin_shift": esh / (2e-6 * max(1.0, rsh.abs().max().item()))}
    assert esc <= 2e-6 * rsc.abs().max().item() and esh <= 2e-6 * max(1.0, rsh.abs().max().item()), (esc, esh)


@pytest.mark.parametrize("direction", ["nchw_to_nhwc", "nhwc_to_nchw"])
@pytest.mark.parametrize("storage", STREAM_STORAGES)
def test_layout_kernels_past_the_wrap_points(storage, direction):
    ops = _ops()
    name = "stream/%s-%s" % (direction, storage)
    _need(name, L.need_bytes(L.rows()[name]))
    h, w, c = IMG
    if direction == "nchw_to_nhwc":
        slots, p_in, _, p_out = run_batched(name, L.N, {"src": ((c, h, w), torch.float32, 1.5, 0.0)}, {}, lambda t, rw, m: (ops.nchw_to_nhwc(t["src"], _tdt(storage)),))
        s = slots[-3]
        _check(name, _host(p_out[s][0]).double(), p_in[s]["src"].cpu().permute(0, 2, 3, 1).double(), _key(storage))
    else:
        slots, p_in, _, p_out = run_batched(name, L.N, {"src": (IMG, _tdt(storage), 1.5, 0.0)}, {}, lambda t, rw, m: (ops.nhwc_to_nchw(t["src"]),))
        s = slots[-3]
        assert torch.equal(p_out[s][0].cpu(), _host(p_in[s]["src"]).permute(0, 3, 1, 2))          # the stored values, exactly


@pytest.mark.parametrize("storage", STREAM_STORAGES)
def test_torgb_past_the_wrap_points(storage):
    """big input, small output"""
    from tests import rgb_kernels as R
    ops = _ops()
    name = "stream/torgb-" + storage
    _need(name, L.need_bytes(L.rows()[name]))
    h, w, c = IMG
    g = torch.Generator().manual_seed(_seed(name, "w"))
    wgt = torch.randn((3, c), generator=g) * (0.4 / math.sqrt(2.048 * c))
    bias = torch.tensor([0.1, -0.2, 0.15, 0.0])
    wd, bd = wgt.to(DEV), bias.to(DEV)
    slots, p_in, p_row, p_out = run_batched(
        name, L.N, {"x": (IMG, _tdt(storage), 1.0, 0.0), "skip": ((h // 2, w // 2, 4), torch.float32, 0.3, 0.0)},
        {"style": _frow((c,), 1.0, 0.5, True), "scale_b": _frow((), 0.5, 1.0)},
        lambda t, rw, m: (ops.torgb(t["x"], wd, rw["style"], rw["scale_b"].reshape(-1), bd, t["skip"]),))
    s = slots[-3]
    ref, _, mag = R.torgb_ref(_host(p_in[s]["x"]).double().numpy(), wgt.numpy(), p_row[s]["style"].cpu().numpy(), p_row[s]["scale_b"].cpu().numpy().reshape(1),
                              bias.numpy(), p_in[s]["skip"].cpu().numpy())
    got = p_out[s][0].cpu().numpy()
    m = float((np.abs(got[..., :3].astype(np.float64) - ref) / (R.BOUND * (mag + 1.0))).max())
    REPORT["margins"][name] = {"margin": m}
    assert m <= 1.0 and (got[..., 3] == 0).all(), m


@pytest.mark.parametrize("storage", STREAM_STORAGES)
def test_conv3x3_rgb_past_the_wrap_points(storage):
    from tests import rgb_kernels as R
    ops = _ops()
    name = "stream/conv3x3_rgb-" + storage
    _need(name, L.need_bytes(L.rows()[name]))
    g = torch.Generator().manual_seed(_seed(name, "w"))
    wgt = torch.randn((3, 3, 3, 64), generator=g) * (0.5 / 24.0)
    if storage == "f16":
        wgt = wgt.half().float()
    bias = torch.tensor([0.1, -0.05, 0.02])
    wd, bd = wgt.to(torch.float16 if storage == "f16" else torch.float32).to(DEV), bias.to(DEV)
    slots, p_in, _, p_out = run_batched(name, L.N, {"x": (IMG, _tdt(storage), 1.0, 0.0)}, {}, lambda t, rw, m: ops.conv3x3_rgb(t["x"], wd, bd, R.ACT_TANH, True, True))
    s = slots[-3]
    band = slice(IMG[0] // 2 - 3, IMG[0] // 2 + 3)                       # rows 45 .. 50: reference over rows 46 .. 49 (the band's own border rows see the zero padding)
    ref, _, mag = R.conv_rgb_ref(_host(p_in[s]["x"])[:, band].double().numpy(), wgt.numpy(), bias.numpy(), R.ACT_TANH)
    ref, mag = ref[:, 1:-1], mag[:, 1:-1]
    got = p_out[s][0].float().cpu().numpy()[:, band][:, 1:-1, :, :3]
    bound = R.BOUND * (mag + 1.0) + (R.F16_EPS * np.abs(ref) if storage == "f16" else 0.0)
    m = float((np.abs(got.astype(np.float64) - ref) / bound).max())
    REPORT["margins"][name] = {"margin": m}
    assert m <= 1.0, m
    assert torch.equal(p_out[s][1].cpu(), p_out[s][0][..., :3].float().permute(0, 3, 1, 2).cpu())


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_sr_postprocess_past_the_wrap_points(storage):
    """at the pipeline's c_ld = 8"""
    ops = _ops()
    name = "stream/sr_postprocess-" + storage
    _need(name, L.need_bytes(L.rows()[name]))
    shape = (96, 4096, 8)
    slots, p_in, _, p_out = run_batched(name, L.N, {"src": (shape, _tdt(storage), 0.7, 0.0)}, {}, lambda t, rw, m: (ops.sr_postprocess(t["src"], u8=True),))
    s = slots[-3]
    y = p_in[s]["src"].cpu()[..., :3]
    want = np.clip((y.float() * 0.5 + 0.5).flip(3).numpy(), 0, 1) * 255.0
    assert np.array_equal(p_out[s][0].cpu().numpy(), np.rint(want).astype(np.uint8))


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_nonfinite_flag_past_the_wrap_points(storage):
    """a clean tensor gives 0; one inf planted at the element on either side of each wrap point, and at the last element, is found — one launch per plant"""
    ops = _ops()
    name = "stream/nonfinite_flag-" + storage
    _need(name, L.need_bytes(L.rows()[name]))
    dt = _tdt(storage)
    x = _big(L.N, _enc((1,) + IMG, dt, _seed(name)), {})
    flat = x.view(-1)
    assert flat.numel() == L.N * L.E > 1 << 31
    assert ops.nonfinite_flag(x).item() == 0
    spots = sorted({off + d for off in L.wrap_points(L.S_BYTES[storage]).values() for d in (-1, 0)} | {flat.numel() - 1})
    missed = []
    for pos in spots:
        keep = flat[pos].clone()
        flat[pos] = float("inf")
        if ops.nonfinite_flag(x).item() != 1:
            missed.append(pos)
        flat[pos] = keep
    assert not missed, "an inf at elements %s is not found" % missed
    assert ops.nonfinite_flag(x).item() == 0


@pytest.mark.parametrize("storage", ["f16", "mx", "split", "f32"])
def test_compare_stats_past_the_wrap_points(storage):
    """groups are images; the probe groups' records equal the n = 1 records; a planted worst element in the last group is reported with its exact 64-bit index"""
    from marconet_amd import _lib
    ops = _ops()
    name = "stream/compare_stats-" + storage
    _need(name, L.need_bytes(L.rows()[name]))
    def launch(t, rw, m):
        return (ops.compare_stats(t["mode"], t["ref"], groups=m),)

    def tweak(who, tensors):                                             # the reference of the LAST image holds 30000 at its last element: the worst pair of that group
        if who == L.N - 1:
            tensors["ref"].view(-1)[-1] = 30000.0

    slots, p_in, _, p_out = run_batched(name, L.N, {"mode": (IMG, _tdt(storage), 1.0, 0.0), "ref": (IMG, torch.float32, 1.0, 0.0)}, {}, launch, tweak=tweak)
    last = _lib.cmp_records(p_out[L.N - 1][0].cpu().numpy())[0]
    assert last.argmax_index == L.E - 1 and last.max_abs_ref == 30000.0 and last.nonfinite_mode == 0 and last.nonfinite_ref == 0
    s = slots[-3]
    rec = _lib.cmp_records(p_out[s][0].cpu().numpy())[0]
    mode, ref = _host(p_in[s]["mode"]).reshape(-1), p_in[s]["ref"].cpu().reshape(-1)
    d = (mode - ref).abs()
    assert rec.max_abs_diff == d.max().item() and rec.argmax_index == int((d == d.max()).nonzero()[0]) and rec.max_abs_ref == ref.abs().max().item()
    assert abs(rec.sum_sq_diff - float((mode.double() - ref.double()).pow(2).sum())) <= 1e-6 * rec.sum_sq_diff


UPFOLD = [(st, False) for st in STREAM_STORAGES] + [("mx", True)]


@pytest.mark.parametrize("storage,f32z", UPFOLD, ids=["%s%s" % (s, "-f32z" if f else "") for s, f in UPFOLD])
def test_upfold3x3_past_the_wrap_points(storage, f32z):
    """the fold and its fp32-plane form: z [n,48,256,9*64] (itself past element offset 2^32) -> y [n,96,512,64], all three vectors, LRELU_SQRT2"""
    from tests.test_kernels_gpu import _rnd
    from tests.test_upfold import epilogue_ref, fold_ref
    ops = _ops()
    name = "stream/upfold3x3_f32z" if f32z else "stream/upfold3x3-" + storage
    _need(name, L.need_bytes(L.rows()[name]))
    h, w, c = QUARTER
    zdt, ydt = (torch.float32 if f32z else _tdt(storage)), _tdt(storage)
    bias = _rnd((c,), _seed(name, "bias"), 0.3)
    bd = bias.to(DEV)
    slots, p_in, p_row, p_out = run_batched(
        name, L.N, {"z": ((h, w, 9 * c), zdt, 1.5, 0.0)}, {"out_scale": _frow((c,), 1.0, 0.5, True), "post_scale": _frow((c,), 1.0, 0.25, True)},
        lambda t, rw, m: (ops.upfold3x3(t["z"], c, out_scale=rw["out_scale"], bias=bd, act=3, post_scale=rw["post_scale"], out_dtype=ydt),))
    s = slots[-3]
    sums = fold_ref(_host(p_in[s]["z"]).permute(0, 3, 1, 2).double().contiguous(), c)
    ref = epilogue_ref(sums, p_row[s]["out_scale"].cpu(), bias, 3, p_row[s]["post_scale"].cpu())
    _check(name, _host(p_out[s][0]).permute(0, 3, 1, 2).double(), ref, _key(storage))


ADAIN = [(st, form) for st in STREAM_STORAGES for form in ("adain_crop_concat", "adain_crop_concat_gn", "adain_crop_concat_gn_split")]


@pytest.mark.parametrize("storage,form", ADAIN, ids=["%s-%s" % a for a in ADAIN])
def test_adain_past_the_wrap_points(storage, form):
    """one glyph per slot, glyph g on image g: out [G,48,48,128] past every wrap point, prior and feat past those their size reaches; G <= 65535, so the split
    form runs the same launch.  (c): the restyled half and the copied half against fp64, the bounds of tests/test_glyph_fusion_gpu.py"""
    from tests import glyph_fusion as GF
    from tests.test_kernels_gpu import _rnd, _tol
    ops = _ops()
    name = "stream/%s-%s" % (form, storage)
    _need(name, L.need_bytes(L.rows()[name]))
    S, C, FW, G = L.GLYPH_S, L.GLYPH_C, L.GLYPH_FW, L.G_ADAIN
    gamma, beta = 1 + 0.1 * _rnd((2 * C,), 402), 0.1 * _rnd((2 * C,), 403)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    win = lambda seed: ((S, S - 1, 17, 33, 2, S)[seed % 6], (seed // 7), (seed // 11))

    def table(seed):                                                    # [1, 3] int32: g_w, x1, y1 of the slot's glyph
        gw, a, b = win(seed)
        return torch.tensor([[gw, a % (FW - gw + 1), b % (S - gw + 1)]], dtype=torch.int32, device=DEV)

    def launch(t, rw, m):
        tab = rw["win"]
        g_img = torch.arange(m, dtype=torch.int32, device=DEV)
        g_w, g_x1, g_y1 = (tab[:, i].contiguous() for i in range(3))
        if form == "adain_crop_concat":
            return (ops.adain_crop_concat(t["prior"], t["feat"], g_img, g_x1, g_y1, g_w),)
        return ops.adain_crop_concat_gn(t["prior"], t["feat"], g_img, g_x1, g_y1, g_w, gd, bd, GF.GN_EPS, split=form.endswith("split"))

    dt = _tdt(storage)
    slots, p_in, p_row, p_out = run_batched(name, G, {"prior": ((S, S, C), dt, 1.0, 0.2), "feat": ((S, FW, C), dt, 0.7, -0.1)}, {"win": table}, launch)
    s = slots[-3]
    gw, x1, y1 = (int(v) for v in p_row[s]["win"][0].tolist())
    prior, feat = _host(p_in[s]["prior"]).permute(0, 3, 1, 2), _host(p_in[s]["feat"]).permute(0, 3, 1, 2)
    wins = [(0, x1, gw, y1)]
    ref = GF.ref_adain_fp64(prior, feat, wins)[0]
    got = _host(p_out[s][0]).permute(0, 3, 1, 2)[0]
    assert (got[:, :, gw:] == 0).all()
    gs = {"f32": GF.F32, "f16": GF.F16, "split": GF.SPLIT, "mx": GF.MX}[storage]
    if storage in ("f32", "f16"):
        ratio = (got[:C, :, :gw].double() - ref[:C]).abs() / GF.adain_bound(prior, feat, wins, gs)[0]
    else:
        ratio = (got[:, :, :gw].double() - ref).abs() / (_tol(_key(storage)) * 2.0 * ref.abs().max())
    REPORT["margins"][name] = {"margin": float(ratio.max())}
    assert float(ratio.max()) <= 1.0, float(ratio.max())
    assert torch.equal(got[C:, :, :gw], feat[0, :, :, x1:x1 + gw])       # the feature half is a copy


@pytest.mark.parametrize("storage", STREAM_STORAGES)
def test_glyph_scatter_affine_past_the_wrap_points(storage):
    """one glyph per image: feat and out [B,48,64,64] past every wrap point, scale / shift [G = B,48,48,64] past those their size reaches.  (c): the existing
    test's exactness — fl(fl(f * sc) + sh), then fl(f + .) of the stored values, rounded once to the storage"""
    from tests import glyph_fusion as GF
    ops, P = _ops(), _P()
    name = "stream/glyph_scatter_affine-" + storage
    _need(name, L.need_bytes(L.rows()[name]))
    S, C, FW, B = L.GLYPH_S, L.GLYPH_C, L.GLYPH_FW, L.B_SCATTER

    def table(seed):                                                    # [1, 2] int32: g_w, x1
        gw = (S, S - 1, 17, 33, 1, S)[seed % 6]
        return torch.tensor([[gw, (seed // 7) % (FW - gw + 1)]], dtype=torch.int32, device=DEV)

    def launch(t, rw, m):
        g_start = torch.arange(m + 1, dtype=torch.int32, device=DEV)
        return (ops.glyph_scatter_affine(t["feat"], t["scale"], t["shift"], g_start, rw["win"][:, 1].contiguous(), rw["win"][:, 0].contiguous()),)

    dt = _tdt(storage)
    slots, p_in, p_row, p_out = run_batched(name, B, {"feat": ((S, FW, C), dt, 1.0, 0.0), "scale": ((S, S, C), dt, 0.5, 0.0), "shift": ((S, S, C), dt, 0.3, 0.0)},
                                            {"win": table}, launch)
    s = slots[-3]
    gw, x1 = (int(v) for v in p_row[s]["win"][0].tolist())
    nchw = lambda t: _host(t).permute(0, 3, 1, 2).contiguous()
    want = GF.ref_scatter(nchw(p_in[s]["feat"]), nchw(p_in[s]["scale"]), nchw(p_in[s]["shift"]), [0, 1], [x1], [gw])
    out = p_out[s][0]
    if storage == "f32":
        assert torch.equal(nchw(out), want)
    elif storage == "f16":
        assert torch.equal(out.cpu().permute(0, 3, 1, 2), want.half())
    else:
        # the columns the glyph owns: the host packer's bytes of the fp32 result; the others: the input's own bytes (decoding and packing again
        # does not give a blocked tensor's bytes back — a residual that underflowed keeps its sign in the lo part — so they are compared raw)
        words = lambda t: P.untag(t).cpu().view(torch.int32)             # [1, S, FW, C]
        got, enc, raw = words(out), words(P.from_float(want.permute(0, 2, 3, 1).contiguous(), dt)), words(p_in[s]["feat"])
        assert torch.equal(got[:, :, x1:x1 + gw], enc[:, :, x1:x1 + gw])
        assert torch.equal(got[:, :, :x1], raw[:, :, :x1]) and torch.equal(got[:, :, x1 + gw:], raw[:, :, x1 + gw:])


# ====================================================================================================================== section 4: the largest LDS-DMA maps
@pytest.mark.parametrize("storage,c0", sorted(L.LARGEST), ids=["%s-c%d" % k for k in sorted(L.LARGEST)])
def test_largest_maps_the_lds_dma_kernels_take(storage, c0):
    """n = 2, h * w the largest the address-range conditions accept (no multiple of 512: a tile straddles the two images), cout 64, 3x3, bias + residual:
    the planner names an LDS-DMA id; the result is inside the geometry contract's bound against fp64 over the first two, the two middle and the last two rows
    of each image; the whole map agrees with the register-staged launch within twice that bound (each is within the bound of the same fp64 value); one row
    past the limit AUTO runs the register-staged kernel and meets the same bound"""
    from tests import conv_contract as C
    from tests import conv_geometry as G
    from tests.test_conv_epilogue_contract_gpu import _tolerances
    from tests.test_kernels_gpu import _pack_w, _rnd
    ops = _ops()
    row = L.LARGEST[(storage, c0)]
    dt, dtype_id, cout, n = _tdt(storage), L.STORAGES.index(storage), 64, 2
    name = "largest/%s-c%d" % (storage, c0)
    esz = L.S_BYTES[storage]
    (h, w), (hp, wp_) = row["ok"], row["past"]
    _need(name, n * hp * wp_ * (c0 + 3 * cout) * esz + n * hp * wp_ * cout * 4)
    seed = _seed(name)
    wt = _rnd((cout, c0, 3, 3), seed, 1.0 / math.sqrt(c0 * 9))
    if storage == "f16":
        wt = wt.half().float()
    wpk = _pack_w(wt, _key(storage))
    bias = _rnd((cout,), seed + 1, 0.3)
    bias_d = bias.to(DEV)
    x_all = _enc((n, hp, wp_, c0), dt, seed + 2)                        # the map one row past the limit; the eligible map is its first h rows (of width w == wp_)
    res_all = _enc((n, hp, wp_, cout), dt, seed + 3)
    assert w == wp_ and hp == h + 1
    rep = {}
    P = _P()

    def sub(t, rows_):
        return P.tag(P.untag(t)[:, :rows_].contiguous())

    def check(tag, hh, k, y, x, res):
        band = [0, 1, hh // 2 - 1, hh // 2, hh - 2, hh - 1]
        need = sorted({r for b in band for r in (b - 1, b, b + 1) if 0 <= r < hh})
        xs = torch.zeros((n, c0, hh + 2, w + 2))
        xs[:, :, [r + 1 for r in need], 1:-1] = _host(_take_rows(x, need)).permute(0, 3, 1, 2)
        rs = _host(_take_rows(res, band)).permute(0, 3, 1, 2).double()
        yb = _take_rows(y, band)
        got = (yb if yb.dtype in (torch.float32, torch.float16) else ops.convert(yb, torch.float32)).float().cpu().permute(0, 3, 1, 2).double()
        bound = None
        for kind, tol in _tolerances(storage, k, {"act": 3, "xform": "none", "src2": "none"}):
            wk = wt if kind in ("true", "emu") else {"mx": G.H.wdec}.get(storage, lambda t: t)(wt)
            conv = (lambda t: G.H.emulate(t, wk, stride=1, padding=0).double()) if kind == "emu" else (lambda t: F.conv2d(t.double(), wk.double()))
            v = torch.cat([conv(xs[:, :, b:b + 3]) for b in band], dim=2) + bias.double()[None, :, None, None] + rs
            ref = G.H.act(v, 3)
            scale = max(float(ref.abs().max()), 1e-6)
            err = float((got - ref).abs().max())
            rep["%s_margin_%s" % (tag, kind)] = err / (tol * scale)
            assert err <= tol * scale, "%s %s: kernel %d vs the %s reference: %.3e > %.1e x %.3e" % (name, tag, k, kind, err, tol, scale)
            bound = max(bound or 0.0, tol * scale)
        return bound

    x, res = sub(x_all, h), sub(res_all, h)
    k = _conv_plan(dtype_id, n, h, w, c0, 0, cout, 0, True, True, False)
    assert C.is_dma(k), "the planner gives the largest eligible map to kernel %d" % k
    y = ops.conv2d(x, wpk, cout, 3, 3, (1, 1), (1, 1), bias=bias_d, residual=res, act=3, algo=k)
    bound = check("dma", h, k, y, x, res)
    yr = ops.conv2d(x, wpk, cout, 3, 3, (1, 1), (1, 1), bias=bias_d, residual=res, act=3, algo=C.ALGO_REG)
    check("reg", h, C.ALGO_REG, yr, x, res)
    dec = lambda t: t.float() if t.dtype in (torch.float32, torch.float16) else ops.convert(t, torch.float32)
    worst = 0.0
    for i in range(n):                                                  # the whole map, on the device, an image at a time
        worst = max(worst, float((dec(P.tag(P.untag(y)[i:i + 1])) - dec(P.tag(P.untag(yr)[i:i + 1]))).abs().max()))
    rep["dma_vs_reg_margin"] = worst / (2 * bound)                     # `bound`: the LDS-DMA launch's bound x the output scale of the reference rows
    assert worst <= 2 * bound, "%s: the LDS-DMA and the register-staged launch differ by %.3e > 2 x %.3e" % (name, worst, bound)
    del y, yr, x, res
    kp = _conv_plan(dtype_id, n, hp, wp_, c0, 0, cout, 0, True, True, False)
    assert kp == C.ALGO_REG, "one row past the limit the planner names kernel %d" % kp
    yp = ops.conv2d(x_all, wpk, cout, 3, 3, (1, 1), (1, 1), bias=bias_d, residual=res_all, act=3, algo=0)
    check("past", hp, kp, yp, x_all, res_all)
    REPORT["margins"][name] = rep
    REPORT["plans"][name] = k
