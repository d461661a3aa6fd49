"""-m gpu: every device writer and reader of the half-range storages (plain f16, split half, fp16+8) against the spec of tests/storage_codec.py, BYTE for byte.

Writers are fed so that the fp32 value in front of the store is known exactly (a copy, x * 1, 0 * -1 + v, 0 + bias), the stored bytes are compared with the
spec's over the whole tensor, the padding bytes 97-127 of an fp16+8 block included.  Readers get raw blocks uploaded as bytes and are compared with the
spec's decoder bit for bit.  The pages (tests/storage_codec.py) sit where encoders go wrong: e4m3 ties, binade edges of the block maximum, maxima that change
binade when rounded to half, fp16-subnormal blocks (the floor of the exponent at 105), blocks whose every hi is +-0, signed zeros.  No finite page is left out
of any comparison; the non-finite pages have a test of their own that asserts what the pipeline relies on.  storage_codec.json in the report directory lists what ran
(per writer, reader and storage: the pages compared, the kernel every conv request resolved to)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import conv_contract as C
from tests import storage_codec as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPORT = {"writers": {}, "readers": {}, "weights": {}, "nonfinite": {}}
PAGES = S.writer_pages()
NAMES = [p["name"] for p in PAGES]
TABLE = S.writer_table()
P = TABLE.shape[0]
STORAGES = ("mx", "split", "f16")


def _ops():
    from marconet_amd import ops
    return ops


def _pk():
    from marconet_amd import packing
    return packing


def _dtype(storage):
    pk = _pk()
    return {"mx": pk.MX_DTYPE, "split": pk.SPLIT_DTYPE, "f16": torch.float16, "f32": torch.float32}[storage]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _raw(t):
    """the bytes of a device tensor of any storage type, flat, on the host"""
    torch.cuda.synchronize()
    return _pk().untag(t).contiguous().view(torch.uint8).reshape(-1).cpu().numpy()


def _upload(raw, shape, storage):
    """raw bytes -> a device tensor of logical ``shape`` in ``storage``"""
    t = _dev(np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1)).view(_dtype(storage)).reshape(shape)
    assert t.data_ptr() % 128 == 0
    return _pk().tag(t)


def _zeros(shape, storage):
    return _pk().new_tensor(shape, _dtype(storage), DEV, zero=True)


def _bad_pages(got, want, names):
    """got, want uint8 [len(names), bytes] -> the names of the rows that differ, with the first differing byte"""
    got, want = got.reshape(len(names), -1), want.reshape(len(names), -1)
    assert got.shape == want.shape, (got.shape, want.shape)
    out = []
    for i in np.nonzero((got != want).any(1))[0]:
        j = int(np.nonzero(got[i] != want[i])[0][0])
        out.append("%s (byte %d of block %d: 0x%02x, spec 0x%02x; %d bytes differ)" % (names[i], j % 128, j // 128, got[i, j], want[i, j], int((got[i] != want[i]).sum())))
    return out


def _log(kind, name, storage, **kw):
    REPORT[kind].setdefault(name, {})[storage] = kw


@pytest.fixture(scope="module", autouse=True)
def _write_report(report_dir):
    yield
    with open(os.path.join(report_dir, "storage_codec.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


# ================================================================================================================ writers: the streaming and layout kernels
@pytest.mark.parametrize("storage", STORAGES)
def test_convert_from_fp32_writes_the_spec_bytes(storage):
    got = _raw(_ops().convert(_dev(TABLE), _dtype(storage)))
    bad = _bad_pages(got, S.ENCODE[storage](TABLE), NAMES)
    _log("writers", "convert", storage, pages=NAMES)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("storage", STORAGES)
def test_nchw_to_nhwc_writes_the_spec_bytes(storage):
    """pixel p of a 5 x 9 map (HW = 45: no multiple of the 32-pixel tile) carries page (p + image) % P; then c = 232 < c_ld = 256: a block filled up with zeros"""
    n, h, w = 2, 5, 9
    idx = (np.arange(h * w)[None, :] + 3 * np.arange(n)[:, None]) % P                    # [n, hw]
    nhwc = TABLE[idx]                                                                   # [n, hw, 256]
    names = ["img%d/px%d/%s" % (i, p, NAMES[idx[i, p]]) for i in range(n) for p in range(h * w)]
    fails = []
    for c in (256, 232):
        src = np.ascontiguousarray(nhwc[:, :, :c].transpose(0, 2, 1)).reshape(n, c, h, w)
        want = nhwc.copy()
        want[:, :, c:] = 0.0
        got = _raw(_ops().nchw_to_nhwc(_dev(src), _dtype(storage), c_ld=256))
        fails += ["c=%d: %s" % (c, b) for b in _bad_pages(got, S.ENCODE[storage](want.reshape(-1, 256)), names)]
    _log("writers", "nchw_to_nhwc", storage, pages=NAMES, shapes=["c=256", "c=232 of c_ld=256"])
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("storage", STORAGES)
def test_embed_gather_writes_the_spec_bytes(storage):
    nc = (P + 1) // 2
    labels = (np.arange(2 * nc) % P).reshape(2, nc)
    out = _ops().embed_gather(_dev(TABLE), _dev(labels.astype(np.int64)), _dtype(storage), P)
    assert tuple(out.shape) == (2, 4, 4 * nc, 256)
    idx = np.broadcast_to(np.repeat(labels, 4, axis=1)[:, None, :], (2, 4, 4 * nc)).reshape(-1)
    bad = _bad_pages(_raw(out), S.ENCODE[storage](TABLE[idx]), ["px%d/%s" % (i, NAMES[j]) for i, j in enumerate(idx)])
    _log("writers", "embed_gather", storage, pages=NAMES)
    assert not bad, "\n".join(bad[:40])


@pytest.mark.parametrize("storage", STORAGES)
def test_affine_act_writes_the_spec_bytes(storage):
    """x = 0, scale = -1, shift = the page: 0 * -1 + v = -0 + v = v for EVERY v, the two zeros included (+0 * 1 + -0 would lose the sign)"""
    hw = 6
    x = _zeros((P, 2, 3, 256), storage)
    out = _ops().affine_act(x, _dev(np.full((P, 256), -1.0, dtype=np.float32)), _dev(TABLE))
    bad = _bad_pages(_raw(out), S.ENCODE[storage](np.repeat(TABLE, hw, axis=0)), ["%s/px%d" % (nm, i) for nm in NAMES for i in range(hw)])
    _log("writers", "affine_act", storage, pages=NAMES)
    assert not bad, "\n".join(bad[:40])


@pytest.mark.parametrize("storage,out", [(s, "same") for s in STORAGES] + [("mx", "f16"), ("split", "f16")])
def test_upsample2x_writes_the_spec_bytes(storage, out):
    """x = 1 everywhere (1/4 + 3/4 is exact in both passes), scale = the page: every output pixel is 1 * v = v.  A 3 x 3 map: corner, edge and inner taps."""
    one = S.ENCODE[storage](np.ones((P * 9, 256), dtype=np.float32))
    x = _upload(one, (P, 3, 3, 256), storage)
    y = _ops().upsample2x(x, scale=_dev(TABLE), out_dtype=torch.float16 if out == "f16" else None)
    so = "f16" if out == "f16" else storage
    assert tuple(y.shape) == (P, 6, 6, 256)
    bad = _bad_pages(_raw(y), S.ENCODE[so](np.repeat(TABLE, 36, axis=0)), ["%s/px%d" % (nm, i) for nm in NAMES for i in range(36)])
    _log("writers", "upsample2x" + ("->f16" if out == "f16" else ""), storage, pages=NAMES)
    assert not bad, "\n".join(bad[:40])


# ================================================================================================================ writers: every conv epilogue
SMALL = (1, 8, 32, 64, 256)                      # n, h, w, cin, cout: 256 output pixels, 8 blocks per pixel — one page per launch
BIG_REQ = {"big64": ("auto", "dma5", "dma13", "strip1"), "big256": ("auto", "dma6", "dma8", "dma9", "dma11", "dma15", "dma16", "strip0")}


def _conv_pages(storage, shape, reqs, fails, where):
    """zero input, zero weights, the page through the bias: every output pixel is 0 + bias (a -0 bias comes out as +0: the spec encodes 0 + v).  One launch per
    page and 256-channel window of the output; the whole output tensor is compared on the device"""
    ops, pk = _ops(), _pk()
    n, h, w, cin, cout = shape
    x = _zeros((n, h, w, cin), storage)
    rows = pk.mx_weight_rows(cout, 3, 3, cin) if storage == "mx" else cout
    wz = _zeros((rows, 3, 3, cin), storage)
    out = _zeros((n, h, w, cout), storage)
    per = cout * (2 if storage == "f16" else 4)
    v = (np.float32(0.0) + TABLE).astype(np.float32)                                      # the epilogue's sum
    want = _dev(S.ENCODE[storage](v.reshape(-1, cout)))                                   # [P * 256 / cout, bytes per pixel]
    for req in reqs:
        algo = C.requests(storage)[req][0]
        k = ops.conv_plan(x, cout, 3, 3, (1, 1), (1, 1), algo=algo)
        if req == "reg":
            named = k == C.ALGO_REG
        elif req == "auto":
            named = C.is_dma(k) or C.is_strip(k)
        else:
            named = k == algo
        _log("writers", "conv/%s/%s" % (where, req), storage, pages=NAMES, kernel=k)
        if not named:
            fails.append("%s %s %s: the request resolved to kernel %d" % (storage, where, req, k))
            continue
        for i in range(want.shape[0]):
            bias = _dev(TABLE.reshape(-1, cout)[i])
            ops.conv2d(x, wz, cout, 3, 3, (1, 1), (1, 1), bias=bias, out=out, algo=algo)
            got = pk.untag(out).view(torch.uint8).reshape(-1, per)
            if not bool((got == want[i][None, :]).all()):
                g = got.cpu().numpy()
                px = int(np.nonzero((g != want[i].cpu().numpy()[None, :]).any(1))[0][0])
                page = NAMES[i * cout // S.PAGE]
                fails.append("%s %s %s (kernel %d), page %s window %d: %s" % (storage, where, req, k, page, i % (S.PAGE // cout), _bad_pages(
                    g[px:px + 1], want[i].cpu().numpy()[None, :], ["pixel %d" % px])[0]))


@pytest.mark.parametrize("storage", STORAGES)
def test_conv_epilogues_write_the_spec_bytes_small(storage):
    reqs = [r for r in C.requests(storage) if not r.startswith("strip")]
    fails = []
    _conv_pages(storage, SMALL, reqs, fails, "small")
    assert not fails, "%d failures:\n%s" % (len(fails), "\n".join(fails[:60]))


@pytest.mark.parametrize("shape", sorted(BIG_REQ))
@pytest.mark.parametrize("storage", STORAGES)
def test_conv_epilogues_write_the_spec_bytes_big(storage, shape):
    """the strip kernels and the big tiles on the one 128 x 512 map they are made for"""
    n, h, w, c0, c1, cout = C.SHAPES[shape][:6]
    reqs = [r for r in BIG_REQ[shape] if r in C.requests(storage)]
    fails = []
    _conv_pages(storage, (n, h, w, c0, cout), reqs, fails, shape)
    assert not fails, "%d failures:\n%s" % (len(fails), "\n".join(fails[:60]))


# ================================================================================================================ readers
def _reader_cases():
    hm, sp = S.reader_table_hm(), S.reader_table_split()
    return {"mx": hm, "split": sp}


@pytest.mark.parametrize("storage", ("mx", "split"))
def test_convert_reads_the_spec_values(storage):
    raw = _reader_cases()[storage]
    nb = raw.shape[0]
    x = _upload(raw, (nb // 8, 256), storage)
    dec = S.DECODE[storage](raw.reshape(nb // 8, 1024))                                   # fp32 bits [nb / 8, 256]
    names = ["blocks %d-%d" % (8 * i, 8 * i + 7) for i in range(nb // 8)]
    fails = []
    got = _raw(_ops().convert(x, torch.float32))
    fails += ["-> fp32: " + b for b in _bad_pages(got, dec.view(np.uint8), names)]
    vals = S.from_bits32(dec)
    for other in ("f16", "split", "mx"):
        if other == storage or (other == "mx" and not np.isfinite(S.f16_round(vals.astype(np.float64))).all()):
            continue                                                                      # (the bytes of a non-finite fp16+8 block are not defined)
        got = _raw(_ops().convert(x, _dtype(other)))
        fails += ["-> %s: %s" % (other, b) for b in _bad_pages(got, S.ENCODE[other](vals), names)]
    _log("readers", "convert", storage, blocks=nb, to=["fp32", "f16", "split" if storage == "mx" else "mx"])
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("storage", ("mx", "split"))
def test_nhwc_to_nchw_reads_the_spec_values(storage):
    raw = _reader_cases()[storage]
    npix = raw.shape[0] // 8
    h = 7 if npix % 7 == 0 else 5
    assert npix % h == 0
    x = _upload(raw, (1, h, npix // h, 256), storage)
    dec = S.DECODE[storage](raw.reshape(npix, 1024))                                      # [npix, 256]
    fails = []
    for c in (256, 250):
        got = _raw(_ops().nhwc_to_nchw(x, c=c)).view(np.uint32).reshape(c, npix)
        if not np.array_equal(got, dec[:, :c].T):
            ch, px = [int(a[0]) for a in np.nonzero(got != dec[:, :c].T)]
            fails.append("c=%d: channel %d of pixel %d: 0x%08x, spec 0x%08x" % (c, ch, px, got[ch, px], dec[px, ch]))
    _log("readers", "nhwc_to_nchw", storage, blocks=raw.shape[0], shapes=["c=256", "c=250 of c_ld=256"])
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("storage", ("mx", "split"))
def test_conv3x3_rgb_staging_reads_the_spec_values(storage):
    """ACT_NONE, zero bias, fp32 weights that are 1 at the centre tap of ONE input channel per output: the output is that decoded channel (+ 0: the sum starts
    from +0 and every other product is a zero, so a decoded -0 comes out as +0).  The one-hot position sweeps the 64 input channels, three per launch."""
    ops = _ops()
    raw = _reader_cases()[storage]
    npix = raw.shape[0] // 2
    h = next(d for d in (28, 8, 5, 4, 2, 1) if npix % d == 0)
    x = _upload(raw, (1, h, npix // h, 64), storage)
    dec = S.from_bits32(S.DECODE[storage](raw.reshape(npix, 256)))                        # [npix, 64]
    assert np.isfinite(dec).all()
    want = S.bits32(dec + np.float32(0.0))
    bias = _dev(np.zeros(3, dtype=np.float32))
    fails = []
    for p0 in range(0, 64, 3):
        wgt = np.zeros((3, 9, 64), dtype=np.float32)
        chans = [min(p0 + o, 63) for o in range(3)]
        for o, ch in enumerate(chans):
            wgt[o, 4, ch] = 1.0
        _, y = ops.conv3x3_rgb(x, _dev(wgt), bias, act=ops.ACT_NONE, nhwc=False, nchw=True)
        got = _raw(y).view(np.uint32).reshape(3, npix)
        for o, ch in enumerate(chans):
            if not np.array_equal(got[o], want[:, ch]):
                px = int(np.nonzero(got[o] != want[:, ch])[0][0])
                fails.append("channel %d of pixel %d: 0x%08x, spec 0x%08x" % (ch, px, got[o, px], want[px, ch]))
    _log("readers", "conv3x3_rgb", storage, blocks=raw.shape[0], channels=64)
    assert not fails, "\n".join(fails[:40])


# ================================================================================================================ non-finite input
def _flag(t):
    f = _ops().nonfinite_flag(t)
    torch.cuda.synchronize()
    return int(f.item())


def test_nonfinite_elements_stay_visible_and_stay_in_their_block():
    """The bytes of a block that holds an inf / NaN / |v| >= 65520 are not defined: the host packer writes scale byte 119 for a block with an inf, the device
    248.  Observed on an MI355X (mnet_convert from fp32, blocks of |v| ~ 3 around the elements; the run prints them and the report keeps them):
        +-inf                       E = 248 (exponent field 255 - 7), lo byte of the element 0xff
        NaN                         E = 122 (fmaxf drops the NaN: the scale of the finite neighbours), lo byte 0xff
        65520, -1e6, 3e38, -65520   E = 248 (hi = +-inf), lo bytes 0x7f / 0xff
    What the pipeline relies on, through every writer of the streaming family (mnet_convert) and every reader:
      * an element that was non-finite decodes non-finite (convert to fp32 and f16, nhwc_to_nchw, conv3x3_rgb's staging),
      * mnet_nonfinite_flag on the decoded fp32 / f16 tensor is 1,
      * the other blocks of the pixel hold the spec's bytes and decode to the spec's values.
    The same for raw fp16+8 blocks with lo bytes 0x7f / 0xff and with hi = inf / NaN (their finite elements decode to the spec's values too)."""
    ops = _ops()
    pages = S.nonfinite_pages()
    v = S.f32(np.stack([p["v"] for p in pages]))                                          # [3, 256]
    bad = np.stack([p["bad"] for p in pages])
    bad_blk = np.repeat(bad.reshape(3, 8, 32).any(-1), 32, axis=1)                        # elements of the blocks that hold one
    fails, seen = [], {}
    for storage in STORAGES:
        t = ops.convert(_dev(v), _dtype(storage))
        raw = _raw(t).reshape(3, -1)
        per = 2 if storage == "f16" else 4
        if storage == "mx":
            seen = {p["name"]: {"E": raw[i].reshape(8, 128)[[0, 5], 96].tolist(), "lo of the elements": sorted(set(
                raw[i].reshape(8, 128)[:, 64:96][:, S.INV_PERM].reshape(-1)[p["bad"]].tolist()))} for i, p in enumerate(pages)}
        clean = np.where(bad_blk, np.float32(0), v)
        want = S.ENCODE[storage](clean)
        mask_b = np.repeat(~bad_blk, per, axis=1) if storage == "f16" else np.repeat((~bad_blk).reshape(3, 8, 32).any(-1), 128, axis=1)
        if not np.array_equal(raw[mask_b], want[mask_b]):
            fails.append("%s: a block without a non-finite element differs from the spec" % storage)
        back = ops.convert(t, torch.float32)
        dec = _raw(back).view(np.float32).reshape(3, 256)
        if np.isfinite(dec[bad]).any():
            fails.append("%s -> fp32: a non-finite element decodes finite" % storage)
        if not np.array_equal(S.bits32(dec[~bad_blk]), S.DECODE[storage](want)[~bad_blk]):
            fails.append("%s -> fp32: finite blocks of the pixel changed" % storage)
        h = ops.convert(t, torch.float16) if storage != "f16" else t
        hv = _raw(h).view(np.float16).reshape(3, 256)
        if np.isfinite(hv[bad]).any():
            fails.append("%s -> f16: a non-finite element decodes finite" % storage)
        if _flag(back) != 1 or _flag(h) != 1:
            fails.append("%s: nonfinite_flag missed it" % storage)
        if storage != "f16":
            nchw = _raw(ops.nhwc_to_nchw(_pk().tag(_pk().untag(t).reshape(1, 1, 3, 256)))).view(np.float32).reshape(256, 3).T
            if np.isfinite(nchw[bad]).any() or not np.array_equal(S.bits32(nchw[~bad_blk]), S.DECODE[storage](want)[~bad_blk]):
                fails.append("%s nhwc_to_nchw: non-finite element finite, or a finite block changed" % storage)
            x4 = _pk().tag(_pk().untag(t).reshape(1, 1, 12, 64))                              # 4 pixels of 64 channels per page
            b64 = bad.reshape(12, 64)
            for ch in sorted(set(np.nonzero(b64)[1].tolist())):
                wgt = np.zeros((3, 9, 64), dtype=np.float32)
                wgt[0, 4, ch] = 1.0
                _, y = ops.conv3x3_rgb(x4, _dev(wgt), _dev(np.zeros(3, dtype=np.float32)), act=ops.ACT_NONE, nhwc=False, nchw=True)
                y0 = _raw(y).view(np.float32).reshape(3, 12)[0]
                if np.isfinite(y0[b64[:, ch]]).any():
                    fails.append("%s conv3x3_rgb: non-finite channel %d came out finite" % (storage, ch))
    for name, (raw, mask) in S.reader_table_hm_special().items():
        x = _upload(raw, (1, 256), "mx")
        want = S.from_bits32(S.decode_hm(raw.reshape(1, 1024)))[0]
        m = mask.reshape(-1)
        back = ops.convert(x, torch.float32)
        dec = _raw(back).view(np.float32)
        nchw = _raw(ops.nhwc_to_nchw(_pk().tag(_pk().untag(x).reshape(1, 1, 1, 256)))).view(np.float32)
        h = ops.convert(x, torch.float16)
        for what, d in (("convert", dec), ("nhwc_to_nchw", nchw)):
            if np.isfinite(d[m]).any() or not np.array_equal(S.bits32(d[~m]), S.bits32(want[~m])):
                fails.append("%s, %s: special element finite, or a finite element differs from the spec" % (name, what))
        if np.isfinite(_raw(h).view(np.float16)[m]).any() or _flag(back) != 1 or _flag(h) != 1:
            fails.append("%s: not visible in f16 / to nonfinite_flag" % name)
    REPORT["nonfinite"] = {"device bytes of the blocks that hold the elements (fp16+8, mnet_convert)": seen}
    print("observed fp16+8 bytes:", seen)
    assert not fails, "\n".join(fails)


# ================================================================================================================ the weight packer
def _pack(w, storage, cout_pad, cin_pad, **kw):
    return _raw(_ops().pack_weights(_dev(w), _dtype(storage), cout_pad=cout_pad, cin_pad=cin_pad, **kw))


def _first_diff(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    j = np.nonzero(got != want)[0]
    return "" if not len(j) else "byte %d: 0x%02x, spec 0x%02x (%d differ)" % (j[0], got[j[0]], want[j[0]], len(j))


@pytest.mark.parametrize("case", list(S.MX_WEIGHT_SHAPES))
@pytest.mark.parametrize("storage", ("mx", "split", "f16", "f32"))
def test_pack_weights_writes_the_spec_bytes(storage, case):
    shape = S.MX_WEIGHT_SHAPES[case]
    cout, cin, kh, kw, cout_pad, cin_pad = shape
    w = S.weight_tensor(shape, seed=list(S.MX_WEIGHT_SHAPES).index(case))
    want = S.encode_weight(S.stored_weight_values(w, storage, cout_pad=cout_pad, cin_pad=cin_pad), storage)
    d = _first_diff(_pack(w, storage, cout_pad, cin_pad), want)
    _log("weights", case, storage, shape=list(shape))
    assert not d, d


@pytest.mark.parametrize("storage", ("mx", "split", "f16", "f32"))
def test_pack_weights_rounds_the_fp32_product(storage):
    """fl32(w * scale) first, then the storage's rounding: row maxima whose exact product rounds to a half in the binade BELOW the one its fp32 rounding
    reaches (another row scale in fp16+8, another half everywhere), and -0 products (v_fma_mixlo_f16 of v * scale + 0 stored +0)"""
    cout, cin, kh, kw, cout_pad, cin_pad = S.DR_SHAPE
    w, _ = S.double_rounding_case()
    want = S.encode_weight(S.stored_weight_values(w, storage, scale=S.DR_SCALE, cout_pad=cout_pad, cin_pad=cin_pad), storage)
    d = _first_diff(_pack(w, storage, cout_pad, cin_pad, scale=S.DR_SCALE), want)
    _log("weights", "double_rounding", storage, shape=list(S.DR_SHAPE))
    assert not d, d


@pytest.mark.parametrize("storage", ("split", "f16", "f32"))
def test_pack_weights_second_grid_stride_trip(storage):
    cout, cin, kh, kw = S.BIG_PLAIN_SHAPE
    w = S.weight_tensor(S.BIG_PLAIN_SHAPE, seed=5)
    want = S.encode_weight(S.stored_weight_values(w, storage), storage)
    d = _first_diff(_pack(w, storage, cout, cin), want)
    _log("weights", "second_trip", storage, shape=list(S.BIG_PLAIN_SHAPE))
    assert not d, d


@pytest.mark.parametrize("K", S.SN_K)
@pytest.mark.parametrize("storage", ("mx", "split", "f16", "f32"))
def test_pack_weights_with_the_spectral_norm_fold(storage, K):
    """sigma = fl32 of the fp64 sum (clear of an fp32 rounding boundary by 2^-30: the CPU tier), then fl32(w / sigma) * scale in fp32: byte-exact too"""
    cout, cin, kh, kw, cout_pad, cin_pad = S.SN_SHAPES[K]
    w, u, v, sigma, margin = S.sn_case(K)
    scale = 0.3
    want = S.encode_weight(S.stored_weight_values(w, storage, scale=scale, sigma=np.float32(sigma), cout_pad=cout_pad, cin_pad=cin_pad), storage)
    d = _first_diff(_pack(w, storage, cout_pad, cin_pad, scale=scale, sn_u=_dev(u), sn_v=_dev(v)), want)
    _log("weights", "sn_K%d" % K, storage, shape=list(S.SN_SHAPES[K]), sigma=sigma)
    assert not d, d
