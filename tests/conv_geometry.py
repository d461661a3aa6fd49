"""The geometry contract of mnet_conv2d_nhwc (include/marconet_hip.h) as data: the one formula the header promises for ANY kh, kw, stride and padding,

    y[n,oh,ow,o] = post_scale * act( out_scale * sum_{r,s,i} W[o,r,s,i] * X'[n, oh*sh - ph + r, ow*sw - pw + s, i] + bias + residual )
    out-of-image taps (and INPUT columns >= valid_w[n]) are zero

on the filters, strides and paddings no other test launches.  This file holds the table of geometries, the launch variants per row (a seeded all-pairs
cover), the fp64 reference built from the definition (explicit zero padding, never F.conv2d's own) and what the header says the planner does with
each launch.  No device needed: the CPU tier (test_conv_geometry_table.py) pins the reference to the header formula and the planner to the
expectations, the GPU tier (test_conv_geometry_gpu.py) launches every row on every kernel.  The epilogue side of the formula is covered by
tests/conv_contract.py; its machinery is reused here."""
import math

import torch
import torch.nn.functional as F

from tests import conv_contract as C

# name -> (n, h, w, kh, kw, (sh, sw), (ph, pw), flags).  flags: "m32" ho*wo % 32 == 0 (fp16+8 id 16 must run itself), "same" output of the input's
# size at stride 1 with an odd filter (GroupNorm sums, the folded skip), "big" >= 65536 output pixels (reference over a band of rows)
ROWS = {
    "1x1": (4, 8, 12, 1, 1, (1, 1), (0, 0), ("m32", "same")),            # division decode
    "1x1s2": (4, 8, 16, 1, 1, (2, 2), (0, 0), ("m32",)),                 # unused last row / column
    "1x1pad": (4, 6, 12, 1, 1, (1, 1), (1, 2), ("m32",)),                # outputs with no tap at all
    "3x3valid": (4, 10, 18, 3, 3, (1, 1), (0, 0), ("m32",)),             # no padding tap anywhere
    "3x3full": (4, 6, 14, 3, 3, (1, 1), (2, 2), ("m32",)),               # pad = k - 1
    "3x3beyond": (4, 2, 8, 3, 3, (1, 1), (4, 5), ("m32",)),              # windows wholly outside; map smaller than the filter
    "3x3s12": (4, 8, 16, 3, 3, (1, 2), (1, 1), ("m32",)),                # stride on w only
    "3x3s22a": (4, 8, 17, 3, 3, (2, 2), (1, 0), ("m32",)),               # pad_h != pad_w, (h + 2p - k) % stride != 0
    "3x3s33": (4, 12, 24, 3, 3, (3, 3), (1, 1), ("m32",)),               # stride = filter, with pad
    "1x3": (4, 8, 12, 1, 3, (1, 1), (0, 1), ("m32", "same")),
    "3x1": (4, 8, 12, 3, 1, (1, 1), (1, 0), ("m32", "same")),            # kw = 1 row wrap
    "2x2p1": (4, 7, 15, 2, 2, (1, 1), (1, 1), ("m32",)),                 # even filter
    "2x2s2": (4, 8, 16, 2, 2, (2, 2), (0, 0), ("m32",)),                 # patchify
    "5x5": (4, 8, 12, 5, 5, (1, 1), (2, 2), ("m32", "same")),            # 25 taps
    "5x5s2": (4, 8, 16, 5, 5, (2, 2), (2, 2), ("m32",)),
    "4x8": (4, 9, 17, 4, 8, (1, 1), (1, 3), ("m32",)),                   # 32 taps, tap 31, sh_hi == 32
    "8x4": (4, 7, 19, 8, 4, (1, 1), (4, 0), ("m32",)),                   # kh = 8, rowrep full
    "h1": (4, 1, 32, 3, 3, (1, 1), (1, 1), ("m32", "same")),             # one-row map
    "w1": (4, 32, 1, 3, 3, (1, 1), (1, 1), ("m32", "same")),             # one-column map
    "pad40": (4, 4, 8, 3, 3, (1, 1), (40, 40), ()),                      # 82 x 86: id 16 -> 15; pads far beyond the shift range
    "6x6": (4, 8, 12, 6, 6, (1, 1), (3, 3), ()),                         # 9 x 13: 36 taps, not LDS-DMA eligible
    "8x8s8": (4, 16, 32, 8, 8, (8, 8), (0, 0), ()),                      # 2 x 4: 64 taps, not eligible
    "big1x3": (1, 128, 512, 1, 3, (1, 1), (0, 1), ("m32", "same", "big")),
    "big3x3s2": (1, 256, 1024, 3, 3, (2, 2), (1, 1), ("m32", "big")),
}
OUT = {"1x1": (8, 12), "1x1s2": (4, 8), "1x1pad": (8, 16), "3x3valid": (8, 16), "3x3full": (8, 16), "3x3beyond": (8, 16), "3x3s12": (8, 8),
       "3x3s22a": (4, 8), "3x3s33": (4, 8), "1x3": (8, 12), "3x1": (8, 12), "2x2p1": (8, 16), "2x2s2": (4, 8), "5x5": (8, 12), "5x5s2": (4, 8),
       "4x8": (8, 16), "8x4": (8, 16), "h1": (1, 32), "w1": (32, 1), "pad40": (82, 86), "6x6": (9, 13), "8x8s8": (2, 4), "big1x3": (128, 512),
       "big3x3s2": (128, 512)}          # the output sizes as the issue's table states them (checked against conv_prepare's rule on the CPU tier)


def flag(rname, f):
    return f in ROWS[rname][7]


def out_size(geo):
    n, h, w, kh, kw, (sh, sw), (ph, pw) = geo[:7]
    return (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1


def valid_widths(geo):
    """the ragged level, in INPUT columns; the 0 is deliberate (the header formula defines it)"""
    n, w = geo[0], geo[2]
    return (w, w // 2 + 1, 1, 0)[:n] if n == 4 else (300,)


def ref_rows(rname):
    """output rows the fp64 reference covers: all, or the border rows plus two in the middle on the big maps"""
    ho = out_size(ROWS[rname])[0]
    return [0, 1, ho // 2 - 1, ho // 2, ho - 2, ho - 1] if flag(rname, "big") else list(range(ho))


# ---- channels ------------------------------------------------------------------------------------------------------------------------------
def chan_variants(storage, req, rname):
    """(c0, c1, cout) of the launches of one (storage, request, row)"""
    if rname == "big1x3":
        return [(64, 64, 64), (64, 64, 256)]
    if rname == "big3x3s2":
        return [(64, 64, 256)]
    out = [(64, 64, 96)]
    if req == "reg":
        out.append((8, 16, 12) if storage in ("f32", "f16") else (32, 32, 32))
    return out


def uses_row(storage, req, rname):
    """the big maps go to auto, reg, the strip requests (which must refuse them) and the big-tile ids"""
    if not flag(rname, "big"):
        return True
    return req in ("auto", "reg") or req.startswith("strip") or C.uses_shape(req, "big64")


# ---- launch variants -----------------------------------------------------------------------------------------------------------------------
G_NAMES = ("epi", "valid_w", "src2", "extra")


def g_levels(storage, req, rname):
    family = C.requests(storage)[req][1]
    src2 = ("none", "concat")
    if flag(rname, "same") and storage != "f32" and family in ("dma", "dma_nogn", "all"):
        src2 += ("center",)
    extra = ("none",)
    if storage == "mx" and flag(rname, "same") and family in ("dma", "strip", "all"):
        extra += ("gn",)
    if req == "reg":
        extra += ("affine", "swish")
    return {"epi": ("bare", "loaded"), "valid_w": ("none", "ragged"), "src2": src2, "extra": extra}


def to_row(g):
    """a geometry variant as a row of the epilogue contract (tests/conv_contract.py): the keys its machinery reads"""
    r = {f: C.FACTORS[f][0] for f in C.NAMES}
    if g["epi"] == "loaded":
        r.update(out_scale="pos", bias="yes", residual="full", act=3)
    r.update(valid_w=g["valid_w"], src2=g["src2"])
    if g["extra"] == "gn":
        r["gn"] = "on"
    elif g["extra"] != "none":
        r["xform"] = g["extra"]
    return r


_BIG = {("big1x3", 64): dict(epi="loaded", valid_w="ragged", src2="none", extra="none"),
        ("big1x3", 256): dict(epi="bare", valid_w="none", src2="center", extra="none"),
        ("big3x3s2", 256): dict(epi="bare", valid_w="ragged", src2="concat", extra="none")}


def variants(storage, req, rname, chans):
    """[(name, epilogue-contract row)]: the seeded all-pairs cover of the row's levels; ONE fixed launch on the big maps"""
    lv = g_levels(storage, req, rname)
    if flag(rname, "big"):
        g = dict(_BIG[(rname, chans[2])])
        if g["src2"] not in lv["src2"]:
            g["src2"] = "concat"
        return [("big", to_row(g))]
    seed = 7 + list(ROWS).index(rname)
    return [("v%02d" % i, to_row(g)) for i, g in enumerate(C.all_pairs(lv, seed, G_NAMES))]


def launches(storage, req):
    """every (row name, channels, variant name, row) the request is asked for"""
    return [(rname, ch, vname, row) for rname in ROWS if uses_row(storage, req, rname) for ch in chan_variants(storage, req, rname)
            for vname, row in variants(storage, req, rname, ch)]


# ---- the planner as the header states it ---------------------------------------------------------------------------------------------------
def expected(storage, req, rname, chans, row):
    """(kind, LDS-DMA id or None) the header (marconet_hip.h) gives this launch: kind 'refused', 'reg', 'skinny', 'strip' or 'dma'.  id None:
    AUTO's choice of tile (any LDS-DMA id; the hand-overs still hold)"""
    n, h, w, kh, kw, (sh, sw), (ph, pw) = ROWS[rname][:7]
    ho, wo = out_size(ROWS[rname])
    c0, c1, cout = chans
    two, center = row["src2"] != "none", row["src2"] == "center"
    cin = c0 + (c1 if two else 0)
    xf, gn, act = row["xform"] != "none", row["gn"] == "on", row["act"]
    blocked = storage in ("split", "mx")
    # gn_partial only 'same'-size stride-1 fp16+8 (cout % 32 == 0, ho*wo % 32 == 0)
    if gn and not (storage == "mx" and (sh, sw) == (1, 1) and (ho, wo) == (h, w) and cout % 32 == 0 and (ho * wo) % 32 == 0):
        return ("refused", None)
    cmul = 32 if blocked else 64
    # LDS-DMA eligible iff the channel rules hold and kh*kw <= 32 and kh, kw <= 8 (no input transform, act <= LRELU_SQRT2)
    dma_ok = (storage != "f32" and not xf and act <= 3 and cin % cmul == 0 and c0 % cmul == 0 and cout >= 64 and cout % (32 if blocked else 8) == 0
              and kh * kw <= 32 and kh <= 8 and kw <= 8)
    # the folded skip: odd filter, 'same' padding, stride 1, a half-range dtype, whole k-slabs, on the LDS-DMA kernel only
    if center:
        ok = (two and kh % 2 == 1 and kw % 2 == 1 and (sh, sw) == (1, 1) and (ph, pw) == (kh // 2, kw // 2) and storage != "f32"
              and c0 % cmul == 0 and c1 % cmul == 0 and dma_ok and (req == "auto" or req.startswith("dma")))
        if not ok:
            return ("refused", None)
    # the strip kernel: 3x3 / stride 1 / pad 1 on >= 65536 pixels, one source
    strip_ok = dma_ok and (kh, kw, sh, sw, ph, pw) == (3, 3, 1, 1, 1, 1) and not two and n * ho * wo >= 65536
    # the skinny kernel: fp32 1x1 / stride 1 / pad 0, one source, no valid_w, no input transform, <= 512 pixels
    skinny_ok = (storage == "f32" and (kh, kw, sh, sw, ph, pw) == (1, 1, 1, 1, 0, 0) and not two and not xf and row["valid_w"] == "none"
                 and cin % 16 == 0 and n * ho * wo <= 512)
    if req.startswith("strip"):
        return ("strip", None) if strip_ok else ("refused", None)       # (no row of the table is strip eligible)
    if req == "skinny":
        return ("skinny", None) if skinny_ok else ("refused", None)
    if req == "reg":
        return ("refused", None) if gn else ("reg", None)
    if req.startswith("dma"):
        if not dma_ok:
            return ("refused", None)
        id_ = int(req[3:])
        if storage == "mx" and id_ == 16 and ((ho * wo) % 32 or act not in C.MX_HANDOVER_ACTS):
            id_ = 15
        if storage == "mx" and id_ == 9 and gn:
            id_ = 8
        return ("dma", id_)
    assert req == "auto"
    if skinny_ok:
        return ("skinny", None)
    if strip_ok:
        return ("strip", None)
    if dma_ok:
        return ("dma", None)
    return ("refused", None) if gn else ("reg", None)


def plan_mismatch(storage, exp, k, rname):
    """what in mnet_conv2d_plan's answer k contradicts the expectation; None when nothing does"""
    kind, id_ = exp
    if kind == "refused":
        return None if k < 0 else "the header refuses it, the planner answers %d" % k
    if k < 0:
        return "the header gives it to the %s kernel, the planner refuses it (%d)" % (kind, k)
    if kind == "reg":
        return None if k == C.ALGO_REG else "header: register-staged, planner: %d" % k
    if kind == "skinny":
        return None if k == C.ALGO_SKINNY else "header: skinny, planner: %d" % k
    if kind == "strip":
        return None if C.is_strip(k) else "header: strip, planner: %d" % k
    if not C.is_dma(k):
        return "header: an LDS-DMA tile, planner: %d" % k
    if id_ is not None and k != C.dma(id_):
        return "header: LDS-DMA id %d, planner: %d" % (id_, k)
    ho, wo = out_size(ROWS[rname])
    if storage == "mx" and k == C.dma(16) and (ho * wo) % 32:
        return "fp16+8 id 16 on ho*wo = %d" % (ho * wo)
    return None


# ---- operands and the fp64 reference -------------------------------------------------------------------------------------------------------
class _H:
    """the epilogue contract's helpers (imported on first use: their modules import the packers)"""
    _names = None

    def __getattr__(self, name):
        if _H._names is None:
            from tests.test_conv_epilogue_contract_gpu import DTYPES, _act, _split_q
            from tests.test_kernels_gpu import _q, _rnd
            from tests.test_mx_gpu import _emulate, _wdec
            _H._names = dict(DTYPES=DTYPES, act=_act, split_q=_split_q, q=_q, rnd=_rnd, emulate=_emulate, wdec=_wdec)
        return _H._names[name]


H = _H()


def live_mask(geo, vw=None):
    """[n, ho, wo] bool: the output's window holds at least one tap inside the image and left of valid_w"""
    n, h, w, kh, kw, (sh, sw), (ph, pw) = geo[:7]
    ho, wo = out_size(geo)
    ih0, iw0 = torch.arange(ho) * sh - ph, torch.arange(wo) * sw - pw
    rows = (torch.minimum(ih0 + kh, torch.tensor(h)) > torch.clamp(ih0, min=0))
    lim = torch.tensor([w] * n if vw is None else [min(v, w) for v in vw])
    cols = torch.minimum(iw0[None, :] + kw, lim[:, None]) > torch.clamp(iw0, min=0)[None, :]
    return rows[None, :, None] & cols[:, None, :]


def explicit_conv(x, geo, vw, rows, conv):
    """the definition: zero the columns >= valid_w, zero-pad the input explicitly — (pw, pw + sw) columns, (ph, ph + sh) rows — convolve with
    padding 0 and crop to ho x wo.  ``conv(xp, stride)`` does the arithmetic (fp64 by default, the fp32 / fp16+8 emulations of the CPU tier);
    ``rows``: the output rows wanted, each from its own band of kh padded input rows.  Returns [n, cout, len(rows), wo]."""
    n, h, w, kh, kw, (sh, sw), (ph, pw) = geo[:7]
    ho, wo = out_size(geo)
    if vw is not None:
        x = x.clone()
        for i, v in enumerate(vw):
            x[i, :, :, v:] = 0
    xp = F.pad(x, (pw, pw + sw, ph, ph + sh))
    if rows == list(range(ho)):
        return conv(xp, (sh, sw))[:, :, :ho, :wo]
    return torch.cat([conv(xp[:, :, oh * sh:oh * sh + kh], (1, sw))[:, :, :1, :wo] for oh in rows], dim=2)


class Operands:
    """the operands of one (storage, row, channels): decoded stored values on the host, and the fp64 reference of a launch variant.  Seeds depend on
    the row and the channels only, so every tier and every request sees the same numbers."""

    def __init__(self, storage, rname, chans):
        self.storage, self.rname, self.chans, self.geo, self.dt = storage, rname, chans, ROWS[rname], H.DTYPES[storage]
        n, h, w, kh, kw, (sh, sw), (ph, pw) = self.geo[:7]
        c0, c1, cout = chans
        self.ho, self.wo = out_size(self.geo)
        self.rows = ref_rows(rname)
        self.big = flag(rname, "big")
        seed = 5000 + 101 * list(ROWS).index(rname) + chans[2]
        self.x_raw = H.rnd((n, c0 + c1, h, w), seed)                            # before storage rounding (the device side packs this)
        if self.big:                                                           # decode only the input rows the reference rows read
            need = sorted({ih for oh in self.rows for ih in range(oh * sh - ph, oh * sh - ph + kh) if 0 <= ih < h})
            self.x = torch.zeros_like(self.x_raw)
            self.x[:, :, need] = torch.cat([H.q(self.x_raw[:, :c0, need].contiguous(), self.dt), H.q(self.x_raw[:, c0:, need].contiguous(), self.dt)], dim=1)
        else:
            self.x = torch.cat([H.q(self.x_raw[:, :c0].contiguous(), self.dt), H.q(self.x_raw[:, c0:].contiguous(), self.dt)], dim=1)
        self.wt = H.rnd((cout, c0 + c1, kh, kw), seed + 1, 1.0 / math.sqrt((c0 + c1) * kh * kw))
        if self.dt == torch.float16:
            self.wt = self.wt.half().float()
        self.out_scale = H.rnd((n, cout), seed + 2).abs() + 0.5
        self.bias = H.rnd((cout,), seed + 6, 0.3)
        self.res_raw = H.rnd((n, cout, self.ho, self.wo), seed + 7)
        self.res = torch.zeros_like(self.res_raw)
        self.res[:, :, self.rows] = H.q(self.res_raw[:, :, self.rows].contiguous(), self.dt)
        self.in_scale = H.rnd((n, c0 + c1), seed + 10).abs() + 0.5
        self.in_shift = H.rnd((n, c0 + c1), seed + 11, 0.2)
        self.vws = valid_widths(self.geo)
        self.convs = {}

    def xprime(self, row):
        """X' of the variant before the valid-width mask: the channels used and the input transform, rounded to the storage as the kernel stages it"""
        c_used = self.chans[0] + (self.chans[1] if row["src2"] != "none" else 0)
        x = self.x[:, :c_used]
        if row["xform"] != "none":
            x = x * self.in_scale[:, :c_used, None, None] + self.in_shift[:, :c_used, None, None]
            if row["xform"] == "swish":
                x = x * torch.sigmoid(x)
            x = x if self.storage == "f32" else x.half().float() if self.storage == "f16" else H.split_q(x)
        return x

    def weights(self, row, kind):
        """kind 'dec': the values the kernel multiplies with; 'true': the unrounded weights (the fp16+8 LDS-DMA kernels vs fp64 and the emulation)"""
        c0 = self.chans[0]
        w = self.wt if row["src2"] != "none" else self.wt[:, :c0].contiguous()
        if kind == "dec":
            w = {"split": lambda t: H.split_q(t * 256.0) / 256.0, "mx": H.wdec}.get(self.storage, lambda t: t)(w)
        if row["src2"] == "center":              # x1 enters at the centre tap (kh/2, kw/2) only
            m = torch.zeros_like(w)
            m[:, :c0] = 1.0
            m[:, c0:, self.geo[3] // 2, self.geo[4] // 2] = 1.0
            w = w * m
        return w

    def conv(self, row, kind):
        """the sum of the header formula over the reference rows: fp64 ('dec' / 'true' weights), 'emu' the fp16+8 three-product emulation, 'f32' an
        fp32 convolution of the stored operands (the CPU tier's headroom check)"""
        key = (row["src2"], row["xform"], row["valid_w"], kind)
        if key not in self.convs:
            wt = self.weights(row, "true" if kind == "emu" else "dec" if kind == "f32" else kind)
            if kind == "emu":
                f = lambda xp, stride: H.emulate(xp, wt, stride=stride, padding=0).double()
            elif kind == "f32":
                f = lambda xp, stride: F.conv2d(xp, wt, stride=stride).double()
            else:
                f = lambda xp, stride: F.conv2d(xp.double(), wt.double(), stride=stride)
            self.convs[key] = explicit_conv(self.xprime(row), self.geo, self.vws if row["valid_w"] != "none" else None, self.rows, f)
        return self.convs[key]

    def epilogue(self, row, v):
        """the output side of the header formula on a sum v [n, cout, len(rows), wo], fp64"""
        if row["out_scale"] != "none":
            v = v * self.out_scale.double()[:, :, None, None]
        if row["bias"] != "none":
            v = v + self.bias.double()[None, :, None, None]
        if row["residual"] != "none":
            v = v + self.res[:, :, self.rows].double()
        return H.act(v, row["act"])

    def reference(self, row, kind):
        return self.epilogue(row, self.conv(row, kind))


def four_loops(op, row):
    """the header formula written out: loops over n, oh, ow and the taps (r, s); the sums over i, for every o, are one fp64 matrix-vector product"""
    n, h, w, kh, kw, (sh, sw), (ph, pw) = op.geo[:7]
    x, wt = op.xprime(row).double(), op.weights(row, "dec").double()
    vws = op.vws if row["valid_w"] != "none" else (w,) * n
    y = torch.zeros(n, wt.shape[0], op.ho, op.wo, dtype=torch.float64)
    for i in range(n):
        for oh in range(op.ho):
            for ow in range(op.wo):
                for r in range(kh):
                    for s in range(kw):
                        ih, iw = oh * sh - ph + r, ow * sw - pw + s
                        if 0 <= ih < h and 0 <= iw < min(vws[i], w):
                            y[i, :, oh, ow] += wt[:, :, r, s] @ x[i, :, ih, iw]
    return op.epilogue(row, y)


_OPS = {}


def operands(storage, rname, chans):
    key = (storage, rname, chans)
    if key not in _OPS:
        if flag(rname, "big"):                       # one big map at a time (hundreds of MB of host memory each)
            for k in [k for k in _OPS if flag(k[1], "big")]:
                del _OPS[k]
        _OPS[key] = Operands(storage, rname, chans)
    return _OPS[key]


# ---- split-K -------------------------------------------------------------------------------------------------------------------------------
# mnet_conv2d_splitk (fp32 patchify: filter == stride, no padding): (h, w, c, kh, kw, cout, the two ksplit values the header allows — multiples of kh whose
# slices of one filter row kw*c are whole 16-float steps).  Every map has an unused last row / column.
SPLITK = {"2x2": (9, 17, 32, 2, 2, 36, (2, 8)), "4x8": (9, 33, 8, 4, 8, 36, (4, 16)), "8x4": (17, 9, 16, 8, 4, 36, (8, 32))}
SPLITK_REFUSED_KSPLIT = ("4x8", 32)                  # 64 floats per filter row in 8 slices: 8-float slices
