"""Where in memory an element lies, as data: the launches of tests/test_large_tensors_gpu.py, whose tensors hold more than 2^31 elements and more than
2^32 bytes, with the wrap points each tensor crosses, the image slots that are probed and the memory each launch needs.  No device needed: the CPU
tier (tests/test_large_tensors.py) checks that every row crosses what it claims.

Wrap points of a tensor with s bytes per logical element (2 for f16; 4 for fp32, split half and fp16+8), as ELEMENT offsets:
    W1  byte offset 2^31     2^31 / s        W2  byte offset 2^32     2^32 / s        W3  element offset 2^31     2^31
The per-image element count E = 96 * 512 * 64 = 3 * 2^20 divides none of them, so each wrap point lies strictly inside an image (inside a row run and
inside a pixel tile); the same E as 96 x 256 x 128 and 96 x 128 x 256 serves the 128- and 256-channel launches, and all three keep ho * wo % 32 == 0 and
the strip kernels' whole-row tiling.  N = 685 images put two whole images beyond W3: 8.03 GiB at s = 4, 4.01 GiB at s = 2.

Probe slots of a launch: per tensor, image 0, the image that holds each wrap point of that tensor with its two neighbours, and the last image; the
launch's set is the union over its tensors.  Every other slot holds one filler image."""

STORAGES = ("f32", "f16", "split", "mx")
S_BYTES = {"f32": 4, "f16": 2, "split": 4, "mx": 4}
E = 96 * 512 * 64
N = 685
SHAPES = {64: (96, 512, 64), 128: (96, 256, 128), 256: (96, 128, 256)}       # (h, w, c): E elements each
SMALL = (12, 16, 64)                                                        # the many-small-images rows: a 512-pixel tile touches four images
N_SMALL = 174800                                                            # 174800 * 12288 elements > 2^31; n_first * img0 passes 2^32 bytes
GIB = 1 << 30
LIMIT = 32 * GIB


def wrap_points(s):
    return {"W1": (1 << 31) // s, "W2": (1 << 32) // s, "W3": 1 << 31}


def crossed(n, e, s):
    """names of the wrap points that lie inside a tensor of n images of e elements"""
    return tuple(k for k, off in sorted(wrap_points(s).items()) if off < n * e)


def wrap_images(n, e, s):
    """{wrap point: (image that holds it, element offset inside that image)} for the wrap points the tensor crosses"""
    return {k: (off // e, off % e) for k, off in wrap_points(s).items() if off < n * e}


def tensor_slots(n, e, s):
    out = {0, n - 1}
    for img, _ in wrap_images(n, e, s).values():
        out.update(i for i in (img - 1, img, img + 1) if 0 <= i < n)
    return out


def probe_slots(tensors):
    """tensors: {name: (n, elements per image, bytes per element)} of one launch, all with the same n"""
    out = set()
    for n, e, s in tensors.values():
        out |= tensor_slots(n, e, s)
    return sorted(out)


def first_wrapped_image(n, e, s, product, per_image_base=False):
    """the image in which a 32-bit form of an address product first goes wrong, or None if the tensor is too small for it to.  product: 'int bytes'
    (a signed 32-bit byte offset: W1), 'unsigned bytes' (W2) or 'int elements' (W3).  per_image_base: the product is the image's base n * e (the first
    image whose base lies at or beyond the limit) instead of an element's own offset (the image that holds the limit)"""
    limit = wrap_points(s)[{"int bytes": "W1", "unsigned bytes": "W2", "int elements": "W3"}[product]]
    img = -(-limit // e) if per_image_base else limit // e
    return img if img < n else None


def need_bytes(tensors):
    return sum(n * e * s for n, e, s in tensors.values())


# ---- conv rows -----------------------------------------------------------------------------------------------------------------------------
# name -> dict(storage, req, C, extra).  req: "reg", "auto", "strip1", "dmaK".  3x3 / stride 1 / pad 1, cin = cout = C, bias + residual + act 3 unless
# `extra` says otherwise.  Ids without a build for a storage are absent: split half has no ids 13 / 15 / 16, f16 no id 15 with correct results
# (ids 11-15 are diagnostic builds there), fp32 has the register-staged kernel only.
CONV = {
    "f32-reg-64": dict(storage="f32", req="reg", C=64),
    "f16-reg-64": dict(storage="f16", req="reg", C=64),
    "f16-auto-64": dict(storage="f16", req="auto", C=64),
    "f16-strip1-64": dict(storage="f16", req="strip1", C=64),
    "f16-dma9-128": dict(storage="f16", req="dma9", C=128),
    "f16-dma16-256": dict(storage="f16", req="dma16", C=256),
    "split-auto-64": dict(storage="split", req="auto", C=64),
    "split-strip1-64": dict(storage="split", req="strip1", C=64),
    "split-dma9-128": dict(storage="split", req="dma9", C=128),
    "split-dma11-256": dict(storage="split", req="dma11", C=256),
    "mx-dma13-64": dict(storage="mx", req="dma13", C=64),
    "mx-strip1-64": dict(storage="mx", req="strip1", C=64),
    "mx-dma8-128": dict(storage="mx", req="dma8", C=128),
    "mx-dma15-256-gn": dict(storage="mx", req="dma15", C=256, extra="gn"),
    "mx-dma16-256-gn": dict(storage="mx", req="dma16", C=256, extra="gn"),
    "mx-dma16-256-two": dict(storage="mx", req="dma16", C=256, extra="two"),          # c0 = c1 = 128: x0, x1 hold E / 2 per image (W1, W2 only)
    "mx-dma16-256-center": dict(storage="mx", req="dma16", C=256, extra="center"),    # the same, x1 at the centre tap
    "mx-shuffle2": dict(storage="mx", req="auto", C=64, extra="shuffle2"),            # x [n,48,256,64] (E / 4: W1 only) -> cout 256 -> y [n,96,512,64]
    "mx-f32out": dict(storage="mx", req="auto", C=64, extra="f32out"),                # y plain fp32; no bias / residual / act
    "f16-small": dict(storage="f16", req="auto", C=64, extra="small"),
    "split-small": dict(storage="split", req="auto", C=64, extra="small"),
    "mx-small": dict(storage="mx", req="auto", C=64, extra="small"),
}


def conv_geometry(name):
    """(n, h, w, c0, c1, cout, y image shape) of a conv row"""
    r = CONV[name]
    ex = r.get("extra")
    if ex == "small":
        h, w, c = SMALL
        return N_SMALL, h, w, c, 0, c, (h, w, c)
    h, w, c = SHAPES[r["C"]]
    if ex in ("two", "center"):
        return N, h, w, c // 2, c // 2, c, (h, w, c)
    if ex == "shuffle2":
        return N, h // 2, w // 2, c, 0, 4 * c, (h, w, c)
    return N, h, w, c, 0, c, (h, w, c)


def conv_tensors(name):
    r = CONV[name]
    s = S_BYTES[r["storage"]]
    n, h, w, c0, c1, cout, (yh, yw, yc) = conv_geometry(name)
    t = {"x0": (n, h * w * c0, s), "y": (n, yh * yw * yc, s)}
    if c1:
        t["x1"] = (n, h * w * c1, s)
    if r.get("extra") not in ("shuffle2", "f32out"):
        t["residual"] = (n, yh * yw * yc, s)
    return t


# what each conv row claims to cross, per tensor (checked on the CPU tier against the arithmetic above)
def conv_claims(name):
    r = CONV[name]
    ex, four = r.get("extra"), S_BYTES[r["storage"]] == 4
    full = ("W1", "W2", "W3") if four else ("W2", "W3")            # s = 2: W1 and W3 are the same offset, named W3
    if ex == "small":
        return {k: full for k in ("x0", "y", "residual")}
    c = {"x0": full, "y": full, "residual": full}
    if ex in ("two", "center"):
        c.update(x0=("W1", "W2"), x1=("W1", "W2"))
    if ex == "shuffle2":
        c = {"x0": ("W1",), "y": full}
    if ex == "f32out":
        c = {"x0": full, "y": full}
    return c


# ---- streaming rows ------------------------------------------------------------------------------------------------------------------------
# name -> {tensor: (n, elements per image, bytes per element)}; every big tensor crosses every wrap point of its element size unless the comment says otherwise
def _t(e, st, n=N):
    return (n, e, S_BYTES[st])


STREAM = {}
for _st in STORAGES:
    if _st != "f32":
        STREAM["convert-from-" + _st] = {"src": _t(E, _st), "dst": _t(E, "f32")}
        STREAM["convert-to-" + _st] = {"src": _t(E, "f32"), "dst": _t(E, _st)}
    STREAM["upsample2x-" + _st] = {"src": _t(E // 4, _st), "dst": _t(E, _st)}                    # src: W1 only at s = 4, none at s = 2
    STREAM["upsample2x-scale-" + _st] = {"src": _t(E // 4, _st), "dst": _t(E, _st)}
    if _st in ("split", "mx"):
        STREAM["upsample2x-tof16-" + _st] = {"src": _t(E // 4, _st), "dst": _t(E, "f16")}
    STREAM["affine_act-" + _st] = {"x": _t(E, _st), "y": _t(E, _st)}
    STREAM["affine_act-inplace-" + _st] = {"x": _t(E, _st)}
    STREAM["groupnorm_affine-" + _st] = {"x": _t(E, _st)}
    STREAM["nchw_to_nhwc-" + _st] = {"src": _t(E, "f32"), "dst": _t(E, _st)}
    STREAM["nhwc_to_nchw-" + _st] = {"src": _t(E, _st), "dst": _t(E, "f32")}
    STREAM["torgb-" + _st] = {"x": _t(E, _st), "out": _t(96 * 512 * 4, "f32")}                   # big input, small output
    STREAM["conv3x3_rgb-" + _st] = {"x": _t(E, _st), "y_nchw": _t(3 * 96 * 512, "f32")}
for _st in ("f32", "f16"):
    STREAM["nonfinite_flag-" + _st] = {"x": _t(E, _st)}
    STREAM["sr_postprocess-" + _st] = {"src": _t(E, _st), "dst": (N, 96 * 512 * 8 * 3, 1)}       # [n,96,512*8 pixels][c_ld = 8] -> uint8 BGR
for _st in ("f16", "mx", "split", "f32"):
    STREAM["compare_stats-" + _st] = {"mode": _t(E, _st), "ref": _t(E, "f32")}
# the fold: y [n,96,512,64] from z [n,48,256,9*64] (9/4 E per image: 18.1 GiB at 4 bytes, itself past element offset 2^32)
for _st in STORAGES:
    STREAM["upfold3x3-" + _st] = {"z": _t(9 * E // 4, _st), "y": _t(E, _st)}
STREAM["upfold3x3_f32z"] = {"z": _t(9 * E // 4, "f32"), "y": _t(E, "mx")}
# the glyph kernels: one glyph per slot.  S = 48 (no power of two, so that no wrap point falls on a glyph boundary), C = 64, feature width 64.
GLYPH_S, GLYPH_C, GLYPH_FW = 48, 64, 64
G_ADAIN = 7290               # out [G,48,48,128]: 7290 * 294912 elements > 2^31; G <= 65535, so the split form takes it too and prior / feat cross what they can
B_SCATTER = 10930            # feat / out [B,48,64,64]: 10930 * 196608 elements > 2^31; scale / shift [G = B,48,48,64]
for _st in STORAGES:
    _ad = {"prior": _t(GLYPH_S * GLYPH_S * GLYPH_C, _st, G_ADAIN), "feat": _t(GLYPH_S * GLYPH_FW * GLYPH_C, _st, G_ADAIN),
           "out": _t(GLYPH_S * GLYPH_S * 2 * GLYPH_C, _st, G_ADAIN)}
    for _form in ("adain_crop_concat", "adain_crop_concat_gn", "adain_crop_concat_gn_split"):
        STREAM["%s-%s" % (_form, _st)] = dict(_ad)
    STREAM["glyph_scatter_affine-" + _st] = {"feat": _t(GLYPH_S * GLYPH_FW * GLYPH_C, _st, B_SCATTER), "scale": _t(GLYPH_S * GLYPH_S * GLYPH_C, _st, B_SCATTER),
                                             "shift": _t(GLYPH_S * GLYPH_S * GLYPH_C, _st, B_SCATTER), "out": _t(GLYPH_S * GLYPH_FW * GLYPH_C, _st, B_SCATTER)}
del _st, _ad, _form


def rows():
    """every launch of the GPU tier: name -> its tensors"""
    out = {"conv/" + k: conv_tensors(k) for k in CONV}
    out.update({"stream/" + k: v for k, v in STREAM.items()})
    return out


# ---- the largest maps the LDS-DMA kernels take (n = 2, a tile straddles the two images) ---------------------------------------------------
def dma_limit_ok(h, w, phys_halves):
    """the header's address-range conditions for a map of more than 512 pixels (two images per tile)"""
    return 2 * h * w < (1 << 23) and 2 * h * w * phys_halves * 2 < (1 << 31) - 1


# storage, c0 -> (h, w) of the largest eligible map with h * w % 512 != 0, and a map one row past the limit
LARGEST = {
    ("mx", 64): dict(phys=128, ok=(2049, 2047), past=(2050, 2047)),          # 2049 * 2047 = 2^22 - 1: both bounds together
    ("mx", 96): dict(phys=192, ok=(1366, 2047), past=(1367, 2047)),          # 2796202 = floor((2^31 - 2) / 768): the 31-bit bound alone
    ("f16", 64): dict(phys=64, ok=(2049, 2047), past=(2050, 2047)),          # the 24-bit bound alone
}
