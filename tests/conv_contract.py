"""The epilogue contract of mnet_conv2d_nhwc (include/marconet_hip.h, mnet_conv_desc) as data: the factors a launch can vary, an all-pairs table
over them per kernel family, the small shapes that reach the tiles' tails, and the planner rules the header states.  No device needed: the CPU
tier (test_conv_epilogue_table.py) checks the table and the planner against these rules, the GPU tier (test_conv_epilogue_contract_gpu.py)
launches every row on every kernel and compares it with an fp64 evaluation of the header formula."""
import itertools
import random

# factor -> levels (the first level is "term absent")
FACTORS = {
    "out_scale": ("none", "pos", "signed"),          # signed: exact zeros and one all-negative column
    "bias": ("none", "yes"),
    "residual": ("none", "full", "mod_img", "mod_div"),   # mod_img: res_mod = ho*wo (one image shared by the batch); mod_div: res_mod = wo
    "act": (0, 1, 2, 3, 4, 5, 6),
    "post_scale": ("none", "pos", "signed"),
    "valid_w": ("none", "ragged"),
    "gn": ("off", "on"),
    "src2": ("none", "concat", "center"),
    "xform": ("none", "affine", "swish"),
}
NAMES = tuple(FACTORS)

# the levels each kernel family accepts (a family's own term pairs are covered by its own table)
FAMILY_LEVELS = {
    "reg": dict(gn=("off",), src2=("none", "concat")),                                  # register-staged (and AUTO on a launch it takes)
    "dma": dict(act=(0, 1, 2, 3), xform=("none",)),                                     # LDS-DMA tile ids, fp16+8 (GroupNorm sums)
    "dma_nogn": dict(act=(0, 1, 2, 3), xform=("none",), gn=("off",)),                   # LDS-DMA tile ids, f16 / split-half
    "strip": dict(act=(0, 1, 2, 3), xform=("none",), src2=("none",)),                   # strip kernel, fp16+8
    "strip_nogn": dict(act=(0, 1, 2, 3), xform=("none",), src2=("none",), gn=("off",)),
    "skinny": dict(gn=("off",), src2=("none",), xform=("none",), valid_w=("none",)),
    "all": dict(),                                                                      # AUTO: every level (the planner picks the kernel)
}


def family_levels(family):
    lv = dict(FACTORS)
    lv.update(FAMILY_LEVELS[family])
    return lv


def _pairs(levels, names=NAMES):
    return {((a, la), (b, lb)) for a, b in itertools.combinations(names, 2) for la in levels[a] for lb in levels[b]}


def row_pairs(row, names=NAMES):
    return {((a, row[a]), (b, row[b])) for a, b in itertools.combinations(names, 2)}


def all_pairs(levels, seed=0, names=NAMES):
    """greedy all-pairs cover: every new row starts from the first uncovered pair and fills the other factors, in a seeded order, with the level that
    covers the most still-uncovered pairs (ties: the seeded generator).  Deterministic for a given seed.  ``names``: the factors, in order (the
    epilogue contract's by default; tests/conv_geometry.py passes its own)."""
    rng = random.Random(seed)
    todo = _pairs(levels, names)
    rows = []
    while todo:
        (a, la), (b, lb) = min(todo, key=repr)
        row = {a: la, b: lb}
        rest = [f for f in names if f not in row]
        rng.shuffle(rest)
        for f in rest:
            def gain(lv):
                return sum(((g, row[g]), (f, lv)) in todo or ((f, lv), (g, row[g])) in todo for g in row)
            best = max(gain(lv) for lv in levels[f])
            row[f] = rng.choice([lv for lv in levels[f] if gain(lv) == best])
        row = {f: row[f] for f in names}
        todo -= row_pairs(row, names)
        rows.append(row)
    return rows


def _row(**kw):
    r = {f: FACTORS[f][0] for f in NAMES}
    r.update(kw)
    return r


# rows every family runs whatever its table: all terms off, all on, each of the four builds of the one-wave tile (fp16+8 id 16: SC = out_scale or
# post_scale, RG = residual or GroupNorm sums), and the signed-zero row (a negative out_scale on an all-zero accumulator, no bias to add)
FORCED = {
    "all_off": _row(),
    "all_on": _row(out_scale="signed", bias="yes", residual="full", act=3, post_scale="signed", valid_w="ragged", gn="on", src2="concat"),
    "w4_plain": _row(bias="yes", act=2),
    "w4_sc": _row(out_scale="signed", post_scale="pos", bias="yes", act=3),
    "w4_rg": _row(residual="mod_img", bias="yes", act=2, valid_w="ragged"),
    "w4_sc_rg_res": _row(out_scale="signed", residual="full", act=3),
    "w4_sc_rg_gn": _row(post_scale="signed", gn="on", act=2, valid_w="ragged"),
    "w4_sc_rg_res_gn": _row(out_scale="pos", residual="mod_div", gn="on", bias="yes", act=0),
    "signed_zero": _row(out_scale="signed", valid_w="ragged"),
}

# the rows outside a family's levels: each is run once (the planner refuses it or hands it to another kernel; either way the launch must agree)
PROBES = {
    "probe_xform": _row(xform="swish", bias="yes", act=2),
    "probe_act_tanh": _row(act=4, bias="yes"),
    "probe_act_gelu": _row(act=5, out_scale="pos"),
    "probe_gn": _row(gn="on", act=2),
    "probe_center": _row(src2="center", bias="yes"),
    "probe_concat": _row(src2="concat"),
    "probe_valid_w": _row(valid_w="ragged"),
}


def table(family, seed=0):
    """(name, row) list of a family: its all-pairs table, the forced rows and the probes"""
    out = [("pair%02d" % i, r) for i, r in enumerate(all_pairs(family_levels(family), seed))]
    out += list(FORCED.items()) + list(PROBES.items())
    return out


# ---- shapes --------------------------------------------------------------------------------------------------------------------------------
# name -> (n, h, w, c0, c1 when a second source is used, cout, k, stride, pad, valid widths of the ragged level, big)
SHAPES = {
    "s8x24": (3, 8, 24, 64, 64, 288, 3, (1, 1), 1, (24, 13, 1), False),   # ho*wo % 32 == 0, cout tail, two 256-channel tiles
    "s10x10": (2, 10, 10, 64, 64, 64, 3, (1, 1), 1, (10, 1), False),       # 100 pixels: the one-wave tile hands over, no GroupNorm sums
    "s_stride21": (2, 8, 16, 64, 64, 64, 3, (2, 1), 1, (16, 5), False),     # stride (2, 1): no GroupNorm sums, no folded skip
    "s1x1": (2, 8, 16, 64, 64, 128, 1, (1, 1), 0, (16, 1), False),         # 1x1
    "big64": (1, 128, 512, 64, 64, 64, 3, (1, 1), 1, (300,), True),        # >= 65536 pixels: strip 64x512, AUTO's big tiles
    "big256": (1, 128, 512, 64, 64, 256, 3, (1, 1), 1, (300,), True),      # >= 65536 pixels, cout 256: one-wave tile (AUTO), strip 256x256
}


def out_size(shape):
    n, h, w, c0, c1, cout, k, stride, pad, vws, big = shape
    return (h + 2 * pad - k) // stride[0] + 1, (w + 2 * pad - k) // stride[1] + 1


def res_mod(row, shape):
    ho, wo = out_size(shape)
    return {"none": 0, "full": 0, "mod_img": ho * wo, "mod_div": wo}[row["residual"]]


# ---- kernel requests -----------------------------------------------------------------------------------------------------------------------
ALGO_AUTO, ALGO_REG, ALGO_SKINNY, ALGO_DMA_CFG0, ALGO_STRIP_CFG0, ALGO_DMA_CFG16, FLAG_X1_CENTER = 0, 1, 3, 16, 32, 64, 512


def dma(id_):
    return ALGO_DMA_CFG0 + id_ if id_ < 16 else ALGO_DMA_CFG16 + id_ - 16


def strip(id_):
    return ALGO_STRIP_CFG0 + id_


def is_dma(k):
    return ALGO_DMA_CFG0 <= k < ALGO_STRIP_CFG0 or k >= ALGO_DMA_CFG16


def is_strip(k):
    return ALGO_STRIP_CFG0 <= k < ALGO_DMA_CFG16


# storage -> {request name: (algo, family)}; the LDS-DMA ids each storage type builds (marconet_hip.h, MNET_CONV_ALGO_DMA_CFG0 / 16)
_DMA_IDS = {"f16": (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 16, 17), "split": (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12),
            "mx": (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 16)}


def requests(storage):
    out = {"reg": (ALGO_REG, "reg"), "auto": (ALGO_AUTO, "all")}
    if storage == "f32":
        out["skinny"] = (ALGO_SKINNY, "skinny")
        return out
    gn = storage == "mx"
    for i in _DMA_IDS[storage]:
        out["dma%d" % i] = (dma(i), "dma" if gn else "dma_nogn")
    for i in ((0, 1) if storage != "split" else (1,)):
        out["strip%d" % i] = (strip(i), "strip" if gn else "strip_nogn")
    return out


# byte identity the header promises across the kernels of one storage type ("same bits for every launch size"): the kernels of this set give the
# same bytes for every row they all accept (f16 id 7 runs another MFMA shape; split-half: value agreement only)
BYTE_IDENTICAL = {
    "f16": {dma(i) for i in (0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 16, 17)} | {strip(0), strip(1)},
    "mx": {dma(i) for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 16)} | {strip(0), strip(1)},
}


def uses_shape(req, shape_name):
    """strip requests are only eligible on the big maps; the big maps run the kernels made for them (AUTO, strip, the big tiles)"""
    big = SHAPES[shape_name][-1]
    if req.startswith("strip"):
        return big
    if big:
        return req in ("auto", "dma5", "dma6", "dma8", "dma9", "dma11", "dma13", "dma15", "dma16")
    return True


# ---- the planner rules of the header (marconet_hip.h), stated as conditions on mnet_conv2d_plan's answer ------------------------------------
MX_HANDOVER_ACTS = (0, 2, 3)


def header_violations(storage, shape, row, algo, k):
    """what in mnet_conv2d_plan's answer ``k`` to request ``algo`` for ``row`` on ``shape`` contradicts the header; [] when nothing does"""
    n, h, w, c0, c1, cout, kk, stride, pad, vws, big = shape
    ho, wo = out_size(shape)
    bad = []
    xform, act, gn, center = row["xform"] != "none", row["act"], row["gn"] == "on", row["src2"] == "center"
    # :120-121: the LDS-DMA kernels take no input transform and no activation beyond LRELU_SQRT2 -> register-staged or refused
    if (xform or act > 3) and k >= 0 and k not in (ALGO_REG, ALGO_SKINNY):
        bad.append("input transform / act %d resolved to LDS-DMA kernel %d" % (act, k))
    # :109-115: GroupNorm sums need fp16+8, stride 1, cout % 32, ho*wo % 32 and an LDS-DMA / strip kernel
    if gn and k >= 0:
        if storage != "mx" or stride != (1, 1) or cout % 32 or (ho * wo) % 32:
            bad.append("gn_partial accepted on storage %s stride %s cout %d ho*wo %d" % (storage, stride, cout, ho * wo))
        if not (is_dma(k) or is_strip(k)):
            bad.append("gn_partial accepted on kernel %d" % k)
    # :162-168: the folded skip (x1 through the centre tap) runs on the LDS-DMA kernel only
    if center and k >= 0 and not is_dma(k):
        bad.append("x1_center accepted on kernel %d" % k)
    base = algo & ~FLAG_X1_CENTER
    if center and (base in (ALGO_REG, ALGO_SKINNY) or is_strip(base)) and k >= 0:
        bad.append("x1_center accepted for request %d" % base)
    # :183-184: the hand-overs (fp16+8 only)
    if storage == "mx" and k >= 0 and base == dma(16):
        want = dma(15) if (act not in MX_HANDOVER_ACTS or (ho * wo) % 32) else dma(16)
        if k != want:
            bad.append("fp16+8 id 16 request resolved to %d, header says %d" % (k, want))
    if storage == "mx" and k >= 0 and base == dma(9) and k != (dma(8) if gn else dma(9)):
        bad.append("fp16+8 id 9 request (gn %s) resolved to %d" % (gn, k))
    # a pinned LDS-DMA id of a storage type that builds it runs that id (or its hand-over) and nothing else
    if k >= 0 and is_dma(base) and not is_dma(k):
        bad.append("pinned LDS-DMA request %d resolved to kernel %d" % (base, k))
    # :120-122: AUTO takes an LDS-DMA (or strip) kernel when the f16 launch is eligible
    if center and stride != (1, 1) and k >= 0:                 # :167: x1 like x0 "(stride 1 launches)"
        bad.append("x1_center accepted on stride %s" % (stride,))
    if storage == "f16" and base == ALGO_AUTO and not xform and not gn and not center and act <= 3 and (c0 + (c1 if row["src2"] != "none" else 0)) % 64 == 0 \
            and c0 % 64 == 0 and cout >= 64 and cout % 8 == 0 and not (is_dma(k) or is_strip(k)):
        bad.append("eligible f16 AUTO launch resolved to kernel %d" % k)
    return bad
