"""CPU tier of the conv epilogue contract (tests/conv_contract.py): the all-pairs tables really cover every pair of factor levels and are the same
on every run, and mnet_conv2d_plan follows the rules include/marconet_hip.h states for every row x storage type x requested kernel."""
import ctypes
import itertools

import pytest

from tests import conv_contract as C

STORAGES = ("f32", "f16", "split", "mx")
_DTYPE = {"f32": 0, "f16": 1, "split": 2, "mx": 3}
_ADDR = 1 << 20          # any 128-byte aligned address: the planner checks presence and alignment of a buffer, never what is behind it


@pytest.mark.parametrize("family", sorted(C.FAMILY_LEVELS))
def test_table_covers_every_pair_and_is_deterministic(family):
    lv = C.family_levels(family)
    rows = C.all_pairs(lv)
    covered = set()
    for r in rows:
        assert set(r) == set(C.NAMES) and all(r[f] in lv[f] for f in C.NAMES)
        covered |= C.row_pairs(r)
    for a, b in itertools.combinations(C.NAMES, 2):
        for la in lv[a]:
            for lb in lv[b]:
                assert ((a, la), (b, lb)) in covered, (family, a, la, b, lb)
    assert rows == C.all_pairs(lv)                     # seeded: the same table on every run
    assert C.table(family) == C.table(family)
    # a greedy cover stays near the lower bound (the product of the two largest level counts)
    big = sorted((len(v) for v in lv.values()), reverse=True)
    assert len(rows) <= 2 * big[0] * big[1]


def test_forced_rows_reach_the_four_one_wave_tile_builds():
    builds = set()
    for r in C.FORCED.values():
        sc = r["out_scale"] != "none" or r["post_scale"] != "none"
        rg = r["residual"] != "none" or r["gn"] == "on"
        builds.add((sc, rg))
    assert builds == {(False, False), (False, True), (True, False), (True, True)}
    sz = C.FORCED["signed_zero"]
    assert sz["out_scale"] == "signed" and sz["bias"] == "none" and sz["valid_w"] == "ragged"


def _desc(storage, shape, row):
    from marconet_amd import _lib
    n, h, w, c0, c1, cout, k, stride, pad, vws, big = shape
    ho, wo = C.out_size(shape)
    d = _lib.ConvDesc()
    d.dtype = _DTYPE[storage]
    d.x0, d.c0 = _ADDR, c0
    d.x1, d.c1 = (None, 0) if row["src2"] == "none" else (_ADDR, c1)
    d.n, d.h, d.w = n, h, w
    d.wgt, d.y = _ADDR, _ADDR
    d.cout, d.kh, d.kw = cout, k, k
    d.stride_h, d.stride_w, d.pad_h, d.pad_w = stride[0], stride[1], pad, pad
    d.ho, d.wo = ho, wo
    xf = row["xform"] != "none"
    d.in_scale, d.in_shift, d.in_swish = (_ADDR if xf else None), (_ADDR if xf else None), int(row["xform"] == "swish")
    d.valid_w = _ADDR if row["valid_w"] != "none" else None
    d.out_scale = _ADDR if row["out_scale"] != "none" else None
    d.bias = _ADDR if row["bias"] != "none" else None
    d.residual = _ADDR if row["residual"] != "none" else None
    d.res_mod = C.res_mod(row, shape)
    d.act = row["act"]
    d.post_scale = _ADDR if row["post_scale"] != "none" else None
    d.gn_partial = _ADDR if row["gn"] == "on" else None
    return d


@pytest.mark.parametrize("storage", STORAGES)
def test_planner_follows_the_header_rules(storage):
    """every table row x shape x requested kernel: mnet_conv2d_plan's answer obeys the LDS-DMA eligibility list, the hand-over list, the gn_partial
    requirements and the x1_center restriction as include/marconet_hip.h writes them"""
    from marconet_amd import _lib
    lib = _lib.load()
    bad = []
    asked = 0
    for req, (algo, family) in sorted(C.requests(storage).items()):
        for sname, shape in C.SHAPES.items():
            if not C.uses_shape(req, sname):
                continue
            for name, row in C.table(family):
                a = algo | (C.FLAG_X1_CENTER if row["src2"] == "center" else 0)
                k = int(lib.mnet_conv2d_plan(ctypes.byref(_desc(storage, shape, row)), a))
                asked += 1
                bad += ["%s %s %s %s: %s" % (storage, req, sname, name, v) for v in C.header_violations(storage, shape, row, a, k)]
    assert asked > 100
    assert not bad, "\n".join(bad[:40])
