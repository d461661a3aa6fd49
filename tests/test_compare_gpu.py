"""-m gpu: mnet_compare_stats against the spec of tests/compare_spec.py — for all six (mode, reference) storage pairs, at the sizes tests/test_compare.py
proves to reach every launch regime of the kernel, with the maximum planted where a reduction goes wrong (first / last element, either side of every slice
boundary, the last chunk of a ragged tail, a duplicate further on that must not win), non-finite elements in one operand and in both, and the invariance
claims (a group alone = the group in a batch; a second launch = the first) as BYTES.  Every launch writes into buffers with a 0xCD guard around the records
and the workspace.  Tensors are the finite writer pages of tests/storage_codec.py encoded into each storage; what is expected is computed from the spec's
decoders over the very bytes uploaded."""
import ctypes

import numpy as np
import pytest
import torch

from tests import compare_spec as C
from tests import storage_codec as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256
PAIR_IDS = ["%s_vs_%s" % p for p in C.PAIRS]


def _pk():
    from marconet_amd import packing
    return packing


def _dtype(storage):
    pk = _pk()
    return {"mx": pk.MX_DTYPE, "split": pk.SPLIT_DTYPE, "f16": torch.float16, "f32": torch.float32}[storage]


def _upload(op):
    t = torch.from_numpy(np.ascontiguousarray(op.raw).reshape(-1)).to(DEV).view(_dtype(op.storage)).reshape(op.groups, op.elems)
    assert t.data_ptr() % 128 == 0
    return _pk().tag(t)


def _run(ta, tb, groups, elems):
    """the C entry itself on guarded buffers -> RECORD_DTYPE array [groups] (the guards are checked here, on every launch of this file)"""
    from marconet_amd import _lib, ops
    lib = _lib.load()
    nrec, nws = groups * C.RECORD_BYTES, _lib.cmp_workspace_bytes(groups, elems)
    assert nws == groups * C.slices(elems) * C.RECORD_BYTES
    o_rec = GUARD
    o_ws = (o_rec + nrec + GUARD + 7) // 8 * 8
    buf = torch.full((o_ws + nws + GUARD,), 0xCD, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 8 == 0
    with torch._C.DisableTorchFunctionSubclass():
        _lib.check(lib.mnet_compare_stats(ops._p(ta), ops._dt(ta), ops._p(tb), ops._dt(tb), groups, elems, ctypes.c_void_p(buf.data_ptr() + o_rec),
                                          ctypes.c_void_p(buf.data_ptr() + o_ws), ops._stream()), "mnet_compare_stats")
    host = buf.cpu().numpy()
    guard = np.concatenate([host[:o_rec], host[o_rec + nrec:o_ws], host[o_ws + nws:]])
    assert (guard == 0xCD).all(), "bytes outside the records / the workspace were written"
    return host[o_rec:o_rec + nrec].copy().view(C.RECORD_DTYPE), host[o_ws:o_ws + nws].copy()


_BASE = {}


def _base(storage, groups, elems):
    """the encoded writer pages, once per (storage, shape) of the session; callers take copies"""
    key = (storage, groups, elems)
    if key not in _BASE:
        _BASE[key] = C.Operand(storage, C.base_values(groups, elems))
    return _BASE[key].copy()


def _check(a, b, what):
    got, _ = _run(_upload(a), _upload(b), a.groups, a.elems)
    bad = C.mismatches(got, C.records(a.decoded_bits(), b.decoded_bits(), a.groups))
    assert not bad, "%s:\n%s" % (what, "\n".join(bad))
    return got


@pytest.mark.parametrize("elems", C.SIZES)
@pytest.mark.parametrize("pair", C.PAIRS, ids=PAIR_IDS)
def test_records_are_exact_wherever_the_maximum_lies(pair, elems):
    """groups {1, 3}: the plain pages (what the two storages make of the same values), then the maximum planted at every position of plant_positions — a
    different one in each group of a launch — with a duplicate of the same size at the next higher planted position, which must not win"""
    ms, rs = pair
    for groups in C.GROUPS:
        _check(_base(ms, groups, elems), _base(rs, groups, elems), "%s vs %s, %d x %d, as encoded" % (ms, rs, groups, elems))
    pos = C.plant_positions(elems)
    groups = 3
    for at in range(0, len(pos), groups):
        a, b = _base(ms, groups, elems), _base(rs, groups, elems)
        want_idx = []
        for g in range(groups):
            p = pos[(at + g) % len(pos)]
            higher = [q for q in pos if q > p]
            for q in [p] + higher[:1]:
                a.set(g, q, -C.PLANT)
                b.set(g, q, C.PLANT)
            want_idx.append(p)
        got = _check(a, b, "%s vs %s, %d elements, maxima planted at %s" % (ms, rs, elems, want_idx))
        assert got["argmax_index"].tolist() == want_idx and (got["max_abs_diff"] == np.float32(2 * C.PLANT)).all()


@pytest.mark.parametrize("pair", C.PAIRS, ids=PAIR_IDS)
def test_nonfinite_pairs_are_counted_and_left_out(pair):
    """the non-finite pages' elements (inf, NaN of both signs; block 0 and block 5 of a page) written over the first page of a group: in the mode's tensor
    (group 0), in the reference's (group 1), in both at the SAME and at other positions (group 2) — beside each a difference that would be the maximum if the
    pair counted.  A group of nothing but non-finite pairs reports no index."""
    ms, rs = pair
    groups, elems = 3, C.WG_ELEMS + 32
    a, b = _base(ms, groups, elems), _base(rs, groups, elems)
    inf_page, nan_page = [p for p in S.nonfinite_pages() if p["name"] in ("inf", "nan")]
    for page, off in ((inf_page, 0), (nan_page, C.WG_ELEMS - S.PAGE + 32)):           # the second copy straddles the slice boundary
        for p in np.nonzero(page["bad"])[0]:
            v = float(page["v"][p])
            a.poke_nonfinite(0, off + p, v)
            b.poke_nonfinite(1, off + p, v)
            a.poke_nonfinite(2, off + p, v)
            b.poke_nonfinite(2, off + (p if p % 2 else p + 2), -v)
    # a finite value of the planted size opposite a non-finite one: it must not become the maximum
    nf0 = int(np.nonzero(inf_page["bad"])[0][0])
    b.set(0, nf0, C.PLANT)
    a.set(1, nf0, -C.PLANT)
    got = _check(a, b, "%s vs %s, non-finite elements" % (ms, rs))
    assert got["nonfinite_mode"][0] > 0 and got["nonfinite_ref"][0] == 0 and got["nonfinite_mode"][1] == 0 and got["nonfinite_ref"][1] > 0
    assert got["nonfinite_mode"][2] > 0 and got["nonfinite_ref"][2] > 0 and (got["max_abs_diff"] < C.PLANT).all()
    a1, b1 = _base(ms, 1, 32), _base(rs, 1, 32)
    for p in range(32):
        (a1 if p % 2 else b1).poke_nonfinite(0, p, np.nan if p % 3 else np.inf)
    got = _check(a1, b1, "%s vs %s, no finite pair" % (ms, rs))
    assert got["argmax_index"][0] == -1 and got["max_abs_diff"][0] == 0 and got["nonfinite_mode"][0] == 16 and got["nonfinite_ref"][0] == 16


@pytest.mark.parametrize("elems", (2 * C.WG_ELEMS + 32, C.MAX_SLICES * C.WG_ELEMS + 32))
@pytest.mark.parametrize("pair", C.PAIRS, ids=PAIR_IDS)
def test_a_group_alone_and_a_second_launch_give_the_same_bytes(pair, elems):
    """batch invariance and determinism as bytes: records AND the workspace's partial records (three slices; the capped grid with its second trip)"""
    ms, rs = pair
    a, b = _base(ms, 3, elems), _base(rs, 3, elems)
    b.set(1, elems // 2, C.PLANT)
    ta, tb = _upload(a), _upload(b)
    rec, ws = _run(ta, tb, 3, elems)
    rec2, ws2 = _run(ta, tb, 3, elems)
    assert rec.tobytes() == rec2.tobytes() and ws.tobytes() == ws2.tobytes()
    per_ws = C.slices(elems) * C.RECORD_BYTES
    with torch._C.DisableTorchFunctionSubclass():
        singles = [(_pk().tag(ta[g:g + 1].contiguous()), _pk().tag(tb[g:g + 1].contiguous())) for g in range(3)]
    for g, (sa, sb) in enumerate(singles):
        assert sa.data_ptr() % 16 == 0 and sb.data_ptr() % 128 == 0 and (ms == "f16" or sa.data_ptr() % 128 == 0)      # (a plain-half group may start on 64 bytes)
        r1, w1 = _run(sa, sb, 1, elems)
        assert r1.tobytes() == rec[g:g + 1].tobytes() and w1.tobytes() == ws[g * per_ws:(g + 1) * per_ws].tobytes(), "group %d alone differs" % g


def test_ops_wrapper_returns_the_records_on_the_device():
    """ops.compare_stats: tagged blocked tensors in, a uint8 device tensor out that _lib.cmp_records reads; ``groups`` regroups the same bytes"""
    from marconet_amd import _lib, ops
    a, b = _base("mx", 3, 224), _base("split", 3, 224)
    b.set(2, 100, C.PLANT)
    ta, tb = _upload(a), _upload(b)
    out = ops.compare_stats(ta, tb)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (3, C.RECORD_BYTES)
    recs = _lib.cmp_records(out.cpu().numpy())
    want = C.records(a.decoded_bits(), b.decoded_bits(), 3)
    assert [r.argmax_index for r in recs] == [w["argmax_index"] for w in want] and recs[2].argmax_index == 100
    assert not C.mismatches(out.cpu().numpy().reshape(-1).view(C.RECORD_DTYPE), want)
    one = ops.compare_stats(ta, tb, groups=1)
    assert not C.mismatches(one.cpu().numpy().reshape(-1).view(C.RECORD_DTYPE), C.records(a.decoded_bits(), b.decoded_bits(), 1))
    with pytest.raises(ValueError):
        ops.compare_stats(ta, tb, groups=5)
    with pytest.raises(_lib.MarconetHipError):
        ops.compare_stats(tb, ta)                                   # (split half, fp16+8): no such pair
