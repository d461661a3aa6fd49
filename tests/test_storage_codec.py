"""CPU tier of the storage byte tests: the tables of tests/storage_codec.py are what they claim to be, the spec agrees with independent conversions of
the same number formats, and the host packers (marconet_amd/mxfmt.py, marconet_amd/packing.py) write the spec's bytes on every finite page.  Every
comparison is exact (bytes / bits)."""
import numpy as np
import pytest
import torch

from tests import storage_codec as S
from marconet_amd import mxfmt, packing

PAGES = S.writer_pages()
TABLE = S.writer_table()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---------------------------------------------------------------------------------------------------------------- the spec against independent conversions
def test_spec_f16_rounding_is_numpy_s():
    rng = np.random.default_rng(0)
    x = np.concatenate([TABLE.reshape(-1), (rng.standard_normal(20000) * np.logspace(-9, 5, 20000)).astype(np.float32),
                        S.from_bits32(rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32))])
    x = x[~np.isnan(x)]
    with np.errstate(over="ignore"):
        assert np.array_equal(S.f16_bits(x), x.astype(np.float16).view(np.uint16))


def test_spec_e4m3_is_torch_s():
    codes = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(codes), np.isnan(S.E4M3_VALUE)) and np.array_equal(np.nan_to_num(codes), np.nan_to_num(S.E4M3_VALUE))
    assert np.array_equal(np.signbit(codes), np.signbit(S.E4M3_VALUE))
    rng = np.random.default_rng(1)
    mids = np.array([t for t, c in S._e4m3_ties()])
    x = np.concatenate([mids, -mids, np.nextafter(mids, 0), np.nextafter(mids, 1e9), S.E4M3_VALUE[S.LO_CODES], rng.uniform(-448, 448, 20000),
                        rng.standard_normal(20000) * np.logspace(-6, 2, 20000), [0.0, -0.0, 1e-12, -1e-12, 448.0, -448.0, 2.0 ** -10, -2.0 ** -10]])
    x = x[np.abs(x) <= 448.0].astype(np.float32)        # (float8 conversion from fp32: every value of the spec's use is an fp32)
    assert np.array_equal(S.e4m3_bits(x.astype(np.float64)), _t(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy())


def test_one_rounding_sum():
    """_sum_to_f32 against exact rational arithmetic on sums that span more than 53 bits"""
    from fractions import Fraction
    rng = np.random.default_rng(2)
    a = np.ldexp(rng.integers(1, 2048, 400).astype(np.float64), rng.integers(-24, 6, 400)) * rng.choice([-1.0, 1.0], 400)
    b = np.ldexp(rng.integers(1, 16, 400).astype(np.float64), rng.integers(-60, 118, 400)) * rng.choice([-1.0, 1.0], 400)
    # ties of the fp32 grid whose decision lies beyond fp64's 53 bits
    a = np.concatenate([a, [2.0 ** -24, -2.0 ** -24, 2.0 ** -24]])
    b = np.concatenate([b, [3 * 2.0 ** 60, 3 * 2.0 ** 60, -(2.0 ** 24 + 1) * 2.0 ** 37]])
    got = S._sum_to_f32(a, b)
    for x, y, g in zip(a, b, got):
        exact = Fraction(float(x)) + Fraction(float(y))
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        d = abs(exact - Fraction(float(g)))
        assert d <= abs(exact - Fraction(float(lo))) and d <= abs(exact - Fraction(float(hi)))
        if d == abs(exact - Fraction(float(lo))) or d == abs(exact - Fraction(float(hi))):
            assert (int(np.float32(g).view(np.uint32)) & 1) == 0           # a true tie goes to even


# ---------------------------------------------------------------------------------------------------------------- the tables
@pytest.mark.parametrize("page", PAGES + S.nonfinite_pages(), ids=lambda p: p["name"])
def test_page_is_in_its_class(page):
    assert page["v"].shape == (S.PAGE,) and page["v"].dtype == np.float32
    assert S.PREDICATES[page["cls"]](page["v"]), "page %s is not in class %s" % (page["name"], page["cls"])
    if page["cls"] == "nonfinite":
        assert np.array_equal(S.nonfinite_mask(page["v"]), page["bad"]) and page["bad"].reshape(8, 32).any(1).sum() == 2      # next to finite neighbours
    else:
        assert np.isfinite(S.f16_round(page["v"].astype(np.float64))).all()
        assert S.lo_reach(page["v"]) <= 256.0          # the header's claim: no finite input saturates e4m3


def test_every_class_of_the_issue_has_a_page():
    have = {p["cls"] for p in PAGES}
    assert have >= {"max_pow2", "max_rounds_up", "half_max", "e4m3_ties", "half_ties", "lo_underflow", "subnormal_blocks", "zero_hi", "zeros", "neg_zero",
                    "one_nonzero", "f32_subnormal"}
    assert {p["name"] for p in S.nonfinite_pages()} == {"inf", "nan", "overflow"}


def test_ties_cover_every_binade_sign_and_parity():
    """binades 0 (e4m3 subnormals) .. 14 ([128, 256)); [256, 448] is beyond every conforming writer (lo_reach <= 256, and 256 itself is a code)"""
    seen = set()
    for p in PAGES:
        seen |= S.tie_census(p["v"])
    need = {(b, neg, odd) for b in range(15) for neg in (False, True) for odd in (False, True)}
    assert need <= seen, sorted(need - seen)


def test_reader_tables_cover_what_they_claim():
    T = S.reader_table_hm()
    assert T.shape[0] % 8 == 0 and T.shape[1] == 128 and not T[:, 97:].any()
    lo = T[:, 64:96][:, S.INV_PERM]                         # channel order
    hi = np.ascontiguousarray(T[:, 0:64]).view(np.uint16)
    for E in S.READER_E:
        rows = T[:, 96] == E
        for j in range(32):
            assert set(lo[rows, j].tolist()) == set(S.LO_CODES.tolist()), (E, j)
            assert set(hi[rows, j].tolist()) == set(S.READER_HI_BITS), (E, j)
    assert not np.isin(lo, (0x7f, 0xff)).any()
    zero = T[:, 96] == 0
    assert zero.sum() >= 14 and not (lo[zero] & 0x7f).any() and (lo[zero] == 0x80).any() and not (hi[zero] & 0x7fff).any()
    assert np.isfinite(S.from_bits32(S.decode_hm(T))).all()
    sp = S.reader_table_hm_special()
    for name in ("lo_nan", "hi_nonfinite"):
        raw, mask = sp[name]
        assert np.array_equal(~np.isfinite(S.from_bits32(S.decode_hm(raw))), mask), name
    R = S.reader_table_split()
    assert R.shape[0] % 8 == 0
    h = np.ascontiguousarray(R).view(np.uint16).reshape(-1, 2, 32)
    assert {(a, b) for a, b in zip(h[:, 0].reshape(-1).tolist(), h[:, 1].reshape(-1).tolist())} == {(a, b) for a in S.READER_HI_BITS for b in S.SPLIT_LO_BITS}


# ---------------------------------------------------------------------------------------------------------------- host packers = spec
def test_host_activation_packers_write_the_spec_bytes():
    t = _t(TABLE)
    for i, p in enumerate(PAGES):
        assert np.array_equal(mxfmt.pack_act(t[i]).numpy(), S.encode_hm(TABLE[i])), "mxfmt.pack_act, page %s" % p["name"]
        assert np.array_equal(packing.untag(packing.split_halves(t[i])).view(torch.uint8).numpy(), S.encode_split(TABLE[i])), "split_halves, page %s" % p["name"]
        assert np.array_equal(t[i].to(torch.float16).view(torch.uint8).numpy(), S.encode_f16(TABLE[i])), ".to(float16), page %s" % p["name"]
        assert np.array_equal(packing.untag(packing.from_float(t[i], packing.MX_DTYPE)).view(torch.uint8).numpy(), S.encode_hm(TABLE[i]))


def test_host_decoders_agree_bit_for_bit():
    hm, sp, h = S.encode_hm(TABLE), S.encode_split(TABLE), S.encode_f16(TABLE)
    assert np.array_equal(S.bits32(mxfmt.unpack_act(_t(hm), S.PAGE).numpy()), S.decode_hm(hm))
    assert np.array_equal(S.bits32(packing.unsplit_halves(_t(sp).view(packing.SPLIT_DTYPE)).numpy()), S.decode_split(sp))
    assert np.array_equal(S.bits32(_t(h).view(torch.float16).float().numpy()), S.decode_f16(h))
    # raw blocks: everything a writer can emit and more (E up to 142; at E = 254 the host's fp32 intermediate lo8 * 2^127 overflows, the device's does not)
    R = S.reader_table_hm()
    R = R[R[:, 96] <= 142]
    assert np.array_equal(S.bits32(mxfmt.unpack_act(_t(R), 32).numpy()), S.decode_hm(R))
    Rs = S.reader_table_split()
    assert np.array_equal(S.bits32(packing.unsplit_halves(_t(Rs).view(packing.SPLIT_DTYPE)).numpy()), S.decode_split(Rs))


def test_zero_hi_block_of_the_finding():
    """x = (1e-9, -2^-26, 2^-25, 0 ...): every hi is +-0, so E = 0, the lo bytes are signed ZERO bytes (they were 0x7e, 0xfe, 0x7e: the residual saturated
    under s = 2^-127) and the block decodes to its hi halves exactly"""
    x = torch.zeros(32)
    x[0], x[1], x[2] = 1e-9, -2.0 ** -26, 2.0 ** -25
    b = mxfmt.pack_act(x)
    assert int(b[96]) == 0 and b[64:67].tolist() == [0x00, 0x80, 0x00] and not (b[64:96] & 0x7f).any() and not b[97:].any()
    assert b[0:6].view(torch.float16).view(torch.int16).tolist() == [0, -32768, 0]
    d = mxfmt.unpack_act(b, 32)
    assert S.bits32(d.numpy()).tolist() == [0, 0x80000000, 0] + [0] * 29


def test_split_halves_accepts_the_whole_half_range():
    top = float(np.nextafter(np.float32(65520.0), np.float32(0)))
    packing.split_halves(torch.full((32,), top))
    with pytest.raises(OverflowError):
        packing.split_halves(torch.full((32,), 65520.0))


# ---------------------------------------------------------------------------------------------------------------- weights
STORAGES = {"f32": torch.float32, "f16": torch.float16, "split": packing.SPLIT_DTYPE, "mx": packing.MX_DTYPE}


@pytest.mark.parametrize("case", list(S.MX_WEIGHT_SHAPES))
@pytest.mark.parametrize("storage", list(STORAGES))
def test_host_weight_packer_writes_the_spec_bytes(case, storage):
    shape = S.MX_WEIGHT_SHAPES[case]
    cout, cin, kh, kw, cout_pad, cin_pad = shape
    w = S.weight_tensor(shape, seed=list(S.MX_WEIGHT_SHAPES).index(case))
    v = S.stored_weight_values(w, storage, cout_pad=cout_pad, cin_pad=cin_pad)
    assert storage != "mx" or S.weight_rows_defined(v)
    m = np.abs(S.f16_round(v[0].astype(np.float64))).max()
    assert m > 0 and np.frexp(m)[0] == 0.5                                         # a row whose maximum is 2^k exactly
    got = packing.pack_conv_weight(_t(w), STORAGES[storage], cin_mult=32, cout_mult=32)
    want = S.encode_weight(v, storage)
    if storage == "mx":
        assert tuple(got.shape) == (S.mx_weight_rows(cout_pad, kh, kw, cin_pad), kh, kw, cin_pad)
        assert S.mx_weight_rows(cout_pad, kh, kw, cin_pad) == packing.mx_weight_rows(cout_pad, kh, kw, cin_pad)
        tail = want[cout_pad * kh * kw * cin_pad * 4:]
        nonzero = np.abs(v.reshape(cout_pad, -1)).max(1) > 0
        assert not tail[cout:].any() and nonzero[:cout].sum() >= cout * 3 // 4 and np.array_equal(tail[:cout_pad] > 0, nonzero)      # zero rows: scale byte 0
    else:
        assert tuple(got.shape) == (cout_pad, kh, kw, cin_pad)
    assert np.array_equal(packing.untag(got).contiguous().view(torch.uint8).reshape(-1).numpy(), want)


@pytest.mark.parametrize("storage", list(STORAGES))
def test_host_weight_packer_rounds_the_fp32_product(storage):
    """(w * scale) is rounded to fp32 and THEN into the storage: elements whose exact product rounds to another half than its fp32 rounding does (the
    maximum of rows 0-3 across a power of two: another row scale in fp16+8), and -0 products"""
    cout, cin, kh, kw, cout_pad, cin_pad = S.DR_SHAPE
    w, others = S.double_rounding_case()
    assert others >= 16
    v = S.stored_weight_values(w, storage, scale=S.DR_SCALE, cout_pad=cout_pad, cin_pad=cin_pad)
    exact = w.reshape(cout, cin).astype(np.float64) * float(np.float32(S.DR_SCALE)) * (256.0 if storage in ("split", "mx") else 1.0)
    twice, once = S.f16_round(v[:cout, 0, 0, :].astype(np.float64)), S.f16_round(exact)
    assert (twice != once).sum() >= 4 + 16 and all(S._floor_log2(np.abs(twice[o]).max()) == S._floor_log2(np.abs(once[o]).max()) + 1 for o in range(4))
    got = packing.pack_conv_weight(_t(w), STORAGES[storage], cin_mult=32, cout_mult=32, scale=S.DR_SCALE)
    assert np.array_equal(packing.untag(got).contiguous().view(torch.uint8).reshape(-1).numpy(), S.encode_weight(v, storage))


@pytest.mark.parametrize("K", S.SN_K)
def test_sigma_is_clear_of_an_fp32_rounding_boundary(K):
    w, u, v, sigma, margin = S.sn_case(K)
    assert w.shape[1] * w.shape[2] * w.shape[3] == K and margin >= 2.0 ** -30
    # another fp64 summation order gives the same fp32
    alt = float(np.sum((u.astype(np.float64)[:, None] * w.reshape(len(u), -1).astype(np.float64)) * v.astype(np.float64)[None, :]))
    assert np.float32(alt) == np.float32(sigma)


def test_big_plain_shape_takes_a_second_grid_stride_trip():
    cout, cin, kh, kw = S.BIG_PLAIN_SHAPE
    assert cout * cin * kh * kw > 16384 * 256 and cin % 32 == 0 and cout % 32 != 0


# ---------------------------------------------------------------------------------------------------------------- the table has teeth
def _encode_hm_mutant(v, scale_from_v=False, no_floor=False):
    """encode_hm with one of the two mistakes the table is there to catch"""
    vb = S._blocks(v).astype(np.float64)
    hi = S.f16_round(vb)
    m = np.abs(vb if scale_from_v else hi).max(axis=-1, keepdims=True)
    E = np.where(m > 0, np.maximum(S._floor_log2(m) + 120, 0 if no_floor else S.E_FLOOR), 0)
    lo8 = S.e4m3_bits(S._lo_scaled(vb - hi, E, 1))
    return E[..., 0], lo8


def test_named_pages_catch_the_two_mutations():
    by = {p["name"]: p["v"] for p in PAGES}
    # block maximum from v instead of hi: the largest fp32 below 2^k has the exponent k - 1 — another scale byte for every k above the floor
    v = by["max_rounds_up"]
    E_ok = S.encode_hm(v).reshape(8, 128)[:, 96]
    E_bad, _ = _encode_hm_mutant(v, scale_from_v=True)
    assert [int(a) - int(b) for a, b in zip(E_ok, E_bad)] == [0 if k == -15 else 1 for k in S.ROUND_UP_K]
    # no floor at 105: fp16-subnormal blocks get a smaller exponent and residuals beyond e4m3 (NaN bytes from the device conversions)
    v = by["subnormal_blocks"]
    E_bad, lo_bad = _encode_hm_mutant(v, no_floor=True)
    assert (E_bad < S.E_FLOOR).sum() >= 6 and (lo_bad & 0x7f == 0x7f).any()
    assert (_encode_hm_mutant(by["max_pow2"], no_floor=True)[0][[0, 6]] == 96).all()           # max 2^-24: 96 without the floor
