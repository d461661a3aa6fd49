"""-m gpu: the TextViT helpers (csrc/vit_kernels.hip: layernorm, token_mix, attention, argmax_rows) and the fp32 style path (pixelnorm, demod,
embed_gather; style_rows, gather_rows, pack_wsq) against the written-out fp64 formulas of tests/row_kernels.py, at the edges of each kernel: every
dispatch bound and guard of layernorm, the token / key masks and the ragged last workgroup of token_mix and attention, scores of +-128 that only a
max-subtracting softmax survives, rows where eps decides, every wave of the style_rows fold, the second trip of the two grid-stride gathers, and the
special values of argmax (ties, +-inf, NaN).

Cases, inputs, references and the metric live in tests/row_kernels.py; tests/test_row_kernels.py proves on a CPU that the cases reach the regimes they
name, that the plain fp32 evaluation of each formula stays within a quarter of the tolerance of the fp64 one, and that each named wrong formula misses
it by 10x or more.

Tolerance: per row |got - ref64| <= 2e-5 * max|ref64 of that row| (demod, pack_wsq: elementwise relative 2e-5); copies, gathers, power-of-two
scalings and indices: torch.equal.  Each test prints its largest error next to the tolerance."""
import pytest
import torch

from tests import row_kernels as K
from tests.test_kernels_gpu import ALL_DTYPES, MX, SPLIT  # noqa: F401  (the storages, shared not copied)

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = dict(zip(K.STORAGES, ALL_DTYPES))
assert DT == {"fp32": torch.float32, "f16": torch.float16, "split": SPLIT, "mx": MX}


def _ops():
    from marconet_amd import ops
    return ops


def _P():
    from marconet_amd import packing
    return packing


def _err():
    from marconet_amd._lib import MarconetHipError
    return MarconetHipError


def _sdt(storage):
    return {"fp32": torch.float32, "f16": torch.float16, "split": _P().SPLIT_DTYPE, "mx": _P().MX_DTYPE}[storage]


def _bytes(t):
    return t.cpu().contiguous().view(torch.uint8)


def _d(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _report(name, worst, tol=K.TOL):
    print("%-60s worst error %.3e  (tolerance %.1e)" % (name, worst, tol))


# ====================================================================================================================== layernorm
@pytest.mark.parametrize("rows", K.LN_ROWS)
@pytest.mark.parametrize("D", K.LN_D)
def test_layernorm_every_width_and_input_kind(D, rows):
    """layernorm_kernel<1 / 8 / 16> at both sides of each dispatch bound and at widths that leave lanes and registers empty (`c < D`), for rows under
    one workgroup, rows % 4 != 0 and many workgroups: N(1, 9) rows; exact-sum grid rows around a large offset (a one-pass variance is off 100-fold
    there); rows of std 0.003 with eps 1e-5 and with eps 1e-3 through the argument (eps is half / all of the denominator); constant rows (finite,
    beta)"""
    ops = _ops()
    worst = 0.0
    for kind in K.LN_KINDS:
        x, g, b, eps = K.ln_case(kind, rows, D)
        y = ops.layernorm(*_d(x, g, b), eps=eps).cpu()
        assert y.shape == (rows, D) and bool(torch.isfinite(y).all()), kind
        e = K.row_error(y, K.layernorm_formula(x, g, b, eps))
        print("    layernorm D=%d rows=%d %-16s %.3e" % (D, rows, kind, e))
        assert e <= K.TOL, "layernorm D=%d rows=%d %s: %.3e" % (D, rows, kind, e)
        worst = max(worst, e)
    _report("layernorm D=%d rows=%d PER=%d" % (D, rows, K.ln_per(D)), worst)


def test_layernorm_refuses_wider_rows_without_a_launch():
    ops = _ops()
    D = K.LN_REFUSED_D
    x, g, b = _d(torch.zeros(2, D), torch.ones(D), torch.zeros(D))
    with pytest.raises(_err(), match="d<=1024"):
        ops.layernorm(x, g, b)
    torch.cuda.synchronize()


# ====================================================================================================================== token_mix
@pytest.mark.parametrize("case", K.TM_CASES, ids=["%dx%dx%dx%d" % c for c in K.TM_CASES])
def test_token_mix_masks_and_ragged_workgroups(case):
    """LayerNorm over T tokens + Linear(T -> J) per (b, d): T = 64 and T < 64 (the `t < T` masks: a statistics loop that runs one token too far
    adds mean^2 to the variance of columns that have an offset), B*D under one workgroup and with a ragged last one (`id >= B*D`), J = 1; half of
    the columns have a variance of the order of eps.  Per [J, D] slice of a batch item"""
    ops = _ops()
    B, T, D, J = case
    x, lg, lb, W, bias = K.tm_case(*case)
    y = ops.token_mix(*_d(x, lg, lb, W, bias), eps=K.TM_EPS).cpu()
    assert y.shape == (B, J, D)
    e = K.row_error(y, K.token_mix_formula(x, lg, lb, W, bias, K.TM_EPS), row_dims=2)
    _report("token_mix B=%d T=%d D=%d J=%d" % case, e)
    assert e <= K.TOL


def test_token_mix_refuses_more_tokens_without_a_launch():
    ops = _ops()
    T = K.TM_REFUSED_T
    x, lg, lb, W, bias = _d(torch.zeros(1, T, 8), torch.ones(T), torch.zeros(T), torch.zeros(2, T), torch.zeros(2))
    with pytest.raises(_err(), match="T<=64"):
        ops.token_mix(x, lg, lb, W, bias)
    torch.cuda.synchronize()


# ====================================================================================================================== attention
@pytest.mark.parametrize("N", K.ATT_N)
def test_attention_every_block_border_and_planted_scores(N):
    """softmax(q k^T * scale) v at every sequence length around the 16-key blocks (1, 15 / 16 / 17, ..., 63 / 64), (B, H) = (3, 8), (1, 1), (2, 3),
    scale 0.125, 0.25, 1/sqrt(48): N(0, 1) inputs; integer-grid inputs (exact scores) with a score of +128 planted on an early key and on the last
    valid key N - 1; a head whose keys are all equal (the output is the mean of v) with one query row at +128 and one whole row at -128 — finite
    only with the max subtraction, and only if no masked key takes part in the maximum"""
    ops = _ops()
    worst = 0.0
    for B, H, scale, kind in K.att_cases(N):
        qkv, marks = K.att_case(kind, B, N, H)
        y = ops.attention(qkv.to(DEV), B, N, H, scale).cpu()
        assert y.shape == (B * N, H * 64)
        ref = K.attention_formula(qkv, B, N, H, scale)
        e = K.row_error(y, ref)
        print("    attention N=%d B=%d H=%d scale=%.4f %-10s %.3e" % (N, B, H, scale, kind, e))
        for b, h, i, _ in marks:
            assert bool(torch.isfinite(y.reshape(B, N, H, 64)[b, i, h]).all()), "planted row (b=%d, h=%d, i=%d) of %s is not finite" % (b, h, i, kind)
        assert e <= K.TOL, "attention N=%d B=%d H=%d scale=%g %s: %.3e" % (N, B, H, scale, kind, e)
        worst = max(worst, e)
    _report("attention N=%d" % N, worst)


def test_attention_refuses_longer_sequences_without_a_launch():
    ops = _ops()
    N = K.ATT_REFUSED_N
    with pytest.raises(_err(), match="N<=64"):
        ops.attention(torch.zeros(1, N, 3 * 64, device=DEV), 1, N, 1, 0.125)
    torch.cuda.synchronize()


# ====================================================================================================================== argmax_rows
@pytest.mark.parametrize("rows", K.ARGMAX_ROWS)
@pytest.mark.parametrize("D", K.ARGMAX_D)
def test_argmax_rows_is_torch_argmax(D, rows):
    """torch.argmax(x, -1) for every row, 0 <= idx < D always: the maximum at 0, at D - 1, at a lane's second element; ties within a lane and across
    lanes (the lower index in the higher lane); all-equal and all-negative rows; +inf; a row of -inf (index 0, not the start value of the search);
    NaN (the maximum, the first one wins) alone, with +inf, twice, everywhere.

    On the kernel before this test — `best = -inf, bi = 0x7fffffff`, candidates taken on `v > best` only — the rows "all -inf" and "all NaN" gave
    2147483647, "one NaN among finite values" / "two NaNs" the finite maximum, "NaN with +inf" the +inf"""
    ops = _ops()
    bad = []
    for t, (x, want) in enumerate(K.argmax_cases(D, rows)):
        ref = torch.argmax(x, -1)
        assert torch.equal(ref, want)
        got = ops.argmax_rows(x.to(DEV)).cpu()
        assert got.dtype == torch.int64 and got.shape == (rows,)
        for r in range(rows):
            if got[r].item() != ref[r].item() or not 0 <= got[r].item() < D:
                bad.append((K.ARGMAX_KINDS[(t * rows + r) % len(K.ARGMAX_KINDS)], got[r].item(), ref[r].item()))
    assert not bad, "argmax_rows D=%d rows=%d: (row kind, got, torch.argmax) %s" % (D, rows, bad)


# ====================================================================================================================== pixelnorm
@pytest.mark.parametrize("rows", K.PN_ROWS)
@pytest.mark.parametrize("D", K.PN_D)
def test_pixelnorm_widths_rows_and_eps(D, rows):
    """x * rsqrt(mean(x^2) + 1e-8) at widths under, at and off the wave size: N(0, 1) rows, rows of magnitude 1e-5 (eps is 99 % of the denominator),
    all-zero rows (exact zeros)"""
    ops = _ops()
    worst = 0.0
    for shift in range(3):
        x, kinds = K.pn_case(rows, D, shift)
        y = ops.pixelnorm(x.to(DEV)).cpu()
        e = K.row_error(y, K.pixelnorm_formula(x))
        assert e <= K.TOL, "pixelnorm D=%d rows=%d %s: %.3e" % (D, rows, kinds, e)
        for r, kd in enumerate(kinds):
            if kd == "zero":
                assert torch.equal(y[r], torch.zeros(D))
        worst = max(worst, e)
    _report("pixelnorm D=%d rows=%d" % (D, rows), worst)


# ====================================================================================================================== demod, pack_wsq
@pytest.mark.parametrize("cin", K.DEMOD_CIN)
def test_demod_quarter_split_and_eps_scale(cin):
    """rsqrt(sum_i s^2 wsq_t + 1e-8 eps_scale) with cin on every side of the quarter split `per = (cin + 3) >> 2` (empty quarters, the 16-wide unroll
    and its tail), cout under / at / off a wave, 1 and 9 styles, with and without eps_scale; an all-zero style row gives rsqrt(1e-8 eps_scale).
    Non-negative terms only: elementwise relative error"""
    ops = _ops()
    worst = 0.0
    for cout in K.DEMOD_COUT:
        for N in K.DEMOD_N:
            style, wsq_t, eps_scale = K.demod_case(N, cin, cout)
            sd, wd, ed = _d(style, wsq_t, eps_scale)
            for es, esd in ((None, None), (eps_scale, ed)):
                got = ops.demod(sd, wd, esd).cpu()
                assert got.shape == (N, cout)
                ref = K.demod_formula(style, wsq_t, es)
                e = K.elementwise_error(got, ref)
                assert e <= K.TOL, "demod cin=%d cout=%d N=%d eps_scale=%s: %.3e" % (cin, cout, N, es is not None, e)
                if N > 1:
                    z = (1e-8 * (1.0 if es is None else es[0].double())) ** -0.5
                    assert float((got[0].double() - z).abs().max()) <= K.TOL * float(z)
                worst = max(worst, e)
    _report("demod cin=%d" % cin, worst)


@pytest.mark.parametrize("case", K.WSQ_CASES, ids=["%dx%dx%d" % (c[0], c[1], c[2][0] * c[2][1]) for c in K.WSQ_CASES])
def test_pack_wsq(case):
    """wsq_t[i][o] = sum over the taps of (scale W[o][i])^2, transposed: 3x3 and 1x1 filters, cout * cin under, off and far over one workgroup"""
    ops = _ops()
    cout, cin, k = case
    w, scale = K.wsq_case(*case)
    got = ops.pack_wsq(w.to(DEV), scale).cpu()
    assert got.shape == (cin, cout)
    e = K.elementwise_error(got, K.pack_wsq_formula(w, scale))
    _report("pack_wsq %dx%dx%s" % (cout, cin, k), e)
    assert e <= K.TOL


# ====================================================================================================================== style_rows
@pytest.mark.parametrize("bcast", K.STYLE_BCAST)
@pytest.mark.parametrize("ncols", K.STYLE_NCOLS)
def test_style_rows_every_wave_holds_the_maximum(ncols, bcast):
    """window + gather + division by 2^e, e from the row's largest magnitude: the maximum sits in turn in a column of each of the four waves, in a
    column only the second trip of the 256-stride loops reaches, and in the last column (negative in every second row), every other value of the
    window is below half of it and every value outside the window is 16 times larger; magnitudes 1e-6 ... 4e6 with exactly 0.5 and 1.0; a zero
    row; with an index (repeats) and without; scale_b over 0 / 3 / 300 columns.  Exactly the host formula"""
    ops = _ops()
    src, idx, plan = K.style_case(ncols)
    for ix in (idx, None):
        want_rows, want_eps, want_sb, e = K.style_host(src, K.STYLE_COL0, ncols, ix, bcast)
        rows, eps, sb = ops.style_rows(src.to(DEV), K.STYLE_COL0, ncols, None if ix is None else ix.to(DEV), bcast=bcast)
        torch.cuda.synchronize()
        bad = (eps.cpu() != want_eps).nonzero().reshape(-1).tolist()
        assert not bad, "style_rows ncols=%d: wrong exponent in rows %s (source rows %s, (max column, magnitude) %s)" % (
            ncols, bad, [r if ix is None else ix[r].item() for r in bad], [plan[r if ix is None else ix[r].item()] for r in bad])
        assert torch.equal(rows.cpu(), want_rows)
        if bcast:
            assert sb.shape == (want_rows.shape[0], bcast) and torch.equal(sb.cpu(), want_sb)
        else:
            assert sb is None


# ====================================================================================================================== gather_rows
def test_gather_rows_windows_and_second_trip():
    """src[idx or every row][col0 : col0 + ncols], exactly: the small windows (one column, the last column, the whole row) and 4100 index rows of a
    512-column window — 2 099 200 elements, more than the 8192 x 256 of one trip of the capped grid"""
    ops = _ops()
    for sr, ld, col0, ncols, nidx in K.GATHER_SMALL + (K.GATHER_TWO_TRIPS,):
        src, idx = K.gather_case(sr, ld, col0, ncols, nidx)
        got = ops.gather_rows(src.to(DEV), col0, ncols, None if idx is None else idx.to(DEV)).cpu()
        want = K.gather_host(src, col0, ncols, idx)
        if not torch.equal(got, want):
            rows = (got != want).any(1).nonzero().reshape(-1)
            raise AssertionError("gather_rows %s: %d of %d rows differ, first %s, last %s" % ((sr, ld, col0, ncols, nidx), rows.numel(), want.shape[0],
                                                                                          rows[:4].tolist(), rows[-4:].tolist()))
    total, blocks, trips = K.gather_launch(K.GATHER_TWO_TRIPS[4], K.GATHER_TWO_TRIPS[3])
    assert trips == 2 and blocks == K.GATHER_CAP


# ====================================================================================================================== embed_gather
def _embed_check(emb, labels, scale, storage):
    ops, P = _ops(), _P()
    N, nc = labels.shape
    C = emb.shape[1]
    embd, labd, scd = _d(emb, labels, scale)
    got = ops.embed_gather(embd, labd, _sdt(storage), K.EMBED_CLASSES, scale=scd)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (N, 4, 4 * nc, C) and got.dtype == _sdt(storage)
    want = P.from_float(K.embed_host(emb, labels, scale), _sdt(storage))
    gb, wb = _bytes(got).reshape(N * 16 * nc, -1), _bytes(want).reshape(N * 16 * nc, -1)
    if not torch.equal(gb, wb):
        pix = (gb != wb).any(1).nonzero().reshape(-1)
        raise AssertionError("embed_gather %s N=%d nc=%d C=%d scale=%s: %d of %d pixels differ from the host packer, first %s, last %s"
                             % (storage, N, nc, C, scale is not None, pix.numel(), gb.shape[0], pix[:4].tolist(), pix[-4:].tolist()))


@pytest.mark.parametrize("storage", K.STORAGES)
def test_embed_gather_every_storage_is_the_host_packer(storage):
    """the SelectText gather into all four storages (the two blocked ones had no op-level test), 1 / 2 / 16 glyph slots, C = 64 and 512, labels
    0 and num_classes - 1 among them, with and without the per-(sample, channel) scale: the bytes the host packer gives for the same fp32 values"""
    for N, nc, C in K.EMBED_CASES:
        emb, labels, scale = K.embed_case(N, nc, C)
        for sc in (None, scale):
            _embed_check(emb, labels, sc, storage)


def test_embed_gather_second_trip():
    """fp32, 130 samples x 16 slots x 512 channels: 4 259 840 chunks, more than the 16384 x 256 of one trip of the capped grid (68 MB out)"""
    emb, labels, scale = K.embed_two_trip_inputs()
    assert K.embed_launch(*K.EMBED_TWO_TRIPS, "fp32")[1:] == (K.EMBED_CAP, 2)
    _embed_check(emb, labels, scale, "fp32")
