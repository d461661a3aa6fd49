"""No device: the cases of tests/test_row_kernels_gpu.py are what tests/row_kernels.py says they are —
  * the mirrored constants (dispatch bounds, size limits, grid caps, rows per workgroup) are still the ones the sources hold;
  * the regimes are reached (every layernorm_kernel<PER> launched, the `c < D` guards fire, ragged last workgroups, second grid-stride trips, every
    wave of style_rows holding the maximum in turn, empty demod quarters);
  * the integer-grid sums and attention scores are exact in fp32 in any order;
  * the written-out formula evaluated in plain fp32 stays within a quarter of the tolerance of its fp64 evaluation (the reference is precise enough,
    and a correct kernel keeps a factor 4 for its summation order);
  * every hazard case bites: the named wrong formula, in fp32, misses the tolerance by at least 10x."""
import math
import os
import re

import pytest
import torch

from tests import row_kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64


def _src(*rel):
    with open(os.path.join(ROOT, *rel)) as f:
        return f.read()


def _body(src, start, end):
    a = src.index(start)
    return src[a:src.index(end, a)]


def _misses(err, bound=K.BITE):
    return not err <= bound                     # (NaN misses)


# ====================================================================================================================== constants and regimes
def test_mirrored_constants_are_the_sources():
    vit = _src("marconet_amd", "csrc", "vit_kernels.hip")
    aux = _src("marconet_amd", "csrc", "aux_kernels.hip")
    pack = _src("marconet_amd", "csrc", "pack_kernels.hip")
    ln = _body(vit, 'extern "C" int mnet_layernorm', "MNET_LAUNCH_CHECK")
    assert "d <= %d, " % K.LN_BOUNDS[2] in ln
    assert "if (d <= %d) hipLaunchKernelGGL(layernorm_kernel<%d>" % (K.LN_BOUNDS[0], K.LN_PER[0]) in ln
    assert "else if (d <= %d) hipLaunchKernelGGL(layernorm_kernel<%d>" % (K.LN_BOUNDS[1], K.LN_PER[1]) in ln
    assert "else hipLaunchKernelGGL(layernorm_kernel<%d>" % K.LN_PER[2] in ln
    assert 64 * K.LN_PER[2] == K.LN_BOUNDS[2] and 64 * K.LN_PER[1] == K.LN_BOUNDS[1] and 64 * K.LN_PER[0] == K.LN_BOUNDS[0]
    assert "const int c = lane + 64 * i; v[i] = c < D ? xr[c] : 0.f;" in vit
    tm = _body(vit, 'extern "C" int mnet_token_mix', "MNET_LAUNCH_CHECK")
    assert "T <= %d &&" % K.TM_MAX_T in tm and "dim3((tot + 255) / 256), dim3(%d)" % K.WG in tm and "const int tot = B * D;" in tm
    assert "if (id >= B * D) return;" in vit and "float v[%d];" % K.TM_MAX_T in vit
    att = _body(vit, 'extern "C" int mnet_attention', "MNET_LAUNCH_CHECK")
    assert "N <= %d &&" % K.ATT_MAX_N in att and "dim3(B * H), dim3(%d)" % K.WG in att
    assert "kb * 16 + l16 < N" in vit
    # one wave per row, four rows per workgroup: layernorm, argmax, pixelnorm
    row_of = "const int row = blockIdx.x * %d + (threadIdx.x >> 6), lane = threadIdx.x & 63;" % K.ROWS_PER_WG
    assert vit.count(row_of) == 2 and aux.count(row_of) >= 1
    assert "dim3 grid((rows + 3) / 4), block(%d);" % K.WG in ln
    assert "dim3((rows + 3) / 4), dim3(%d)" % K.WG in _body(vit, 'extern "C" int mnet_argmax_rows', "MNET_LAUNCH_CHECK")
    assert "dim3((N_ + 3) / 4), dim3(%d)" % K.WG in _body(aux, 'extern "C" int mnet_pixelnorm', "MNET_LAUNCH_CHECK")
    ga = _body(pack, 'extern "C" int mnet_gather_rows', "MNET_LAUNCH_CHECK")
    assert "(total + 255) / 256 < %d ? (total + 255) / 256 : %d" % (K.GATHER_CAP, K.GATHER_CAP) in ga and "(long long)rows * ncols" in ga
    em = _body(aux, 'extern "C" int mnet_embed_gather_scaled', "MNET_LAUNCH_CHECK")
    assert "(total + 255) / 256 < %d ? (total + 255) / 256 : %d" % (K.EMBED_CAP, K.EMBED_CAP) in em
    assert "(long long)N_ * 16 * nc * (C / N)" in em
    assert "const int per = (cin + 3) >> 2, i0 = q * per, i1 = min(cin, i0 + per);" in aux and "for (; i + 16 <= i1; i += 16)" in aux
    st = _body(pack, "void __launch_bounds__(256) style_rows_kernel", 'extern "C"')
    assert "for (int c = t; c < ncols; c += 256)" in st and "fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))" in st


def test_layernorm_cases_launch_every_kernel_and_fire_the_guards():
    assert {K.ln_per(d) for d in K.LN_D} == set(K.LN_PER)                              # PER = 1, 8, 16 all launched
    assert [K.ln_per(d) for d in K.LN_D] == [1, 1, 1, 8, 8, 8, 16, 16, 16]
    assert set(K.LN_BOUNDS) <= set(K.LN_D) and {b + 1 for b in K.LN_BOUNDS[:2]} <= set(K.LN_D) and {b - 1 for b in K.LN_BOUNDS[:2]} <= set(K.LN_D)
    for per in K.LN_PER:                                                               # per kernel: a width with idle lanes and the full one
        ds = [d for d in K.LN_D if K.ln_per(d) == per]
        assert any(K.ln_guard_fires(d) for d in ds) and any(not K.ln_guard_fires(d) for d in ds), per
    assert any(d % 64 not in (0, 1, 63) for d in K.LN_D)                               # (1000: a partly filled last register)
    assert K.LN_REFUSED_D == K.LN_BOUNDS[2] + 1
    launches = [K.row_kernel_launch(r) for r in K.LN_ROWS]
    assert launches[0] == (1, 3) and launches[1][0] == 2 and launches[1][1] > 0 and launches[2][0] > 4 and launches[2][1] > 0
    for rows in (K.ARGMAX_ROWS, K.PN_ROWS):
        ls = [K.row_kernel_launch(r) for r in rows]
        assert ls[0] == (1, 3) and ls[1][0] == 2 and ls[1][1] > 0 and ls[2][0] > 4 and ls[2][1] > 0


def test_token_mix_cases_cover_the_masks_and_the_ragged_workgroup():
    launches = {c: K.token_mix_launch(c[0], c[2]) for c in K.TM_CASES}
    assert any(c[1] == K.TM_MAX_T for c in K.TM_CASES) and sum(c[1] < K.TM_MAX_T for c in K.TM_CASES) >= 4          # `t < T` masks
    assert any(c[1] == 1 for c in K.TM_CASES) and any(c[1] == K.TM_MAX_T - 1 for c in K.TM_CASES)
    assert any(tot < K.WG for tot, _, _ in launches.values())                                                       # under one workgroup
    assert any(wgs > 1 and idle > 0 for _, wgs, idle in launches.values())                                          # ragged last workgroup
    assert any(wgs > 1 and idle == 0 for _, wgs, idle in launches.values())                                         # the full one of the old test
    assert launches[(2, 63, 129, 16)] == (258, 2, 254) and launches[(3, 37, 300, 5)] == (900, 4, 124)
    assert any(c[3] == 1 for c in K.TM_CASES) and K.TM_REFUSED_T == K.TM_MAX_T + 1


def test_gather_and_embed_cases_reach_the_second_trip():
    sr, ld, col0, ncols, nidx = K.GATHER_TWO_TRIPS
    total, blocks, trips = K.gather_launch(nidx, ncols)
    assert (total, blocks, trips) == (2099200, K.GATHER_CAP, 2) and total > K.GATHER_CAP * K.WG and total % (K.GATHER_CAP * K.WG) != 0
    assert col0 > 0 and col0 + ncols < ld
    for sr, ld, col0, ncols, nidx in K.GATHER_SMALL:
        n = ld - col0 if ncols is None else ncols
        assert K.gather_launch(nidx or sr, n)[2] == 1 and col0 + n <= ld
    assert any(c[3] == 1 for c in K.GATHER_SMALL)
    N, nc, C = K.EMBED_TWO_TRIPS
    total, blocks, trips = K.embed_launch(N, nc, C, "fp32")
    assert (total, blocks, trips) == (4259840, K.EMBED_CAP, 2) and total % (K.EMBED_CAP * K.WG) != 0
    assert 60e6 < N * 4 * 4 * nc * C * 4 < 75e6                                        # the largest allocation of the GPU tier
    for N, nc, C in K.EMBED_CASES:
        for s in K.STORAGES:
            assert K.embed_launch(N, nc, C, s)[2] == 1 and C % 32 == 0
        emb, labels, scale = K.embed_case(N, nc, C)
        assert labels.min().item() == 0 and labels.max().item() == K.EMBED_CLASSES - 1
    emb, labels, scale = K.embed_two_trip_inputs()
    assert 0 <= labels.min().item() and labels.max().item() == K.EMBED_CLASSES - 1 and labels.shape == (130, 16)
    assert {nc for _, nc, _ in K.EMBED_CASES} == {1, 2, 16} and {C for _, _, C in K.EMBED_CASES} == {64, 512}
    ref = K.embed_host(emb[:, :8], labels[:2])
    assert ref.shape == (2, 4, 64, 8) and torch.equal(ref[1, 3, 4 * 5 + 2], emb[labels[1, 5], :8])


def test_demod_cases_hit_the_quarter_split():
    q = {cin: K.demod_quarters(cin) for cin in K.DEMOD_CIN}
    assert q[1] == [(0, 1), (1, 1), (2, 1), (3, 1)] and q[5] == [(0, 2), (2, 4), (4, 5), (6, 5)]      # empty quarters, i0 beyond cin
    assert q[3] == [(0, 1), (1, 2), (2, 3), (3, 3)]
    assert q[64] == [(0, 16), (16, 32), (32, 48), (48, 64)]                            # exactly one 16-wide step, no tail
    assert q[63][3] == (48, 63) and q[65][0] == (0, 17) and q[65][3] == (51, 65)      # 16 + a tail of 1; the last quarter shorter
    assert q[515][0] == (0, 129) and q[515][3] == (387, 515)                          # 8 steps + a tail of 1 / 8 steps
    for cin, qs in q.items():
        assert sum(max(0, b - a) for a, b in qs) == cin
    assert any(c < 64 for c in K.DEMOD_COUT) and any(c % 64 not in (0, 1, 63) for c in K.DEMOD_COUT) and 64 in K.DEMOD_COUT
    style, wsq_t, eps_scale = K.demod_case(9, 17, 65)
    assert float(style[0].abs().max()) == 0.0 and bool((wsq_t > 0).all())
    assert bool((torch.frexp(eps_scale).mantissa == 0.5).all()) and len(set(eps_scale.tolist())) > 2          # powers of two, several
    ref = K.demod_formula(style, wsq_t, eps_scale)
    assert torch.allclose(ref[0], (1 / torch.sqrt(1e-8 * eps_scale[0].double())).expand(65), rtol=1e-12)


@pytest.mark.parametrize("ncols", K.STYLE_NCOLS)
def test_style_cases_put_the_maximum_in_every_wave(ncols):
    src, idx, plan = K.style_case(ncols)
    pos = K.style_positions(ncols)
    assert ncols - 1 in pos
    waves = {(c % 256) >> 6 for c in pos}
    assert waves == set(range(min(4, (ncols + 63) // 64)))                             # every wave that owns a column holds the maximum in turn
    assert (ncols > 256) == any(c >= 256 for c in pos)                                 # ... and the second trip of the column loop where there is one
    c0, ld = K.STYLE_COL0, src.shape[1]
    assert c0 > 0 and ld > c0 + ncols and src.shape[0] == len(plan)
    win = src[:, c0:c0 + ncols]
    for r, (c, M) in enumerate(plan):
        m32 = torch.tensor(M, dtype=F32).item()
        inside = win[r].abs()
        outside = torch.cat([src[r, :c0], src[r, c0 + ncols:]]).abs()
        assert outside.min().item() > inside.max().item() or (M == 0.0 and outside.min().item() > 0)       # larger values outside the window
        if c is None:
            assert inside.max().item() == 0.0
            continue
        assert inside.max().item() == m32 and inside.argmax().item() == c and win[r, c].item() == (-m32 if r % 2 else m32)
        rest = inside.clone()
        rest[c] = 0
        assert rest.max().item() < 0.5 * m32                                           # losing the maximum changes the exponent
        assert m32 >= 2.0 ** -63
    used = {c for c, _ in plan if c is not None}
    assert used == set(pos)
    mags = [M for _, M in plan]
    assert 0.5 in mags and 1.0 in mags and min(m for m in mags if m) <= 1e-6 and max(mags) >= 4e6
    assert any(r % 2 == 1 and c is not None for r, (c, _) in enumerate(plan))         # negative maxima
    assert len(set(idx.tolist())) < idx.numel() and set(idx.tolist()) == set(range(src.shape[0]))            # repeats, every row
    rows, eps, sb, e = K.style_host(src, c0, ncols, idx, 3)
    nz = rows.abs().amax(1) > 0
    assert bool(((rows.abs().amax(1)[nz] >= 0.5) & (rows.abs().amax(1)[nz] < 1.0)).all()) and int((~nz).sum()) >= 3          # (the zero row, three times or more)
    assert torch.equal(rows.double() * torch.exp2(e.double())[:, None], src[idx][:, c0:c0 + ncols].double())    # the scaling is exact
    assert torch.equal(eps, torch.exp2(-2 * e)) and bool(torch.isfinite(eps).all()) and sb.shape == (idx.numel(), 3)
    assert {0.0, 1.0} <= set(e.tolist())                                               # exactly 0.5 -> e = 0, exactly 1.0 -> e = 1
    assert 0 in K.STYLE_BCAST and max(K.STYLE_BCAST) > K.WG


# ====================================================================================================================== layernorm
@pytest.mark.parametrize("D", K.LN_D)
def test_layernorm_fp32_formula_within_a_quarter_of_the_tolerance(D):
    for rows in K.LN_ROWS:
        for kind in K.LN_KINDS:
            x, g, b, eps = K.ln_case(kind, rows, D)
            ref = K.layernorm_formula(x, g, b, eps)
            assert bool(torch.isfinite(ref).all())
            err = K.row_error(K.layernorm_formula(x, g, b, eps, F32), ref)
            assert err <= K.QUARTER, (kind, rows, D, err)
            if kind == "constant":
                assert torch.equal(ref, b.double().expand(rows, D))
            if kind == "grid":                                                         # the row sums are exact in fp32 in any order
                k16 = x.double() * 16
                assert torch.equal(k16, k16.round()) and float(k16.abs().max()) * D < 2 ** 24
                assert torch.equal(x.sum(-1).double(), x.double().sum(-1)) and torch.equal(x.flip(-1).cumsum(-1)[:, -1].double(), x.double().sum(-1))
                k = k16 - 16 * K.ln_grid_offset(D)
                assert float(k.min()) >= -8 and float(k.max()) <= 8


def test_layernorm_hazard_cases_bite():
    worst = {}
    for D in (64, 512, 1024):                                                          # one-pass variance on the offset-64 grid rows
        assert K.ln_grid_offset(D) == 64.0
        x, g, b, eps = K.ln_case("grid", 130, D)
        err = K.row_error(K.layernorm_formula(x, g, b, eps, F32, variance="one-pass"), K.layernorm_formula(x, g, b, eps))
        worst["one-pass %d" % D] = err
        assert _misses(err), (D, err)
    for D in (63, 512, 1000):                                                          # eps ignored / wrong on rows of std 0.003
        for kind, true_eps in (("lowstd", 1e-5), ("lowstd-eps1e-3", 1e-3)):
            x, g, b, eps = K.ln_case(kind, 5, D)
            assert eps == true_eps and abs(float(x.std()) - K.LN_LOW_STD) < 0.001
            ref = K.layernorm_formula(x, g, b, eps)
            for wrong in (0.0, 1e-6, 1e-5 if true_eps != 1e-5 else 1e-4):
                err = K.row_error(K.layernorm_formula(x, g, b, wrong, F32), ref)
                worst["eps %g for %g, D=%d" % (wrong, true_eps, D)] = err
                assert _misses(err), (D, kind, wrong, err)
    for D in (512, 513, 1000, 1024):                                                   # unbiased variance
        x, g, b, eps = K.ln_case("normal", 5, D)
        err = K.row_error(K.layernorm_formula(x, g, b, eps, F32, variance="unbiased"), K.layernorm_formula(x, g, b, eps))
        worst["unbiased %d" % D] = err
        assert _misses(err), (D, err)
    print(worst)


# ====================================================================================================================== token_mix
@pytest.mark.parametrize("case", K.TM_CASES, ids=["%dx%dx%dx%d" % c for c in K.TM_CASES])
def test_token_mix_fp32_formula_and_bite(case):
    B, T, D, J = case
    x, lg, lb, W, bias = K.tm_case(*case)
    ref = K.token_mix_formula(x, lg, lb, W, bias, K.TM_EPS)
    assert ref.shape == (B, J, D)
    err = K.row_error(K.token_mix_formula(x, lg, lb, W, bias, K.TM_EPS, F32), ref, row_dims=2)
    assert err <= K.QUARTER, (case, err)
    if T >= 16:                                                                        # eps decides on the low-variance columns
        var = x.double().var(1, unbiased=False)
        assert bool((var[:, 1::2] < 3e-5).all()) and bool((var[:, 0::2] > 0.1).all())
        e0 = K.row_error(K.token_mix_formula(x, lg, lb, W, bias, 0.0, F32), ref, row_dims=2)
        assert _misses(e0), (case, e0)
    if 1 < T < K.TM_MAX_T:                                                             # a statistics loop that runs one token too far
        e1 = K.row_error(K.token_mix_formula(x, lg, lb, W, bias, K.TM_EPS, F32, extra_zero_token=True), ref, row_dims=2)
        assert _misses(e1), (case, e1)


# ====================================================================================================================== attention
@pytest.mark.parametrize("N", K.ATT_N)
def test_attention_cases_exact_scores_fp32_formula_and_bite(N):
    cases = K.att_cases(N)
    assert {kind for _, _, _, kind in cases} == set(K.ATT_KINDS)
    assert {(B, H) for B, H, _, _ in cases} == ({(3, 8)} if N in (64, 16) else {(1, 1), (2, 3)})
    for B, H, scale, kind in cases:
        qkv, marks = K.att_case(kind, B, N, H)
        assert qkv.shape == (B, N, 3 * H * 64)
        assert torch.tensor(scale, dtype=F32).item() == scale                          # the wrapper passes this very value
        ref = K.attention_formula(qkv, B, N, H, scale)
        err = K.row_error(K.attention_formula(qkv, B, N, H, scale, F32), ref)
        assert err <= K.QUARTER, (N, B, H, scale, kind, err)
        if kind == "random":
            continue
        s64 = K.attention_scores(qkv, B, N, H, F64)
        s32 = K.attention_scores(qkv, B, N, H, F32)
        sflip = K.attention_scores(qkv.reshape(B, N, 3 * H, 64).flip(-1).reshape(B, N, -1), B, N, H, F32)     # another summation order
        assert torch.equal(s32.double(), s64) and torch.equal(sflip.double(), s64) and torch.equal(s64, s64.round())
        qk = qkv.reshape(B, N, 3, H, 64)[:, :, :2]
        assert torch.equal(qk, qk.round()) and float(qk.abs().max()) == 4.0 and float(s64.abs().max()) <= K.ATT_PLANTED_SCORE
        out = ref.reshape(B, N, H, 64)
        nomax = K.attention_formula(qkv, B, N, H, scale, F32, subtract_max=False).reshape(B, N, H, 64)
        for b, h, i, score in marks:
            row = s64[b, h, i]
            assert float(row.max() if score > 0 else row.min()) == score and abs(score * scale) >= 128
            assert not bool(torch.isfinite(nomax[b, i, h]).all())                       # exp overflows / the whole row underflows: NaN
            if kind == "planted":                                                      # ... on an early key and on the last valid key
                assert {int(s64[0, 0, N // 2].argmax()), int(s64[0, 0, 0].argmax())} == {0, N - 1}
        if kind == "equal-keys":
            b, h = B - 1, H - 1
            assert bool((row == score).all())                                          # the whole row at -1024 (N = 1) or the rows at +-1024
            v = qkv.double().reshape(B, N, 3, H, 64)[b, :, 2, h]
            assert torch.allclose(out[b, :, h], v.mean(0).expand(N, 64), rtol=0, atol=1e-12)                  # the output is the mean of v
            if N < K.ATT_MAX_N:                                                        # a mask that lets key N through: the row at -1024 loses its maximum
                e = K.row_error(K.attention_formula(qkv, B, N, H, scale, F32, extra_zero_key=True), ref)
                assert _misses(e), (N, e)
        assert _misses(K.row_error(nomax.reshape(B * N, H * 64), ref))
    if N < K.ATT_MAX_N:                                                                # random inputs catch the extra key as well
        B, H, scale, _ = cases[0]
        qkv, _ = K.att_case("random", B, N, H)
        e = K.row_error(K.attention_formula(qkv, B, N, H, scale, F32, extra_zero_key=True), K.attention_formula(qkv, B, N, H, scale))
        assert _misses(e), (N, e)
    assert K.ATT_REFUSED_N == K.ATT_MAX_N + 1


# ====================================================================================================================== argmax_rows
@pytest.mark.parametrize("D", K.ARGMAX_D)
def test_argmax_cases_are_what_they_claim(D):
    for rows in K.ARGMAX_ROWS:
        cases = K.argmax_cases(D, rows)
        assert sum(x.shape[0] for x, _ in cases) >= len(K.ARGMAX_KINDS)
        for x, want in cases:
            assert x.shape == (rows, D) and bool(((want >= 0) & (want < D)).all())
            assert torch.equal(torch.argmax(x, -1), want)                              # torch: NaN is the maximum, the first one wins
    g = K._gen(1)
    for kind in K.ARGMAX_KINDS:
        x, want = K.argmax_row(kind, D, g)
        nan, inf = torch.isnan(x), torch.isinf(x)
        if kind == "all -inf":
            assert bool((x == -math.inf).all())
        if kind == "all NaN":
            assert bool(nan.all())
        if kind == "NaN with +inf" and D > 2:
            assert int(nan.sum()) == 1 and bool((x == math.inf).any()) and int((x == math.inf).nonzero()[0]) < want
        if kind == "two NaNs" and D > 70:
            assert int(nan.sum()) == 3 and want % 64 > 70 % 64                         # the first NaN sits in a higher lane than the second
        if kind == "tie across lanes" and D > 70:
            assert int((x == x[want]).sum()) == 3 and want % 64 > 70 % 64
        if kind == "tie within a lane" and D > 64:
            assert bool((x[want::64] == x[want]).all()) and int((x == x[want]).sum()) == len(range(want, D, 64)) >= 2
        if kind == "max at a lane's second element" and D > 71:
            assert 64 <= want < 128
        if kind == "all negative":
            assert bool((x < 0).all())
        if kind == "one NaN among finite values":
            assert int(nan.sum()) == 1 and not bool(inf.any()) and (D == 1 or x[0] == 50.0)


# ====================================================================================================================== pixelnorm, demod, pack_wsq
@pytest.mark.parametrize("D", K.PN_D)
def test_pixelnorm_fp32_formula_and_bite(D):
    seen = set()
    for rows in K.PN_ROWS:
        for shift in range(3):
            x, kinds = K.pn_case(rows, D, shift)
            seen |= {(rows, kd) for kd in kinds}
            ref = K.pixelnorm_formula(x)
            err = K.row_error(K.pixelnorm_formula(x, F32), ref)
            assert err <= K.QUARTER, (rows, D, shift, err)
            for r, kd in enumerate(kinds):
                if kd == "zero":
                    assert float(x[r].abs().max()) == 0.0 and float(ref[r].abs().max()) == 0.0
                if kd == "tiny":                                                       # eps decides: without it the row is off several-fold
                    assert float((x[r].double() ** 2).mean()) < 1e-8 / 10
                    e = K.row_error(K.pixelnorm_formula(x[r:r + 1], F32, eps=0.0), ref[r:r + 1])
                    assert e > 1.0, (rows, D, r, e)
    assert seen == {(rows, kd) for rows in K.PN_ROWS for kd in K.PN_KINDS}


@pytest.mark.parametrize("cin", K.DEMOD_CIN)
def test_demod_fp32_formula_within_a_quarter_of_the_tolerance(cin):
    for cout in K.DEMOD_COUT:
        for N in K.DEMOD_N:
            style, wsq_t, eps_scale = K.demod_case(N, cin, cout)
            for es in (None, eps_scale):
                ref = K.demod_formula(style, wsq_t, es)
                err = K.elementwise_error(K.demod_formula(style, wsq_t, es, F32), ref)
                assert err <= K.QUARTER, (cin, cout, N, err)
            if N > 1:                                                                  # the eps term decides on rows 0 and (small cin) 1
                no_eps = K.demod_formula(style[1:], wsq_t, eps_scale[1:] * 0, F32)
                if cin <= 17:
                    assert _misses(K.elementwise_error(no_eps[:1], K.demod_formula(style[1:2], wsq_t, eps_scale[1:2])))


def test_pack_wsq_fp32_formula_within_a_quarter_of_the_tolerance():
    assert {k[0] * k[1] for _, _, k in K.WSQ_CASES} == {1, 9}
    for cout, cin, k in K.WSQ_CASES:
        w, scale = K.wsq_case(cout, cin, k)
        ref = K.pack_wsq_formula(w, scale)
        assert ref.shape == (cin, cout)
        assert K.elementwise_error(K.pack_wsq_formula(w, scale, F32), ref) <= K.QUARTER


def test_the_metric_itself():
    ref = torch.tensor([[1.0, -2.0], [0.0, 0.0], [2.0 ** -10, 0.0]], dtype=F64)
    assert K.row_error(ref.float(), ref) == 0.0
    got = ref.clone()
    got[2, 1] = 2.0 ** -27                                                             # 2^-17 of ITS row's maximum, 2^-28 of the tensor's
    assert K.row_error(got, ref) == 2.0 ** -17
    got[1, 0] = 1e-30
    assert K.row_error(got, ref) == math.inf                                           # an all-zero reference row has to be exact
    got = ref.clone()
    got[0, 0] = math.nan
    assert K.row_error(got, ref) == math.inf
    assert K.row_error(ref.reshape(1, 3, 2) * 1.0, ref.reshape(1, 3, 2), row_dims=2) == 0.0
    pos = torch.tensor([1.0, 1e-6], dtype=F64)
    assert abs(K.elementwise_error(pos * (1 + 1e-5), pos) - 1e-5) < 1e-10
    assert re.match(r"2e-0?5", "%g" % K.TOL) and K.QUARTER == 5e-6
