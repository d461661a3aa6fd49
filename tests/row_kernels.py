"""The TextViT helpers (csrc/vit_kernels.hip: layernorm, token_mix, attention, argmax_rows) and the fp32 style path (pixelnorm, demod, embed_gather of
csrc/aux_kernels.hip; style_rows, gather_rows, pack_wsq of csrc/pack_kernels.hip) as data: the case tables of tests/test_row_kernels_gpu.py, the input
builders, small mirrors of the host launch arithmetic, and the references.  No device use: tests/test_row_kernels.py proves on a CPU that every case is
what it claims to be (regimes reached, sums and scores exact, the reference precise enough, the hazard it is there for really biting).

References.  Every floating-point reference is the op's formula WRITTEN OUT below and evaluated in fp64 (`dtype=torch.float64`); the same function
evaluated with `dtype=torch.float32` is the "plain fp32 evaluation" whose distance to fp64 has to stay within a quarter of the tolerance, and its
named wrong variants (one-pass variance, no eps, no max subtraction, ...) are the formulas a subtly wrong kernel would compute.  No ATen fp32
normalisation op is a reference (F.layer_norm evaluates x * scale + bias and is off by 1.7e-5 on large-mean rows).

Metric.  fp32 outputs: per row |got - ref64| <= TOL * max|ref64 over that row| (`row_error`; the row is the normalised axis — one output row for
layernorm / pixelnorm / attention, the [J, D] slice of one batch item for token_mix).  demod / pack_wsq sum non-negative terms only: elementwise
relative error <= TOL (`elementwise_error`).  Copies, gathers, power-of-two scalings and indices: torch.equal.

Known limit, style_rows: row magnitudes below 2^-63 are left out — eps_scale = 4^-e overflows there, and that range is not the pipeline's."""
import functools
import math

import numpy as np
import torch

TOL = 2e-5                    # the project's fp32 figure (`_tol` of tests/test_kernels_gpu.py), applied per row
QUARTER = TOL / 4             # plain fp32 evaluation vs fp64: leaves a kernel a factor 4 for its own summation order
BITE = 10 * TOL               # a named wrong formula has to miss by at least this much
WG = 256                      # threads per workgroup of every kernel here
F64, F32 = torch.float64, torch.float32


def _cdiv(a, b):
    return (a + b - 1) // b


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, g):
    return torch.randn(shape, generator=g)


# ================================================================================================================ metric
def row_error(got, ref, row_dims=1):
    """max over rows of max|got - ref| / max|ref| (the last `row_dims` dimensions are one row); a row whose reference is all zeros has to be exact
    zeros; NaN / inf anywhere in `got` where the reference is finite -> inf"""
    n = int(np.prod(ref.shape[-row_dims:]))
    g, r = got.double().reshape(-1, n), ref.double().reshape(-1, n)
    assert g.shape == r.shape and bool(torch.isfinite(r).all())
    d = torch.nan_to_num((g - r).abs(), nan=math.inf).amax(1)
    m = r.abs().amax(1)
    rel = torch.where(m > 0, d / m.clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, math.inf)))
    return rel.max().item()


def elementwise_error(got, ref):
    """max |got - ref| / |ref| (the reference is positive everywhere)"""
    g, r = got.double(), ref.double()
    assert g.shape == r.shape and bool((r > 0).all()) and bool(torch.isfinite(r).all())
    return torch.nan_to_num((g - r).abs() / r, nan=math.inf).max().item()


# ================================================================================================================ launch mirrors
# vit_kernels.hip, mnet_layernorm: `if (d <= 64) ...<1>  else if (d <= 512) ...<8>  else ...<16>`, refused beyond `d <= 1024`
LN_BOUNDS, LN_PER = (64, 512, 1024), (1, 8, 16)
ROWS_PER_WG = 4               # layernorm / argmax / pixelnorm: `row = blockIdx.x * 4 + (threadIdx.x >> 6)`, grid `(rows + 3) / 4`: four waves, a row each
ATT_MAX_N, TM_MAX_T = 64, 64  # mnet_attention `N <= 64`, mnet_token_mix `T <= 64`
GATHER_CAP, EMBED_CAP = 8192, 16384


def ln_per(d):
    """values per lane of the layernorm_kernel<PER> the wrapper launches for width d"""
    assert 0 < d <= LN_BOUNDS[2]
    return LN_PER[0] if d <= LN_BOUNDS[0] else LN_PER[1] if d <= LN_BOUNDS[1] else LN_PER[2]


def ln_guard_fires(d):
    """some `c < D` guard of the launched kernel is false for some lane"""
    return d < 64 * ln_per(d)


def row_kernel_launch(rows):
    """-> (workgroups, waves of the last workgroup without a row) of the one-wave-per-row kernels"""
    wgs = _cdiv(rows, ROWS_PER_WG)
    return wgs, wgs * ROWS_PER_WG - rows


def token_mix_launch(B, D):
    """-> (threads with work, workgroups, threads of the last workgroup beyond B*D) — `dim3((tot + 255) / 256)`, `if (id >= B * D) return;`"""
    tot = B * D
    wgs = _cdiv(tot, WG)
    return tot, wgs, wgs * WG - tot


def gather_launch(rows, ncols):
    """-> (elements, workgroups, trips) of mnet_gather_rows: `(total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192`, grid-stride loop"""
    total = rows * ncols
    blocks = min(_cdiv(total, WG), GATHER_CAP)
    return total, blocks, _cdiv(total, blocks * WG)


def chunk_n(storage):
    """channels per 16-byte chunk (common.h chunk_n): 4 in fp32, 8 in every other storage"""
    return 4 if storage == "fp32" else 8


def embed_launch(n, nc, c, storage):
    """-> (chunks, workgroups, trips) of mnet_embed_gather_scaled: `total = N_ * 16 * nc * (C / N)`, cap 16384"""
    total = n * 16 * nc * (c // chunk_n(storage))
    blocks = min(_cdiv(total, WG), EMBED_CAP)
    return total, blocks, _cdiv(total, blocks * WG)


def demod_quarters(cin):
    """[(i0, i1)] of the four waves of demod_kernel: `per = (cin + 3) >> 2, i0 = q * per, i1 = min(cin, i0 + per)` (i1 <= i0: an empty quarter)"""
    per = (cin + 3) >> 2
    return [(q * per, min(cin, q * per + per)) for q in range(4)]


# ================================================================================================================ layernorm
def layernorm_formula(x, gamma, beta, eps, dtype=F64, variance="two-pass"):
    """mean, biased variance, (x - mean) / sqrt(var + eps) * gamma + beta.  Wrong variants: "one-pass" E[x^2] - mean^2, "unbiased" / (D - 1)"""
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    D = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / D
    if variance == "one-pass":
        var = (x * x).sum(-1, keepdim=True) / D - mean * mean
    elif variance == "unbiased":
        var = ((x - mean) ** 2).sum(-1, keepdim=True) / (D - 1)
    else:
        var = ((x - mean) ** 2).sum(-1, keepdim=True) / D
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


LN_D = (1, 63, 64, 65, 511, 512, 513, 1000, 1024)
LN_ROWS = (1, 5, 130)          # under one workgroup, rows % 4 != 0, many workgroups
LN_KINDS = ("normal", "grid", "lowstd", "lowstd-eps1e-3", "constant")
LN_REFUSED_D = 1025
LN_LOW_STD = 0.003


def ln_grid_offset(D):
    """grid rows offset + k/16: 64 at the widths where the mean is exact (D a power of two), 8 at ragged widths, where the rounded mean of a plain
    fp32 evaluation already costs more than a quarter of the tolerance at offset 64"""
    return 64.0 if D in (64, 512, 1024) else 8.0


def ln_case(kind, rows, D):
    """-> (x [rows, D], gamma [D], beta [D], eps)"""
    g = _gen(1000 + 7 * D + rows + 100003 * LN_KINDS.index(kind))
    gamma, beta = 1 + 0.1 * _randn((D,), g), 0.1 * _randn((D,), g)
    eps = 1e-5
    if kind == "normal":                                       # N(1, 9)
        x = _randn((rows, D), g) * 3 + 1
    elif kind == "grid":                                       # offset + k/16, integer k in [-8, 8]: every partial sum is exact in fp32
        x = ln_grid_offset(D) + torch.randint(-8, 9, (rows, D), generator=g).float() / 16
    elif kind in ("lowstd", "lowstd-eps1e-3"):                 # variance 9e-6: eps = 1e-5 is half of the denominator
        x = LN_LOW_STD * _randn((rows, D), g)
        eps = 1e-3 if kind == "lowstd-eps1e-3" else 1e-5
    elif kind == "constant":                                   # variance 0: the output is beta, finite
        x = ((torch.arange(rows) % 7).float() - 3.0)[:, None] * 0.75 + torch.full((rows, D), 0.125)
    else:
        raise KeyError(kind)
    return x.contiguous(), gamma, beta, eps


# ================================================================================================================ token_mix
def token_mix_formula(x, ln_g, ln_b, wgt, bias, eps, dtype=F64, extra_zero_token=False):
    """x [B, T, D]: LayerNorm over the T tokens of every (b, d) with ln_g / ln_b [T], then Linear(T -> J): y[b, j, d] = sum_t v[t] W[j, t] + bias[j].
    Wrong variant `extra_zero_token`: the variance sum runs over one token too many (a zero that contributes mean^2)"""
    x, ln_g, ln_b, wgt, bias = [t.to(dtype) for t in (x, ln_g, ln_b, wgt, bias)]
    T = x.shape[1]
    xt = x.permute(0, 2, 1)                                    # [B, D, T]
    mean = xt.sum(-1, keepdim=True) / T
    q = ((xt - mean) ** 2).sum(-1, keepdim=True)
    if extra_zero_token:
        q = q + mean * mean
    v = (xt - mean) / torch.sqrt(q / T + eps) * ln_g + ln_b
    y = (v[:, :, None, :] * wgt[None, None, :, :]).sum(-1) + bias            # [B, D, J]
    return y.permute(0, 2, 1).contiguous()


TM_CASES = ((3, 64, 512, 16), (3, 64, 512, 1), (1, 1, 7, 2), (3, 16, 100, 3), (3, 37, 300, 5), (2, 63, 129, 16))       # (B, T, D, J)
TM_REFUSED_T = 65
TM_EPS = 1e-5


def tm_case(B, T, D, J):
    """-> (x [B, T, D], ln_g [T], ln_b [T], W [J, T], bias [J]).  Column d has its own offset; odd columns have a spread of 0.003 (variance 9e-6
    against eps 1e-5) around a small offset, even columns a spread of 1 around an offset of order 2"""
    g = _gen(2000 + 13 * T + D + 1009 * J)
    low = (torch.arange(D) % 2 == 1)
    sig = torch.where(low, torch.tensor(0.003), torch.tensor(1.0))
    off = _randn((D,), g) * torch.where(low, torch.tensor(0.01), torch.tensor(2.0))
    x = off + sig * _randn((B, T, D), g)
    return x.contiguous(), 1 + 0.1 * _randn((T,), g), 0.1 * _randn((T,), g), 0.125 * _randn((J, T), g), 0.1 * _randn((J,), g)


# ================================================================================================================ attention
def attention_formula(qkv, B, N, H, scale, dtype=F64, subtract_max=True, extra_zero_key=False):
    """qkv [B, N, 3 * H * 64] (q | k | v, each H heads of 64) -> softmax(q k^T * scale) v as [B * N, H * 64].  Wrong variants: `subtract_max=False`
    (exp of the raw scores), `extra_zero_key` (one key too many: score 0, value 0 — what a mask that lets key N through computes)"""
    t = qkv.to(dtype).reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)         # [3, B, H, N, 64]
    q, k, v = t[0], t[1], t[2]
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    if extra_zero_key:
        s = torch.cat([s, torch.zeros_like(s[..., :1])], dim=-1)
        v = torch.cat([v, torch.zeros_like(v[..., :1, :])], dim=-2)
    if subtract_max:
        s = s - s.amax(-1, keepdim=True)
    e = torch.exp(s)
    p = e / e.sum(-1, keepdim=True)
    return torch.matmul(p, v).permute(0, 2, 1, 3).reshape(B * N, H * 64)


def attention_scores(qkv, B, N, H, dtype):
    """q k^T before the scale, [B, H, N, N]"""
    t = qkv.to(dtype).reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    return torch.matmul(t[0], t[1].transpose(-1, -2))


ATT_N = (1, 5, 15, 16, 17, 32, 33, 48, 49, 63, 64)
ATT_KINDS = ("random", "planted", "equal-keys")
ATT_SCALE_48 = float(np.float32(1 / math.sqrt(48)))           # the fp32 value the wrapper passes
ATT_REFUSED_N = 65
ATT_PLANTED_SCORE = 1024                                       # 64 * 4 * 4: +-128 at scale 0.125


def att_cases(N):
    """[(B, H, scale, kind)] for sequence length N: (3, 8) at the TextViT's two lengths, (1, 1) and (2, 3) elsewhere; scale 0.125, with 0.25 and
    1/sqrt(48) at four lengths (inside a 16-key block, one past a block border, on a border, full)"""
    shapes = ((3, 8),) if N in (64, 16) else ((1, 1), (2, 3))
    out = [(B, H, 0.125, kind) for B, H in shapes for kind in ATT_KINDS]
    if N in (5, 17, 48, 64):
        B, H = shapes[-1]
        out += [(B, H, sc, kind) for sc in (0.25, ATT_SCALE_48) for kind in ATT_KINDS]
    return out


def _assemble_qkv(q, k, v):
    """[B, H, N, 64] x 3 -> [B, N, 3 * H * 64]"""
    B, H, N, _ = q.shape
    return torch.stack([q, k, v]).permute(1, 3, 0, 2, 4).reshape(B, N, 3 * H * 64).contiguous()


def att_case(kind, B, N, H):
    """-> (qkv, marks): marks = [(b, h, query row, score before the scale)] of the planted rows.
    random: N(0, 1).  planted / equal-keys: q and k integers in [-4, 4] (every score an exact fp32 integer in any summation order), v N(0, 1), and
      planted:    in head (0, 0), q[N // 2] = k[0] = 4 p and q[0] = k[N - 1] = 4 p' for sign patterns p, p': score +1024 on an early key and on the
                  last valid key
      equal-keys: every key of the last head is 4 p (each output row of that head is the mean of v); its query row 0 is 4 p (a whole row at +1024),
                  its query row N - 1 is -4 p (a whole row at -1024)"""
    g = _gen(3000 + 17 * N + 5 * B + H + 101 * ATT_KINDS.index(kind))
    v = _randn((B, H, N, 64), g)
    if kind == "random":
        return _assemble_qkv(_randn((B, H, N, 64), g), _randn((B, H, N, 64), g), v), []
    q = torch.randint(-4, 5, (B, H, N, 64), generator=g).float()
    k = torch.randint(-4, 5, (B, H, N, 64), generator=g).float()
    p = 4.0 * (torch.randint(0, 2, (2, 64), generator=g).float() * 2 - 1)
    if kind == "planted":
        q[0, 0, N // 2], k[0, 0, 0] = p[0], p[0]
        q[0, 0, 0], k[0, 0, N - 1] = p[1], p[1]                # (N = 1: the one query and the one key)
        marks = [(0, 0, N // 2, ATT_PLANTED_SCORE), (0, 0, 0, ATT_PLANTED_SCORE)]
    elif kind == "equal-keys":
        k[B - 1, H - 1] = p[0]
        q[B - 1, H - 1, 0] = p[0]
        q[B - 1, H - 1, N - 1] = -p[0]                         # (N = 1: the one row sits at -1024)
        marks = [(B - 1, H - 1, N - 1, -ATT_PLANTED_SCORE)] + ([(B - 1, H - 1, 0, ATT_PLANTED_SCORE)] if N > 1 else [])
    else:
        raise KeyError(kind)
    return _assemble_qkv(q, k, v), marks


# ================================================================================================================ argmax_rows
ARGMAX_D = (1, 63, 64, 65, 6736)
ARGMAX_ROWS = (1, 5, 70)
ARGMAX_KINDS = ("max at 0", "max at D-1", "max at a lane's second element", "tie within a lane", "tie across lanes", "all equal", "all negative",
                "+inf present", "all -inf", "one NaN among finite values", "NaN with +inf", "two NaNs", "all NaN", "-inf row with one finite value")


def argmax_row(kind, D, g):
    """-> (row [D], the index torch.argmax has to give).  Lane l of the kernel's wave holds the elements l, l + 64, ..."""
    x = _randn((D,), g)                                        # |x| < 6
    big = 50.0
    last = D - 1
    if kind == "max at 0":
        x[0] = big
        want = 0
    elif kind == "max at D-1":
        x[last] = big
        want = last
    elif kind == "max at a lane's second element":
        want = min(64 + 7, last)
        x[want] = big
    elif kind == "tie within a lane":                          # i and i + 64, i + 128
        want = 5 if D > 69 else 0
        x[want::64] = big
    elif kind == "tie across lanes":                           # the lower index sits in the higher lane: 10 (lane 10) before 70 (lane 6)
        want = min(10, last)
        x[want] = x[min(70, last)] = x[last] = big
    elif kind == "all equal":
        x[:] = 1.25
        want = 0
    elif kind == "all negative":
        x = -x.abs() - 1.0
        want = min(40, last)
        x[want] = -0.5
    elif kind == "+inf present":
        want = D // 2
        x[want] = x[last] = math.inf
    elif kind == "all -inf":
        x[:] = -math.inf
        want = 0
    elif kind == "one NaN among finite values":
        want = (2 * D) // 3
        x[0] = big
        x[want] = math.nan
    elif kind == "NaN with +inf":                              # the NaN wins although +inf comes first
        want = (2 * D) // 3
        x[D // 3] = math.inf
        x[want] = math.nan
    elif kind == "two NaNs":                                   # the first wins: across lanes (10 before 70), and last
        want = min(10, last)
        x[want] = x[min(70, last)] = x[last] = math.nan
    elif kind == "all NaN":
        x[:] = math.nan
        want = 0
    elif kind == "-inf row with one finite value":
        x[:] = -math.inf
        want = (3 * D) // 4
        x[want] = -3.0e38
    else:
        raise KeyError(kind)
    return x, want


def argmax_cases(D, rows):
    """-> [(x [rows, D], want [rows])]: as many tensors of `rows` rows as it takes to run every kind once"""
    g = _gen(4000 + D + 31 * rows)
    out = []
    for first in range(0, len(ARGMAX_KINDS), rows):
        rs = [argmax_row(ARGMAX_KINDS[(first + r) % len(ARGMAX_KINDS)], D, g) for r in range(rows)]
        out.append((torch.stack([x for x, _ in rs]).contiguous(), torch.tensor([w for _, w in rs], dtype=torch.int64)))
    return out


# ================================================================================================================ pixelnorm
def pixelnorm_formula(x, dtype=F64, eps=1e-8):
    x = x.to(dtype)
    return x / torch.sqrt((x * x).sum(-1, keepdim=True) / x.shape[-1] + eps)


PN_D = (1, 63, 64, 65, 512, 515)
PN_ROWS = (1, 5, 37)
PN_KINDS = ("normal", "tiny", "zero")                          # N(0, 1); magnitude 1e-5 (x^2 = 1e-10 against eps 1e-8); all zeros


def pn_case(rows, D, shift):
    """-> (x [rows, D], kind per row): row r is of kind (r + shift) % 3, so that three shifts show every kind to every row count"""
    g = _gen(5000 + D + 11 * rows + shift)
    kinds = [PN_KINDS[(r + shift) % 3] for r in range(rows)]
    x = _randn((rows, D), g)
    for r, kd in enumerate(kinds):
        x[r] *= {"normal": 1.0, "tiny": 1e-5, "zero": 0.0}[kd]
    x[x == 0] = 0.0                                            # (no -0.0)
    return x.contiguous(), kinds


# ================================================================================================================ demod, pack_wsq
def demod_formula(style, wsq_t, eps_scale=None, dtype=F64):
    """1 / sqrt(sum_i style[n, i]^2 wsq_t[i, o] + 1e-8 * eps_scale[n])"""
    s, w = style.to(dtype), wsq_t.to(dtype)
    eps = 1e-8 * (torch.ones(s.shape[0], dtype=dtype) if eps_scale is None else eps_scale.to(dtype))
    return 1 / torch.sqrt(((s * s)[:, :, None] * w[None, :, :]).sum(1) + eps[:, None])


DEMOD_CIN = (1, 3, 5, 15, 16, 17, 63, 64, 65, 515)
DEMOD_COUT = (1, 63, 64, 65, 100)
DEMOD_N = (1, 9)


def demod_case(N, cin, cout):
    """-> (style [N, cin], wsq_t [cin, cout] >= 0, eps_scale [N] = 4^-e).  N = 9: row 0 is all zeros (the output is rsqrt(1e-8 * eps_scale)),
    row 1 has magnitude 1e-3 (the sum is of the order of the eps for a small cin)"""
    g = _gen(6000 + 3 * cin + 1013 * cout + N)
    style = _randn((N, cin), g) + 1.0
    if N > 1:
        style[0] = 0.0
        style[1] *= 1e-3
    wsq_t = _randn((cin, cout), g).abs() * 0.01 + 1e-6
    eps_scale = torch.exp2(-2.0 * torch.randint(-3, 4, (N,), generator=g).float())
    return style.contiguous(), wsq_t.contiguous(), eps_scale


def pack_wsq_formula(w, scale, dtype=F64):
    """wsq_t[i][o] = sum over the taps of (scale * W[o][i])^2"""
    w = w.to(dtype)
    return ((scale * w) ** 2).sum([2, 3]).t().contiguous()


WSQ_CASES = ((48, 24, (3, 3)), (5, 3, (1, 1)), (100, 515, (3, 3)))          # (cout, cin, (kh, kw)): khw = 9, 1, 9


def wsq_case(cout, cin, k):
    g = _gen(7000 + cout + 7 * cin)
    return (_randn((cout, cin) + tuple(k), g) * 0.1).contiguous(), 1 / math.sqrt(cin * k[0] * k[1])


# ================================================================================================================ style_rows
STYLE_NCOLS = (1, 64, 255, 256, 257, 512, 1000)
STYLE_BCAST = (0, 3, 300)
STYLE_MAGS = (1e-6, 0.5, 1.0, 37.0, 4.0e6, 0.26, 1e-3, 3.0e5, 2.0 ** -20, 1.9999999)
STYLE_COL0, STYLE_MARGIN = 7, 9                                # window [col0, col0 + ncols) inside rows of ld = col0 + ncols + margin


def style_positions(ncols):
    """columns the row maximum is placed at: one owned by each of the four waves (thread c % 256, wave (c % 256) >> 6), one reached only on the
    second trip of the `c += 256` loops, the last one"""
    want = [5, 64 + 5, 128 + 5, 192 + 5, 256 + 64 + 9, ncols - 1]
    return sorted({c for c in want if 0 <= c < ncols})


def style_host(src, col0, ncols, idx, bcast):
    """the host formula (tests/test_kernels_gpu.py::test_style_rows_and_scaled_demod): rows * 2^-e, 4^-e, 2^e with e = exponent of max|row window|
    (frexp: max * 2^-e in [0.5, 1)), e = 0 for an all-zero window.  Power-of-two factors: exact"""
    plain = (src if idx is None else src[idx])[:, col0:col0 + ncols]
    m = plain.abs().amax(dim=1)
    e = torch.where(m > 0, torch.frexp(m).exponent.float(), torch.zeros_like(m))
    sb = torch.exp2(e)[:, None].expand(plain.shape[0], bcast).contiguous() if bcast else None
    return plain * torch.exp2(-e)[:, None], torch.exp2(-2 * e), sb, e


def style_case(ncols):
    """-> (src [R, ld], idx with repeats, [(max column, magnitude)] per source row).  Row r: |values| <= 0.4 M inside the window except the one
    column that holds +-M (so that losing it changes the exponent), +-16 M ... 32 M outside the window; the last row is all zeros inside"""
    g = _gen(8000 + ncols)
    pos = style_positions(ncols)
    plan = [(pos[i % len(pos)], STYLE_MAGS[i % len(STYLE_MAGS)]) for i in range(max(len(STYLE_MAGS), 2 * len(pos)))]
    R, ld = len(plan) + 1, STYLE_COL0 + ncols + STYLE_MARGIN
    src = torch.empty((R, ld))
    for r, (c, M) in enumerate(plan):
        src[r] = (torch.rand((ld,), generator=g) * 16 + 16) * M * (torch.randint(0, 2, (ld,), generator=g).float() * 2 - 1)
        src[r, STYLE_COL0:STYLE_COL0 + ncols] = (torch.rand((ncols,), generator=g) * 0.8 - 0.4) * M
        src[r, STYLE_COL0 + c] = -M if r % 2 else M
    src[R - 1] = 1.0e7
    src[R - 1, STYLE_COL0:STYLE_COL0 + ncols] = 0.0
    perm = torch.randperm(R, generator=g)
    idx = torch.cat([perm, perm[:3], torch.tensor([R - 1, R - 1, 0])]).to(torch.int64)
    return src.contiguous(), idx, plan + [(None, 0.0)]


# ================================================================================================================ gather_rows
# (src rows, ld, col0, ncols or None for "to the end", index rows or None for "every row in order")
GATHER_SMALL = ((9, 40, 5, 20, 7), (9, 40, 8, 32, None), (9, 40, 0, None, 7), (9, 40, 39, 1, 7), (9, 40, 0, 1, None), (1, 1, 0, 1, None))
GATHER_TWO_TRIPS = (9, 600, 40, 512, 4100)                     # 2 099 200 elements against a cap of 8192 * 256 = 2 097 152


def gather_case(src_rows, ld, col0, ncols, nidx):
    g = _gen(9000 + ld + col0 + (nidx or 0))
    src = _randn((src_rows, ld), g)
    idx = None if nidx is None else torch.randint(0, src_rows, (nidx,), generator=g).to(torch.int64)
    if idx is not None and nidx >= 3:
        idx[0], idx[1], idx[-1] = src_rows - 1, 0, src_rows - 1
    return src.contiguous(), idx


def gather_host(src, col0, ncols, idx):
    rows = src if idx is None else src[idx]
    return rows[:, col0:(src.shape[1] if ncols is None else col0 + ncols)].contiguous()


# ================================================================================================================ embed_gather
STORAGES = ("fp32", "f16", "split", "mx")                      # the order of ALL_DTYPES in tests/test_kernels_gpu.py
EMBED_CLASSES = 100
EMBED_CASES = tuple((3, nc, C) for nc in (1, 2, 16) for C in (64, 512))              # (N, nc, C), every storage, with and without scale
EMBED_TWO_TRIPS = (130, 16, 512)                               # fp32: 4 259 840 chunks against a cap of 16384 * 256 = 4 194 304; output 68 MB


def embed_case(N, nc, C):
    """-> (emb [classes, C], labels [N, nc] in range, with 0 and classes - 1 among them, scale [N, C])"""
    g = _gen(10000 + N + 3 * nc + C)
    emb = _randn((EMBED_CLASSES, C), g)
    labels = torch.randint(0, EMBED_CLASSES, (N, nc), generator=g).to(torch.int64)
    labels[0, 0], labels[-1, -1] = 0, EMBED_CLASSES - 1
    if nc > 1:
        labels[0, 1], labels[-1, 0] = EMBED_CLASSES - 1, 0
    return emb.contiguous(), labels.contiguous(), (_randn((N, C), g) + 1.5).contiguous()


def embed_host(emb, labels, scale=None):
    """fp32 [N, 4, 4 * nc, C]: glyph slot x / 4 of sample n holds emb[labels[n, x / 4]] (* scale[n]) at every one of its 4 x 4 pixels"""
    N, nc = labels.shape
    rows = emb[labels]                                         # [N, nc, C]
    if scale is not None:
        rows = rows * scale[:, None, :]
    return rows.repeat_interleave(4, dim=1)[:, None].expand(N, 4, 4 * nc, emb.shape[1]).contiguous()


@functools.lru_cache(maxsize=None)
def embed_two_trip_inputs():
    return embed_case(*EMBED_TWO_TRIPS)
