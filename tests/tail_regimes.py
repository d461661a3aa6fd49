"""The launch arithmetic of the streaming ("tail") kernels of marconet_amd/csrc/aux_kernels.hip as data: small pure-Python mirrors of the host code of
each wrapper, the case tables of tests/test_tail_kernels_gpu.py, and for every case the regime it is there for as a predicate over that arithmetic.
No device needed: the CPU tier (test_tail_regimes.py) checks that every case lands in the regime it names, so a later change to a cap or a run length
cannot silently turn a multi-trip case into a single-trip one; the GPU tier asserts the same before it launches.

The formulas are COPIED from the sources (the line each one mirrors is named next to it); when one of those lines changes, change its mirror here and
re-derive the shapes below."""

import functools
import os
import re

F32, F16, SPLIT, MX = "fp32", "f16", "split", "mx"
STORAGES = (F32, F16, SPLIT, MX)
WG = 256                      # every kernel here launches 256 threads per workgroup


def _cdiv(a, b):
    return (a + b - 1) // b


def vec_n(dtype):
    """channels per 16-byte chunk — aux_kernels.hip, every wrapper: `const int N = chunk_n(dtype);`, common.h: `return dt == MNET_F32 ? 4 : 8;`"""
    return 4 if dtype == F32 else 8


# ---------------------------------------------------------------------------------------------------------------- upsample2x
UPS_RUN = 4                   # aux_kernels.hip:101  #define MNET_UPS_RUN 4
UPS_CAP = 2048                # aux_kernels.hip:216  `... < 2048 ? (per + 255) / 256 : 2048`


def ups_launch(n, h, w, c, dtype):
    """-> (per, gx, trips, xcd_remap_on) of mnet_upsample2x_convert_nhwc.
    per: aux_kernels.hip:215 `((h + MNET_UPS_RUN - 1) / MNET_UPS_RUN) * w * (c / N)`; gx: :216; grid (gx, n);
    trips of `for (id = bx * 256 + tid; id < per; id += gridDim.x * 256)` (:129); remap: :124 `(NWG & 7u) == 0u` with NWG = gridDim.x * gridDim.y"""
    per = _cdiv(h, UPS_RUN) * w * (c // vec_n(dtype))
    gx = min(_cdiv(per, WG), UPS_CAP)
    return per, gx, _cdiv(per, gx * WG), (gx * n) % 8 == 0


def ups_runs(h):
    """(number of row runs, rows in the last run) — aux_kernels.hip:131 `y0 = (col / W) * R, y1 = min(y0 + R, H)`; odd runs walk up (:175)"""
    runs = _cdiv(h, UPS_RUN)
    return runs, h - (runs - 1) * UPS_RUN


# ---------------------------------------------------------------------------------------------------------------- upfold3x3
def _upf_run():
    """the #define MNET_UPF_RUN line of upfold_kernels.hip (read, not copied: tests/test_upfold_gpu.py reads it the same way)"""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "marconet_amd", "csrc", "upfold_kernels.hip")
    with open(src) as f:
        return int(re.search(r"#define MNET_UPF_RUN (\d+)", f.read()).group(1))


UPF_RUN = _upf_run()
UPF_CAP = 2048                # upfold_kernels.hip, launcher: `(per + 255) / 256 < 2048 ? (per + 255) / 256 : 2048`


def upf_launch(n, h, w, c, dtype):
    """-> (per, gx, trips, xcd_remap_on) of mnet_upfold3x3_nhwc (c: OUTPUT channels; z holds 9 c).
    per: `((h + MNET_UPF_RUN - 1) / MNET_UPF_RUN) * 2 * w * (c / N)` — one thread per (chunk, HI-res column, run of low-res rows); gx: the cap line;
    grid (gx, n); trips of `for (id = bx * 256u + threadIdx.x; id < items_per_image; id += gridDim.x * 256u)`; remap: `(NWG & 7u) == 0u`"""
    per = _cdiv(h, UPF_RUN) * 2 * w * (c // vec_n(dtype))
    gx = min(_cdiv(per, WG), UPF_CAP)
    return per, gx, _cdiv(per, gx * WG), (gx * n) % 8 == 0


def upf_runs(h):
    """(number of row runs, low-res rows in the last run) — `y0 = (col / W2) * R, y1 = min(y0 + R, H)`"""
    runs = _cdiv(h, UPF_RUN)
    return runs, h - (runs - 1) * UPF_RUN


def upf_guards_ok(n, h, w, c, dtype):
    """the launcher's two "image too large" guards"""
    return w * 9 * c < 1 << 29 and h * w * (c // vec_n(dtype)) * 4 < 1 << 31


# ---------------------------------------------------------------------------------------------------------------- GroupNorm statistics
GN_SLICE_CAP = 128            # ops.py:299 `slices = max(1, min(128, (h * w) // 512))`


def gn_slices(h, w):
    return max(1, min(GN_SLICE_CAP, (h * w) // 512))


def gn_launch(h, w, c, dtype):
    """-> (slices, per, last, plane): pixels per slice (aux_kernels.hip:254 `per = (HW + slices - 1) / slices`), pixels of the last slice
    (:255 `p_end = min(HW, p_begin + per)`; <= 0 would be an empty slice), pixel lanes per workgroup (:250 `plane = 256 / (C / N)`)"""
    hw, s = h * w, gn_slices(h, w)
    per = _cdiv(hw, s)
    return s, per, hw - per * (s - 1), WG // (c // vec_n(dtype))


@functools.lru_cache(maxsize=None)
def gn_shortest_last_slice(limit=1 << 18):
    """(last / per, HW) of the map size whose last slice is the shortest share of a full one, over every HW < limit with more than one slice"""
    best = None
    for hw in range(1024, limit):
        s = gn_slices(1, hw)
        per = _cdiv(hw, s)
        key = ((hw - per * (s - 1)) / per, hw)
        if best is None or key < best:
            best = key
    return best


# ---------------------------------------------------------------------------------------------------------------- GroupNorm apply
def affine_ppt(c, dtype):
    """chunks per thread — aux_kernels.hip:1031 `c / N >= 128 ? 2 : 1` (MNET_AFFINE_PPT unset)"""
    return 2 if c // vec_n(dtype) >= 128 else 1


def affine_launch(hw, c, dtype):
    """-> (per, ppt, gx, tail): chunks per image (aux_kernels.hip:1046), chunks per thread, workgroups per image (:1032
    `(per + 256 * ppt - 1) / (256 * ppt)`), chunks left for the last workgroup.  Thread t of a workgroup takes chunks `first + 256 k`, k < ppt (:1008):
    with ppt = 2, tail <= 256 puts every second chunk of the last workgroup beyond the image, tail < 256 both chunks of threads tail..255"""
    per = hw * (c // vec_n(dtype))
    ppt = affine_ppt(c, dtype)
    gx = _cdiv(per, WG * ppt)
    return per, ppt, gx, per - (gx - 1) * WG * ppt


AFFINE_OLD_CAP = 1024         # the workgroups-per-image cap the kernel had before it went to one trip per thread


# ---------------------------------------------------------------------------------------------------------------- flat kernels
FLAG_CAP, CONVERT_CAP, SR_CAP, FBA_CAP = 4096, 16384, 65536, 16384


def flag_launch(numel, dtype):
    """-> (nv, grid, trips, tail) of mnet_nonfinite_flag: 16-byte vectors (aux_kernels.hip:1119 `n / chunk_n(dtype)`), workgroups
    (:1120: ceil(nv / 256) clamped to [1, 4096]), trips of the grid-stride loop (:1100), elements of the scalar tail (:1109 `i = nv * N; i < n`)"""
    n = vec_n(dtype)
    nv = numel // n
    grid = max(1, min(_cdiv(nv, WG), FLAG_CAP))
    return nv, grid, _cdiv(nv, grid * WG), numel - nv * n


def convert_launch(count):
    """-> (n8, blocks, trips) of mnet_convert: aux_kernels.hip:940 `n8 = count / 8`, :941 `(n8 + 255) / 256 < 16384 ? ... : 16384`, loop :918"""
    n8 = count // 8
    blocks = min(_cdiv(n8, WG), CONVERT_CAP)
    return n8, blocks, _cdiv(n8, blocks * WG)


def sr_launch(npix):
    """-> (grid, trips) of mnet_sr_postprocess: aux_kernels.hip:1080 `(npix + 255) / 256 < 65536 ? ... : 65536`, loop :1062"""
    grid = min(_cdiv(npix, WG), SR_CAP)
    return grid, _cdiv(npix, grid * WG)


def fba_launch(total):
    """-> (blocks, trips) of mnet_fused_bias_act: aux_kernels.hip:970 `(total + 255) / 256 < 16384 ? ... : 16384`, loop :959"""
    blocks = min(_cdiv(total, WG), FBA_CAP)
    return blocks, _cdiv(total, blocks * WG)


# ================================================================================================================ case tables
# Every case: (regime name, parameters).  REGIME[name](parameters, dtype) is True iff the launch really is in that regime.

# ---- nonfinite_flag: numel per dtype.  N = 8 (f16) / 4 (fp32); 2400 / 1200 elements = 300 vectors = two workgroups, one of them partly idle;
#      the last entry makes 513 vectors more than one full trip of the capped grid
def flag_sizes(dtype):
    n = vec_n(dtype)
    big = (FLAG_CAP * WG + 513) * n
    return [("below one vector, tail only", 1), ("below one vector, tail only", n - 1), ("one vector, no tail", n), ("one vector, tail 1", n + 1),
            ("one vector, tail N-1", 2 * n - 1), ("two workgroups, no tail", 300 * n), ("two workgroups, tail 1", 300 * n + 1),
            ("two workgroups, tail N-1", 300 * n + n - 1), ("2 trips, no tail", big), ("2 trips, tail 1", big + 1), ("2 trips, tail N-1", big + n - 1)]


def _flag_regime(want_nv, want_trips, want_tail):
    def ok(numel, dtype):
        nv, grid, trips, tail = flag_launch(numel, dtype)
        n = vec_n(dtype)
        return want_nv(nv, grid) and trips == want_trips and tail == want_tail(n)
    return ok


FLAG_REGIME = {
    "below one vector, tail only": lambda numel, dt: flag_launch(numel, dt)[0] == 0 and flag_launch(numel, dt)[1] == 1 and flag_launch(numel, dt)[3] == numel,
    "one vector, no tail": _flag_regime(lambda nv, g: nv == 1 and g == 1, 1, lambda n: 0),
    "one vector, tail 1": _flag_regime(lambda nv, g: nv == 1 and g == 1, 1, lambda n: 1),
    "one vector, tail N-1": _flag_regime(lambda nv, g: nv == 1 and g == 1, 1, lambda n: n - 1),
    "two workgroups, no tail": _flag_regime(lambda nv, g: g == 2 and nv % WG != 0, 1, lambda n: 0),
    "two workgroups, tail 1": _flag_regime(lambda nv, g: g == 2 and nv % WG != 0, 1, lambda n: 1),
    "two workgroups, tail N-1": _flag_regime(lambda nv, g: g == 2 and nv % WG != 0, 1, lambda n: n - 1),
    "2 trips, no tail": _flag_regime(lambda nv, g: g == FLAG_CAP and nv % (FLAG_CAP * WG) != 0, 2, lambda n: 0),
    "2 trips, tail 1": _flag_regime(lambda nv, g: g == FLAG_CAP and nv % (FLAG_CAP * WG) != 0, 2, lambda n: 1),
    "2 trips, tail N-1": _flag_regime(lambda nv, g: g == FLAG_CAP and nv % (FLAG_CAP * WG) != 0, 2, lambda n: n - 1),
}

# ---- groupnorm_affine: (regime, (n, h, w, c, valid_w or None)).  valid_w: ragged, with w, 1 and a width in between (None: the kernel's no-mask path)
GN_CASES = [
    ("2 slices, odd HW", (3, 29, 37, 1024, None)),
    ("2 slices, odd HW", (3, 29, 37, 1024, (37, 1, 20))),
    ("2 slices, odd HW", (3, 29, 37, 32, (20, 37, 1))),
    ("4 slices, short last slice", (3, 41, 51, 256, (1, 33, 51))),
    ("32 slices, production map", (3, 32, 512, 64, (512, 1, 301))),
    ("32 slices, production map", (3, 32, 512, 64, None)),
    ("128 slices, cap binds, short last slice", (2, 65, 1031, 64, (1031, 517))),
    ("128 slices, shortest last slice", (3, 1, 65537, 32, (65537, 1, 40000))),
]
GN_BATCH_CASE = ("4 slices, short last slice", (3, 41, 51, 256, (1, 33, 51)))      # batch invariance: image i alone == image i in the batch, bit for bit


def _gn(p, dt):
    return gn_launch(p[1], p[2], p[3], dt)


GN_REGIME = {
    "2 slices, odd HW": lambda p, dt: _gn(p, dt)[0] == 2 and (p[1] * p[2]) % 2 == 1 and 0 < _gn(p, dt)[2] < _gn(p, dt)[1],
    "4 slices, short last slice": lambda p, dt: _gn(p, dt)[0] == 4 and 0 < _gn(p, dt)[2] < _gn(p, dt)[1],
    "32 slices, production map": lambda p, dt: _gn(p, dt)[0] == 32 and (p[1], p[2]) == (32, 512),
    "128 slices, cap binds, short last slice": lambda p, dt: (p[1] * p[2]) // 512 > GN_SLICE_CAP and _gn(p, dt)[0] == GN_SLICE_CAP and 0 < _gn(p, dt)[2] < _gn(p, dt)[1],
    "128 slices, shortest last slice": lambda p, dt: _gn(p, dt)[0] == GN_SLICE_CAP and (_gn(p, dt)[2] / _gn(p, dt)[1], p[1] * p[2]) == gn_shortest_last_slice(),
}

# ---- upsample2x: (regime, (n, h, w, c)).  h x 24 x 64 maps: 3 (8-channel chunks) / 6 (fp32) workgroups per image and run, more with more runs
UPS_CASES = [
    ("several workgroups, XCD remap on", (8, 16, 24, 64)),
    ("several workgroups, XCD remap off", (3, 16, 24, 64)),
    ("H%4=0, even runs", (3, 8, 24, 64)), ("H%4=0, odd runs", (3, 12, 24, 64)),
    ("H%4=1, even runs", (3, 5, 24, 64)), ("H%4=1, odd runs", (8, 9, 24, 64)),
    ("H%4=2, even runs", (8, 6, 24, 64)), ("H%4=2, odd runs", (3, 10, 24, 64)),
    ("H%4=3, even runs", (3, 7, 24, 64)), ("H%4=3, odd runs", (8, 11, 24, 64)),
    ("H<4", (3, 1, 40, 64)), ("H<4", (8, 2, 40, 64)), ("H<4", (3, 3, 40, 64)),
    ("W=1", (3, 17, 1, 512)), ("W=1", (8, 40, 1, 512)),
]
UPS_CAP_CASE = ("2 trips + XCD", {F32: (1, 130, 1009, 64), F16: (1, 130, 2017, 64), SPLIT: (1, 130, 2017, 64), MX: (1, 130, 2017, 64)})


def _ups_h(mod, odd):
    def ok(p, dt):
        runs, last = ups_runs(p[1])
        return p[1] % 4 == mod and runs % 2 == (1 if odd else 0) and runs > 1 and last == (mod or 4) and ups_launch(*p, dt)[1] > 1
    return ok


UPS_REGIME = {
    "several workgroups, XCD remap on": lambda p, dt: ups_launch(*p, dt)[1] > 1 and ups_launch(*p, dt)[2] == 1 and ups_launch(*p, dt)[3],
    "several workgroups, XCD remap off": lambda p, dt: ups_launch(*p, dt)[1] > 1 and ups_launch(*p, dt)[2] == 1 and not ups_launch(*p, dt)[3],
    "H<4": lambda p, dt: p[1] < 4 and ups_runs(p[1]) == (1, p[1]) and ups_launch(*p, dt)[1] > 1,
    "W=1": lambda p, dt: p[2] == 1 and ups_launch(*p, dt)[1] > 1,
    "2 trips + XCD": lambda p, dt: (ups_launch(*p, dt)[1] == UPS_CAP and ups_launch(*p, dt)[2] == 2 and ups_launch(*p, dt)[0] % (UPS_CAP * WG) != 0
                                    and ups_launch(*p, dt)[3] and 4 * p[1] * p[2] * p[3] * 4 <= 300 << 20),      # output <= 300 MB in fp32 / split
}
for _m in range(4):
    UPS_REGIME["H%%4=%d, even runs" % _m] = _ups_h(_m, False)
    UPS_REGIME["H%%4=%d, odd runs" % _m] = _ups_h(_m, True)

# ---- upfold3x3: (regime, (n, h, w, c)), c = output channels.  h x 24 x 64 maps: 48 hi-res columns x 8 (16 in fp32) chunks per run = 384 (768) items,
#      so two runs make 3 (6) workgroups per image; c = 64 gives two 32-channel blocks per pixel in the blocked storages
UPF_CASES = [
    ("several workgroups, XCD remap on", (8, 16, 24, 64)),
    ("several workgroups, XCD remap off", (3, 16, 24, 64)),
    ("H%8=0", (3, 16, 24, 64)), ("H%8=1", (8, 9, 24, 64)), ("H%8=2", (3, 10, 24, 64)), ("H%8=3", (8, 11, 24, 64)),
    ("H%8=4", (3, 12, 24, 64)), ("H%8=5", (8, 13, 24, 64)), ("H%8=6", (3, 14, 24, 64)), ("H%8=7", (8, 15, 24, 64)),
    ("three runs", (3, 17, 24, 64)), ("three runs", (8, 24, 24, 64)),
    ("one run, H<8", (3, 1, 40, 64)), ("one run, H<8", (3, 2, 40, 64)), ("one run, H<8", (3, 3, 40, 64)), ("one run, H<8", (3, 7, 40, 64)),
    ("one run, H=8", (3, 8, 40, 64)),                       # the top and the bottom edge fall into the same full run
    ("W=1", (3, 17, 1, 512)), ("W=1", (8, 9, 1, 1024)),     # every column clamps on both sides ((8, 9, 1, 512) is ONE workgroup per image in the 8-channel-chunk storages)
    ("W=2", (3, 9, 2, 512)),                                # the left and the right clamp on neighbouring columns
]
# the smallest map that reaches the second trip with one 32-channel block: per = 2 * 65600 * 4 = 2 * 32800 * 8 = 524 800 items > 2048 * 256 = 524 288;
# z = 2 * 65600 * 288 elements (151 MB at 4 bytes), y = 4 * 131200 * 32 (67 MB)
UPF_CAP_CASE = ("2 trips + XCD", {F32: (1, 2, 32800, 32), F16: (1, 2, 65600, 32), SPLIT: (1, 2, 65600, 32), MX: (1, 2, 65600, 32)})


# input scale of z per case: 1.5 (the scale of tests/test_upfold_gpu.py's first cases) unless the case has no headroom with it.  fp16+8 holds an output in [8, 16)
# to 2^-13 = 1.22e-4, so the half bound 1e-5 x max |ref| of tests/test_tail_regimes.py::test_upfold_reference_headroom needs max |ref| >= 12.2: at scale 1.5 the
# (3, 17, 1, 512) map has max |ref| = 12.22 (0.9998 of the half bound); at 1.8 it is 14.7, still below 16
UPF_Z_SCALE = {(3, 17, 1, 512): 1.8}


def upf_z_scale(p):
    return UPF_Z_SCALE.get(tuple(p), 1.5)


def _upf_h(mod):
    def ok(p, dt):
        runs, last = upf_runs(p[1])
        per, gx, trips, _ = upf_launch(*p, dt)
        return p[1] % UPF_RUN == mod and runs >= 2 and last == (mod or UPF_RUN) and gx > 1 and trips == 1
    return ok


def _upf_cap(p, dt):
    per, gx, trips, remap = upf_launch(*p, dt)
    return gx == UPF_CAP and trips == 2 and per % (UPF_CAP * WG) != 0 and remap and p[0] == 1 and upf_guards_ok(*p, dt)


UPF_REGIME = {
    "several workgroups, XCD remap on": lambda p, dt: upf_launch(*p, dt)[1] > 1 and upf_launch(*p, dt)[2] == 1 and upf_launch(*p, dt)[3],
    "several workgroups, XCD remap off": lambda p, dt: upf_launch(*p, dt)[1] > 1 and upf_launch(*p, dt)[2] == 1 and not upf_launch(*p, dt)[3],
    "three runs": lambda p, dt: upf_runs(p[1])[0] == 3 and upf_launch(*p, dt)[1] > 1 and upf_launch(*p, dt)[2] == 1,
    "one run, H<8": lambda p, dt: p[1] < UPF_RUN and upf_runs(p[1]) == (1, p[1]) and upf_launch(*p, dt)[1] > 1 and upf_launch(*p, dt)[2] == 1,
    "one run, H=8": lambda p, dt: p[1] == UPF_RUN and upf_runs(p[1]) == (1, UPF_RUN) and upf_launch(*p, dt)[1] > 1 and upf_launch(*p, dt)[2] == 1,
    "W=1": lambda p, dt: p[2] == 1 and upf_runs(p[1])[0] >= 2 and upf_launch(*p, dt)[1] > 1 and upf_launch(*p, dt)[2] == 1,
    "W=2": lambda p, dt: p[2] == 2 and upf_runs(p[1])[0] >= 2 and upf_launch(*p, dt)[1] > 1 and upf_launch(*p, dt)[2] == 1,
    "2 trips + XCD": _upf_cap,
}
for _m in range(8):
    UPF_REGIME["H%%8=%d" % _m] = _upf_h(_m)

# ---- affine_act: (regime, (n, hw as (h, w), c)) per storage
AFFINE_CASES = {
    F32: [("2 chunks, last workgroup's second chunk beyond", (2, (6, 7), 512)), ("2 chunks, both beyond for part of the last workgroup", (2, (5, 9), 512)),
          ("2 chunks, last workgroup's second chunk beyond", (2, (5, 9), 1024)), ("1 chunk, more workgroups than the old cap", (2, (130, 253), 64))],
}
for _dt in (F16, SPLIT, MX):
    AFFINE_CASES[_dt] = [("2 chunks, last workgroup's second chunk beyond", (2, (6, 7), 1024)),
                         ("2 chunks, both beyond for part of the last workgroup", (2, (5, 9), 1024)),
                         ("1 chunk, more workgroups than the old cap", (2, (130, 253), 64))]


def _aff(p, dt):
    return affine_launch(p[1][0] * p[1][1], p[2], dt)


AFFINE_REGIME = {
    "2 chunks, last workgroup's second chunk beyond": lambda p, dt: _aff(p, dt)[1] == 2 and _aff(p, dt)[2] > 1 and _aff(p, dt)[3] == WG,
    "2 chunks, both beyond for part of the last workgroup": lambda p, dt: _aff(p, dt)[1] == 2 and _aff(p, dt)[2] > 1 and 0 < _aff(p, dt)[3] < WG,
    "1 chunk, more workgroups than the old cap": lambda p, dt: _aff(p, dt)[1] == 1 and _aff(p, dt)[2] > AFFINE_OLD_CAP and _aff(p, dt)[3] < WG,
}

# ---- flat kernels past their caps
CONVERT_COUNT = (CONVERT_CAP * WG + 1000 * 4) * 8         # 4 000 chunks into the second trip; a multiple of 64: both halves are whole 32-channel blocks
CONVERT_PAIRS = [(F32, F16), (F32, SPLIT), (F32, MX), (F16, F32), (SPLIT, F32), (MX, F32), (MX, F16)]      # the conversions the pipeline makes
SR_SHAPE = (1, 4100, 4096, 3)                              # c_ld = 3: 4 x 4096 pixel rows into the second trip
FBA_SHAPE = (3, 12, 331, 353)                              # inner = 331 * 353 (odd)


def convert_regime_ok():
    n8, blocks, trips = convert_launch(CONVERT_COUNT)
    h8, hb, ht = convert_launch(CONVERT_COUNT // 2)
    return (blocks == CONVERT_CAP and trips == 2 and n8 % (CONVERT_CAP * WG) != 0 and CONVERT_COUNT % 64 == 0
            and hb < CONVERT_CAP and ht == 1)               # ... and each half alone is a single-trip launch below the cap


def sr_regime_ok():
    npix = SR_SHAPE[0] * SR_SHAPE[1] * SR_SHAPE[2]
    grid, trips = sr_launch(npix)
    return grid == SR_CAP and trips == 2 and npix % (SR_CAP * WG) != 0 and SR_SHAPE[3] == 3


def fba_regime_ok():
    total = 1
    for s in FBA_SHAPE:
        total *= s
    inner = FBA_SHAPE[2] * FBA_SHAPE[3]
    blocks, trips = fba_launch(total)
    return blocks == FBA_CAP and trips == 2 and total % (FBA_CAP * WG) != 0 and inner & (inner - 1) != 0 and inner % 2 == 1
