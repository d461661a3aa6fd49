"""No device: mnet_compare_stats' record layout and argument checks, the spec of tests/compare_spec.py on hand-made cases, the proof that the GPU case table
reaches every launch regime of compare_kernels.hip, and the decision logic of the report MarconetPipeline.calibrate returns."""
import ctypes
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch

from tests import compare_spec as C
from tests import storage_codec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(*rel):
    with open(os.path.join(ROOT, *rel)) as f:
        return f.read()


# ================================================================================================================ the record and the workspace macro
def test_cmp_stats_layout_and_workspace_macro_match_c():
    """a C program compiled from the header against the ctypes mirror, the numpy mirror of the tests and the Python forms of the macros"""
    from marconet_amd import _lib
    fields = [n for n, _ in _lib.CmpStats._fields_]
    sizes = (32, 2048, 2080, 4128, 65536, 65568, 1 << 20)
    code = '#include <stdio.h>\n#include <stddef.h>\n#include "marconet_hip.h"\nint main(void){ printf("%zu", sizeof(mnet_cmp_stats));\n'
    code += "".join(' printf(" %%zu", offsetof(mnet_cmp_stats, %s));\n' % f for f in fields)
    code += "".join(' printf(" %%d %%zu", (int)MNET_CMP_SLICES(%d), (size_t)MNET_CMP_WORKSPACE_BYTES(3, %d));\n' % (e, e) for e in sizes)
    code += ' printf(" %d %d\\n", MNET_CMP_WG_ELEMS, MNET_CMP_MAX_SLICES); return 0; }\n'
    d = tempfile.mkdtemp(prefix="mnet_cmp_")
    cpath, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
    with open(cpath, "w") as f:
        f.write(code)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), cpath, "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    want = [ctypes.sizeof(_lib.CmpStats)] + [getattr(_lib.CmpStats, f).offset for f in fields]
    for e in sizes:
        want += [_lib.cmp_slices(e), _lib.cmp_workspace_bytes(3, e)]
    want += [_lib.CMP_WG_ELEMS, _lib.CMP_MAX_SLICES]
    assert got == want
    assert ctypes.sizeof(_lib.CmpStats) == C.RECORD_BYTES == C.RECORD_DTYPE.itemsize
    assert [C.RECORD_DTYPE.fields[f][1] for f in fields] == [getattr(_lib.CmpStats, f).offset for f in fields]
    assert [_lib.cmp_slices(e) for e in sizes] == [C.slices(e) for e in sizes] == [1, 1, 2, 3, 32, 32, 32]


def test_argument_validation_without_device():
    """every refusal comes before any HIP call: the checks run on a box without a GPU"""
    from marconet_amd import _lib
    lib = _lib.load()

    def call(mode=128, mdt=3, ref=128, rdt=2, groups=2, elems=64, stats=256, ws=256):
        return lib.mnet_compare_stats(mode, mdt, ref, rdt, groups, elems, stats, ws, None)

    ok_pairs = {(C.DTYPE_ID[m], C.DTYPE_ID[r]) for m, r in C.PAIRS}
    assert len(ok_pairs) == 6
    for mdt in range(-1, 5):
        for rdt in range(-1, 5):
            if (mdt, rdt) not in ok_pairs:
                assert call(mdt=mdt, rdt=rdt) == -1 and b"pair" in lib.mnet_last_error(), (mdt, rdt)
    for kw in (dict(mode=None), dict(ref=None), dict(stats=None), dict(ws=None)):
        assert call(**kw) == -1 and b"null" in lib.mnet_last_error(), kw
    for elems in (0, -32, 8, 16, 24, 33, 48, 2047):
        assert call(elems=elems) == -1, elems
    assert b"multiple of 32" in lib.mnet_last_error()
    for groups in (0, -1):
        assert call(groups=groups) == -1, groups
    # bases: 16 bytes for F32 / F16, 128 for the blocked storages; records and workspace 8
    assert call(mode=64) == -2 and call(ref=64) == -2 and call(mode=144, mdt=1, ref=64) == -2          # fp16+8 / split half at 64; split half at 64 under an f16 mode
    assert call(mode=8, mdt=1) == -2 and call(mode=8, mdt=0, ref=16, rdt=0) == -2 and call(mode=16, mdt=0, ref=24, rdt=0) == -2
    assert call(stats=260) == -2 and call(ws=4) == -2 and b"8-byte" in lib.mnet_last_error()


# ================================================================================================================ the spec on hand-made cases
def _bits(v):
    return S.bits32(np.asarray(v, dtype=np.float32))


def test_spec_tie_takes_the_lowest_index():
    m = np.zeros(64, dtype=np.float32)
    r = m.copy()
    r[[5, 17, 40]] = [2.0, -2.0, 2.0]
    r[9] = 1.0
    rec = C.record(_bits(m), _bits(r))
    assert rec["max_abs_diff"] == 2.0 and rec["argmax_index"] == 5 and rec["max_abs_ref"] == 2.0 and rec["max_abs_mode"] == 0.0
    assert rec["sum_sq_diff"] == 13.0 and rec["sum_sq_ref"] == 13.0 and rec["nonfinite_mode"] == rec["nonfinite_ref"] == 0


def test_spec_a_nonfinite_pair_is_counted_and_left_out():
    m = np.array([1.0, np.nan, 3.0, np.inf, 100.0, 7.0] + [0.0] * 26, dtype=np.float32)
    r = np.array([1.5, 1e9, np.nan, -np.inf, 100.0, np.inf] + [0.0] * 26, dtype=np.float32)
    rec = C.record(_bits(m), _bits(r))
    assert rec["nonfinite_mode"] == 2 and rec["nonfinite_ref"] == 3
    assert rec["max_abs_diff"] == 0.5 and rec["argmax_index"] == 0            # the 1e9 beside a NaN, the 7 beside an inf do not count
    assert rec["max_abs_ref"] == 100.0 and rec["max_abs_mode"] == 100.0 and rec["sum_sq_diff"] == 0.25 and rec["sum_sq_ref"] == 1.5 ** 2 + 1e4
    none = C.record(_bits([np.nan] * 32), _bits([1.0] * 32))
    assert none["argmax_index"] == -1 and none["max_abs_diff"] == 0 and none["nonfinite_mode"] == 32 and none["nonfinite_ref"] == 0 and none["sum_sq_ref"] == 0.0


def test_spec_signed_zeros_differ_by_zero():
    rec = C.record(_bits([-0.0] * 32), _bits([0.0] * 32))
    assert rec["max_abs_diff"] == 0 and np.float32(rec["max_abs_diff"]).tobytes() == np.float32(0).tobytes() and rec["argmax_index"] == 0
    assert rec["sum_sq_diff"] == 0.0 and rec["max_abs_ref"] == 0


def test_spec_reads_what_the_decoders_return():
    """an Operand's bits follow its bytes: a planted value is read back exactly in every storage, its block neighbours as the storage holds them"""
    v = C.base_values(2, 96)
    for st in C.STORAGES:
        op = C.Operand(st, v)
        assert np.array_equal(op.decoded_bits().reshape(-1, 32), C.DECODE[st](C.ENCODE[st](v.reshape(-1, 32))))
        op.set(1, 40, -C.PLANT)
        assert S.from_bits32(op.decoded_bits())[1, 40] == -C.PLANT
        want = v.copy()
        want[1, 40] = -C.PLANT
        assert np.array_equal(op.decoded_bits().reshape(-1, 32), C.DECODE[st](C.ENCODE[st](want.reshape(-1, 32))))
        op.poke_nonfinite(0, 7, np.inf)
        assert np.isinf(S.from_bits32(op.decoded_bits())[0, 7]) and np.isfinite(S.from_bits32(op.decoded_bits())[0, 8:32]).all()


# ================================================================================================================ regimes
def test_mirrored_constants_are_the_sources():
    hip, hdr, lib = _src("marconet_amd", "csrc", "compare_kernels.hip"), _src("include", "marconet_hip.h"), _src("marconet_amd", "_lib.py")
    assert re.search(r"constexpr int CMP_THREADS = %d;" % C.THREADS, hip) and re.search(r"constexpr int CMP_UNIT = %d;" % C.UNIT, hip)
    assert re.search(r"#define MNET_CMP_WG_ELEMS %d\b" % C.WG_ELEMS, hdr) and re.search(r"#define MNET_CMP_MAX_SLICES %d\b" % C.MAX_SLICES, hdr)
    assert "CMP_WG_ELEMS, CMP_MAX_SLICES = %d, %d" % (C.WG_ELEMS, C.MAX_SLICES) in lib
    # the map the regimes are worked out from: a linear thread -> unit map, slices striding by the whole grid, the clamp to the group's last block
    assert "const long long stride = (long long)slices * CMP_THREADS;" in hip and "const long long first = (long long)s * CMP_THREADS;" in hip
    assert "const long long u = first + t * stride + threadIdx.x;" in hip and "units - 4 + (threadIdx.x & 3)" in hip
    assert "const dim3 grid((unsigned)n_groups, (unsigned)slices);" in hip and "(int)MNET_CMP_SLICES(elems_per_group)" in hip
    assert "atomic" not in hip.split("#include")[1]                      # the reduction has none


def test_launch_mirror_on_sizes_worked_out_by_hand():
    assert C.launch(32) == (4, 1, 1, 4) and C.launch(96) == (12, 1, 1, 12) and C.launch(224) == (28, 1, 1, 28)
    assert C.launch(2048) == (256, 1, 1, 256) and C.launch(2080) == (260, 2, 1, 4) and C.launch(4128) == (516, 3, 1, 4)
    assert C.launch(65536) == (8192, 32, 1, 256) and C.launch(65568) == (8196, 32, 2, 256)         # workgroup 0's second trip: 4 live threads
    assert C.launch(128 * 2048 * 8) == (262144, 32, 32, 256)


def test_every_gpu_case_lands_in_its_regime():
    reached = set()
    for e in C.SIZES:
        assert e % 32 == 0
        for name in C.CASE_REGIMES[e]:
            assert C.REGIME[name](e), (name, e, C.launch(e))
            reached.add(name)
    assert reached == set(C.REGIME)
    assert set(C.SIZES) == set(C.CASE_REGIMES) and max(C.SIZES) * max(C.GROUPS) <= 1 << 20
    # the first sizes over one workgroup and over the cap: one block of 32 elements less is still the regime below
    assert not C.REGIME["multi_slice"](C.WG_ELEMS) and not C.REGIME["second_trip"](C.MAX_SLICES * C.WG_ELEMS)
    for e in C.SIZES:
        pos = C.plant_positions(e)
        assert pos[0] == 0 and pos[-1] == e - 1 and e - C.UNIT in pos
        for k in range(1, C.slices(e)):
            assert k * C.WG_ELEMS - 1 in pos and k * C.WG_ELEMS in pos
    assert C.MAX_SLICES * C.WG_ELEMS in C.plant_positions(C.SIZES[-1])     # the first element of the second trip


# ================================================================================================================ the report
def _rec(d=0.0, ref=1.0, idx=0, ssd=0.0, nfm=0, nfr=0):
    return types.SimpleNamespace(max_abs_diff=d, max_abs_ref=ref, max_abs_mode=ref, argmax_index=idx, sum_sq_diff=ssd, sum_sq_ref=0.0, nonfinite_mode=nfm, nonfinite_ref=nfr)


def _report(tol=5e-4, **stages):
    from marconet_amd import precision_guard as pg
    rep = pg.PrecisionReport(mode="fp16x2", reference="fp16x3", tol=tol, strips=2)
    for name in pg.STAGES:
        recs, owner = stages.get(name, ([_rec(), _rec()], [0, 1]))
        setattr(rep, name, pg.stage_from_records(name, recs, owner, 2, 64))
    return rep


def test_report_decision_logic():
    from marconet_amd import precision_guard as pg
    good = _report(sr=([_rec(4e-4), _rec(5e-4, idx=9)], [0, 1]))
    assert good.ok and good.first_stage_over is None and good.raise_if_failed() is good and good.sr.worst_strip == 1 and good.sr.worst_index == 9
    assert "OK" in str(good) and "sr" in str(good)
    over = _report(sr=([_rec(5.01e-4), _rec(1e-4)], [0, 1]))
    assert not over.ok and over.first_stage_over == "sr" and over.sr.worst_strip == 0 and over.sr.per_strip == [5.01e-4, 1e-4]
    with pytest.raises(pg.PrecisionMarginError) as ei:
        over.raise_if_failed()
    assert isinstance(ei.value, ArithmeticError) and "FAILED" in str(ei.value) and "sr" in str(ei.value)
    # first_stage_over is relative to max(1, |ref|) and does not enter ok: a large-magnitude feature map over tol in absolute terms only is not named,
    # one over it in relative terms is, and the decision stays with sr.max_abs_diff
    feat = _report(feat32_fused=([_rec(0.2, ref=1000.0), _rec()], [0, 1]), feat64_fused=([_rec(), _rec(2.0, ref=1000.0)], [0, 1]))
    assert feat.ok and feat.first_stage_over == "feat64_fused" and feat.feat32_fused.rel == pytest.approx(2e-4) and feat.feat64_fused.worst_strip == 1
    small = _report(style_w=([_rec(6e-4, ref=0.1), _rec()], [0, 1]))
    assert small.style_w.rel == pytest.approx(6e-4) and small.first_stage_over == "style_w" and small.ok
    # a non-finite element anywhere fails the check even with sr inside tol
    nan = _report(prior32=([_rec(nfm=1), _rec(), _rec()], [0, 0, 1]))
    assert not nan.ok and nan.nonfinite == 1 and "non-finite" in str(nan)
    assert not _report(sr=([_rec(nfr=2), _rec()], [0, 1])).ok
    # rms over all elements of the stage
    assert _report(sr=([_rec(ssd=32.0), _rec(ssd=96.0)], [0, 1])).sr.rms == 1.0


def test_report_maps_glyphs_to_strips():
    from marconet_amd import precision_guard as pg
    assert pg.glyph_to_strip([2, 0, 3]) == [0, 0, 2, 2, 2]
    st = pg.stage_from_records("prior64", [_rec(1e-4), _rec(3e-4), _rec(2e-4), _rec(7e-4, idx=5), _rec(7e-4, idx=1)], pg.glyph_to_strip([2, 0, 3]), 3, 32)
    assert st.per_strip == [3e-4, 0.0, 7e-4] and st.worst_strip == 2 and st.worst_index == 5 and st.max_abs_diff == 7e-4
    with pytest.raises(ValueError):
        pg.stage_from_records("prior64", [_rec()], [0, 0], 1, 32)


def test_reference_must_be_more_accurate_than_the_mode():
    from marconet_amd import precision_guard as pg
    for modes in (["fp16x2"] * 4, ["fp16"] * 4, ["fp16x2", "fp16x2", "fp16x2", "fp16"]):
        pg.check_reference(modes, "fp16x3")
    for modes in (["fp32"] * 4, ["fp16x3"] * 4, ["fp16x2"] * 4, ["fp16"] * 4):
        pg.check_reference(modes, "fp32")
    for modes, ref in ((["fp16x3"] * 4, "fp16x3"), (["fp32"] * 4, "fp16x3"), (["fp16x2", "fp16x2", "fp16x2", "fp32"], "fp16x3"),
                       (["fp16"] * 4, "fp16x2"), (["fp16"] * 4, "fp16"), (["fp16x2"] * 4, "bf16")):
        with pytest.raises(ValueError):
            pg.check_reference(modes, ref)


def test_calibrate_has_no_cpu_path_and_checks_the_reference_first():
    from marconet_amd import networks
    from marconet_amd.pipeline import MarconetPipeline
    from oracle import synth
    enc, gan, sr = networks.TextContextEncoderV2(), networks.TSPGAN(), networks.TSPSRNet()
    pipe = MarconetPipeline(enc, gan, sr, precision="fp16x2")
    lq, labels, locs = synth.make_lq(7, 1, [512]), [synth.make_labels(8, 3)], synth.make_locs([3], [512])
    with pytest.raises(RuntimeError, match="no CPU path"):
        pipe.calibrate(lq, labels, locs)
    pipe.set_precision("fp16x3")
    with pytest.raises(ValueError, match="not more accurate"):
        pipe.calibrate(lq, labels, locs)
    assert pipe.precision == "fp16x3" and sr.scale_branch_precision is None


def test_ops_compare_stats_refuses_cpu_tensors():
    from marconet_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.compare_stats(torch.zeros(2, 64), torch.zeros(2, 64))
