"""not-gpu: the pure-host definition of a blind reading (marconet_amd/blind.py) — the probes of a line and what each owns, one probe's prediction
turned into characters, the merge's guarantees on hand-written and on random predictions, ``plan_windows`` on what the merge returns — and the
host side of mnet_lq_windows_u8: the descriptor's C layout, the wrapper's refusals and the entry point's argument checks (the library loads
without a GPU)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from marconet_amd import _lib, blind, long_lines, lq_device, lq_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
BLANK = 6735


def _limit(h):
    """the widest line ``shape_geometry`` accepts at height h"""
    w = 512 * h // 32 + 2
    while long_lines.too_wide(h, w):
        w -= 1
    return w


def _locs(pairs):
    """(left, right) pairs in units of the 512-px canvas → the encoder's fp32 row of 32"""
    row = np.zeros((32,), np.float32)
    row[:2 * len(pairs)] = np.asarray(pairs, np.float32).reshape(-1)
    return row


def _indices(labels):
    """a row of 64 argmax indices that collapses to ``labels``: each label once, a blank after it"""
    row = []
    for v in labels:
        row += [v, BLANK]
    return row + [BLANK] * (64 - len(row))


# ------------------------------------------------------------------------------------------------------------------------- plan_probes
@pytest.mark.parametrize("h", (8, 24, 32, 33, 40, 97))
def test_a_line_at_the_limit_is_one_probe_and_one_column_wider_is_at_least_two(h):
    w = _limit(h)
    assert blind.plan_probes(h, w) == [(0, w, 0, w)] and blind.plan_probes(h, h) == [(0, h, 0, h)]
    assert len(blind.plan_probes(h, w + 1)) >= 2


@pytest.mark.parametrize("h", (8, 24, 32, 40, 97))
@pytest.mark.parametrize("probe_width", (32, 128, 384, 512))
def test_probes_cover_the_line_and_ownership_partitions_it(h, probe_width):
    P = blind.probe_crop_width(h, probe_width)
    assert lq_device._axis(h, P, 32)[0] <= probe_width < lq_device._axis(h, P + 1, 32)[0]
    for w in (_limit(h) + 1, _limit(h) + 2, 2 * P + 1, 3 * P, 5 * P // 2 + 7, 3 * _limit(h) + 11):
        if w <= _limit(h):
            continue
        pr = blind.plan_probes(h, w, probe_width)
        assert len(pr) >= 2 and pr[0][0] == 0 and pr[-1][1] == w and pr[-1][0] == w - P          # the last probe is flush right
        assert pr[0][2] == 0 and pr[-1][3] == w
        for k, (c0, c1, lo, hi) in enumerate(pr):
            assert c1 - c0 == P and 0 <= c0 <= lo < hi <= c1 <= w
            assert lq_device.shape_geometry(h, c1 - c0).dw <= probe_width
            if k + 1 < len(pr):
                n0, n1 = pr[k + 1][:2]
                assert n0 > c0 and n0 < c1                                                      # strictly advancing, overlapping: no column uncovered
                assert pr[k + 1][2] == hi == (n0 + c1) // 2                                      # the partition: one owner per column
                if k + 2 < len(pr):
                    assert n0 - c0 == P // 2                                                     # every start but the last on the half-probe grid
        for k in range(1, len(pr) - 1):                                                          # an interior probe between two on the grid owns its middle half
            if k + 2 < len(pr):
                c0, c1, lo, hi = pr[k]
                assert lo - c0 >= P // 4 and c1 - hi >= P // 4


def test_a_line_slightly_wider_than_a_probe_has_two_probes_that_overlap_almost_wholly():
    h = 32
    P = blind.probe_crop_width(h, 512)
    assert P == 512 and long_lines.too_wide(h, P + 1)
    assert blind.plan_probes(h, P + 1, 512) == [(0, P, 0, (1 + P) // 2), (1, P + 1, (1 + P) // 2, P + 1)]


def test_plan_probes_refusals():
    for bad in (0, 28, 30, 386, 516, 1024, -384, 384.0, "384", None, True):
        with pytest.raises(ValueError, match="probe_width"):
            blind.plan_probes(32, 2000, bad)
    with pytest.raises(ValueError, match="too narrow"):
        blind.plan_probes(1, 100, 32)                           # P = 1: two probes could not overlap
    with pytest.raises(ValueError, match="empty"):
        blind.plan_probes(0, 100)
    with pytest.raises(ValueError, match="empty"):
        blind.plan_probes(32, 0)
    with pytest.raises(ValueError, match="line 1: .*too narrow"):
        blind.line_probes([(32, 10), (1, 5000)], 32)


# -------------------------------------------------------------------------------------------------------------------- read_probe, merge
def test_read_probe_places_boxes_and_orders_left_and_right():
    h, probe = 64, (100, 868, 100, 868)                          # 512 * h / 32 = 1024 source px per canvas
    labels, boxes, overflow = blind.read_probe(_indices([5, 6]), _locs([(0.25, 0.125), (0.5, 0.625)]), probe, h)
    assert labels == [5, 6] and not overflow
    assert boxes == [(100 + 0.125 * 1024, 100 + 0.25 * 1024), (100 + 0.5 * 1024, 100 + 0.625 * 1024)]       # left > right: x1 is the smaller
    assert blind.read_probe([7, 7, 7, BLANK, 7] + [BLANK] * 59, _locs([(0.1, 0.2), (0.3, 0.4)]), (0, 1024, 0, 1024), 64)[0] == [7, 7]


def test_a_centre_on_an_ownership_boundary_has_exactly_one_owner():
    h = 32                                                       # 512 source px per canvas: loc k / 512 is column k exactly
    left, right = (0, 384, 0, 288), (192, 576, 288, 576)
    a = blind.read_probe(_indices([9]), _locs([(280 / 512, 296 / 512)]), left, h)                     # centre 288 = the boundary
    b = blind.read_probe(_indices([9]), _locs([((280 - 192) / 512, (296 - 192) / 512)]), right, h)
    assert a[0] == [] and b[0] == [9] and b[1] == [(280.0, 296.0)]
    a = blind.read_probe(_indices([9]), _locs([(279 / 512, 296 / 512)]), left, h)                     # centre 287.5: the left probe's
    b = blind.read_probe(_indices([9]), _locs([((279 - 192) / 512, (296 - 192) / 512)]), right, h)
    assert a[0] == [9] and b[0] == []
    assert blind.read_probe(_indices([9]), _locs([(float("nan"), 0.5)]), left, h)[0] == []            # not a number: nobody's


def test_seventeen_labels_overflow_and_keep_sixteen_boxes():
    pairs = [(k / 16, (k + 0.5) / 16) for k in range(16)]
    labels, boxes, overflow = blind.read_probe(_indices(list(range(17))), _locs(pairs), (0, 512, 0, 512), 32)
    assert overflow and labels == list(range(16)) and len(boxes) == 16
    labels, boxes, overflow = blind.read_probe(_indices(list(range(16))), _locs(pairs), (0, 512, 0, 512), 32)
    assert not overflow and len(boxes) == 16
    got = blind.decode([(32, 512)], [[(0, 512, 0, 512)]], [_indices(list(range(17)))], [_locs(pairs)])[0]
    assert got["overflow"] and len(got["labels"]) == 16 and got["text"] == lq_io.text_from_labels(range(16)) and got["probes"] == [(0, 512, 0, 512)]


def test_merge_drops_the_duplicate_across_a_boundary_and_keeps_a_repeat_inside_a_probe():
    a = ([3, 4], [(100.0, 120.0), (180.0, 200.0)], False)
    b = ([4, 4, 5], [(182.0, 201.0), (205.0, 225.0), (230.0, 250.0)], False)
    labels, boxes = blind.merge(32, 400, [a, b])
    assert labels == [3, 4, 4, 5]                                # 4 seen by both probes once; 4 twice inside probe b kept
    assert [b_[0] for b_ in boxes] == [100.0, 180.0, 205.0, 230.0] and boxes[1][2] == 200.0
    labels, _ = blind.merge(32, 400, [a, ([6], [(182.0, 201.0)], False)])
    assert labels == [3, 4, 6]                                   # another label at the same place: not a duplicate
    labels, _ = blind.merge(32, 400, [a, ([4], [(195.0, 215.0)], False)])
    assert labels == [3, 4, 4]                                   # 5 of 20 px shared: not more than half of the narrower


def test_merge_makes_nested_and_overlapping_boxes_disjoint_clamps_and_drops_subpixel_boxes():
    reads = [([1, 2, 3, 4, 5, 6], [(-30.0, 12.0), (10.0, 50.0), (20.0, 30.0), (280.0, 340.0), (100.0, 100.5), (400.0, 420.0)], False)]
    labels, boxes = blind.merge(40, 300, reads)
    assert labels == [1, 3, 2, 4]                                # by centre: 1 (clamped to 0..12), 3 (25), 2 (30); 5 is under a pixel; 6 is outside
    assert boxes[0] == [0.0, 0.0, 12.0, 40.0]                    # clamped into the line; it does not reach its neighbour 3
    assert boxes[1] == [20.0, 0.0, 25.0, 40.0] and boxes[2] == [25.0, 0.0, 50.0, 40.0]      # 3 nested in 2: they meet at the middle of what they share
    assert boxes[-1] == [280.0, 0.0, 300.0, 40.0]                # clamped into the line
    for p, q in zip(boxes, boxes[1:]):
        assert p[2] <= q[0]
    assert all(b[2] - b[0] >= 1.0 and 0.0 <= b[0] and b[2] <= 300.0 for b in boxes)


def test_an_empty_reading_is_none():
    assert blind.merge(32, 100, []) == ([], []) and blind.merge(32, 100, [([], [], False)]) == ([], [])
    assert blind.decode([(32, 100)], [[(0, 100, 0, 100)]], [[BLANK] * 64], [_locs([])]) == [None]
    assert blind.merge(32, 100, [([1], [(float("inf"), 3.0)], False), ([2], [(float("nan"), float("nan"))], False)]) == ([], [])


@pytest.mark.parametrize("seed", range(6))
def test_random_predictions_keep_the_invariants_and_plan_or_refuse_in_plan_windows_words(seed):
    rng = np.random.default_rng(seed)
    planned = 0
    for _ in range(60):
        h = int(rng.choice((8, 24, 32, 40, 97)))
        w = int(rng.integers(1, 12 * h * 16))
        probes = blind.plan_probes(h, w, int(rng.choice((128, 384, 512))))
        rows, locs = [], []
        for _p in probes:
            n = int(rng.integers(0, 20))
            rows.append(_indices([int(v) for v in rng.integers(0, 40, n)]))
            mode = int(rng.integers(0, 3))
            if mode == 0:                                        # sane: sorted edges across the canvas
                e = np.sort(rng.uniform(0.0, 1.0, 32))
            elif mode == 1:                                      # anything, also outside the canvas and reversed
                e = rng.uniform(-0.5, 1.5, 32)
            else:                                                # degenerate: many equal, some not finite
                e = rng.choice(np.array([0.0, 0.25, 0.2500001, 0.5, 1.0, np.nan, np.inf, -np.inf]), 32)
            locs.append(e.astype(np.float32))
        reads = [blind.read_probe(r, l, p, h) for r, l, p in zip(rows, locs, probes)]
        for (labels, boxes, _), p in zip(reads, probes):
            assert len(labels) == len(boxes) <= 16 and all(2 * p[2] <= a + b < 2 * p[3] and a <= b for a, b in boxes)
        labels, boxes = blind.merge(h, w, reads)
        assert len(labels) == len(boxes) and all(len(b) == 4 and b[1] == 0.0 and b[3] == float(h) for b in boxes)
        assert all(0.0 <= b[0] and b[2] <= float(w) and b[2] - b[0] >= 1.0 for b in boxes)
        assert all(p[2] <= q[0] and p[0] + p[2] <= q[0] + q[2] for p, q in zip(boxes, boxes[1:]))
        assert (blind.decode([(h, w)], [probes], rows, locs)[0] is None) == (not labels)
        if labels:
            try:
                plan = long_lines.plan_windows(h, w, boxes)
                planned += 1
                assert plan[0].c0 == 0 and plan[-1].c1 == w and plan[-1].g1 == len(labels)
            except ValueError as e:
                assert str(e).startswith("plan_windows: ")
    assert planned > 0


# ----------------------------------------------------------------------------------------------------------- mnet_lq_windows_u8, host side
def test_windows_header_declares_exactly_the_bound_symbol_and_the_descriptor_layout(tmp_path):
    text = open(os.path.join(INCLUDE, "marconet_hip_windows.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(mnet_\w+)\s*\(", code)) == set(_lib.WINDOW_SYMBOLS) == {"mnet_lq_windows_u8"}
    assert len(_lib.WINDOW_SYMBOLS["mnet_lq_windows_u8"][1]) == 9
    cpath, exe = str(tmp_path / "probe.c"), str(tmp_path / "probe")
    fields = ("offset", "pitch", "h", "w", "dw", "scale")
    with open(cpath, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "marconet_hip_windows.h"\nint main(void) {\n'
                'printf("%d %d ' + "%d " * 6 + '\\n", (int)sizeof(mnet_lq_window), MNET_ABI_VERSION, '
                + ", ".join("(int)offsetof(mnet_lq_window, %s)" % n for n in fields) + ');\nreturn 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", INCLUDE, cpath])
    subprocess.check_call(["gcc", "-std=c99", "-I", INCLUDE, cpath, "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    S = _lib.LqWindow
    assert got == [ctypes.sizeof(S), _lib.ABI_VERSION] + [getattr(S, n).offset for n in fields]
    assert got == [32, 4, 0, 8, 12, 16, 20, 24] and [n for n, _ in S._fields_] == list(fields) and np.dtype(S).itemsize == 32
    lib = _lib.load()
    assert hasattr(lib, "mnet_lq_windows_u8") and lib.mnet_abi_version() == 4
    assert not set(_lib.WINDOW_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.MIXED_SYMBOLS) | set(_lib.QUAD_SYMBOLS) | set(_lib.CURVE_SYMBOLS))


def test_windows_entry_point_validates_arguments_without_device():
    lib = _lib.load()
    e_arg = lib.mnet_lq_from_u8(None, None, 0, 0, 0, None, 0, None)                                   # MNET_E_ARG
    ok = dict(src=64, src_bytes=1000, windows=128, n=2, dst_h=32, canvas_w=512, dst=256, form=_lib.LQ_FORM_F32_NCHW, stream=None)
    for change, status in ((dict(src=None), -1), (dict(windows=None), -1), (dict(dst=None), -1), (dict(n=0), -1), (dict(dst_h=0), -1),
                           (dict(canvas_w=0), -1), (dict(src_bytes=0), -1), (dict(form=_lib.LQ_FORM_U8_HWC), -1), (dict(form=7), -1),
                           (dict(windows=132), None), (dict(dst=258), None), (dict(n=2 ** 31 - 1, canvas_w=2 ** 20), -1)):
        a = dict(ok, **change)
        got = lib.mnet_lq_windows_u8(a["src"], a["src_bytes"], a["windows"], a["n"], a["dst_h"], a["canvas_w"], a["dst"], a["form"], a["stream"])
        assert got < 0 and (got == e_arg) == (status is not None), change                             # an alignment: MNET_E_ALIGN, another negative
        assert b"lq_windows_u8" in lib.mnet_last_error()


def test_check_windows_raises_the_geometry_errors_and_refuses_what_lies_outside():
    nbytes = 97 * 211 * 3
    pitch = 211 * 3
    assert [g.w for g in lq_device.check_windows([(0, pitch, 97, 211), (nbytes - 3, pitch, 1, 1), (5, 3, 7, 1)], nbytes)] == [211, 1, 1]
    with pytest.raises(ValueError, match="empty output"):
        lq_device.check_windows([(0, pitch, 0, 5)], nbytes)
    with pytest.raises(ValueError, match="empty output"):
        lq_device.check_windows([(0, pitch, 5, 0)], nbytes)
    with pytest.raises(lq_io.StripTooWide):
        lq_device.check_windows([(0, pitch, 8, 131)], nbytes)
    for bad in ((-1, pitch, 4, 4), (0, 11, 4, 4), (0, pitch, 97, 212), (3, pitch, 97, 211), (nbytes - 2, pitch, 1, 1), (0, pitch, 98, 4),
                (0, 2 ** 31, 1, 4)):
        with pytest.raises(ValueError, match="window 1 .*lies outside"):
            lq_device.check_windows([(0, pitch, 4, 4), bad], nbytes)
    tab = lq_device.window_table(lq_device.check_windows([(6, pitch, 31, 100)], nbytes), [(6, pitch, 31, 100)])
    g = lq_device.shape_geometry(31, 100)
    assert tab.dtype.itemsize == 32 and tab[0].tolist() == (6, pitch, 31, 100, g.dw, g.scale)
    assert lq_device.line_window(1000, 40, 300, 25, 125) == (1075, 900, 40, 100)


def test_build_script_registers_the_window_kernels():
    sh = open(os.path.join(ROOT, "marconet_amd", "csrc", "build.sh")).read()
    assert re.search(r'^SRCS="[^"]*\bwindow_kernels\b[^"]*"', sh, flags=re.M) and 'window_kernels) echo "-ffp-contract=off" ;;' in sh
    stamp = re.search(r'\[ "\$1" = window_kernels \] && cat ([^;]*);', sh).group(1)
    for name in ("lq_taps.h", "page_tile.h", "marconet_hip_windows.h"):
        assert name in stamp


# ------------------------------------------------------------------------------------------------------------------ the entry points' intake
def test_restore_lines_keeps_its_refusal_of_no_texts_and_reading_needs_a_device():
    """the host checks need neither weights on a device nor a launch: ``texts=None`` is refused by restore_lines as it always was; a None ENTRY is a
    request to read, which the encoder cannot serve from the CPU"""
    from marconet_amd import networks
    from marconet_amd.pipeline import MarconetPipeline
    pipe = MarconetPipeline(networks.TextContextEncoderV2(), networks.TSPGAN(), networks.TSPSRNet())
    line = np.zeros((32, 900, 3), np.uint8)
    with pytest.raises(ValueError, match="restore_lines needs texts: .*cut characters in half.*\\[None\\] \\* len\\(images\\)"):
        pipe.restore_lines([line], None)
    with pytest.raises(ValueError, match="restore_lines needs texts: .*HIP device"):
        pipe.restore_lines([line, line], [None, lq_io.alphabet()[10]])
    with pytest.raises(ValueError, match="one text per image"):
        pipe.restore_lines([line, line], [lq_io.alphabet()[10]])
    with pytest.raises(ValueError, match="restore_page needs texts: .*HIP device"):
        pipe.restore_page(np.zeros((60, 200, 3), np.uint8), [[0, 0, 100, 30]], [None])
