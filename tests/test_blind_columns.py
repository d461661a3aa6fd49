"""not-gpu: the pure-host definition of reading a vertical column blind (marconet_amd/blind_columns.py) — the ink profile against a plain double loop,
the first-pass cuts on hand-made profiles and on seeded synthetic columns, the probes of whole cells as properties, the way back from the virtual
strip to page rows, ``settle``'s totality — and the host side of mnet_row_ink_u8: the descriptor's C layout, the symbol table, the entry point's
argument checks (the library loads without a GPU).

The synthetic columns are the ones the rule was designed on: a column ``cw`` px wide (12..39) of n characters (2..19), cells whose heights are integers
within ±5 % of ``cw``, between two glyphs a flat gap of 8..20 % of ``cw`` (at least 2 rows: a cut BETWEEN two flat rows needs two) centred on the cell
boundary, every glyph row with ink, and a flat band of 2 rows through the middle of every glyph — the trap a cut must not fall into."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from marconet_amd import _lib, blind, blind_columns as bc, columns, pages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


# ------------------------------------------------------------------------------------------------------------------------------- row_ink
def _ink_loops(page, box):
    x1, y1, x2, y2 = box
    out = []
    for y in range(y1, y2):
        luma = [(77 * int(page[y, x, 0]) + 150 * int(page[y, x, 1]) + 29 * int(page[y, x, 2]) + 128) >> 8 for x in range(x1, x2)]
        out.append(sum(abs(luma[k + 1] - luma[k]) for k in range(len(luma) - 1)))
    return out


@pytest.mark.parametrize("channel", [0, 1, 2, None])
def test_row_ink_is_the_double_loop_channel_by_channel(channel):
    """one channel varying at a time: a wrong weight, weights swapped or a missing + 128 change the sums"""
    rng = np.random.default_rng(7 + (3 if channel is None else channel))
    page = np.full((9, 23, 3), 128, np.uint8)
    if channel is None:
        page = rng.integers(0, 256, page.shape, dtype=np.uint8)
    else:
        page[:, :, channel] = rng.integers(0, 256, page.shape[:2], dtype=np.uint8)
    for box in ([0, 0, 23, 9], [3, 2, 20, 7], [22, 0, 23, 9], [5, 8, 7, 9]):
        got = bc.row_ink(page, box)
        assert got.dtype == np.int32 and got.tolist() == _ink_loops(page, box), box
    assert bc.row_ink(page, [22, 0, 23, 9]).tolist() == [0] * 9                                   # w == 1
    # the rounding: R = 1 alone gives (77 + 128) >> 8 = 0, R = 2 gives (154 + 128) >> 8 = 1; without the + 128 both would be 0
    step = np.zeros((1, 2, 3), np.uint8)
    step[0, 1, 0] = 2
    assert bc.row_ink(step, [0, 0, 2, 1]).tolist() == [1]
    step[0, 1, 0] = 1
    assert bc.row_ink(step, [0, 0, 2, 1]).tolist() == [0]


def test_row_ink_ignores_polarity_and_is_zero_on_flat_rows():
    rng = np.random.default_rng(11)
    gray = rng.integers(0, 256, (12, 17), dtype=np.uint8)
    gray[4] = 90
    page = np.stack([gray] * 3, axis=2)
    a, b = bc.row_ink(page, [0, 0, 17, 12]), bc.row_ink(255 - page, [0, 0, 17, 12])
    assert a.tolist() == b.tolist() and a[4] == 0 and all(v > 0 for k, v in enumerate(a) if k != 4)


# ---------------------------------------------------------------------------------------------------------------------------- first_cuts
def test_first_cuts_on_hand_made_profiles():
    box = [3, 0, 13, 40]                                                     # cw 10, ch 40: n = 4; the first cut: t = 10, R = 40 // 16 = 2
    flat = [5] * 40
    assert bc.cell_count(box) == 4
    assert bc.first_cuts(box, flat) == [0, 10, 20, 30, 40]                   # equal cost everywhere: the smallest |r - t| wins, r = t
    snap = list(flat)
    snap[10] = snap[11] = 0                                                  # the cut between rows 10 and 11 is free: r = 11
    # ... and the later cuts are placed relative to it: t = 11 + rint(29 / 3) = 21, then 21 + rint(19 / 2) = 31 (half up), not the grid's 20, 30
    assert bc.first_cuts(box, snap) == [0, 11, 21, 31, 40]
    tie = list(flat)
    tie[8], tie[9], tie[10], tie[11] = 0, 1, 1, 0                            # r = 9 and r = 11 both cost 1 at |r - t| = 1, r = 10 costs 2: the smaller r
    assert bc.first_cuts(box, tie)[1] == 9
    far = list(flat)
    far[5] = far[6] = 0                                                      # r = 6 is free but 4 rows from t, outside R = 2: ignored
    assert bc.first_cuts(box, far) == [0, 10, 20, 30, 40]
    near = list(flat)
    near[7] = near[8] = 0                                                    # r = 8 = t - R is the radius' edge: taken
    assert bc.first_cuts(box, near)[1] == 8
    assert bc.first_cuts([0, 7, 10, 12], [1] * 5) == [7, 12] and bc.first_cuts([0, 0, 4, 6], [0] * 6) == [0, 3, 6]
    with pytest.raises(ValueError, match="profile of 40 rows"):
        bc.first_cuts(box, flat[:-1])
    with pytest.raises(ValueError, match="empty column"):
        bc.first_cuts([3, 5, 3, 9], [0] * 4)


def synthetic_column(rng, cw=None, n=None):
    """one column of the module's head → (page uint8 [ch, cw, 3], the true cell boundaries T_0 = 0 < ... < T_n = ch, per inner boundary its flat rows)"""
    cw = int(rng.integers(12, 40)) if cw is None else cw
    n = int(rng.integers(2, 20)) if n is None else n
    lo, hi = -(-95 * cw // 100), 105 * cw // 100                             # integers within ±5 % of cw
    heights = rng.integers(lo, hi + 1, n)
    T = [0] + [int(v) for v in np.cumsum(heights)]
    gaps = [max(2, int(np.rint(rng.uniform(0.08, 0.20) * cw))) for _ in range(n + 1)]
    page = rng.integers(0, 256, (T[-1], cw, 3), dtype=np.uint8)
    page[:, 0], page[:, 1] = 0, 255                                          # every glyph row has ink
    bg = rng.integers(0, 256, 3, dtype=np.uint8)
    flat = []
    for j, (t, g) in enumerate(zip(T, gaps)):
        a, b = max(t - g // 2, 0), min(t + g - g // 2, T[-1])
        page[a:b] = bg
        flat.append((a, b))
    for j in range(n):                                                       # the band through the middle of glyph j
        mid = (flat[j][1] + flat[j + 1][0]) // 2
        page[mid - 1:mid + 1] = bg
    return page, T, flat


def test_first_cuts_on_synthetic_columns_fall_into_the_right_gaps():
    rng = np.random.default_rng(20250121)
    for k in range(300):
        page, T, flat = synthetic_column(rng)
        box = [0, 0, page.shape[1], page.shape[0]]
        ink = bc.row_ink(page, box)
        cuts = bc.first_cuts(box, ink)
        assert len(cuts) == len(T), (k, cuts, T)                             # n is the number drawn
        assert cuts[0] == 0 and cuts[-1] == T[-1] and all(a < b for a, b in zip(cuts, cuts[1:])), (k, cuts)
        for j in range(1, len(T) - 1):
            a, b = flat[j]
            assert a < cuts[j] < b and ink[cuts[j] - 1] == 0 and ink[cuts[j]] == 0, (k, j, cuts, T)


def test_first_cuts_increase_strictly_on_any_profile():
    rng = np.random.default_rng(5)
    for _ in range(400):
        cw, ch = int(rng.integers(1, 30)), int(rng.integers(1, 200))
        y1 = int(rng.integers(0, 50))
        ink = rng.integers(0, 4, ch) * rng.integers(0, 2, ch)
        cuts = bc.first_cuts([2, y1, 2 + cw, y1 + ch], ink)
        assert cuts[0] == y1 and cuts[-1] == y1 + ch and len(cuts) == bc.cell_count([2, y1, 2 + cw, y1 + ch]) + 1
        assert all(a < b for a, b in zip(cuts, cuts[1:])), (cw, ch, cuts)


# ---------------------------------------------------------------------------------------------------------------------- plan_cell_probes
def test_plan_cell_probes_properties():
    rng = np.random.default_rng(3)
    seen_multi = 0
    for _ in range(300):
        pw = int(rng.choice([32, 64, 128, 384, 512]))
        n = int(rng.integers(1, 60))
        widths = [int(v) for v in rng.integers(1, min(pw, 80) + 1, n)]
        o = columns.cell_offsets(widths)
        probes = bc.plan_cell_probes(widths, pw)
        seen_multi += len(probes) > 1
        covered = set()
        for k, (g0, g1, c0, c1, lo, hi) in enumerate(probes):
            assert 0 <= g0 < g1 <= n and c0 == o[g0] and c1 == o[g1]                                # whole cells
            assert c1 - c0 <= pw and g1 - g0 <= pw // 32                                            # the caps
            assert c0 <= lo <= hi <= c1                                                             # what it owns lies inside it
            covered |= set(range(g0, g1))
            # the longest run: one more cell would break a cap (the last probe grows to the left, the others to the right)
            if k < len(probes) - 1:
                assert g1 < n and (g1 + 1 - g0 > pw // 32 or o[g1 + 1] - c0 > pw)
            elif g0 > 0:
                assert n - g0 + 1 > pw // 32 or o[n] - o[g0 - 1] > pw
        assert covered == set(range(n))                                                             # every cell lies in some probe
        assert probes[0][4] == 0 and probes[-1][5] == o[n] and probes[-1][1] == n
        assert all(p[5] == q[4] for p, q in zip(probes, probes[1:]))                                # the ownership intervals tile [0, Wv)
        assert all(p[0] < q[0] and q[0] <= p[1] for p, q in zip(probes, probes[1:]))                # they advance, and leave no cell out
        for p, q in zip(probes, probes[1:-1]):
            assert q[0] - p[0] == max(1, (p[1] - p[0]) // 2)                                        # half a probe later
        assert all(q[4] == (q[2] + p[3]) // 2 for p, q in zip(probes, probes[1:]))                  # the middle of the overlap
    assert seen_multi > 100
    assert bc.plan_cell_probes([32] * 12) == [(0, 12, 0, 384, 0, 384)]                              # 12 square cells are one probe at the default
    assert [p[:2] for p in bc.plan_cell_probes([32] * 18)] == [(0, 12), (6, 18)]
    assert [p[:2] for p in bc.plan_cell_probes([32] * 25)] == [(0, 12), (6, 18), (12, 24), (13, 25)]
    assert bc.plan_cell_probes([32] * 18)[0][4:] == (0, (6 * 32 + 384) // 2)
    windows = bc.probe_windows(bc.plan_cell_probes([30, 34] * 9))
    assert [(w.g0, w.g1, w.c0, w.c1) for w in windows] == [(0, 12, 0, 384), (6, 18, 192, 576)]


def test_plan_cell_probes_refusals():
    with pytest.raises(ValueError, match=r"region 4: character 2: its cell is 385 px wide at height 32: a probe of 384 px cannot hold it"):
        bc.plan_cell_probes([32, 32, 385, 32], 384, region=4)
    with pytest.raises(ValueError, match="character 0: its cell is 40 px wide"):
        bc.plan_cell_probes([40], 32)
    with pytest.raises(ValueError, match="probe_width must be a multiple of 4"):
        bc.plan_cell_probes([32], 30)
    with pytest.raises(ValueError, match="without a cell"):
        bc.plan_cell_probes([])


# ------------------------------------------------------------------------------------------------------------------------- strip_to_rows
def test_strip_to_rows_is_monotone_and_exact_at_cell_boundaries():
    rng = np.random.default_rng(9)
    for _ in range(100):
        n = int(rng.integers(1, 12))
        cuts = [int(v) for v in np.cumsum(rng.integers(1, 40, n + 1))]
        widths = [int(v) for v in rng.integers(1, 50, n)]
        o = columns.cell_offsets(widths)
        assert bc.strip_to_rows(o, cuts, widths) == [float(c) for c in cuts]                        # exact at the boundaries, x = Wv included
        xs = np.sort(rng.uniform(0, o[-1], 200))
        rows = bc.strip_to_rows(xs, cuts, widths)
        assert all(isinstance(r, float) for r in rows) and all(a <= b for a, b in zip(rows, rows[1:]))
        assert cuts[0] <= rows[0] and rows[-1] <= cuts[-1]
        j = int(rng.integers(0, n))
        mid = bc.strip_to_rows(o[j] + widths[j] / 2, cuts, widths)
        assert mid == cuts[j] + (widths[j] / 2) * (cuts[j + 1] - cuts[j]) / widths[j]


# -------------------------------------------------------------------------------------------------------------------------------- settle
def test_settle_never_raises_and_its_result_is_one_the_given_path_accepts():
    rng = np.random.default_rng(13)
    emptied = kept_all = 0
    for trial in range(400):
        cw, ch = int(rng.integers(4, 40)), int(rng.integers(1, 300))
        x1, y1 = int(rng.integers(0, 20)), int(rng.integers(0, 20))
        box = [x1, y1, x1 + cw, y1 + ch]
        scale = int(rng.integers(1, 9))
        n = int(rng.integers(0, 24))
        ys = np.sort(rng.uniform(y1 - 5, y1 + ch + 5, 2 * n)) if trial % 3 else rng.uniform(y1 - 50, y1 + ch + 50, 2 * n)
        cb = [[float(x1), float(ys[2 * k]), float(x1 + cw), float(ys[2 * k + 1])] for k in range(n)]
        if n and trial % 7 == 0:
            cb[int(rng.integers(0, n))][1] = float(rng.choice([np.nan, np.inf, -np.inf]))
        labels = [int(v) for v in rng.integers(0, 6735, n)]
        got_l, got_b = bc.settle(box, labels, cb, scale)
        assert len(got_l) == len(got_b) <= n
        pairs = list(zip(labels, cb))
        it = iter(pairs)
        assert all(any(l == p[0] and b == p[1] for p in it) for l, b in zip(got_l, got_b))         # a subsequence of the reading, in order
        emptied += not got_l
        kept_all += len(got_l) == n > 0
        if got_l:
            cuts = columns.cell_cuts(box, len(got_l), got_b)
            columns.check_columns(y1 + ch, x1 + cw, [box], [True], [cuts], scale, 0)                # the given path's refusals: none
            assert bc.settle(box, got_l, got_b, scale) == (got_l, got_b)                            # settled stays settled
    assert emptied > 5 and kept_all > 5
    # the shortest cell goes, ties the later: cells of 10, 2, 2, 10 rows at scale 1 (a cell needs 8 rows) lose character 2, then what was character 1
    cb = [[0, 0, 8, 9], [0, 11, 8, 11.5], [0, 13, 8, 13.5], [0, 15, 8, 24]]
    assert columns.cell_cuts([0, 0, 8, 24], 4, cb) == [0, 10, 12, 14, 24]
    assert bc.settle([0, 0, 8, 24], [1, 2, 3, 4], cb, 1) == ([1, 4], [[0.0, 0.0, 8.0, 9.0], [0.0, 15.0, 8.0, 24.0]])
    assert bc.settle([0, 0, 8, 24], [1, 2, 3, 4], cb, 4) == ([1, 2, 3, 4], [[float(v) for v in b] for b in cb])     # 4 x 2 rows = 8: all stay
    assert bc.settle([0, 0, 8, 1], [5], [[0, 0, 8, 1]], 4) == ([], []) and bc.settle([0, 0, 8, 24], [], [], 4) == ([], [])
    assert bc.settle([0, 0, 8, 24], [5], [[0, 0, 8, 24]], "x") == ([], [])                             # total: a scale that is none settles to nothing


def test_decode_maps_the_reading_back_to_page_rows():
    """one probe over a column of three cells: the encoder's pairs in the virtual strip become boxes in page rows, through the cells' own scales"""
    box, cuts = [10, 100, 42, 200], [100, 132, 168, 200]                                            # cells 32, 36 and 32 rows high, 32 px wide
    widths = columns.cell_widths(box, cuts)
    assert widths == [32, 28, 32]
    plans = [dict(box=box, first_cuts=cuts, widths=widths, probes=bc.plan_cell_probes(widths))]
    rows = [[7, 6735, 9, 6735, 11] + [6735] * 59]
    locs = np.zeros((1, 32), np.float32)
    locs[0, :6] = np.array([2, 30, 34, 58, 62, 90], np.float32) / 512
    out = bc.decode(plans, rows, locs, scale=4)[0]
    assert out["labels"] == [7, 9, 11] and len(out["text"]) == 3 and out["overflow"] is False and out["first_cuts"] == cuts
    assert out["probes"] == [(0, 3, 0, 92, 0, 92)]
    assert out["char_boxes"] == [[10.0, 102.0, 42.0, 130.0], [10.0, 132 + 2 * 36 / 28, 42.0, 132 + 26 * 36 / 28], [10.0, 170.0, 42.0, 198.0]]
    assert out["cuts"] == columns.cell_cuts(box, 3, out["char_boxes"]) == [100, 132, 167, 200]
    assert bc.decode(plans, [[6735] * 64], locs, scale=4) == [None]                                 # an empty reading


# ---------------------------------------------------------------------------------------------------------- mnet_row_ink_u8, host side
def test_rowink_header_declares_exactly_the_bound_symbol_and_the_descriptor_layout(tmp_path):
    text = open(os.path.join(INCLUDE, "marconet_hip_rowink.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(mnet_\w+)\s*\(", code)) == set(_lib.ROWINK_SYMBOLS) == {"mnet_row_ink_u8"}
    assert len(_lib.ROWINK_SYMBOLS["mnet_row_ink_u8"][1]) == 8
    cpath, exe = str(tmp_path / "probe.c"), str(tmp_path / "probe")
    fields = ("offset", "pitch", "h", "w", "out")
    with open(cpath, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "marconet_hip_rowink.h"\nint main(void) {\n'
                'printf("%d %d ' + "%d " * 5 + '\\n", (int)sizeof(mnet_ink_box), MNET_ABI_VERSION, '
                + ", ".join("(int)offsetof(mnet_ink_box, %s)" % n for n in fields) + ');\nreturn 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", INCLUDE, cpath])
    subprocess.check_call(["gcc", "-std=c99", "-I", INCLUDE, cpath, "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    S = _lib.RowInkBox
    assert ctypes.sizeof(S) == 24 and np.dtype(S).itemsize == 24
    assert got == [24, 4, 0, 8, 12, 16, 20] == [ctypes.sizeof(S), _lib.ABI_VERSION] + [getattr(S, n).offset for n in fields]
    assert [n for n, _ in S._fields_] == list(fields)
    lib = _lib.load()
    assert hasattr(lib, "mnet_row_ink_u8") and lib.mnet_abi_version() == 4                          # the built library exports it
    others = [getattr(_lib, name) for name in dir(_lib) if name.endswith("SYMBOLS") and name != "ROWINK_SYMBOLS"]
    assert len(others) >= 9 and not any(set(_lib.ROWINK_SYMBOLS) & set(t) for t in others)


def test_rowink_entry_point_validates_arguments_without_device():
    lib = _lib.load()
    e_arg = lib.mnet_lq_from_u8(None, None, 0, 0, 0, None, 0, None)                                 # MNET_E_ARG
    ok = dict(src=64, src_bytes=1000, boxes=128, n=2, max_h=5, dst=256, dst_len=10, stream=None)
    for change, status in ((dict(src=None), -1), (dict(boxes=None), -1), (dict(dst=None), -1), (dict(n=0), -1), (dict(max_h=0), -1),
                           (dict(src_bytes=0), -1), (dict(dst_len=0), -1), (dict(n=65536), -1), (dict(n=65535, max_h=2 ** 31 - 1), -1),
                           (dict(n=8192, max_h=8192), -1), (dict(boxes=132), None), (dict(dst=258), None)):
        a = dict(ok, **change)
        got = lib.mnet_row_ink_u8(a["src"], a["src_bytes"], a["boxes"], a["n"], a["max_h"], a["dst"], a["dst_len"], a["stream"])
        assert got < 0 and (got == e_arg) == (status is not None), change                           # an alignment: MNET_E_ALIGN, another negative
        assert b"row_ink_u8" in lib.mnet_last_error()


def test_example_scripts_take_a_vertical_region_without_text_only_with_blind_columns(tmp_path):
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("restore_page_example", os.path.join(ROOT, "examples", "restore_page.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    path = str(tmp_path / "regions.json")
    with open(path, "w", encoding="utf8") as f:
        json.dump([dict(box=[5, 5, 30, 90], vertical=True), dict(box=[40, 5, 90, 25], text="cd")], f)
    with pytest.raises(SystemExit, match='except for a "vertical" region without --blind-columns'):
        mod.load_regions(path)
    boxes, texts, char_boxes, quads, vertical, polygons = mod.load_regions(path, blind_columns=True)
    assert texts == [None, "cd"] and vertical == [True, False] and quads is None and polygons is None and char_boxes is None
    for script in ("restore_page.py", "restore_regions.py"):
        r = subprocess.run([os.sys.executable, os.path.join(ROOT, "examples", script), "--help"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "--blind-columns" in r.stdout


def test_the_pieces_the_reading_uses_are_the_project_s_own():
    assert bc.LQ_H == 32 and bc.ROW_H == 128 and pages.MIN_RECT_H_DIV == 16 and blind.SLOTS == 16
