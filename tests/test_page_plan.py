"""not-gpu: the packed layout of a page's windows (marconet_amd/restore.py: page_layout) and the ink table of the blind columns
(marconet_amd/blind_columns.py: ink_table) — what sits at which byte of the ragged batch and which row of ``lq`` belongs to which window, host
arithmetic that a GPU test would only see as wrong pixels.  The records are ``regions.normalize_regions``' of the mixed scene of
tests/regions_scene.py: lines, columns, quadrilaterals and curves, two of them not restored; the windows are made by hand, one to three per
region, requested in a region order that interleaves the kinds."""
import numpy as np
import pytest

from marconet_amd import _lib, blind_columns as bc, columns, regions
from marconet_amd.restore import page_layout, region_geometry
from tests import regions_scene as rs

W = rs.PAGE_W
REGS = [dict(box=[10, 5, 110, 45]),                                                  # 0 a line
        dict(quad=[(30, 12), (95, 20), (92, 36), (27, 28)]),                         # 1 a quadrilateral over it
        dict(polygon=rs.arc(64.0, 60.0, 22.0, 38.0, 160.0, 20.0, 7)),                # 2 an arc over both
        dict(box=[0, 50, 20, 60]),                                                   # 3 a line that is not restored
        dict(box=[120, 30, 140, 66], vertical=True),                                 # 4 a column of two cells
        dict(quad=rs.TWIN),                                                          # 5
        dict(polygon=rs.TAPERED),                                                    # 6
        dict(box=[112, 2, 148, 26]),                                                 # 7 a second line
        dict(box=[100, 40, 112, 68], vertical=True)]                                 # 8 a column that is not restored
RESTORED = [True, True, True, False, True, True, True, True, False]


@pytest.fixture(scope="module")
def scene():
    recs = regions.normalize_regions(rs.PAGE_H, W, REGS, RESTORED, ["ab"] * len(REGS), None, 1, 3, "order", 32)
    assert [r["kind"] for r in recs] == ["line", "quad", "curve", "line", "column", "quad", "curve", "line", "column"] and "widths" not in recs[8]
    sizes, _, maps = region_geometry(recs, None)
    o = columns.cell_offsets(recs[4]["widths"])
    assert sizes[4] == (32, o[2]) and sizes[0] == (40, 100) and sizes[1] == (recs[1]["ch"], recs[1]["cw"]) and maps[1] is not None and maps[2] is None
    cw = lambda i: sizes[i][1]
    wins = {0: [(0, 0, 0, 60), (0, 1, 50, 100)],
            1: [(1, 0, 0, cw(1))],
            2: [(2, 0, 0, cw(2) // 2), (2, 1, cw(2) // 3, cw(2) - 5), (2, 2, cw(2) - 9, cw(2))],
            4: [(4, 0, 0, o[1], 0, 1), (4, 1, o[1], o[2], 1, 2)],
            5: [(5, 0, 0, cw(5) // 2), (5, 1, cw(5) // 2 - 3, cw(5))],
            6: [(6, 0, 2, cw(6))],
            7: [(7, 0, 0, 36)]}
    order = [6, 0, 4, 1, 7, 2, 5]                                                    # curve, line, column, quad, line, curve, quad
    return recs, maps, [w for i in order for w in wins[i]]


def _kind(recs, key):
    return recs[key[0]]["kind"]


@pytest.mark.parametrize("lines_as_views", [False, True])
def test_every_window_has_one_place_and_the_rows_come_back_in_the_order_asked(scene, lines_as_views):
    recs, maps, windows = scene
    lay = page_layout(recs, maps, W, lines_as_views, windows)
    want = [w[:2] for w in windows]
    size = {w[:2]: ((recs[w[0]]["box"][3] - recs[w[0]]["box"][1] if _kind(recs, w) == "line" else 32 if _kind(recs, w) == "column" else recs[w[0]]["ch"]),
                    w[3] - w[2]) for w in windows}
    # exactly one slot or one view per window
    assert len(lay.views) == len(lay.view_keys) and sorted(lay.view_keys + list(lay.slots)) == sorted(want) and len(set(want)) == len(want)
    assert set(lay.view_keys) == ({k for k in want if _kind(recs, k) == "line"} if lines_as_views else set())
    # a view of line i, columns [c0, c1)
    for key, view in zip(lay.view_keys, lay.views):
        x1, y1, _, y2 = recs[key[0]]["box"]
        c0, c1 = next(w[2:4] for w in windows if w[:2] == key)
        assert view == ((y1 * W + x1 + c0) * 3, 3 * W, y2 - y1, c1 - c0)
    # a slot is 3·h·w bytes; slots are disjoint, inside the buffer, the kinds in order, each contiguous from its base
    spans = sorted((off, off + 3 * h * w, key) for key, ((h, w), off) in lay.slots.items())
    assert all(lay.slots[key][0] == size[key] for key in lay.slots)
    assert spans[0][0] == 0 and spans[-1][1] == lay.nbytes and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    rank = {"line": 0, "column": 1, "quad": 2, "curve": 3}
    kinds = [rank[_kind(recs, key)] for _, _, key in spans]
    assert kinds == sorted(kinds) and set(kinds) == ({1, 2, 3} if lines_as_views else {0, 1, 2, 3})
    first = {k: min(s[0] for s in spans if rank[_kind(recs, s[2])] == k) for k in set(kinds)}
    assert first[1] == lay.head and first[2] == lay.q_base and first[3] == lay.c_base and lay.head == (0 if lines_as_views else 3 * 40 * 60 + 3 * 40 * 50 + 3 * 24 * 36)
    assert [c[0] for c in lay.crops] == [lay.slots[k][1] for k in lay.slots if _kind(recs, k) == "line"] and (not lay.crops or lay.crops[0][0] == 0)
    assert lay.crops == ([] if lines_as_views else [(0, slice(5, 45), slice(10, 70)), (7200, slice(5, 45), slice(60, 110)), (13200, slice(2, 26), slice(112, 148))])
    # the tables are the modules' own, from those bases, and their offsets are the slots'
    assert lay.q_tab.dtype == np.dtype(_lib.QuadCrop) and lay.c_tab.dtype == np.dtype(_lib.CurveCrop) and lay.cell_tab.dtype == np.dtype(_lib.ColumnCell)
    assert lay.q_tab["offset"].tolist() == [lay.slots[k][1] for k in [(1, 0), (5, 0), (5, 1)]] and lay.q_tab["c0"].tolist() == [0, 0, recs[5]["cw"] // 2 - 3]
    assert lay.c_tab["offset"].tolist() == [lay.slots[k][1] for k in [(6, 0), (2, 0), (2, 1), (2, 2)]] and lay.c_tab["seg0"].tolist() == [0] + [len(recs[6]["segs"])] * 3
    assert len(lay.c_segs) == len(recs[6]["segs"]) + len(recs[2]["segs"]) and sorted(set(lay.cell_tab["offset"].tolist())) == [lay.slots[(4, 0)][1], lay.slots[(4, 1)][1]]
    # the rows as they are produced — the views, then the slots in the caller's order — and the way back to the order asked
    produced = lay.view_keys + list(lay.slots)
    assert lay.have == produced and (produced if lay.order is None else [produced[j] for j in lay.order]) == want
    assert (lay.order is None) == (not lines_as_views)                               # all packed: produced in the caller's order; views come first
    assert [k for k in want if k in lay.slots] == list(lay.slots)


def test_one_source_keeps_the_order_and_without_head_and_columns_the_quads_start_at_0(scene):
    recs, maps, windows = scene
    warped = [w for w in windows if recs[w[0]]["kind"] in ("quad", "curve")]
    lay = page_layout(recs, maps, W, True, warped + [(0, 0, 0, 60)])
    assert lay.head == 0 and lay.q_base == 0 and len(lay.cell_tab) == 0 and min(off for _, off in lay.slots.values()) == 0 == lay.slots[(1, 0)][1]
    assert lay.order is not None and lay.view_keys == [(0, 0)]                        # the view is produced first, asked for last
    lay = page_layout(recs, maps, W, True, warped)
    assert lay.order is None and lay.have == [w[:2] for w in warped] and lay.views == []
    lay = page_layout(recs, maps, W, False, [])
    assert lay.nbytes == 0 and lay.slots == {} and lay.have == [] and lay.order is None


def test_a_window_that_cannot_hold_a_cell_is_refused_by_the_layout():
    """one cell of 140 x 8 px is 560 px wide at height 32: no window of at most 512 columns ends on its boundary — ``gather_table``'s refusal"""
    recs = regions.normalize_regions(rs.PAGE_H, W, [dict(box=[5, 30, 145, 38], vertical=True)], [True], ["a"], None, 1, 0, "order", 32)
    assert recs[0]["widths"] == [560]
    with pytest.raises(ValueError, match=r"the window of characters 0..1 spans columns 0..512 of the virtual strip, not its cells' 0..560"):
        page_layout(recs, [None], W, False, [(0, 0, 0, 512, 0, 1)])
    assert page_layout(recs, [None], W, False, [(0, 0, 0, 560, 0, 1)]).nbytes == 3 * 32 * 560


def test_ink_table_is_the_boxes_as_views_of_the_page():
    boxes = [[4, 3, 20, 291], [30, 10, 46, 410]]
    tab, starts, total = bc.ink_table(boxes, 200)
    assert tab.dtype == np.dtype(_lib.RowInkBox) and starts == [0, 288] and total == 688
    assert [tuple(int(v) for v in t) for t in tab] == [((3 * 200 + 4) * 3, 600, 288, 16, 0), ((10 * 200 + 30) * 3, 600, 400, 16, 288)]
    assert bc.ink_table([], 200)[1:] == ([], 0)
