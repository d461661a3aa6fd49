"""not-gpu: the pure-host definition of finding a page's text lines (marconet_amd/layout.py) — both ink profiles against a plain double loop, the
noise floor at its edge, the cut on hand-written profiles, the two-column scene the rules were tried on (tests/layout_scene.py), fixed scenes,
properties on seeded random pages — and the host side of mnet_box_ink_u8: the descriptor's C layout, the symbol table, build.sh, the entry point's
argument checks (the library loads without a GPU), examples/restore_scan.py's arguments and its JSON."""
import ctypes
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

from marconet_amd import _lib, blind_columns as bc, layout
from tests import layout_scene as ls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


# ------------------------------------------------------------------------------------------------------------------------------- box_ink
def _ink_loops(page, box, floor):
    x1, y1, x2, y2 = box
    rows, cols = [0] * (y2 - y1), [0] * (x2 - x1)
    for y in range(y1, y2):
        luma = [(77 * int(page[y, x, 0]) + 150 * int(page[y, x, 1]) + 29 * int(page[y, x, 2]) + 128) >> 8 for x in range(x1, x2)]
        for k in range(len(luma) - 1):
            d = abs(luma[k + 1] - luma[k])
            if d >= floor:
                rows[y - y1] += d
                cols[k] += d
    return rows, cols


def test_box_ink_is_the_double_loop_on_random_boxes():
    rng = np.random.default_rng(20250301)
    page = rng.integers(0, 256, (20, 34, 3), dtype=np.uint8)
    boxes = [[0, 0, 34, 20], [33, 0, 34, 20], [5, 7, 6, 8], [0, 19, 34, 20]]
    for _ in range(12):
        x1, y1 = int(rng.integers(0, 33)), int(rng.integers(0, 19))
        boxes.append([x1, y1, int(rng.integers(x1 + 1, 35)), int(rng.integers(y1 + 1, 21))])
    for box in boxes:
        for floor in (0, 1, 24, 100, 255):
            rows, cols = layout.box_ink(page, box, floor)
            want = _ink_loops(page, box, floor)
            assert rows.dtype == cols.dtype == np.int32 and (rows.tolist(), cols.tolist()) == want, (box, floor)
            assert cols[-1] == 0 and rows.sum() == cols.sum()
        for floor in (0, 1):
            assert np.array_equal(layout.box_ink(page, box, floor)[0], bc.row_ink(page, box))


def test_the_floor_at_its_edge():
    """grey steps of exactly floor - 1, floor and floor + 1 (a grey level is its own luma: 77 + 150 + 29 = 256)"""
    floor = 24
    for step, kept in ((floor - 1, False), (floor, True), (floor + 1, True)):
        page = np.full((3, 4, 3), 100, np.uint8)
        page[:, 2:] = 100 + step
        rows, cols = layout.box_ink(page, [0, 0, 4, 3], floor)
        assert rows.tolist() == [step if kept else 0] * 3 and cols.tolist() == [0, 3 * step if kept else 0, 0, 0]
        rows, cols = layout.box_ink(255 - page, [0, 0, 4, 3], floor)                                 # polarity-free
        assert rows.tolist() == [step if kept else 0] * 3
    page = np.full((1, 2, 3), 0, np.uint8)
    page[0, 1] = 255
    assert layout.box_ink(page, [0, 0, 2, 1], 255)[0].tolist() == [255]


# ----------------------------------------------------------------------------------------------------------------------------------- cut
def test_cut_on_hand_written_profiles():
    assert layout.cut([0, 0, 0], 2) == [] and layout.cut([], 1) == []                               # all blank
    assert layout.cut([3, 1, 9], 1) == [(0, 3)]                                                     # no blank
    assert layout.cut([0, 0, 5, 5, 0], 1) == [(2, 4)]                                               # the ends are trimmed whatever min_gap
    assert layout.cut([0, 0, 5, 5, 0], 9) == [(2, 4)]
    assert layout.cut([1, 0, 0, 1], 3) == [(0, 4)]                                                  # a run of min_gap - 1 does not split
    assert layout.cut([1, 0, 0, 0, 1], 3) == [(0, 1), (4, 5)]                                       # a run of exactly min_gap does
    assert layout.cut([0, 7, 0, 7, 0, 0, 7, 7, 0, 0, 0, 7, 0], 2) == [(1, 4), (6, 8), (11, 12)]
    assert layout.cut([1, 0, 1], 0) == [(0, 1), (2, 3)]                                             # min_gap under 1 is 1
    assert layout.pixel_profile([0, 4, 0, 0, 2, 0]).tolist() == [0, 4, 4, 0, 2, 2]                  # an edge keeps both of its pixels


# ------------------------------------------------------------------------------------------------------------------- the two-column scene
@pytest.fixture(scope="module")
def scene():
    page, lines = ls.two_columns()
    return dict(page=page, lines=lines, found=layout.find_lines_host(page, text_h=ls.TEXT_H))


def test_two_columns_are_found_line_by_line_in_reading_order(scene):
    found, tight = scene["found"], ls.expected_tight(scene["lines"])
    assert len(tight) == 24 and found["tight"] == tight and found["skipped"] == []
    # pass 1 (Y): the page → the band of the columns, the wide line; 2 (X): the band → two blocks, the wide line trimmed; 3 (Y): the blocks → their
    # lines; 4 (X): the ragged lines trimmed; 5 and 6 change nothing
    assert found["passes"] == 6
    # allowances: between two lines of a column half the blank rows (pitch 14: 2 rows → 1, pitch 15: 3 → 1), at the page's side everything up to it
    # capped by pad = 3, in the gutter of 30 half of it capped too
    left, right, wide = tight[:12], tight[12:23], tight[23]
    grown = found["boxes"]
    assert grown[0] == [left[0][0] - 3, left[0][1] - 3, left[0][2] + 3, left[0][3] + 1]
    assert grown[5] == [left[5][0] - 3, left[5][1] - 1, left[5][2] + 3, left[5][3] + 1]
    assert grown[12] == [right[0][0] - 3, right[0][1] - 3, right[0][2] + 3, right[0][3] + 1]
    assert grown[23] == [wide[0] - 3, wide[1] - 3, wide[2] + 3, wide[3] + 3]
    for g, t in zip(grown, tight):
        assert all(0 <= a - b <= 3 for a, b in ((t[0], g[0]), (t[1], g[1]), (g[2], t[2]), (g[3], t[3])))
    _check_disjoint_inside(grown, 600, 400)


def test_boxes_grow_by_min_pad_allowance(scene):
    page = scene["page"]
    params = layout.line_params(600, ls.TEXT_H)
    assert params == dict(text_h=12, floor=24, pad=3, min_h=3, min_w=6, max_h=48)
    profiles = lambda boxes, axis: [layout.box_ink(page, b, 24)[axis] for b in boxes]
    boxes, allows, passes = layout.xy_cut(profiles, 600, 400, ls.TEXT_H)
    assert boxes == scene["found"]["tight"] and passes == 6
    assert scene["found"]["boxes"] == [[b[0] - min(3, a[0]), b[1] - min(3, a[1]), b[2] + min(3, a[2]), b[3] + min(3, a[3])] for b, a in zip(boxes, allows)]
    assert allows[0][:2] == [29, 40] and allows[1][1] == 1 and allows[0][3] == 1                     # the page's side; half of 2 blank rows
    wide = layout.find_lines_host(page, text_h=ls.TEXT_H, pad=1000)["boxes"]                        # grown by the whole allowance: still disjoint
    _check_disjoint_inside(wide, 600, 400)
    assert layout.find_lines_host(page, text_h=ls.TEXT_H, pad=0)["boxes"] == boxes
    assert layout.line_params(3508) == dict(text_h=35, floor=24, pad=8, min_h=8, min_w=17, max_h=140) and layout.line_params(200)["text_h"] == 8
    for bad in (dict(text_h=0), dict(floor=256), dict(floor=-1), dict(pad=-1), dict(max_h=1.5)):
        with pytest.raises(ValueError):
            layout.line_params(600, **bad)


def _check_disjoint_inside(boxes, H, W):
    for i, a in enumerate(boxes):
        assert 0 <= a[0] < a[2] <= W and 0 <= a[1] < a[3] <= H, a
        for b in boxes[:i]:
            assert not (a[0] < b[2] and b[0] < a[2] and a[1] < b[3] and b[1] < a[3]), (a, b)


# --------------------------------------------------------------------------------------------------------------------------- fixed scenes
def test_a_blank_page_and_a_page_of_ink():
    rng = np.random.default_rng(3)
    blank = layout.find_lines_host(ls.paper(rng, 120, 90))
    assert blank == dict(boxes=[], tight=[], skipped=[], passes=3)                                  # the page vanishes in pass 1; 2 and 3 change nothing
    ink = rng.integers(0, 2, (40, 90, 1), dtype=np.uint8).repeat(3, axis=2) * 200
    assert (layout.box_ink(ink, [0, 0, 90, 40], 24)[0] > 0).all() and (layout.pixel_profile(layout.box_ink(ink, [0, 0, 90, 40], 24)[1]) > 0).all()
    full = layout.find_lines_host(ink, text_h=10)
    assert full == dict(boxes=[[0, 0, 90, 40]], tight=[[0, 0, 90, 40]], skipped=[], passes=2)
    assert layout.find_lines_host(np.zeros((1, 1, 3), np.uint8))["boxes"] == []
    thin = rng.integers(0, 256, (1, 300, 3), dtype=np.uint8)                                        # a page lower than min_h = 2
    assert layout.find_lines_host(thin)["boxes"] == [] and len(layout.find_lines_host(thin, min_h=0)["boxes"]) >= 1


def test_a_gutter_one_pixel_under_gap_x_does_not_split():
    page, lines = ls.two_columns(gutter=2 * ls.TEXT_H, wide=False)
    assert layout.find_lines_host(page, text_h=ls.TEXT_H)["tight"] == ls.expected_tight(lines)
    page, lines = ls.two_columns(gutter=2 * ls.TEXT_H - 1, wide=False)
    found = layout.find_lines_host(page, text_h=ls.TEXT_H)
    x1, x2 = min(b[0] for b in lines) - 1, max(b[2] for b in lines) + 1
    assert found["tight"] == [] and [s["box"] for s in found["skipped"]] == [[x1, 40, x2, 40 + 11 * 14 + ls.TEXT_H]]      # one block, both columns: too tall
    assert "max_h = 48" in found["skipped"][0]["reason"]


def test_specks_are_dropped_and_a_tall_block_is_skipped():
    page, line = ls.specks_and_figure()
    found = layout.find_lines_host(page, text_h=12)
    assert found["tight"] == ls.expected_tight([line])
    assert [s["box"] for s in found["skipped"]] == [[29, 150, 91, 199]]
    loose = layout.find_lines_host(page, text_h=12, min_h=0, min_w=0, max_h=49)
    assert loose["tight"] == ls.expected_tight([line]) + [[249, 100, 252, 101], [19, 120, 21, 121], [119, 120, 121, 121], [269, 140, 273, 144], [29, 150, 91, 199]]
    assert loose["skipped"] == []


# ------------------------------------------------------------------------------------------------------------------------ random pages
@pytest.mark.parametrize("chunk", range(5))
def test_properties_on_seeded_random_pages(chunk):
    for seed in range(12 * chunk, 12 * chunk + 12):                                                 # 60 pages in all
        page = ls.random_page(seed)
        H, W = page.shape[:2]
        floor, text_h = (24, 0, 1, 60)[seed % 4], (8, 12, 5)[seed % 3]
        profiles = lambda boxes, axis: [layout.box_ink(page, b, floor)[axis] for b in boxes]
        tight, allows, passes = layout.xy_cut(profiles, H, W, text_h, max_passes=64)
        assert passes < 64, seed                                                                    # it converged: the last two passes changed nothing
        _check_disjoint_inside(tight, H, W)
        # every pair that counts lies inside exactly one tight box — both of its pixels —, and every tight box's sides are tight
        y = bc.luma(page)
        d = np.abs(y[:, 1:] - y[:, :-1])
        ys, xs = np.nonzero((d >= floor) & (d > 0))
        owner = np.zeros((H, W), np.int32)
        for b in tight:
            owner[b[1]:b[3], b[0]:b[2]] += 1
        assert (owner <= 1).all() and (owner[ys, xs] == 1).all() and (owner[ys, xs + 1] == 1).all(), seed
        for b in tight:
            rows, cols = layout.box_ink(page, b, floor)
            c = layout.pixel_profile(cols)
            assert rows[0] and rows[-1] and c[0] and c[-1], (seed, b)
        # cutting its own result again changes nothing
        again = layout.xy_cut(profiles, H, W, text_h, max_passes=64, start=(tight, allows))
        assert again == (tight, allows, 2), seed
        # the grown boxes: disjoint, inside the page, around their tight boxes — whatever the pad
        for pad in (None, 10 ** 6):
            found = layout.find_lines_host(page, text_h=text_h, floor=floor, pad=pad, min_h=0, min_w=0, max_h=10 ** 6)
            assert found["tight"] == layout.xy_cut(profiles, H, W, text_h)[0], seed
            _check_disjoint_inside(found["boxes"], H, W)
            assert all(g[0] <= t[0] and g[1] <= t[1] and g[2] >= t[2] and g[3] >= t[3] for g, t in zip(found["boxes"], found["tight"]))


def test_the_front_end_off_the_device(scene):
    """with the networks on no HIP device ``find_lines`` runs the host definition; ``restore_page_auto`` reads, and says what it needs"""
    import torch
    from marconet_amd import restore

    class OnHost(restore.RestoreFrontEnd):
        def _device(self):
            return torch.device("cpu")
    pipe = OnHost()
    assert pipe.find_lines(scene["page"], text_h=ls.TEXT_H) == scene["found"]
    assert pipe.find_lines(scene["page"], text_h=ls.TEXT_H, pad=0, floor=30) == layout.find_lines_host(scene["page"], text_h=ls.TEXT_H, pad=0, floor=30)
    with pytest.raises(ValueError, match="find_lines: text_h must be"):
        pipe.find_lines(scene["page"], text_h=0)
    with pytest.raises(TypeError):
        pipe.find_lines(scene["page"][..., :2])
    with pytest.raises(ValueError, match="restore_page_auto: the lines it finds are read by the encoder, which needs the networks on a HIP device"):
        pipe.restore_page_auto(scene["page"])
    with pytest.raises(ValueError, match="restore_page_auto: scale must be"):
        pipe.restore_page_auto(scene["page"], scale=0)


def test_launch_chunks():
    assert layout.launch_chunks([], [], 32, 256) == []
    assert layout.launch_chunks([5] * 70000, [9] * 70000, 32, 256) == [(0, 65535), (65535, 70000)]
    assert layout.launch_chunks([3508, 40, 40], [2480, 600, 600], 32, 256) == [(0, 3)]
    big = layout.launch_chunks([32 * 4096] + [1] * 9000, [256 * 1024] + [1] * 9000, 32, 256)        # 2^22 tiles a box: 3 boxes a launch beside the big one
    assert big[0] == (0, 3) and big[1] == (3, 9001)


# ----------------------------------------------------------------------------------------------------------- mnet_box_ink_u8, host side
def test_boxink_header_declares_exactly_the_bound_symbol_and_the_descriptor_layout(tmp_path):
    text = open(os.path.join(INCLUDE, "marconet_hip_boxink.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(mnet_\w+)\s*\(", code)) == set(_lib.BOXINK_SYMBOLS) == {"mnet_box_ink_u8"}
    assert len(_lib.BOXINK_SYMBOLS["mnet_box_ink_u8"][1]) == 10
    cpath, exe = str(tmp_path / "probe.c"), str(tmp_path / "probe")
    fields = ("offset", "pitch", "h", "w", "out_rows", "out_cols", "reserved")
    with open(cpath, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "marconet_hip_boxink.h"\nint main(void) {\n'
                'printf("%d %d %d ' + "%d " * len(fields) + '\\n", (int)sizeof(mnet_ink_box2), (int)_Alignof(mnet_ink_box2), MNET_ABI_VERSION, '
                + ", ".join("(int)offsetof(mnet_ink_box2, %s)" % n for n in fields) + ');\nreturn 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", INCLUDE, cpath])
    subprocess.check_call(["gcc", "-std=c11", "-I", INCLUDE, cpath, "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    S = _lib.BoxInkBox
    assert ctypes.sizeof(S) == 32 and np.dtype(S).itemsize == 32 and ctypes.alignment(S) == 8
    assert got == [32, 8, 4, 0, 8, 12, 16, 20, 24, 28] == [ctypes.sizeof(S), ctypes.alignment(S), _lib.ABI_VERSION] + [getattr(S, n).offset for n in fields]
    assert [n for n, _ in S._fields_] == list(fields)
    lib = _lib.load()
    assert hasattr(lib, "mnet_box_ink_u8") and lib.mnet_abi_version() == 4 and len(_lib.SYMBOLS) == 45
    others = [getattr(_lib, name) for name in dir(_lib) if name.endswith("SYMBOLS") and name != "BOXINK_SYMBOLS"]
    assert len(others) >= 10 and not any(set(_lib.BOXINK_SYMBOLS) & set(t) for t in others)
    rowink = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "marconet_hip_rowink.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(mnet_\w+)\s*\(", rowink)) == {"mnet_row_ink_u8"}                     # the old header is as it was
    src = open(os.path.join(ROOT, "marconet_amd", "csrc", "ink_kernels.hip")).read()
    assert (_lib.BOXINK_TILE_W, _lib.BOXINK_TILE_H) == tuple(int(re.search(r"BOXINK_TILE_%s = (\d+)" % a, src).group(1)) for a in "WH")


def test_build_sh_lists_the_source_and_stamps_its_header():
    sh = open(os.path.join(ROOT, "marconet_amd", "csrc", "build.sh")).read()
    srcs = re.search(r'^SRCS="([^"]*)"', sh, flags=re.M).group(1).split()
    assert "ink_kernels" in srcs and len(srcs) == len(set(srcs))
    assert '[ "$1" = ink_kernels ] && cat "$HERE/ink.h" "$HERE/../../include/marconet_hip_rowink.h" "$HERE/../../include/marconet_hip_boxink.h" ' \
           '"$HERE/../../include/marconet_hip_skewink.h"' in sh
    from marconet_amd import ops
    assert "box_ink_u8" in ops.__all__ and "row_ink_u8" in ops.__all__


def test_load_binds_every_symbol_table_as_it_is_written():
    lib = _lib.load()
    tables = {name: getattr(_lib, name) for name in dir(_lib) if name.endswith("SYMBOLS")}
    declared = set()
    for header in os.listdir(INCLUDE):                                                              # one table per header, every declared function bound
        declared |= set(re.findall(r"\b(mnet_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)))
    assert len(tables) == len(os.listdir(INCLUDE)) and "SYMBOLS" in tables
    assert sorted(n for t in tables.values() for n in t) == sorted(declared)                        # no name twice, none missing
    for table in tables.values():
        for name, (res, args) in table.items():
            fn = getattr(lib, name)
            assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_boxink_entry_point_validates_arguments_without_device():
    lib = _lib.load()
    e_arg = lib.mnet_lq_from_u8(None, None, 0, 0, 0, None, 0, None)                                 # MNET_E_ARG
    ok = dict(src=64, src_bytes=1000, boxes=128, n=2, max_h=5, max_w=7, floor=24, dst=256, dst_len=10, stream=None)
    for change, status in ((dict(src=None), -1), (dict(boxes=None), -1), (dict(dst=None), -1), (dict(n=0), -1), (dict(n=-1), -1), (dict(max_h=0), -1),
                           (dict(max_w=0), -1), (dict(src_bytes=0), -1), (dict(dst_len=0), -1), (dict(n=65536), -1), (dict(floor=-1), -1),
                           (dict(floor=256), -1), (dict(max_h=2 ** 23), -1), (dict(max_w=2 ** 23), -1),
                           (dict(max_h=32 * 65535 + 1), -1),                                        # 65536 row tiles
                           (dict(n=65535, max_h=32 * 300, max_w=256 * 300), -1),                    # 2^32 threads and more
                           (dict(boxes=132), None), (dict(dst=258), None)):
        a = dict(ok, **change)
        got = lib.mnet_box_ink_u8(a["src"], a["src_bytes"], a["boxes"], a["n"], a["max_h"], a["max_w"], a["floor"], a["dst"], a["dst_len"], a["stream"])
        assert got < 0 and (got == e_arg) == (status is not None), change                           # an alignment: MNET_E_ALIGN, another negative
        assert b"box_ink_u8" in lib.mnet_last_error()


# ------------------------------------------------------------------------------------------------------------- examples/restore_scan.py
def _example(name):
    spec = importlib.util.spec_from_file_location(name.replace(".py", "_example"), os.path.join(ROOT, "examples", name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_restore_scan_arguments_and_its_regions_file(tmp_path, scene):
    scan, page_example = _example("restore_scan.py"), _example("restore_page.py")
    a = scan.parse_args(["-i", "page.png", "-o", "out.png"])
    assert (a.image, a.output, a.text_h, a.floor, a.regions_out, a.scale, a.feather) == ("page.png", "out.png", None, 24, None, 4, 8)
    a = scan.parse_args(["-i", "p.png", "-o", "o.png", "--text-h", "35", "--floor", "0", "--regions-out", "found.json", "--scale", "2"])
    assert (a.text_h, a.floor, a.regions_out, a.scale) == (35, 0, "found.json", 2)
    for bad in (["-i", "p.png"], ["-o", "o.png"], ["-i", "p", "-o", "o", "--floor", "256"], ["-i", "p", "-o", "o", "--floor", "-1"],
                ["-i", "p", "-o", "o", "--text-h", "0"], ["-i", "p", "-o", "o", "--text-h", "x"]):
        with pytest.raises(SystemExit):
            scan.parse_args(bad)
    path = str(tmp_path / "found.json")
    boxes = scene["found"]["boxes"]
    scan.write_regions(path, [np.asarray(b) for b in boxes])                                        # numpy integers too
    assert json.load(open(path, encoding="utf8")) == [dict(box=b) for b in boxes]
    got = page_example.load_regions(path)                                                           # what restore_page.py -r reads
    assert got == (boxes, [None] * len(boxes), None, None, None, None)
