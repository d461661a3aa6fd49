"""not-gpu: the host side of the page path (marconet_amd/pages.py, mnet_paste_u8) — csrc/page_blend.h compiled for the CPU against the Python
formulas, the properties of the host definition, its refusals, the C layout of the region descriptor, the entry point's argument checks (the
library loads without a GPU), the build script's lines and the gfx950 ISA of the kernel's tap code.  Integers only: every comparison is exact."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from marconet_amd import _lib, lq_io, pages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marconet_amd", "csrc")
BYTES = (0, 1, 127, 128, 254, 255)
FEATHERS = (1, 2, 3, 7, 1024)


def _cxx():
    for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    raise RuntimeError("no C++ compiler found")


# ---------------------------------------------------------------------------------------------------------------------- page_blend.h
_BLEND_MAIN = r'''
#include <stdio.h>
#include "page_blend.h"
/* stdin: commands, see below -> stdout: result bytes */
static const unsigned v[6] = {0, 1, 127, 128, 254, 255};
int main(void) {
    unsigned F, n;
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'f') {                 /* f F: every (a, b), a and b in [1, 2F], at the 6 x 6 bytes: one result byte each */
            if (scanf("%u", &F) != 1) return 2;
            for (unsigned a = 1; a <= 2 * F; ++a)
                for (unsigned b = 1; b <= 2 * F; ++b)
                    for (int i = 0; i < 6; ++i)
                        for (int j = 0; j < 6; ++j) {
                            const uint32_t r = page_feather(v[i], v[j], a, b, F);
                            if (r > 255u) return 3;
                            fputc((int)r, stdout);
                        }
        } else if (what == 'x') {          /* x n F: page_feather_axis of every coordinate of an axis of n pixels, as 16-bit little endian */
            if (scanf("%u %u", &n, &F) != 2) return 2;
            for (unsigned u = 0; u < n; ++u) {
                const uint32_t a = page_feather_axis(u, n, F);
                fputc((int)(a & 255u), stdout);
                fputc((int)(a >> 8), stdout);
            }
        } else if (what == 'b') {          /* b: the box average of every cnt in [1, 64] at the sums 0, 1, cnt 255 - 1, cnt 255, and every multiple of cnt / 2 around a half */
            for (unsigned cnt = 1; cnt <= 64; ++cnt) {
                const unsigned sums[8] = {0, 1, cnt * 255 - 1, cnt * 255, cnt / 2, (cnt + 1) / 2, cnt * 127 + cnt / 2, cnt * 127 + (cnt + 1) / 2};
                for (int i = 0; i < 8; ++i) {
                    const uint32_t r = page_box_avg(sums[i], cnt);
                    if (r > 255u) return 3;
                    fputc((int)r, stdout);
                }
            }
        } else return 4;
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def blend_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("page_blend")
    src, exe = str(d / "page_blend_main.cpp"), str(d / "page_blend_main")
    with open(src, "w") as f:
        f.write(_BLEND_MAIN)
    subprocess.check_call([_cxx(), "-O2", "-ffp-contract=off", "-I", CSRC, src, "-o", exe])
    return exe


def _run(exe, text):
    return np.frombuffer(subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout, dtype=np.uint8)


def test_feather_header_matches_the_python_formula(blend_exe):
    bg, fg = np.meshgrid(np.int64(BYTES), np.int64(BYTES), indexing="ij")
    for F in FEATHERS:
        if F == 1024:
            continue
        raw = _run(blend_exe, "f %d" % F)
        n = 2 * F
        assert raw.size == n * n * 36
        got = raw.reshape(n, n, 6, 6).astype(np.int64)
        a = np.arange(1, n + 1, dtype=np.int64)
        m = (a[:, None] * a[None, :])[:, :, None, None]
        D = 4 * F * F
        want = (bg * (D - m) + fg * m + D // 2) // D
        assert np.array_equal(got, want), F
        assert (got >= np.minimum(bg, fg)).all() and (got <= np.maximum(bg, fg)).all(), F
        assert np.array_equal(got[n - 1, n - 1], fg)                                          # weight 1 from F pixels inside: the line's byte
        assert np.array_equal(got, got.transpose(1, 0, 2, 3)), F                              # symmetric in the two axes


def test_feather_header_at_the_largest_feather(blend_exe):
    """F = 1024: every (a, b) in [1, 2048]², 36 byte pairs each, against the Python formula, and the 32-bit bound of the header's arithmetic"""
    F, n, D = 1024, 2048, 4 * 1024 * 1024
    raw = _run(blend_exe, "f %d" % F)
    assert raw.size == n * n * 36
    got = raw.reshape(n, n, 36)
    bg, fg = (v.reshape(-1) for v in np.meshgrid(np.int64(BYTES), np.int64(BYTES), indexing="ij"))
    a = np.arange(1, n + 1, dtype=np.int64)
    for lo in range(0, n, 256):                                                               # by slabs of a: bounded memory
        m = (a[lo:lo + 256, None] * a[None, :])[:, :, None]
        want = (bg * (D - m) + fg * m + D // 2) // D
        assert np.array_equal(got[lo:lo + 256], want.astype(np.uint8)), lo
    assert 255 * D + D // 2 < 1 << 31 and D == 1 << 22                                        # the header's 32-bit range, at its largest numerator
    assert pages.MAX_FEATHER == F
    one = np.full((1, 1, 3), 255, np.uint8)
    assert np.array_equal(pages.feather_blend(one, one, F), one)


def test_feather_axis_header_matches_python(blend_exe):
    for n, F in ((1, 1), (2, 1), (7, 3), (8, 3), (9, 100), (64, 7), (65, 1024), (5000, 1024)):
        raw = _run(blend_exe, "x %d %d" % (n, F))
        got = raw[0::2].astype(np.int64) + 256 * raw[1::2].astype(np.int64)
        want = pages.feather_axis(n, F)
        assert np.array_equal(got, want), (n, F)
        assert np.array_equal(want, want[::-1]) and want.min() == 1 and want.max() <= 2 * F
        if n >= 2 * F:
            assert (want[F:n - F] == 2 * F).all() and want[F - 1] == 2 * F - 1               # exactly 1 from F pixels inside


def test_box_average_header_matches_python(blend_exe):
    raw = _run(blend_exe, "b")
    assert raw.size == 64 * 8
    got = raw.reshape(64, 8).astype(np.int64)
    for cnt in range(1, 65):
        sums = np.int64([0, 1, cnt * 255 - 1, cnt * 255, cnt // 2, (cnt + 1) // 2, cnt * 127 + cnt // 2, cnt * 127 + (cnt + 1) // 2])
        assert np.array_equal(got[cnt - 1], (2 * sums + cnt) // (2 * cnt)), cnt
        assert got[cnt - 1, 3] == 255 and got[cnt - 1, 0] == 0
    # box_reduce is that formula: k = 4 on a 9-column line → blocks of 16, 16 and 4 bytes
    rng = np.random.default_rng(1)
    line = rng.integers(0, 256, (8, 9, 3), dtype=np.uint8)
    red = pages.box_reduce(line, 4)
    assert red.shape == (2, 3, 3) and red.dtype == np.uint8
    for r in range(2):
        for c, (x0, x1) in enumerate(((0, 4), (4, 8), (8, 9))):
            s = line[4 * r:4 * r + 4, x0:x1].astype(np.int64).sum(axis=(0, 1))
            cnt = 4 * (x1 - x0)
            assert np.array_equal(red[r, c], (2 * s + cnt) // (2 * cnt))
    assert np.array_equal(pages.box_reduce(line, 1), line)
    with pytest.raises(ValueError):
        pages.box_reduce(line, 3)
    with pytest.raises(ValueError):
        pages.box_reduce(line[:6], 4)


# ------------------------------------------------------------------------------------------------------------------- the definition
def test_box_factor():
    assert [pages.box_factor(rh, 128) for rh in (200, 128, 64, 32, 16)] == [1, 1, 2, 4, 8]
    assert [pages.box_factor(rh, 128) for rh in (129, 127, 65, 63, 33, 31, 17, 15, 8, 1)] == [1, 1, 1, 2, 2, 4, 4, 8, 8, 8]
    assert [pages.box_factor(rh, 16) for rh in (40, 16, 8, 4, 2)] == [1, 1, 2, 4, 8]
    for rh in range(8, 300):                                                                 # after the reduction the cubic never shrinks by more than 2
        k = pages.box_factor(rh, 128)
        assert k * rh <= 128 or k == 1
        assert 128 // k <= 2 * rh and (k == 8 or 2 * k * rh > 128)


def test_resize_cubic_to_is_resize_cubic_where_the_sizes_give_its_factor():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (12, 20, 3), dtype=np.uint8)
    for f in (1, 2, 3, 4, 0.5, 0.25, 1.5):
        dw, dh = int(np.rint(20 * f)), int(np.rint(12 * f))
        assert dw / 20 == f and dh / 12 == f
        assert np.array_equal(pages.resize_cubic_to(img, dw, dh), lq_io.resize_cubic(img, f, f)), f
    assert np.array_equal(pages.resize_cubic_to(img, 20, 12), img)
    out = pages.resize_cubic_to(img, 37, 5)                                                  # the sizes themselves: no factor behind them
    assert out.shape == (5, 37, 3) and out.dtype == np.uint8
    xi, xt = lq_io._cubic_taps(37, 20, 37 / 20)
    yi, yt = lq_io._cubic_taps(5, 12, 5 / 12)
    y, x = 3, 30
    v = sum(int(yt[y, j]) * sum(int(xt[x, i]) * int(img[yi[y, j], xi[x, i], 1]) for i in range(4)) for j in range(4))
    assert out[y, x, 1] == min(max((v + (1 << 21)) >> 22, 0), 255)
    assert pages.axis_scale(37, 20) == 1.0 / (37 / 20)
    with pytest.raises(ValueError):
        pages.resize_cubic_to(img, 0, 5)


def test_paste_host_properties():
    rng = np.random.default_rng(3)
    line = rng.integers(0, 256, (128, 300, 3), dtype=np.uint8)
    page = rng.integers(0, 256, (260, 500, 3), dtype=np.uint8)
    # a rectangle of the line's own size with F = 0 is the line flipped to RGB; nothing outside the rectangle changes
    out = pages.paste_host(page.copy(), line, (50, 100, 300, 128), 0)
    assert np.array_equal(out[100:228, 50:350], line[:, :, ::-1])
    mask = np.ones(page.shape[:2], bool)
    mask[100:228, 50:350] = False
    assert np.array_equal(out[mask], page[mask])
    # any k, any F: outside the rectangle nothing changes; a constant line on a constant page of the same value stays constant
    for rh, k in ((200, 1), (128, 1), (64, 2), (32, 4), (16, 8), (9, 8)):
        rw = max(1, (300 * rh) // 128 + 3)
        for F in (0, 1, 5, 8, 1024):
            rect = (7, 11, rw, rh)
            out = pages.paste_host(page.copy(), line, rect, F)
            mask = np.ones(page.shape[:2], bool)
            mask[11:11 + rh, 7:7 + rw] = False
            assert np.array_equal(out[mask], page[mask]), (rh, F)
            assert F > 8 or (out[~mask].reshape(rh, rw, 3) != page[11:11 + rh, 7:7 + rw]).any()      # (a small rectangle under F = 1024 keeps the background)
            for value in (0, 77, 255):
                flat = pages.paste_host(np.full_like(page, value), np.full_like(line, value), rect, F)
                assert (flat == value).all(), (rh, F, value)
        assert pages.box_factor(rh) == k
    # the feather: the line's byte from F pixels inside, a mix at the edge that stays between the two
    bg, fg = np.zeros((40, 60, 3), np.uint8), np.full((128, 192, 3), 200, np.uint8)
    out = pages.paste_host(bg, fg, (0, 0, 60, 40), 4)
    assert (out[4:36, 4:56] == 200).all() and out[0, 0, 0] == (200 * 1 + 32) // 64 and out[0, 30, 0] == (200 * 8 + 32) // 64
    assert np.array_equal(out, out[::-1]) and np.array_equal(out, out[:, ::-1])
    with pytest.raises(ValueError):
        pages.paste_host(page.copy(), line, (450, 100, 51, 128), 0)


def test_compose_host_and_its_refusals():
    rng = np.random.default_rng(4)
    page = rng.integers(0, 256, (40, 90, 3), dtype=np.uint8)
    lines = [rng.integers(0, 256, (128, 333, 3), dtype=np.uint8), None, rng.integers(0, 256, (128, 64, 3), dtype=np.uint8)]
    boxes = [[2, 3, 60, 20], [0, 0, 90, 40], [70, 25, 90, 40]]                              # region 1 has no line: it may cover the others
    out = pages.compose_host(page, lines, boxes, 2, 3)
    want = lq_io.resize_cubic(page, 2, 2)
    assert out.shape == (80, 180, 3) and np.array_equal(lq_io.resize_cubic(page, 1, 1), page)
    pages.paste_host(want, lines[0], (4, 6, 116, 34), 3)
    pages.paste_host(want, lines[2], (140, 50, 40, 30), 3)
    assert np.array_equal(out, want)
    assert np.array_equal(pages.compose_host(page, [None] * 3, boxes, 2, 3), lq_io.resize_cubic(page, 2, 2))
    assert np.array_equal(pages.compose_host(page, [], [], 1, 0), page)

    def refused(match, lines=lines, boxes=boxes, scale=2, feather=3):
        with pytest.raises(ValueError, match=match):
            pages.compose_host(page, lines, boxes, scale, feather)

    refused("regions 0 and 2 overlap", boxes=[boxes[0], boxes[1], [59, 19, 90, 40]])
    pages.compose_host(page, lines, [boxes[0], boxes[1], [60, 19, 90, 40]], 2, 3)            # touching rectangles do not overlap
    refused("region 2: .*outside", boxes=[boxes[0], boxes[1], [70, 25, 91, 40]])
    refused("region 0: .*outside", boxes=[[-1, 3, 60, 20], boxes[1], boxes[2]])
    refused("region 1: .*outside", boxes=[boxes[0], [0, 0, 90, 41], boxes[2]])                # the box of a region without a line is checked too
    refused("region 0: .*empty", boxes=[[5, 3, 5, 20], boxes[1], boxes[2]])
    refused("region 0: .*integer", boxes=[[2.5, 3, 60, 20], boxes[1], boxes[2]])
    refused("region 2: .*6 rows", boxes=[boxes[0], boxes[1], [70, 25, 90, 28]])              # 3 page rows x 2
    pages.compose_host(page, lines, [boxes[0], boxes[1], [70, 25, 90, 29]], 2, 3)            # 8 rows: accepted
    for scale in (0, 9, 1.5, -1):
        refused("scale", scale=scale)
    for feather in (-1, 1025, 0.5):
        refused("feather", feather=feather)
    refused("one line", lines=lines[:2])
    assert pages.round_box([2.5, 3.0, 59.2, 19.9], 40, 90) == [2, 3, 60, 20] and pages.round_box([-4, -1, 95.5, 40.01], 40, 90) == [0, 0, 90, 40]


def test_build_table_rows():
    rects = [(4, 6, 116, 34), (0, 0, 180, 80), (140, 50, 40, 16)]
    tab = pages.build_table(rects, [333, None, 65], 3)
    assert tab.dtype.itemsize == ctypes.sizeof(_lib.PasteRegion) == 48 and len(tab) == 2
    assert tuple(tab[0])[:8] == (0, 333, 4, 6, 116, 34, 3, 2) and tuple(tab[1])[:8] == (1, 65, 140, 50, 40, 16, 3, 8)
    assert tab["scale_x"].tolist() == [1.0 / (116 / 167), 1.0 / (40 / 9)] and tab["scale_y"].tolist() == [1.0 / (34 / 64), 1.0 / (16 / 16)]


# ------------------------------------------------------------------------------------------------------------------------- the C-ABI
FIELDS = ("line_index", "src_w", "x0", "y0", "rw", "rh", "feather", "k", "scale_x", "scale_y")


def test_paste_region_layout_matches_c(tmp_path):
    """sizeof / offsetof of mnet_paste_region from a C program compiled against the header == the ctypes mirror"""
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "marconet_hip.h"\nint main(void){ printf("%zu %zu", sizeof(mnet_paste_region), '
            '_Alignof(mnet_paste_region));\n' + "".join('printf(" %%zu", offsetof(mnet_paste_region, %s));\n' % f for f in FIELDS) + "return 0; }\n")
    cpath, exe = str(tmp_path / "paste_probe.c"), str(tmp_path / "paste_probe")
    with open(cpath, "w") as f:
        f.write(code)
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), cpath, "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    R = _lib.PasteRegion
    assert got == [ctypes.sizeof(R), ctypes.alignment(R)] + [getattr(R, f).offset for f in FIELDS]
    assert got == [48, 8, 0, 4, 8, 12, 16, 20, 24, 28, 32, 40] and np.dtype(R).itemsize == 48
    assert "mnet_paste_u8" in _lib.SYMBOLS and len(_lib.SYMBOLS) == 43 + 2                  # 43 entry points, mnet_last_error and mnet_abi_version


def test_paste_u8_argument_validation_without_device():
    lib = _lib.load()
    ok = dict(lines=16, n_lines=3, rows=128, line_w=2048, regions=16, n_regions=2, page=16, page_h=400, page_w=600)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mnet_paste_u8(a["lines"], a["n_lines"], a["rows"], a["line_w"], a["regions"], a["n_regions"], a["page"], a["page_h"], a["page_w"], None)

    for bad in ("lines", "regions", "page"):
        assert call(**{bad: None}) == -1 and b"null" in lib.mnet_last_error()
    for bad in (dict(n_lines=0), dict(n_lines=-2), dict(rows=0), dict(line_w=0), dict(line_w=-5), dict(n_regions=0), dict(n_regions=-1), dict(page_h=0),
                dict(page_w=0), dict(page_w=-7)):
        assert call(**bad) == -1 and b"bad shape" in lib.mnet_last_error()
    assert call(n_regions=1 << 20, page_h=1 << 15, page_w=1 << 15) == -1 and b"too large" in lib.mnet_last_error()
    for bad in (dict(regions=20), dict(regions=17), dict(regions=2)):
        assert call(**bad) == -2 and b"aligned" in lib.mnet_last_error()


def test_ops_and_driver_refuse_cpu_tensors_and_bad_tables():
    from marconet_amd import ops
    lines = torch.zeros((2, 128, 300, 3), dtype=torch.uint8)
    page = torch.zeros((80, 180, 3), dtype=torch.uint8)
    tab = torch.zeros((1, 48), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.paste_u8(lines, tab, page)
    with pytest.raises(ValueError, match="one joined line per region"):
        pages.compose_page(page, lines, [300], [[0, 0, 90, 40]], 2, 3)
    with pytest.raises(ValueError, match="regions 0 and 1 overlap"):                          # found before any copy or launch
        pages.compose_page(page.numpy(), lines, [300, 200], [[0, 0, 90, 40], [80, 30, 100, 50]], 1, 3)
    with pytest.raises(ValueError, match="line width 301"):
        pages.compose_page(page.numpy(), lines, [301, 200], [[0, 0, 90, 40], [90, 40, 100, 50]], 1, 3)
    with pytest.raises(TypeError):
        pages.compose_page(page.numpy().astype(np.float32), lines, [300, 200], [[0, 0, 90, 40], [90, 40, 100, 50]], 1, 3)


def test_restore_page_refuses_before_anything_runs():
    """the entry point's host checks need neither weights on a device nor a launch"""
    from marconet_amd import networks
    from marconet_amd.pipeline import MarconetPipeline
    pipe = MarconetPipeline(networks.TextContextEncoderV2(), networks.TSPGAN(), networks.TSPSRNet())
    assert hasattr(pipe, "restore_page")
    page = np.zeros((60, 200, 3), np.uint8)
    a = lq_io.alphabet()[10]
    with pytest.raises(ValueError, match="needs texts"):
        pipe.restore_page(page, [[0, 0, 100, 30]], None)
    with pytest.raises(ValueError, match="one text"):
        pipe.restore_page(page, [[0, 0, 100, 30]], [a, a])
    with pytest.raises(ValueError, match="restore_page: regions 0 and 1 overlap"):
        pipe.restore_page(page, [[0, 0, 100, 30], [99, 29, 150, 50]], [a, a])
    with pytest.raises(ValueError, match="restore_page: region 1: .*empty or lies outside"):
        pipe.restore_page(page, [[0, 0, 100, 30], [300, 10, 350, 50]], [a, a])
    with pytest.raises(ValueError, match="restore_page: region 0: .*4 rows"):
        pipe.restore_page(page, [[0, 0, 100, 4]], [a], scale=1)
    with pytest.raises(ValueError, match="scale"):
        pipe.restore_page(page, [[0, 0, 100, 30]], [a], scale=9)
    with pytest.raises(ValueError, match="feather"):
        pipe.restore_page(page, [[0, 0, 100, 30]], [a], feather=2000)
    with pytest.raises(TypeError):
        pipe.restore_page(page.astype(np.float32), [[0, 0, 100, 30]], [a])


# ----------------------------------------------------------------------------------------------------------------------- the build
def test_build_script_compiles_and_stamps_the_kernel():
    sh = open(os.path.join(CSRC, "build.sh")).read()
    assert re.search(r'^SRCS="[^"]*\bpage_kernels\b[^"]*"', sh, flags=re.M)
    assert 'panel_kernels) echo "-ffp-contract=off" ;; page_kernels) echo "-ffp-contract=off" ;;' in sh
    assert '[ "$1" = page_kernels ] && cat "$HERE/lq_taps.h" "$HERE/page_blend.h" "$HERE/page_tile.h" "$HERE/../../include/marconet_hip_columns.h"' in sh
    assert '[ "$1" = lq_kernels ] && cat "$HERE/lq_taps.h" "$HERE/page_tile.h"' in sh
    src = open(os.path.join(CSRC, "page_kernels.hip")).read()
    assert '#include "page_tile.h"' in src and '#include "page_blend.h"' in src and "marconet_hip_columns.h" in src and "pt_stage_taps(" in src
    # the taps are staged once, in the shared header, for this unit, lq_kernels and column_kernels
    tile = open(os.path.join(CSRC, "page_tile.h")).read()
    assert '#include "lq_taps.h"' in tile and tile.count("lq_cubic_taps(") == 2
    assert '#include "page_tile.h"' in open(os.path.join(CSRC, "lq_kernels.hip")).read()


def test_device_build_of_the_page_kernel_is_not_contracted(tmp_path):
    """the gfx950 ISA of page_kernels.hip under build.sh's own flags holds no floating-point fused multiply-add at all (the kernel has no divide
    to expand: its divisions are integer); integer v_mad_u* / v_mad_i* do not count.  The tap arithmetic is there, unfused, in fp32 and fp64."""
    sh = open(os.path.join(CSRC, "build.sh")).read()
    flags = re.search(r'^FLAGS="([^"]*)"', sh, flags=re.M).group(1).split()
    extra = re.search(r'page_kernels\) echo "([^"]*)"', sh).group(1).split()
    assert "-ffp-contract=off" in extra
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    asm = str(tmp_path / "page_kernels.s")
    subprocess.check_call([hipcc] + flags + extra + ["-S", "--cuda-device-only", os.path.join(CSRC, "page_kernels.hip"), "-o", asm], stderr=subprocess.DEVNULL)
    ops_ = re.findall(r"^\s+(v_[a-z0-9_]+)", open(asm).read(), flags=re.M)
    assert any(o.startswith("v_mul_f32") for o in ops_) and any(o.startswith("v_mul_f64") for o in ops_)
    fused = [o for o in ops_ if re.match(r"v_(pk_)?(fma|fmac|fmaak|fmamk|mad|mac)_", o) and not o.startswith("v_mad_u") and not o.startswith("v_mad_i")]
    assert fused == [], sorted(set(fused))
