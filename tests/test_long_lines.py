"""not-gpu: the host side of the long-line path (marconet_amd/long_lines.py, mnet_stitch_u8) — the window plan's guarantees on random lines, the
blend of csrc/stitch_blend.h compiled for the CPU against the Python formula, stitch_host on the plans it must leave alone, the C layout of the two
descriptors and the entry point's argument checks (the library loads without a GPU)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from marconet_amd import _lib, long_lines, lq_device, lq_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marconet_amd", "csrc")
HEIGHTS = (17, 32, 48, 100)


def _random_line(rng, h, n):
    """n character boxes left to right: widths 0.3 h .. 1.5 h, gaps 0 .. 0.4 h, margins 0 .. h → (w, boxes)"""
    x, boxes = int(rng.integers(0, h + 1)), []
    for _ in range(n):
        cw = int(rng.integers(max(1, (3 * h) // 10), (3 * h) // 2 + 1))
        boxes.append([x, 0, x + cw, h])
        x += cw + int(rng.integers(0, (2 * h) // 5 + 1))
    return x + int(rng.integers(0, h + 1)), boxes


def _check_plan(plan, h, w, boxes, max_glyphs=16):
    n = len(boxes)
    assert plan[0].c0 == 0 and plan[0].g0 == 0 and plan[0].offset == 0 and plan[-1].c1 == w and plan[-1].g1 == n
    whole = np.zeros(n, bool)
    for p in plan:
        assert 0 <= p.c0 < p.c1 <= w and 0 <= p.g0 < p.g1 <= n and p.g1 - p.g0 <= max_glyphs
        g = lq_device.strip_geometry(np.zeros((h, p.c1 - p.c0, 3), np.uint8))                # accepted: no StripTooWide
        assert g.dw <= lq_io.LQ_W and p.show_w == g.show_w and p.offset == (256 * p.c0 + h) // (2 * h)
        for c in range(p.g0, p.g1):
            whole[c] |= p.c0 <= boxes[c][0] and boxes[c][2] <= p.c1
    assert whole.all()                                                                       # every character whole in at least one window
    out_w = long_lines.plan_out_w(plan)
    cover = np.zeros(out_w, np.int64)
    for p in plan:
        cover[p.offset:p.offset + p.show_w] += 1
    assert cover.min() >= 1 and cover.max() <= 2                                             # every output column once or twice
    for a, b in zip(plan, plan[1:]):
        assert a.g0 < b.g0 and a.offset < b.offset < a.offset + a.show_w                      # advances; consecutive windows overlap
    assert abs(out_w - lq_device._axis(h, w, lq_device.SHOW_H)[0]) <= 1                        # the whole line's own show_w
    return out_w


def test_plan_properties_on_random_lines():
    rng = np.random.default_rng(20240901)
    multi = single = 0
    for case in range(200):
        h = HEIGHTS[case % 4]
        n = (1, 80, 2, 17)[case // 4] if case < 16 else int(rng.integers(1, 81))
        w, boxes = _random_line(rng, h, n)
        plan = long_lines.plan_windows(h, w, boxes)
        _check_plan(plan, h, w, boxes)
        multi += len(plan) >= 3
        single += len(plan) == 1
    assert multi >= 50 and single >= 5


def test_plan_at_the_width_limit():
    """512 px at height 32 with 16 characters is one window — restore_images' own strip; one pixel more makes two"""
    for h, w_fit in ((32, 512), (17, 272), (48, 768), (100, 1600)):
        assert not long_lines.too_wide(h, w_fit)
        w_over = w_fit + 1
        while not long_lines.too_wide(h, w_over):                                           # the first width the reference refuses
            w_over += 1
        w_fit = w_over - 1
        bx = lq_io.evenly_spaced_boxes(16, w_fit, h)
        plan = long_lines.plan_windows(h, w_fit, bx)
        assert plan == [long_lines.Window(0, w_fit, 0, 16, 0, lq_device.strip_geometry(np.zeros((h, w_fit, 3), np.uint8)).show_w)]
        bx = lq_io.evenly_spaced_boxes(16, w_over, h)
        with pytest.raises(lq_io.StripTooWide):
            lq_device.strip_geometry(np.zeros((h, w_over, 3), np.uint8))
        plan = long_lines.plan_windows(h, w_over, bx)
        assert len(plan) == 2 and plan[0].g1 == 15 and plan[1].g0 == 13
        _check_plan(plan, h, w_over, bx)
    # a narrow line with more characters than a window takes is cut by the character limit alone
    bx = lq_io.evenly_spaced_boxes(20, 400, 32)
    plan = long_lines.plan_windows(32, 400, bx, max_glyphs=8, overlap_glyphs=1)
    assert [(p.g0, p.g1) for p in plan] == [(0, 8), (7, 15), (14, 20)]
    _check_plan(plan, 32, 400, bx, max_glyphs=8)


def test_plan_refuses_what_it_cannot_guarantee():
    h = 32
    wide = [[0, 0, 40, h], [40, 0, 640, h], [640, 0, 680, h]]                                # character 1 is 600 px wide at height 32
    with pytest.raises(ValueError, match="character 1 does not fit a window"):
        long_lines.plan_windows(h, 680, wide)
    two_wide = [[300 * k, 0, 300 * k + 300, h] for k in range(4)]                            # one character per window: an overlap of 2 cannot advance
    with pytest.raises(ValueError, match="character 0 .*cannot advance"):
        long_lines.plan_windows(h, 1200, two_wide)
    with pytest.raises(ValueError, match="no shared column|cannot be joined"):                # windows that only touch have nothing to cross-fade over
        long_lines.plan_windows(h, 1200, two_wide, overlap_glyphs=0)
    with pytest.raises(ValueError):
        long_lines.plan_windows(h, 100, [])
    with pytest.raises(ValueError):
        long_lines.plan_windows(h, 100, [[0, 0, 100, h]], max_glyphs=2, overlap_glyphs=2)


def test_the_golden_line_of_the_gpu_test_has_three_windows():
    from tests.long_lines_cases import golden_line
    img, text = golden_line()
    plan = long_lines.plan_windows(img.shape[0], img.shape[1], lq_io.evenly_spaced_boxes(len(text), img.shape[1], img.shape[0]))
    assert len(plan) >= 3 and len(text) == 40 and min(lq_io.labels_from_text(text)) >= 0


# ------------------------------------------------------------------------------------------------------------------------ the blend
_BLEND_MAIN = r'''
#include <stdio.h>
#include "stitch_blend.h"
/* stdin: D values -> stdout: for every t in [0, D) and every (a, b) of the 6 x 6 bytes below, one result byte */
int main(void) {
    static const unsigned v[6] = {0, 1, 127, 128, 254, 255};
    unsigned D;
    while (scanf("%u", &D) == 1)
        for (unsigned t = 0; t < D; ++t)
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j < 6; ++j) {
                    const uint32_t r = stitch_blend(v[i], v[j], t, D);
                    if (r > 255u) return 3;
                    fputc((int)r, stdout);
                }
    return 0;
}
'''
BYTES = (0, 1, 127, 128, 254, 255)
BLEND_D = tuple(range(1, 65)) + (127, 2047)


def _cxx():
    for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    raise RuntimeError("no C++ compiler found")


def test_blend_header_matches_the_python_formula(tmp_path):
    src, exe = str(tmp_path / "blend_main.cpp"), str(tmp_path / "blend_main")
    with open(src, "w") as f:
        f.write(_BLEND_MAIN)
    subprocess.check_call([_cxx(), "-O2", "-I", CSRC, src, "-o", exe])
    raw = np.frombuffer(subprocess.run([exe], input=" ".join(str(d) for d in BLEND_D).encode(), stdout=subprocess.PIPE, check=True).stdout, dtype=np.uint8)
    assert raw.size == 36 * sum(BLEND_D)
    a, b = np.meshgrid(np.int64(BYTES), np.int64(BYTES), indexing="ij")
    o = 0
    for D in BLEND_D:
        got = raw[o:o + 36 * D].reshape(D, 6, 6).astype(np.int64)
        o += 36 * D
        t = np.arange(D, dtype=np.int64)[:, None, None]
        want = (a * (2 * D - 2 * t - 1) + b * (2 * t + 1) + D) // (2 * D)
        assert np.array_equal(got, want), D
        assert np.array_equal(long_lines.blend(a, b, t, D), want)
        assert (got >= np.minimum(a, b)).all() and (got <= np.maximum(a, b)).all(), D
        assert np.array_equal(got, got[::-1].transpose(0, 2, 1)), D                          # (a, b, t) -> (b, a, D - 1 - t): the same byte
    assert int(long_lines.blend(255, 255, 0, 1 << 22)) == 255 and 511 * (1 << 22) < 1 << 32    # the header's 32-bit range


# ---------------------------------------------------------------------------------------------------------------------- stitch_host
def test_stitch_host_is_the_identity_on_one_window():
    rng = np.random.default_rng(5)
    for h, w in ((32, 300), (17, 40), (100, 1600)):
        plan = long_lines.plan_windows(h, w, lq_io.evenly_spaced_boxes(5, w, h))
        assert len(plan) == 1
        win = rng.integers(0, 256, (7, plan[0].show_w, 3), dtype=np.uint8)
        out = long_lines.stitch_host([win], plan)
        assert out.dtype == np.uint8 and np.array_equal(out, win)


def test_stitch_host_on_two_windows():
    """outside the overlap the windows' own bytes; inside, the ramp — equal windows stay as they are, 0 → 255 rises monotonically and symmetrically"""
    W = long_lines.Window
    plan = [W(0, 10, 0, 3, 0, 40), W(8, 20, 2, 5, 32, 50)]                                   # overlap [32, 40): D = 8
    a, b = np.zeros((2, 40, 3), np.uint8), np.full((2, 50, 3), 255, np.uint8)
    out = long_lines.stitch_host([a, b], plan)
    assert out.shape == (2, 82, 3) and not out[:, :32].any() and (out[:, 40:] == 255).all()
    ramp = out[0, 32:40, 0].astype(int)
    assert ramp.tolist() == [(255 * (2 * t + 1) + 8) // 16 for t in range(8)] and (np.diff(ramp) > 0).all()
    assert np.array_equal(ramp + ramp[::-1], np.full(8, 255))
    same = np.random.default_rng(1).integers(0, 256, (2, 82, 3), dtype=np.uint8)
    assert np.array_equal(long_lines.stitch_host([same[:, :40], same[:, 32:]], plan), same)
    with pytest.raises(ValueError):
        long_lines.stitch_host([a], plan)
    with pytest.raises(ValueError):
        long_lines.stitch_host([a, b[:, :49]], plan)
    with pytest.raises(ValueError):                                                          # a gap between the windows
        long_lines.stitch_host([a, b], [plan[0], W(8, 20, 2, 5, 41, 50)])


def test_cover_fault_names_the_window():
    f = long_lines.cover_fault
    assert f([0, 30, 60], [40, 40, 40], 100) is None and f([0], [1], 1) is None
    assert f([0, 40], [40, 40], 80) is None                                                  # touching windows cover every column once
    assert f([1], [40], 41) == 0 and f([0, 41], [40, 40], 81) == 1                           # column 0 / column 40 in no window
    assert f([0, 10, 20], [40, 40, 40], 60) == 2                                             # column 20 in three
    assert f([0, 30, 30], [40, 40, 40], 70) == 2 and f([0, 30, 20], [40, 40, 40], 70) == 2   # offsets not strictly increasing
    assert f([0, 30], [40, 0], 40) == 1 and f([-1, 30], [40, 40], 70) == 0
    assert f([0, 30], [40, 40], 71) == 2                                                     # the last column in no window


def test_build_tables_rows():
    W = long_lines.Window
    plans = [[W(0, 10, 0, 3, 0, 40), W(8, 20, 2, 5, 32, 50)], [W(0, 9, 0, 2, 0, 65)]]
    lines, wins = long_lines.build_tables(plans)
    assert lines.dtype.itemsize == ctypes.sizeof(_lib.StitchLine) == 16 and wins.dtype.itemsize == ctypes.sizeof(_lib.StitchWindow) == 16
    assert [tuple(int(v) for v in r) for r in lines.tolist()] == [(82, 0, 2, 0), (65, 2, 1, 0)]
    assert [tuple(int(v) for v in r) for r in wins.tolist()] == [(0, 0, 40, 0), (1, 32, 50, 0), (2, 0, 65, 0)]
    _, wins = long_lines.build_tables(plans, sr_index=[5, 3, 4])
    assert wins["sr_index"].tolist() == [5, 3, 4]


# ------------------------------------------------------------------------------------------------------------------------- the C-ABI
def test_stitch_descriptor_layout_matches_c(tmp_path):
    """sizeof / offsetof of mnet_stitch_line and mnet_stitch_window from a C program compiled against the header == the ctypes mirrors"""
    code = r'''
#include <stdio.h>
#include <stddef.h>
#include "marconet_hip.h"
int main(void){ printf("%zu %zu %zu %zu %zu  %zu %zu %zu %zu %zu\n", sizeof(mnet_stitch_line), offsetof(mnet_stitch_line, out_w), offsetof(mnet_stitch_line, win0),
  offsetof(mnet_stitch_line, n_win), offsetof(mnet_stitch_line, reserved), sizeof(mnet_stitch_window), offsetof(mnet_stitch_window, sr_index),
  offsetof(mnet_stitch_window, offset), offsetof(mnet_stitch_window, show_w), offsetof(mnet_stitch_window, reserved)); return 0; }
'''
    cpath, exe = str(tmp_path / "stitch_probe.c"), str(tmp_path / "stitch_probe")
    with open(cpath, "w") as f:
        f.write(code)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), cpath, "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    L, W = _lib.StitchLine, _lib.StitchWindow
    assert got == [ctypes.sizeof(L), L.out_w.offset, L.win0.offset, L.n_win.offset, L.reserved.offset,
                   ctypes.sizeof(W), W.sr_index.offset, W.offset.offset, W.show_w.offset, W.reserved.offset]
    assert got == [16, 0, 4, 8, 12, 16, 0, 4, 8, 12] and np.dtype(L).itemsize == 16 and np.dtype(W).itemsize == 16


def test_stitch_u8_argument_validation_without_device():
    lib = _lib.load()
    ok = dict(sr=16, n_sr=3, rows=128, sr_w=2048, lines=16, windows=16, n_lines=1, out_w=300, dst=16)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mnet_stitch_u8(a["sr"], a["n_sr"], a["rows"], a["sr_w"], a["lines"], a["windows"], a["n_lines"], a["out_w"], a["dst"], None)

    for bad in ("sr", "lines", "windows", "dst"):
        assert call(**{bad: None}) == -1 and b"null" in lib.mnet_last_error()
    for bad in (dict(n_lines=0), dict(n_lines=-2), dict(rows=0), dict(sr_w=0), dict(out_w=0), dict(out_w=-7), dict(n_sr=0), dict(n_sr=-1)):
        assert call(**bad) == -1 and b"bad shape" in lib.mnet_last_error()
    assert call(sr_w=(1 << 22) + 1) == -1 and b"too large" in lib.mnet_last_error()
    assert call(n_lines=1 << 30, out_w=1 << 20) == -1 and b"too large" in lib.mnet_last_error()
    for bad in (dict(lines=18), dict(windows=17), dict(lines=2, windows=2)):
        assert call(**bad) == -2 and b"aligned" in lib.mnet_last_error()


def test_ops_and_driver_refuse_cpu_tensors_and_bad_plans():
    from marconet_amd import ops
    sr = torch.zeros((2, 128, 2048, 3), dtype=torch.uint8)
    tab = torch.zeros((1, 16), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.stitch_u8(sr, tab, tab, out_w=10)
    W = long_lines.Window
    with pytest.raises(ValueError, match="one SR image per window"):
        long_lines.compose_lines(sr, [[W(0, 10, 0, 3, 0, 40)]])
    with pytest.raises(ValueError, match="line 0 cannot be followed"):                        # a gap, found before any copy or launch
        long_lines.compose_lines(sr, [[W(0, 10, 0, 3, 0, 40), W(8, 20, 2, 5, 41, 50)]])
    with pytest.raises(ValueError, match="line 0 cannot be followed"):                        # wider than the SR image
        long_lines.compose_lines(sr, [[W(0, 10, 0, 3, 0, 2049), W(8, 20, 2, 5, 2000, 50)]])


def test_build_script_compiles_and_stamps_the_kernel():
    sh = open(os.path.join(CSRC, "build.sh")).read()
    import re
    assert re.search(r'^SRCS="[^"]*\bstitch_kernels\b[^"]*"', sh, flags=re.M)
    assert '[ "$1" = stitch_kernels ] && cat "$HERE/stitch_blend.h"' in sh
