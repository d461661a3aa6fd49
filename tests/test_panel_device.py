"""not-gpu: the host-side pieces of the device panel path (marconet_amd/panel_device.py, mnet_panel_u8) against the pure-host definition lq_io —
the tap function of csrc/panel_taps.h compiled for the CPU, the mark intervals against draw_locs, the descriptor's C layout, the entry point's
argument checks, the build flags of panel_kernels.hip (no fused multiply-add in its gfx950 ISA) and the two facts the kernel leans on: the
vertical pass of resize_linear is the identity for 128 → 128 rows, and panel_rgb_u8 is what save_panel writes."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from marconet_amd import _lib, lq_io, panel_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marconet_amd", "csrc")

_TAPS_MAIN = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "panel_taps.h"
/* stdin: lines "n_dst n_src step" (step as a C99 hex float) -> stdout: n_dst x (i0, i1, bits of t) int32 per line, binary */
int main(void) {
    int n_dst, n_src; char buf[128];
    while (scanf("%d %d %127s", &n_dst, &n_src, buf) == 3) {
        const double step = strtod(buf, NULL);
        for (int x = 0; x < n_dst; ++x) {
            const PanelTap p = panel_linear_tap(x, n_src, step);
            int out[3] = {p.i0, p.i1, 0};
            memcpy(&out[2], &p.t, sizeof(float));
            fwrite(out, sizeof(int), 3, stdout);
        }
    }
    return 0;
}
'''


def _cxx():
    for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    raise RuntimeError("no C++ compiler found")


@pytest.fixture(scope="module")
def taps_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("panel_taps")
    src, exe = str(d / "taps_main.cpp"), str(d / "taps_main")
    with open(src, "w") as f:
        f.write(_TAPS_MAIN)
    # -ffp-contract=off: every operation rounded separately (build.sh gives the device build the same flag)
    subprocess.check_call([_cxx(), "-O2", "-ffp-contract=off", "-I", CSRC, src, "-o", exe])
    return exe


def _linear_taps(n_dst, n_src):
    """lq_io.resize_linear's inner ``taps`` restated (a closure cannot be called from here); ``test_tap_function_matches_resize_linear`` pins
    this restatement to resize_linear itself on random rows before it compares the header with it"""
    f = (np.arange(n_dst, dtype=np.float64) + 0.5) * (n_src / n_dst) - 0.5
    i0 = np.floor(f).astype(np.int64)
    t = (f - i0).astype(np.float32)
    t[i0 < 0] = 0.0
    i0 = np.maximum(i0, 0)
    t[i0 >= n_src - 1] = 0.0
    i0 = np.minimum(i0, n_src - 1)
    return i0, np.minimum(i0 + 1, n_src - 1), t


def test_tap_function_matches_resize_linear(taps_exe):
    """csrc/panel_taps.h on the CPU == resize_linear's taps(show_w, 128 n) for every show_w in 1..2050 and n in {1, 2, 3, 7, 16}: the header's
    (i0, i1, t) equal the restated taps, and the restated taps blend a random row into exactly what resize_linear returns for it"""
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 7, 16):
        n_src = 128 * n
        row = rng.standard_normal((1, n_src, 3)).astype(np.float32)
        widths = list(range(1, 2051))
        text = "".join("%d %d %s\n" % (w, n_src, float(n_src / w).hex()) for w in widths)
        raw = np.frombuffer(subprocess.run([taps_exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout, dtype=np.int32)
        assert raw.size == 3 * sum(widths)
        o = 0
        for w in widths:
            got = raw[o:o + 3 * w].reshape(w, 3)
            o += 3 * w
            i0, i1, t = _linear_taps(w, n_src)
            want = row[:, i0, :] * (np.float32(1) - t)[None, :, None] + row[:, i1, :] * t[None, :, None]
            assert np.array_equal(lq_io.resize_linear(row, w, 1), want), (n, w)          # the restatement IS resize_linear's
            assert np.array_equal(got[:, 0], i0) and np.array_equal(got[:, 1], i1), (n, w)
            assert np.array_equal(got[:, 2].copy().view(np.float32), t), (n, w)
            assert i0.min() >= 0 and i1.max() <= n_src - 1


def test_vertical_pass_is_the_identity_for_128_rows():
    """the kernel has no vertical pass: resize_linear(img[128, w], dst_w, 128) is, row by row, the horizontal resize alone"""
    rng = np.random.default_rng(12)
    for w, dst_w in ((128, 1), (128, 128), (384, 37), (256, 700), (2048, 65), (640, 641)):
        img = rng.standard_normal((128, w, 3)).astype(np.float32)
        full = lq_io.resize_linear(img, dst_w, 128)
        rows = np.concatenate([lq_io.resize_linear(img[y:y + 1], dst_w, 1) for y in range(128)], axis=0)
        assert full.dtype == np.float32 and np.array_equal(full, rows)


def _paint(show, marks):
    """the marks row from the resolved intervals, as the kernel paints it: plain non-negative column ranges"""
    out = np.array(show, copy=True)
    for a, b, r, t in marks.tolist():
        assert 0 <= a <= show.shape[1] and 0 <= b <= show.shape[1] and 0 <= r <= show.shape[1] and 0 <= t <= show.shape[1]
        for x in range(a, b):
            out[:64, x] = (255, 0, 0)
        for x in range(r, t):
            out[64:, x] = (0, 0, 255)
    return out


FIXED_LOCS = (
    ("wrap_left_edge_below_minus_2", [-0.002, 0.0005, 0.3, 0.05]),       # x = -5: the red slice 0:-3 wraps to 0:show_w - 3
    ("wrap_exactly_minus_2", [-0.001, 0.0, 0.5, 0.0]),                    # x = -2: the red slice 0:0 is empty, blue 0:-1 wraps
    ("right_of_show_w_and_of_2048", [0.99, 0.02, 1.2, 0.1, 0.2, 0.9]),     # edges beyond the preview and beyond 2048
    ("zero_half_width", [0.1, 0.0, 0.05, 0.0]),
    ("all_left_of_the_canvas", [-0.5, 0.1]),
    ("edge_at_show_w", [300 / 2048, 0.0, 1 / 2048, 0.0, 3 / 2048, 0.0]),
)


@pytest.mark.parametrize("show_w", (1, 3, 300, 2048))
def test_mark_intervals_paint_what_draw_locs_paints(show_w):
    rng = np.random.default_rng(show_w)
    show = rng.integers(0, 256, (128, show_w, 3), dtype=np.uint8)
    cases = [(name, np.float32(l)) for name, l in FIXED_LOCS]
    for k in range(60):
        n = int(rng.integers(1, 17))
        loc = np.empty(2 * n, np.float32)
        loc[0::2] = rng.uniform(-0.05, 1.1, n) * (show_w / 2048 if k % 2 else 1.0)
        loc[1::2] = rng.uniform(-0.01, 0.06, n)
        cases.append(("random%d" % k, loc))
    painted = 0
    for name, loc in cases:
        n = loc.size // 2
        m = panel_device.mark_intervals(loc, n, show_w)
        assert m.shape == (n, 4) and m.dtype == np.int32
        want = lq_io.draw_locs(show, loc, n)
        assert np.array_equal(_paint(show, m), want), name
        painted += int((want != show).any())
    assert painted >= 5                                                                 # not vacuous, even on a one-column preview
    assert panel_device.mark_intervals(np.zeros(0, np.float32), 0, show_w).shape == (0, 4)              # n = 0: nothing to paint
    assert np.array_equal(lq_io.draw_locs(show, np.zeros(0, np.float32), 0), show)
    # a torch row, as restore_images' strips carry it
    assert np.array_equal(panel_device.mark_intervals(torch.tensor([0.25, 0.01]), 1, show_w), panel_device.mark_intervals(np.float32([0.25, 0.01]), 1, show_w))


def test_negative_stop_wraps_as_the_issue_states():
    """locs (-0.002, 0.0005) on a 300-wide preview paint red on columns 0..296"""
    show = np.full((128, 300, 3), 7, np.uint8)
    m = panel_device.mark_intervals(np.float32([-0.002, 0.0005]), 1, 300)
    assert m[0, :2].tolist() == [0, 297]
    red = (lq_io.draw_locs(show, np.float32([-0.002, 0.0005]), 1)[:64] == (255, 0, 0)).all(axis=(0, 2))
    assert red[:297].all() and not red[297:].any()


def test_build_tables_rows():
    tab, marks = panel_device.build_tables([2, 0], [300, 65], [3, 16], [np.float32([0.1, 0.01] * 3), np.float32([0.5, 0.02] * 16)])
    assert tab.dtype.itemsize == ctypes.sizeof(_lib.PanelStrip) == 24 and marks.shape == (19, 4) and marks.dtype == np.int32
    one = _lib.PanelStrip.from_buffer_copy(tab[1].tobytes())
    assert (one.show_w, one.preview_index, one.glyph0, one.n_glyphs, one.step) == (65, 0, 3, 16, 2048 / 65)
    assert tab[0]["step"] == 384 / 300 and tab[0]["glyph0"] == 0
    assert np.array_equal(marks[3:], panel_device.mark_intervals(np.float32([0.5, 0.02] * 16), 16, 65))


def test_panel_strip_layout_matches_c(tmp_path):
    """sizeof / offsetof of mnet_panel_strip from a C program compiled against the header == the ctypes mirror"""
    code = r'''
#include <stdio.h>
#include <stddef.h>
#include "marconet_hip.h"
int main(void){ printf("%zu %zu %zu %zu %zu %zu\n", sizeof(mnet_panel_strip), offsetof(mnet_panel_strip, show_w), offsetof(mnet_panel_strip, preview_index),
  offsetof(mnet_panel_strip, glyph0), offsetof(mnet_panel_strip, n_glyphs), offsetof(mnet_panel_strip, step)); return 0; }
'''
    cpath, exe = str(tmp_path / "panel_probe.c"), str(tmp_path / "panel_probe")
    with open(cpath, "w") as f:
        f.write(code)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), cpath, "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    S = _lib.PanelStrip
    assert got == [ctypes.sizeof(S), S.show_w.offset, S.preview_index.offset, S.glyph0.offset, S.n_glyphs.offset, S.step.offset]
    assert got == [24, 0, 4, 8, 12, 16] and np.dtype(S).itemsize == 24


def test_panel_u8_argument_validation_without_device():
    lib = _lib.load()
    ok = dict(preview=16, preview_w=2048, sr=16, sr_w=2048, prior=16, strips=16, marks=16, n=1, out_w=300, dst=16)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mnet_panel_u8(a["preview"], a["preview_w"], a["sr"], a["sr_w"], a["prior"], a["strips"], a["marks"], a["n"], a["out_w"], a["dst"], None)

    for bad in ("preview", "sr", "prior", "strips", "marks", "dst"):
        assert call(**{bad: None}) == -1 and b"null" in lib.mnet_last_error()
    for bad in (dict(n=0), dict(n=-3), dict(out_w=0), dict(out_w=-5), dict(preview_w=299), dict(sr_w=0)):
        assert call(**bad) == -1 and b"bad shape" in lib.mnet_last_error()
    assert call(n=1 << 30, out_w=1 << 20, preview_w=1 << 20) == -1 and b"too large" in lib.mnet_last_error()
    for bad in (dict(prior=8), dict(strips=20), dict(marks=18)):
        assert call(**bad) == -2 and b"aligned" in lib.mnet_last_error()


def test_ops_panel_u8_refuses_cpu_tensors_and_wrong_shapes():
    from marconet_amd import ops
    pv, sr = torch.zeros((1, 128, 64, 3), dtype=torch.uint8), torch.zeros((1, 128, 2048, 3), dtype=torch.uint8)
    prior, strips, marks = torch.zeros((1, 128, 128, 4)), torch.zeros((1, 24), dtype=torch.uint8), torch.zeros((1, 4), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.panel_u8(pv, sr, prior, strips, marks)


def test_compose_panels_refuses_a_strip_wider_than_the_sr_image_on_the_host():
    """h = 64, w = 1025 passes the 512-px check with show_w = 2050 > 2048: ValueError naming the strip, before any copy or launch (CPU tensors
    would be refused further down)"""
    from marconet_amd import lq_device
    g = lq_device.strip_geometry(np.zeros((64, 1025, 3), np.uint8))
    assert g.dw == 512 and g.show_w == 2050
    pv, sr = torch.zeros((2, 128, 2050, 3), dtype=torch.uint8), torch.zeros((2, 128, 2048, 3), dtype=torch.uint8)
    prior = torch.zeros((2, 128, 128, 4))
    with pytest.raises(ValueError, match="strip 1 is 2050 px wide"):
        panel_device.compose_panels(pv, [0, 1], [300, 2050], sr, prior, [1, 1], [np.float32([0.5, 0.1])] * 2)
    with pytest.raises(ValueError, match="strip 0 has no character"):
        panel_device.compose_panels(pv, [0, 1], [300, 200], sr, prior, [0, 2], [np.float32([0.5, 0.1] * 2)] * 2)
    with pytest.raises(ValueError):                                                     # lq_io.panel raises there too
        lq_io.panel(None, np.float32([0.5, 0.1]), 1, np.zeros((128, 2048, 3), np.uint8), np.zeros((128, 128, 3), np.float32),
                    show=np.zeros((128, 2050, 3), np.uint8))


def test_panel_rgb_u8_is_what_save_panel_writes(tmp_path):
    rng = np.random.default_rng(3)
    bgr = rng.uniform(-20, 280, (16, 9, 3)).astype(np.float32)
    bgr[0, :6, 0] = (0.5, 1.5, 2.5, 254.5, 255.5, -0.5)                                # halves go to even, both ends saturate
    u8 = lq_io.panel_rgb_u8(bgr)
    assert u8.dtype == np.uint8 and u8.flags["C_CONTIGUOUS"] and u8[0, :6, 2].tolist() == [0, 2, 2, 254, 255, 0]
    assert np.array_equal(u8, np.clip(np.rint(bgr.astype(np.float64)), 0, 255).astype(np.uint8)[:, :, ::-1])
    path = str(tmp_path / "p.png")
    lq_io.save_panel(path, bgr)
    assert np.array_equal(lq_io.load_png(path), u8)


def test_device_build_of_the_panel_kernel_is_not_contracted(tmp_path):
    """the gfx950 ISA of panel_kernels.hip under build.sh's own flags holds no floating-point fused multiply-add at all (the kernel has no
    divide to expand); integer v_mad_u* / v_mad_i* do not count.  build.sh keeps the lq_kernels arm as tests/test_lq_device.py parses it."""
    sh = open(os.path.join(CSRC, "build.sh")).read()
    assert 'lq_kernels) echo "-ffp-contract=off" ;;' in sh
    assert re.search(r'^SRCS="[^"]*\bpanel_kernels\b[^"]*"', sh, flags=re.M)
    assert '[ "$1" = panel_kernels ] && cat "$HERE/panel_taps.h"' in sh
    flags = re.search(r'^FLAGS="([^"]*)"', sh, flags=re.M).group(1).split()
    extra = re.search(r'panel_kernels\) echo "([^"]*)"', sh).group(1).split()
    assert "-ffp-contract=off" in extra
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    asm = str(tmp_path / "panel_kernels.s")
    subprocess.check_call([hipcc] + flags + extra + ["-S", "--cuda-device-only", os.path.join(CSRC, "panel_kernels.hip"), "-o", asm], stderr=subprocess.DEVNULL)
    ops_ = re.findall(r"^\s+(v_[a-z0-9_]+)", open(asm).read(), flags=re.M)
    assert any(o.startswith("v_mul_f32") for o in ops_) and any(o.startswith("v_mul_f64") for o in ops_)      # the arithmetic is there, unfused
    fused = [o for o in ops_ if re.match(r"v_(pk_)?(fma|fmac|fmaak|fmamk|mad|mac)_", o) and not o.startswith("v_mad_u") and not o.startswith("v_mad_i")]
    assert fused == [], sorted(set(fused))
