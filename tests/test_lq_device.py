"""not-gpu: the host-side pieces of the device LQ path (marconet_amd/lq_device.py, mnet_lq_from_u8) against the pure-host definition lq_io —
the tap function of csrc/lq_taps.h compiled for the CPU, the per-strip scalars and errors, the descriptor's C layout, the entry point's argument
checks, and the two facts the kernel's arithmetic leans on (int32 holds every sum; correctly rounded fp32 divides give torch's Normalize)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from marconet_amd import _lib, lq_device, lq_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_TAPS_MAIN = r'''
#include <stdio.h>
#include <stdlib.h>
#include "lq_taps.h"
/* stdin: lines "n_dst n_src scale" (scale as a C99 hex float) -> stdout: n_dst x (4 indices, 4 taps) int32 per line, binary */
int main(void) {
    int n_dst, n_src; char buf[128];
    while (scanf("%d %d %127s", &n_dst, &n_src, buf) == 3) {
        const double scale = strtod(buf, NULL);
        for (int d = 0; d < n_dst; ++d) {
            const LqTaps t = lq_cubic_taps(d, n_src, scale);
            fwrite(t.idx, sizeof(int), 4, stdout);
            fwrite(t.tap, sizeof(int), 4, stdout);
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
    d = tmp_path_factory.mktemp("lq_taps")
    src, exe = str(d / "taps_main.cpp"), str(d / "taps_main")
    with open(src, "w") as f:
        f.write(_TAPS_MAIN)
    # -ffp-contract=off: every operation of the weights rounded separately (build.sh gives the device build the same flag)
    subprocess.check_call([_cxx(), "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "marconet_amd", "csrc"), src, "-o", exe])
    return exe


def _run_taps(exe, cases):
    """cases: [(n_dst, n_src, scale)] -> list of (idx [n_dst,4], taps [n_dst,4])"""
    text = "".join("%d %d %s\n" % (nd, ns, float(sc).hex()) for nd, ns, sc in cases)
    raw = np.frombuffer(subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout, dtype=np.int32)
    assert raw.size == 8 * sum(c[0] for c in cases)
    out, o = [], 0
    for nd, _, _ in cases:
        a = raw[o:o + 8 * nd].reshape(nd, 8)
        out.append((a[:, :4], a[:, 4:]))
        o += 8 * nd
    return out


def test_tap_function_matches_cubic_taps(taps_exe):
    """csrc/lq_taps.h on the CPU == lq_io._cubic_taps: the row axis of both products for every source height 1..600, and column axes whose
    length is not tied to the scale (a strip's width at its height's scale); sum |taps| <= 2816, the bound the kernel's int32 sums rest on"""
    cases, inv = [], []
    for n_dst in (32, 128):
        for n_src in range(1, 601):
            fx = n_dst / n_src
            cases.append((n_dst, n_src, 1.0 / fx))
            inv.append(fx)
    for dst_h, h, w in ((32, 47, 300), (128, 47, 300), (32, 100, 1600), (128, 100, 1601), (32, 251, 1999), (128, 251, 1999), (32, 8, 3), (32, 1, 7),
                        (32, 19, 109), (128, 15, 128), (32, 33, 528), (32, 64, 7), (128, 7, 11), (32, 600, 9000), (128, 3, 40)):
        fx = dst_h / h
        cases.append((int(np.rint(w * fx)), w, 1.0 / fx))
        inv.append(fx)
    worst = 0
    for (nd, ns, _), fx, (idx, taps) in zip(cases, inv, _run_taps(taps_exe, cases)):
        ridx, rtaps = lq_io._cubic_taps(nd, ns, fx)
        assert np.array_equal(idx, ridx), (nd, ns)
        assert np.array_equal(taps, rtaps), (nd, ns)
        worst = max(worst, int(np.abs(rtaps).sum(axis=1).max()))
    assert worst <= 2816
    assert 255 * 2816 * 2816 + (1 << 21) < (1 << 31)



def test_device_build_of_the_taps_is_not_contracted(tmp_path):
    """the gfx950 ISA of lq_kernels.hip under build.sh's own flags: no fused multiply-add outside the expansion of the 12 correctly rounded
    fp32 divides of form 0 (2 per colour), which is 3 v_fma_f32 + 2 v_fmac_f32 + 1 v_div_fmas_f32 each — none in fp64, none packed, none with
    a literal.  (The _rn intrinsics of the tap code are plain operators; without -ffp-contract=off hipcc fuses 20 of them.)"""
    import re
    sh = open(os.path.join(ROOT, "marconet_amd", "csrc", "build.sh")).read()
    flags = re.search(r'^FLAGS="([^"]*)"', sh, flags=re.M).group(1).split()
    extra = re.search(r'lq_kernels\) echo "([^"]*)"', sh).group(1).split()
    assert "-ffp-contract=off" in extra
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    asm = str(tmp_path / "lq_kernels.s")
    subprocess.check_call([hipcc] + flags + extra + ["-S", "--cuda-device-only", os.path.join(ROOT, "marconet_amd", "csrc", "lq_kernels.hip"), "-o", asm],
                          stderr=subprocess.DEVNULL)
    ops_ = re.findall(r"^\s+(v_[a-z0-9_]+)", open(asm).read(), flags=re.M)
    fused = [o for o in ops_ if re.match(r"v_(pk_)?(fma|fmac|fmaak|fmamk|mad|mac)_", o) and not o.startswith("v_mad_u") and not o.startswith("v_mad_i")]
    divs = sum(o.startswith("v_div_fmas_f32") for o in ops_)
    assert divs == 12
    assert sorted(set(fused)) == ["v_fma_f32", "v_fmac_f32_e32"], sorted(set(fused))
    assert sum(o == "v_fma_f32" for o in fused) == 3 * divs and sum(o == "v_fmac_f32_e32" for o in fused) == 2 * divs


def test_normalize_is_two_correctly_rounded_divides():
    """form 0 evaluates (u8 / 255 - 0.5) / 0.5 with IEEE fp32 divides: torch's ToTensor + Normalize values for all 256 inputs"""
    u = np.arange(256, dtype=np.uint8)
    t = torch.from_numpy(u.copy()).to(torch.float32).div(255).sub_(0.5).div_(0.5).numpy()
    k = (u.astype(np.float32) / np.float32(255) - np.float32(0.5)) / np.float32(0.5)
    assert k.dtype == np.float32 and np.array_equal(t, k) and t[0] == -1.0 and t[255] == 1.0


def _img(h, w, dtype=np.uint8):
    return np.zeros((h, w, 3), dtype=dtype)


def test_strip_geometry_scalars_and_errors():
    g = lq_device.strip_geometry
    assert g(_img(64, 5)).dw == 2 and g(_img(64, 7)).dw == 4                      # 2.5 -> 2, 3.5 -> 4: half to even
    assert g(_img(33, 528)).dw == 512                                             # the widest accepted strip
    for h, w in ((33, 529), (2, 33)):
        with pytest.raises(lq_io.StripTooWide):
            g(_img(h, w))
        with pytest.raises(lq_io.StripTooWide):
            lq_io.lq_from_image(_img(h, w))
    with pytest.raises(ValueError, match="empty output"):
        g(_img(64, 1))
    # the host path's error types, unchanged
    for bad in (_img(8, 8, np.float32), np.zeros((8, 8), np.uint8), np.zeros((2, 8, 8, 3), np.uint8), _img(64, 1)):
        with pytest.raises((TypeError, ValueError)) as host:
            lq_io.lq_from_image(bad)
        with pytest.raises(host.type):
            g(bad)
    with pytest.raises(ValueError):
        g(np.zeros((8, 8, 4), np.uint8))
    # every scalar is the host's: widths from lq_from_image's own arithmetic, the sampling step from _cubic_taps'
    rng = np.random.default_rng(5)
    for _ in range(300):
        h, w = int(rng.integers(1, 400)), int(rng.integers(1, 3000))
        try:
            geo = g(_img(h, w))
        except ValueError:
            continue
        assert geo.dw == int(np.rint(w * (32 / h))) and geo.show_w == int(np.rint(w * (128 / h)))
        assert geo.scale == 1.0 / (32 / h) and geo.show_scale == 1.0 / (128 / h)


def test_fixed_output_height_holds_up_to_4096():
    """the kernel resizes to a fixed height; the host's own rint(h * (dst_h / h)) is that height for every h <= 4096"""
    for dst_h in (32, 128):
        assert all(lq_device._axis(h, 1, dst_h)[1] == dst_h for h in range(1, 4097))


def test_table_rows_and_packing_offsets():
    geoms = [lq_device.strip_geometry(_img(47, 300)), lq_device.strip_geometry(_img(19, 109))]
    tab = lq_device.build_table(geoms, [0, 47 * 300 * 3], True)
    assert tab.shape == (2, 2) and tab.dtype.itemsize == ctypes.sizeof(_lib.LqImage)
    assert tab[0, 1]["offset"] == 42300 and tab[0, 1]["h"] == 19 and tab[0, 1]["w"] == 109 and tab[0, 1]["dw"] == geoms[1].dw
    assert tab[1, 1]["dw"] == geoms[1].show_w and tab[1, 0]["scale"] == 1.0 / (128 / 47) and tab[0, 0]["scale"] == 1.0 / (32 / 47)
    one = _lib.LqImage.from_buffer_copy(tab[1, 1].tobytes())
    assert (one.offset, one.h, one.w, one.dw, one.reserved, one.scale) == (42300, 19, 109, geoms[1].show_w, 0, geoms[1].show_scale)


def test_lq_image_layout_matches_c(tmp_path):
    """sizeof / offsetof of mnet_lq_image from a C program compiled against the header == the ctypes mirror"""
    code = r'''
#include <stdio.h>
#include <stddef.h>
#include "marconet_hip.h"
int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(mnet_lq_image), offsetof(mnet_lq_image, offset), offsetof(mnet_lq_image, h),
  offsetof(mnet_lq_image, w), offsetof(mnet_lq_image, dw), offsetof(mnet_lq_image, reserved), offsetof(mnet_lq_image, scale)); return 0; }
'''
    cpath, exe = str(tmp_path / "lq_probe.c"), str(tmp_path / "lq_probe")
    with open(cpath, "w") as f:
        f.write(code)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), cpath, "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    L = _lib.LqImage
    assert got == [ctypes.sizeof(L), L.offset.offset, L.h.offset, L.w.offset, L.dw.offset, L.reserved.offset, L.scale.offset]
    assert np.dtype(L).itemsize == ctypes.sizeof(L) == 32


def test_lq_from_u8_argument_validation_without_device():
    lib = _lib.load()
    ok = dict(src=16, images=16, n=1, dst_h=32, canvas_w=512, dst=16, form=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mnet_lq_from_u8(a["src"], a["images"], a["n"], a["dst_h"], a["canvas_w"], a["dst"], a["form"], None)

    for bad in (dict(src=None), dict(images=None), dict(dst=None)):
        assert call(**bad) == -1 and b"null" in lib.mnet_last_error()
    for bad in (dict(n=0), dict(n=-3), dict(dst_h=0), dict(canvas_w=0), dict(canvas_w=-512)):
        assert call(**bad) == -1 and b"bad shape" in lib.mnet_last_error()
    for form in (2, -1):
        assert call(form=form) == -1 and b"unknown form" in lib.mnet_last_error()
    assert call(n=1 << 30, canvas_w=1 << 20) == -1 and b"too large" in lib.mnet_last_error()


def test_ops_lq_from_u8_refuses_cpu_tensors():
    from marconet_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lq_from_u8(torch.zeros(12, dtype=torch.uint8), torch.zeros((1, 32), dtype=torch.uint8), 32, 512)
