"""The identity behind the tap-conv + fold form of the generator's up-convs, stated in fp64 on the host:

    conv3x3(U x; W)[o, p] = sum_t (U Z_t)[o, p + t],    Z_t[o, q] = sum_c W[o, c, t] x[c, q]       (zero where p + t leaves the hi-res map)

U = bilinear x2 (align_corners=False, edge clamp).  Z is ONE 1x1 conv of the low-res map with packing.tapconv_weight's row order (t·O + o, t = 3·ky + kx);
`fold_ref` is the sum over the nine up-sampled, shifted planes.  The identity is exact at the borders (U keeps its clamp, the shift keeps the hi-res zero
padding), so the maps here are the ones where clamp and padding meet.  `fold_ref` / `epilogue_ref` are the references of tests/test_upfold_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

from marconet_amd import packing

MAPS = [(1, 1), (1, 5), (2, 2), (5, 7), (4, 4)]


def tap_planes(x, w):
    """x [N,Cin,h,w], w [O,Cin,3,3] (both fp64) → Z [N,9·O,h,w]: the 1x1 conv with the tap-major rows of packing.tapconv_weight"""
    return F.conv2d(x, packing.tapconv_weight(w))


def _fold(z, c):
    n, c9, h, w = z.shape
    assert c9 == 9 * c
    up = F.pad(F.interpolate(z, scale_factor=2, mode="bilinear", align_corners=False), (1, 1, 1, 1))
    y = torch.zeros((n, c, 2 * h, 2 * w), dtype=z.dtype)
    for ky in range(3):
        for kx in range(3):
            t = 3 * ky + kx
            y += up[:, t * c:(t + 1) * c, ky:ky + 2 * h, kx:kx + 2 * w]
    return y


def fold_ref(z, c):
    """z [N,9·c,h,w] fp64 (channel t·c + o) → [N,c,2h,2w]: sum over the taps of the bilinear x2 of plane t, shifted by tap t, zero outside the hi-res map"""
    assert z.dtype == torch.float64
    return _fold(z, c)


def fold_f32(z, c):
    """fold_ref's formula evaluated in fp32 (what a correct fp32 kernel can at best hold before it rounds to its storage)"""
    assert z.dtype == torch.float32
    return _fold(z, c)


def fold_ref_banded(z, c, band):
    """fold_ref in bands of ``band`` low-res columns with a one-column halo on each side (maps whose padded up-sampled copy does not fit in memory): hi-res columns
    2a ... 2b-1 read up-sampled columns 2a-1 ... 2b, i.e. low-res columns a-1 ... b; inside the halo the band's own clamp and zero padding are cut away, at the map's
    edges they are the map's.  Equal to fold_ref bit for bit (the same products and the same order of sums per output)."""
    n, _, h, w = z.shape
    assert z.dtype == torch.float64 and band >= 1
    y = torch.empty((n, c, 2 * h, 2 * w), dtype=torch.float64)
    for a in range(0, w, band):
        b = min(a + band, w)
        lo, hi = max(a - 1, 0), min(b + 1, w)
        y[:, :, :, 2 * a:2 * b] = fold_ref(z[:, :, :, lo:hi].contiguous(), c)[:, :, :, 2 * (a - lo):2 * (a - lo) + 2 * (b - a)]
    return y


def fold_input(p, seed, scale=1.5):
    """random z [n,h,w,9c] fp32 NHWC for the map p = (n, h, w, c)"""
    n, h, w, c = p
    return torch.randn((n, h, w, 9 * c), generator=torch.Generator().manual_seed(seed)) * scale


def epilogue_ref(v, out_scale=None, bias=None, act=3, post_scale=None):
    """the conv epilogue's contract on NCHW fp64 ``v``: post_scale[n,c] · act(out_scale[n,c] · v + bias[c]); act 0 / 2 / 3 = none / LeakyReLU(0.2) / ·√2"""
    if out_scale is not None:
        v = v * out_scale.double()[:, :, None, None]
    if bias is not None:
        v = v + bias.double()[None, :, None, None]
    if act in (2, 3):
        v = F.leaky_relu(v, 0.2) * (2.0 ** 0.5 if act == 3 else 1.0)
    if post_scale is not None:
        v = v * post_scale.double()[:, :, None, None]
    return v


def test_tapconv_weight_is_the_tap_major_permutation():
    w = torch.arange(2 * 3 * 9, dtype=torch.float64).reshape(2, 3, 3, 3)
    wt = packing.tapconv_weight(w)
    assert tuple(wt.shape) == (18, 3, 1, 1)
    for ky in range(3):
        for kx in range(3):
            for o in range(2):
                assert torch.equal(wt[(3 * ky + kx) * 2 + o, :, 0, 0], w[o, :, ky, kx])
    with pytest.raises(ValueError):
        packing.tapconv_weight(torch.zeros(2, 3, 1, 1))
    with pytest.raises(ValueError):      # blocked storages: the taps' row blocks must not be padded apart
        packing.pack_tapconv_weight(torch.zeros(8, 32, 3, 3), packing.MX_DTYPE)


@pytest.mark.parametrize("hw", MAPS, ids=["%dx%d" % m for m in MAPS])
def test_fold_of_tap_planes_is_the_upconv(hw):
    h, w = hw
    g = torch.Generator().manual_seed(1000 + 10 * h + w)
    x = torch.randn((2, 5, h, w), generator=g, dtype=torch.float64)
    wgt = torch.randn((4, 5, 3, 3), generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False), wgt, padding=1)
    got = fold_ref(tap_planes(x, wgt), 4)
    err = (got - ref).abs().max().item()
    print("upfold identity %dx%d: max|d| = %.3e (ref max %.3e)" % (h, w, err, ref.abs().max().item()))
    assert err <= 1e-12


def test_pack_tapconv_weight_host_path_holds_the_permuted_values():
    """the fp16+8 pack of the tap-major rows decodes to the permuted weights (through the ordinary pack_conv_weight: no packing of its own)"""
    g = torch.Generator().manual_seed(7)
    w = torch.randn((32, 64, 3, 3), generator=g) * 0.05
    a = packing.pack_tapconv_weight(w, torch.float32, scale=0.5)
    assert tuple(a.shape) == (288, 1, 1, 64)
    assert torch.equal(a.reshape(9, 32, 64), (w * 0.5).permute(2, 3, 0, 1).reshape(9, 32, 64))
    m = packing.pack_tapconv_weight(w, packing.MX_DTYPE, scale=0.5)
    assert m.dtype == packing.MX_DTYPE and m.shape[0] == packing.mx_weight_rows(288, 1, 1, 64) and tuple(m.shape[1:]) == (1, 1, 64)


# ------------------------------------------------------------------------------------------------ the entry point's own header and binding
def _upfold_header():
    import os
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "marconet_hip_upfold.h")


def test_upfold_header_matches_its_binding_and_the_library():
    """include/marconet_hip_upfold.h declares exactly the functions of _lib.UPFOLD_SYMBOLS, the library exports them, and none of them sits in the
    table of marconet_hip.h (tests/test_abi.py checks that one the same way)"""
    import re
    from marconet_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(_upfold_header()).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mnet_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.UPFOLD_SYMBOLS) == ["mnet_upfold3x3_nhwc"]
    assert not set(names) & set(_lib.SYMBOLS)
    lib = _lib.load()
    for n in names:
        fn = getattr(lib, n)
        assert fn.restype is _lib.UPFOLD_SYMBOLS[n][0] and list(fn.argtypes) == _lib.UPFOLD_SYMBOLS[n][1]
    proto = re.search(r"int\s+mnet_upfold3x3_nhwc\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    assert len(proto.split(",")) == len(_lib.UPFOLD_SYMBOLS["mnet_upfold3x3_nhwc"][1]) == 12
    assert lib.mnet_abi_version() == _lib.ABI_VERSION == 4


def test_upfold_header_is_plain_c(tmp_path):
    import os
    import shutil
    import subprocess
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    cpath = str(tmp_path / "probe.c")
    with open(cpath, "w") as f:
        f.write('#include "marconet_hip_upfold.h"\nint main(void) { int (*f)(const void*, void*, int32_t, int32_t, int32_t, int32_t, int32_t, const float*, const float*, int32_t, const float*, void*) = mnet_upfold3x3_nhwc; (void)f; return MNET_ABI_VERSION == 4 ? 0 : 1; }\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(_upfold_header()), cpath])


def test_upfold_refuses_bad_arguments_without_a_device():
    """every argument is checked before anything is enqueued: these calls fail on a machine without a GPU too"""
    import ctypes
    from marconet_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 127) // 128 * 128
    z, y = ctypes.c_void_p(a), ctypes.c_void_p(a + 2048)
    f = lib.mnet_upfold3x3_nhwc
    assert f(None, y, 3, 1, 1, 1, 32, None, None, 0, None, None) == -1              # null pointer
    assert f(z, z, 3, 1, 1, 1, 32, None, None, 0, None, None) == -1                 # in place
    assert f(z, y, 3, 0, 1, 1, 32, None, None, 0, None, None) == -1                 # geometry
    assert f(z, y, 7, 1, 1, 1, 32, None, None, 0, None, None) == -1                 # dtype
    assert f(z, y, 3, 1, 1, 1, 32, None, None, 4, None, None) == -1                 # activation outside NONE / LRELU / LRELU_SQRT2
    assert f(z, y, 3, 1, 1, 1, 24, None, None, 0, None, None) == -2                 # blocked storage: c % 32
    assert f(ctypes.c_void_p(a + 16), y, 3, 1, 1, 1, 32, None, None, 0, None, None) == -2      # blocked storage: 128-byte alignment
    assert f(z, y, 1, 1, 1, 1, 32, None, ctypes.c_void_p(a + 4), 0, None, None) == -2          # vector not 16-byte aligned
    assert b"upfold3x3" in lib.mnet_last_error()
