"""not-gpu: the fp32 tap planes of the tap-conv + fold form — MNET_CONV_ALGO_FLAG_F32_OUT in the planner and mnet_upfold3x3_f32z_nhwc's header, binding and
argument checks.  Everything here is answered before any HIP call, so it runs on a machine without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "marconet_hip_upfold_f32.h")


def _desc(dtype=3, n=4, h=16, w=16, c0=512, cout=9 * 256, k=1):
    from marconet_amd import _lib
    d = _lib.ConvDesc()
    d.dtype = dtype
    d.x0 = d.wgt = d.y = 128
    d.n, d.h, d.w, d.ho, d.wo = n, h, w, h, w
    d.c0, d.cout, d.kh, d.kw = c0, cout, k, k
    d.stride_h = d.stride_w = 1
    d.pad_h = d.pad_w = k // 2
    return d


def test_header_matches_its_binding_and_the_library():
    """include/marconet_hip_upfold_f32.h declares exactly the functions of _lib.UPFOLD_F32Z_SYMBOLS, the library exports them, and none of them sits in the
    table of marconet_hip.h or in marconet_hip_upfold.h"""
    from marconet_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mnet_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.UPFOLD_F32Z_SYMBOLS) == ["mnet_upfold3x3_f32z_nhwc"]
    assert not set(names) & (set(_lib.SYMBOLS) | set(_lib.UPFOLD_SYMBOLS))
    lib = _lib.load()
    fn = lib.mnet_upfold3x3_f32z_nhwc
    assert fn.restype is _lib.UPFOLD_F32Z_SYMBOLS[names[0]][0] and list(fn.argtypes) == _lib.UPFOLD_F32Z_SYMBOLS[names[0]][1]
    proto = re.search(r"int\s+mnet_upfold3x3_f32z_nhwc\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    assert len(proto.split(",")) == len(fn.argtypes) == 12
    assert lib.mnet_abi_version() == _lib.ABI_VERSION == 4
    flags = re.search(r"MNET_CONV_ALGO_FLAG_F32_OUT\s*=\s*(\d+)", open(os.path.join(ROOT, "include", "marconet_hip.h")).read())
    assert int(flags.group(1)) == _lib.ALGO_FLAG_F32_OUT == 2048


def test_header_is_plain_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    cpath = str(tmp_path / "probe.c")
    with open(cpath, "w") as f:
        f.write('#include "marconet_hip_upfold_f32.h"\nint main(void) { int (*f)(const float*, void*, int32_t, int32_t, int32_t, int32_t, int32_t, const float*, '
                'const float*, int32_t, const float*, void*) = mnet_upfold3x3_f32z_nhwc; (void)f; '
                'return (MNET_CONV_ALGO_FLAGS & MNET_CONV_ALGO_FLAG_F32_OUT) && MNET_ABI_VERSION == 4 ? 0 : 1; }\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), cpath])


def test_planner_accepts_the_plain_one_wave_launch_only():
    """mnet_conv2d_plan under MNET_CONV_ALGO_FLAG_F32_OUT: the one-wave tile (id 16) whatever the batch, and a refusal — with a message that says why — for every
    epilogue term, another storage, an activation, and a launch that resolves to another tile"""
    from marconet_amd import _lib
    lib = _lib.load()
    F = _lib.ALGO_FLAG_F32_OUT
    plan = lambda d, algo=0: lib.mnet_conv2d_plan(ctypes.byref(d), algo | F)
    for n in (1, 2, 4096):                                                       # 256 pixels ... the flagship's 2^20: the form never depends on the batch
        for cout in (9 * 256, 9 * 512):
            assert plan(_desc(n=n, cout=cout)) == _lib.ALGO_DMA_CFG16
    assert plan(_desc(n=1, h=4, w=8, c0=32, cout=288), _lib.ALGO_DMA_CFG16) == _lib.ALGO_DMA_CFG16      # 32 pixels, one k-slab
    assert plan(_desc(k=3, c0=64, cout=256)) == _lib.ALGO_DMA_CFG16              # (not only 1x1)
    for field, word in (("bias", b"bias"), ("out_scale", b"scale"), ("post_scale", b"scale"), ("residual", b"residual"), ("gn_partial", b"gn_partial"),
                        ("valid_w", b"valid_w"), ("in_scale", b"F32_OUT")):
        d = _desc()
        setattr(d, field, 128)
        assert plan(d) == -1 and word in lib.mnet_last_error() and b"F32_OUT" in lib.mnet_last_error(), field
    for act in range(1, 7):
        d = _desc()
        d.act = act
        assert plan(d) == -1 and b"activation" in lib.mnet_last_error()
    for dtype in (0, 1, 2):
        d = _desc(dtype=dtype)
        assert plan(d) == -1 and b"MNET_F16M" in lib.mnet_last_error()
    assert plan(_desc(), _lib.ALGO_FLAG_SHUFFLE2) < 0
    # another tile: pinned, or the one-wave tile's own hand-overs (32-pixel fragments inside one image; 512 k-slabs)
    for algo in (_lib.ALGO_DMA_CFG0 + 15, _lib.ALGO_DMA_CFG0 + 10, _lib.ALGO_DMA_CFG0 + 6):
        assert plan(_desc(), algo) == -1 and b"one-wave" in lib.mnet_last_error()
    assert plan(_desc(h=6, w=6)) == -1 and b"resolves to id 15" in lib.mnet_last_error()
    assert plan(_desc(k=3, c0=1856, cout=256)) == -1 and b"resolves to id 15" in lib.mnet_last_error()
    for algo in (_lib.ALGO_REG_STAGED, _lib.ALGO_STRIP_CFG0, _lib.ALGO_SKINNY):
        assert plan(_desc(), algo) == -1 and b"LDS-DMA" in lib.mnet_last_error()
    assert plan(_desc(c0=48)) < 0                                                # cin % 32
    # without the flag nothing changed: the same descriptors keep their answers
    assert lib.mnet_conv2d_plan(ctypes.byref(_desc(n=4096)), 0) == _lib.ALGO_DMA_CFG16
    assert lib.mnet_conv2d_plan(ctypes.byref(_desc(n=2)), 0) == _lib.ALGO_DMA_CFG0 + 10


def test_launch_refuses_what_the_planner_refuses_without_a_device():
    from marconet_amd import _lib
    lib = _lib.load()
    d = _desc()
    d.bias = 128
    assert lib.mnet_conv2d_nhwc_ex(ctypes.byref(d), _lib.ALGO_FLAG_F32_OUT, None) == -1 and b"F32_OUT" in lib.mnet_last_error()
    assert lib.mnet_conv2d_nhwc_ex(ctypes.byref(_desc()), _lib.ALGO_FLAG_F32_OUT | (_lib.ALGO_DMA_CFG0 + 15), None) == -1 and b"one-wave" in lib.mnet_last_error()
    assert lib.mnet_conv2d_nhwc_ex(ctypes.byref(_desc(dtype=2)), _lib.ALGO_FLAG_F32_OUT, None) == -1


def test_ops_plan_and_wrappers_on_the_host():
    """ops.upfold_plan(out_f32=True) asks with the flag (no device needed), and ops.upfold3x3 refuses a storage pair the kernels do not have"""
    from marconet_amd import _lib, ops
    from marconet_amd.packing import MX_DTYPE, SPLIT_DTYPE, tag

    def new_tensor(shape, dtype, device, zero=True):                            # 128-byte aligned on the host too (the planner's answer depends on it)
        numel = shape[0] * shape[1] * shape[2] * shape[3]
        buf = torch.zeros(numel + 32, dtype=dtype, device=device)
        off = (-buf.data_ptr() % 128) // 4
        return tag(buf[off:off + numel].view(shape))

    x = new_tensor((2, 16, 16, 512), MX_DTYPE, "cpu", zero=True)
    assert ops.upfold_plan(x, 256, out_f32=True) == ops.upfold_plan(x, 512, out_f32=True) == _lib.ALGO_DMA_CFG16
    assert ops.upfold_plan(new_tensor((1, 16, 16, 512), MX_DTYPE, "cpu", zero=True), 256, out_f32=True) == _lib.ALGO_DMA_CFG16
    assert ops.upfold_plan(x, 256) == _lib.ALGO_DMA_CFG0 + 10                   # the fp16+8 planes: the planner's ordinary choice
    assert ops.upfold_plan(x, 128, out_f32=True) < 0 and ops.upfold_plan(x, 256, levels={}, out_f32=True) < 0
    assert ops.upfold_plan(new_tensor((2, 16, 16, 512), SPLIT_DTYPE, "cpu", zero=True), 256, out_f32=True) < 0
    assert ops.conv_plan(x, 9 * 256, 1, 1, act=ops.ACT_LRELU, algo=_lib.ALGO_FLAG_F32_OUT) < 0


def test_fold_refuses_bad_arguments_without_a_device():
    """every argument is checked before anything is enqueued; the two "image too large" guards are those of mnet_upfold3x3_nhwc on fp16+8"""
    from marconet_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 127) // 128 * 128
    z, y = ctypes.c_void_p(a), ctypes.c_void_p(a + 2048)
    f = lib.mnet_upfold3x3_f32z_nhwc
    for ydtype in (0, 1, 2, 7):
        assert f(z, y, ydtype, 1, 1, 1, 32, None, None, 0, None, None) == -1 and b"MNET_F16M" in lib.mnet_last_error()
    assert f(None, y, 3, 1, 1, 1, 32, None, None, 0, None, None) == -1              # null pointer
    assert f(z, z, 3, 1, 1, 1, 32, None, None, 0, None, None) == -1                 # in place
    assert f(z, y, 3, 0, 1, 1, 32, None, None, 0, None, None) == -1                 # geometry
    assert f(z, y, 3, 65536, 1, 1, 32, None, None, 0, None, None) == -1             # more images than grid.y takes
    for act in (1, 4, 5, 6):
        assert f(z, y, 3, 1, 1, 1, 32, None, None, act, None, None) == -1           # activation outside NONE / LRELU / LRELU_SQRT2
    assert f(z, y, 3, 1, 1, 1, 24, None, None, 0, None, None) == -2                 # c % 32
    assert f(ctypes.c_void_p(a + 16), y, 3, 1, 1, 1, 32, None, None, 0, None, None) == -2      # z: 128-byte alignment
    assert f(z, ctypes.c_void_p(a + 2048 + 64), 3, 1, 1, 1, 32, None, None, 0, None, None) == -2
    assert f(z, y, 3, 1, 1, 1, 32, None, ctypes.c_void_p(a + 4), 0, None, None) == -2          # vector not 16-byte aligned
    # image too large: w * 9 c >= 2^29; h * w * (c / 8) * 4 >= 2^31 — and the largest maps below each guard pass the checks up to it
    w_big = -(-(1 << 29) // (9 * 32))
    assert f(z, y, 3, 1, 1, w_big, 32, None, None, 0, None, None) == -1 and b"too large" in lib.mnet_last_error()
    assert f(z, y, 3, 1, 32768, 4096, 32, None, None, 0, None, None) == -1 and b"too large" in lib.mnet_last_error()
    assert b"upfold3x3" in lib.mnet_last_error()


HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")
def test_fp32_output_build_isa(tmp_path):
    """conv_dma_w4_f32.hip, as tests/test_isa_hot_path.py checks the production builds of the tile: one kernel, 256 AGPRs, no spilled VGPR, no VALU write of an
    MFMA operand inside its two wait states and no compiler-made accumulator-file move (tools/isa_mfma_hazards.py), no scratch access on the slab loop's hot path
    (tools/isa_hot_scratch.py); and the translation unit has a line of its own in build.sh"""
    asm = str(tmp_path / "conv_dma_w4_f32.s")
    cc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    r = subprocess.run([cc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        os.path.join(ROOT, "marconet_amd", "csrc", "conv_dma_w4_f32.hip"), "-o", asm], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    s = open(asm).read()
    assert re.findall(r"\.name:\s+(_Z\S*conv_dma_w4\S*)", s) == ["_Z22conv_dma_w4_f32_kernelILb0ELb0EEv8ConvArgs"]
    assert len(re.findall(r"\.agpr_count:\s+256", s)) == 1 and re.findall(r"\.vgpr_spill_count:\s+(\d+)", s) == ["0"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_mfma_hazards.py"), asm, "conv_dma_w4_f32_kernel"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count("128 MFMAs checked") == 1 and r.stdout.count(" 0 finding(s)") == 1, r.stdout + r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_hot_scratch.py"), asm, "conv_dma_w4_f32_kernel"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "scratch accesses on the hot path: 0" in r.stdout, r.stdout + r.stderr
    srcs = re.search(r'^SRCS="([^"]*)"', open(os.path.join(ROOT, "marconet_amd", "csrc", "build.sh")).read(), flags=re.M).group(1).split()
    assert "conv_dma_w4_f32" in srcs and "conv_dma_w4" in srcs and "conv_dma_w4_shuf" in srcs
