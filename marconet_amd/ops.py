"""Tensor-level wrappers over the C-ABI.  PyTorch is plumbing only: it owns the device memory
(caching allocator) and the current HIP stream; every arithmetic op below is a hand-written gfx950 kernel.

Activations are NHWC torch tensors of shape [N,H,W,C] and dtype float32, float16 or — the split-half storage of the fp16x3
mode (MNET_F16X2) — packing.SPLIT_DTYPE (a 4-byte tag: a (hi, lo) pair of halves per logical element, C % 32 == 0).
"""
import ctypes
import functools
import os

import numpy as np
import torch

from . import _lib
from ._lib import (ACT_GELU, ACT_LRELU, ACT_LRELU_SQRT2, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, MNET_F16,
                   MNET_F16M, MNET_F16X2, MNET_F32, ConvDesc)
from .packing import MX_DTYPE, SPLIT_DTYPE, is_split, mx_weight_rows, new_tensor, tag, untag

__all__ = ["conv2d", "linear", "nchw_to_nhwc", "nhwc_to_nchw", "upsample2x", "affine_act", "groupnorm_affine",
           "adain_crop_concat", "adain_crop_concat_gn", "glyph_scatter_affine", "layernorm", "token_mix", "attention", "pixelnorm",
           "embed_gather", "demod", "argmax_rows", "convert", "fused_bias_act", "sr_postprocess", "lq_from_u8", "lq_windows_u8", "row_ink_u8", "box_ink_u8", "skew_ink_u8", "panel_u8", "paste_u8", "quad_crop_u8", "quad_paste_u8", "curve_crop_u8", "curve_paste_u8", "paste_ordered_u8", "conv3x3_rgb", "torgb", "stats",
           "pack_weights", "pack_wsq", "gather_rows", "style_rows", "nonfinite_flag", "compare_stats", "gn_partial_buffer", "can_emit_gn_partial", "groupnorm_affine_from_partial",
           "polyphase_plan", "upconv3x3_polyphase", "polyphase_ring_fix", "groupnorm_affine_from_partial_ring", "upfold_plan", "upfold3x3",
           "ACT_NONE", "ACT_RELU", "ACT_LRELU", "ACT_LRELU_SQRT2", "ACT_TANH", "ACT_GELU", "ACT_SIGMOID"]


def _plumbing(fn):
    """kernel wrappers read shapes / dtypes / pointers of blocked-storage tensors many times per launch: inside a wrapper the
    BlockedTensor guard (packing.BlockedTensor.__torch_function__, ~2.5 us per access) is switched off; outputs are tagged again"""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        with torch._C.DisableTorchFunctionSubclass():
            return fn(*args, **kwargs)
    return wrapper


def _dt(t):
    if t.dtype == torch.float32:
        return MNET_F32
    if t.dtype == torch.float16:
        return MNET_F16
    if t.dtype == SPLIT_DTYPE:          # split half (fp16x3 mode): (hi, lo) per logical element, tagged as complex32
        return MNET_F16X2
    if t.dtype == MX_DTYPE:             # fp16+8 (fp16x2 mode): hi half + e4m3 lo byte + block scale, tagged as uint32
        return MNET_F16M
    raise TypeError("marconet_amd: unsupported dtype %s" % t.dtype)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _addr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_cuda(*ts):
    """every tensor of a launch must be contiguous and live on the CURRENT HIP device: the C side launches on the current
    device, on that device's current stream (the module forwards enter ``torch.cuda.device(input.device)`` first)"""
    cur = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("marconet_amd: tensors must live on a HIP device (got %s); there is no CPU path" % t.device)
        if cur is None:
            cur = torch.cuda.current_device()
        if t.device.index != cur:
            raise RuntimeError("marconet_amd: tensor on %s but the current device is cuda:%d — enter torch.cuda.device(...) "
                               "(the nn.Module forwards and MarconetPipeline do)" % (t.device, cur))
        if not t.is_contiguous():
            raise RuntimeError("marconet_amd: non-contiguous tensor passed to a kernel wrapper")


def _raw(t):
    """split-half tensors are moved by PyTorch as plain halves (twice the channels): cat / index_select over the outer dimension
    never depend on the (experimental) complex32 support of an operator"""
    return untag(t).view(torch.float16) if is_split(t.dtype) else t


@_plumbing
def cat_rows(parts):
    """concatenation of NHWC tensors along dim 0 (any storage dtype)"""
    if len(parts) == 1:
        return parts[0]
    out = torch.cat([_raw(p) for p in parts], dim=0)
    return tag(out.view(parts[0].dtype)) if is_split(parts[0].dtype) else out


@_plumbing
def take_rows(t, idx):
    """t[idx] along dim 0 (any storage dtype)"""
    out = _raw(t).index_select(0, idx)
    return tag(out.view(t.dtype)) if is_split(t.dtype) else out


def on_device(t):
    """context manager: the HIP device of ``t`` becomes the current device (launches and the stream lookup follow the current
    device); a CPU tensor raises — there is no CPU path"""
    if not t.is_cuda:
        raise RuntimeError("marconet_amd: tensors must live on a HIP device (got %s); there is no CPU path" % t.device)
    return torch.cuda.device(t.device)


class _Stats:
    """Optional accounting for bench.py: algorithmic FLOPs and per-launch HIP-event timing of the conv kernel."""

    def __init__(self):
        self.enabled = False
        self.timing = False
        self.reset()

    def reset(self):
        self.conv_flops = 0.0
        self.conv_launches = 0
        self.events = []       # (start, end, flops, dtype, kernel id from mnet_conv2d_plan)
        self.tail_events = []  # HBM-bound kernels: (start, end, algorithmic bytes — every tensor of the launch once —, name)

    def conv_time_ms(self):
        return sum(ev[0].elapsed_time(ev[1]) for ev in self.events)

    def tail(self, name, tensors, launch):
        """run ``launch()``; in an instrumented pass (bench.py's roofline pass) bracket it with HIP events on the launch stream and
        book the storage bytes of ``tensors`` (inputs and outputs, each once) under ``name``"""
        if not (self.enabled and self.timing):
            return launch()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        r = launch()
        e.record()
        self.tail_events.append((s, e, float(sum(t.numel() * t.element_size() for t in tensors if t is not None)), name))
        return r


stats = _Stats()


def _out_size(h, w, kh, kw, stride, pad):
    return (h + 2 * pad[0] - kh) // stride[0] + 1, (w + 2 * pad[1] - kw) // stride[1] + 1


def _conv_desc(x0, x1, cout, kh, kw, stride, pad, wgt, y, in_scale=None, in_shift=None, in_swish=False, valid_w=None, out_scale=None,
               bias=None, residual=None, res_mod=0, act=ACT_NONE, post_scale=None, gn_partial=None):
    """mnet_conv_desc of ``conv2d(x0, …)`` (and of ``conv_plan``'s question about it): the sources as tensors, every other buffer as a
    device address or None"""
    n, h, w, c0 = x0.shape
    d = ConvDesc()
    d.dtype = _dt(x0)
    d.x0, d.c0 = x0.data_ptr(), c0
    d.x1, d.c1 = (None, 0) if x1 is None else (x1.data_ptr(), x1.shape[3])
    d.n, d.h, d.w = n, h, w
    d.wgt = wgt
    d.cout, d.kh, d.kw = cout, kh, kw
    d.stride_h, d.stride_w, d.pad_h, d.pad_w = stride[0], stride[1], pad[0], pad[1]
    d.ho, d.wo = _out_size(h, w, kh, kw, stride, pad)
    d.in_scale, d.in_shift, d.in_swish = in_scale, in_shift, 1 if in_swish else 0
    d.valid_w = valid_w
    d.out_scale, d.bias, d.residual, d.res_mod = out_scale, bias, residual, res_mod
    d.act = act
    d.post_scale = post_scale
    d.y = y
    d.gn_partial = gn_partial
    return d


@_plumbing
def conv2d(x0, wgt, cout, kh=1, kw=1, stride=(1, 1), pad=(0, 0), x1=None, in_scale=None, in_shift=None,
           in_swish=False, valid_w=None, out_scale=None, bias=None, residual=None, res_mod=0, act=ACT_NONE,
           post_scale=None, out=None, algo=0, splitk=0, x1_center=False, gn_partial=None, shuffle2=False, out_f32=False):
    """mnet_conv2d_nhwc(_ex).  x0 [N,H,W,C0] (+ optional x1 [N,H,W,C1]); wgt packed [cout,kh,kw,C0+C1] same dtype.
    ``splitk`` > 0: mnet_conv2d_splitk with that many K-slices (fp32 filter == stride convs over <= 512 output pixels).
    ``x1_center``: x1 enters through the filter's centre tap only (MNET_CONV_ALGO_FLAG_X1_CENTER: a 1x1 skip conv as extra K).
    ``gn_partial``: fp32 [n*ho*wo/32, cout/32, 2] buffer (``gn_partial_buffer``) the epilogue fills with the GroupNorm partial sums of the output
    (fp16+8 launches on the LDS-DMA / strip kernels only: MarconetHipError otherwise, nothing enqueued).
    ``shuffle2``: MNET_CONV_ALGO_FLAG_SHUFFLE2 — ``cout`` = 4 C phase-major and the output is the [N,2H,2W,C] tensor (see ``upconv3x3_polyphase``).
    ``out_f32``: MNET_CONV_ALGO_FLAG_F32_OUT — an fp16+8 launch whose output is a plain fp32 tensor (the value before the storage's rounding; plain epilogue,
    one-wave tile only: MarconetHipError otherwise, nothing enqueued)."""
    lib = _lib.load()
    _need_cuda(x0, x1, wgt, in_scale, in_shift, valid_w, out_scale, bias, residual, post_scale, out)
    n, h, w, c0 = x0.shape
    c1 = 0 if x1 is None else x1.shape[3]
    need = cout * kh * kw * (c0 + c1)
    if x0.dtype == MX_DTYPE:            # + the per-output-channel scale bytes behind the weight rows
        need = mx_weight_rows(cout, kh, kw, c0 + c1) * kh * kw * (c0 + c1)
    if wgt.dtype != x0.dtype or wgt.numel() != need:
        raise RuntimeError("conv2d: weight dtype/shape mismatch (%s %s vs cout=%d k=%dx%d cin=%d)"
                           % (wgt.dtype, tuple(wgt.shape), cout, kh, kw, c0 + c1))
    ho, wo = _out_size(h, w, kh, kw, stride, pad)
    oshape = (n, 2 * ho, 2 * wo, cout // 4) if shuffle2 else (n, ho, wo, cout)
    if shuffle2:
        algo |= _lib.ALGO_FLAG_SHUFFLE2
    if out_f32:
        algo |= _lib.ALGO_FLAG_F32_OUT
    odtype = torch.float32 if out_f32 else x0.dtype
    if out is None:
        out = new_tensor(oshape, odtype, x0.device)
    elif tuple(out.shape) != oshape or out.dtype != odtype:
        raise RuntimeError("conv2d: out is %s %s, expected %s %s" % (tuple(out.shape), out.dtype, oshape, odtype))
    if gn_partial is not None:
        _need_cuda(gn_partial)
        if gn_partial.dtype != torch.float32 or gn_partial.numel() != (n * ho * wo // 32) * (cout // 32) * 2:
            raise RuntimeError("conv2d: gn_partial must be fp32 [n*ho*wo/32, cout/32, 2]")
    d = _conv_desc(x0, x1, cout, kh, kw, stride, pad, wgt=wgt.data_ptr(), y=out.data_ptr(), in_scale=_addr(in_scale), in_shift=_addr(in_shift),
                   in_swish=in_swish, valid_w=_addr(valid_w), out_scale=_addr(out_scale), bias=_addr(bias), residual=_addr(residual),
                   res_mod=res_mod, act=act, post_scale=_addr(post_scale), gn_partial=_addr(gn_partial))
    for t, nm in ((in_scale, "in_scale"), (in_shift, "in_shift"), (out_scale, "out_scale"), (bias, "bias"),
                  (post_scale, "post_scale")):
        if t is not None and t.dtype != torch.float32:
            raise TypeError("conv2d: %s must be float32" % nm)
    if valid_w is not None and valid_w.dtype != torch.int32:
        raise TypeError("conv2d: valid_w must be int32")
    if residual is not None and residual.dtype != x0.dtype:
        raise TypeError("conv2d: residual dtype mismatch")
    if x1_center:
        if x1 is None:
            raise RuntimeError("conv2d: x1_center needs x1")
        algo |= _lib.ALGO_FLAG_X1_CENTER
    if splitk:
        ws = torch.empty((splitk * n * ho * wo * cout,), dtype=torch.float32, device=x0.device)
        if stats.enabled:
            stats.conv_flops += lib.mnet_conv2d_flops(ctypes.byref(d))
            stats.conv_launches += 1
        _lib.check(lib.mnet_conv2d_splitk(ctypes.byref(d), splitk, _p(ws), _stream()), "mnet_conv2d_splitk")
        return out
    if stats.enabled:
        fl = lib.mnet_conv2d_flops(ctypes.byref(d))
        if x1_center:                       # the second source is multiplied at one tap, not kh * kw
            fl -= 2.0 * n * ho * wo * cout * (kh * kw - 1) * c1
        stats.conv_flops += fl
        stats.conv_launches += 1
        if stats.timing:
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            s.record()
            _lib.check(lib.mnet_conv2d_nhwc_ex(ctypes.byref(d), algo, _stream()), "mnet_conv2d_nhwc")
            e.record()
            stats.events.append((s, e, fl, d.dtype, lib.mnet_conv2d_plan(ctypes.byref(d), algo)))
            return out
    _lib.check(lib.mnet_conv2d_nhwc_ex(ctypes.byref(d), algo, _stream()), "mnet_conv2d_nhwc")
    return out


def linear(x, wgt, out_features, bias=None, act=ACT_NONE, residual=None, res_mod=0):
    """nn.Linear as a 1x1 conv over a [1,1,M,K] map: x [M,K] → [M,out_features]."""
    m, k = x.shape
    r = None if residual is None else residual.reshape(1, 1, -1, out_features)
    y = conv2d(x.reshape(1, 1, m, k), wgt, out_features, bias=bias, act=act, residual=r, res_mod=res_mod)
    return y.reshape(m, out_features)


@_plumbing
def nchw_to_nhwc(src, dtype, c_ld=None):
    lib = _lib.load()
    _need_cuda(src)
    if src.dtype != torch.float32:
        raise TypeError("nchw_to_nhwc: fp32 NCHW input expected (the reference's tensors are fp32)")
    n, c, h, w = src.shape
    c_ld = c_ld or c
    dst = new_tensor((n, h, w, c_ld), dtype, src.device)
    stats.tail("layout", (src, dst), lambda: _lib.check(lib.mnet_nchw_to_nhwc(_p(src), _p(dst), _dt(dst), n, c, h, w, c_ld, _stream()), "mnet_nchw_to_nhwc"))
    return dst


@_plumbing
def nhwc_to_nchw(src, c=None):
    lib = _lib.load()
    _need_cuda(src)
    n, h, w, c_ld = src.shape
    c = c or c_ld
    dst = torch.empty((n, c, h, w), dtype=torch.float32, device=src.device)
    stats.tail("layout", (src, dst), lambda: _lib.check(lib.mnet_nhwc_to_nchw(_p(src), _dt(src), _p(dst), n, c, h, w, c_ld, _stream()), "mnet_nhwc_to_nchw"))
    return dst


@_plumbing
def upsample2x(src, scale=None, out_dtype=None):
    """bilinear x2 (align_corners=False); optional per-(n,c) fp32 multiplier fused into the store; ``out_dtype``: torch.float16 for a
    split-half / fp16+8 source (the conversion rides in the store: no separate convert pass), default the source's storage type"""
    lib = _lib.load()
    _need_cuda(src, scale)
    n, h, w, c = src.shape
    dst = new_tensor((n, 2 * h, 2 * w, c), out_dtype or src.dtype, src.device)
    stats.tail("upsample2x", (src, dst), lambda: _lib.check(lib.mnet_upsample2x_convert_nhwc(_p(src), _dt(src), _p(dst), _dt(dst), n, h, w, c, _p(scale), _stream()),
                                                            "mnet_upsample2x_convert_nhwc"))
    return dst


@_plumbing
def affine_act(x, scale, shift=None, swish=False, out=None):
    """y = f(x*scale[n,c] + shift[n,c]) elementwise over NHWC x [N,H,W,C] (GroupNorm apply + swish)."""
    lib = _lib.load()
    _need_cuda(x, scale, shift, out)
    n, h, w, c = x.shape
    y = tag(torch.empty_like(x)) if out is None else out
    stats.tail("groupnorm_apply", (x, y), lambda: _lib.check(lib.mnet_affine_act_nhwc(_p(x), _p(y), _dt(x), n, h * w, c, _p(scale), _p(shift), 1 if swish else 0,
                                                                                   _stream()), "mnet_affine_act_nhwc"))
    return y


@_plumbing
def groupnorm_affine(x, gamma, beta, eps=1e-6, valid_w=None):
    """→ (scale [N,C], shift [N,C]) fp32 for conv2d(in_scale=, in_shift=, in_swish=True)."""
    lib = _lib.load()
    _need_cuda(x, gamma, beta, valid_w)
    n, h, w, c = x.shape
    slices = max(1, min(128, (h * w) // 512))      # a function of the map size only: the fp64 fold order never depends on the batch
    partial = torch.empty((n * slices * (c // 32) * 2,), dtype=torch.float64, device=x.device)
    scale = torch.empty((n, c), dtype=torch.float32, device=x.device)
    shift = torch.empty((n, c), dtype=torch.float32, device=x.device)
    stats.tail("groupnorm_stats", (x,), lambda: _lib.check(lib.mnet_groupnorm_affine(_p(x), _dt(x), n, h, w, c, _p(valid_w), _p(gamma), _p(beta), eps,
                                                                                  _p(partial), slices, _p(scale), _p(shift), _stream()), "mnet_groupnorm_affine"))
    return scale, shift


def gn_partial_buffer(n, h, w, c, device):
    """buffer for conv2d(gn_partial=...): per (32-pixel fragment, 32-channel group) sum and sum of squares of the conv's output"""
    return torch.empty((n * h * w // 32, c // 32, 2), dtype=torch.float32, device=device)


_PLAN_CACHE = {}
_PLAN_ADDR = 1 << 20      # a buffer the launch will pass but the question has not allocated: the planner checks its presence and alignment, never what is behind it


def _align(t):
    """the alignment of a source that the planner's answer can depend on (16 / 128 bytes)"""
    return None if t is None else (128 if t.data_ptr() % 128 == 0 else 16 if t.data_ptr() % 16 == 0 else 0)


def conv_plan(x0, cout, kh=1, kw=1, stride=(1, 1), pad=(0, 0), x1=None, act=ACT_NONE, in_scale=False, residual=False, out_scale=False,
              gn_partial=False, x1_center=False, algo=0):
    """mnet_conv2d_plan for ``conv2d(x0, …, x1=…, act=…)``: the kernel ``algo`` resolves to (_lib.ALGO_REG_STAGED, ALGO_SKINNY, ALGO_DMA_CFG0 + id,
    ALGO_STRIP_CFG0 + id, ALGO_DMA_CFG16 + id), or a negative MNET_E_* when the planner refuses it.  The flags say which of in_scale, residual,
    out_scale / post_scale and gn_partial the launch will pass, and whether it sets x1_center.  Nothing is launched; the callers that choose
    between two forms of a layer ask this instead of launching and parsing an error message.  Accepted answers are cached per everything they
    depend on (storage type, shape, filter, flags, algo and the alignment of x0 / x1); refusals are not."""
    n, h, w, c0 = x0.shape
    if x1_center:
        algo |= _lib.ALGO_FLAG_X1_CENTER
    key = (_dt(x0), n, h, w, c0, None if x1 is None else x1.shape[3], _align(x0), _align(x1), cout, kh, kw, tuple(stride), tuple(pad), act,
           bool(in_scale), bool(residual), bool(out_scale), bool(gn_partial), algo)
    k = _PLAN_CACHE.get(key)
    if k is None:
        addr = [_PLAN_ADDR if present else None for present in (in_scale, residual, out_scale, gn_partial)]
        d = _conv_desc(x0, x1, cout, kh, kw, stride, pad, wgt=_PLAN_ADDR, y=_PLAN_ADDR, in_scale=addr[0], residual=addr[1], out_scale=addr[2],
                       act=act, gn_partial=addr[3])
        k = int(_lib.load().mnet_conv2d_plan(ctypes.byref(d), algo))
        if k >= 0:
            _PLAN_CACHE[key] = k
    return k


def polyphase_plan(x, c, act=ACT_NONE, gn_partial=True, algo=0):
    """the planner's answer for the main launch of ``upconv3x3_polyphase(x, …)`` with ``c`` output channels (negative: refused — the caller keeps
    the two-launch form).  It depends on the per-image map shape, the channel counts and the storage type, never on the batch."""
    if x.dtype != MX_DTYPE:
        return -1
    return conv_plan(x, 4 * c, 3, 3, (1, 1), (1, 1), act=act, gn_partial=gn_partial, algo=algo | _lib.ALGO_FLAG_SHUFFLE2)


@_plumbing
def polyphase_ring_fix(top, bottom, left, right, y):
    """mnet_polyphase_ring_fix: hi-res rows / columns {0, 1, last two} of ``y`` [N,2H,2W,C] from the strips' two-launch results (top / bottom [N,4,2W,C],
    left / right [N,2H,4,C]) → fp64 [N, C/32, 2] sums of the stored ring values"""
    lib = _lib.load()
    _need_cuda(top, bottom, left, right, y)
    n, h2, w2, c = y.shape
    if tuple(top.shape) != (n, 4, w2, c) or tuple(bottom.shape) != (n, 4, w2, c) or tuple(left.shape) != (n, h2, 4, c) or tuple(right.shape) != (n, h2, 4, c):
        raise RuntimeError("polyphase_ring_fix: strips %s %s %s %s do not fit y %s" % (tuple(top.shape), tuple(bottom.shape), tuple(left.shape), tuple(right.shape), tuple(y.shape)))
    sums = torch.empty((n, c // 32, 2), dtype=torch.float64, device=y.device)
    # (bytes: half of every strip is read, as much of y written)
    stats.tail("polyphase_ring", (top, left, top, left), lambda: _lib.check(lib.mnet_polyphase_ring_fix(_p(top), _p(bottom), _p(left), _p(right), _p(y), _dt(y), n, h2, w2, c,
                                                                                                      _p(sums), _stream()), "mnet_polyphase_ring_fix"))
    return sums


def groupnorm_affine_from_partial_ring(partial, ring_sums, n, h, w, c, gamma, beta, eps=1e-6):
    """``groupnorm_affine_from_partial`` for a polyphase conv's output [n,h,w,c] (hi-res): masked partial sums + the ring's sums"""
    lib = _lib.load()
    _need_cuda(partial, ring_sums, gamma, beta)
    scale = torch.empty((n, c), dtype=torch.float32, device=partial.device)
    shift = torch.empty((n, c), dtype=torch.float32, device=partial.device)
    _lib.check(lib.mnet_groupnorm_affine_from_partial_ring(_p(partial), _p(ring_sums), n, h, w, c, _p(gamma), _p(beta), eps, _p(scale), _p(shift), _stream()),
               "mnet_groupnorm_affine_from_partial_ring")
    return scale, shift


@_plumbing
def _strip_pair(x, dim):
    """the first two and the last two rows (dim 1) / columns (dim 2) of NHWC ``x``, stacked along the batch: [2N,2,W,C] / [2N,H,2,C]"""
    r = _raw(x)
    k = r.shape[dim]
    out = torch.cat([r.narrow(dim, 0, 2), r.narrow(dim, k - 2, 2)], dim=0)
    return tag(out.view(x.dtype)) if is_split(x.dtype) else out


def upconv3x3_polyphase(x, wgt_poly, bias_poly, wgt, bias, c, act=ACT_NONE, algo=0, out=None):
    """conv3x3(bilinear_x2(x)) + bias + act without the up-sampled tensor: ONE conv on the low-res map with the four phases' combined weights
    (``wgt_poly`` [4c,3,3,cin], ``bias_poly`` [4c]: packing.polyphase_conv_weight) stored pixel-shuffled, then the hi-res ring — rows and columns
    {0, 1, last two}, where clamping the up-sample differs from zero-padding its phases — from the two-launch form on four thin strips with the
    ordinary ``wgt`` / ``bias``.  → (y [N,2H,2W,c], partial, ring_sums) for ``groupnorm_affine_from_partial_ring``.  The caller has asked
    ``polyphase_plan``; ``algo`` pins the main launch's tile."""
    n, h, w, _ = x.shape
    part = gn_partial_buffer(n, h, w, 4 * c, x.device)
    y = conv2d(x, wgt_poly, 4 * c, 3, 3, (1, 1), (1, 1), bias=bias_poly, act=act, gn_partial=part, algo=algo, shuffle2=True, out=out)
    tb = conv2d(upsample2x(_strip_pair(x, 1)), wgt, c, 3, 3, (1, 1), (1, 1), bias=bias, act=act)        # [2N,4,2W,c]
    lr = conv2d(upsample2x(_strip_pair(x, 2)), wgt, c, 3, 3, (1, 1), (1, 1), bias=bias, act=act)        # [2N,2H,4,c]
    return y, part, polyphase_ring_fix(tb[:n], tb[n:], lr[:n], lr[n:], y)


# Up-convs that take the tap-conv + fold form: (cin, cout) → the smallest low-res map height accepted.  The generator's 16→32 (512→512) and 32→64 (512→256)
# levels — the ones that measured faster than up-sample + conv (profiles/upfold_ab.txt); 4→8 and 8→16 (512→512 on smaller maps) keep the old form.
# A table of per-glyph shapes: the form of a layer never depends on the batch.
UPFOLD_LEVELS = {(512, 512): 16, (512, 256): 16}


def upfold_plan(x, cout, levels=None, out_f32=False):
    """the planner's answer for the 1x1 launch of the tap-conv form of conv3x3(bilinear_x2(x)) with ``cout`` output channels (``conv2d(x, w_tap, 9·cout)``,
    then ``upfold3x3``), or a negative value — the caller keeps up-sample + conv.  fp16+8 storage only, the levels of ``UPFOLD_LEVELS`` (``levels``: another
    table), and only when the planner hands the launch to an LDS-DMA tile.  It depends on the per-glyph map shape, the channel counts and the storage type,
    never on the batch.  ``out_f32``: the question about the launch that writes the tap planes in fp32 (``conv2d(..., out_f32=True)``, folded by ``upfold3x3``
    with ``out_dtype=MX_DTYPE``) — accepted only where it resolves to the one-wave tile."""
    if x.dtype != MX_DTYPE:
        return -1
    _, h, _, cin = x.shape
    min_h = (UPFOLD_LEVELS if levels is None else levels).get((cin, cout))
    if min_h is None or h < min_h:
        return -1
    k = conv_plan(x, 9 * cout, 1, 1, algo=_lib.ALGO_FLAG_F32_OUT if out_f32 else 0)
    return k if k >= 0 and plan_is_lds_dma(k) else -1


@_plumbing
def upfold3x3(z, c, out_scale=None, bias=None, act=ACT_NONE, post_scale=None, out=None, out_dtype=None):
    """mnet_upfold3x3_nhwc: ``z`` [N,h,w,9·c] (tap-major: channel t·c + o, t = 3·ky + kx; the 1x1 conv of the low-res map with packing.pack_tapconv_weight) →
    y [N,2h,2w,c] = post_scale · act(out_scale · Σ_t (bilinear_x2 z_t) shifted by tap t + bias): conv3x3(bilinear_x2(x)) with the conv epilogue's contract,
    without the up-sampled tensor.  y has z's storage, except that fp32 ``z`` (``conv2d(..., out_f32=True)``) folds into an fp16+8 y when ``out`` is one or
    ``out_dtype`` says so (mnet_upfold3x3_f32z_nhwc)"""
    lib = _lib.load()
    _need_cuda(z, out_scale, bias, post_scale, out)
    ydtype = out.dtype if out is not None and out_dtype is None else (z.dtype if out_dtype is None else out_dtype)
    if ydtype != z.dtype and not (z.dtype == torch.float32 and ydtype == MX_DTYPE):
        raise RuntimeError("upfold3x3: z is %s and y %s — y has z's storage, or z is float32 and y fp16+8" % (z.dtype, ydtype))
    n, h, w, c9 = z.shape
    if c9 != 9 * c:
        raise RuntimeError("upfold3x3: z has %d channels, expected 9 x %d" % (c9, c))
    for t, nm in ((out_scale, "out_scale"), (bias, "bias"), (post_scale, "post_scale")):
        if t is not None and t.dtype != torch.float32:
            raise TypeError("upfold3x3: %s must be float32" % nm)
    oshape = (n, 2 * h, 2 * w, c)
    if out is None:
        out = new_tensor(oshape, ydtype, z.device)
    elif tuple(out.shape) != oshape or out.dtype != ydtype:
        raise RuntimeError("upfold3x3: out is %s %s, expected %s %s" % (tuple(out.shape), out.dtype, oshape, ydtype))
    if ydtype != z.dtype:
        stats.tail("upfold", (z, out), lambda: _lib.check(lib.mnet_upfold3x3_f32z_nhwc(_p(z), _p(out), _dt(out), n, h, w, c, _p(out_scale), _p(bias), act,
                                                                                      _p(post_scale), _stream()), "mnet_upfold3x3_f32z_nhwc"))
        return out
    stats.tail("upfold", (z, out), lambda: _lib.check(lib.mnet_upfold3x3_nhwc(_p(z), _p(out), _dt(z), n, h, w, c, _p(out_scale), _p(bias), act, _p(post_scale),
                                                                             _stream()), "mnet_upfold3x3_nhwc"))
    return out


def plan_is_lds_dma(k):
    """a planner answer that names one of the LDS-DMA tile configurations (not the strip kernel, not the register-staged / skinny ones)"""
    return _lib.ALGO_DMA_CFG0 <= k < _lib.ALGO_STRIP_CFG0 or k >= _lib.ALGO_DMA_CFG16


def can_emit_gn_partial(x0, x1, cout, stride, ho, wo, act=ACT_NONE):
    """the launches whose epilogue can write GroupNorm partial sums (mnet_conv_desc.gn_partial): fp16+8 storage, and a launch with gn_partial the
    planner accepts (it gives those to the LDS-DMA / strip kernels; 3x3 'same' geometry of this network's GroupNorm producers)"""
    c = x0.shape[3] + (0 if x1 is None else x1.shape[3])
    if not (x0.dtype == MX_DTYPE and tuple(stride) == (1, 1) and cout >= 64 and cout % 32 == 0 and c % 32 == 0 and x0.shape[3] % 32 == 0
            and (ho * wo) % 32 == 0 and not _NO_EPILOGUE_GN):
        return False
    return conv_plan(x0, cout, 3, 3, stride, (1, 1), x1=x1, act=act, gn_partial=True) >= _lib.ALGO_DMA_CFG0


def groupnorm_affine_from_partial(partial, n, h, w, c, gamma, beta, eps=1e-6, valid_w=None):
    """→ (scale [N,C], shift [N,C]) fp32 from the partial sums a conv epilogue wrote (no pass over the map)"""
    lib = _lib.load()
    _need_cuda(partial, gamma, beta, valid_w)
    scale = torch.empty((n, c), dtype=torch.float32, device=partial.device)
    shift = torch.empty((n, c), dtype=torch.float32, device=partial.device)
    _lib.check(lib.mnet_groupnorm_affine_from_partial(_p(partial), n, h, w, c, _p(valid_w), _p(gamma), _p(beta), eps, _p(scale), _p(shift), _stream()),
               "mnet_groupnorm_affine_from_partial")
    return scale, shift


@_plumbing
def adain_crop_concat(prior, feat, g_img, g_x1, g_y1, g_w):
    lib = _lib.load()
    _need_cuda(prior, feat, g_img, g_x1, g_y1, g_w)
    G, S, S2, C = prior.shape
    B, FH, FW, FC = feat.shape
    if S != S2 or FH != S or FC != C or prior.dtype != feat.dtype:
        raise RuntimeError("adain_crop_concat: shape mismatch prior %s feat %s" % (tuple(prior.shape), tuple(feat.shape)))
    out = new_tensor((G, S, S, 2 * C), prior.dtype, prior.device)
    _lib.check(lib.mnet_adain_crop_concat(_p(prior), _p(feat), _p(out), _dt(prior), G, S, C, FW, _p(g_img), _p(g_x1),
                                          _p(g_y1), _p(g_w), _stream()), "mnet_adain_crop_concat")
    return out


_NO_EPILOGUE_GN = os.environ.get("MNET_NO_EPILOGUE_GN", "0") == "1"      # A/B knob: GroupNorm statistics by their own pass over the map (round 4)
ADAIN_SPLIT_BELOW = 256      # glyphs per launch below which the three-launch (16 workgroups per glyph) form is used
_ADAIN_SPLIT = {"0": False, "1": True}.get(os.environ.get("MNET_ADAIN_SPLIT", ""))     # A/B knob


@_plumbing
def adain_crop_concat_gn(prior, feat, g_img, g_x1, g_y1, g_w, gamma, beta, eps=1e-6, split=None):
    """adain_crop_concat + the GroupNorm affine of its output (closed form from the AdaIN statistics) → (out, scale, shift).
    ``split``: None = by glyph count; the two forms agree up to the association of the fp64 statistic sums."""
    lib = _lib.load()
    _need_cuda(prior, feat, g_img, g_x1, g_y1, g_w, gamma, beta)
    G, S, S2, C = prior.shape
    B, FH, FW, FC = feat.shape
    if S != S2 or FH != S or FC != C or prior.dtype != feat.dtype or gamma.numel() != 2 * C:
        raise RuntimeError("adain_crop_concat_gn: shape mismatch prior %s feat %s" % (tuple(prior.shape), tuple(feat.shape)))
    out = new_tensor((G, S, S, 2 * C), prior.dtype, prior.device)
    scale = torch.empty((G, 2 * C), dtype=torch.float32, device=prior.device)
    shift = torch.empty((G, 2 * C), dtype=torch.float32, device=prior.device)
    if split is None:
        split = _ADAIN_SPLIT if _ADAIN_SPLIT is not None else G < ADAIN_SPLIT_BELOW
    if split:       # few glyphs (a strip at a time): spread each glyph over 16 workgroups instead of one
        slices = 16
        partial = torch.empty((G * slices * C * 4,), dtype=torch.float64, device=prior.device)
        stat = torch.empty((G, 4, C), dtype=torch.float32, device=prior.device)
        stats.tail("adain", (prior, prior, out), lambda: _lib.check(lib.mnet_adain_crop_concat_split(
            _p(prior), _p(feat), _p(out), _dt(prior), G, S, C, FW, _p(g_img), _p(g_x1), _p(g_y1), _p(g_w), _p(gamma), _p(beta), eps, _p(scale), _p(shift),
            _p(partial), _p(stat), slices, _stream()), "mnet_adain_crop_concat_split"))
        return out, scale, shift
    # bytes: the prior, a window of feat of the prior's size, the concatenated output
    stats.tail("adain", (prior, prior, out), lambda: _lib.check(lib.mnet_adain_crop_concat_gn(
        _p(prior), _p(feat), _p(out), _dt(prior), G, S, C, FW, _p(g_img), _p(g_x1), _p(g_y1), _p(g_w), _p(gamma), _p(beta), eps, _p(scale), _p(shift), _stream()),
        "mnet_adain_crop_concat_gn"))
    return out, scale, shift


@_plumbing
def glyph_scatter_affine(feat, scale, shift, g_start, g_x1, g_w):
    lib = _lib.load()
    _need_cuda(feat, scale, shift, g_start, g_x1, g_w)
    B, S, FW, C = feat.shape
    out = tag(torch.empty_like(feat))
    stats.tail("glyph_scatter", (feat, scale, shift, out), lambda: _lib.check(lib.mnet_glyph_scatter_affine(
        _p(feat), _p(scale), _p(shift), _p(out), _dt(feat), B, S, C, FW, _p(g_start), _p(g_x1), _p(g_w), _stream()), "mnet_glyph_scatter_affine"))
    return out


def layernorm(x, gamma, beta, eps=1e-5):
    lib = _lib.load()
    _need_cuda(x, gamma, beta)
    rows, d = x.shape
    y = tag(torch.empty_like(x))
    _lib.check(lib.mnet_layernorm(_p(x), _p(gamma), _p(beta), _p(y), rows, d, eps, _stream()), "mnet_layernorm")
    return y


def token_mix(x, ln_g, ln_b, wgt, bias, eps=1e-5):
    lib = _lib.load()
    _need_cuda(x, ln_g, ln_b, wgt, bias)
    B, T, D = x.shape
    J = wgt.shape[0]
    y = torch.empty((B, J, D), dtype=torch.float32, device=x.device)
    _lib.check(lib.mnet_token_mix(_p(x), _p(ln_g), _p(ln_b), _p(wgt), _p(bias), _p(y), B, T, D, J, eps, _stream()),
               "mnet_token_mix")
    return y


def attention(qkv, B, N, H, scale):
    lib = _lib.load()
    _need_cuda(qkv)
    out = torch.empty((B * N, H * 64), dtype=torch.float32, device=qkv.device)
    _lib.check(lib.mnet_attention(_p(qkv), _p(out), B, N, H, scale, _stream()), "mnet_attention")
    return out


def pixelnorm(x):
    lib = _lib.load()
    _need_cuda(x)
    y = tag(torch.empty_like(x))
    _lib.check(lib.mnet_pixelnorm(_p(x), _p(y), x.shape[0], x.shape[1], _stream()), "mnet_pixelnorm")
    return y


@_plumbing
def embed_gather(emb, labels, dtype, num_classes, scale=None):
    """SelectText gather; ``scale`` (fp32 [N, C], optional): per-(sample, channel) factor applied before the storage rounding"""
    lib = _lib.load()
    _need_cuda(emb, labels, scale)
    N, nc = labels.shape
    C = emb.shape[1]
    if scale is not None and (tuple(scale.shape) != (N, C) or scale.dtype != torch.float32 or not scale.is_contiguous()):
        raise ValueError("embed_gather: scale must be a contiguous fp32 [N, C] tensor")
    out = new_tensor((N, 4, 4 * nc, C), dtype, emb.device)
    _lib.check(lib.mnet_embed_gather_scaled(_p(emb), _p(labels), _p(scale), _p(out), _dt(out), N, nc, C, num_classes, _stream()),
               "mnet_embed_gather_scaled")
    return out


def demod(style, wsq_t, eps_scale=None):
    """rsqrt(Σ_i style² wsq_t + 1e-8·eps_scale[n]) — eps_scale (fp32 [N], 4^-e) for rows normalised by ``style_rows``"""
    lib = _lib.load()
    _need_cuda(style, wsq_t, eps_scale)
    N, cin = style.shape
    cout = wsq_t.shape[1]
    out = torch.empty((N, cout), dtype=torch.float32, device=style.device)
    _lib.check(lib.mnet_demod_scaled(_p(style), _p(wsq_t), _p(out), N, cin, cout, _p(eps_scale), _stream()), "mnet_demod_scaled")
    return out


def style_rows(src, col0, ncols, idx=None, bcast=0):
    """mnet_style_rows: window + row gather of the modulation GEMM's output with every row divided by 2^e (largest magnitude in
    [0.5, 1)) → (rows [R,ncols], eps_scale [R] = 4^-e, scale_b [R,bcast] = 2^e or None)"""
    lib = _lib.load()
    _need_cuda(src, idx)
    if src.dtype != torch.float32 or src.dim() != 2 or (idx is not None and idx.dtype != torch.int64):
        raise TypeError("style_rows: fp32 [rows, ld] source and int64 indices expected")
    rows = src.shape[0] if idx is None else idx.shape[0]
    dst = torch.empty((rows, ncols), dtype=torch.float32, device=src.device)
    eps = torch.empty((rows,), dtype=torch.float32, device=src.device)
    sb = torch.empty((rows, bcast), dtype=torch.float32, device=src.device) if bcast else None
    if rows:
        _lib.check(lib.mnet_style_rows(_p(src), src.shape[0], src.shape[1], col0, ncols, _p(idx), rows, _p(dst), _p(eps), _p(sb), bcast,
                                       _stream()), "mnet_style_rows")
    return dst, eps, sb


def argmax_rows(x):
    lib = _lib.load()
    _need_cuda(x)
    rows, d = x.shape
    idx = torch.empty((rows,), dtype=torch.int64, device=x.device)
    _lib.check(lib.mnet_argmax_rows(_p(x), _p(idx), rows, d, _stream()), "mnet_argmax_rows")
    return idx


@_plumbing
def convert(x, dtype):
    if x.dtype == dtype:
        return x
    lib = _lib.load()
    _need_cuda(x)
    y = new_tensor(x.shape, dtype, x.device)
    stats.tail("convert", (x, y), lambda: _lib.check(lib.mnet_convert(_p(x), _dt(x), _p(y), _dt(y), x.numel(), _stream()), "mnet_convert"))
    return y


def fused_bias_act(x, bias, negative_slope=0.2, scale=2 ** 0.5):
    """basicsr.ops.fused_act.fused_leaky_relu semantics on a contiguous fp32 [N,C,...] tensor."""
    lib = _lib.load()
    _need_cuda(x, bias)
    if x.dtype != torch.float32:
        raise TypeError("fused_bias_act: fp32 expected")
    C = x.shape[1]
    inner = 1
    for s in x.shape[2:]:
        inner *= s
    y = tag(torch.empty_like(x))
    _lib.check(lib.mnet_fused_bias_act(_p(x), _p(bias), _p(y), x.numel(), C, inner, negative_slope, scale, _stream()),
               "mnet_fused_bias_act")
    return y


@_plumbing
def sr_postprocess(y_nhwc, u8=True):
    """test_sr.py:198-200 on the NHWC SR tensor [B,H,W,c_ld] (RGB in channels 0..2) → [B,H,W,3] BGR, uint8 (cv2.imwrite's
    rounding) or float32 (the array the script passes to cv2)."""
    lib = _lib.load()
    _need_cuda(y_nhwc)
    b, h, w, c_ld = y_nhwc.shape
    out = torch.empty((b, h, w, 3), dtype=torch.uint8 if u8 else torch.float32, device=y_nhwc.device)
    _lib.check(lib.mnet_sr_postprocess(_p(y_nhwc), _dt(y_nhwc), _p(out), 1 if u8 else 0, b * h * w, c_ld, _stream()),
               "mnet_sr_postprocess")
    return out


def table_to_device(records, device):
    """numpy record array [..., n] whose dtype is that of a ``_lib`` structure (``np.dtype(_lib.LqImage)``, ...) → uint8 [..., n, sizeof(struct)] on
    ``device``, the form the descriptor-table kernels take: ONE host→device copy of the whole table"""
    records = np.ascontiguousarray(records)
    return torch.from_numpy(records.view(np.uint8).reshape(records.shape + (records.dtype.itemsize,))).to(device)


def _check_table(who, what, table, struct, align):
    """a descriptor table on the device: uint8 [n, sizeof(struct)] (TypeError), its rows aligned as the kernel reads them (ValueError)"""
    if table.dtype != torch.uint8 or table.dim() != 2 or table.shape[1] != ctypes.sizeof(struct):
        raise TypeError("%s: a uint8 [n, %d] %s expected" % (who, ctypes.sizeof(struct), what))
    if table.data_ptr() % align:
        raise ValueError("%s: the %s must be %d-byte aligned" % (who, what, align))


def _out(who, out, shape, dtype, device):
    """``out`` as given when it has exactly this shape and dtype (TypeError otherwise); None → a new tensor"""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype:
        raise TypeError("%s: out must be %s %s" % (who, dtype, list(shape)))
    return out


def lq_from_u8(src, table, dst_h, canvas_w, preview=False, out=None):
    """mnet_lq_from_u8 (test_sr.py:98-115 on the device; the bits of lq_io.lq_from_image / lq_io.show_lq): ``src`` uint8 [bytes], a ragged batch
    of tightly packed HxWx3 images; ``table`` uint8 [n, sizeof(mnet_lq_image)], the images' descriptors (``_lib.LqImage``), both on the device.
    → fp32 [n,3,dst_h,canvas_w] (normalised, −1 beyond an image's width) or, ``preview=True``, uint8 [n,dst_h,canvas_w,3] (0 beyond it).
    The kernel writes the whole of ``out``."""
    lib = _lib.load()
    _need_cuda(src, table, out)
    if src.dtype != torch.uint8:
        raise TypeError("lq_from_u8: uint8 pixels expected")
    _check_table("lq_from_u8", "descriptor table", table, _lib.LqImage, 8)
    n = int(table.shape[0])
    out = _out("lq_from_u8", out, (n, dst_h, canvas_w, 3) if preview else (n, 3, dst_h, canvas_w), torch.uint8 if preview else torch.float32, src.device)
    _lib.check(lib.mnet_lq_from_u8(_p(src), _p(table), n, dst_h, canvas_w, _p(out), _lib.LQ_FORM_U8_HWC if preview else _lib.LQ_FORM_F32_NCHW,
                                   _stream()), "mnet_lq_from_u8")
    return out


def lq_windows_u8(src, table, dst_h=32, canvas_w=512, out=None):
    """mnet_lq_windows_u8 (``lq_from_u8``'s fp32 form for windows that are VIEWS of images on the device): ``src`` uint8 [bytes]; ``table`` uint8
    [n, sizeof(mnet_lq_window)], the windows' descriptors (``_lib.LqWindow``: first byte, row pitch, size), both on the device.
    → fp32 [n,3,dst_h,canvas_w], the bits ``lq_from_u8`` gives for each window's pixels copied out tightly (−1 beyond a window's width).
    The kernel writes the whole of ``out``; a descriptor that does not lie inside ``src`` is written as fill (``lq_device.prepare_windows`` refuses it)."""
    lib = _lib.load()
    _need_cuda(src, table, out)
    if src.dtype != torch.uint8 or src.dim() != 1 or not src.is_contiguous():
        raise TypeError("lq_windows_u8: uint8 [bytes] pixels expected")
    _check_table("lq_windows_u8", "window table", table, _lib.LqWindow, 8)
    n = int(table.shape[0])
    out = _out("lq_windows_u8", out, (n, 3, dst_h, canvas_w), torch.float32, src.device)
    _lib.check(lib.mnet_lq_windows_u8(_p(src), src.numel(), _p(table), n, dst_h, canvas_w, _p(out), _lib.LQ_FORM_F32_NCHW, _stream()),
               "mnet_lq_windows_u8")
    return out


def panel_u8(preview, sr_bgr, prior_nhwc4, strips, marks, out_w=None, out=None):
    """mnet_panel_u8 (test_sr.py:203-232 on the device; the bytes of lq_io.panel_rgb_u8(lq_io.panel(...))): ``preview`` uint8 [P,128,preview_w,3]
    RGB (``lq_from_u8(preview=True)``), ``sr_bgr`` uint8 [n,128,sr_w,3] (``sr_postprocess``), ``prior_nhwc4`` fp32 [G,128,128,4] (the generator's
    structure images), ``strips`` uint8 [n, sizeof(mnet_panel_strip)] (``_lib.PanelStrip``), ``marks`` int32 [G,4] — all on the device.
    → uint8 [n,512,out_w,3] RGB (``out_w`` defaults to preview_w), 0 at the columns beyond a strip's show_w.  The kernel writes the whole of ``out``."""
    lib = _lib.load()
    _need_cuda(preview, sr_bgr, prior_nhwc4, strips, marks, out)
    if preview.dtype != torch.uint8 or preview.dim() != 4 or preview.shape[1] != 128 or preview.shape[3] != 3:
        raise TypeError("panel_u8: preview must be uint8 [P,128,W,3]")
    if sr_bgr.dtype != torch.uint8 or sr_bgr.dim() != 4 or sr_bgr.shape[1] != 128 or sr_bgr.shape[3] != 3:
        raise TypeError("panel_u8: sr_bgr must be uint8 [n,128,W,3]")
    if prior_nhwc4.dtype != torch.float32 or prior_nhwc4.dim() != 4 or tuple(prior_nhwc4.shape[1:]) != (128, 128, 4):
        raise TypeError("panel_u8: prior_nhwc4 must be fp32 [G,128,128,4]")
    if marks.dtype != torch.int32 or marks.dim() != 2 or marks.shape[1] != 4:
        raise TypeError("panel_u8: marks must be int32 [G,4]")
    _check_table("panel_u8", "descriptor table", strips, _lib.PanelStrip, 8)
    n = int(strips.shape[0])
    if n < 1 or sr_bgr.shape[0] != n:
        raise ValueError("panel_u8: one SR image per descriptor expected (%d descriptors, %d images)" % (n, sr_bgr.shape[0]))
    if prior_nhwc4.data_ptr() % 16:
        raise ValueError("panel_u8: prior_nhwc4 must be 16-byte aligned")
    out_w = int(preview.shape[2]) if out_w is None else int(out_w)
    if out_w < 1 or out_w > preview.shape[2]:
        raise ValueError("panel_u8: out_w %d outside [1, preview width %d]" % (out_w, preview.shape[2]))
    out = _out("panel_u8", out, (n, 512, out_w, 3), torch.uint8, preview.device)
    _lib.check(lib.mnet_panel_u8(_p(preview), int(preview.shape[2]), _p(sr_bgr), int(sr_bgr.shape[2]), _p(prior_nhwc4), _p(strips), _p(marks), n, out_w,
                                 _p(out), _stream()), "mnet_panel_u8")
    return out


def stitch_u8(sr, lines, windows, out_w, out=None):
    """mnet_stitch_u8 (the bytes of long_lines.stitch_host): ``sr`` uint8 [n_sr,rows,sr_w,3] (``sr_postprocess``), ``lines`` uint8
    [L, sizeof(mnet_stitch_line)] (``_lib.StitchLine``), ``windows`` uint8 [W, sizeof(mnet_stitch_window)] (``_lib.StitchWindow``) — all on the
    device; every line's (win0, n_win) must lie inside ``windows``.  → uint8 [L,rows,out_w,3] in sr's channel order, 0 at the columns beyond a
    line's width and over a line whose descriptors cannot be followed.  The kernel writes the whole of ``out``."""
    lib = _lib.load()
    _need_cuda(sr, lines, windows, out)
    if sr.dtype != torch.uint8 or sr.dim() != 4 or sr.shape[3] != 3:
        raise TypeError("stitch_u8: sr must be uint8 [n,rows,W,3]")
    _check_table("stitch_u8", "line table", lines, _lib.StitchLine, 4)
    _check_table("stitch_u8", "window table", windows, _lib.StitchWindow, 4)
    n_lines, out_w = int(lines.shape[0]), int(out_w)
    if n_lines < 1 or windows.shape[0] < 1 or out_w < 1 or sr.numel() == 0:
        raise ValueError("stitch_u8: empty batch (%d lines, %d windows, out_w %d, sr %s)" % (n_lines, windows.shape[0], out_w, list(sr.shape)))
    out = _out("stitch_u8", out, (n_lines, int(sr.shape[1]), out_w, 3), torch.uint8, sr.device)
    _lib.check(lib.mnet_stitch_u8(_p(sr), int(sr.shape[0]), int(sr.shape[1]), int(sr.shape[2]), _p(lines), _p(windows), n_lines, out_w, _p(out),
                                  _stream()), "mnet_stitch_u8")
    return out


_U8_FORMS = {1: "[bytes]", 3: "[H,W,3]", 4: "[L,rows,W,3]"}


def _need_u8(who, name, t, dims):
    """``t`` is a uint8 tensor of ``dims`` dimensions, the last of them 3 channels where there are several (TypeError)"""
    if t.dtype != torch.uint8 or t.dim() != dims or (dims > 1 and t.shape[-1] != 3):
        raise TypeError("%s: %s must be uint8 %s" % (who, name, _U8_FORMS[dims]))


def _paste_lines(who, unit, struct, lines, table, page):
    """``paste_u8`` and ``column_paste_u8``: the one wrapper of the two per-descriptor pastes, whose descriptor ``who`` calls a ``unit``"""
    lib = _lib.load()
    _need_cuda(lines, table, page)
    _need_u8(who, "lines", lines, 4)
    _need_u8(who, "page", page, 3)
    _check_table(who, "%s table" % unit, table, struct, 8)
    if table.shape[0] < 1 or lines.numel() == 0 or page.numel() == 0:
        raise ValueError("%s: empty batch (%d %ss, lines %s, page %s)" % (who, table.shape[0], unit, list(lines.shape), list(page.shape)))
    _lib.check(getattr(lib, "mnet_" + who)(_p(lines), int(lines.shape[0]), int(lines.shape[1]), int(lines.shape[2]), _p(table), int(table.shape[0]), _p(page),
                                           int(page.shape[0]), int(page.shape[1]), _stream()), "mnet_" + who)
    return page


def paste_u8(lines, regions, page):
    """mnet_paste_u8 (the bytes of pages.paste_host, region by region): ``lines`` uint8 [L,rows,line_w,3] BGR (``stitch_u8``), ``regions`` uint8
    [R, sizeof(mnet_paste_region)] (``_lib.PasteRegion``), ``page`` uint8 [H,W,3] RGB holding the background — all on the device.  ``page`` is
    modified IN PLACE inside the regions' rectangles and returned; a region whose descriptor cannot be followed keeps the background."""
    return _paste_lines("paste_u8", "region", _lib.PasteRegion, lines, regions, page)


def column_paste_u8(lines, cells, page):
    """mnet_column_paste_u8 (the bytes of columns.paste_column_host, cell by cell): ``lines`` uint8 [L,rows,line_w,3] BGR (``stitch_u8``), ``cells``
    uint8 [n, sizeof(mnet_column_paste)] (``_lib.ColumnPaste``), ``page`` uint8 [H,W,3] RGB holding the background — all on the device.  ``page`` is
    modified IN PLACE inside the cells' rectangles and returned; a cell whose descriptor cannot be followed keeps the background."""
    return _paste_lines("column_paste_u8", "cell", _lib.ColumnPaste, lines, cells, page)


def _warp(who, src_name, src, table_name, table, struct, segs, max_w, max_h, dst_name, dst):
    """the one wrapper of the quadrilateral's and the curve's crop and paste: ``src`` (the page, or the atlas) is read through ``table`` (and the
    curve's ``segs``, None for a quadrilateral) into ``dst`` (the flat batch [bytes], or the page), which is returned"""
    lib = _lib.load()
    _need_cuda(*[t for t in (src, table, segs, dst) if t is not None])
    _need_u8(who, src_name, src, 3)
    _need_u8(who, dst_name, dst, 3 if dst_name == "page" else 1)
    _check_table(who, "%s table" % table_name, table, struct, 8)
    if segs is not None:
        _check_table(who, "segment table", segs, _lib.CurveSeg, 8)
    if table.shape[0] < 1 or (segs is not None and segs.shape[0] < 1) or src.numel() == 0 or dst.numel() == 0 or int(max_w) < 1 or int(max_h) < 1:
        ends = "atlas %s, page %s" % (list(src.shape), list(dst.shape)) if dst_name == "page" else "page %s, %d bytes" % (list(src.shape), dst.numel())
        raise ValueError("%s: empty batch (%d %ss of at most %d x %d, %s%s)" % (who, table.shape[0], table_name, int(max_w), int(max_h),
                                                                               "" if segs is None else "%d segments, " % segs.shape[0], ends))
    seg_args = () if segs is None else (_p(segs), int(segs.shape[0]))
    dst_args = (int(dst.shape[0]), int(dst.shape[1])) if dst_name == "page" else (int(dst.numel()),)
    _lib.check(getattr(lib, "mnet_" + who)(_p(src), int(src.shape[0]), int(src.shape[1]), _p(table), int(table.shape[0]), *seg_args, int(max_w), int(max_h),
                                           _p(dst), *dst_args, _stream()), "mnet_" + who)
    return dst


def quad_crop_u8(page, crops, max_w, max_h, dst):
    """mnet_quad_crop_u8 (the bytes of quads.warp_crop_host, crop by crop): ``page`` uint8 [H,W,3] RGB, ``crops`` uint8 [n, sizeof(mnet_quad_crop)]
    (``_lib.QuadCrop``), ``dst`` uint8 [bytes], the flat buffer of the ragged batch — all on the device; ``max_w`` / ``max_h``: the largest crop size
    of the table.  ``dst`` is written inside the crops only and returned; a crop whose descriptor cannot be followed leaves its bytes as they are."""
    return _warp("quad_crop_u8", "page", page, "crop", crops, _lib.QuadCrop, None, max_w, max_h, "dst", dst)


def quad_paste_u8(atlas, regions, max_bw, max_bh, page):
    """mnet_quad_paste_u8 (the bytes of quads.warp_paste_host, region by region): ``atlas`` uint8 [AH,AW,3] RGB holding the regions' upright
    foregrounds, ``regions`` uint8 [R, sizeof(mnet_quad_region)] (``_lib.QuadRegion``), ``page`` uint8 [H,W,3] RGB holding the background — all on
    the device; ``max_bw`` / ``max_bh``: the largest bounding box of the table.  ``page`` is modified IN PLACE inside the quadrilaterals and
    returned; a region whose descriptor cannot be followed keeps the background."""
    return _warp("quad_paste_u8", "atlas", atlas, "region", regions, _lib.QuadRegion, None, max_bw, max_bh, "page", page)


def curve_crop_u8(page, crops, segs, max_w, max_h, dst):
    """mnet_curve_crop_u8 (the bytes of curves.warp_crop_host, crop by crop): ``page`` uint8 [H,W,3] RGB, ``crops`` uint8 [n, sizeof(mnet_curve_crop)]
    (``_lib.CurveCrop``), ``segs`` uint8 [S, sizeof(mnet_curve_seg)] (``_lib.CurveSeg``), ``dst`` uint8 [bytes], the flat buffer of the ragged batch —
    all on the device; ``max_w`` / ``max_h``: the largest crop size of the table.  ``dst`` is written inside the crops only and returned; a crop whose
    descriptor cannot be followed leaves its bytes as they are."""
    return _warp("curve_crop_u8", "page", page, "crop", crops, _lib.CurveCrop, segs, max_w, max_h, "dst", dst)


def curve_paste_u8(atlas, regions, segs, max_bw, max_bh, page):
    """mnet_curve_paste_u8 (the bytes of curves.warp_paste_host, region by region): ``atlas`` uint8 [AH,AW,3] RGB holding the regions' upright
    foregrounds, ``regions`` uint8 [R, sizeof(mnet_curve_region)] (``_lib.CurveRegion``), ``segs`` uint8 [S, sizeof(mnet_curve_seg)]
    (``_lib.CurveSeg``), ``page`` uint8 [H,W,3] RGB holding the background — all on the device; ``max_bw`` / ``max_bh``: the largest bounding box of
    the table.  ``page`` is modified IN PLACE inside the regions and returned; a region whose descriptor cannot be followed keeps the background."""
    return _warp("curve_paste_u8", "atlas", atlas, "region", regions, _lib.CurveRegion, segs, max_bw, max_bh, "page", page)


def column_gather_u8(page, cells, max_dw, dst_h, dst):
    """mnet_column_gather_u8 (the bytes of columns.virtual_strip, cell by cell): ``page`` uint8 [H,W,3] RGB, ``cells`` uint8
    [n, sizeof(mnet_column_cell)] (``_lib.ColumnCell``), ``dst`` uint8 [bytes], the flat buffer of the ragged batch of window images of height
    ``dst_h`` — all on the device; ``max_dw``: the largest cell width of the table.  ``dst`` is written inside the cells' columns only and returned; a
    cell whose descriptor cannot be followed leaves its bytes as they are."""
    lib = _lib.load()
    _need_cuda(page, cells, dst)
    _need_u8("column_gather_u8", "page", page, 3)
    _need_u8("column_gather_u8", "dst", dst, 1)
    _check_table("column_gather_u8", "cell table", cells, _lib.ColumnCell, 8)
    if cells.shape[0] < 1 or page.numel() == 0 or dst.numel() == 0 or int(max_dw) < 1 or int(dst_h) < 1:
        raise ValueError("column_gather_u8: empty batch (%d cells of at most %d x %d, page %s, %d bytes)"
                         % (cells.shape[0], int(max_dw), int(dst_h), list(page.shape), dst.numel()))
    _lib.check(lib.mnet_column_gather_u8(_p(page), int(page.shape[0]), int(page.shape[1]), _p(cells), int(cells.shape[0]), int(max_dw), int(dst_h),
                                         _p(dst), int(dst.numel()), _stream()), "mnet_column_gather_u8")
    return dst


def _ink_dst(who, src, dst_len, dst):
    """the rule of the two ink kernels that ADD: either ``dst_len`` → a new int32 tensor of zeros beside ``src``, or the caller's ``dst``"""
    if (dst is None) == (dst_len is None):
        raise TypeError("%s: either dst_len (the profiles are returned in a new tensor of zeros) or dst (they are added to it)" % who)
    return torch.zeros((int(dst_len),), dtype=torch.int32, device=src.device) if dst is None else dst


def _ink(fn, who, src, as_page, what, table, struct, dims, dst):
    """the one wrapper of the three ink-profile kernels, ``fn`` the entry point of ``who``: ``src`` — the page as uint8 [bytes], or ``as_page``: [H,W,3]
    and its size — is read through ``table``, ``who``'s ``what``, into the int32 ``dst``, which is returned; ``dims``: the call's integers between them"""
    _need_cuda(src, table, dst)
    if as_page:
        _need_u8(who, "page", src, 3)
    elif src.dtype != torch.uint8 or src.dim() != 1:
        raise TypeError("%s: uint8 [bytes] pixels expected" % who)
    if dst.dtype != torch.int32 or dst.dim() != 1:
        raise TypeError("%s: int32 [len] dst expected" % who)
    _check_table(who, what, table, struct, 8)
    status = fn(_p(src), *(src.shape[:2] if as_page else (src.numel(),)), _p(table), table.shape[0], *dims, _p(dst), dst.numel(), _stream())
    if status:
        _lib.check(status, "mnet_" + who)
    return dst


def row_ink_u8(src, boxes, max_h, dst):
    """mnet_row_ink_u8 (``blind_columns.row_ink``, box by box, with ==): ``src`` uint8 [bytes], the page; ``boxes`` uint8 [n, sizeof(mnet_ink_box)]
    (``_lib.RowInkBox``: first byte, row pitch, size, first index in ``dst``); ``dst`` int32 [len] — all on the device; ``max_h``: the largest box
    height of the table.  ``dst[out + r]`` = row r's total horizontal variation of integer luma, written for the rows of the boxes only (−1 for a
    box that does not lie inside ``src``; nothing for rows that do not lie inside ``dst``); ``dst`` is returned.  One launch for all boxes."""
    return _ink(_lib.load().mnet_row_ink_u8, "row_ink_u8", src, False, "box table", boxes, _lib.RowInkBox, (int(max_h),), dst)


def box_ink_u8(src, boxes, max_h, max_w, floor, dst_len=None, dst=None):
    """mnet_box_ink_u8 (``layout.box_ink``, box by box, with ==): ``src`` uint8 [bytes], the page; ``boxes`` uint8 [n, sizeof(mnet_ink_box2)]
    (``_lib.BoxInkBox``: first byte, row pitch, size, the first index of the row profile and of the column profile in ``dst``) — on the device;
    ``max_h`` / ``max_w``: the largest box size of the table; ``floor``: 0..255, a luma difference below it counts as nothing.  The kernel ADDS
    the profiles: ``dst_len`` → a new int32 [dst_len] of zeros holds them; ``dst`` (instead) → an int32 [len] tensor of the caller's they are added
    to.  −1 in both profiles of a box that does not lie inside ``src``, nothing for a box whose ranges do not lie inside ``dst``.  One launch for
    all boxes; the profiles' tensor is returned."""
    return _ink(_lib.load().mnet_box_ink_u8, "box_ink_u8", src, False, "box table", boxes, _lib.BoxInkBox, (int(max_h), int(max_w), int(floor)),
                _ink_dst("box_ink_u8", src, dst_len, dst))


def skew_ink_u8(page, boxes, max_h, max_w, floor, dst_len=None, dst=None):
    """mnet_skew_ink_u8 (``skew.frame_ink``, record by record, with ==): ``page`` uint8 [H,W,3] RGB; ``boxes`` uint8 [n, sizeof(mnet_skew_box)]
    (``_lib.SkewInkBox``: frame box, slope, the first index of the row profile and of the column profile in ``dst`` — −1: not wanted —, the page
    rectangle to scan) — on the device; ``max_h`` / ``max_w``: the largest scan rectangle of the table; ``floor``: 0..255.  The kernel ADDS the
    profiles: ``dst_len`` → a new int32 [dst_len] of zeros holds them; ``dst`` (instead) → an int32 [len] tensor of the caller's they are added to.
    −1 in the wanted, in-range profiles of a record that cannot be followed (include/marconet_hip_skewink.h).  One launch for all records; the
    profiles' tensor is returned."""
    return _ink(_lib.load().mnet_skew_ink_u8, "skew_ink_u8", page, True, "record table", boxes, _lib.SkewInkBox, (int(max_h), int(max_w), int(floor)),
                _ink_dst("skew_ink_u8", page, dst_len, dst))


def page_tiles(page_h, page_w):
    """the count of 64 x 16 tiles of a page, row-major from its origin (csrc/page_tile.h's pt_grid(1, page_w, page_h)) → (tiles_x, tiles_y)"""
    return -(-int(page_w) // 64), -(-int(page_h) // 16)


def _check_order(who, spans, order, items=None):
    """what the two page-tile compositors ask alike of their spans and order (and the mixed one of its items)"""
    _check_table(who, "span table", spans, _lib.TileSpan, 4)
    if order.dtype != torch.int32 or order.dim() != 1:
        raise TypeError("%s: order must be int32 [n]" % who)
    if not spans.is_contiguous() or not order.is_contiguous() or not (items is None or items.is_contiguous()):
        raise ValueError("%s: %sspans and order must be contiguous" % (who, "" if items is None else "items, "))


def _check_span_count(who, spans, page):
    tiles_x, tiles_y = page_tiles(page.shape[0], page.shape[1])
    if spans.shape[0] != tiles_x * tiles_y:
        raise ValueError("%s: %d spans for a page of %d x %d tiles" % (who, spans.shape[0], tiles_x, tiles_y))


def paste_ordered_u8(lines, cells, spans, order, page):
    """mnet_paste_ordered_u8 (the bytes of pages.paste_host / columns.paste_column_host applied cell after cell in the table's order, overlaps
    included): ``lines`` uint8 [L,rows,line_w,3] BGR (``stitch_u8``), ``cells`` uint8 [n, sizeof(mnet_column_paste)] (``_lib.ColumnPaste``; a plain
    region as ``pages.as_cell`` states it), ``spans`` uint8 [tiles, sizeof(mnet_tile_span)] (``_lib.TileSpan``), one per 64 x 16 tile of the page,
    ``order`` int32 [n_order], indices into ``cells`` (``pages.bin_tiles`` makes both), ``page`` uint8 [H,W,3] RGB holding the background — all on the
    device.  ``page`` is modified IN PLACE inside the cells' rectangles and returned; a span, an entry or a cell that cannot be followed is skipped."""
    lib = _lib.load()
    who = "paste_ordered_u8"
    _need_cuda(lines, cells, spans, order, page)
    _need_u8(who, "lines", lines, 4)
    _need_u8(who, "page", page, 3)
    _check_table(who, "cell table", cells, _lib.ColumnPaste, 8)
    _check_order(who, spans, order)
    if cells.shape[0] < 1 or order.shape[0] < 1 or lines.numel() == 0 or page.numel() == 0:
        raise ValueError("paste_ordered_u8: empty batch (%d cells, %d order entries, lines %s, page %s)"
                         % (cells.shape[0], order.shape[0], list(lines.shape), list(page.shape)))
    _check_span_count(who, spans, page)
    _lib.check(lib.mnet_paste_ordered_u8(_p(lines), int(lines.shape[0]), int(lines.shape[1]), int(lines.shape[2]), _p(cells), int(cells.shape[0]),
                                         _p(spans), int(spans.shape[0]), _p(order), int(order.shape[0]), _p(page), int(page.shape[0]),
                                         int(page.shape[1]), _stream()), "mnet_paste_ordered_u8")
    return page


def paste_mixed_u8(lines, atlas, cells, quads, curves, segs, items, spans, order, page):
    """mnet_paste_mixed_u8 (the bytes of regions.compose_regions_host's loop: pages.paste_host / columns.paste_column_host / quads.warp_paste_host /
    curves.warp_paste_host applied item after item in the table's order, overlaps included): ``lines`` uint8 [L,rows,line_w,3] BGR, ``atlas`` uint8
    [AH,AW,3] RGB holding the upright foregrounds of every quadrilateral and curved region, the tables ``cells`` (``_lib.ColumnPaste``), ``quads``
    (``_lib.QuadRegion``), ``curves`` (``_lib.CurveRegion``) with ``segs`` (``_lib.CurveSeg``) — each None where the page has none of its kind, ``lines``
    None without cells and ``atlas`` None without quads and curves —, ``items`` uint8 [n, sizeof(mnet_page_item)] (``_lib.PageItem``), ``spans`` /
    ``order`` over the items as ``paste_ordered_u8`` takes them over cells, ``page`` uint8 [H,W,3] RGB holding the background — all on the device.
    ``page`` is modified IN PLACE inside the items and returned; a span, an entry, an item or a descriptor that cannot be followed is skipped."""
    lib = _lib.load()
    who = "paste_mixed_u8"
    _need_cuda(*[t for t in (lines, atlas, cells, quads, curves, segs, items, spans, order, page) if t is not None])
    _need_u8(who, "page", page, 3)
    if lines is not None:
        _need_u8(who, "lines", lines, 4)
    if atlas is not None:
        _need_u8(who, "atlas", atlas, 3)
    for what, table, struct in (("cell table", cells, _lib.ColumnPaste), ("quad table", quads, _lib.QuadRegion), ("curve table", curves, _lib.CurveRegion),
                                ("segment table", segs, _lib.CurveSeg)):
        if table is not None:
            _check_table(who, what, table, struct, 8)
    _check_table(who, "item table", items, _lib.PageItem, 4)
    _check_order(who, spans, order, items)
    n = [0 if t is None else int(t.shape[0]) for t in (cells, quads, curves, segs)]
    if items.shape[0] < 1 or order.shape[0] < 1 or page.numel() == 0 or (n[0] and (lines is None or lines.numel() == 0)) or \
            ((n[1] or n[2]) and (atlas is None or atlas.numel() == 0)) or (n[2] and not n[3]):
        raise ValueError("%s: empty batch (%d items, %d order entries, %d cells, %d quads, %d curves, %d segments, lines %s, atlas %s, page %s)"
                         % (who, items.shape[0], order.shape[0], n[0], n[1], n[2], n[3], None if lines is None else list(lines.shape),
                            None if atlas is None else list(atlas.shape), list(page.shape)))
    _check_span_count(who, spans, page)
    ptr = lambda t: None if t is None else _p(t)
    ls = (0, 0, 0) if lines is None else tuple(int(v) for v in lines.shape[:3])
    ats = (0, 0) if atlas is None else tuple(int(v) for v in atlas.shape[:2])
    _lib.check(lib.mnet_paste_mixed_u8(ptr(lines), ls[0], ls[1], ls[2], ptr(atlas), ats[0], ats[1], ptr(cells), n[0], ptr(quads), n[1], ptr(curves), n[2],
                                       ptr(segs), n[3], _p(items), int(items.shape[0]), _p(spans), int(spans.shape[0]), _p(order), int(order.shape[0]),
                                       _p(page), int(page.shape[0]), int(page.shape[1]), _stream()), "mnet_paste_mixed_u8")
    return page


def nonfinite_flag(x, out=None):
    """mnet_nonfinite_flag: int32 [1] device tensor (``out``: a one-element int32 view to write into), 1 iff the fp32 / fp16 tensor
    ``x`` holds an inf or NaN (no synchronisation here)"""
    lib = _lib.load()
    _need_cuda(x, out)
    flag = torch.empty((1,), dtype=torch.int32, device=x.device) if out is None else out
    if flag.dtype != torch.int32 or flag.numel() != 1:
        raise TypeError("nonfinite_flag: out must be one int32 element")
    _lib.check(lib.mnet_nonfinite_flag(_p(x), _dt(x), x.numel(), _p(flag), _stream()), "mnet_nonfinite_flag")
    return flag


@_plumbing
def compare_stats(a, b, groups=None):
    """mnet_compare_stats: ``a`` (the mode's tensor) against ``b`` (the reference's) — the same logical shape, each in its own storage (fp32, fp16, or a
    tagged split-half / fp16+8 tensor; the accepted pairs: include/marconet_hip.h).  ``groups``: how many equal leading parts get a record of their own
    (None: ``a.shape[0]``; it must divide the element count into multiples of 32).  → uint8 [groups, sizeof(mnet_cmp_stats)] on the device, one
    ``_lib.CmpStats`` per group (``_lib.cmp_records`` reads a host copy).  No synchronisation, no statistics booked: this is not a kernel of the forward."""
    lib = _lib.load()
    _need_cuda(a, b)
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError("compare_stats: shapes differ (%s, %s)" % (tuple(a.shape), tuple(b.shape)))
    groups = int(a.shape[0]) if groups is None else int(groups)
    if groups < 1 or a.numel() == 0 or a.numel() % groups:
        raise ValueError("compare_stats: %d elements do not split into %d groups" % (a.numel(), groups))
    per = a.numel() // groups
    out = torch.empty((groups, ctypes.sizeof(_lib.CmpStats)), dtype=torch.uint8, device=a.device)
    ws = torch.empty((_lib.cmp_workspace_bytes(groups, per),), dtype=torch.uint8, device=a.device)
    _lib.check(lib.mnet_compare_stats(_p(a), _dt(a), _p(b), _dt(b), groups, per, _p(out), _p(ws), _stream()), "mnet_compare_stats")
    return out


@_plumbing
def pack_weights(w, dtype, cout_pad=None, cin_pad=None, scale=1.0, sn_u=None, sn_v=None):
    """mnet_pack_weights: w fp32 [cout,cin,kh,kw] (or [out,in] for a Linear) on the device → [cout_pad,kh,kw,cin_pad] in ``dtype``,
    every element (w / sigma) * scale with sigma = uᵀ(W_mat v) when the spectral-norm vectors are given (models/networks.py:14)."""
    lib = _lib.load()
    w = w.detach()
    if w.dim() == 2:
        w = w.reshape(w.shape[0], w.shape[1], 1, 1)
    w = w.contiguous()
    if w.dtype != torch.float32:
        w = w.float()
    if sn_u is not None:
        sn_u, sn_v = sn_u.detach().float().contiguous(), sn_v.detach().float().contiguous()
    _need_cuda(w, sn_u, sn_v)
    cout, cin, kh, kw = w.shape
    cout_pad, cin_pad = cout_pad or cout, cin_pad or cin
    rows = mx_weight_rows(cout_pad, kh, kw, cin_pad) if dtype == MX_DTYPE else cout_pad
    out = new_tensor((rows, kh, kw, cin_pad), dtype, w.device, zero=dtype == MX_DTYPE)
    ws = torch.empty((cout + 1,), dtype=torch.float64, device=w.device) if sn_u is not None else None
    _lib.check(lib.mnet_pack_weights(_p(w), cout, cin, kh, kw, _p(sn_u), _p(sn_v), float(scale), _dt(out), cout_pad, cin_pad, _p(out),
                                     _p(ws), _stream()), "mnet_pack_weights")
    return out


def pack_wsq(w, scale):
    """mnet_pack_wsq: demodulation table [cin,cout] of a ModulatedConv2d weight [cout,cin,kh,kw] (fp32, device)"""
    lib = _lib.load()
    w = w.detach().float().contiguous()
    _need_cuda(w)
    cout, cin, kh, kw = w.shape
    out = torch.empty((cin, cout), dtype=torch.float32, device=w.device)
    _lib.check(lib.mnet_pack_wsq(_p(w), cout, cin, kh * kw, float(scale), _p(out), _stream()), "mnet_pack_wsq")
    return out


def gather_rows(src, col0=0, ncols=None, idx=None):
    """dst[r, :] = src[idx[r] (or r), col0:col0+ncols] — fp32 [rows, ncols] contiguous (mnet_gather_rows)"""
    lib = _lib.load()
    _need_cuda(src, idx)
    if src.dtype != torch.float32 or src.dim() != 2 or (idx is not None and idx.dtype != torch.int64):
        raise TypeError("gather_rows: fp32 [rows, ld] source and int64 indices expected")
    ld = src.shape[1]
    ncols = ld - col0 if ncols is None else ncols
    rows = src.shape[0] if idx is None else idx.shape[0]
    dst = torch.empty((rows, ncols), dtype=torch.float32, device=src.device)
    if rows:
        _lib.check(lib.mnet_gather_rows(_p(src), src.shape[0], ld, col0, ncols, _p(idx), rows, _p(dst), _stream()), "mnet_gather_rows")
    return dst


@_plumbing
def torgb(x, wgt, style, scale_b, bias, skip=None):
    """mnet_torgb (ToRGB.forward, models/networks.py:313-321): x NHWC [N,H,W,C] any storage dtype; wgt fp32 [3,C]; style fp32 [N,C];
    scale_b fp32 [N] / [N,1] or None; bias fp32 [>=3]; skip fp32 [N,H/2,W/2,4] or None → fp32 [N,H,W,4] (RGB0)"""
    lib = _lib.load()
    _need_cuda(x, wgt, style, scale_b, bias, skip)
    n, h, w, c = x.shape
    if wgt.dtype != torch.float32 or wgt.numel() != 3 * c or style.dtype != torch.float32 or tuple(style.shape) != (n, c):
        raise RuntimeError("torgb: weight [3,C] / style [N,C] fp32 expected")
    if skip is not None and (skip.dtype != torch.float32 or tuple(skip.shape) != (n, h // 2, w // 2, 4)):
        raise RuntimeError("torgb: skip must be fp32 [N,H/2,W/2,4]")
    out = torch.empty((n, h, w, 4), dtype=torch.float32, device=x.device)
    stats.tail("torgb", (x, skip, out), lambda: _lib.check(lib.mnet_torgb(_p(x), _dt(x), n, h, w, c, _p(wgt), _p(style), _p(scale_b), _p(bias), _p(skip), _p(out), _stream()), "mnet_torgb"))
    return out


@_plumbing
def conv3x3_rgb(x, wgt, bias, act=ACT_TANH, nhwc=True, nchw=False):
    """conv_final.6 (+ tanh): x NHWC [N,H,W,64]; wgt [3,3,3,64] same dtype (fp32 for a split-half x); bias fp32 [3] → NHWC
    [N,H,W,8] (same dtype; fp32 for a split-half x) and/or fp32 NCHW [N,3,H,W]; returns (y_nhwc or None, y_nchw or None)."""
    lib = _lib.load()
    _need_cuda(x, wgt, bias)
    n, h, w, c = x.shape
    odt = torch.float32 if is_split(x.dtype) else x.dtype            # split-half / fp16+8 input: fp32 weights, fp32 outputs
    if wgt.dtype != odt or wgt.numel() != 3 * 9 * c:
        raise RuntimeError("conv3x3_rgb: weight dtype/shape mismatch")
    y1 = torch.empty((n, h, w, 8), dtype=odt, device=x.device) if nhwc else None
    y2 = torch.empty((n, 3, h, w), dtype=torch.float32, device=x.device) if nchw else None
    stats.tail("conv3x3_rgb", (x, y1, y2), lambda: _lib.check(lib.mnet_conv3x3_rgb(_p(x), _dt(x), n, h, w, c, _p(wgt), _p(bias), act, _p(y1), _p(y2), _stream()), "mnet_conv3x3_rgb"))
    return y1, y2
