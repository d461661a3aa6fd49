"""The input side of the script's driver glue on the GPU: what ``lq_io.lq_from_image`` / ``lq_io.show_lq`` do to a strip
before ``modelEncoder(LQ)`` (test_sr.py:98-115) — for a whole batch of raw uint8 RGB arrays with one kernel launch per output
(``mnet_lq_from_u8``), one host→device copy of the packed pixels and one of the descriptor table.  The host computes per image only scalars
(sizes, the resized widths, the sampling step); there is no per-pixel host work.

``lq_io`` stays the pure-host definition: the device path returns its bits (tests/test_lq_device_gpu.py) and raises its errors.
"""
import collections

import numpy as np
import torch

from . import _lib, ops
from .lq_io import LQ_H, LQ_W, StripTooWide

SHOW_H = 4 * LQ_H             # test_sr.py:99: ShowLQ, the strip at height 128

Geometry = collections.namedtuple("Geometry", "h w dw scale show_w show_scale")
Prepared = collections.namedtuple("Prepared", "lq content_w show_w index preview skipped")


def _axis(h, w, dst_h):
    """``resize_cubic(img, dst_h / h, dst_h / h)``'s output size and the table's sampling step: (dw, dh, scale) exactly as the host computes
    them (Python floats; numpy's round half to even)"""
    fx = dst_h / h
    return int(np.rint(w * fx)), int(np.rint(h * fx)), 1.0 / fx


def strip_geometry(img, preview=True):
    """the scalars of one strip, with the host path's errors in the host path's order (``lq_io.lq_from_image``): TypeError for an array that is
    not uint8 HxWxC, ValueError for an empty output or another channel count than 3, StripTooWide beyond 512 px at height 32"""
    shape = np.shape(img)
    if len(shape) != 3:
        raise ValueError("uint8 RGB HxWx3 array expected, got shape %s" % (tuple(shape),))
    if np.asarray(img).dtype != np.uint8:
        raise TypeError("resize_cubic: uint8 HxWxC image expected")
    h, w, c = (int(v) for v in shape)
    if c != 3:
        raise ValueError("uint8 RGB HxWx3 array expected, got %d channels" % c)
    return shape_geometry(h, w, preview)


def shape_geometry(h, w, preview=True):
    """``strip_geometry`` of a uint8 RGB strip of h x w pixels, from its size alone (its errors from ``resize_cubic: empty output`` on)"""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError("resize_cubic: empty output")
    dw, dh, scale = _axis(h, w, LQ_H)
    if dw <= 0 or dh <= 0:
        raise ValueError("resize_cubic: empty output")
    show_w, show_h, show_scale = _axis(h, w, SHOW_H)
    if dw > LQ_W:
        raise StripTooWide("strip is %d px wide at height 32 (limit %d): crop it into shorter segments" % (dw, LQ_W))
    # the kernel resizes to a FIXED height: the host's own output height rint(h * (dst_h / h)) must be that height (it is for every h <= 4096)
    if dh != LQ_H or (preview and (show_h != SHOW_H or show_w <= 0)):
        raise ValueError("strip of height %d does not resize to height %d / %d" % (h, LQ_H, SHOW_H))
    return Geometry(h, w, dw, scale, show_w, show_scale)


def build_table(geoms, offsets, preview):
    """→ numpy record array of ``mnet_lq_image`` [1 or 2, n]: row 0 the height-32 descriptors, row 1 (``preview``) the height-128 ones"""
    n = len(geoms)
    tab = np.zeros((2 if preview else 1, n), dtype=np.dtype(_lib.LqImage))
    for k, (g, off) in enumerate(zip(geoms, offsets)):
        tab[0, k] = (off, g.h, g.w, g.dw, 0, g.scale)
        if preview:
            tab[1, k] = (off, g.h, g.w, g.show_w, 0, g.show_scale)
    return tab


def prepare_strips(images, device, preview=False, skip_too_wide=False):
    """images: list of uint8 RGB HxWx3 arrays → ``Prepared``:

        lq         fp32 [B,3,32,512] on ``device`` — ``lq_io.lq_from_image(img)[0]`` of the B accepted images, bit for bit
        content_w  their widths at height 32, ``show_w`` their widths at height 128 (lists of B ints)
        index      positions of the accepted images in ``images``
        preview    ``preview=True``: uint8 [B,128,max(show_w),3] on ``device`` — ``lq_io.show_lq(img)`` at columns < show_w[k], 0 beyond
        skipped    ``skip_too_wide=True`` only: [(position, StripTooWide)] — the strips the script skips with a warning (test_sr.py:108-110)

    Every error of the host path is raised as ``lq_io.lq_from_image`` raises it — StripTooWide included, before anything is copied or
    launched; ``skip_too_wide=True`` (``MarconetPipeline.restore_images``) leaves such strips out of the batch instead, as the script does."""
    device = torch.device(device)
    geoms, index, skipped, flat, offsets, off = [], [], [], [], [], 0
    for i, img in enumerate(images):
        try:
            g = strip_geometry(img, preview)
        except StripTooWide as e:
            if not skip_too_wide:
                raise
            skipped.append((i, e))
            continue
        geoms.append(g)
        index.append(i)
        offsets.append(off)
        flat.append(np.ascontiguousarray(img).reshape(-1))
        off += g.h * g.w * 3
    if not geoms:
        return Prepared(torch.empty((0, 3, LQ_H, LQ_W), dtype=torch.float32, device=device), [], [], [],
                        torch.empty((0, SHOW_H, 0, 3), dtype=torch.uint8, device=device) if preview else None, skipped)
    src = torch.from_numpy(np.concatenate(flat)).to(device)                            # the one copy of the pixels
    return _resize_packed(src, geoms, offsets, index, skipped, preview)


def _resize_packed(src, geoms, offsets, index, skipped, preview):
    """the launches of ``prepare_strips`` / ``prepare_packed``: ``src`` uint8 [bytes] on the device holds image k at ``offsets[k]``, ``geoms[k]`` its scalars"""
    content_w, show_w = [g.dw for g in geoms], [g.show_w for g in geoms]
    table = ops.table_to_device(build_table(geoms, offsets, preview), src.device)       # the one copy of the table (both rows)
    with ops.on_device(src):
        lq = ops.lq_from_u8(src, table[0], LQ_H, LQ_W)
        show = ops.lq_from_u8(src, table[1], SHOW_H, max(show_w), preview=True) if preview else None
    return Prepared(lq, content_w, show_w, index, show, skipped)


def prepare_packed(src_device, shapes, offsets, preview=False):
    """``prepare_strips`` from pixels that are on the device already: ``src_device`` uint8 [bytes], a ragged batch of tightly packed HxWx3 images
    (``ops.quad_crop_u8`` writes one); ``shapes[k]`` = (h, w) of image k and ``offsets[k]`` its first byte → ``Prepared`` of all images, the bits
    ``prepare_strips`` gives for the same pixels.  No pixel is copied; one copy of the table.  Per image, in order: the errors of its size as ``prepare_strips``
    raises them (``shape_geometry``; a strip too wide raises StripTooWide), then ValueError if it does not lie inside ``src_device`` — all before
    anything is launched."""
    if not torch.is_tensor(src_device) or src_device.dtype != torch.uint8 or src_device.dim() != 1:
        raise TypeError("prepare_packed: uint8 [bytes] device tensor expected")
    if len(shapes) != len(offsets) or not shapes:
        raise ValueError("prepare_packed: one offset per image, and at least one image, expected (%d shapes, %d offsets)" % (len(shapes), len(offsets)))
    geoms = []
    for k, ((h, w), off) in enumerate(zip(shapes, offsets)):
        geoms.append(shape_geometry(h, w, preview))
        if int(off) < 0 or int(off) + 3 * int(h) * int(w) > src_device.numel():
            raise ValueError("prepare_packed: image %d (%d x %d at byte %d) lies outside the %d bytes given" % (k, int(w), int(h), int(off), src_device.numel()))
    return _resize_packed(src_device, geoms, [int(o) for o in offsets], list(range(len(geoms))), [], preview)


def check_windows(windows, nbytes, who="prepare_windows"):
    """the host half of ``prepare_windows``, which needs no device: ``windows[k]`` = (offset, pitch, h, w) inside a buffer of ``nbytes`` bytes → their
    ``Geometry``s; per window, in order, the errors of its size (``shape_geometry``), then ValueError for a negative offset, a pitch under 3·w or a
    last row that ends outside the buffer"""
    geoms = []
    for k, (off, pitch, h, w) in enumerate(windows):
        g = shape_geometry(h, w, False)
        off, pitch = int(off), int(pitch)
        if off < 0 or pitch < 3 * g.w or pitch > 0x7fffffff or off + (g.h - 1) * pitch + 3 * g.w > int(nbytes):
            raise ValueError("%s: window %d (%d x %d at byte %d, pitch %d) lies outside the %d bytes given, or its rows overlap"
                             % (who, k, g.w, g.h, off, pitch, int(nbytes)))
        geoms.append(g)
    return geoms


def window_table(geoms, windows):
    """→ numpy record array of ``mnet_lq_window`` [n]"""
    tab = np.zeros((len(geoms),), dtype=np.dtype(_lib.LqWindow))
    for k, (g, win) in enumerate(zip(geoms, windows)):
        tab[k] = (int(win[0]), int(win[1]), g.h, g.w, g.dw, g.scale)
    return tab


def upload_lines(images, device):
    """images: uint8 RGB HxWx3 arrays → (uint8 [bytes] on ``device``, the images packed tightly one behind the other — each an image of its own
    pitch 3·w —, the byte at which each begins): the one copy of the pixels that every window of every line is then a view of.  ``strip_geometry``'s
    errors for an array that is no uint8 HxWx3 image; the sizes themselves are the windows' business."""
    flat, offsets, off = [], [], 0
    for img in images:
        shape = np.shape(img)
        if len(shape) != 3:
            raise ValueError("uint8 RGB HxWx3 array expected, got shape %s" % (tuple(shape),))
        if np.asarray(img).dtype != np.uint8:
            raise TypeError("resize_cubic: uint8 HxWxC image expected")
        if int(shape[2]) != 3:
            raise ValueError("uint8 RGB HxWx3 array expected, got %d channels" % int(shape[2]))
        offsets.append(off)
        flat.append(np.ascontiguousarray(img).reshape(-1))
        off += flat[-1].size
    src = torch.from_numpy(np.concatenate(flat) if flat else np.zeros((0,), dtype=np.uint8)).to(torch.device(device))
    return src, offsets


def line_window(offset, h, w, c0, c1):
    """the columns [c0, c1) of a tightly packed h x w image that begins at byte ``offset``, as a window of ``prepare_windows``"""
    return (int(offset) + 3 * int(c0), 3 * int(w), int(h), int(c1) - int(c0))


def prepare_windows(src_device, windows):
    """``prepare_strips`` for windows that are VIEWS of images on the device: ``src_device`` uint8 [bytes]; ``windows[k]`` = (offset, pitch, h, w) — the
    byte of the window's first pixel, the bytes per row of the image it lies in, its size → ``Prepared`` of all windows (no preview), the bits
    ``prepare_strips`` gives for the same pixels copied out tightly: BORDER_REPLICATE clamps into the window, not into the image around it.  No pixel
    is copied, overlapping windows share theirs; one copy of the table, ONE launch (``mnet_lq_windows_u8``).  ``check_windows``' errors, all before
    anything is launched."""
    if not torch.is_tensor(src_device) or src_device.dtype != torch.uint8 or src_device.dim() != 1:
        raise TypeError("prepare_windows: uint8 [bytes] device tensor expected")
    windows = list(windows)
    if not windows:
        raise ValueError("prepare_windows: at least one window expected")
    geoms = check_windows(windows, src_device.numel())
    table = ops.table_to_device(window_table(geoms, windows), src_device.device)               # the one copy of the table
    with ops.on_device(src_device):
        lq = ops.lq_windows_u8(src_device, table, LQ_H, LQ_W)
    return Prepared(lq, [g.dw for g in geoms], [g.show_w for g in geoms], list(range(len(geoms))), None, [])
