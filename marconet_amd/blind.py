"""Reading a line blind: the text and the character boxes of a line of any width from the encoder itself, so that the windows of
``long_lines.plan_windows`` — runs of WHOLE characters — can be cut without a transcription.  The encoder (``TextViT``) reads a strip of at most
512 px at height 32 and reports at most 16 (left, right) pairs; a wider line is read through overlapping probe windows, each probe keeping only
the characters that lie well inside it.  This module is the pure-host definition of that reading; ``MarconetPipeline.read_lines`` is the device
path and returns exactly this (tests/test_blind_gpu.py compares the two with ``==``).

The rules:

    plan_probes   A line ``lq_device.shape_geometry`` accepts is one probe (0, w, 0, w).  Otherwise P is the largest crop width whose width at
                  height 32 is <= ``probe_width`` (``lq_device._axis``'s arithmetic); probes [c0, c0 + P) start at 0, P//2, 2 (P//2), ... while
                  c0 + P < w, and the last one is flush right, c0 = w - P.  A probe OWNS the columns up to the middle of its overlap with each
                  neighbour, (c0_{k+1} + c1_k) // 2; the first owns from 0, the last to w.  An interior probe so owns its middle half: every
                  owned character stands at least a quarter probe from a cut.  ``probe_width`` < 512 leaves room for the encoder's 16 slots.
    read_probe    labels = ``labels.collapse_indices`` of the probe's argmax row; the first min(len, 16) get boxes, the rest are dropped and
                  reported (``overflow``), as ``restore_images(texts=None)`` truncates.  Edges: c0 + float(loc) * 512 * h / 32 in fp64, x1 the
                  smaller and x2 the larger.  A character is kept iff 2 own_lo <= x1 + x2 < 2 own_hi (a centre on a boundary has one owner).
    merge         The kept characters of a line's probes → (labels, boxes [[x1, 0, x2, h]]).  Total: it never raises.  In order: edges that are
                  not finite are dropped; boxes are clamped into [0, w]; a box under 1 px is dropped; a stable sort by centre (ties: probe
                  order); of two consecutive characters from DIFFERENT probes with the same label whose boxes overlap by more than half of the
                  narrower one, the later is dropped (one glyph seen on both sides of an ownership boundary); two neighbours that overlap meet
                  at the middle of their overlap; a box that cannot keep 1 px is dropped.  The result is left to right, pairwise disjoint,
                  inside [0, w], every box at least 1 px wide.
    The arithmetic is fp64 (Python floats) only, on the fp32 values the encoder returned: the host and the device path agree exactly.

An empty reading makes the line a skipped one (None), as an empty text does.  Nothing here claims reading QUALITY: that is the checkpoint's.
"""
import math

import numpy as np
import torch

from . import lq_device, lq_io, ops
from .labels import collapse_indices
from .lq_io import LQ_H, LQ_W, StripTooWide

SLOTS = 16                    # TextViT returns 16 (left, right) pairs


def check_probe_width(probe_width):
    """``probe_width`` as an int; ValueError unless it is a multiple of 4 in 32..512"""
    if isinstance(probe_width, (bool, float)) or not isinstance(probe_width, (int, np.integer)) or not 32 <= int(probe_width) <= LQ_W or int(probe_width) % 4:
        raise ValueError("plan_probes: probe_width must be a multiple of 4 in 32..%d (got %r)" % (LQ_W, probe_width))
    return int(probe_width)


def probe_crop_width(h, probe_width=384):
    """P: the largest crop width of a line h px high whose width at height 32 is <= ``probe_width``; ValueError for a ``probe_width`` that is not a
    multiple of 4 in 32..512, or for P < 2"""
    h, probe_width = int(h), check_probe_width(probe_width)
    if h < 1:
        raise ValueError("plan_probes: empty line (height %d)" % h)
    p = probe_width * h // LQ_H + 2                                        # dw is monotone in the crop width: walk down to the largest that fits
    while p >= 1 and lq_device._axis(h, p, LQ_H)[0] > probe_width:
        p -= 1
    if p < 2:
        raise ValueError("plan_probes: a line %d px high leaves probes of %d px: too narrow to overlap" % (h, p))
    return p


def plan_probes(h, w, probe_width=384):
    """the probes of a line of h x w source pixels → list of (c0, c1, own_lo, own_hi) in source columns (the module's head states the rules)"""
    h, w, probe_width = int(h), int(w), check_probe_width(probe_width)
    try:
        lq_device.shape_geometry(h, w, False)
        return [(0, w, 0, w)]
    except StripTooWide:
        pass
    P = probe_crop_width(h, probe_width)
    lq_device.shape_geometry(h, P, False)                                 # a height the kernel cannot resize: its ValueError, before any probe
    starts, c0 = [], 0
    while c0 + P < w:                                                      # P < w: the line is wider than 512 px at height 32, a probe is not
        starts.append(c0)
        c0 += P // 2
    starts.append(w - P)
    cuts = [0] + [(starts[k + 1] + starts[k] + P) // 2 for k in range(len(starts) - 1)] + [w]
    return [(c, c + P, cuts[k], cuts[k + 1]) for k, c in enumerate(starts)]


def read_probe(indices64, locs32, probe, h):
    """one probe's prediction — its row of argmax indices and its row of fp32 (left, right) pairs — → (labels, boxes [(x1, x2)], overflow): the
    characters the probe owns, in the encoder's order, in the line's source columns"""
    c0, _, own_lo, own_hi = (int(v) for v in probe)
    row = [int(v) for v in indices64]
    lab = collapse_indices(row)
    n = min(len(lab), SLOTS)
    labels, boxes = [], []
    for j in range(n):
        a = c0 + float(locs32[2 * j]) * 512 * int(h) / 32
        b = c0 + float(locs32[2 * j + 1]) * 512 * int(h) / 32
        x1, x2 = (a, b) if a <= b else (b, a)
        if 2 * own_lo <= x1 + x2 < 2 * own_hi:                              # False for an edge that is not a number
            labels.append(lab[j])
            boxes.append((x1, x2))
    return labels, boxes, len(lab) > SLOTS


def merge(h, w, reads):
    """``reads``: one ``read_probe`` result per probe of a line of h x w pixels, in probe order → (labels, boxes [[x1, 0, x2, h]]), left to right,
    disjoint, inside the line (the module's head states the rules).  Never raises."""
    h, w = float(h), float(w)
    items = []
    for k, (labels, boxes, _) in enumerate(reads):
        for lab, (x1, x2) in zip(labels, boxes):
            x1, x2 = float(x1), float(x2)
            if not (math.isfinite(x1) and math.isfinite(x2)):
                continue
            if x1 > x2:
                x1, x2 = x2, x1
            x1, x2 = min(max(x1, 0.0), w), min(max(x2, 0.0), w)
            if x2 - x1 >= 1.0:
                items.append([int(lab), x1, x2, k])
    items.sort(key=lambda it: it[1] + it[2])                                # stable: ties stay in probe order
    kept = []
    for it in items:
        if kept and kept[-1][3] != it[3] and kept[-1][0] == it[0]:
            p = kept[-1]
            shared = min(p[2], it[2]) - max(p[1], it[1])
            if shared > 0.5 * min(p[2] - p[1], it[2] - it[1]):
                continue                                                   # one glyph, seen on both sides of an ownership boundary
        kept.append(it)
    for a, b in zip(kept, kept[1:]):
        if a[2] > b[1]:                                                    # they overlap: both end at the middle of what they share
            m = (max(a[1], b[1]) + min(a[2], b[2])) / 2.0
            m = max(m, a[1])                                               # b ends left of what is left of a: a keeps nothing, b starts there
            a[2], b[1], b[2] = m, m, max(b[2], m)
    kept = [it for it in kept if it[2] - it[1] >= 1.0]
    return [it[0] for it in kept], [[it[1], 0.0, it[2], h] for it in kept]


def decode(sizes, probes, rows, locs):
    """the host half of a reading, shared by ``read_host`` and ``MarconetPipeline.read_lines``: ``sizes[i]`` = (h, w) of line i, ``probes[i]`` its
    ``plan_probes``, ``rows`` / ``locs`` the argmax indices [ΣP, 64] and the fp32 (left, right) pairs [ΣP, 32] of all probes in line order →
    per line dict(text, labels, boxes, probes, overflow), None for an empty reading"""
    out, j = [], 0
    for (h, w), pr in zip(sizes, probes):
        reads = [read_probe(rows[j + k], locs[j + k], p, h) for k, p in enumerate(pr)]
        j += len(pr)
        labels, boxes = merge(h, w, reads)
        out.append(dict(text=lq_io.text_from_labels(labels), labels=labels, boxes=boxes, probes=list(pr), overflow=any(r[2] for r in reads))
                   if labels else None)
    return out


def encode(pipe, lq):
    """the encoder on a batch of probes → (argmax indices, list of ΣP rows of 64 ints; the (left, right) pairs, fp32 numpy [ΣP, 32]): one forward,
    ``clear_labels_batch``'s argmax, ONE device→host copy of both (an index < 6736 is exact in fp32)"""
    logits, locs_lr, _ = pipe.encoder(lq)
    B, T, C = logits.shape
    with ops.on_device(logits):
        idx = ops.argmax_rows(logits.reshape(B * T, C).contiguous().float()).reshape(B, T)
    both = torch.cat([idx.to(torch.float32), locs_lr.reshape(B, -1).float()], dim=1).cpu().numpy()          # the one device→host copy
    return both[:, :T].astype(np.int64).tolist(), np.ascontiguousarray(both[:, T:])


def line_probes(sizes, probe_width=384):
    """``plan_probes`` per line; a refusal names the line"""
    probes = []
    for i, (h, w) in enumerate(sizes):
        try:
            probes.append(plan_probes(h, w, probe_width))
        except ValueError as e:
            raise type(e)("line %d: %s" % (i, e)) from None
    return probes


@torch.no_grad()
def read_host(pipe, images, probe_width=384):
    """the definition of ``MarconetPipeline.read_lines``: the probes' crops taken on the host and resized by ``lq_device.prepare_strips`` (one batch
    in probe order), the encoder on that batch, ``read_probe`` and ``merge`` → what ``read_lines`` returns, to be compared with ``==``"""
    sizes = [(int(img.shape[0]), int(img.shape[1])) for img in images]
    probes = line_probes(sizes, probe_width)
    if not images:
        return []
    crops = [np.ascontiguousarray(img[:, p[0]:p[1]]) for img, pr in zip(images, probes) for p in pr]
    prep = lq_device.prepare_strips(crops, next(pipe.sr.parameters()).device)
    rows, locs = encode(pipe, prep.lq)
    return decode(sizes, probes, rows, locs)
