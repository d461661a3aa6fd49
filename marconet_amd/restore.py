"""The restore front end of ``MarconetPipeline``: strips, images, panels, whole lines, pages of four kinds of region, and the blind reading of
lines, regions and columns — everything between a caller's pixels and ``_restore_batch``, and back to the caller's page.  ``RestoreFrontEnd`` is
a mixin; the page path's packed layout (``page_layout``) and its per-kind questions (``region_geometry``, ``region_details``) are plain functions
that need no device."""
import collections
import contextlib

import numpy as np
import torch

from . import blind, blind_columns as bc, columns as cl, curves as cv, ink, layout, long_lines, lq_device, lq_io, ops, pages, panel_device, quads as qd, \
    regions as rg, skew
from .labels import clear_labels_batch, collapse_indices, locs_from_left_right, prepared_rows, script_skips


@contextlib.contextmanager
def _named(who):
    """a ValueError raised inside is re-raised with ``who`` in front: "<who>: <its message>" """
    try:
        yield
    except ValueError as e:
        raise ValueError("%s: %s" % (who, e)) from None


def page_to_device(image, device):
    """the one copy of the page: uint8 RGB [H, W, 3] on ``device``"""
    return torch.from_numpy(np.ascontiguousarray(image)).to(device)


def boxes_in_crop(char_boxes, box):
    """character boxes in page pixels → in the crop of ``box`` (None stays None)"""
    return None if char_boxes is None else [[c[0] - box[0], c[1] - box[1], c[2] - box[0], c[3] - box[1]] for c in char_boxes]


def region_details(rec, with_kind=False):
    """what ``details`` reports of region ``rec`` beside its plan, whichever entry point asks: ``rect`` for a line, ``rect``, ``cuts`` and ``widths``
    for a restored column, ``quad`` / ``polygon`` (the points in the result) and ``size`` (rw, rh) for a quadrilateral / a curve; ``with_kind``:
    also ``kind`` (``restore_page_regions``)"""
    if rec["kind"] == "quad":
        d = dict(quad=rec["out_quad"], size=(rec["rw"], rec["rh"]))
    elif rec["kind"] == "curve":
        d = dict(polygon=rec["out_polygon"], size=(rec["rw"], rec["rh"]))
    elif "widths" in rec:
        d = dict(rect=rec["rect"], cuts=rec["cuts"], widths=rec["widths"])
    else:
        d = dict(rect=rec["rect"])
    return dict(d, kind=rec["kind"]) if with_kind else d


def region_geometry(recs, char_boxes):
    """``recs[i]``: region i's record as ``regions.normalize_regions`` gives it; ``char_boxes[i]`` its character boxes in PAGE pixels, ``{"crop":
    boxes}`` for boxes in its crop already, or None → (per region the (h, w) of its crop — a restored column's virtual strip —, its character
    boxes in the crop, a quadrilateral's crop map).  A kind's ValueError names the region."""
    sizes, local, maps = [], [None] * len(recs), [None] * len(recs)
    for i, r in enumerate(recs):
        cb = None if char_boxes is None else char_boxes[i]
        with _named("region %d" % i):
            if r["kind"] == "column" and "widths" in r:
                sizes.append((cl.LQ_H, sum(r["widths"])))
                local[i] = cl.virtual_boxes(r["widths"])
            elif r["kind"] in ("line", "column"):
                sizes.append((r["box"][3] - r["box"][1], r["box"][2] - r["box"][0]))
                local[i] = cb["crop"] if isinstance(cb, dict) else boxes_in_crop(cb, r["box"])
            else:
                sizes.append((r["ch"], r["cw"]))
                if r["kind"] == "quad":
                    maps[i] = qd.quad_map(r["quad"], r["cw"], r["ch"])
                if isinstance(cb, dict):                        # boxes in the rectified crop already: what ``details`` reports of a region that was read
                    local[i] = cb["crop"]
                elif cb is not None:
                    local[i] = qd.char_boxes_in_crop(cb, maps[i], r["cw"], r["ch"]) if r["kind"] == "quad" else \
                        cv.char_boxes_in_crop(cb, r["segs"], r["cw"], r["ch"])
    return sizes, local, maps


# the packed layout of a page's windows (``page_layout``): ``views``: the lines' windows that are views of the page, (byte offset, pitch, h, w) each,
# in ``view_keys``' order; ``crops``: the lines' host crops at the buffer's head, (byte offset, row slice, column slice of the page) each, ``head``
# bytes in all; ``cell_tab``: ``columns.gather_table``'s records; ``q_tab`` from byte ``q_base`` and ``c_tab`` / ``c_segs`` from ``c_base``: the
# quadrilaterals' and the curves' crop tables; ``nbytes``: the buffer's size; ``slots``: {(region, k): ((h, w), byte offset)} of every packed
# window, in the caller's order; ``have``: the keys of the ``lq`` rows as they are produced — the views, then the slots —; ``order``: the produced
# row that the caller's j-th window is, None where the rows are produced in the caller's order
PageLayout = collections.namedtuple("PageLayout", "views view_keys crops head cell_tab q_tab q_base c_tab c_segs c_base nbytes slots have order")


def page_layout(recs, maps, page_w, lines_as_views, windows):
    """Where every window of a page sits — host arithmetic only, nothing is copied or launched.  ``recs`` / ``maps`` as ``region_geometry`` takes and
    gives them; ``windows``: (region i, index k, c0, c1) — the columns [c0, c1) of region i's crop —, for a column (i, k, c0, c1, g0, g1): its
    cells [g0, g1) as well, what ``columns.gather_table`` reads of a ``long_lines.Window``.  A line's window is a view of the page
    (``lines_as_views``) or a host crop at the head of the one ragged buffer; behind the head the columns', the quadrilaterals' and the curves'
    windows, each kind contiguous from its own base → ``PageLayout``.  ``gather_table``'s refusals are raised here."""
    W, of = int(page_w), lambda kind: [w for w in windows if recs[w[0]]["kind"] == kind]
    views, crops, slots, head, col_plans = {}, [], {}, 0, {}
    for i, k, c0, c1 in of("line"):
        x1, y1, _, y2 = recs[i]["box"]
        if lines_as_views:
            views[(i, k)] = ((y1 * W + x1 + int(c0)) * 3, 3 * W, y2 - y1, int(c1) - int(c0))
            continue
        crops.append((head, slice(y1, y2), slice(x1 + c0, x1 + c1)))
        slots[(i, k)] = ((y2 - y1, c1 - c0), head)
        head += 3 * (y2 - y1) * (c1 - c0)
    for i, k, c0, c1, g0, g1 in of("column"):
        col_plans.setdefault(i, []).append((k, long_lines.Window(c0, c1, g0, g1, 0, 0)))
    cell_tab, shapes, offsets, q_base = cl.gather_table([(recs[i]["box"], recs[i]["cuts"], recs[i]["widths"], [p for _, p in plan])
                                                         for i, plan in col_plans.items()], head)
    slots.update(zip([(i, k) for i, plan in col_plans.items() for k, _ in plan], zip(shapes, offsets)))
    q_wins, c_wins = of("quad"), of("curve")
    size = lambda w: (w[3] - w[2], recs[w[0]]["ch"])
    q_tab, c_base = qd.crop_table([maps[w[0]] for w in q_wins], [size(w) for w in q_wins], [w[2] for w in q_wins], q_base)
    c_tab, c_segs, nbytes = cv.crop_table([recs[w[0]]["segs"] for w in c_wins], [size(w) for w in c_wins], [w[2] for w in c_wins], c_base)
    for w, off in zip(q_wins + c_wins, q_tab["offset"].tolist() + c_tab["offset"].tolist()):
        slots[w[:2]] = (size(w)[::-1], int(off))
    want = [w[:2] for w in windows]
    view_keys = [key for key in want if key in views]
    slots = {key: slots[key] for key in want if key in slots}
    have = view_keys + list(slots)
    at = {key: j for j, key in enumerate(have)}
    return PageLayout([views[key] for key in view_keys], view_keys, crops, head, cell_tab, q_tab, q_base, c_tab, c_segs, c_base, nbytes, slots, have,
                      None if have == want else [at[key] for key in want])


def page_windows_lq(layout, page_d, image):
    """the encoder input of the windows of a ``PageLayout``, fp32 [n,3,32,512] in the caller's order: ``page_d`` the page on the device, ``image``
    the same page on the host (the lines' crops are cut from it).  At most one gather / crop launch per kind into the one ragged buffer, the one
    upload of the host crops, ``lq_device.prepare_windows`` for the views, ``lq_device.prepare_packed`` for the buffer — each only where it has work."""
    dev, parts = page_d.device, []
    if layout.slots:
        packed = torch.empty((layout.nbytes,), dtype=torch.uint8, device=dev)                  # the ragged batch of every kind's windows
        with ops.on_device(page_d):
            if len(layout.cell_tab):
                ops.column_gather_u8(page_d, ops.table_to_device(layout.cell_tab, dev), int(layout.cell_tab["dw"].max()), cl.LQ_H, packed)
            if len(layout.q_tab):
                ops.quad_crop_u8(page_d, ops.table_to_device(layout.q_tab, dev), int(layout.q_tab["w"].max()), int(layout.q_tab["h"].max()), packed)
            if len(layout.c_tab):
                ops.curve_crop_u8(page_d, ops.table_to_device(layout.c_tab, dev), ops.table_to_device(layout.c_segs, dev), int(layout.c_tab["w"].max()),
                                  int(layout.c_tab["h"].max()), packed)
        if layout.crops:                                                                       # the lines' crops: the one upload beside the page's
            packed[:layout.head].copy_(torch.from_numpy(np.concatenate([np.ascontiguousarray(image[ys, xs]).reshape(-1) for _, ys, xs in layout.crops])))
    if layout.views:
        parts.append(lq_device.prepare_windows(page_d.reshape(-1), layout.views).lq)
    if layout.slots:
        parts.append(lq_device.prepare_packed(packed, [hw for hw, _ in layout.slots.values()], [off for _, off in layout.slots.values()]).lq)
    rows = parts[0] if len(parts) == 1 else torch.cat(parts)
    return rows if layout.order is None else rows.index_select(0, torch.tensor(layout.order, dtype=torch.int64, device=dev))


class RestoreFrontEnd:
    """The restore and read entry points of ``MarconetPipeline``, which inherits them.  Of the inference core this mixin takes five things and
    nothing else of ``self``: ``self.encoder``, ``self._restore_batch``, ``self._require_prior_image``, the generator's ``class_num`` and the
    device the networks are on.  (``forward_blind`` is the core's own ``forward_batch`` on what the encoder reads.)"""

    def _device(self):
        return next(self.sr.parameters()).device

    def _kept(self, strips):
        """positions of the strips the script would restore (a strip that is None was too wide: ``_strips_from_images``)"""
        return [i for i, s in enumerate(strips) if s is not None and not script_skips(s["labels"], self.gan.TextGenerator.class_num)]

    def _show_sr(self, lq, strips, keep, with_prior):
        """``restore_strips``' result for ``strips``, of which the strips ``keep`` are restored; ``lq``: their rows, on the device"""
        out = [None] * len(strips)
        if not keep:
            return out
        kept = [strips[i] for i in keep]
        y, prior = self._restore_batch(lq, [s["labels"] for s in kept], [s["locs"] for s in kept], with_prior)
        y = y.cpu().numpy()
        if with_prior:
            prior = (prior[..., :3] * 0.5 + 0.5).cpu().numpy()                              # test_sr.py:208, on the NHWC images
        g = 0
        for k, (i, s) in enumerate(zip(keep, kept)):
            out[i] = y[k, :, :s["show_w"], :]
            if with_prior:
                n = int(s["labels"].shape[0])
                out[i] = (out[i], prior[g:g + n].transpose(1, 0, 2, 3).reshape(128, 128 * n, 3))   # hstack of the n images (:209-211)
                g += n
        return out

    @torch.no_grad()
    def restore_strips(self, strips, with_prior=False):
        """The body of test_sr.py's ``for img_name`` loop (:77-201) for a list of strips prepared by ``lq_io.strip_from_png``
        (dicts with lq [1,3,32,512], labels int64 [n,1], locs [1,2n], show_w) — as ONE batch.  → list of uint8 BGR arrays
        [128, show_w, 3] on the host (``ShowSR``, test_sr.py:198-201: the post-processed SR result cropped to the content
        width); ``None`` for a strip the script would skip (a character outside the alphabet → label −1 → the generator
        raises, test_sr.py:181-190; no character at all, :168-170).
        ``with_prior=True`` → list of ``(ShowSR, prior128)``: ``prior128`` = the strip's structure images side by side, float32 RGB
        [128, 128·n, 3] = ``np.hstack`` of ``prior_cha * 0.5 + 0.5`` (test_sr.py:208-211) — the array the script hands to ``cv2.resize``
        for the panel's last row (:212; cv2 is not part of this build, the resize stays with the caller).  It is taken from the
        generator's NHWC images as ``_core`` leaves them — the fp32 values of ``forward_batch(return_prior=True)``'s NCHW tensor."""
        keep = self._kept(strips)
        lq = torch.cat([strips[i]["lq"] for i in keep]).to(self._device()) if keep else None
        return self._show_sr(lq, strips, keep, with_prior)

    @torch.no_grad()
    def restore_images(self, images, texts=None, boxes=None, with_prior=False, max_glyphs=16, details=False):
        """``restore_strips`` from RAW strips: ``images`` is a list of uint8 RGB HxWx3 arrays (``lq_io.load_png``, a detector's crops), and the
        script's input pre-processing (test_sr.py:98-115) runs on the device for the whole batch (``lq_device.prepare_strips``: one kernel
        launch, one copy of the pixels) instead of per strip in host numpy.  → what ``restore_strips`` returns for
        ``lq_io.strip_from_png`` of the same strips, the same bytes; ``None`` for a strip the script skips (wider than 512 px at height 32,
        :108-110; no character, :168-170; a character outside the alphabet, :181-190).
        ``texts`` (one string per image): labels through the alphabet and one evenly spaced box per character, or ``boxes[i]`` where given —
        as ``lq_io.strip_from_png``, except that an empty text gives ``None`` (the script's skip, :168-170) where ``strip_from_png`` raises.  ``texts=None``: labels (at most ``max_glyphs``) and locations come from the encoder itself, as in
        ``forward_blind``.
        ``details=True`` → ``(results, strips)``: per image also the dict ``restore_strips`` consumed (lq on the device, labels, locs, text,
        content_w, show_w) plus ``show``, the uint8 RGB preview [128, show_w, 3] (``lq_io.show_lq``, resized on the device); None where skipped."""
        prep, strips = self._strips_from_images(images, texts, boxes, max_glyphs, preview=details, host_preview=details)
        keep = self._kept(strips)
        out = self._show_sr(prepared_rows(prep, keep)[1], strips, keep, with_prior)
        return (out, strips) if details else out

    @torch.no_grad()
    def restore_panels(self, images, texts=None, boxes=None, max_glyphs=16, details=False):
        """``restore_images`` up to the file the script saves (test_sr.py:203-232): per image the panel — preview | preview with box marks | SR |
        structure images — as a uint8 RGB host array [512, show_w, 3], the bytes of ``lq_io.panel_rgb_u8(lq_io.panel(...))`` of what
        ``restore_images(..., with_prior=True, details=True)`` returns (``Image.fromarray(panel).save(path)`` writes ``lq_io.save_panel``'s file);
        ``None`` where ``restore_images`` gives ``None``.  ``images`` / ``texts`` / ``boxes`` / ``max_glyphs`` as there.
        Nothing per pixel happens on the host: the preview, the uint8 SR output and the generator's structure images stay on the device, one
        launch composes all panels (``panel_device.compose_panels``) and ONE device→host copy brings them back.
        ``details=True`` → ``(panels, strips)``: per image also the dict of its inputs (``text`` for the file name), None where too wide."""
        self._require_prior_image("restore_panels")
        prep, strips = self._strips_from_images(images, texts, boxes, max_glyphs, preview=True, host_preview=False)
        keep = self._kept(strips)
        out = [None] * len(images)
        if keep:
            kept = [strips[i] for i in keep]
            rows, lq = prepared_rows(prep, keep)
            labels, locs_rows, show_w = [s["labels"] for s in kept], [s["locs"] for s in kept], [s["show_w"] for s in kept]
            y, prior = self._restore_batch(lq, labels, locs_rows, with_prior=True)
            panels = panel_device.compose_panels(prep.preview, rows, show_w, y, prior, [int(l.shape[0]) for l in labels], [r[0] for r in locs_rows])
            panels = panels.cpu().numpy()                                                            # the one device→host copy
            for k, i in enumerate(keep):
                out[i] = panels[k, :, :show_w[k], :]
        return (out, strips) if details else out

    @torch.no_grad()
    def restore_lines(self, images, texts, boxes=None, max_glyphs=16, overlap_glyphs=2, details=False, probe_width=384):
        """Whole text lines, however wide: what the script tells its user to do by hand for a strip wider than 512 px at height 32 ("crop it into
        shorter segments", test_sr.py:108-110) and the joining it leaves to them.  ``images``: uint8 RGB HxWx3 arrays; ``texts[i]``: the line's
        characters; ``boxes[i]``: its character boxes in source pixels, or evenly spaced ones.  Per line ``long_lines.plan_windows`` cuts windows of
        at most ``max_glyphs`` whole characters, consecutive ones sharing ``overlap_glyphs``; the crops are taken on the host, each with its slice
        of the text and its boxes shifted into the crop, and ALL windows of ALL lines are restored as one batch exactly as ``restore_images``
        restores strips (``lq_device.prepare_strips``, the same labels and locs, one forward, the finiteness check).  One launch then joins every
        line on the device (``long_lines.compose_lines``: the bytes of ``long_lines.stitch_host``) and ONE device→host copy brings them back.
        → per image a uint8 BGR array [128, out_w, 3] (a line that fits one window: ``restore_images``' own bytes); ``None`` for a line with no
        character or with a character outside the alphabet — ``restore_strips``' decisions, applied to the line as a whole.
        ``None`` as a line's entry of ``texts`` means "read it" (``blind``'s head states the reading; ``read_lines`` returns it) — ``[None] *
        len(images)`` reads every line.  ``texts`` itself stays required: ``texts=None`` is refused as it always was here (a caller who forgot
        the texts is told so; the page entry points, where the boxes are the caller's statement, take ``texts=None`` as a None per region).  The
        lines are uploaded once, packed one behind the other, and every probe window of every line that is read goes through the encoder as ONE
        batch of views of them (``lq_device.prepare_windows``).  A line of one probe takes its labels (at most ``max_glyphs``) and ``preds_locs``
        straight from the encoder, as ``restore_images(texts=None)`` does — a call that holds only such lines gives its bytes —; a line of several
        probes is read, and its text and boxes are planned as given ones are (``plan_windows``' ValueErrors name the line).  The planned windows
        are then views of the uploaded lines too.  An empty reading gives ``None``.  With every text given nothing changes.
        ``details=True`` → ``(lines, plans)``; where a text was ``None``, ``(lines, plans, readings)``: per line that was read a dict with ``text``,
        ``boxes`` (source pixels) and ``overflow`` (a probe held more than the encoder's 16 characters), None for the others."""
        if texts is None:
            raise ValueError("restore_lines needs texts: a window is a run of whole characters, and windows cut blind would cut characters in half "
                             "(restore_images(texts=None) reads a strip of at most 512 px at height 32 without them) — None as a line's ENTRY of "
                             "texts has the encoder read that line: [None] * len(images) reads them all")
        joined, plans, live, read = self._joined_lines(images, texts, boxes, max_glyphs, overlap_glyphs, "restore_lines", "image", probe_width)
        out = [None] * len(images)
        if live:
            joined = joined.cpu().numpy()                                                         # the one device→host copy
            for l, i in enumerate(live):
                out[i] = joined[l, :, :long_lines.plan_out_w(plans[i]), :]
        if details and read is not None:
            return out, plans, [self._reading_details(read.get(i)) for i in range(len(images))]
        return (out, plans) if details else out

    @torch.no_grad()
    def read_lines(self, images, probe_width=384):
        """What the encoder reads in whole text lines, however wide: per image dict(text, labels, boxes [[x1, 0, x2, h]] in source pixels, probes,
        overflow), None for an empty reading — ``blind.read_host``'s result, ``==`` (``blind``'s head states the rules).  ONE upload of the lines
        packed one behind the other, ONE ``mnet_lq_windows_u8`` launch over all probes of all lines (views: overlapping probes share their
        pixels), ONE encoder forward and ONE device→host copy of the indices and the locations; the merge, a few hundred short rows, runs on
        the host."""
        sizes = [tuple(int(v) for v in np.shape(img)[:2]) for img in images]
        src, offsets = lq_device.upload_lines(images, self._device())
        probes = blind.line_probes(sizes, probe_width)
        if not images:
            return []
        wins = [lq_device.line_window(offsets[i], h, w, p[0], p[1]) for i, (h, w) in enumerate(sizes) for p in probes[i]]
        rows, locs = blind.encode(self, lq_device.prepare_windows(src, wins).lq)
        return blind.decode(sizes, probes, rows, locs)

    @torch.no_grad()
    def read_columns(self, image, boxes, scale=4, probe_width=384):
        """What the encoder reads in vertical text columns whose text is unknown: ``image`` uint8 RGB [H, W, 3], ``boxes[i]`` column i's box
        [x1, y1, x2, y2] in page pixels (rounded outward: ``pages.round_box``) → per column dict(text, labels, char_boxes [[x1, ya, x2, yb]] in
        PAGE pixels top to bottom, cuts — ``columns.cell_cuts`` of that reading —, first_cuts, probes, overflow), None for an empty reading:
        ``blind_columns.read_columns_host``'s result, ``==`` (``blind_columns``' head states the rules).  ``scale``: the scale of the restoration the
        reading is meant for — ``settle`` drops characters whose cells it could not paste.  ONE upload of the page, ONE ``mnet_row_ink_u8`` launch
        over all columns as views of the page, one device→host copy of all profiles, the first-pass cells and the probes on the host, ONE
        ``mnet_column_gather_u8`` launch for every probe of every column (``columns.gather_table``, the probes as windows),
        ``lq_device.prepare_packed``, ONE encoder forward and ``blind.encode``'s one copy back.  ValueError for a scale outside 1..8 and for a box
        that is empty or outside the page, before anything is copied."""
        image = pages._page_array(image)
        boxes = bc.check_boxes(image.shape[0], image.shape[1], boxes, scale)
        if not boxes:
            return []
        return self._read_columns(page_to_device(image, self._device()), boxes, scale, probe_width)

    def _read_columns(self, page_d, boxes, scale, probe_width, regions=None):
        """``read_columns`` of a page that is on the device: ``page_d`` uint8 RGB [H, W, 3], ``boxes``: integer boxes inside it; ``regions[k]``: the
        number a refusal gives column k"""
        plans = bc.plan_columns(boxes, ink.row_profiles(page_d.reshape(-1), int(page_d.shape[1]), boxes), probe_width, regions)
        packed, shapes, offsets = cl.gather_columns(page_d, [(p["box"], p["first_cuts"], p["widths"], bc.probe_windows(p["probes"])) for p in plans])
        rows, locs = blind.encode(self, lq_device.prepare_packed(packed, shapes, offsets).lq)
        return bc.decode(plans, rows, locs, scale)

    @torch.no_grad()
    def find_lines(self, image, text_h=None, floor=layout.DEFAULT_FLOOR, pad=None, min_h=None, min_w=None, max_h=None):
        """The text lines of a page nobody has boxed: ``image`` uint8 RGB [H, W, 3] → dict(boxes: integer [x1, y1, x2, y2] in page pixels, in
        reading order; tight; skipped; passes) — ``layout.find_lines_host``'s result, ``==`` (``layout``'s head states the rules — a recursive XY-cut
        over ink profiles above the noise floor ``floor`` — the defaults, and what is out of scope: anything but horizontal lines in columns
        on plain paper, and any claim of detection quality; a page skewed as a whole is ``find_lines_skewed``'s).  ONE upload of the page; per pass of the cut ONE ``mnet_box_ink_u8`` launch over all
        current boxes as views of the page and one device→host copy of their profiles; the cuts, a few thousand integers, run on the host through
        the same ``layout.xy_cut``.  With the networks on no HIP device the host definition runs.  TypeError for a page that is not uint8
        RGB HxWx3, ValueError for ``layout.line_params``' refusals, before anything is copied."""
        image = pages._page_array(image)
        with _named("find_lines"):
            params = layout.line_params(image.shape[0], text_h, floor, pad, min_h, min_w, max_h)
        if self._device().type != "cuda":
            return layout.find_lines_host(image, **params)
        return self._find_lines(page_to_device(image, self._device()), params)

    def _find_lines(self, page_d, params):
        """``find_lines`` of a page that is on the device: ``page_d`` uint8 RGB [H, W, 3], ``params``: ``layout.line_params``' dict"""
        H, W, flat = int(page_d.shape[0]), int(page_d.shape[1]), page_d.reshape(-1)
        return layout.lines_from_profiles(lambda boxes, axis: ink.box_profiles(flat, W, boxes, params["floor"], axis), H, W, params)

    @torch.no_grad()
    def estimate_skew(self, image, floor=layout.DEFAULT_FLOOR, max_slope=6144):
        """The skew of a scanned page: ``image`` uint8 RGB [H, W, 3] → dict(slope: Q16, the text runs along (1, slope / 65536); scores: [(m, S(m))]
        of every candidate) — ``skew.estimate_host``'s result, ``==`` (``skew``'s head states the rule, Postl's criterion on the row profiles of a
        sheared frame, its two stages and its defaults, which are design choices).  ONE upload of the page; per stage ONE ``mnet_skew_ink_u8`` launch
        whose table is the page's frame box at every candidate slope, rows only, and one device→host copy of the profiles; the scores are Python
        integers, computed on the host.  With the networks on no HIP device the host definition runs.  TypeError for a page that is not uint8
        RGB HxWx3, ValueError for ``skew.estimate_params``' refusals, before anything is copied.  Not covered: skew beyond ``max_slope`` (at most
        8192, about 7 degrees), 90 / 180 degree orientation, perspective, per-block skew, and the estimate's quality on real scans."""
        image = pages._page_array(image)
        with _named("estimate_skew"):
            params = skew.estimate_params(floor, max_slope)
        if self._device().type != "cuda":
            return skew.estimate_host(image, **params)
        return self._estimate_skew(page_to_device(image, self._device()), params)

    def _estimate_skew(self, page_d, params):
        """``estimate_skew`` of a page that is on the device; ``params``: ``skew.estimate_params``' dict"""
        H, W = int(page_d.shape[0]), int(page_d.shape[1])
        return skew.estimate(lambda slopes: [rows for rows, _ in ink.frame_profiles(page_d, [(skew.frame_box(H, W, m), m, False) for m in slopes],
                                                                                       params["floor"])], params)

    @torch.no_grad()
    def find_lines_skewed(self, image, slope=None, text_h=None, floor=layout.DEFAULT_FLOOR, pad=None, min_h=None, min_w=None, max_h=None):
        """``find_lines`` for a page that was scanned skewed: ``image`` uint8 RGB [H, W, 3] → dict(slope, frame_boxes, tight, quads, skipped, passes,
        scores) — ``skew.find_lines_host``'s result, ``==`` (``skew``'s head states the rules: ``layout``'s cut in the coordinates of a frame sheared
        by ``slope``, Q16; ``quads[i]``: the four page corners of line i, what ``restore_page_quads`` takes).  ``slope=None``: ``estimate_skew`` runs
        first, on the same upload.  Per pass of the cut ONE ``mnet_skew_ink_u8`` launch over all current frame boxes and one device→host copy of
        their profiles; the cuts run on the host through the same ``layout.xy_cut``.  With the networks on no HIP device the host definition runs.
        TypeError for a page that is not uint8 RGB HxWx3, ValueError for ``layout.line_params``' refusals and a ``slope`` that is no integer within
        ±8192, before anything is copied.  Not covered: what ``estimate_skew`` and ``find_lines`` do not cover."""
        image = pages._page_array(image)
        with _named("find_lines_skewed"):
            params = layout.line_params(image.shape[0], text_h, floor, pad, min_h, min_w, max_h)
            slope = None if slope is None else skew.check_slope(slope)
        if self._device().type != "cuda":
            return skew.find_lines_host(image, slope, **params)
        return self._find_lines_skewed(page_to_device(image, self._device()), params, slope)

    def _find_lines_skewed(self, page_d, params, slope):
        """``find_lines_skewed`` of a page that is on the device; ``slope``: checked, or None"""
        est = dict(slope=slope, scores=[]) if slope is not None else self._estimate_skew(page_d, skew.estimate_params(params["floor"]))
        m = est["slope"]

        def profiles(boxes, axis):
            return [p[axis] for p in ink.frame_profiles(page_d, [(b, m, axis == layout.AXIS_X) for b in boxes], params["floor"])]
        return skew.lines_from_frame_profiles(profiles, int(page_d.shape[0]), int(page_d.shape[1]), m, params, est["scores"])

    def _blind_columns_first(self, who, image, blind_at, blind_columns, precheck, texts, char_boxes, restored, scale, probe_width):
        """the pre-pass of the two entry points that take columns: ``blind_at``: the positions of the columns whose text is None.  A column's
        cells are cut from its text, one per character, so without ``blind_columns`` such a column is refused.  With it: ``precheck()`` — the
        refusals that need no pixel; it returns every region's integer box —, the one copy of the page, ``_read_columns``, and the readings' text
        and character boxes stand in for given ones → (the page on the device, to be shared with ``_restore_page_records``, None where nothing
        was read; texts; char_boxes; ``restored`` with the columns that were read judged by their reading's text; {position: reading}).  An empty
        reading leaves the text "": the column keeps the background."""
        if not blind_at:
            return None, texts, char_boxes, restored, {}
        if not blind_columns:
            raise ValueError("%s: region %d: a column needs its text (its cells are cut from it, one per character): only horizontal lines, "
                             "quadrilaterals and curves are read where the text is None" % (who, blind_at[0]))
        with _named(who):
            boxes = precheck()
        page_d = page_to_device(image, self._device())
        with _named(who):
            readings = self._read_columns(page_d, [boxes[i] for i in blind_at], scale, probe_width, blind_at)
        texts, char_boxes = list(texts), [None] * len(texts) if char_boxes is None else list(char_boxes)
        for i, r in zip(blind_at, readings):
            texts[i], char_boxes[i] = ("", None) if r is None else (r["text"], r["char_boxes"])
        n_cls = self.gan.TextGenerator.class_num
        restored = [not script_skips(lq_io.label_tensor(texts[i]), n_cls) if i in blind_at else r for i, r in enumerate(restored)]
        return page_d, texts, char_boxes, restored, dict(zip(blind_at, readings))

    @staticmethod
    def _column_reading_details(extra, read):
        """what ``details`` adds for a column that was read: ``text``, ``char_boxes`` (page pixels), ``first_cuts`` and ``overflow``"""
        return [e if read.get(i) is None else dict(e, **{k: read[i][k] for k in ("text", "char_boxes", "first_cuts", "overflow")}) for i, e in enumerate(extra)]

    @staticmethod
    def _reading_details(r, dx=0.0, dy=0.0):
        """what ``details`` reports of a reading (None stays None): text, boxes — moved by (dx, dy) — and overflow"""
        return None if r is None else dict(text=r["text"], boxes=[[b[0] + dx, b[1] + dy, b[2] + dx, b[3] + dy] for b in r["boxes"]], overflow=r["overflow"])

    @staticmethod
    def _region_probes(sizes, need, probe_width, who, what):
        """``blind.plan_probes`` of every line (region) of ``need``, {i: probes}; a refusal names ``who`` and the line"""
        probes = {}
        for i in need:
            with _named("%s: %s %d" % (who, what, i)):
                probes[i] = blind.plan_probes(sizes[i][0], sizes[i][1], probe_width)
        return probes

    def _read_regions(self, sizes, need, probes, lq, max_glyphs):
        """the reading pass of the restore entry points: ``need``: the lines (regions) whose text is None; ``lq``: the encoder input of their
        probes (``probes[i]``: ``_region_probes``' of line i), fp32 [ΣP,3,32,512] in ``need``'s order → {i: reading}.  A line of
        several probes: ``blind.decode``'s dict, None for an empty reading.  A line of one probe: labels (int64 [n,1], at most ``max_glyphs``) and
        ``locs``, its ``preds_locs`` row, straight from the encoder as ``_strips_from_images(texts=None)`` takes them, beside text, boxes, overflow."""
        rows, locs = blind.encode(self, lq)
        read, j = {}, 0
        for i in need:
            (h, w), pr = sizes[i], probes[i]
            if len(pr) > 1:
                read[i] = blind.decode([sizes[i]], [pr], rows[j:j + len(pr)], locs[j:j + len(pr)])[0]
            else:
                lab = collapse_indices(rows[j])
                labels = torch.tensor(lab, dtype=torch.int64).reshape(-1, 1)[:max_glyphs]
                n = int(labels.shape[0])
                lr = torch.from_numpy(np.array(locs[j:j + 1], dtype=np.float32))
                edges = [(float(lr[0, 2 * g]) * 512 * h / 32, float(lr[0, 2 * g + 1]) * 512 * h / 32) for g in range(min(n, blind.SLOTS))]
                read[i] = dict(labels=labels, locs=locs_from_left_right(lr)[:, :2 * n].contiguous(), text=lq_io.text_from_labels(labels.flatten().tolist()),
                               boxes=[[min(a, b), 0.0, max(a, b), float(h)] for a, b in edges], probes=list(pr), overflow=len(lab) > n)
            j += len(pr)
        return read

    def _joined_lines(self, images, texts, boxes, max_glyphs, overlap_glyphs, who, what, probe_width=384):
        """``restore_lines`` up to the joined lines on the device: → (uint8 BGR [L,128,max out_w,3] — ``long_lines.compose_lines`` of the L lines
        that are restored, or None where there is none —, the plan per image (None for a line that is skipped), the positions of the L lines in
        ``images``, and — where a text is None — the readings, {position: ``_read_regions``' entry}, else None).  ``who`` / ``what`` name the entry
        point and its unit ("image", "region") in the errors.  With every text given the windows' crops are taken on the host; with a text to read
        the lines are uploaded once and the probes and the planned windows are views of them (``lq_device.prepare_windows``)."""
        sizes = [tuple(int(v) for v in np.shape(img)[:2]) for img in images]
        dev = self._device()
        texts = self._texts_or_read(who, texts, len(images))
        need = [i for i, t in enumerate(texts) if t is None] if len(texts) == len(images) else []
        if not need:
            plans, labels, locs_rows, live = self._plan_lines(sizes, texts, boxes, max_glyphs, overlap_glyphs, who, what)
            if not live:
                return None, plans, live, None
            crops = [np.ascontiguousarray(images[i][:, p.c0:p.c1]) for i in live for p in plans[i]]
            prep = lq_device.prepare_strips(crops, dev)
            return self._restore_planned(prep.lq, labels, locs_rows, plans, live), plans, live, None
        probes = self._region_probes(sizes, need, probe_width, who, what)
        src, offsets = lq_device.upload_lines(images, dev)                                        # the one copy of the pixels
        view = lambda i, c0, c1: lq_device.line_window(offsets[i], sizes[i][0], sizes[i][1], c0, c1)
        read = self._read_regions(sizes, need, probes, lq_device.prepare_windows(src, [view(i, p[0], p[1]) for i in need for p in probes[i]]).lq, max_glyphs)
        plans, labels, locs_rows, live = self._plan_lines(sizes, texts, boxes, max_glyphs, overlap_glyphs, who, what, read)
        if not live:
            return None, plans, live, read
        prep = lq_device.prepare_windows(src, [view(i, p.c0, p.c1) for i in live for p in plans[i]])
        return self._restore_planned(prep.lq, labels, locs_rows, plans, live), plans, live, read

    def _plan_lines(self, sizes, texts, boxes, max_glyphs, overlap_glyphs, who, what, read=None):
        """the planning half of ``_joined_lines``, which needs no pixel: ``sizes[i]`` = (h, w) of line i, ``boxes[i]`` its character boxes in its own
        pixels (or None: evenly spaced ones) → (the plan per line, None for a line that is skipped; per window of the batch, in the plans' order,
        its label tensor and its ``preds_locs`` row; the positions of the lines that are restored).  ``read``: {i: the reading of a line whose text
        is None} (``_read_regions``): an empty one skips the line, a one-probe line is one window with the encoder's own labels and ``preds_locs``,
        a read line's labels and boxes stand in for the given ones."""
        if len(texts) != len(sizes):
            raise ValueError("%s: one text per %s expected (%d %ss, %d texts)" % (who, what, len(sizes), what, len(texts)))
        n_cls = self.gan.TextGenerator.class_num
        plans, labels, locs_rows = [None] * len(sizes), [], []
        for i, ((h, w), text) in enumerate(zip(sizes, texts)):
            r = None if read is None or i not in read else read[i]
            if text is None:
                if r is None:                                                  # an empty reading: the script's skip of an empty text
                    continue
                if "locs" in r:
                    if not script_skips(r["labels"], n_cls):
                        plans[i] = [long_lines.Window(0, w, 0, int(r["labels"].shape[0]), 0, int(lq_device.shape_geometry(h, w).show_w))]
                        labels.append(r["labels"])
                        locs_rows.append(r["locs"])
                    continue
                text = r["labels"]
            lab = lq_io.label_tensor(text)
            if script_skips(lab, n_cls):
                continue
            bx = r["boxes"] if r is not None else boxes[i] if boxes is not None and boxes[i] is not None else lq_io.evenly_spaced_boxes(len(text), w, h)
            with _named("%s: %s %d" % (who, what, i)):
                plans[i] = long_lines.plan_windows(h, w, bx, max_glyphs, overlap_glyphs)
            for p in plans[i]:
                labels.append(lab[p.g0:p.g1])
                locs_rows.append(lq_io.locs_from_boxes([[b[0] - p.c0, b[1], b[2] - p.c0, b[3]] for b in bx[p.g0:p.g1]], h))
        return plans, labels, locs_rows, [i for i, p in enumerate(plans) if p is not None]

    def _restore_planned(self, lq, labels, locs_rows, plans, live):
        """the restoring half of ``_joined_lines``: ``lq`` [ΣW,3,32,512] on the device, the encoder input of every window of the lines ``live`` in the
        plans' order → their joined lines, uint8 BGR [L,128,max out_w,3] on the device"""
        y, _ = self._restore_batch(lq, labels, locs_rows)
        return long_lines.compose_lines(y, [plans[i] for i in live])

    def _page_front(self, who, image, n, texts, per_region, expected, units):
        """the intake of the three ``restore_page*`` entry points, ``who``: the ``texts`` refusal, one text — and one entry of every list of
        ``per_region`` that is not None — per region (``n`` of them; the message says ``expected`` of ``units``), a uint8 RGB HxWx3 page (TypeError)
        → (the page as an array, per region whether it is restored: it has a character and none outside the alphabet, the texts as a list).
        ``texts=None`` stands for a None per region; a region whose text is None is read (``_restore_page_records``) and is checked as a restored
        one — whether it has a character is known only once the page is on the device."""
        texts = self._texts_or_read(who, texts, n)
        if len(texts) != n or any(l is not None and len(l) != n for l in per_region):
            raise ValueError("%s: %s expected (%d %s, %d texts)" % (who, expected, n, units, len(texts)))
        image = np.asarray(image)
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3 or image.size == 0:
            raise TypeError("%s: uint8 RGB HxWx3 page expected" % who)
        return image, [t is None or not script_skips(lq_io.label_tensor(t), self.gan.TextGenerator.class_num) for t in texts], list(texts)

    def _texts_or_read(self, who, texts, n):
        """``texts`` as a list, ``texts=None`` standing for a None — "read it" — per unit.  Reading is the encoder's work: with the networks on no
        HIP device a text that is None is refused here, before anything is copied, in the words this refusal always had"""
        texts = [None] * n if texts is None else texts
        if any(t is None for t in texts) and self._device().type != "cuda":
            raise ValueError("%s needs texts: a window is a run of whole characters, and windows cut blind would cut characters in half — a text "
                             "that is None is read by the encoder, which needs the networks on a HIP device (they are on %s)"
                             % (who, self._device()))
        return texts

    @staticmethod
    def _page_finish(plans, compose, details, extra):
        """the end of the three ``restore_page*`` entry points: ``compose(out_ws)`` → the finished page on the device, ``out_ws[i]`` the width of
        region i's restored line (None where it keeps the background) → the page on the host, by ONE device→host copy; with ``details`` also per
        restored region a dict with ``plan``, ``out_w`` and the keys of ``extra[i]``"""
        out_ws = [None if p is None else long_lines.plan_out_w(p) for p in plans]
        page = compose(out_ws).cpu().numpy()                                                  # the one device→host copy
        if not details:
            return page
        return page, [None if p is None else dict(plan=p, out_w=w, **e) for p, w, e in zip(plans, out_ws, extra)]

    @torch.no_grad()
    def restore_page(self, image, boxes, texts=None, char_boxes=None, scale=4, feather=8, max_glyphs=16, overlap_glyphs=2, details=False, overlap="refuse",
                     probe_width=384):
        """A page and its text regions → the page enlarged ``scale`` times with every text line restored in place: uint8 RGB [s·H, s·W, 3] on the
        host, the bytes of ``pages.compose_host(image, self.restore_lines(crops, texts, char_boxes), boxes, scale, feather)`` for the crops
        ``image[y1:y2, x1:x2]``.  ``image``: uint8 RGB [H, W, 3]; ``boxes[i]``: region i's text-line box [x1, y1, x2, y2] in page pixels (numbers that
        are not integers are rounded outward and clamped into the page: ``pages.round_box``); ``texts[i]``: its characters; ``char_boxes[i]``: its
        character boxes in PAGE pixels, or evenly spaced ones.  ``scale``: an integer 1..8; ``feather``: 0..1024, the width in output pixels of the
        ramp over which a line is blended into the background at its rectangle's edge (``pages.feather_blend``; 0: none).
        The crops are taken on the host and ALL regions are restored as ONE batch by ``restore_lines``' own machinery (the windows of a region wider
        than 512 px at height 32, ``lq_device.prepare_strips``, one forward, the finiteness check); the joined lines stay on the device.  The page is
        uploaded once, ``mnet_lq_from_u8`` makes the background (``lq_io.resize_cubic(image, s, s)``), ONE ``mnet_paste_u8`` launch pastes every
        region (``pages.compose_page``) and ONE device→host copy brings the page back: nothing per pixel happens on the host.
        A region ``restore_lines`` answers with ``None`` (no character, a character outside the alphabet) keeps the background; with no boxes at all
        the result is the background.  ValueError naming the region, before anything is copied or launched, for a box that is empty or outside the
        page, a rectangle under 8 output rows, and two restored regions that overlap.
        ``overlap="order"`` lifts that last refusal: overlapping regions — stacked lines whose outward-rounded boxes share a row, ascenders and
        descenders of neighbours — are pasted in list order, a later region blended under its own ramp into what the page holds by then (painter's
        order, ``pages``' head), the bytes of ``pages.compose_host(..., overlap="order")``.  The crops are still taken from the original page.  The
        page is then composed by ONE ``mnet_paste_ordered_u8`` launch whose workgroups own page tiles, with or without overlaps.
        ``texts=None``, or ``None`` as one region's text, means "read it", as in ``restore_lines`` (``blind``'s head states the reading): the probe
        windows of every region that is read are views of the uploaded page (``lq_device.prepare_windows``: no crop is cut, no second upload), ONE
        encoder forward reads them all, and the region's text and boxes are then planned as given ones are — so are the planned windows of such
        a page views of it.  A region whose reading is empty keeps the background; it is checked (its rectangle, overlaps) as a restored one.
        ``details=True`` → ``(page, regions)``: per region a dict with ``plan`` (its windows), ``out_w`` (the width of its restored line at height
        128) and ``rect`` (x0, y0, rw, rh in the result), for a region that was read also ``text``, ``boxes`` (its character boxes in PAGE pixels)
        and ``overflow`` (a probe held more than the encoder's 16 characters); None where it kept the background.
        Not covered: a blend of overlapping regions other than painter's order; vertical columns that are rotated or in perspective (upright columns of stacked characters:
        ``restore_page_columns``; rotated, quadrilateral and perspective regions: ``restore_page_quads``; curved text: ``restore_page_curves``; a page
        that mixes these kinds, overlapping or not: ``restore_page_regions``); detection beyond ``restore_page_auto``'s — horizontal lines in columns
        on plain paper, found by ``find_lines``' XY-cut; every other box is the caller's — and the QUALITY of a blind reading
        (the checkpoint's: a text the caller's recogniser supplies is used as given); repairing a probe that overflowed; reading a column
        (``restore_page_columns(blind_columns=True)`` does); several pages in one launch."""
        who = "restore_page"
        image, restored, texts = self._page_front(who, image, len(boxes), texts, [char_boxes], "one text (and one list of character boxes, or None) per box", "boxes")
        return self._restore_page_boxes(who, image, boxes, texts, char_boxes, restored, scale, feather, max_glyphs, overlap_glyphs, details, overlap, probe_width)

    def _restore_page_boxes(self, who, image, boxes, texts, char_boxes, restored, scale, feather, max_glyphs, overlap_glyphs, details, overlap, probe_width,
                            page_d=None):
        """``restore_page`` behind its intake, for ``restore_page_auto`` too: ``page_d``: the page on the device where the caller has uploaded it"""
        H, W = int(image.shape[0]), int(image.shape[1])
        boxes = [pages.round_box(b, H, W) for b in boxes]
        with _named(who):
            rects = pages.region_rects(H, W, boxes, restored, scale, feather, overlap=overlap)

        def paste(out, joined, out_ws, live, plans):
            if pages.check_overlap(overlap):
                return pages.paste_ordered(out, joined, pages.as_cell(pages.build_table(rects, out_ws, feather, int(joined.shape[1]))))
            return pages.paste_rects(out, joined, rects, out_ws, feather)
        return self._restore_page_records(who, image, [dict(kind="line", box=b, rect=r) for b, r in zip(boxes, rects)], texts, char_boxes, scale, max_glyphs,
                                          overlap_glyphs, paste, details, probe_width, page_d)

    @torch.no_grad()
    def restore_page_auto(self, image, scale=4, feather=8, details=False, probe_width=384, max_glyphs=16, overlap_glyphs=2, text_h=None,
                          floor=layout.DEFAULT_FLOOR, pad=None, min_h=None, min_w=None, max_h=None, deskew=False):
        """``restore_page`` for a bare page: nobody supplies the boxes, nobody the texts.  ``find_lines`` finds the page's text lines (``text_h``,
        ``floor``, ``pad``, ``min_h``, ``min_w``, ``max_h`` are its arguments; ``layout``'s head states the rules), and the page — already on
        the device, it is uploaded ONCE for the finding, the reading and the restoration — then goes exactly the way of ``restore_page(image, boxes,
        texts=None, ...)``: a call that finds its lines returns, byte for byte, the call given ``details``' ``boxes``.  A found box whose rectangle
        ``pages.region_rects`` would refuse (``scale`` · h · 16 < 128: under 8 output rows) is dropped and reported in ``skipped``, beside the boxes
        ``find_lines`` skipped.  A page with no line returns the enlarged page.
        ``details=True`` → ``(page, found)``: ``find_lines``' dict — ``boxes`` and ``tight`` without the dropped ones, ``skipped`` with them,
        ``passes`` — plus ``regions`` (``restore_page``'s per-region dicts, None where a line kept the background) and ``text`` (per line what the
        encoder read, None for an empty reading).
        ValueError for ``scale``, ``feather`` and ``layout.line_params``' refusals, and where the networks are on no HIP device (the reading is the
        encoder's), before anything is copied.
        ``deskew=True``: for a page scanned skewed.  The page — still uploaded ONCE, for the estimate, the finding, the reading and the restoration
        — goes through ``estimate_skew`` and ``find_lines_skewed`` (``skew``'s head states the rules), and the found quadrilaterals go exactly the way
        of ``restore_page_quads(image, quads, texts=None, ...)``: the result is, byte for byte, that call given ``details``' ``quads``.  A quadrilateral
        ``quads.check_quads`` would refuse for its size goes to ``skipped``.  ``details`` is then ``find_lines_skewed``'s dict — ``slope``,
        ``frame_boxes``, ``tight``, ``quads``, ``skipped``, ``passes``, ``scores`` — plus ``regions`` (``restore_page_quads``' dicts) and ``text``.
        Not covered: what ``find_lines`` does not cover — vertical columns, rotated or curved text, tables with vertical rules, textured
        backgrounds; without ``deskew`` any skew, with it skew beyond about 5 degrees (the range ``estimate_skew`` searches), 90 / 180 degree
        orientation, perspective and per-block skew (ONE slope is found per page) —, the QUALITY of the finding and of the skew estimate on real
        scans (their defaults are design choices, not measurements) and of the blind reading (the checkpoint's); several pages in one launch."""
        who = "restore_page_auto"
        image = np.asarray(image)
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3 or image.size == 0:
            raise TypeError("%s: uint8 RGB HxWx3 page expected" % who)
        with _named(who):
            pages.check_request(scale, feather, 0, 0, "box", "boxes")
            params = layout.line_params(image.shape[0], text_h, floor, pad, min_h, min_w, max_h)
        if self._device().type != "cuda":
            raise ValueError("%s: the lines it finds are read by the encoder, which needs the networks on a HIP device (they are on %s) — find_lines alone "
                             "runs its host definition there" % (who, self._device()))
        page_d = page_to_device(image, self._device())
        if deskew:
            return self._restore_page_deskewed(who, image, page_d, params, scale, feather, details, probe_width, max_glyphs, overlap_glyphs)
        found = self._find_lines(page_d, params)
        keep = [int(scale) * (b[3] - b[1]) * pages.MIN_RECT_H_DIV >= pages.ROW_H for b in found["boxes"]]
        found["skipped"] = found["skipped"] + [dict(box=b, reason="%d rows high at scale %d: under the %d output rows a line can be reduced to"
                                                    % (b[3] - b[1], int(scale), pages.ROW_H // pages.MIN_RECT_H_DIV)) for b, k in zip(found["boxes"], keep) if not k]
        found["boxes"], found["tight"] = [b for b, k in zip(found["boxes"], keep) if k], [b for b, k in zip(found["tight"], keep) if k]
        n = len(found["boxes"])
        out = self._restore_page_boxes(who, image, found["boxes"], [None] * n, None, [True] * n, scale, feather, max_glyphs, overlap_glyphs, details, "refuse",
                                       probe_width, page_d)
        if not details:
            return out
        return out[0], dict(found, regions=out[1], text=[None if r is None else r["text"] for r in out[1]])

    def _restore_page_deskewed(self, who, image, page_d, params, scale, feather, details, probe_width, max_glyphs, overlap_glyphs):
        """``restore_page_auto(deskew=True)`` behind its intake: ``page_d``: the page on the device, ``params``: ``layout.line_params``' dict"""
        found, s = self._find_lines_skewed(page_d, params, None), int(scale)
        rows = [s * qd.crop_size(q)[1] for q in found["quads"]]
        keep = [h * pages.MIN_RECT_H_DIV >= pages.ROW_H for h in rows]
        found["skipped"] = found["skipped"] + [dict(box=b, reason="%d rows high at scale %d: under the %d output rows a line can be reduced to"
                                                    % (h, s, pages.ROW_H // pages.MIN_RECT_H_DIV)) for b, h, k in zip(found["frame_boxes"], rows, keep) if not k]
        for key in ("frame_boxes", "tight", "quads"):
            found[key] = [v for v, k in zip(found[key], keep) if k]
        n = len(found["quads"])
        with _named(who):
            regions = qd.check_quads(int(image.shape[0]), int(image.shape[1]), found["quads"], [True] * n, scale, feather)
        out = self._restore_page_records(who, image, [dict(r, kind="quad") for r in regions], [None] * n, None, scale, max_glyphs, overlap_glyphs,
                                         lambda out, joined, out_ws, live, plans: qd.paste_quads(out, joined, out_ws, regions, int(feather)), details,
                                         probe_width, page_d)
        if not details:
            return out
        return out[0], dict(found, regions=out[1], text=[None if r is None else r["text"] for r in out[1]])

    @torch.no_grad()
    def restore_page_quads(self, image, quads, texts=None, char_boxes=None, scale=4, feather=8, max_glyphs=16, overlap_glyphs=2, details=False, probe_width=384):
        """``restore_page`` for text regions that are convex quadrilaterals — rotated rectangles and four-point polygons, what a text detector emits
        for a sign photographed at an angle, a slanted scan or a line of rotated characters.  ``quads[i]``: region i's four corners [[x, y]] x 4 in
        page pixels (any numbers), in the text's own reading order: top-left, top-right, bottom-right, bottom-left of the line as it is read (a line
        rotated by 90 degrees is a quadrilateral whose first corner is elsewhere).  ``texts``, ``scale``, ``feather``, ``max_glyphs``,
        ``overlap_glyphs`` as in ``restore_page``; ``char_boxes[i]``: the region's character boxes in PAGE pixels, boxes [x1, y1, x2, y2] or four
        corners each (``quads.char_boxes_in_crop`` takes them into the rectified crop), or evenly spaced ones.
        → uint8 RGB [s·H, s·W, 3] on the host: the bytes of ``quads.compose_quads_host(image, lines, quads, scale, feather)`` for the lines
        ``restore_lines`` gives for the rectified crops ``quads.warp_crop_host(image, quads.quad_map(q, cw, ch), cw, ch)``.  For integer axis-aligned
        boxes given as their corners these are ``restore_page``'s bytes.
        The page is uploaded once and the crops never exist on the host: ``mnet_lq_from_u8`` makes the background, ONE ``mnet_quad_crop_u8`` launch
        rectifies every window of every region into the packed batch ``lq_device.prepare_packed`` turns into the encoder's input, all windows are
        restored as ONE batch and joined on the device as in ``restore_lines``, one ``mnet_paste_u8`` launch brings every line to its upright
        foreground, ONE ``mnet_quad_paste_u8`` launch pastes every region and ONE device→host copy brings the page back.
        A region with no character or a character outside the alphabet keeps the background.  ValueError naming the region, before anything is
        copied or launched: ``quads.check_quads``' refusals.  A quadrilateral partly outside the page is allowed (the crop replicates the page's
        border, the paste is clipped).  ``details=True`` → ``(page, regions)``: per region a dict with ``plan``, ``out_w``, ``quad`` (the corners
        in the result) and ``size`` (rw, rh: the upright foreground's size), None where it kept the background.
        Not covered: overlapping regions, and other kinds of region on the same page (both: ``restore_page_regions``); vertical columns that are
        rotated or in perspective (upright columns: ``restore_page_columns``); curved vertical columns (curved text: ``restore_page_curves``);
        detection; several pages in one launch.
        ``texts=None`` / a region's text ``None``: the region is read as in ``restore_page`` — its probe windows come from one more
        ``mnet_quad_crop_u8`` launch (the probes' first columns and widths) through ``lq_device.prepare_packed`` —; ``details`` then adds ``text``,
        ``boxes`` (in the RECTIFIED CROP's pixels) and ``overflow``.  ``char_boxes[i]`` may be ``{"crop": boxes}``: boxes in the crop already."""
        who = "restore_page_quads"
        image, restored, texts = self._page_front(who, image, len(quads), texts, [char_boxes],
                                                  "one text (and one list of character boxes, or None) per quadrilateral", "quadrilaterals")
        with _named(who):
            regions = qd.check_quads(int(image.shape[0]), int(image.shape[1]), quads, restored, scale, feather)
        return self._restore_page_records(who, image, [dict(r, kind="quad") for r in regions], texts, char_boxes, scale, max_glyphs, overlap_glyphs,
                                          lambda out, joined, out_ws, live, plans: qd.paste_quads(out, joined, out_ws, regions, int(feather)), details, probe_width)

    @torch.no_grad()
    def restore_page_curves(self, image, polygons, texts=None, char_boxes=None, scale=4, feather=8, max_glyphs=16, overlap_glyphs=2, details=False, probe_width=384):
        """``restore_page_quads`` for text regions that are curved strips — seals and round stamps, arched shop signs, logos, text on bottles and
        banners: what a text detector emits as a polygon of 2K points (CTW1500, Total-Text and ArT style).  ``polygons[i]``: region i's 2K points
        [[x, y]] in page pixels (any numbers), 2 <= K <= 33: the K top points left to right in reading order, then the K bottom points right to
        left — clockwise with y down; for K = 2 exactly ``restore_page_quads``' corner order.  ``texts``, ``scale``, ``feather``, ``max_glyphs``,
        ``overlap_glyphs`` as in ``restore_page``; ``char_boxes[i]``: the region's character boxes in PAGE pixels, boxes [x1, y1, x2, y2] or four
        corners each (``curves.char_boxes_in_crop`` takes them into the rectified strip), or evenly spaced ones.
        The region is the chain of the K - 1 quadrilaterals between facing points, each mapped bilinearly (the ruled surface between the two
        polylines: ``curves``' head states the geometry), so the encoder sees a straight line and the restored line is bent back along the curve.
        → uint8 RGB [s·H, s·W, 3] on the host: the bytes of ``curves.compose_curves_host(image, lines, polygons, scale, feather)`` for the lines
        ``restore_lines`` gives for the rectified strips ``curves.warp_crop_host(image, segs, cw, ch)``.  For 4-point polygons that are
        parallelograms, integer axis-aligned boxes included, these are ``restore_page_quads``' bytes.
        The page is uploaded once and the strips never exist on the host: ``mnet_lq_from_u8`` makes the background, ONE ``mnet_curve_crop_u8``
        launch rectifies every window of every region into the packed batch ``lq_device.prepare_packed`` turns into the encoder's input, all
        windows are restored as ONE batch and joined on the device as in ``restore_lines``, one ``mnet_paste_u8`` launch brings every line to its
        upright foreground, ONE ``mnet_curve_paste_u8`` launch pastes every region back along its curve and ONE device→host copy brings the page
        back.  A region with no character or a character outside the alphabet keeps the background.  ValueError naming the region, before
        anything is copied or launched: ``curves.check_curves``' refusals.  A region partly outside the page is allowed (the crop replicates the
        page's border, the paste is clipped).  ``details=True`` → ``(page, regions)``: per region a dict with ``plan``, ``out_w``, ``polygon``
        (the points in the result) and ``size`` (rw, rh: the upright foreground's size), None where it kept the background.
        Not covered: overlapping regions — a seal over the text lines — and other kinds of region on the same page (both:
        ``restore_page_regions``); curved vertical columns (upright ones: ``restore_page_columns``); detection; several pages in one launch.
        ``texts=None`` / a region's text ``None``: the region is read as in ``restore_page_quads``, its probes by one more ``mnet_curve_crop_u8``
        launch; ``details`` then adds ``text``, ``boxes`` (in the rectified strip's pixels) and ``overflow``; ``char_boxes[i]`` may be ``{"crop": boxes}``."""
        who = "restore_page_curves"
        image, restored, texts = self._page_front(who, image, len(polygons), texts, [char_boxes],
                                                  "one text (and one list of character boxes, or None) per polygon", "polygons")
        with _named(who):
            regions = cv.check_curves(int(image.shape[0]), int(image.shape[1]), polygons, restored, scale, feather)
        return self._restore_page_records(who, image, [dict(r, kind="curve") for r in regions], texts, char_boxes, scale, max_glyphs, overlap_glyphs,
                                          lambda out, joined, out_ws, live, plans: cv.paste_curves(out, joined, out_ws, regions, int(feather)), details, probe_width)

    @torch.no_grad()
    def restore_page_columns(self, image, boxes, texts, vertical=None, char_boxes=None, scale=4, feather=8, max_glyphs=16, overlap_glyphs=2, details=False,
                             overlap="refuse", probe_width=384, blind_columns=False):
        """``restore_page`` for pages with vertical text: columns of upright characters stacked top to bottom (shop signs, couplets, book spines,
        traditional typesetting).  ``boxes[i]``: region i's box [x1, y1, x2, y2] in page pixels, rounded outward as in ``restore_page``;
        ``vertical[i]``: region i is a column, read top to bottom (None: every region is); a region with ``vertical[i]`` false is a horizontal line,
        handled exactly as in ``restore_page`` — real pages mix both.  ``texts``, ``scale``, ``feather``, ``max_glyphs``, ``overlap_glyphs`` as there;
        ``char_boxes[i]``: the region's character boxes in PAGE pixels (a column's top to bottom), or evenly spaced ones.
        A column's cells (``columns.cell_cuts``) are each resized on their own to height 32 and laid side by side: the virtual strip
        ``columns.virtual_strip``, an ordinary line from there on, so the networks see upright characters.  → uint8 RGB [s·H, s·W, 3] on the host: the
        bytes of ``columns.compose_columns_host(image, lines, boxes, cuts, scale, feather)`` for the lines ``restore_lines`` gives for the virtual
        strips (with ``columns.virtual_boxes``) and the horizontal crops.  With ``vertical`` all false these are ``restore_page``'s bytes.
        The page is uploaded once and the virtual strips never exist on the host: ``mnet_lq_from_u8`` makes the background, ONE
        ``mnet_column_gather_u8`` launch makes every window of every column (the horizontal crops travel beside them as in ``restore_page``), ALL
        windows of ALL regions are restored as ONE batch and joined on the device, one ``mnet_paste_u8`` launch pastes the horizontal regions, ONE
        ``mnet_column_paste_u8`` launch brings every restored character back to its cell — blended by one ramp along the column's outer edge, none
        between cells — and ONE device→host copy brings the page back.
        A region with no character or a character outside the alphabet keeps the background.  ValueError naming the region (and the character),
        before anything is copied or launched: ``restore_page``'s refusals across both kinds of region, a count of character boxes other than the
        text's length, an empty cell, a cell under 8 output rows, ``plan_windows``' refusals (a cell wider than 512 px at height 32).
        ``details=True`` → ``(page, regions)``: per region ``restore_page``'s dict, for a column with ``cuts`` (page rows) and ``widths`` (its cells'
        widths in the virtual strip) added; None where it kept the background.
        ``overlap="order"`` as in ``restore_page``, across both kinds of region (a sign's column over the line next to it): the bytes of
        ``columns.compose_columns_host(..., overlap="order")``, composed by ONE ``mnet_paste_ordered_u8`` launch over one table that holds the lines'
        regions and the columns' cells together in region order, a column's cells consecutive, in the place of the two paste launches.
        Not covered: a blend of overlapping regions other than painter's order; vertical columns that are rotated or in perspective; right-to-left ordering of columns (the caller's);
        curved vertical columns (curved horizontal text: ``restore_page_curves``); a column on one page with a quadrilateral or a curved region
        (``restore_page_regions``); detection, and the quality of a column's segmentation and reading (``blind_columns``' head: columns whose
        cells are far from square); several pages in one launch.
        A horizontal region whose text is ``None`` is read as in ``restore_page``; a COLUMN whose text is ``None`` is a ValueError that names it
        (its cells are cut from its text, one per character) unless ``blind_columns=True``: such a column is then read first
        (``read_columns``: its cells measured from its ink profile, ``blind_columns``' head) and its reading's text and character boxes stand in
        for given ones — the call returns, byte for byte, the call given ``details``' ``text`` and ``char_boxes`` for that column.  The refusals
        that need no pixel (scale, feather, a box outside the page, ``overlap``) are still raised before anything is copied; the page is
        uploaded once, for the reading and the restoration; the columns' probes go through an encoder forward of their own, beside the one that
        reads the horizontal lines.  A column whose reading is empty keeps the background.  ``details`` adds ``text``, ``char_boxes`` (page
        pixels), ``first_cuts`` and ``overflow`` for a column that was read."""
        who, n = "restore_page_columns", len(boxes)
        image, restored, texts = self._page_front(who, image, n, texts, [char_boxes, vertical],
                                                  "one text (one flag, and one list of character boxes, or None) per box", "boxes")
        H, W = int(image.shape[0]), int(image.shape[1])
        vertical = [True] * n if vertical is None else [bool(v) for v in vertical]
        boxes = [pages.round_box(b, H, W) for b in boxes]
        precheck = lambda: (pages.region_rects(H, W, boxes, restored, scale, feather, overlap=overlap), boxes)[1]     # the refusals that need no pixel
        page_d, texts, char_boxes, restored, read = self._blind_columns_first(who, image, [i for i in range(n) if vertical[i] and texts[i] is None],
                                                                              blind_columns, precheck, texts, char_boxes, restored, scale, probe_width)
        with _named(who):
            ordered = pages.check_overlap(overlap)
            pages.region_rects(H, W, boxes, restored, scale, feather, overlap=overlap)
            cuts = [cl.cell_cuts(boxes[i], len(texts[i]), None if char_boxes is None else char_boxes[i], region=i) if vertical[i] and restored[i] else None
                    for i in range(n)]
            rects = cl.check_columns(H, W, boxes, restored, cuts, scale, feather, overlap=overlap)
        recs = [dict(kind="line", box=b, rect=r) if c is None else dict(kind="column", box=b, rect=r, cuts=c, widths=cl.cell_widths(b, c))
                for b, r, c in zip(boxes, rects, cuts)]

        def paste(out, joined, out_ws, live, plans):
            line_of = {i: l for l, i in enumerate(live)}
            cols, lines_ = [i for i in live if cuts[i] is not None], [i for i in live if cuts[i] is None]
            columns = [(boxes[i], cuts[i], recs[i]["widths"], plans[i]) for i in cols]
            if ordered:                                                                          # one table in region order, one launch by page tile
                col_of = dict(zip(cols, columns))
                return pages.paste_ordered(out, joined, cl.mixed_table(joined, [(line_of[i], rects[i], col_of.get(i, out_ws[i])) for i in live], int(feather)))
            pages.paste_rects(out, joined, rects, [out_ws[i] if i in lines_ else None for i in range(n)], int(feather), [line_of[i] for i in lines_])
            return cl.paste_columns(out, joined, [line_of[i] for i in cols], columns, [rects[i] for i in cols], int(feather))
        return self._restore_page_records(who, image, recs, texts, char_boxes, scale, max_glyphs, overlap_glyphs, paste, details, probe_width, page_d, read)

    @torch.no_grad()
    def restore_page_regions(self, image, regions, texts=None, char_boxes=None, scale=4, feather=8, max_glyphs=16, overlap_glyphs=2, details=False,
                             overlap="refuse", probe_width=384, blind_columns=False):
        """``restore_page`` for a page that MIXES kinds of text region, which may lie over one another: a seal stamped over the text lines, a slanted
        stamp across a table, a sign's column beside a rotated line.  ``regions[i]``: a dict with exactly one of ``"box"`` ([x1, y1, x2, y2], rounded
        outward as in ``restore_page``; with ``"vertical": True`` a column of upright characters as in ``restore_page_columns``), ``"quad"`` (four
        corners as in ``restore_page_quads``) and ``"polygon"`` (2K points as in ``restore_page_curves``) — the JSON ``examples/restore_regions.py``
        reads; other keys are ignored.  ``texts``, ``char_boxes`` (in PAGE pixels), ``scale``, ``feather``, ``max_glyphs``, ``overlap_glyphs`` as in
        those entry points.
        → uint8 RGB [s·H, s·W, 3] on the host: the bytes of ``regions.compose_regions_host(image, lines, regions, texts, char_boxes, scale, feather,
        overlap)`` for the lines ``restore_lines`` gives for each region's crop as its kind defines it.  A page of one kind without overlaps gives
        that kind's entry point's bytes.
        The page is uploaded once.  ALL windows of ALL regions go into ONE packed buffer — the host crops of the horizontal boxes at its head, then
        at most one ``mnet_column_gather_u8``, one ``mnet_quad_crop_u8`` and one ``mnet_curve_crop_u8`` launch, each writing from its own base
        offset — and are restored as ONE batch and joined on the device.  One ``mnet_paste_u8`` launch brings the lines of the quadrilaterals and
        curves to their upright foregrounds in one atlas, ONE ``mnet_paste_mixed_u8`` launch whose workgroups own page tiles pastes every region in
        list order, and ONE device→host copy brings the page back.
        ``overlap="refuse"`` (the default): two restored regions whose interiors intersect, of whatever kinds, are a ValueError that names both
        (``regions``' head states the rule; regions that only touch are not an overlap).  ``overlap="order"``: painter's order, ``pages``' head.
        Both modes compose through the same launch.  Every refusal — each kind's own, naming the region — is raised before anything is copied or
        launched.  ``details=True`` → ``(page, regions)``: per region its kind's existing dict plus ``kind`` ("line", "column", "quad", "curve"),
        None where it kept the background.
        ``texts=None`` / a region's text ``None``: lines, quadrilaterals and curves are read, each as in its own entry point — the lines' probes
        views of the page, at most one crop launch per kind for the other probes, ONE encoder forward for all —; a column whose text is ``None`` is
        a ValueError that names it.  ``details`` then adds ``text``, ``boxes`` (a line's in page pixels, a quadrilateral's and a curve's in their
        crops) and ``overflow``; ``char_boxes[i]`` may be ``{"crop": boxes}`` for boxes that are in the region's crop already.
        ``blind_columns=True``: a column whose text is ``None`` is read first, as in ``restore_page_columns`` (``read_columns``; an encoder
        forward of its own beside the one that reads the other kinds), and its reading's text and character boxes stand in for given ones: the
        call returns, byte for byte, the call given ``details``' ``text`` and ``char_boxes`` for that column.  Every refusal that needs no pixel
        is still raised before anything is copied, and the page is uploaded once.  ``details`` adds ``text``, ``char_boxes``, ``first_cuts`` and
        ``overflow`` for such a column; one whose reading is empty keeps the background.
        Not covered: a blend of overlapping regions other than painter's order; vertical columns that are rotated or curved; detection (the
        caller's; ``find_lines`` finds horizontal lines on plain paper only) and the quality of a blind reading (the checkpoint's) — for a column also that of its segmentation, and columns whose cells are
        far from square (``blind_columns``' head); several pages in one launch."""
        who, n = "restore_page_regions", len(regions)
        image, restored, texts = self._page_front(who, image, n, texts, [char_boxes], "one text (and one list of character boxes, or None) per region", "regions")
        H, W = int(image.shape[0]), int(image.shape[1])
        blind_at = [i for i, r in enumerate(regions) if texts[i] is None and isinstance(r, dict) and "box" in r and r.get("vertical")]
        # called before and after the columns are read: with the texts, character boxes and ``restored`` that hold by then
        normalize = lambda cuts=None: rg.normalize_regions(H, W, regions, restored, texts, [None if char_boxes is None else char_boxes[i] for i in range(n)],
                                                           scale, feather, overlap, cuts=cuts)

        def precheck():                                                 # the refusals that need no pixel: every blind column checked as one cell
            one_cell = [None] * n
            for i in blind_at:
                try:
                    b = pages.round_box(regions[i]["box"], H, W)
                    one_cell[i] = [b[1], b[3]]
                except (TypeError, ValueError):
                    pass                                                # ``normalize_regions`` refuses the box in its own words
            return [r.get("box") for r in normalize(one_cell)]
        page_d, texts, char_boxes, restored, read = self._blind_columns_first(who, image, blind_at, blind_columns, precheck, texts, char_boxes, restored,
                                                                              scale, probe_width)
        with _named(who):
            recs = normalize()
        return self._restore_page_records(who, image, recs, texts, char_boxes, scale, max_glyphs, overlap_glyphs,
                                          lambda out, joined, out_ws, live, plans: rg.paste_regions(out, joined, out_ws, recs, int(feather)), details,
                                          probe_width, page_d, read, with_kind=True)

    def _restore_page_records(self, who, image, recs, texts, char_boxes, scale, max_glyphs, overlap_glyphs, paste, details, probe_width=384, page_d=None,
                              columns_read=None, with_kind=False):
        """the one driver of the five ``restore_page*`` entry points, from their checked regions to the page on the host.  ``recs[i]``: region i's
        record as ``regions.normalize_regions`` gives it — ``kind`` "line" or "column" with ``box`` (a column that is restored: ``cuts``, ``widths``),
        "quad" (``quads.check_quads``' record) or "curve" (``curves.check_curves``') —; ``char_boxes`` in PAGE pixels.  In order: per kind the
        crop's size and the character boxes in the crop (``region_geometry``; a kind's ValueError names ``who`` and the region); where a text is
        None the reading (``_read_regions``) — the page goes to the device then, once, and the probes are windows like any other: a line's views
        of the page, the quadrilaterals' and curves' one crop launch per kind (``page_layout`` with ``lines_as_views``, ``page_windows_lq``); the
        reading's boxes are in crop coordinates, what ``_plan_lines`` plans —; ``_plan_lines``; the packed layout of the planned windows
        (``page_layout``: on a page that was read the lines' windows are views of it, in the place of the host crops and their upload); and in
        ``compose``: the one upload of the page, the background, ``page_windows_lq``, the forward and the join, then ``paste(out, joined, out_ws,
        live, plans)``, the caller's paste, and ``_page_finish`` with ``region_details`` of every region (``with_kind``).
        ``page_d``: the page on the device, where the caller uploaded it already to read its columns (``_blind_columns_first``; it is not copied
        again), and ``columns_read``: those readings, for ``details``."""
        n, W = len(recs), int(image.shape[1])
        with _named(who):
            sizes, local, maps = region_geometry(recs, char_boxes)
        extra = self._column_reading_details([region_details(r, with_kind) for r in recs], columns_read or {})
        need = [i for i in range(n) if texts[i] is None]                # the regions that are read: lines, quadrilaterals, curves (a column is refused)
        read = None
        if need:
            probes = self._region_probes(sizes, need, probe_width, who, "region")
            layout = page_layout(recs, maps, W, True, [(i, k, p[0], p[1]) for i in need for k, p in enumerate(probes[i])])
            page_d = page_to_device(image, self._device()) if page_d is None else page_d
            read = self._read_regions(sizes, need, probes, page_windows_lq(layout, page_d, image), max_glyphs)
        if details and need:
            shift = lambda i: (float(recs[i]["box"][0]), float(recs[i]["box"][1])) if recs[i]["kind"] == "line" else (0.0, 0.0)
            extra = [e if i not in read or read[i] is None else dict(e, **self._reading_details(read[i], *shift(i))) for i, e in enumerate(extra)]
        plans, labels, locs_rows, live = self._plan_lines(sizes, texts, local, max_glyphs, overlap_glyphs, who, "region", read)
        layout = page_layout(recs, maps, W, bool(need), [(i, k, p.c0, p.c1) + ((p.g0, p.g1) if recs[i]["kind"] == "column" else ())
                                                         for i in live for k, p in enumerate(plans[i])])     # its refusals, before anything is copied

        def compose(out_ws):
            page = page_to_device(image, self._device()) if page_d is None else page_d          # the one copy of the page
            out = pages.enlarge(page, int(scale))
            if live:
                paste(out, self._restore_planned(page_windows_lq(layout, page, image), labels, locs_rows, plans, live), out_ws, live, plans)
            return out
        return self._page_finish(plans, compose, details, extra)

    @torch.no_grad()
    def _strips_from_images(self, images, texts, boxes, max_glyphs, preview, host_preview):
        """the per-strip inputs of ``restore_images`` / ``restore_panels``: → (``lq_device.Prepared``, list with one dict per image — lq on the
        device, labels, locs, text, content_w, show_w; ``host_preview``: also ``show``, the preview copied to the host — or None for a strip
        wider than 512 px at height 32)"""
        prep = lq_device.prepare_strips(images, self._device(), preview=preview, skip_too_wide=True)
        strips = [None] * len(images)
        if prep.index:
            if texts is None:
                logits, locs_lr, _ = self.encoder(prep.lq)
                lab_all = clear_labels_batch(logits)
                locs_all = locs_from_left_right(locs_lr).float().cpu()
            show = prep.preview.cpu().numpy() if host_preview else None
            for k, i in enumerate(prep.index):
                h = int(images[i].shape[0])
                if texts is None:
                    labels = lab_all[k][:max_glyphs]
                    n = int(labels.shape[0])
                    locs, text = locs_all[k:k + 1, :2 * n].contiguous(), lq_io.text_from_labels(labels.flatten().tolist())
                else:
                    text = texts[i]
                    n = len(text)
                    bx = boxes[i] if boxes is not None and boxes[i] is not None else lq_io.evenly_spaced_boxes(n, int(images[i].shape[1]), h)
                    labels = lq_io.label_tensor(text)
                    locs = lq_io.locs_from_boxes(bx, h)
                strips[i] = dict(lq=prep.lq[k:k + 1], labels=labels, locs=locs, text=text, content_w=prep.content_w[k], show_w=prep.show_w[k])
                if host_preview:
                    strips[i]["show"] = show[k, :, :prep.show_w[k], :]
        return prep, strips

    @torch.no_grad()
    def forward_blind(self, lq, max_glyphs=16):
        """Self-contained end-to-end pass (SURVEY.md §8f NEXT-2): labels and glyph locations come from the encoder itself
        instead of the YOLO + OCR front-end — labels = ``clear_labels(logits)`` (test_w.py:34-40), locs = the encoder's
        (left, right) pairs converted to (centre, half-width) (Train/tspgan/models/tspgan_model.py:331-336).
        → (SR [B,3,128,2048], labels list, locs [B,32])."""
        logits, locs_lr, _ = self.encoder(lq)
        labels = [l[:max_glyphs] for l in clear_labels_batch(logits)]
        locs = locs_from_left_right(locs_lr)
        return self.forward_batch(lq, [l.to(lq.device) for l in labels], locs), labels, locs
