"""Batched driver for the hot path (SURVEY.md §8f NEXT-1): replaces the reference's batch-1 ``for img_name``
loop (test_sr.py:77-197) by one pass over a whole batch —

    encoder(LQ[B]) → w[B] → TSPGAN over all ΣN glyphs of the batch at once (each glyph uses its image's single
    style vector, test_sr.py:183) → TSPSRNet with the NHWC priors handed over in place

— and shards images data-parallel across the GPUs of a node (one process per GPU, torch.distributed on RCCL)
with one all-gather of the SR outputs.  Images are independent, so there is no other
collective and no weight traffic.
"""
import numpy as np
import torch

from . import ops
from .glyphs import GlyphTables
from .networks import returned_image_precision
from .packing import default_precision, new_tensor, torch_dtype


class MarconetPipeline:
    def __init__(self, encoder, gan, sr, precision=None, glyph_chunk=1024, need_prior_image=True, check_finite=None,
                 prior_image_precision="auto"):
        """``precision``: None → MARCONET_PRECISION or "fp32" (the parity mode, ≤1e-3 vs the CPU reference).  The fp16
        storage modes are opt-in: plain "fp16" stores activations as one half (max 65504, 11 significant bits) and has only
        been validated on O(1)-activation synthetic checkpoints — with trained StyleGAN-type weights a modulated activation
        can overflow.  ``check_finite`` (default: on for every precision but fp32) makes forward_batch verify that the SR
        result is finite (one flag read back per batch) and raise FloatingPointError instead of returning inf/NaN silently."""
        self.encoder, self.gan, self.sr = encoder, gan, sr
        self.glyph_chunk = glyph_chunk
        self.check_finite = check_finite
        precision = default_precision() if precision is None else precision
        # True (default): the generator also produces its 128-px structure image, as test_sr.py:183 does (it is only ever
        # used for the saved visualisation, test_sr.py:203-232).  False is an opt-in for throughput serving.
        self.need_prior_image = need_prior_image
        # precision mode of the generator levels that feed only that image (while forward_batch drops it; ``return_prior=True`` returns it, in the mode's arithmetic): "auto" = plain fp16 in
        # the fp16x2 / fp16x3 modes, the mode's own arithmetic otherwise; None = always the mode's own.  The priors and the SR output
        # do not depend on it (tests/test_modules_gpu.py::test_prior_image_precision_leaves_sr_bits_unchanged)
        self.prior_image_precision = prior_image_precision
        self.set_precision(precision)

    def _image_precision(self):
        if self.prior_image_precision == "auto":
            return "fp16" if self.precision in ("fp16x2", "fp16x3") else None
        return self.prior_image_precision

    def _checks(self):
        return self.check_finite if self.check_finite is not None else self.precision != "fp32"

    def set_precision(self, precision):
        for m in (self.encoder, self.gan, self.sr):
            m.set_precision(precision)
        self.precision = precision
        return self

    @torch.no_grad()
    def forward_batch(self, lq, labels, locs, return_nhwc=False, output="nchw_f32", return_prior=False):
        """lq [B,3,32,512] fp32 (device); labels: list of B int64 [n_b,1] tensors; locs [B, ≥2·max n_b] fp32 — labels and
        locs on the device or (preferably: no synchronisation then) on the host.
        → SR [B,3,128,2048] fp32 NCHW (the reference's return), or NHWC [B,128,2048,8] in the compute dtype if return_nhwc,
        or — output="u8_bgr" — the script's post-processed image [B,128,2048,3] uint8 BGR (test_sr.py:198-200; 4x fewer bytes
        to copy to the host or to all-gather).
        ``return_prior=True`` → ``(that, prior_cha)``: the generator's structure images of all glyphs, fp32 NCHW [ΣN,3,128,128] in
        strip order — what test_sr.py:183 names ``prior_cha`` and :207-212 turn into the panel's last row.  The levels behind the two
        prior levels then run in the MODE's arithmetic (``prior_image_precision="auto"`` demotes them to plain fp16 only while the
        image is dropped) — in the fp16x2 mode in fp16x3 (``networks.returned_image_precision``), while the levels up to the priors
        keep fp16x2: 5.4e-4 on the image, inside the 1e-3 bar but not ``TSPGAN.forward``'s 3.8e-5, which runs the WHOLE generator in
        fp16x3 (see the comment there); the SR output is the same bits either way."""
        dev = lq.device
        counts = [int(l.shape[0]) for l in labels]
        if return_prior:
            self._require_prior_image("return_prior=True")
        with ops.on_device(lq):
            lab, img_of = self._host_prep(labels, counts, dev)
            prior = torch.empty((sum(counts), 128, 128, 4), dtype=torch.float32, device=dev) if return_prior else None
            y, flag = self._core(lq, lab, img_of, counts, locs, None, return_nhwc, output, prior_images=prior)
            self._raise_if_not_finite(flag)
            return (y, ops.nhwc_to_nchw(prior, c=3) if sum(counts) else prior.new_zeros((0, 3, 128, 128))) if return_prior else y

    def _raise_if_not_finite(self, flag):
        """half-range modes (fp16 / fp16x3 / fp16x2 store |activation| < 65504): an overflow turns into NaN on its way through the
        GroupNorm statistics of the following layers (and the last layer writes an infinite pre-activation as NaN instead of
        tanh's +-1), so the SR result carries it; one flag is read back per batch."""
        if flag is not None:                      # None: check off
            raise_if_flagged(flag, self.precision)

    def _require_prior_image(self, what):
        if not self.need_prior_image:
            raise ValueError("%s needs MarconetPipeline(need_prior_image=True): the 128-px level is what produces the structure images" % what)

    def _host_prep(self, labels, counts, dev):
        """labels (host or device) → validated device tensors (labels [ΣN,1], glyph→image index [ΣN])"""
        tg = self.gan.TextGenerator
        if not sum(counts):
            return None, None
        lab = torch.cat([l.reshape(-1, 1) for l in labels if l.shape[0]], dim=0).long()
        # labels / locs held on the HOST (where the OCR / detector front-end leaves them, test_sr.py:121-149) cost no
        # device→host synchronisation: the whole forward is then enqueued without the host ever waiting for the GPU
        if int(lab.min()) < 0 or int(lab.max()) >= tg.class_num:
            raise RuntimeError("label index out of range [0,%d)" % tg.class_num)
        return lab.to(dev).contiguous(), torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts)).to(dev)

    @torch.no_grad()
    def _core(self, lq, lab, img_of, counts, locs, tables, return_nhwc=False, output="nchw_f32", prior_images=None, precision=None, taps=None):
        """the device-side part of forward_batch: nothing here touches host data (it can be captured in a HIP graph).
        ``prior_images`` (fp32 [ΣN,128,128,4] or None): filled with the generator's structure images, chunk by chunk.
        ``precision``: all three nets run THIS call in that mode (None: as configured); no module's state is written, the SR net's per-layer plan
        (``scale_branch_precision``) is off and an image nobody asked for is not computed.  ``taps``: a dict that receives references to ``style_w``,
        the priors as the SR net reads them, its two fused maps and its output (TSPSRNet.forward_packed) — what ``calibrate`` compares.
        → (output, finiteness flag of the SR result: int32 [1] on the device, or None with the check off)"""
        _, _, w = self.encoder(lq, precision=precision)               # test_sr.py:146
        if taps is not None:
            taps["style_w"] = w
        gen_prec = self.precision if precision is None else precision
        need_image = self.need_prior_image if precision is None else prior_images is not None
        tg = self.gan.TextGenerator
        if sum(counts):
            # w0.repeat(n,1) per image (test_sr.py:183): the generator gets the B distinct styles + the glyph→image index
            # the generator runs in chunks of glyphs (bounded working set for huge batches) and writes its two prior levels
            # straight into the all-glyph buffers TSPSRNet reads (no concatenation pass: 34 GB of copies per step at batch 256)
            G, gdt = lab.shape[0], torch_dtype(gen_prec)
            p64 = new_tensor((G, 64, 64, 256), gdt, lq.device)
            p32 = new_tensor((G, 32, 32, 512), gdt, lq.device)
            # a returned image is computed in the mode's arithmetic; a dropped one under ``prior_image_precision`` (see forward_batch)
            # (a RETURNED image in the fp16x2 mode: its image-only level in the three-product arithmetic, networks.returned_image_precision)
            img_prec = self._image_precision() if prior_images is None or self.prior_image_precision != "auto" else returned_image_precision(self.precision)
            if precision is not None:
                img_prec = None                                       # the override's own arithmetic
            for s in range(0, G, self.glyph_chunk):
                e = min(G, s + self.glyph_chunk)
                img = tg.forward_nhwc(w, lab[s:e].contiguous(), need_image=need_image, style_index=img_of[s:e].contiguous(),
                                      p64_out=p64[s:e], p32_out=p32[s:e], image_precision=img_prec, precision=gen_prec)[0]
                if prior_images is not None:
                    prior_images[s:e].copy_(img)
            sr_dtype = torch_dtype(self.sr.precision if precision is None else precision)     # the three nets may run in different precision modes
            p64, p32 = ops.convert(p64, sr_dtype), ops.convert(p32, sr_dtype)
        else:
            p64 = p32 = None
        nchw = output != "u8_bgr" and not return_nhwc
        y = self.sr.forward_packed(lq, p64, p32, counts, counts, locs, nchw_out=nchw, tables=tables, precision=precision, taps=taps)   # test_sr.py:197
        flag = ops.nonfinite_flag(y) if self._checks() else None          # device-side flag (mnet_nonfinite_flag): no synchronisation here
        if output == "u8_bgr":                                           # test_sr.py:198-200 fused: [B,128,2048,3] uint8
            y = ops.sr_postprocess(y, u8=True)
        return y, flag

    @torch.no_grad()
    def calibrate(self, lq, labels, locs, *, reference="fp16x3", tol=5e-4, max_strips=8, apply=False):
        """The precision margin guard — the first thing to run on real checkpoints: is the configured (fast) mode inside the parity bar on THESE
        weights, and if not, where does the deviation enter?  Runs the first ``max_strips`` strips of the batch twice on the device — once exactly
        as ``forward_batch`` would now (the per-module modes, ``scale_branch_precision`` and ``prior_image_precision`` included), once with all
        three nets in ``reference`` ("fp16x3": for the fp16x2 / fp16 modes; "fp32": for any mode) — and compares the two runs stage by stage with
        one ``ops.compare_stats`` launch each: the encoder's style vector, the generator's two priors as the SR net reads them, the SR net's two
        fused feature maps and its output.  No CPU oracle, no host arithmetic on tensors; one device→host copy of the records at the end.
        → ``precision_guard.PrecisionReport``.  ``ok`` means: no non-finite element in any stage and max |SR(mode) − SR(reference)| ≤ ``tol``.

        Why 5e-4: |mode − truth| ≤ |mode − reference| + |reference − truth|.  The parity bar is 1e-3; the most fp16x3 has been seen to deviate from
        the fp32 oracle is 3.2e-4 (measured on an ill-conditioned net with a planted ×1000 GroupNorm gain, 2.7e-4 in the emulation; 2.7e-5 on regular weights), so a passing check keeps
        the mode inside 1e-3 for as long as the reference itself stays within 5e-4 of the truth.  ``reference="fp32"`` removes that assumption at
        several times the cost.  ``first_stage_over`` names the first stage whose deviation relative to max(1, |reference|) exceeds ``tol`` —
        diagnostic only.

        ``apply=True`` and not ok: ``set_precision(reference)``, the SR net's ``scale_branch_precision`` cleared, ``report.applied = True`` — the
        pipeline then computes what one constructed at the reference mode computes.  Otherwise no state of the pipeline or its modules changes.
        Not covered: there is no ``precision="auto"``; ``GraphedForward`` (a captured graph keeps the mode it was captured in — calibrate first),
        ``forward_sharded`` (calibrate on one rank and apply the same mode on all), the generator's returned structure image."""
        from . import _lib, precision_guard as pg
        modes = [self.precision] + [m.precision for m in (self.encoder, self.gan, self.sr)]
        pg.check_reference(modes, reference)
        n = min(int(lq.shape[0]), int(max_strips))
        if n < 1:
            raise ValueError("calibrate: at least one strip is needed")
        labels = list(labels[:n])
        counts = [int(l.shape[0]) for l in labels]
        with ops.on_device(lq):
            lq = lq[:n].contiguous()
            locs = locs[:n]
            lab, img_of = self._host_prep(labels, counts, lq.device)
            runs = []
            for prec in (None, reference):          # each run's buffers other than its taps are gone before the other starts
                taps = {}
                self._core(lq, lab, img_of, counts, locs, None, precision=prec, taps=taps)
                runs.append(taps)
            g2s = pg.glyph_to_strip(counts)
            recs, plan = [], []
            for name in pg.STAGES:
                a, b = runs[0].get(name), runs[1].get(name)
                if a is None or b is None:
                    continue
                groups = int(a.shape[0])
                recs.append(ops.compare_stats(a.contiguous(), b.contiguous(), groups=groups))
                plan.append((name, groups, a.numel() // groups, g2s if name.startswith("prior") else list(range(n))))
            del runs, taps, a, b
            host = torch.cat(recs).cpu().numpy()                      # the one device→host copy
        report = pg.PrecisionReport(mode=self._mode_text(), reference=reference, tol=float(tol), strips=n)
        at = 0
        for name, groups, per, owner in plan:
            setattr(report, name, pg.stage_from_records(name, _lib.cmp_records(host[at:at + groups].tobytes()), owner, n, per))
            at += groups
        if apply and not report.ok:
            self.set_precision(reference)
            self.sr.scale_branch_precision = None
            report.applied = True
        return report

    def _mode_text(self):
        parts = ["%s %s" % (k, m.precision) for k, m in (("encoder", self.encoder), ("gan", self.gan), ("sr", self.sr)) if m.precision != self.precision]
        sb = getattr(self.sr, "scale_branch_precision", None)
        if sb is not None:
            parts.append("sr scale branches %s" % sb)
        return self.precision + (" (%s)" % ", ".join(parts) if parts else "")

    def forward_mixed_widths(self, lq, content_widths, labels, locs, bucket=64):
        with torch.no_grad(), ops.on_device(lq):
            return self._forward_mixed_widths(lq, content_widths, labels, locs, bucket)

    def _forward_mixed_widths(self, lq, content_widths, labels, locs, bucket):
        """BASELINE configs[4]: a batch of strips of different content widths (each zero-padded to 512, i.e. -1 after
        Normalize, test_sr.py:100-115).  The encoder needs the 512-wide strip (its token-axis LayerNorm(64)/Linear(64,.)
        pin 64 tokens, models/textvit_arch.py:59-62,141-144); TSPSRNet is width-agnostic, so images are bucketed by
        ``ceil(w_b / bucket) * bucket`` and each bucket runs the SR net at its own width W'.  Glyph centres are the INTEGER centres of
        the 512-padded run the locs were normalised for — trunc(loc * 512) at the 32-row scale, trunc(loc * 1024) at the 64-row scale
        (models/networks.py:426) — with the windows clipped to W' (2 W'); re-normalising loc to W' in fp32 could move a centre by one
        pixel.  SURVEY.md §8d: the oracle of this mode is the reference TSPSRNet called at the same W' with locs that reproduce those
        centres — it is NOT equal to the 512-padded run (GroupNorm reduces over the whole map; a window that crosses the bucket edge is
        clipped there).
        → list (input order) of SR tensors [3, 128, 4·W'_b] fp32."""
        dev = lq.device
        B = lq.shape[0]
        if lq.shape[-1] != 512 or len(content_widths) != B or len(labels) != B:
            raise ValueError("forward_mixed_widths: lq must be [B,3,32,512] with one content width and one label list per image")
        counts = [int(l.shape[0]) for l in labels]
        widths = []
        for w_ in content_widths:
            w_ = int(w_)
            if w_ <= 0 or w_ > 512:                      # the reference skips wider strips (test_sr.py:108-110)
                raise ValueError("content width %d outside (0, 512]: split the strip into <=512-px segments" % w_)
            widths.append(min(512, (w_ + bucket - 1) // bucket * bucket))
        _, _, w = self.encoder(lq)
        tg = self.gan.TextGenerator
        starts = [0]
        for c in counts:
            starts.append(starts[-1] + c)
        p64 = p32 = None
        if starts[-1]:
            lab, _ = MarconetPipeline._host_prep(self, labels, counts, dev)     # (this method needs only self.gan of a duck-typed self)
            img_of = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(counts, device=dev))
            _, p64, p32 = tg.forward_nhwc(w.index_select(0, img_of).contiguous(), lab, need_image=self.need_prior_image,
                                          image_precision=self._image_precision(), precision=self.precision)
        out = [None] * B
        buckets = sorted(set(widths))
        flags = torch.empty((len(buckets),), dtype=torch.int32, device=dev) if self._checks() else None     # one finiteness flag per bucket
        for kb, wb in enumerate(buckets):
            idx = [b for b in range(B) if widths[b] == wb]
            gsel = [g for b in idx for g in range(starts[b], starts[b + 1])]
            cb = [counts[b] for b in idx]
            it = torch.tensor(idx, device=dev)
            lq_b = lq.index_select(0, it)[:, :, :, :wb].contiguous()
            # glyph centres as in the 512-padded run the locs were normalised for (trunc(loc * 512) / trunc(loc * 1024): integer tables
            # from the ORIGINAL locs — re-normalising to the bucket width in fp32 can move a centre by one pixel), windows clipped to
            # the bucket's width
            lh = locs.detach().float().cpu().numpy()[idx]
            tables = (GlyphTables(lh, cb, wb, 16, dev, centre_w=512), GlyphTables(lh, cb, 2 * wb, 32, dev, centre_w=1024)) if gsel else None
            if gsel:
                gt = torch.tensor(gsel, device=dev)
                a, c = ops.take_rows(p64, gt), ops.take_rows(p32, gt)
            else:
                a = c = None
            y = self.sr.forward_packed(lq_b, a, c, cb, cb, None, nchw_out=True, tables=tables)
            if flags is not None:
                ops.nonfinite_flag(y, out=flags[kb:kb + 1])
            for k, b in enumerate(idx):
                out[b] = y[k]
        self._raise_if_not_finite(flags)
        return out


    @torch.no_grad()
    def forward_sharded(self, lq, labels, locs, output="u8_bgr", group=None, force_collective=False):
        """Data-parallel form of forward_batch: every rank of the process group (one process per GPU; backend
        'nccl' = RCCL over xGMI) is handed the SAME global batch description (lq [B,3,32,512] on the host or on the rank's
        device, labels list, locs [B,2m]), processes its contiguous shard ``shard_range(B, rank, world)`` and all-gathers the
        outputs — the one collective of the path; by default the post-processed uint8 BGR image (0.75 MiB per image instead of
        the 3 MiB fp32 tensor).  → [B,128,2048,3] uint8 (or [B,3,128,2048] fp32 for output="nchw_f32") on every rank, equal
        bit for bit to a single-GPU forward_batch of the whole batch (kernels are batch-invariant).
        ``force_collective``: run the all-gather even in a world of one (an initialised process group is required) — the
        RCCL path exercised on a single-GPU box."""
        import torch.distributed as dist
        world = dist.get_world_size(group) if dist.is_initialized() else 1
        rank = dist.get_rank(group) if dist.is_initialized() else 0
        B = lq.shape[0]
        a, b = shard_range(B, rank, world)
        dev = next(self.sr.parameters()).device
        if b > a:
            y = self.forward_batch(lq[a:b].to(dev), labels[a:b], locs[a:b], output=output)
        else:                         # more ranks than images: an empty shard still takes part in the collective
            shape = (0, 128, 4 * lq.shape[3], 3) if output == "u8_bgr" else (0, 3, 128, 4 * lq.shape[3])
            y = torch.empty(shape, dtype=torch.uint8 if output == "u8_bgr" else torch.float32, device=dev)
        if world == 1 and not force_collective:
            return y
        if not dist.is_initialized():
            raise RuntimeError("forward_sharded(force_collective=True) needs an initialised process group")
        return all_gather_outputs(y, B, group, force=force_collective)

    def _kept(self, strips):
        """positions of the strips the script would restore (a strip that is None was too wide: ``_strips_from_images``)"""
        n_cls = self.gan.TextGenerator.class_num
        return [i for i, s in enumerate(strips) if s is not None and not script_skips(s["labels"], n_cls)]

    @torch.no_grad()
    def _restore_batch(self, lq, labels, locs_rows, with_prior=False):
        """The front end every restore entry point shares.  ``lq`` [n,3,32,512] on the device, the kept strips' label tensors and their
        ``preds_locs`` rows → (the script's post-processed image, uint8 BGR [n,128,2048,3] (test_sr.py:198-200); ``with_prior``: the generator's
        structure images, fp32 NHWC4 [ΣN,128,128,4] in strip order, else None) — both still on the device, the finiteness check done."""
        if with_prior:
            self._require_prior_image("with_prior=True")
        counts = [int(l.shape[0]) for l in labels]
        locs = padded_locs(locs_rows)
        with ops.on_device(lq):
            lab, img_of = self._host_prep(labels, counts, lq.device)
            prior = torch.empty((sum(counts), 128, 128, 4), dtype=torch.float32, device=lq.device) if with_prior else None
            y, flag = self._core(lq, lab, img_of, counts, locs, None, False, "u8_bgr", prior_images=prior)
            self._raise_if_not_finite(flag)
        return y, prior

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
        lq = torch.cat([strips[i]["lq"] for i in keep]).to(next(self.sr.parameters()).device) if keep else None
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
        from . import panel_device
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
            from . import long_lines
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
        from . import blind, lq_device
        sizes = [tuple(int(v) for v in np.shape(img)[:2]) for img in images]
        src, offsets = lq_device.upload_lines(images, next(self.sr.parameters()).device)
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
        from . import blind_columns as bc, pages
        image = pages._page_array(image)
        boxes = bc.check_boxes(image.shape[0], image.shape[1], boxes, scale)
        if not boxes:
            return []
        page_d = torch.from_numpy(np.ascontiguousarray(image)).to(next(self.sr.parameters()).device)      # the one copy of the page
        return self._read_columns(page_d, boxes, scale, probe_width)

    def _read_columns(self, page_d, boxes, scale, probe_width, regions=None):
        """``read_columns`` of a page that is on the device: ``page_d`` uint8 RGB [H, W, 3], ``boxes``: integer boxes inside it; ``regions[k]``: the
        number a refusal gives column k"""
        from . import _lib, blind, blind_columns as bc, columns as cl, lq_device
        W = int(page_d.shape[1])
        tab, starts, total = np.zeros((len(boxes),), dtype=np.dtype(_lib.RowInkBox)), [], 0
        for k, (x1, y1, x2, y2) in enumerate(boxes):                    # the boxes as views of the page, as ``page_view`` has a line's windows
            tab[k] = ((y1 * W + x1) * 3, 3 * W, y2 - y1, x2 - x1, total)
            starts.append(total)
            total += y2 - y1
        ink = torch.empty((total,), dtype=torch.int32, device=page_d.device)
        with ops.on_device(page_d):
            ops.row_ink_u8(page_d.reshape(-1), ops.table_to_device(tab, page_d.device), int(tab["h"].max()), ink)
        ink = ink.cpu().numpy()                                         # the one device→host copy of all profiles
        plans = bc.plan_columns(boxes, [ink[s:s + b[3] - b[1]] for s, b in zip(starts, boxes)], probe_width, regions)
        packed, shapes, offsets = cl.gather_columns(page_d, [(p["box"], p["first_cuts"], p["widths"], bc.probe_windows(p["probes"])) for p in plans])
        rows, locs = blind.encode(self, lq_device.prepare_packed(packed, shapes, offsets).lq)
        return bc.decode(plans, rows, locs, scale)

    def _columns_read_first(self, who, image, blind, boxes, texts, char_boxes, scale, probe_width):
        """``blind_columns=True``: the columns ``blind`` (positions in ``boxes``, integer boxes), whose text is None, are read (``_read_columns``)
        and their readings' text and character boxes stand in for given ones → (the page on the device, to be shared with
        ``_restore_page_records``; texts; char_boxes; {position: reading}).  An empty reading leaves the text "": the column keeps the background."""
        n = len(boxes)
        page_d = torch.from_numpy(np.ascontiguousarray(image)).to(next(self.sr.parameters()).device)      # the one copy of the page
        try:
            readings = self._read_columns(page_d, [boxes[i] for i in blind], scale, probe_width, blind)
        except ValueError as e:
            raise ValueError("%s: %s" % (who, e)) from None
        texts, char_boxes = list(texts), [None] * n if char_boxes is None else list(char_boxes)
        for i, r in zip(blind, readings):
            texts[i], char_boxes[i] = ("", None) if r is None else (r["text"], r["char_boxes"])
        return page_d, texts, char_boxes, dict(zip(blind, readings))

    def _restored_again(self, restored, texts, blind):
        """``_page_front``'s ``restored``, with the columns that were read judged by their reading's text"""
        from . import lq_io
        n_cls = self.gan.TextGenerator.class_num
        return [not script_skips(lq_io.label_tensor(texts[i]), n_cls) if i in blind else r for i, r in enumerate(restored)]

    @staticmethod
    def _column_reading_details(extra, read):
        """what ``details`` adds for a column that was read: ``text``, ``char_boxes`` (page pixels), ``first_cuts`` and ``overflow``"""
        return [e if read.get(i) is None else dict(e, **{k: read[i][k] for k in ("text", "char_boxes", "first_cuts", "overflow")}) for i, e in enumerate(extra)]

    @staticmethod
    def _reading_details(r, dx=0.0, dy=0.0):
        """what ``details`` reports of a reading (None stays None): text, boxes — moved by (dx, dy) — and overflow"""
        return None if r is None else dict(text=r["text"], boxes=[[b[0] + dx, b[1] + dy, b[2] + dx, b[3] + dy] for b in r["boxes"]], overflow=r["overflow"])

    def _read_regions(self, sizes, need, probe_width, max_glyphs, make_lq, who, what):
        """the reading pass of the restore entry points: ``need``: the lines (regions) whose text is None; ``make_lq(probes)`` → the encoder input
        of their probes (``probes[i]``: ``blind.plan_probes`` of line i), fp32 [ΣP,3,32,512] in ``need``'s order → {i: reading}.  A line of
        several probes: ``blind.decode``'s dict, None for an empty reading.  A line of one probe: labels (int64 [n,1], at most ``max_glyphs``) and
        ``locs``, its ``preds_locs`` row, straight from the encoder as ``_strips_from_images(texts=None)`` takes them, beside text, boxes, overflow."""
        from . import blind, lq_io
        probes = {}
        for i in need:
            try:
                probes[i] = blind.plan_probes(sizes[i][0], sizes[i][1], probe_width)
            except ValueError as e:
                raise ValueError("%s: %s %d: %s" % (who, what, i, e)) from None
        rows, locs = blind.encode(self, make_lq(probes))
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
        from . import lq_device
        sizes = [tuple(int(v) for v in np.shape(img)[:2]) for img in images]
        dev = next(self.sr.parameters()).device
        texts = self._texts_or_read(who, texts, len(images))
        need =[i for i, t in enumerate(texts) if t is None] if len(texts) == len(images) else []
        if not need:
            plans, labels, locs_rows, live = self._plan_lines(sizes, texts, boxes, max_glyphs, overlap_glyphs, who, what)
            if not live:
                return None, plans, live, None
            crops = [np.ascontiguousarray(images[i][:, p.c0:p.c1]) for i in live for p in plans[i]]
            prep = lq_device.prepare_strips(crops, dev)
            return self._restore_planned(prep.lq, labels, locs_rows, plans, live), plans, live, None
        src, offsets = lq_device.upload_lines(images, dev)                                        # the one copy of the pixels
        view = lambda i, c0, c1: lq_device.line_window(offsets[i], sizes[i][0], sizes[i][1], c0, c1)
        read = self._read_regions(sizes, need, probe_width, max_glyphs,
                                  lambda probes: lq_device.prepare_windows(src, [view(i, p[0], p[1]) for i in need for p in probes[i]]).lq, who, what)
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
        from . import long_lines, lq_device, lq_io
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
            try:
                plans[i] = long_lines.plan_windows(h, w, bx, max_glyphs, overlap_glyphs)
            except ValueError as e:
                raise ValueError("%s: %s %d: %s" % (who, what, i, e)) from None
            for p in plans[i]:
                labels.append(lab[p.g0:p.g1])
                locs_rows.append(lq_io.locs_from_boxes([[b[0] - p.c0, b[1], b[2] - p.c0, b[3]] for b in bx[p.g0:p.g1]], h))
        return plans, labels, locs_rows, [i for i, p in enumerate(plans) if p is not None]

    def _restore_planned(self, lq, labels, locs_rows, plans, live):
        """the restoring half of ``_joined_lines``: ``lq`` [ΣW,3,32,512] on the device, the encoder input of every window of the lines ``live`` in the
        plans' order → their joined lines, uint8 BGR [L,128,max out_w,3] on the device"""
        from . import long_lines
        y, _ = self._restore_batch(lq, labels, locs_rows)
        return long_lines.compose_lines(y, [plans[i] for i in live])

    def _page_front(self, who, image, n, texts, per_region, expected, units):
        """the intake of the three ``restore_page*`` entry points, ``who``: the ``texts`` refusal, one text — and one entry of every list of
        ``per_region`` that is not None — per region (``n`` of them; the message says ``expected`` of ``units``), a uint8 RGB HxWx3 page (TypeError)
        → (the page as an array, per region whether it is restored: it has a character and none outside the alphabet, the texts as a list).
        ``texts=None`` stands for a None per region; a region whose text is None is read (``_restore_page_records``) and is checked as a restored
        one — whether it has a character is known only once the page is on the device."""
        from . import lq_io
        texts = self._texts_or_read(who, texts, n)
        if len(texts) != n or any(l is not None and len(l) != n for l in per_region):
            raise ValueError("%s: %s expected (%d %s, %d texts)" % (who, expected, n, units, len(texts)))
        image = np.asarray(image)
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3 or image.size == 0:
            raise TypeError("%s: uint8 RGB HxWx3 page expected" % who)
        n_cls = self.gan.TextGenerator.class_num
        return image, [t is None or not script_skips(lq_io.label_tensor(t), n_cls) for t in texts], list(texts)

    def _texts_or_read(self, who, texts, n):
        """``texts`` as a list, ``texts=None`` standing for a None — "read it" — per unit.  Reading is the encoder's work: with the networks on no
        HIP device a text that is None is refused here, before anything is copied, in the words this refusal always had"""
        texts = [None] * n if texts is None else texts
        if any(t is None for t in texts) and next(self.sr.parameters()).device.type != "cuda":
            raise ValueError("%s needs texts: a window is a run of whole characters, and windows cut blind would cut characters in half — a text "
                             "that is None is read by the encoder, which needs the networks on a HIP device (they are on %s)"
                             % (who, next(self.sr.parameters()).device))
        return texts

    @staticmethod
    def _rows_in_order(parts, have, want):
        """``parts``: tensors whose rows, concatenated, are the items ``have`` → the rows of the items ``want`` (the same items in another order)"""
        rows = parts[0] if len(parts) == 1 else torch.cat(parts)
        if have == want:
            return rows
        at = {key: j for j, key in enumerate(have)}
        return rows.index_select(0, torch.tensor([at[key] for key in want], dtype=torch.int64, device=rows.device))

    @staticmethod
    def _columns_need_text(who, columns):
        """``columns``: the columns whose text is None.  A column's cells are cut from its text, one per character, so it cannot be read blind"""
        if columns:
            raise ValueError("%s: region %d: a column needs its text (its cells are cut from it, one per character): only horizontal lines, "
                             "quadrilaterals and curves are read where the text is None" % (who, columns[0]))

    @staticmethod
    def _page_finish(plans, compose, details, extra):
        """the end of the three ``restore_page*`` entry points: ``compose(out_ws)`` → the finished page on the device, ``out_ws[i]`` the width of
        region i's restored line (None where it keeps the background) → the page on the host, by ONE device→host copy; with ``details`` also per
        restored region a dict with ``plan``, ``out_w`` and the keys of ``extra[i]``"""
        from . import long_lines
        out_ws = [None if p is None else long_lines.plan_out_w(p) for p in plans]
        page = compose(out_ws).cpu().numpy()                                                  # the one device→host copy
        if not details:
            return page
        return page, [None if p is None else dict(plan=p, out_w=w, **e) for p, w, e in zip(plans, out_ws, extra)]

    @staticmethod
    def _boxes_in_crop(char_boxes, box):
        """character boxes in page pixels → in the crop of ``box`` (None stays None)"""
        return None if char_boxes is None else [[c[0] - box[0], c[1] - box[1], c[2] - box[0], c[3] - box[1]] for c in char_boxes]

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
        that mixes these kinds, overlapping or not: ``restore_page_regions``); detection (the caller's: the boxes) and the QUALITY of a blind reading
        (the checkpoint's: a text the caller's recogniser supplies is used as given); repairing a probe that overflowed; reading a column
        (``restore_page_columns(blind_columns=True)`` does); several pages in one launch."""
        from . import pages
        who = "restore_page"
        image, restored, texts = self._page_front(who, image, len(boxes), texts, [char_boxes], "one text (and one list of character boxes, or None) per box", "boxes")
        H, W = int(image.shape[0]), int(image.shape[1])
        boxes = [pages.round_box(b, H, W) for b in boxes]
        try:
            rects = pages.region_rects(H, W, boxes, restored, scale, feather, overlap=overlap)
        except ValueError as e:
            raise ValueError("%s: %s" % (who, e)) from None

        def paste(out, joined, out_ws, live, plans):
            if pages.check_overlap(overlap):
                return pages.paste_ordered(out, joined, pages.as_cell(pages.build_table(rects, out_ws, feather, int(joined.shape[1]))))
            return pages.paste_rects(out, joined, rects, out_ws, feather)
        return self._restore_page_records(who, image, [dict(kind="line", box=b, rect=r) for b, r in zip(boxes, rects)], texts, char_boxes, scale, max_glyphs,
                                          overlap_glyphs, paste, details, [dict(rect=r) for r in rects], probe_width)

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
        from . import quads as qd
        who = "restore_page_quads"
        image, restored, texts = self._page_front(who, image, len(quads), texts, [char_boxes],
                                           "one text (and one list of character boxes, or None) per quadrilateral", "quadrilaterals")
        try:
            regions = qd.check_quads(int(image.shape[0]), int(image.shape[1]), quads, restored, scale, feather)
        except ValueError as e:
            raise ValueError("%s: %s" % (who, e)) from None
        return self._restore_page_records(who, image, [dict(r, kind="quad") for r in regions], texts, char_boxes, scale, max_glyphs, overlap_glyphs,
                                          lambda out, joined, out_ws, live, plans: qd.paste_quads(out, joined, out_ws, regions, int(feather)), details,
                                          [dict(quad=r["out_quad"], size=(r["rw"], r["rh"])) for r in regions], probe_width)

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
        from . import curves as cv
        who = "restore_page_curves"
        image, restored, texts = self._page_front(who, image, len(polygons), texts, [char_boxes],
                                           "one text (and one list of character boxes, or None) per polygon", "polygons")
        try:
            regions = cv.check_curves(int(image.shape[0]), int(image.shape[1]), polygons, restored, scale, feather)
        except ValueError as e:
            raise ValueError("%s: %s" % (who, e)) from None
        return self._restore_page_records(who, image, [dict(r, kind="curve") for r in regions], texts, char_boxes, scale, max_glyphs, overlap_glyphs,
                                          lambda out, joined, out_ws, live, plans: cv.paste_curves(out, joined, out_ws, regions, int(feather)), details,
                                          [dict(polygon=r["out_polygon"], size=(r["rw"], r["rh"])) for r in regions], probe_width)

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
        from . import columns as cl, pages
        who, n = "restore_page_columns", len(boxes)
        image, restored, texts = self._page_front(who, image, n, texts, [char_boxes, vertical],
                                           "one text (one flag, and one list of character boxes, or None) per box", "boxes")
        H, W = int(image.shape[0]), int(image.shape[1])
        vertical = [True] * n if vertical is None else [bool(v) for v in vertical]
        boxes = [pages.round_box(b, H, W) for b in boxes]
        blind, page_d, read = [i for i in range(n) if vertical[i] and texts[i] is None], None, {}
        if not blind_columns:
            self._columns_need_text(who, blind)
        elif blind:
            try:
                pages.region_rects(H, W, boxes, restored, scale, feather, overlap=overlap)          # the refusals that need no pixel
            except ValueError as e:
                raise ValueError("%s: %s" % (who, e)) from None
            page_d, texts, char_boxes, read = self._columns_read_first(who, image, blind, boxes, texts, char_boxes, scale, probe_width)
            restored = self._restored_again(restored, texts, blind)
        try:
            ordered = pages.check_overlap(overlap)
            pages.region_rects(H, W, boxes, restored, scale, feather, overlap=overlap)
            cuts = [cl.cell_cuts(boxes[i], len(texts[i]), None if char_boxes is None else char_boxes[i], region=i) if vertical[i] and restored[i] else None
                    for i in range(n)]
            rects = cl.check_columns(H, W, boxes, restored, cuts, scale, feather, overlap=overlap)
        except ValueError as e:
            raise ValueError("%s: %s" % (who, e)) from None
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
        extra = [dict(rect=r["rect"]) if "cuts" not in r else dict(rect=r["rect"], cuts=r["cuts"], widths=r["widths"]) for r in recs]
        return self._restore_page_records(who, image, recs, texts, char_boxes, scale, max_glyphs, overlap_glyphs, paste, details,
                                          self._column_reading_details(extra, read), probe_width, page_d)

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
        caller's) and the quality of a blind reading (the checkpoint's) — for a column also that of its segmentation, and columns whose cells are
        far from square (``blind_columns``' head); several pages in one launch."""
        from . import pages, regions as rg
        who, n = "restore_page_regions", len(regions)
        image, restored, texts = self._page_front(who, image, n, texts, [char_boxes], "one text (and one list of character boxes, or None) per region", "regions")
        blind, page_d, read = [i for i, r in enumerate(regions) if texts[i] is None and isinstance(r, dict) and "box" in r and r.get("vertical")], None, {}
        if not blind_columns:
            self._columns_need_text(who, blind)
        elif blind:
            H, W = int(image.shape[0]), int(image.shape[1])
            one_cell = [None] * n                                       # the refusals that need no pixel: every blind column checked as one cell
            for i in blind:
                try:
                    b = pages.round_box(regions[i]["box"], H, W)
                    one_cell[i] = [b[1], b[3]]
                except (TypeError, ValueError):
                    pass                                                # ``normalize_regions`` refuses the box in its own words
            try:
                pre = rg.normalize_regions(H, W, regions, restored, texts, [None if char_boxes is None else char_boxes[i] for i in range(n)], scale,
                                           feather, overlap, cuts=one_cell)
            except ValueError as e:
                raise ValueError("%s: %s" % (who, e)) from None
            page_d, texts, char_boxes, read = self._columns_read_first(who, image, blind, [r.get("box") for r in pre], texts, char_boxes, scale, probe_width)
            restored = self._restored_again(restored, texts, blind)
        try:
            recs = rg.normalize_regions(int(image.shape[0]), int(image.shape[1]), regions, restored, texts,
                                        [None if char_boxes is None else char_boxes[i] for i in range(n)], scale, feather, overlap)
        except ValueError as e:
            raise ValueError("%s: %s" % (who, e)) from None
        extra = []
        for r in recs:
            if r["kind"] in ("line", "column"):
                extra.append(dict(kind=r["kind"], rect=r["rect"], **({"cuts": r["cuts"], "widths": r["widths"]} if "widths" in r else {})))
            elif r["kind"] == "quad":
                extra.append(dict(kind="quad", quad=r["out_quad"], size=(r["rw"], r["rh"])))
            else:
                extra.append(dict(kind="curve", polygon=r["out_polygon"], size=(r["rw"], r["rh"])))
        return self._restore_page_records(who, image, recs, texts, char_boxes, scale, max_glyphs, overlap_glyphs,
                                          lambda out, joined, out_ws, live, plans: rg.paste_regions(out, joined, out_ws, recs, int(feather)), details,
                                          self._column_reading_details(extra, read), probe_width, page_d)

    def _restore_page_records(self, who, image, recs, texts, char_boxes, scale, max_glyphs, overlap_glyphs, paste, details, extra, probe_width=384,
                              page_d=None):
        """the one driver of the five ``restore_page*`` entry points, from their checked regions to the page on the host.  ``recs[i]``: region i's
        record as ``regions.normalize_regions`` gives it — ``kind`` "line" or "column" with ``box`` (a column that is restored: ``cuts``, ``widths``),
        "quad" (``quads.check_quads``' record) or "curve" (``curves.check_curves``') —; ``char_boxes`` in PAGE pixels.  Per kind the crop's size and
        the character boxes in the crop (a kind's ValueError names ``who`` and the region), ``_plan_lines``, the packed layout — the host crops of
        the lines at the head, then the columns', the quadrilaterals' and the curves' windows, each kind from its own base —, and in ``compose``:
        one upload of the page, the background, at most one gather / crop launch per kind present, ``lq_device.prepare_packed``, the forward and
        the join, then ``paste(out, joined, out_ws, live, plans)``, the caller's paste, and ``_page_finish`` with the caller's ``extra``.
        A region whose text is None is read first (``_read_regions``): the page goes to the device then, once; a line's probes are views of it, the
        quadrilaterals' and curves' probes one crop launch per kind into a buffer of their own; the reading's boxes are in crop coordinates, what
        ``_plan_lines`` plans.  On such a page the lines' planned windows are views of the page too, in the place of the host crops and their upload.
        ``page_d``: the page on the device, where the caller uploaded it already (to read its columns: ``_columns_read_first``); it is not copied again."""
        from . import columns as cl, curves as cv, lq_device, pages, quads as qd
        n = len(recs)
        cb = [None if char_boxes is None else char_boxes[i] for i in range(n)]
        sizes, local, maps = [], [None] * n, [None] * n
        for i, r in enumerate(recs):
            try:
                if r["kind"] == "column" and "widths" in r:
                    sizes.append((cl.LQ_H, sum(r["widths"])))
                    local[i] = cl.virtual_boxes(r["widths"])
                elif r["kind"] in ("line", "column"):
                    sizes.append((r["box"][3] - r["box"][1], r["box"][2] - r["box"][0]))
                    local[i] = cb[i]["crop"] if isinstance(cb[i], dict) else self._boxes_in_crop(cb[i], r["box"])
                else:
                    sizes.append((r["ch"], r["cw"]))
                    if r["kind"] == "quad":
                        maps[i] = qd.quad_map(r["quad"], r["cw"], r["ch"])
                    if isinstance(cb[i], dict):                 # boxes in the rectified crop already: what ``details`` reports of a region that was read
                        local[i] = cb[i]["crop"]
                    elif cb[i] is not None:
                        local[i] = qd.char_boxes_in_crop(cb[i], maps[i], r["cw"], r["ch"]) if r["kind"] == "quad" else \
                            cv.char_boxes_in_crop(cb[i], r["segs"], r["cw"], r["ch"])
            except ValueError as e:
                raise ValueError("%s: region %d: %s" % (who, i, e)) from None
        page_dev, W = [] if page_d is None else [page_d], int(image.shape[1])     # ``page_d``: the page, where the caller has uploaded it already

        def page_on_device():                                           # the one copy of the page, made when it is first needed
            if not page_dev:
                page_dev.append(torch.from_numpy(np.ascontiguousarray(image)).to(next(self.sr.parameters()).device))
            return page_dev[0]

        def page_view(i, c0, c1):                                       # the columns [c0, c1) of line i's box as a window of the page
            x1, y1, _, y2 = recs[i]["box"]
            return ((y1 * W + x1 + int(c0)) * 3, 3 * W, y2 - y1, int(c1) - int(c0))

        def read_lq(probes):                                            # the encoder input of every probe, in ``need``'s order
            page_d = page_on_device()
            keys = [[(i, k) for i in need if recs[i]["kind"] == kind for k in range(len(probes[i]))] for kind in ("line", "quad", "curve")]
            parts = []
            if keys[0]:
                parts.append(lq_device.prepare_windows(page_d.reshape(-1), [page_view(i, *probes[i][k][:2]) for i, k in keys[0]]).lq)
            if keys[1] or keys[2]:
                size = lambda i, k: (probes[i][k][1] - probes[i][k][0], recs[i]["ch"])
                q_sz, c_sz = [size(i, k) for i, k in keys[1]], [size(i, k) for i, k in keys[2]]
                q_c0, c_c0 = [probes[i][k][0] for i, k in keys[1]], [probes[i][k][0] for i, k in keys[2]]
                q_t, base = qd.crop_table([maps[i] for i, _ in keys[1]], q_sz, q_c0, 0)
                c_t, _, total = cv.crop_table([recs[i]["segs"] for i, _ in keys[2]], c_sz, c_c0, base)
                buf = torch.empty((total,), dtype=torch.uint8, device=page_d.device)
                if keys[1]:
                    qd.crop_quads(page_d, [maps[i] for i, _ in keys[1]], q_sz, q_c0, 0, buf)
                if keys[2]:
                    cv.crop_curves(page_d, [recs[i]["segs"] for i, _ in keys[2]], c_sz, c_c0, base, buf)
                parts.append(lq_device.prepare_packed(buf, [(h, w) for w, h in q_sz + c_sz], [int(o) for o in q_t["offset"]] + [int(o) for o in c_t["offset"]]).lq)
            return self._rows_in_order(parts, keys[0] + keys[1] + keys[2], [(i, k) for i in need for k in range(len(probes[i]))])

        need = [i for i in range(n) if texts[i] is None]                # the regions that are read: lines, quadrilaterals, curves (a column is refused)
        read = self._read_regions(sizes, need, probe_width, max_glyphs, read_lq, who, "region") if need else None
        if details and need:
            shift = lambda i: (float(recs[i]["box"][0]), float(recs[i]["box"][1])) if recs[i]["kind"] == "line" else (0.0, 0.0)
            extra = [e if i not in read or read[i] is None else dict(e, **self._reading_details(read[i], *shift(i))) for i, e in enumerate(extra)]
        plans, labels, locs_rows, live = self._plan_lines(sizes, texts, local, max_glyphs, overlap_glyphs, who, "region", read)
        of_kind = lambda kind: [i for i in live if recs[i]["kind"] == kind]
        cols = of_kind("column")
        q_wins, c_wins = [[(i, k, p) for i in of_kind(kind) for k, p in enumerate(plans[i])] for kind in ("quad", "curve")]
        flat, where, head, views = [], {}, 0, {}                        # the horizontal windows' crops, at the head of the packed batch
        for i in of_kind("line"):
            x1, y1, x2, y2 = recs[i]["box"]
            for k, p in enumerate(plans[i]):
                if need:                                                # a page that is read is on the device already: its lines' windows are views of it
                    views[(i, k)] = page_view(i, p.c0, p.c1)
                    continue
                where[(i, k)] = ((y2 - y1, p.c1 - p.c0), head)
                flat.append(np.ascontiguousarray(image[y1:y2, x1 + p.c0:x1 + p.c1]).reshape(-1))
                head += flat[-1].size
        columns = [(recs[i]["box"], recs[i]["cuts"], recs[i]["widths"], plans[i]) for i in cols]
        cell_tab, shapes, offsets, q_base = cl.gather_table(columns, head)                          # its refusals, before anything is copied
        for key, h_w, off in zip([(i, k) for i in cols for k in range(len(plans[i]))], shapes, offsets):
            where[key] = (h_w, off)
        q_sizes, c_sizes = [(p.c1 - p.c0, recs[i]["ch"]) for i, _, p in q_wins], [(p.c1 - p.c0, recs[i]["ch"]) for i, _, p in c_wins]
        q_tab, c_base = qd.crop_table([maps[i] for i, _, _ in q_wins], q_sizes, [p.c0 for _, _, p in q_wins], q_base)
        c_tab, _, nbytes = cv.crop_table([recs[i]["segs"] for i, _, _ in c_wins], c_sizes, [p.c0 for _, _, p in c_wins], c_base)
        for wins, wh, tab in ((q_wins, q_sizes, q_tab), (c_wins, c_sizes, c_tab)):
            for (i, k, _), (w, h), off in zip(wins, wh, tab["offset"]):
                where[(i, k)] = ((h, w), int(off))

        def compose(out_ws):
            page_d = page_on_device()                                                            # the one copy of the page
            out = pages.enlarge(page_d, int(scale))
            if live:
                packed = torch.empty((nbytes,), dtype=torch.uint8, device=page_d.device)         # the ragged batch of every kind's windows
                if cols:
                    with ops.on_device(page_d):
                        ops.column_gather_u8(page_d, ops.table_to_device(cell_tab, page_d.device), int(cell_tab["dw"].max()), cl.LQ_H, packed)
                if q_wins:
                    qd.crop_quads(page_d, [maps[i] for i, _, _ in q_wins], q_sizes, [p.c0 for _, _, p in q_wins], q_base, packed)
                if c_wins:
                    cv.crop_curves(page_d, [recs[i]["segs"] for i, _, _ in c_wins], c_sizes, [p.c0 for _, _, p in c_wins], c_base, packed)
                if head:
                    packed[:head].copy_(torch.from_numpy(np.concatenate(flat)))               # the lines' crops: the one upload beside the page's
                keys = [(i, k) for i in live for k in range(len(plans[i]))]
                packed_keys, parts = [key for key in keys if key in where], []
                if views:
                    parts.append(lq_device.prepare_windows(page_d.reshape(-1), [views[key] for key in keys if key in views]).lq)
                if packed_keys:
                    parts.append(lq_device.prepare_packed(packed, [where[key][0] for key in packed_keys], [where[key][1] for key in packed_keys]).lq)
                lq = self._rows_in_order(parts, [key for key in keys if key in views] + packed_keys, keys)
                paste(out, self._restore_planned(lq, labels, locs_rows, plans, live), out_ws, live, plans)
            return out
        return self._page_finish(plans, compose, details, extra)

    @torch.no_grad()
    def _strips_from_images(self, images, texts, boxes, max_glyphs, preview, host_preview):
        """the per-strip inputs of ``restore_images`` / ``restore_panels``: → (``lq_device.Prepared``, list with one dict per image — lq on the
        device, labels, locs, text, content_w, show_w; ``host_preview``: also ``show``, the preview copied to the host — or None for a strip
        wider than 512 px at height 32)"""
        from . import lq_device, lq_io
        dev = next(self.sr.parameters()).device
        prep = lq_device.prepare_strips(images, dev, preview=preview, skip_too_wide=True)
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
        labels = clear_labels_batch(logits)
        labels = [l[:max_glyphs] for l in labels]
        locs = locs_from_left_right(locs_lr)
        return self.forward_batch(lq, [l.to(lq.device) for l in labels], locs), labels, locs


def script_skips(labels, class_num):
    """True for a strip the script would skip: no character (test_sr.py:168-170), or a label the generator raises on — −1 for a character
    outside the alphabet, or one at or beyond ``class_num`` (:181-190).  ``labels``: the strip's int64 label tensor"""
    return labels.numel() == 0 or int(labels.min()) < 0 or int(labels.max()) >= class_num


def padded_locs(rows):
    """the strips' ``preds_locs`` rows (each [1, 2·n_k]) → one fp32 [n, max 2·n_k] host tensor, zeros behind each row's end"""
    locs = torch.zeros((len(rows), max(int(r.shape[1]) for r in rows)), dtype=torch.float32)
    for k, r in enumerate(rows):
        locs[k, :r.shape[1]] = r[0]
    return locs


def prepared_rows(prep, keep):
    """the images ``keep`` (positions in the caller's list) in a ``lq_device.Prepared`` batch → (their rows in it, those rows of ``prep.lq``)"""
    rows = [prep.index.index(i) for i in keep]
    return rows, prep.lq.index_select(0, torch.tensor(rows, dtype=torch.int64, device=prep.lq.device))


def raise_if_flagged(flag, precision):
    """flag: int32 flags of ``ops.nonfinite_flag`` on the device (1 = inf / NaN found) — ONE device→host copy, tested on the host"""
    if any(flag.cpu().tolist()):
        raise FloatingPointError("marconet_amd: non-finite SR output in %s mode (activations beyond the fp16 range 65504?) — use "
                                 "precision='fp32' for these weights" % precision)


ALPHABET_SIZE = 6735          # utils/alphabets.py: 6735 characters; class 6735 = blank / padding


def clear_labels_batch(logits):
    """test_w.py:34-40 for a whole batch: argmax over the 6736 classes (HIP kernel, first maximal index like torch.max, a NaN
    counting as the maximum as it does there),
    ONE device→host copy of the [B,64] indices, then the CTC-style collapse on the host (drop repeats, drop blanks).
    → list of B int64 tensors [n_b, 1] (CPU)."""
    B, T, C = logits.shape
    with ops.on_device(logits):
        idx = ops.argmax_rows(logits.reshape(B * T, C).contiguous().float()).reshape(B, T).cpu().tolist()
    return [torch.tensor(collapse_indices(row), dtype=torch.int64).reshape(-1, 1) for row in idx]


def collapse_indices(row, alphabet_size=ALPHABET_SIZE):
    """the CTC-style collapse of test_w.py:37-39 on one row of argmax indices: drop repeats, drop blanks (>= alphabet size)"""
    return [v for i, v in enumerate(row) if not (i > 0 and row[i - 1] == v) and v < alphabet_size]


def locs_from_left_right(locs_lr):
    """(left, right) pairs → (centre, half-width) pairs, Train/tspgan/models/tspgan_model.py:331-336 (elementwise; tiny)."""
    l, r = locs_lr[:, 0::2], locs_lr[:, 1::2]
    out = torch.empty_like(locs_lr)
    out[:, 0::2] = (r + l) / 2.0
    out[:, 1::2] = (r - l) / 2.0
    return out


@torch.no_grad()
def w_interpolation(gan, w1, w2, labels, steps=11):
    """test_w.py:104-108: structure images for styles s·w1 + (1-s)·w2, s = i/(steps-1) — all interpolation steps in ONE
    generator call (each glyph is independent).  w1, w2 [1,512]; labels int64 [n,1] → images [steps, n, 3, 128, 128]."""
    n = labels.shape[0]
    ws = torch.cat([(w1 * (i / (steps - 1)) + w2 * (1 - i / (steps - 1))).repeat(n, 1) for i in range(steps)], dim=0)
    img, _, _ = gan(styles=ws.contiguous(), labels=labels.to(w1.device).repeat(steps, 1), noise=None)
    return img.reshape(steps, n, *img.shape[1:])


class GraphedForward:
    """The whole forward for one (batch size, glyphs per image) signature captured in a HIP graph: the script's batch-1 loop
    (test_sr.py:77) is launch-bound on the host (≈400 kernel launches, 9.5 ms per image against ≈6 ms of GPU work), a graph
    replay is one submission.  Inputs live in static device buffers refreshed before each replay (LQ, labels, glyph→image
    index, the glyph window tables); the output is a static buffer too — consume or clone it before the next call."""

    def __init__(self, pipe, batch, counts, output="nchw_f32", device="cuda"):
        from .glyphs import GlyphTables
        import numpy as np
        self.pipe, self.counts, self.output = pipe, [int(c) for c in counts], output
        if len(self.counts) != batch:
            raise ValueError("one glyph count per image")
        dev = torch.device(device)
        G = sum(self.counts)
        self.lq = torch.zeros((batch, 3, 32, 512), dtype=torch.float32, device=dev)
        self.lab = torch.zeros((G, 1), dtype=torch.int64, device=dev) if G else None
        self.img_of = torch.repeat_interleave(torch.arange(batch), torch.tensor(self.counts)).to(dev) if G else None
        dummy = np.full((batch, 2 * max(self.counts + [1])), 0.5, dtype=np.float32)
        self.widths = (self.lq.shape[3], 2 * self.lq.shape[3])           # feature widths at the 32- and 64-row scales
        self.tables = (GlyphTables(dummy, self.counts, self.widths[0], 16, dev),
                       GlyphTables(dummy, self.counts, self.widths[1], 32, dev)) if G else None
        with ops.on_device(self.lq):
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):                              # warm-up: packs weights, raises kernel attributes
                for _ in range(2):
                    pipe._core(self.lq, self.lab, self.img_of, self.counts, None, self.tables, output=output)
            torch.cuda.current_stream(dev).wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                # _flag: the finiteness flag this graph refreshes on every replay (None: captured with the check off)
                self.out, self._flag = pipe._core(self.lq, self.lab, self.img_of, self.counts, None, self.tables, output=output)
            self._checks = pipe._checks()
            self._quiet_without_flag = pipe.precision == "fp32" and pipe.check_finite is None     # as captured

    @property
    def has_flag(self):
        """True when this graph refreshes a finiteness flag on every replay (captured with the check on)"""
        return self._flag is not None

    def raise_if_not_finite(self):
        """reads this graph's own flag (one device→host synchronisation) — for callers that replay with check=False and test later"""
        if self._flag is None:
            if self._quiet_without_flag:
                return       # fp32 has no half-range overflow to report: code shared with the half-range modes may call this unconditionally
            raise RuntimeError("GraphedForward: this graph was captured with the finiteness check off (check_finite=False): "
                               "there is no flag to read — capture with MarconetPipeline(check_finite=True); `has_flag` tells")
        raise_if_flagged(self._flag, self.pipe.precision)

    @torch.no_grad()
    def __call__(self, lq, labels, locs, check=None):
        """``check``: None = as the pipe was configured at capture (on for the half-range modes: one flag read back, i.e. one
        synchronisation per replay); False = no read-back on the latency path — call raise_if_not_finite() when the output is consumed;
        True on a graph captured WITHOUT the flag raises RuntimeError (a check that cannot happen must not pass silently)"""
        from .glyphs import GlyphTables
        counts = [int(l.shape[0]) for l in labels]
        if counts != self.counts or tuple(lq.shape) != tuple(self.lq.shape):
            raise ValueError("this graph was captured for batch %d with glyph counts %s" % (self.lq.shape[0], self.counts))
        self.lq.copy_(lq, non_blocking=True)
        if self.lab is not None:
            lab, _ = self.pipe._host_prep(labels, counts, self.lq.device)
            self.lab.copy_(lab, non_blocking=True)
            lh = locs.detach().float().cpu().numpy()
            GlyphTables(lh, counts, self.widths[0], 16, "cpu").copy_into(self.tables[0])
            GlyphTables(lh, counts, self.widths[1], 32, "cpu").copy_into(self.tables[1])
        self.graph.replay()
        if self._checks if check is None else check:
            self.raise_if_not_finite()
        return self.out


def balance_shards(content_widths, glyph_counts, world, bucket=64):
    """configs[4] on N GPUs: assign images to ranks so that the algorithmic work per rank is balanced
    (longest-processing-time greedy on F_b = 108.0 + 3.69 + 484.1·W'_b/512 + 89.03·n_b GFLOP).
    → list of ``world`` index lists (each sorted by bucket width so a rank runs few distinct widths)."""
    cost = []
    for b, (w_, n) in enumerate(zip(content_widths, glyph_counts)):
        wb = min(512, (int(w_) + bucket - 1) // bucket * bucket)
        cost.append((108.0 + 3.69 + 484.1 * wb / 512.0 + 89.03 * int(n), wb, b))
    load = [0.0] * world
    parts = [[] for _ in range(world)]
    for c, wb, b in sorted(cost, reverse=True):
        r = min(range(world), key=lambda k: (load[k], k))
        load[r] += c
        parts[r].append((wb, b))
    return [[b for _, b in sorted(p_)] for p_ in parts]


def shard_range(total, rank, world):
    """contiguous, balanced split of ``total`` images over ``world`` ranks → (start, stop) of ``rank``"""
    base, rem = divmod(total, world)
    start = rank * base + min(rank, rem)
    return start, start + base + (1 if rank < rem else 0)


def all_gather_outputs(local, total, group=None, force=False):
    """all-gather of per-rank SR outputs [b_r,...] → [total,...] on every rank (RCCL over xGMI when the
    backend is 'nccl'; gloo in the CPU tests).  Uneven shards are padded to the largest shard.  A world of one returns
    ``local`` without a collective unless ``force`` (the collective then really runs: one rank gathering from itself)."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    if world == 1 and not force:
        return local
    sizes = [shard_range(total, r, world) for r in range(world)]
    mx = max(b - a for a, b in sizes)
    if local.shape[0] < mx:
        pad = torch.zeros((mx - local.shape[0],) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
        local = torch.cat([local, pad])
    out = torch.empty((world * mx,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(out, local.contiguous(), group=group)
    if all(b - a == mx for a, b in sizes):
        return out
    return torch.cat([out[r * mx: r * mx + (b - a)] for r, (a, b) in enumerate(sizes)])


class OverlappedGather:
    """The all-gather of step i runs (on the collective backend's own stream) while step i+1 computes: ``submit`` enqueues
    it asynchronously into one of two rotating output buffers and returns the gathered result of the PREVIOUS submit
    (None the first time); ``flush`` waits for the last one.  Even shards only (the data-parallel bench)."""

    def __init__(self, group=None):
        self.group = group
        self._bufs = [None, None]
        self._pending = None          # (work handle, buffer, source tensor kept alive)
        self._i = 0

    def submit(self, local):
        import torch.distributed as dist
        world = dist.get_world_size(self.group)
        done = self.flush()
        shape = (world * local.shape[0],) + tuple(local.shape[1:])
        buf = self._bufs[self._i]
        if buf is None or buf.shape != shape or buf.dtype != local.dtype or buf.device != local.device:
            buf = self._bufs[self._i] = torch.empty(shape, dtype=local.dtype, device=local.device)
        src = local.contiguous()
        work = dist.all_gather_into_tensor(buf, src, group=self.group, async_op=True)
        self._pending = (work, buf, src)
        self._i ^= 1
        return done

    def flush(self):
        if self._pending is None:
            return None
        work, buf, _ = self._pending
        work.wait()
        self._pending = None
        return buf
