#!/usr/bin/env python
"""The reference's test_sr.py as ONE batch per call on the HIP path: a directory of low-quality text strips in, one panel PNG per strip out
(preview | box marks | super-resolved strip | structure priors — the file test_sr.py:232 writes, under the same name).

    python examples/restore_strips.py -i <strips dir> -o <out dir> [-m] [--precision fp16x2] [--batch 64] [--device-prep | --device-panel]
                                      [--calibrate [--calibrate-apply]] [--long-lines [--blind]]

Same flags as the script (-i / -o / -m, test_sr.py:236-241).  What differs, and why:
  * the YOLO character detector and the modelscope OCR (test_sr.py:55-56,86-96) are not part of this build (SURVEY.md §8f NEXT-4).  With
    ``-m`` the text comes from the file name as in the script (:156-158) and the boxes are evenly spaced over the strip; without it both
    come from the encoder itself (its class logits and its (left, right) predictions: MarconetPipeline.forward_blind's sources);
  * weights: the three checkpoints are looked for in ``$MARCONET_CKPT_DIR`` (the names of checkpoints/download_github.py); without them
    the seeded synthetic weights run — the panel then shows the plumbing, not a restoration;
  * all strips of a batch go through the three networks in one call (the script: one strip at a time, :77);
  * ``--device-prep`` (opt-in): the resize / canvas / normalise in front of the encoder and the 128-px preview (test_sr.py:98-115) run on the GPU
    for the whole batch (MarconetPipeline.restore_images) instead of per strip in host numpy — the same panels, byte for byte;
  * ``--device-panel`` (opt-in, implies ``--device-prep``): the panel itself (test_sr.py:203-232) is composed on the GPU too
    (MarconetPipeline.restore_panels: one launch and one device→host copy per batch) — the same files; only PNG decode / encode stay on the host.
  * ``--calibrate`` (opt-in; the first thing to run on real checkpoints): before anything is restored, the first batch's first 8 strips run in the chosen
    mode and in the fp16x3 reference mode (fp32 for ``--precision fp16x3``) on the device and the report of ``MarconetPipeline.calibrate`` is printed — is the
    mode inside half the 1e-3 parity bar on THESE weights, and at which stage does the deviation enter.  A failed check ends the program with status 2;
    with ``--calibrate-apply`` the pipeline falls back to the reference mode instead and goes on.
  * ``--long-lines`` (opt-in, needs ``-m`` or ``--blind``): a strip the script skips for its width (more than 512 px at height 32, test_sr.py:108-110) is cut into
    overlapping windows of whole characters, all windows are restored in one batch and joined on the GPU (MarconetPipeline.restore_lines); it is saved
    under the script's file name as the super-resolved line ALONE (the four-row panel is bounded by the 2048-px SR canvas).  Everything else is
    saved as before.  With ``--blind`` in the place of ``-m`` the encoder reads the wide strips too: overlapping probe windows, each keeping the
    characters well inside it (marconet_amd/blind.py), give the text and the character boxes the windows are cut by.
Needs the GPU (there is no CPU path in this package)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from marconet_amd import checkpoints, lq_io                                      # noqa: E402
from marconet_amd.pipeline import MarconetPipeline, clear_labels_batch, locs_from_left_right   # noqa: E402


def manual_strips(paths):
    """-m: text after the last underscore of the file name (test_sr.py:156-158), one evenly spaced box per character"""
    out = []
    for p in paths:
        try:
            out.append(lq_io.strip_from_png(p))
        except lq_io.StripTooWide as e:                                          # test_sr.py:108-110
            print("Warning!!! %s: %s" % (os.path.basename(p), e))
            out.append(None)
    return out


def blind_strips(pipe, paths, dev, max_glyphs=16):
    """no -m: labels = the encoder's collapsed arg-max sequence (test_w.py:34-40), boxes = its (left, right) predictions"""
    pre, out = [], []
    for p in paths:
        img = lq_io.load_png(p)
        try:
            pre.append((img,) + tuple(lq_io.lq_from_image(img)))
        except lq_io.StripTooWide as e:
            print("Warning!!! %s: %s" % (os.path.basename(p), e))
            pre.append(None)
    ok = [i for i, v in enumerate(pre) if v is not None]
    if not ok:
        return [None] * len(paths)
    with torch.no_grad():
        logits, locs_lr, _ = pipe.encoder(torch.cat([pre[i][1] for i in ok]).to(dev))
    labels = clear_labels_batch(logits)
    locs = locs_from_left_right(locs_lr).float().cpu()
    k = 0
    for i, v in enumerate(pre):
        if v is None:
            out.append(None)
            continue
        lab = labels[k][:max_glyphs]
        n = int(lab.shape[0])
        out.append(dict(lq=v[1], labels=lab, locs=locs[k:k + 1, :2 * n].contiguous(), text=lq_io.text_from_labels(lab.flatten().tolist()),
                        content_w=v[2], show_w=v[3], image=v[0]))
        k += 1
    return out


def device_strips(pipe, paths, manual, max_glyphs=16):
    """--device-prep: the strips as loaded go to the device as they are; → (strips, results) in the form the loop below consumes"""
    images = [lq_io.load_png(p) for p in paths]
    texts = [lq_io.manual_text(p) for p in paths] if manual else None
    res, strips = pipe.restore_images(images, texts=texts, with_prior=True, max_glyphs=max_glyphs, details=True)
    for p, img, s in zip(paths, images, strips):
        if s is None:
            print("Warning!!! %s: wider than %d px at height 32: crop it into shorter segments" % (os.path.basename(p), lq_io.LQ_W))
        else:
            s["image"] = img
    return strips, res


def device_panels(pipe, paths, names, manual, save_path, max_glyphs=16):
    """--device-panel: PNG in → PNG out; the host only decodes, encodes and prints the script's messages"""
    from PIL import Image
    images = [lq_io.load_png(p) for p in paths]
    texts = [lq_io.manual_text(p) for p in paths] if manual else None
    panels, strips = pipe.restore_panels(images, texts=texts, max_glyphs=max_glyphs, details=True)
    for name, panel, s in zip(names, panels, strips):
        if s is None:                                                            # test_sr.py:108-110
            print("Warning!!! %s: wider than %d px at height 32: crop it into shorter segments" % (name, lq_io.LQ_W))
        elif s["labels"].numel() == 0:                                           # test_sr.py:168-170
            print("Warning!!! No character is detected in %s. Continue..." % name)
        elif panel is None:                                                      # test_sr.py:181-190
            print("Error in %s (a character outside the alphabet). Continue..." % name)
        else:
            out = os.path.join(save_path, "%s_%s.png" % (os.path.splitext(name)[0], s["text"]))       # test_sr.py:232
            Image.fromarray(panel).save(out)
            print("Restoring %s. Using %s text: %s -> %s" % (name, "given" if manual else "predicted", s["text"], out))


def long_lines(pipe, paths, names, save_path, blind=False):
    """--long-lines: the strips of the chunk that are too wide go through restore_lines and are saved; → the positions of the others.
    ``blind``: their texts are read by the encoder (restore_lines with None per line) and not taken from the file names"""
    from PIL import Image
    from marconet_amd.long_lines import too_wide
    wide = []
    for i, p in enumerate(paths):
        with Image.open(p) as im:
            if too_wide(im.size[1], im.size[0]):
                wide.append(i)
    if wide:
        images = [lq_io.load_png(paths[i]) for i in wide]
        if blind:
            lines, _, read = pipe.restore_lines(images, [None] * len(images), details=True)
            texts = ["" if r is None else r["text"] for r in read]
            for i, r in zip(wide, read):
                if r is not None and r["overflow"]:
                    print("Warning: %s: a probe window held more than 16 characters; those beyond the sixteenth were not read" % names[i])
        else:
            texts = [lq_io.manual_text(paths[i]) for i in wide]
            lines = pipe.restore_lines(images, texts)
        for i, text, line in zip(wide, texts, lines):
            if line is None:                                                     # test_sr.py:168-170, :181-190
                print("Error in %s (no character, or a character outside the alphabet). Continue..." % names[i])
                continue
            out = os.path.join(save_path, "%s_%s.png" % (os.path.splitext(names[i])[0], text))       # test_sr.py:232
            Image.fromarray(np.ascontiguousarray(line[:, :, ::-1])).save(out)    # BGR → RGB
            print("Restoring %s as a long line of %d px. Using %s text: %s -> %s" % (names[i], line.shape[1], "predicted" if blind else "given", text, out))
    return [i for i in range(len(paths)) if i not in wide]


def calibrate_on(pipe, strips, dev, reference, apply):
    """MarconetPipeline.calibrate on the strips of the first batch (the batch layout of MarconetPipeline.restore_strips) → the report, or None when the
    batch holds no strip with a character of the alphabet"""
    n_cls = pipe.gan.TextGenerator.class_num
    keep = [s for s in strips if s is not None and s["labels"].numel() > 0 and int(s["labels"].min()) >= 0 and int(s["labels"].max()) < n_cls]
    if not keep:
        return None
    locs = torch.zeros((len(keep), 2 * max(int(s["labels"].shape[0]) for s in keep)), dtype=torch.float32)
    for k, s in enumerate(keep):
        locs[k, :s["locs"].shape[1]] = s["locs"][0]
    return pipe.calibrate(torch.cat([s["lq"] for s in keep]).to(dev), [s["labels"] for s in keep], locs, reference=reference, apply=apply)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-i", "--test_path", type=str, default="./Testsets/LQs")
    ap.add_argument("-o", "--save_path", type=str, default=None)
    ap.add_argument("-m", "--manual", action="store_true")
    ap.add_argument("--precision", default="fp16x2", choices=["fp16x2", "fp16x3", "fp16", "fp32"])
    ap.add_argument("--batch", type=int, default=64, help="strips per call")
    ap.add_argument("--device-prep", action="store_true", help="resize / normalise the strips on the GPU (MarconetPipeline.restore_images)")
    ap.add_argument("--device-panel", action="store_true", help="also compose the saved panel on the GPU (MarconetPipeline.restore_panels); implies --device-prep")
    ap.add_argument("--calibrate", action="store_true", help="check the precision mode against a more accurate one on the first batch (MarconetPipeline.calibrate) and exit with status 2 if it fails")
    ap.add_argument("--calibrate-apply", action="store_true", help="with --calibrate: fall back to the reference mode instead of exiting")
    ap.add_argument("--long-lines", action="store_true", help="with -m or --blind: restore strips wider than 512 px at height 32 window by window and join them (MarconetPipeline.restore_lines)")
    ap.add_argument("--blind", action="store_true", help="with --long-lines: the encoder reads the wide strips' text and character boxes itself (restore_lines with None as their texts)")
    a = ap.parse_args()
    if a.blind and not a.long_lines:
        ap.error("--blind applies to --long-lines (a strip of at most 512 px at height 32 is read blind without -m anyway)")
    if a.long_lines and not (a.manual or a.blind):
        ap.error("--long-lines needs -m or --blind: a window is a run of whole characters, so the text is given (-m) or read by the encoder (--blind)")
    save_path = a.save_path or a.test_path.rstrip("/") + "_" + time.strftime("%m-%d_%H-%M", time.localtime()) + "_MARCONet"
    os.makedirs(save_path, exist_ok=True)
    if not torch.cuda.is_available():
        raise SystemExit("restore_strips.py: no GPU visible — this package has no CPU path")
    dev = "cuda"
    sde, sdg, sds, source = checkpoints.load_state_dicts()
    print("%28s : %s" % ("Weights", source))
    pipe = MarconetPipeline(*checkpoints.build_networks(sde, sdg, sds, dev), precision=a.precision)
    names = sorted(f for f in os.listdir(a.test_path) if f.lower().endswith((".png", ".jpg", ".jpeg", ".bmp")))
    for s0 in range(0, len(names), a.batch):
        chunk = names[s0:s0 + a.batch]
        paths = [os.path.join(a.test_path, f) for f in chunk]
        if a.long_lines:
            rest = long_lines(pipe, paths, chunk, save_path, blind=a.blind and not a.manual)
            chunk, paths = [chunk[i] for i in rest], [paths[i] for i in rest]
            if not chunk:
                continue
        if a.calibrate and s0 == 0:
            if a.precision == "fp32":
                print("%28s : nothing to check, fp32 is the parity mode" % "Precision margin")
            else:
                report = calibrate_on(pipe, manual_strips(paths) if a.manual else blind_strips(pipe, paths, dev), dev,
                                      "fp32" if a.precision == "fp16x3" else "fp16x3", a.calibrate_apply)
                print(report if report is not None else "Precision margin: no strip with characters in the first batch, nothing checked")
                if report is not None and not report.ok and not report.applied:
                    raise SystemExit(2)
        if a.device_panel:
            device_panels(pipe, paths, chunk, a.manual, save_path)
            continue
        if a.device_prep:
            strips, done = device_strips(pipe, paths, a.manual)
        else:
            strips = manual_strips(paths) if a.manual else blind_strips(pipe, paths, dev)
        live = [i for i, s in enumerate(strips) if s is not None and s["labels"].numel() > 0]
        for i, s in enumerate(strips):
            if s is not None and s["labels"].numel() == 0:
                print("Warning!!! No character is detected in %s. Continue..." % chunk[i])          # test_sr.py:168-170
        res = [done[i] for i in live] if a.device_prep else pipe.restore_strips([strips[i] for i in live], with_prior=True)
        for i, r in zip(live, res):
            s = strips[i]
            if r is None:                                                        # a character outside the alphabet (test_sr.py:181-190)
                print("Error in %s (a character outside the alphabet). Continue..." % chunk[i])
                continue
            show_sr, prior128 = r
            n = int(s["labels"].shape[0])
            base = os.path.splitext(chunk[i])[0]
            out = os.path.join(save_path, "%s_%s.png" % (base, s["text"]))       # test_sr.py:232
            lq_io.save_panel(out, lq_io.panel(s["image"], s["locs"][0], n, show_sr, prior128, show=s.get("show")))
            print("Restoring %s. Using %s text: %s -> %s" % (chunk[i], "given" if a.manual else "predicted", s["text"], out))


if __name__ == "__main__":
    main()
