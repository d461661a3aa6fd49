"""Labels and locations between the encoder and the generator: the small helpers the inference core (``pipeline``) and the restore front end
(``restore``, ``blind``) share.  A leaf: of the package it needs only ``ops``, for ``clear_labels_batch``'s argmax kernel."""
import torch

from . import ops

ALPHABET_SIZE = 6735          # utils/alphabets.py: 6735 characters; class 6735 = blank / padding


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
