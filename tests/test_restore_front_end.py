"""not-gpu: the host-side pieces every restore entry point of MarconetPipeline shares — the skip predicate, the padded locs tensor, the script's
label conversion — and the one upload of a descriptor table (ops.table_to_device), each against its written-out definition."""
import ctypes

import numpy as np
import pytest
import torch

from marconet_amd import _lib, lq_io, ops
from marconet_amd.pipeline import ALPHABET_SIZE, padded_locs, script_skips


def test_script_skips_and_padded_locs():
    n_cls = ALPHABET_SIZE
    for lab in ([], [-1], [n_cls], [0, n_cls], [3, -1, 5]):
        assert script_skips(lq_io.label_tensor(lab), n_cls) is True, lab
    for lab in ([0], [n_cls - 1], [0, n_cls - 1, 7]):
        assert script_skips(lq_io.label_tensor(lab), n_cls) is False, lab
    rows = [torch.tensor([[0.25, 0.5]]), torch.tensor([[0.1, 0.2, 0.3, 0.4, 0.5, 0.6]]), torch.tensor([[0.7, 0.8, 0.9, 1.0]])]
    locs = padded_locs(rows)
    assert locs.shape == (3, 6) and locs.dtype == torch.float32 and locs.device.type == "cpu"
    want = torch.tensor([[0.25, 0.5, 0, 0, 0, 0], [0.1, 0.2, 0.3, 0.4, 0.5, 0.6], [0.7, 0.8, 0.9, 1.0, 0, 0]])
    assert torch.equal(locs, want)


def test_label_tensor_is_the_scripts_conversion():
    text = "ab c"                                                                # the space is not in the alphabet: label -1
    want = torch.tensor(lq_io.labels_from_text(text), dtype=torch.float32).type(torch.LongTensor).unsqueeze(1)   # test_sr.py:179
    got = lq_io.label_tensor(text)
    assert int(want.min()) == -1 and want.shape == (4, 1)
    assert got.dtype == want.dtype == torch.int64 and got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(lq_io.label_tensor(lq_io.labels_from_text(text)), want)   # a list of alphabet indices
    assert lq_io.label_tensor("").shape == (0, 1) and lq_io.label_tensor("").dtype == torch.int64


@pytest.mark.parametrize("struct", [_lib.LqImage, _lib.PanelStrip, _lib.StitchLine, _lib.StitchWindow], ids=lambda s: s.__name__)
@pytest.mark.parametrize("n", [1, 3])
def test_table_to_device_keeps_every_byte(struct, n):
    size = ctypes.sizeof(struct)
    rec = np.frombuffer(np.random.default_rng(size * 10 + n).integers(0, 256, n * size, dtype=np.uint8).tobytes(), dtype=np.dtype(struct)).copy()
    assert rec.shape == (n,) and rec.dtype.itemsize == size
    got = ops.table_to_device(rec, "cpu")
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, size) and got.is_contiguous()
    assert got.numpy().tobytes() == rec.tobytes()
    if struct is _lib.LqImage:                                                   # prepare_strips' table: both rows in one copy
        two = np.stack([rec, rec[::-1]])
        got = ops.table_to_device(two, "cpu")
        assert got.dtype == torch.uint8 and tuple(got.shape) == (2, n, size) and got.numpy().tobytes() == two.tobytes()
