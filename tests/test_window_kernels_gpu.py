"""-m gpu: mnet_lq_windows_u8 / lq_device.prepare_windows — the encoder's input from windows that are VIEWS of images on the device — against
lq_device.prepare_strips of the same pixels copied out on the host: every comparison is torch.equal.  The page is random, so a clamp into the
page instead of into the window changes bits at every window edge that is not the page's.  The references are computed once per module."""
import numpy as np
import pytest
import torch

from marconet_amd import _lib, long_lines, lq_device, lq_io, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAGE_H, PAGE_W = 97, 211
IMG2_H, IMG2_W = 40, 55
PAGE_AT, GAP = 7, 3           # the page begins at an odd byte; so does the second image, GAP bytes behind it
GUARD = 4096


def _widest(h, most):
    """the widest window of height h, at most ``most`` columns, that ``shape_geometry`` accepts"""
    w = most
    while long_lines.too_wide(h, w):
        w -= 1
    return w


def _page_windows():
    """(x, y, h, w) in the page"""
    wins = []
    for h, x, y in ((8, 3, 5), (31, 10, 60), (32, 1, 33), (33, 0, 64), (97, 0, 0)):
        for w in (1, 2, _widest(h, PAGE_W - x)):
            if h == 97 and w == 1:
                continue                                         # rint(32 / 97) = 0 columns: refused, below
            wins.append((x, y, h, w))
    wins.append((40, 80, 8, 128))                                # dw == 512 exactly
    wins += [(0, 0, 20, 30), (PAGE_W - 30, 0, 20, 30), (0, PAGE_H - 20, 20, 30), (PAGE_W - 30, PAGE_H - 20, 20, 30)]      # the page's corners
    wins.append((50, 30, 20, 40))                                # strictly inside: every edge of the window has other pixels behind it
    wins += [(40, 10, 32, 100), (90, 20, 32, 100)]               # two that overlap
    wins.append((0, 0, PAGE_H, PAGE_W))                          # the whole page
    return wins


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(20250117)
    page = rng.integers(0, 256, (PAGE_H, PAGE_W, 3), dtype=np.uint8)
    img2 = rng.integers(0, 256, (IMG2_H, IMG2_W, 3), dtype=np.uint8)
    at2 = PAGE_AT + page.size + GAP
    assert PAGE_AT % 2 == 1 and at2 % 2 == 1
    buf = rng.integers(0, 256, (at2 + img2.size + 5,), dtype=np.uint8)
    buf[PAGE_AT:PAGE_AT + page.size] = page.reshape(-1)
    buf[at2:at2 + img2.size] = img2.reshape(-1)
    wins, crops = [], []
    for x, y, h, w in _page_windows():
        wins.append((PAGE_AT + (y * PAGE_W + x) * 3, PAGE_W * 3, h, w))
        crops.append(np.ascontiguousarray(page[y:y + h, x:x + w]))
    for x, y, h, w in ((0, 0, IMG2_H, IMG2_W), (5, 4, 32, 50), (IMG2_W - 9, IMG2_H - 9, 9, 9)):          # the image of another pitch
        wins.append((at2 + (y * IMG2_W + x) * 3, IMG2_W * 3, h, w))
        crops.append(np.ascontiguousarray(img2[y:y + h, x:x + w]))
    want = lq_device.prepare_strips(crops, DEV)                  # the existing kernel on the host crops: the reference, computed once
    assert 512 in want.content_w and 1 in want.content_w and len(wins) == 26
    return dict(src=torch.from_numpy(buf).to(DEV), wins=wins, want=want)


def test_windows_equal_the_host_crops_bit_for_bit(data):
    got = lq_device.prepare_windows(data["src"], data["wins"])
    assert got.lq.shape == (len(data["wins"]), 3, 32, 512) and got.lq.dtype == torch.float32
    assert torch.equal(got.lq, data["want"].lq)
    assert got.content_w == data["want"].content_w and got.index == list(range(len(data["wins"]))) and got.preview is None and got.skipped == []
    assert got.show_w == [lq_device.shape_geometry(h, w).show_w for _, _, h, w in data["wins"]]


@pytest.mark.parametrize("n", (1, 70))
def test_any_batch_size_in_one_launch_leaves_the_guards_alone(data, n):
    pick = [(5 * k + 3) % len(data["wins"]) for k in range(n)]
    wins = [data["wins"][j] for j in pick]
    table = ops.table_to_device(lq_device.window_table(lq_device.check_windows(wins, data["src"].numel()), wins), DEV)
    size = n * 3 * 32 * 512
    buf = torch.full((size + 2 * GUARD,), float(np.frombuffer(b"\xcd" * 4, np.float32)[0]), dtype=torch.float32, device=DEV)
    out = buf[GUARD:GUARD + size].view(n, 3, 32, 512)
    got = ops.lq_windows_u8(data["src"], table, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(got, data["want"].lq[torch.tensor(pick, device=DEV)])
    raw = buf.view(torch.uint8)
    assert bool((raw[:4 * GUARD] == 0xCD).all()) and bool((raw[4 * (GUARD + size):] == 0xCD).all())


def test_the_wrapper_refuses_every_bad_descriptor_before_a_launch(data):
    src, nbytes, pitch = data["src"], data["src"].numel(), PAGE_W * 3
    good = data["wins"][0]
    for bad, exc in (((PAGE_AT, pitch, 0, 5), ValueError), ((PAGE_AT, pitch, 5, 0), ValueError), ((PAGE_AT, pitch, 97, 1), ValueError),
                     ((PAGE_AT, pitch, 8, 131), lq_io.StripTooWide), ((-1, pitch, 4, 4), ValueError), ((PAGE_AT, 11, 4, 4), ValueError),
                     ((nbytes - 11, pitch, 1, 4), ValueError), ((PAGE_AT, pitch, PAGE_H + 12, PAGE_W), ValueError)):       # its last row ends beyond the buffer
        with pytest.raises(exc):
            lq_device.prepare_windows(src, [good, bad])
    with pytest.raises(ValueError, match="at least one window"):
        lq_device.prepare_windows(src, [])
    with pytest.raises(TypeError):
        lq_device.prepare_windows(src.float(), [good])
    with pytest.raises(TypeError):
        ops.lq_windows_u8(src, torch.zeros((2, 24), dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError, match="out must be"):
        ops.lq_windows_u8(src, torch.zeros((2, 32), dtype=torch.uint8, device=DEV), out=torch.zeros((2, 3, 32, 256), device=DEV))


def test_the_kernel_writes_a_descriptor_it_cannot_follow_as_fill(data):
    """the table is the caller's: what ``prepare_windows`` refuses never reaches the kernel through it, and a hand-made table cannot take the kernel
    out of ``src`` — h < 1, w < 1, pitch < 3 w, a negative offset and a last row that ends beyond ``src`` give the fill, the neighbours their bits"""
    nbytes, pitch = data["src"].numel(), PAGE_W * 3
    g = lq_device.shape_geometry(20, 30)
    tab = np.zeros((7,), dtype=np.dtype(_lib.LqWindow))
    tab[0] = (data["wins"][0][0], pitch, data["wins"][0][2], data["wins"][0][3], data["want"].content_w[0], lq_device.shape_geometry(*data["wins"][0][2:]).scale)
    tab[1] = (PAGE_AT, pitch, 0, 30, g.dw, g.scale)
    tab[2] = (PAGE_AT, pitch, 20, 0, g.dw, g.scale)
    tab[3] = (PAGE_AT, 89, 20, 30, g.dw, g.scale)
    tab[4] = (-3, pitch, 20, 30, g.dw, g.scale)
    tab[5] = (nbytes - 19 * pitch - 89, pitch, 20, 30, g.dw, g.scale)          # its last row ends one byte beyond src
    tab[6] = (nbytes - 19 * pitch - 90, pitch, 20, 30, g.dw, g.scale)          # ... and this one's on src's last byte
    got = ops.lq_windows_u8(data["src"], ops.table_to_device(tab, DEV))
    assert torch.equal(got[0], data["want"].lq[0])
    assert bool((got[1:6] == -1.0).all())
    host = data["src"].cpu().numpy()
    last = np.stack([host[int(tab[6]["offset"]) + r * pitch:][:90] for r in range(20)]).reshape(20, 30, 3)
    assert torch.equal(got[6], lq_device.prepare_strips([last], DEV).lq[0])
