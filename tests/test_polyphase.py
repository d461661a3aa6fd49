"""CPU: conv3x3 ∘ bilinear×2 in polyphase form (packing.polyphase_weight) — the combined weights reproduce conv(up(x)) in fp64 away from the hi-res
ring, and the ring is exactly rows and columns {0, 1, last two}: what the ring fix-up of ops.upconv3x3_polyphase has to rewrite, no more."""
import pytest
import torch
import torch.nn.functional as F

from marconet_amd.packing import POLYPHASE_TAPS, polyphase_weight


def _both(h, w, o=3, i=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    wt = torch.randn(o, i, 3, 3, dtype=torch.float64, generator=g)
    x = torch.randn(2, i, h, w, dtype=torch.float64, generator=g)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False), wt, padding=1)
    wp = polyphase_weight(wt.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)                      # [4 O, I, 3, 3], phase-major
    y = F.conv2d(x, wp, padding=1).reshape(2, 2, 2, o, h, w).permute(0, 3, 4, 1, 5, 2).reshape(2, o, 2 * h, 2 * w)      # pixel shuffle
    return y, ref


@pytest.mark.parametrize("h,w", [(4, 4), (5, 7), (4, 7), (7, 6), (8, 32)])
def test_combined_weights_reproduce_conv_of_upsample_on_the_interior(h, w):
    y, ref = _both(h, w)
    assert (y - ref)[:, :, 2:-2, 2:-2].abs().max().item() <= 1e-13


@pytest.mark.parametrize("h,w", [(5, 7), (6, 4), (8, 9)])
def test_the_ring_is_exactly_rows_and_columns_0_1_and_the_last_two(h, w):
    y, ref = _both(h, w, seed=1)
    differs = ((y - ref).abs() > 1e-9).any(dim=1).any(dim=0)          # [2h, 2w]
    ring = torch.zeros_like(differs)
    ring[:2] = ring[-2:] = True
    ring[:, :2] = ring[:, -2:] = True
    assert torch.equal(differs, ring), "random operands differ on every ring pixel and on no other"


def test_every_hi_res_tap_is_spread_over_low_res_taps_with_unit_weight():
    # column r of a phase's table holds the up-sample's two coefficients of hi-res tap r: they sum to one
    for p in range(2):
        for r in range(3):
            assert sum(POLYPHASE_TAPS[p][a][r] for a in range(3)) == 1.0


def test_only_3x3_filters():
    with pytest.raises(ValueError):
        polyphase_weight(torch.zeros(4, 1, 1, 2))
