"""CPU: the closed-form tap mask of the LDS-DMA kernels' per-tile set-up against the definition it replaced — bit t = r*kw + q is set iff input
row ih0 + r lies in [0, H) and input column iw0 + q in [0, valid_w).  The expression exists twice on the device, and this transcribes both copies:
marconet_amd/csrc/conv_igemm_dma.hip, setup() (every lock-step and software-pipelined tile) and marconet_amd/csrc/conv_dma_w4.hip, setup() (the
one-wave tile, fp16+8 id 16).  The device code computes (column range) * (row range of rowrep) with 32-bit shifts that are only defined below 32: the
clamps (min(kw, .), min(kh, .): a padding beyond the filter must not reach the shifts) and the sh_hi / sh_lo >= 32 guards are part of what is
checked.  The device code itself runs in tests/test_conv_geometry_gpu.py."""
import itertools


def mask_by_definition(kh, kw, ih0, iw0, h, vw):
    m = 0
    for r in range(kh):
        for q in range(kw):
            if 0 <= ih0 + r < h and 0 <= iw0 + q < vw:
                m |= 1 << (r * kw + q)
    return m


def mask_closed_form(kh, kw, ih0, iw0, h, vw):
    u32 = 0xFFFFFFFF
    rowrep = 0
    for r in range(8):
        if r < kh:
            rowrep |= 1 << (r * kw)
    qlo, qhi = min(kw, max(0, -iw0)), min(kw, vw - iw0)               # clamped like the device code
    rlo, rhi = min(kh, max(0, -ih0)), min(kh, h - ih0)
    assert 0 <= qlo <= 31 and max(qhi, 0) <= 31                      # shift counts of the device code
    cm = (((1 << max(qhi, 0)) - 1) & ~((1 << qlo) - 1)) & u32
    sh_hi, sh_lo = max(rhi, 0) * kw, rlo * kw
    assert 0 <= sh_hi <= 32 and 0 <= sh_lo <= 32                     # what the >= 32 guards below must cover, and no more
    hi = rowrep if sh_hi >= 32 else rowrep & ((1 << sh_hi) - 1)
    lo = 0 if sh_lo >= 32 else (~((1 << sh_lo) - 1)) & u32
    rr = hi & lo
    prod = cm * rr
    assert prod <= u32                                               # no carry out of 32 bits: kh * kw <= 32
    return prod


def test_closed_form_tap_mask_equals_the_definition():
    n = 0
    for kh, kw in itertools.product(range(1, 9), range(1, 9)):
        if kh * kw > 32:                                             # eligibility of the LDS-DMA path
            continue
        for ph, pw in ((0, 0), (kh // 2, kw // 2), (kh - 1, kw - 1), (min(7, kh), min(7, kw))):
            for h, w in ((1, 1), (3, 5), (4, 4), (8, 16)):
                for vw in sorted({0, 1, w // 2, w - 1, w} - {-1}):
                    for oh, ow, sh, sw in itertools.product(range(0, h + 2, max(1, h // 2)), range(0, w + 2, max(1, w // 2)), (1, 2), (1, 2)):
                        ih0, iw0 = oh * sh - ph, ow * sw - pw
                        assert mask_closed_form(kh, kw, ih0, iw0, h, vw) == mask_by_definition(kh, kw, ih0, iw0, h, vw), (kh, kw, ih0, iw0, h, vw)
                        n += 1
    assert n > 20000


def test_closed_form_tap_mask_with_pads_at_and_beyond_the_filter():
    """pads of k, k + 3 and 40 (windows wholly outside the image on every side: without the clamps the shift counts leave [0, 31]) and stride 3;
    every output position of the padded map's corners and middle"""
    n = 0
    for kh, kw in itertools.product(range(1, 9), range(1, 9)):
        if kh * kw > 32:
            continue
        for ph, pw in ((kh, kw), (kh + 3, kw + 3), (40, 40), (kh + 3, 0), (0, 40)):
            for h, w in ((1, 1), (2, 8), (4, 4)):
                for sh, sw in ((1, 1), (3, 3), (1, 3)):
                    ho, wo = (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1
                    ohs = sorted({0, 1, ph // sh, (ph + h - 1) // sh, ho // 2, ho - 1} & set(range(ho)))
                    ows = sorted({0, 1, pw // sw, (pw + w - 1) // sw, wo // 2, wo - 1} & set(range(wo)))
                    for vw in sorted({0, 1, w}):
                        for oh, ow in itertools.product(ohs, ows):
                            ih0, iw0 = oh * sh - ph, ow * sw - pw
                            assert mask_closed_form(kh, kw, ih0, iw0, h, vw) == mask_by_definition(kh, kw, ih0, iw0, h, vw), (kh, kw, ih0, iw0, h, vw)
                            n += 1
    assert n > 20000
