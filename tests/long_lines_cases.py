"""The long line shared by tests/test_long_lines.py (its window count, on the CPU) and tests/test_long_lines_gpu.py (through the networks)."""
import os

import numpy as np

from marconet_amd import lq_io
from tests.golden import cases_png

LINE_PNGS = ("real_lq13.png", "w1.png", "w2.png", "real_lq13.png")       # the reference strips of height 32, side by side: 1321 px


def golden_line():
    """→ (uint8 RGB [32, 1321, 3], a text of 40 characters of the alphabet: the manual labels of the reference's two labelled strips, repeated)"""
    img = np.hstack([lq_io.load_png(os.path.join(cases_png.PNG_DIR, f)) for f in LINE_PNGS])
    text = "".join(lq_io.manual_text(f) for f in cases_png.SR_STRIPS.values())
    return np.ascontiguousarray(img), (text * 3)[:40]
