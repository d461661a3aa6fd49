"""The pages tests/test_layout.py and tests/test_layout_gpu.py find lines on (marconet_amd/layout.py), shared not copied.

``two_columns``: the scene the cut rules were tried on, scaled down — a 400 x 600 page, text_h = 12: a left column of 12 lines at pitch 14 and a
right one of 11 lines at pitch 15 that starts 2 rows lower, so every row of the band holds ink of one of them and no page row separates the
columns (the precondition is asserted); a gutter of ``gutter`` >= gap_x = 24 blank pixels between the columns' widest lines; one wide line below;
paper noise of amplitude 5 around 230 (luma differences up to 10, under the floor of 24).  A glyph is a block 5..9 px wide of random two-level
texture (30 / 110) whose first and last column are dark on every row, 3 px of paper between two glyphs; the lines end ragged.

``random_page``: paper noise with seeded rectangles of texture, specks and rules on it — nothing is known about what the cut returns but its
properties."""
import numpy as np

TEXT_H, PAPER, NOISE, FLOOR = 12, 230, 5, 24


def paper(rng, H, W):
    return (PAPER + rng.integers(-NOISE, NOISE + 1, (H, W, 1))).astype(np.uint8).repeat(3, axis=2)


def draw_line(rng, page, x1, y1, x2, y2):
    """glyph blocks from x1 to at most x2 on the rows [y1, y2) → the line's true right end"""
    x = x1
    while True:
        gw = int(rng.integers(5, 10))
        if x + gw > x2:
            return x - 3
        tex = rng.integers(0, 2, (y2 - y1, gw))
        tex[:, 0] = tex[:, -1] = 1
        page[y1:y2, x:x + gw] = np.where(tex, 30, 110).astype(np.uint8)[..., None]
        x += gw + 3


def two_columns(seed=7, gutter=30, wide=True):
    """→ (page uint8 [600, 400, 3], the drawn lines [x1, y1, x2, y2] in reading order: left column, right column, the wide line).  ``gutter``: the
    blank pixels of the X profile between the columns — from the pixel right of the left column's widest line to the pixel left of the right
    column, both of which belong to an edge"""
    rng = np.random.default_rng(seed)
    page, lines, right_x = paper(rng, 600, 400), [], None
    for left, y0, pitch, count in ((True, 40, 14, 12), (False, 42, 15, 11)):
        xa = 30 if left else right_x
        col = []
        for k in range(count):
            y = y0 + k * pitch
            col.append([xa, y, draw_line(rng, page, xa, y, xa + 150 - int(rng.integers(0, 30)), y + TEXT_H), y + TEXT_H])
        lines.append(col)
        right_x = max(b[2] for b in col) + 2 + int(gutter)
    if wide:
        lines.append([[30, 240, draw_line(rng, page, 30, 240, max(b[2] for b in lines[1]), 240 + TEXT_H), 240 + TEXT_H]])
    inked = np.zeros(600, bool)
    for col in lines[:2]:
        for b in col:
            inked[b[1]:b[3]] = True
    assert inked[40:42 + 10 * 15 + TEXT_H].all(), "no page row separates the two columns"
    return page, [b for col in lines for b in col]


def expected_tight(lines):
    """a drawn line as the cut finds it: the background pixel on either side of its outermost vertical edges belongs to it"""
    return [[b[0] - 1, b[1], b[2] + 1, b[3]] for b in lines]


def specks_and_figure(seed=11):
    """→ (page uint8 [200, 300, 3], its one text line): beside the line things that are no lines"""
    rng = np.random.default_rng(seed)
    page = paper(rng, 200, 300)
    line = [40, 30, draw_line(rng, page, 40, 30, 200, 42), 42]
    page[100, 250] = 0                                                                              # a speck: 1 row, 3 pixels with its edges
    page[120, 20:120] = 20                                                                          # a rule: flat inside, so only its two ends hold ink
    page[140:144, 270:272] = 0                                                                      # 4 rows, but 4 px wide with its edges: under min_w = 6
    page[150:199, 30:90] = np.where(rng.integers(0, 2, (49, 60)), 30, 110).astype(np.uint8)[..., None]     # a figure: 49 rows > max_h = 48
    return page, line


def random_page(seed):
    """a page 90..220 px a side: texture rectangles, single-pixel specks and one-row rules on noisy paper"""
    rng = np.random.default_rng(seed)
    H, W = int(rng.integers(90, 221)), int(rng.integers(90, 221))
    page = paper(rng, H, W)
    for _ in range(int(rng.integers(0, 9))):
        h, w = int(rng.integers(2, 30)), int(rng.integers(2, 60))
        y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        page[y:y + h, x:x + w] = np.where(rng.integers(0, 2, (h, w)), 30, 110).astype(np.uint8)[..., None]
    for _ in range(int(rng.integers(0, 6))):
        page[int(rng.integers(0, H)), int(rng.integers(0, W))] = int(rng.integers(0, 120))
    if rng.integers(0, 2):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W // 2))
        page[y, x:x + int(rng.integers(8, W // 2))] = 20
    return page
