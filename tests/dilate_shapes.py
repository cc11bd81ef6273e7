"""Frame sizes and crafted cases for the dilated-selection tests.  A plain helper module of the test suite, numpy only:
tests/test_gpu_dilate.py crafts the statistics of every case on the device, tests/test_dilate_cpu.py checks without a device that every
builder returns what its name says and that every size reaches the edge it is listed for.

The dilation (csrc/rt_dilate.h) works on bitmasks over the linear pixel index p = y * width + x, 64 pixels per word, written by waves of
64 lanes in blocks of 256; what can go wrong is the row clip where the width is no multiple of 64, the clear high bits of the last word,
and a read one word past the end.  A case is (name, sources, stopped): 'sources' are the pixels that get no samples (raw-active under
CRAFT), 'stopped' (or None) pixels that get one sample more than the rest and so sit at max_samples: dilation must not list them."""
import numpy as np

WORD = 64
BLOCK = 256  # RT_SELECT_BLOCK
SCAN = 1024  # RT_SELECT_SCAN_BLOCK

# under these, raw = count < 2 and eligible = count < 3 with finite sums, whatever the moments are
CRAFT = dict(min_samples=2, max_samples=3, threshold=float("inf"), floor=1.0)
RADII = (0, 1, 2, 16)

# (width, height) -> what the size is in the suite for
SIZES = {
    (1, 1): "one lane",
    (63, 1): "a partial wave: the high bit of the only word stays clear",
    (65, 1): "a wave and a lane: a row across two words, one bit in the last",
    (1, 67): "a column: 64 rows in a word, every horizontal window one pixel",
    (5, 40): "several rows in a word, rows straddling words unevenly (5 does not divide 64)",
    (64, 5): "rows equal words",
    (65, 4): "a row one pixel over a word: every row starts at another bit",
    (257, 3): "ragged blocks: 3 pixels in the last block",
    (97, 41): "ragged: the last wave of the last block is partial; a light in view",
    (641, 409): "more blocks than the scan has lanes: its second entry per lane",
}


def geometry(w, h):
    """(pixels, words of a mask, blocks of a launch, entries per lane of the scan)"""
    n = w * h
    blocks = (n + BLOCK - 1) // BLOCK
    return n, (n + WORD - 1) // WORD, blocks, (blocks + SCAN - 1) // SCAN


def _px(w, h, points):
    m = np.zeros((h, w), bool)
    for x, y in points:
        m[y, x] = True
    return m


def _block_around(w, h, x, y, reach):
    m = np.zeros((h, w), bool)
    m[max(y - reach, 0):y + reach + 1, max(x - reach, 0):x + reach + 1] = True
    return m


def cases(w, h):
    """[(name, sources (h, w) bool, stopped (h, w) bool or None)]; a case whose two masks equal an earlier case's is left out (at small
    sizes the corners, the pixels and the rows coincide)"""
    n = w * h
    y = h // 2
    out = [("none", np.zeros((h, w), bool), None), ("all", np.ones((h, w), bool), None),
           ("top_left", _px(w, h, [(0, 0)]), None), ("top_right", _px(w, h, [(w - 1, 0)]), None),
           ("bottom_left", _px(w, h, [(0, h - 1)]), None), ("bottom_right", _px(w, h, [(w - 1, h - 1)]), None)]
    if h >= 2:
        yy = (h - 2) // 2                                              # (both mid-frame from 4 rows on; below, one of them is a corner)
        out.append(("row_end", _px(w, h, [(w - 1, yy)]), None))        # must not light column 0 of the next row (unless the window does)
        out.append(("row_start", _px(w, h, [(0, yy + 1)]), None))      # ... nor the end of the row before
    for p in (63, 64):                                                 # either side of the first word boundary
        if p < n:
            out.append(("pixel%d" % p, _px(w, h, [(p % w, p // w)]), None))
    row = np.zeros((h, w), bool)
    row[y] = True
    col = np.zeros((h, w), bool)
    col[:, w // 2] = True
    out += [("one_row", row, None), ("one_column", col, None)]
    if n >= 300:
        src = np.zeros(n, bool)
        src[np.random.default_rng(3000 + n).choice(n, (n + 50) // 100, replace=False)] = True
        stopped = (np.random.default_rng(4000 + n).random(n) < 0.05) & ~src
        out.append(("seeded_01", src.reshape(h, w), stopped.reshape(h, w)))
    # the stopped class next to a source: the 5 x 5 block around a mid-frame source, without the source
    s = _px(w, h, [(w // 2, y)])
    ring = _block_around(w, h, w // 2, y, 2) & ~s
    if ring.any():
        out.append(("stopped_ring", s, ring))
    seen, kept = set(), []
    for name, src, stopped in out:
        key = (src.tobytes(), None if stopped is None else stopped.tobytes())
        if key not in seen:
            seen.add(key)
            kept.append((name, src, stopped))
    return kept


def complement_list(mask):
    """the list to render so that exactly the pixels of 'mask' stay without samples"""
    return np.flatnonzero(~np.asarray(mask, bool).reshape(-1)).astype(np.uint32)


def crafted_counts(sources, stopped):
    """the counts the crafting leaves: 0 on the sources, 3 on the stopped pixels, 2 elsewhere"""
    c = np.where(sources, 0, 2)
    if stopped is not None:
        c = np.where(stopped, 3, c)
    return c.astype(np.uint32)
