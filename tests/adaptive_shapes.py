"""Frame sizes, crafted masks and pixel lists for the adaptive-sampling shape tests.  A plain helper module of the test suite, numpy
only: tests/test_gpu_adaptive_shapes.py drives rt_select_active / rt_render_active with them, tests/test_adaptive_cpu.py checks on a
machine without a device that every builder returns what its name says and that every size reaches the edge it is listed for.

The selection's compaction (csrc/rt_adaptive.h) is three launches: a block of BLOCK lanes owns BLOCK consecutive pixels and counts its
active ones in waves of WAVE lanes; one block of SCAN lanes scans the block totals, every lane owning a run of 'per' consecutive totals;
the scatter ranks the pixels again.  geometry() restates that arithmetic, so a change to the two constants in the library makes the
tests say that their sizes no longer reach the edges."""
import numpy as np

BLOCK = 256   # RT_SELECT_BLOCK
SCAN = 1024   # RT_SELECT_SCAN_BLOCK
WAVE = 64

# (width, height) -> (pixels, blocks of the count / scatter launches, entries per lane of the scan): what each size is in the suite for
SIZES = {
    (1, 1): (1, 1, 1),              # one lane
    (63, 1): (63, 1, 1),            # a partial wave
    (65, 1): (65, 1, 1),            # one full wave plus one lane
    (255, 1): (255, 1, 1),          # one short of a block
    (257, 3): (771, 4, 1),          # ragged, 3 pixels in the last block
    (97, 41): (3977, 16, 1),        # ragged, the last wave of the last block is partial
    (641, 409): (262169, 1025, 2),  # per = 2: scan lane 512 owns one entry, lanes 513 and up are clamped to empty
    (1280, 721): (922880, 3605, 4),  # per = 4: 902 owning lanes, the last owns one entry; the last block is full
    (1279, 721): (922159, 3603, 4),  # per = 4: 901 owning lanes, the last owns three; ragged last block
}
# the parameters under which exactly the pixels without samples are active, whatever their moments (count < min_samples)
CRAFT = dict(min_samples=2, max_samples=2, threshold=0.0, floor=1.0)


def geometry(n):
    """pixels -> (blocks, per, owners, last_owns): the launches' blocks, the scan's entries per lane, the scan lanes that own at least
    one entry and how many the last of them owns"""
    blocks = (n + BLOCK - 1) // BLOCK
    per = (blocks + SCAN - 1) // SCAN
    owners = (blocks + per - 1) // per
    return blocks, per, owners, blocks - (owners - 1) * per


def _blocks_mask(n, first, last):
    """every pixel of blocks [first, last)"""
    m = np.zeros(n, bool)
    m[first * BLOCK:last * BLOCK] = True
    return m


def _all(w, h):
    return np.ones(w * h, bool)


def _none(w, h):
    return np.zeros(w * h, bool)


def _first(w, h):
    n = w * h
    if n == 1:
        return None  # the frame itself
    m = np.zeros(n, bool)
    m[0] = True
    return m


def _last(w, h):
    n = w * h
    if n == 1:
        return None
    m = np.zeros(n, bool)
    m[n - 1] = True
    return m


def _last_block(w, h):
    """exactly the pixels of the last block (partial wherever the frame is ragged)"""
    n = w * h
    blocks = geometry(n)[0]
    return None if blocks == 1 else _blocks_mask(n, blocks - 1, blocks)


def _all_but_last_block(w, h):
    n = w * h
    blocks = geometry(n)[0]
    return None if blocks == 1 else _blocks_mask(n, 0, blocks - 1)


def _alternate_blocks(w, h):
    """blocks 0, 2, 4, ... full, the odd ones empty"""
    n = w * h
    if geometry(n)[0] == 1:
        return None
    return (np.arange(n) // BLOCK) % 2 == 0


def _lane0(w, h):
    n = w * h
    return None if n <= WAVE else np.arange(n) % WAVE == 0  # (one wave: the first pixel)


def _lane63(w, h):
    n = w * h
    return None if n < WAVE else np.arange(n) % WAVE == WAVE - 1  # (no full wave: no pixel)


def _every_other(w, h):
    n = w * h
    return None if n == 1 else np.arange(n) % 2 == 0


def _one_row(w, h):
    if h == 1:
        return None
    m = np.zeros((h, w), bool)
    m[h // 2] = True
    return m.reshape(-1)


def _seeded_30(w, h):
    n = w * h
    return None if n < WAVE - 1 else np.random.default_rng(1000 + n).random(n) < 0.3


def _seeded_01(w, h):
    """one pixel in a thousand, exactly: most blocks total 0"""
    n = w * h
    if n < 2000:
        return None
    m = np.zeros(n, bool)
    m[np.random.default_rng(2000 + n).choice(n, (n + 500) // 1000, replace=False)] = True
    return m


def _full_to_1023(w, h):
    """blocks 0 .. SCAN - 1 full, the rest empty (frames with more blocks than the scan has lanes)"""
    n = w * h
    return None if geometry(n)[1] == 1 else _blocks_mask(n, 0, SCAN)


def _full_from_1024(w, h):
    n = w * h
    blocks, per = geometry(n)[:2]
    return None if per == 1 else _blocks_mask(n, SCAN, blocks)


def scan_lane_blocks(n, lane):
    """the block totals scan lane 'lane' owns: [first, last)"""
    blocks, per = geometry(n)[:2]
    first = min(lane * per, blocks)
    return first, min(first + per, blocks)


def _scan_lane_mid(w, h):
    """full for exactly the entries of scan lane 64 (lane 0 of the scan's second wave: its base is the first wave's sum)"""
    n = w * h
    return None if geometry(n)[1] == 1 else _blocks_mask(n, *scan_lane_blocks(n, WAVE))


def _scan_lane_last(w, h):
    """full for exactly the entries of the last owning scan lane (a run shorter than per at every size of the table)"""
    n = w * h
    blocks, per, owners, _ = geometry(n)
    return None if per == 1 else _blocks_mask(n, *scan_lane_blocks(n, owners - 1))


# name -> builder(width, height) -> bool mask over the w * h pixels, or None where the mask is degenerate at that size by construction
# (it would be another mask of the table)
MASKS = {
    "all": _all, "none": _none, "first": _first, "last": _last, "last_block": _last_block, "all_but_last_block": _all_but_last_block,
    "alternate_blocks": _alternate_blocks, "lane0": _lane0, "lane63": _lane63, "every_other": _every_other, "one_row": _one_row,
    "seeded_30": _seeded_30, "seeded_01": _seeded_01, "full_to_1023": _full_to_1023, "full_from_1024": _full_from_1024,
    "scan_lane_mid": _scan_lane_mid, "scan_lane_last": _scan_lane_last,
}


def masks(w, h):
    """[(name, mask)] of every mask that is not degenerate at w x h"""
    out = []
    for name, fn in MASKS.items():
        m = fn(w, h)
        if m is not None:
            out.append((name, m))
    return out


def acceptable(lst, n):
    """what rt_set_active_pixels accepts for a frame of n pixels: uint32, every entry below n, strictly ascending"""
    lst = np.asarray(lst)
    return lst.dtype == np.uint32 and lst.ndim == 1 and (len(lst) == 0 or (int(lst.max()) < n and bool(np.all(np.diff(lst.astype(np.int64)) > 0))))


def complement_list(mask):
    """the list to render so that exactly the pixels of 'mask' stay without samples"""
    return np.flatnonzero(~mask).astype(np.uint32)


def seeded_list(w, h, seed=5, density=0.3):
    """about 'density' of the pixels: pixel 0, the last pixel, one complete row, a seeded rest (uint32, ascending)"""
    on = np.random.default_rng(seed).random(w * h) < max(0.0, (density - 1.0 / h) / (1.0 - 1.0 / h))  # (the row is 1 / h of the frame)
    on[0] = on[w * h - 1] = True
    on[(h // 3) * w:(h // 3 + 1) * w] = True
    return np.flatnonzero(on).astype(np.uint32)


def last_row_list(w, h):
    return np.arange((h - 1) * w, h * w, dtype=np.uint32)


def side_columns_list(w, h):
    """column 0 and column w - 1 of every row"""
    y = np.arange(h, dtype=np.uint32) * np.uint32(w)
    return np.sort(np.concatenate([y, y + np.uint32(w - 1)]))


def slots_branch(slots, listed, nframes):
    """What render_batches / trace_samples (csrc/rt_api_render.inc) do with a list of 'listed' pixels and RT_SLOTS=slots:
    ("recycle", nframes) when not even one frame of the list fits, so one batch runs on fewer slots than samples (k_finish hands the
    slots on); otherwise ("own", frames per batch), every sample with a slot of its own and the call cut into batches of that many frames."""
    if listed > slots:
        return "recycle", nframes
    return "own", min(nframes, slots // listed)
