"""The row sets of rt_select_active_rows / rt_select_budget_rows without a device (include/rt_amd.h; csrc/rt_adaptive.h RowMap):
  1. the index arithmetic lane -> pixel, restated in numpy: strictly ascending, and exactly the shard's pixels, for every size and split
     tests/test_gpu_adaptive_multi.py runs on the device -- and those sizes reach the compaction's edges the table there names;
  2. a shard's selection is the frame's selection cut by rows: adaptive_ref's list restricted to the shard equals the list of the shard
     taken as a row_count x width frame, indices mapped back; budget_ref's budgets of that sub-frame equal the whole-frame budgets at
     those pixels while no fit rule lowers a cap -- and differ once the shard's own limit does."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_ref as ar  # noqa: E402
import adaptive_shapes as sh  # noqa: E402
import budget_ref as br  # noqa: E402
import budget_shapes as tc  # noqa: E402

# (width, height) -> the splits n run at that size (every rank r < n of each)
SPLITS = {(97, 41): (2, 3), (257, 3): (2,), (64, 5): (4,), (1, 7): (3,), (641, 409): (2,)}


def shard_rows(h, r, n):
    """the rows r, r + n, ... of a frame of h rows: (row_first, row_stride, row_count) as rt_render_rows takes them"""
    return r, n, (h - r + n - 1) // n


def row_map(w, row_first, row_stride, row_count):
    """csrc/rt_adaptive.h row_map_pixel for every lane i < row_count * w, in int32 like the device"""
    i = np.arange(row_count * w, dtype=np.int32)
    k = i // np.int32(w)
    return (np.int32(row_first) + k * np.int32(row_stride)) * np.int32(w) + (i - k * np.int32(w))


def shard_pixels(w, h, r, n):
    """the pixels of the shard, ascending, from the definition (row by row)"""
    return np.concatenate([np.arange(y * w, (y + 1) * w) for y in range(r, h, n)])


ALL = [(size, n, r) for size, ns in SPLITS.items() for n in ns for r in range(n)]


@pytest.mark.parametrize("size,n,r", ALL, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))
def test_row_map_ascends_and_covers_the_shard(size, n, r):
    w, h = size
    first, stride, count = shard_rows(h, r, n)
    assert count >= 1 and first + (count - 1) * stride < h <= first + count * stride  # rt_gather_rows' rule holds, and no row is left out
    p = row_map(w, first, stride, count)
    assert p.dtype == np.int32 and np.all(np.diff(p.astype(np.int64)) > 0)
    assert np.array_equal(p, shard_pixels(w, h, r, n))
    if stride == 1:
        assert np.array_equal(p, first * w + np.arange(count * w))  # the shortcut the device takes for consecutive rows


def test_the_shards_of_a_split_partition_the_frame():
    for (w, h), ns in SPLITS.items():
        for n in ns:
            parts = [row_map(w, *shard_rows(h, r, n)) for r in range(n)]
            assert np.array_equal(np.sort(np.concatenate(parts)), np.arange(w * h))
    assert np.array_equal(row_map(13, 0, 1, 9), np.arange(13 * 9))  # the whole frame is the row set (0, 1, height)


def test_the_sizes_reach_the_edges_they_are_listed_for():
    share = lambda size, n, r: shard_rows(size[1], r, n)[2] * size[0]  # noqa: E731
    assert [shard_rows(41, r, 2)[2] for r in range(2)] == [21, 20] and [shard_rows(41, r, 3)[2] for r in range(3)] == [14, 14, 13]
    assert all(share((97, 41), n, r) % sh.BLOCK != 0 for n in (2, 3) for r in range(n))          # ragged last block
    assert (share((257, 3), 2, 0), share((257, 3), 2, 1)) == (2 * sh.BLOCK + 2, sh.BLOCK + 1)   # two blocks plus two lanes, one plus one
    assert [shard_rows(5, r, 4)[2] for r in range(4)] == [2, 1, 1, 1] and sh.WAVE == 64         # a row is exactly one wave
    assert [share((1, 7), 3, r) for r in range(3)] == [3, 2, 2]                                  # width 1
    for r in range(2):                                                                          # more than 256 blocks: per = 1, every scan wave totals
        blocks, per, owners, _ = sh.geometry(share((641, 409), 2, r))
        assert blocks > 256 and per == 1 and owners == blocks > 4 * sh.WAVE


@pytest.fixture(scope="module")
def uneven(scenes, oracle_api):
    w, h = 97, 41
    S = tc.oracle_stack(scenes, oracle_api, "mixed_small", w, h)
    return tc.uneven_moments(S, w, h)


@pytest.mark.parametrize("n", [2, 3])
def test_a_shard_selects_what_the_frame_selects_in_its_rows(n, uneven):
    w, h = 97, 41
    cnt, sy, syy = uneven
    whole = ar.active_list(cnt, sy, syy, **tc.SELECT)
    assert 0.05 * w * h < len(whole) < 0.95 * w * h
    b_whole = br.budgets(cnt, sy, syy, 64, **tc.SELECT).reshape(-1)
    lists = []
    for r in range(n):
        rows = np.arange(r, h, n)
        p = row_map(w, *shard_rows(h, r, n))
        sub = (cnt[rows], sy[rows], syy[rows])  # the shard as a row_count x width frame
        lst, b, total, cap = br.plan(*sub, pass_cap=64, **tc.SELECT)
        assert cap == 64  # no cap lowered: the budgets are the frame's at those pixels
        assert np.array_equal(p[lst], whole[np.isin(whole, p)])
        assert np.array_equal(b, b_whole[p[lst]]) and total == int(b_whole[p].sum())
        lists.append(p[lst])
        # the shard's own limit: HALVE lists every pixel, and a limit between the shard's totals at caps 3 and 1 halves twice -- the budgets
        # are then no longer the ones the frame has at cap 7
        t7, t3, t1 = (int(br.budgets(*sub, cap, **tc.HALVE).sum()) for cap in (7, 3, 1))
        assert t7 > t3 > t1 == len(p)
        lst, b, total, cap = br.plan(*sub, pass_cap=7, max_pass_samples=t3 - 1, **tc.HALVE)
        assert cap == 1 and total == t1
        assert not np.array_equal(b, br.budgets(cnt, sy, syy, 7, **tc.HALVE).reshape(-1)[p[lst]])
    assert np.array_equal(np.sort(np.concatenate(lists)), whole)
