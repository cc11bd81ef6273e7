"""tests/support.py on crafted inputs, without a device: the knob list against the source that reads the knobs, the bitwise comparisons
every exactness claim of the GPU tier rests on, the snapshot comparison of the adaptive tests, and clean_env."""
import os
import re

import numpy as np

import support as sp
from conftest import ROOT

F32 = np.float32


def test_knobs_are_the_ones_read_knobs_reads():
    src = open(os.path.join(ROOT, "ray-and-pathtracer_amd", "csrc", "rt_ctx.h")).read()
    read = re.findall(r'num\("(RT_[A-Z0-9_]+)"', src)
    assert set(sp.KNOBS) == set(read) and len(sp.KNOBS) == len(set(sp.KNOBS)) == 19
    first = sorted(set(read), key=read.index)
    assert list(sp.KNOBS) == first  # ... in the order it reads them


def _nan(payload):
    return np.array([0x7FC00000 | payload], np.uint32).view(F32)


def test_bits_and_same():
    assert not sp.same(F32([0.0]), F32([-0.0])) and F32(0.0) == F32(-0.0)
    assert not sp.same(_nan(1), _nan(2))
    assert sp.same(_nan(1), _nan(1)) and not np.array_equal(_nan(1), _nan(1))
    a = np.arange(6, dtype=F32)
    assert np.array_equal(a.reshape(2, 3), a.reshape(2, 3)) and not sp.same(a.reshape(2, 3), a.reshape(3, 2)) and not sp.same(a, a[:5])
    assert sp.same(a, a.copy()) and sp.same_state((a, _nan(1)), (a.copy(), _nan(1))) and not sp.same_state((a, _nan(1)), (a, _nan(2)))
    m = np.arange(24, dtype=F32).reshape(4, 6)
    part = m[1::2, ::2]
    assert not part.flags["C_CONTIGUOUS"]
    assert np.array_equal(sp.bits(part), sp.bits(part.copy())) and sp.bits(part).dtype == np.uint32 and sp.bits(part).shape == (2, 3)
    assert np.array_equal(sp.bits(F32([1.0, -0.0])), np.array([0x3F800000, 0x80000000], np.uint32))


def _crafted():
    """a 2 x 3 state with counts 0, 1 and 2 and the three snapshots it is made of"""
    rng = np.random.default_rng(3)
    snaps = [(rng.random((2, 3, 4)).astype(F32), np.full((2, 3), n, np.uint32), rng.random((2, 3)).astype(F32), rng.random((2, 3)).astype(F32)) for n in range(3)]
    cnt = np.array([[0, 1, 2], [2, 1, 0]], np.uint32)
    st = [np.zeros((2, 3, 4), F32), cnt, np.zeros((2, 3), F32), np.zeros((2, 3), F32)]
    for n in range(3):
        for k in (0, 2, 3):
            st[k][cnt == n] = snaps[n][k][cnt == n]
    return st, snaps


def test_differs_from_snapshot_of_its_count():
    st, snaps = _crafted()
    assert sp.differs_from_snapshot_of_its_count(st, snaps) is None
    assert sp.differs_from_snapshot_of_its_count(st, snaps, np.ones((2, 3), bool)) is None
    syy = st[3].copy()
    syy[0, 2] = np.nextafter(syy[0, 2], F32(2.0))  # a pixel with count 2, one ulp off
    assert sp.bits(syy)[0, 2] == sp.bits(st[3])[0, 2] + 1
    off = (st[0], st[1], st[2], syy)
    what = sp.differs_from_snapshot_of_its_count(off, snaps)
    assert what is not None and "count 2" in what
    where = np.ones((2, 3), bool)
    assert "count 2" in sp.differs_from_snapshot_of_its_count(off, snaps, where)
    where[0, 2] = False
    assert sp.differs_from_snapshot_of_its_count(off, snaps, where) is None  # the other pixel with count 2 is still compared, and equal
    acc = st[0].copy()
    acc[1, 1, 3] = -acc[1, 1, 3]  # ... and the accumulator of a pixel with count 1
    assert "count 1" in sp.differs_from_snapshot_of_its_count((acc, st[1], st[2], st[3]), snaps)


def test_clean_env(monkeypatch):
    monkeypatch.setenv("RT_WIDE", "1")
    monkeypatch.setenv("RT_LEVEL_CAP", "256")
    monkeypatch.setenv("RT_NOT_A_KNOB", "7")
    sp.clean_env(monkeypatch, {"RT_FUSE": "1"})
    assert {k: v for k, v in os.environ.items() if k in sp.KNOBS} == {"RT_FUSE": "1"}
    assert os.environ["RT_NOT_A_KNOB"] == "7"
    sp.clean_env(monkeypatch)
    assert not set(os.environ) & set(sp.KNOBS)


def test_small_helpers():
    assert sp.env_id({}) == "default" and sp.env_id({"RT_STREAM": "0", "RT_SLOTS": "777"}) == "RT_STREAM=0,RT_SLOTS=777"
    assert sp.layout_knobs() == sp.layout_knobs({}) == (-1, 0, 1)
    assert sp.layout_knobs({"RT_TLAS_LDS": "0", "RT_WIDE": "1", "RT_WIDE8": "1"}) == (1, 1, 0)
