"""The Q-learning guided sampler (csrc/rt_qlearn.h, rt_api_qlearn.inc, the QL instantiation of k_shade_s) on crafted tables, cells and
hits -- tests/qlearn_cases.py -- against the numpy restatement tests/qlearn_ref.py and the oracle.  tests/test_qlearn_cpu.py holds the
oracle to the restatement and shows that these inputs reach their branches.
  A  the fold of crafted pending sums into the table, bit for bit, in the library's arrays and in caller memory;
  B  the derived rows (band sums, V) of a crafted table, through what one rendered batch pays and shows;
  C  cells and patches predicted exactly from the stream states: a floor under the sky, then tilted planes on the sector boundaries;
  D  rewards by hit kind: sky, light disk, diffuse, glass, metal;
  E  one set of bits under every schedule;  F  several internal batches in one call;  G  refusals.
Bars: integers equal; tables bit-equal; radiance within RADIANCE_TOL of the oracle (the project's bar), schedules bit-equal.
Measured on an MI355X (figures printed before they are asserted): A bit-exact at every grid and alpha; every sum and count equal; largest
radiance error 1.6e-7 in B, 2.9e-7 in C, 2.4e-7 in D, 1.5e-7 in E, 1.2e-7 in F.  The rt_trace_batch refusals of G on the commit before the
rule: RT_OK, all 96 values written (unguided radiance from the slot wavefront), no reward paid."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_cases as dc  # noqa: E402
import qlearn_cases as qc  # noqa: E402
import qlearn_ref as qr  # noqa: E402
import support as sp  # noqa: E402
from conftest import rel_err  # noqa: E402
from test_gpu_parity import RADIANCE_TOL  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
PATH = 1
PROBE_BOX, PROBE_GRID, PROBE_W, PROBE_H = ((-4, -1, -4), (4, 5, 6)), 3, 16, 8
FLOOR_MATS = {0: (qc.FLOOR_ALBEDO, qc.FLOOR_COL)}
OWN_ENVS = [{"RT_SHADE_LDS": "0"}, {"RT_PRIMARY_TABLE": "0"}, {"RT_BOUNCE_TABLE": "0"}, {"RT_TLAS_LDS": "0"}]


# ---- the two sides ----------------------------------------------------------------------------------------------------------------------
def _fill(scenes, name):
    if name == "probe":
        return lambda b: scenes.REGISTRY["qlearn_probe"](b)
    return lambda b: qc.SCENES[name](b, rt=True)


def _device(host_api, scenes, monkeypatch, name, env=None, w=8, h=8):
    return sp.renderer(host_api, monkeypatch, _fill(scenes, name), w, h, env=env)


_ORACLES = {}


def _oracle(oracle_api, scenes, name, w=8, h=8):
    key = (name, w, h)
    if key not in _ORACLES:
        o = oracle_api.OracleScene()
        _fill(scenes, name)(o)
        o.set_raytracer(False)
        _ORACLES[key] = (o, oracle_api.OracleRenderer(o, w, h))
    return _ORACLES[key]


def _load(r, grid, lo, hi, mask, table, alpha=1.0):
    """the crafted table into the device, by part A's route: its sums folded with alpha = 1; bit-equal to the restated one"""
    r.qlearn_enable(grid, lo, hi, alpha, qc.EPS, qc.Q_INIT, mask)
    if table is None:
        return np.full((grid ** 3, 64), f32(qc.Q_INIT))
    assert alpha == 1.0
    r.qlearn_set_sums(*qc.table_sums(table, grid ** 3))
    r.qlearn_apply()
    tab = qc.table(table, grid ** 3)
    assert sp.same(r.qlearn_table(), tab)
    return tab


_REFS = {}


def _oracle_rays(oracle_api, scenes, name, grid, lo, hi, mask, table, O, D, depth):
    """(values, sums, counts) of one batch of caller rays on the oracle, from empty sums (computed once per session)"""
    key = (name, grid, tuple(lo), tuple(hi), mask, table, depth, O.tobytes())
    if key not in _REFS:
        o, orr = _oracle(oracle_api, scenes, name)
        orr.qlearn_enable(grid, lo, hi, 1.0, qc.EPS, qc.Q_INIT, mask)
        if table is not None:
            orr.qlearn_set_table(qc.table(table, grid ** 3))
        rgb = orr.trace_rays(1, O, D, depth, (1, 1, 1), qc.SEED_BASE)
        s, c, _ = orr.qlearn_state()
        _REFS[key] = (rgb, s, c)
    return _REFS[key]


def _device_rays(r, O, D, depth):
    """(values, sums, counts) of one batch on the device, from empty sums"""
    n = r._qgrid ** 3
    r.qlearn_set_sums(np.zeros((n, 64), np.int64), np.zeros((n, 64), np.uint32))
    rgb = r.trace_batch(PATH, O, D, depth=depth, seed_base=qc.SEED_BASE)
    return (rgb,) + tuple(r.qlearn_sums())


def _radiance(got, ref, what):
    err, cls_ok = rel_err(got, ref)
    print("qlearn-err %s: max relative error %.3g, non-finite %d" % (what, err.max(), int((~np.isfinite(ref)).sum())))
    assert cls_ok and err.max() <= RADIANCE_TOL, (what, err.max())
    return float(err.max())


# ---- A: table arithmetic ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", qc.ALPHAS)
@pytest.mark.parametrize("grid", qc.APPLY_GRIDS)
def test_apply_of_crafted_sums(grid, alpha, host_api, scenes, monkeypatch):
    """rt_qlearn_set_sums(crafted) -> rt_qlearn_apply -> rt_qlearn_get_table / get_sums equals qlearn_ref.apply bit for bit: unpaid
    entries keep their sum and leave the table alone, a second apply changes nothing, and repeated towards 0 the floor holds.
    (125 cells: not a multiple of the 64-thread block; 262144: the restatement alone.)"""
    r = _device(host_api, scenes, monkeypatch, "floor")
    cells = grid ** 3
    r.qlearn_enable(grid, *qc.box(grid, "face"), alpha, qc.EPS, qc.Q_INIT, 0)
    tab = np.full((cells, 64), f32(qc.Q_INIT))
    assert sp.same(r.qlearn_table(), tab)
    sums, counts, at = qc.crafted_sums(cells)
    idx = np.arange(cells)
    reps = 40 if alpha == 0.3 and grid < 64 else 2
    for rep in range(reps):
        r.qlearn_set_sums(sums, counts)
        assert all(np.array_equal(a, b) for a, b in zip(r.qlearn_sums(), (sums, counts)))
        r.qlearn_apply()
        want, s2, c2 = qr.apply(tab, sums, counts, alpha)
        got, (gs, gc) = r.qlearn_table(), r.qlearn_sums()
        differ = int((sp.bits(got) != sp.bits(want)).sum())
        if rep == 0:
            print("qlearn-apply grid=%d alpha=%g: %d of %d table values differ by bits" % (grid, alpha, differ, want.size))
        assert differ == 0 and np.array_equal(gs, s2) and np.array_equal(gc, c2), (rep, differ)
        assert sp.same(got[idx, at["unpaid"]], tab[idx, at["unpaid"]]) and np.all(gs[idx, at["unpaid"]] == qc.ENTRIES["unpaid"][0])
        assert np.all(got[idx, at["negative"]] == qr.Q_MIN)
        r.qlearn_apply()
        assert sp.same(r.qlearn_table(), want) and np.array_equal(r.qlearn_sums()[0], s2)
        tab = want
    if alpha == 1.0 or reps == 40:
        assert np.all(tab[idx, at["zero"]] == qr.Q_MIN)
    if alpha == 1.0:
        assert np.all(tab[idx, at["full"]] == 64)
    r.close()


def test_apply_in_caller_memory(host_api, scenes, monkeypatch):
    """the same fold with the sums bound to caller memory (rt_qlearn_bind_sums): set, fold and read through the caller's arrays; after a
    re-enable with another grid the arrays bound before are no longer written"""
    import torch
    r = _device(host_api, scenes, monkeypatch, "floor")
    grid, cells = 5, 125
    r.qlearn_enable(grid, *qc.box(grid, "face"), 0.3, qc.EPS, qc.Q_INIT, 0)
    qs = torch.zeros(cells * 64, dtype=torch.int64, device="cuda")
    qn = torch.zeros(cells * 64, dtype=torch.int32, device="cuda")
    r.qlearn_bind_sums(qs.data_ptr(), qn.data_ptr())
    sums, counts, at = qc.crafted_sums(cells)
    r.qlearn_set_sums(sums, counts)
    torch.cuda.synchronize()
    assert np.array_equal(qs.cpu().numpy().reshape(cells, 64), sums) and np.array_equal(qn.cpu().numpy().view(np.uint32).reshape(cells, 64), counts)
    r.qlearn_apply()
    r.synchronize()
    want, s2, c2 = qr.apply(np.full((cells, 64), f32(qc.Q_INIT)), sums, counts, 0.3)
    assert sp.same(r.qlearn_table(), want)
    assert np.array_equal(qs.cpu().numpy().reshape(cells, 64), s2) and np.array_equal(qn.cpu().numpy().view(np.uint32).reshape(cells, 64), c2)
    # another grid: the library's own arrays again
    qs.fill_(-7), qn.fill_(7)
    torch.cuda.synchronize()
    r.qlearn_enable(2, *qc.box(2, "face"), 1.0, qc.EPS, qc.Q_INIT, 0)
    s8, c8, _ = qc.crafted_sums(8)
    r.qlearn_set_sums(s8, c8)
    r.qlearn_apply()
    O, D, _ = qc.rays_of(qc.floor_points(2, "face"))
    r.trace_batch(PATH, O, D, depth=1, seed_base=qc.SEED_BASE)
    assert r.qlearn_sums()[1].sum() > 0
    r.synchronize()
    torch.cuda.synchronize()
    assert bool((qs == -7).all()) and bool((qn == 7).all())
    r.close()


# ---- B: derived rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", qc.TABLES)
def test_derived_rows_follow_a_crafted_table(table, host_api, oracle_api, scenes, monkeypatch):
    """V and the band sums cannot be downloaded: the same crafted table on both sides, one rendered batch each -- the picks read the band
    sums, the rewards of diffuse hits the V rows, those of glass and metal the band sums again.  Sums and counts integer for integer,
    the frame within the radiance bar."""
    r = _device(host_api, scenes, monkeypatch, "probe", w=PROBE_W, h=PROBE_H)
    o, orr = _oracle(oracle_api, scenes, "probe", PROBE_W, PROBE_H)
    tab = _load(r, PROBE_GRID, *PROBE_BOX, 0, table)
    orr.qlearn_enable(PROBE_GRID, *PROBE_BOX, 1.0, qc.EPS, qc.Q_INIT, 0)
    orr.qlearn_set_table(tab)
    orr.clear(), r.clear()
    orr.render(0, 2, nthreads=0)
    r.render(PATH, 0, 2)
    so, co, _ = orr.qlearn_state()
    sg, cg = r.qlearn_sums()
    assert co.sum() >= 32 and np.array_equal(co, cg) and np.array_equal(so, sg)   # (most of the 256 samples see the sky first)
    _radiance(r.accumulator()[..., :3], orr.accumulator()[..., :3], "B table=%s" % table)
    r.close()


# ---- C: cells and patches -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["face", "lo"])
@pytest.mark.parametrize("grid", qc.GRIDS)
def test_cells_and_patches_on_the_floor(grid, kind, host_api, oracle_api, scenes, monkeypatch):
    """straight down onto a floor under the sky: counts per (cell, patch) are what qlearn_ref predicts from StreamSeed(SEED_BASE + i) --
    four draws a pick, no light draws -- and the sums, sky rewards, are the prediction's and the oracle's; only the dead samples pay at
    depth 0, every learner once at depth 1, nobody under learn_mask 0xFFFFFFFF; patches below the floor hold sums of exactly 0.
    (Grid 64: the oracle under mask 0 only -- its enable is a 64 x 64 product for each of 262144 cells.)"""
    lo, hi = qc.box(grid, kind)
    O, D, where = qc.rays_of(qc.floor_points(grid, kind))
    r = _device(host_api, scenes, monkeypatch, "floor")
    o, _ = _oracle(oracle_api, scenes, "floor")
    below = np.arange(64) % 8 >= 4
    for mask in qc.MASKS:
        tab = _load(r, grid, lo, hi, mask, "random")
        for depth in (0, 1):
            rgb, s, c = _device_rays(r, O, D, depth)
            ps, pc, first = qc.predict(tab, grid, lo, hi, mask, o, FLOOR_MATS, O, D, depth)
            assert np.array_equal(c, pc), (mask, depth, np.argwhere(c != pc)[:4])
            assert np.array_equal(s, ps), (mask, depth)
            L = first["learner"]
            assert c.sum() == ((L & first["dead"]).sum() if depth == 0 else L.sum())
            assert np.all(s[:, below] == 0) and (depth == 1 or np.all(s == 0))
            if mask == 0xFFFFFFFF:
                assert c.sum() == 0
            if grid < 64 or mask == 0:
                ref, so, co = _oracle_rays(oracle_api, scenes, "floor", grid, lo, hi, mask, "random", O, D, depth)
                assert np.array_equal(s, so) and np.array_equal(c, co), (mask, depth)
                _radiance(rgb, ref, "C floor grid=%d %s mask=%x depth=%d" % (grid, kind, mask, depth))
    r.close()


def test_cells_and_patches_under_tilted_planes(host_api, oracle_api, scenes, monkeypatch):
    """the guided children meet planes whose normals sit on the sector boundaries (|x| = |y|, x = 0, y = -0.0) and at both poles: sums and
    counts are the oracle's and the prediction's, whose reward is the V row at qlearn_ref.patch_of(normal)"""
    lo, hi = qc.TILT_BOX
    O, D, _ = qc.rays_of(qc.TILT_POINTS, qc.TILT_REPS)
    r = _device(host_api, scenes, monkeypatch, "tilt")
    o, _ = _oracle(oracle_api, scenes, "tilt")
    for mask in (0, 3):
        tab = _load(r, qc.TILT_GRID, lo, hi, mask, "random")
        for depth in (1, 2):
            rgb, s, c = _device_rays(r, O, D, depth)
            ref, so, co = _oracle_rays(oracle_api, scenes, "tilt", qc.TILT_GRID, lo, hi, mask, "random", O, D, depth)
            ps, pc, _ = qc.predict(tab, qc.TILT_GRID, lo, hi, mask, o, qc.TILT_MATS, O, D, depth)
            assert c.sum() > 0 and np.array_equal(c, co) and np.array_equal(s, so), (mask, depth)
            assert np.array_equal(c, pc) and np.array_equal(s, ps), (mask, depth)
            _radiance(rgb, ref, "C tilt mask=%x depth=%d" % (mask, depth))
    r.close()


# ---- D: rewards by hit kind -------------------------------------------------------------------------------------------------------------------
def test_rewards_by_hit_kind(host_api, oracle_api, scenes, monkeypatch):
    """guided children that meet the sky, an area light's disk (exactly 64: some (cell, patch) ends with sum == count << 22), a diffuse
    sphere (a V row), glass and metal (the mean of Q): sums and counts are the oracle's, the values within the radiance bar (a path
    into the disk is +inf on both sides)"""
    lo, hi = qc.KIND_BOX
    O, D, where = qc.kind_rays()
    r = _device(host_api, scenes, monkeypatch, "kinds")
    for mask in (0, 3):
        _load(r, qc.KIND_GRID, lo, hi, mask, "random")
        for depth in (1, 2):
            rgb, s, c = _device_rays(r, O, D, depth)
            ref, so, co = _oracle_rays(oracle_api, scenes, "kinds", qc.KIND_GRID, lo, hi, mask, "random", O, D, depth)
            assert c.sum() >= (len(O) if mask == 0 else 1) and np.array_equal(c, co) and np.array_equal(s, so), (mask, depth)
            if mask == 0:
                assert ((c > 0) & (s == c.astype(np.int64) << 22)).any()
            _radiance(rgb, ref, "D mask=%x depth=%d" % (mask, depth))
    r.close()


# ---- E: schedules -----------------------------------------------------------------------------------------------------------------------------
_FIRST = {}


def _schedule_run(host_api, scenes, monkeypatch, env):
    """what part E compares: the batches of C and D and one 16 x 8 frame, under one environment"""
    out = {}
    jobs = [("floor", 3, qc.box(3, "face"), 3, qc.rays_of(qc.floor_points(3, "face"))[:2], (0, 1)),
            ("tilt", qc.TILT_GRID, qc.TILT_BOX, 0, qc.rays_of(qc.TILT_POINTS, qc.TILT_REPS)[:2], (2,)),
            ("kinds", qc.KIND_GRID, qc.KIND_BOX, 0, qc.kind_rays()[:2], (1, 2))]
    for name, grid, (lo, hi), mask, (O, D), depths in jobs:
        r = _device(host_api, scenes, monkeypatch, name, env=env)
        _load(r, grid, lo, hi, mask, "random")
        for depth in depths:
            out[name, depth] = _device_rays(r, O, D, depth)
        r.close()
    r = _device(host_api, scenes, monkeypatch, "probe", env=env, w=PROBE_W, h=PROBE_H)
    _load(r, PROBE_GRID, *PROBE_BOX, 3, "random")
    r.clear()
    r.render(PATH, 0, 2)
    out["probe", 4] = (r.accumulator(),) + tuple(r.qlearn_sums())
    r.close()
    return out


@pytest.mark.parametrize("env", dc.PATH_ENVS + OWN_ENVS, ids=sp.env_id)
def test_one_set_of_bits_under_every_schedule(env, host_api, oracle_api, scenes, monkeypatch):
    """the fuse modes, the producer-side decisions off, RT_STREAM=0 (with the sampler on still the dense wavefront), the tables of the
    shade step from memory, no primary-hit table, no bounce table, the TLAS from memory: the values, the accumulator, the sums and the
    counts have the bits of the default schedule, whose frame is within the radiance bar of the oracle's"""
    got = _schedule_run(host_api, scenes, monkeypatch, env)
    first = _FIRST.setdefault("run", got)
    for key in got:
        v, s, c = got[key]
        fv, fs, fc = first[key]
        assert c.sum() > 0 and np.array_equal(s, fs) and np.array_equal(c, fc), key
        assert sp.same(v, fv), key
    if got is first:
        o, orr = _oracle(oracle_api, scenes, "probe", PROBE_W, PROBE_H)
        orr.qlearn_enable(PROBE_GRID, *PROBE_BOX, 1.0, qc.EPS, qc.Q_INIT, 3)
        orr.qlearn_set_table(qc.table("random", PROBE_GRID ** 3))
        orr.clear()
        orr.render(0, 2, nthreads=0)
        so, co, _ = orr.qlearn_state()
        v, s, c = got["probe", 4]
        assert np.array_equal(s, so) and np.array_equal(c, co)
        _radiance(v[..., :3], orr.accumulator()[..., :3], "E probe frame")


# ---- F: several internal batches ------------------------------------------------------------------------------------------------------------
def test_internal_batches_of_one_call(host_api, oracle_api, scenes, monkeypatch):
    """an 8 x 4 frame under RT_SLOTS=64: five frames in one call are three internal batches (2, 2, 1 frames), each folding its reward
    words into the sums; the same frames one call per batch, and the oracle, give the same sums and the same frame"""
    w, h, frames = 8, 4, 5
    r = _device(host_api, scenes, monkeypatch, "probe", env={"RT_SLOTS": "64"}, w=w, h=h)
    _load(r, PROBE_GRID, *PROBE_BOX, 0, "random")
    r.clear()
    r.render(PATH, 0, frames)
    one, (s1, c1) = r.accumulator(), r.qlearn_sums()
    n = PROBE_GRID ** 3
    r.qlearn_set_sums(np.zeros((n, 64), np.int64), np.zeros((n, 64), np.uint32))
    r.clear()
    for f0, nf in ((0, 2), (2, 2), (4, 1)):
        r.render(PATH, f0, nf)
    many, (s3, c3) = r.accumulator(), r.qlearn_sums()
    assert c1.sum() >= 16 and np.array_equal(s1, s3) and np.array_equal(c1, c3) and sp.same(one, many)
    o, orr = _oracle(oracle_api, scenes, "probe", w, h)
    orr.qlearn_enable(PROBE_GRID, *PROBE_BOX, 1.0, qc.EPS, qc.Q_INIT, 0)
    orr.qlearn_set_table(qc.table("random", n))
    orr.clear()
    orr.render(0, frames, nthreads=0)
    so, co, _ = orr.qlearn_state()
    assert np.array_equal(s1, so) and np.array_equal(c1, co)
    _radiance(one[..., :3], orr.accumulator()[..., :3], "F five frames")
    r.close()


# ---- G: refusals ------------------------------------------------------------------------------------------------------------------------------
def _raw_trace(r, host_api, O, D, depth, out):
    return r.rt.rt_trace_batch_energy(r.ctx, PATH, len(O), O.ctypes.data_as(C.c_void_p), D.ctypes.data_as(C.c_void_p), depth, qc.SEED_BASE,
                                      (C.c_float * 3)(1, 1, 1), out.ctypes.data_as(C.c_void_p))


@pytest.mark.parametrize("how", ["slots", "count_reference"])
def test_trace_batch_refuses_what_it_cannot_guide(how, host_api, scenes, monkeypatch):
    """rt_trace_batch in path mode with the sampler on and a batch that is not stream-eligible -- 32 rays under RT_SLOTS=24, or
    RT_COUNT_REFERENCE -- returns RT_E_UNSUPPORTED in rt_render's words; rgb_out, the pending sums and the accumulator stay as they were.
    (Before this rule the call fell through to the slot wavefront: unguided radiance, RT_OK, no rewards.)"""
    r = _device(host_api, scenes, monkeypatch, "floor", env={"RT_SLOTS": "24"} if how == "slots" else None)
    lo, hi = qc.box(3, "face")
    _load(r, 3, lo, hi, 0, "random")
    O, D, _ = qc.rays_of(qc.floor_points(3, "face"))
    O, D = np.ascontiguousarray(O[:32]), np.ascontiguousarray(D[:32])
    fit = 24 if how == "slots" else 32
    r.clear()
    r.trace_batch(PATH, O[:fit], D[:fit], depth=1, seed_base=qc.SEED_BASE)   # a batch that fits pays
    s0, c0 = r.qlearn_sums()
    acc0 = r.accumulator()
    assert c0.sum() == fit
    if how == "count_reference":
        r.set_counting(host_api.RT_COUNT_REFERENCE)
    out = np.full((32, 3), f32(-7.0))
    rc = _raw_trace(r, host_api, O, D, 1, out)
    msg = r.rt.rt_last_error(r.ctx).decode()
    print("rt_trace_batch [%s]: rc %d, %s; %d values written" % (how, rc, msg, int((out != -7.0).sum())))
    assert rc == host_api.RT_E_UNSUPPORTED and "the Q-learning sampler needs a path batch with an entry per sample" in msg
    assert np.all(out == -7.0)
    s1, c1 = r.qlearn_sums()
    assert np.array_equal(s0, s1) and np.array_equal(c0, c1) and sp.same(acc0, r.accumulator())
    r.set_counting(0)
    with pytest.raises(RuntimeError, match="entry per sample"):   # rt_render over the budget / under the reference's tallies
        if how == "slots":
            r.render(PATH, 0, 1)   # 64 pixels, 24 slots
        else:
            r.set_counting(host_api.RT_COUNT_REFERENCE)
            r.render(PATH, 0, 1)
    r.set_counting(0)
    r.qlearn_disable()   # off: the slot wavefront's batch like any other
    assert _raw_trace(r, host_api, O, D, 1, out) == 0 and np.all(out != -7.0)
    r.close()


BAD = {"grid 0": dict(grid=0), "grid 65": dict(grid=65), "empty box": dict(hi=(4, -1, 4)), "NaN box": dict(lo=(np.nan, -1, -4)),
       "inf box": dict(hi=(np.inf, 5, 4)), "-inf box": dict(lo=(-np.inf, -1, -4)), "alpha 0": dict(alpha=0.0), "alpha > 1": dict(alpha=1.5),
       "alpha NaN": dict(alpha=np.nan), "eps < 0": dict(epsilon=-0.1), "eps > 1": dict(epsilon=1.1), "q_init 0": dict(q_init=0.0),
       "q_init inf": dict(q_init=np.inf), "q_init NaN": dict(q_init=np.nan)}


def test_enable_refuses_bad_parameters(host_api, scenes, monkeypatch):
    """every refusal is RT_E_ARG, and leaves the sampler OFF whatever it was (include/rt_amd.h: the previous table is freed before the
    arguments are looked at): rt_qlearn_get_table fails, and a plain frame has the bits it had before the sampler was ever on -- as after
    rt_qlearn_enable(NULL)"""
    r = _device(host_api, scenes, monkeypatch, "probe", w=PROBE_W, h=PROBE_H)
    r.clear()
    r.render(PATH, 0, 2)
    plain = r.accumulator()
    good = dict(grid=3, lo=(-4, -1, -4), hi=(4, 5, 4), alpha=0.3, epsilon=0.2, q_init=1.0)
    for what, bad in BAD.items():
        r.qlearn_enable(**good)
        r.clear()
        r.render(PATH, 0, 2)
        assert not sp.same(r.accumulator(), plain)   # guided: other bits
        with pytest.raises(RuntimeError, match="rt_amd error %d: rt_qlearn_enable" % host_api.RT_E_ARG):
            r.qlearn_enable(**dict(good, **bad))
        with pytest.raises(RuntimeError, match="the sampler is off"):
            r.qlearn_table()
        r.clear()
        r.render(PATH, 0, 2)
        assert sp.same(r.accumulator(), plain), what
    r.qlearn_enable(**good)
    r.qlearn_disable()
    r.clear()
    r.render(PATH, 0, 2)
    assert sp.same(r.accumulator(), plain)
    r.close()
