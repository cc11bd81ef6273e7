"""The Q-learning guided sampler without a device: the oracle's statement (oracle/orc_qlearn.h) against the numpy restatement
tests/qlearn_ref.py, bit for bit, on the crafted inputs of tests/qlearn_cases.py; the round trip patch_of(direction(.)) with its two
documented edges; and, on the oracle alone, that the inputs of tests/test_gpu_qlearn.py reach every cell and branch they are listed for
and that each case's twin pays other rewards."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qlearn_cases as qc  # noqa: E402
import qlearn_ref as qr  # noqa: E402
import support as sp  # noqa: E402

f32 = np.float32
US = np.array([2.0 ** -20] + [k / 16 for k in range(1, 16)] + [1 - 2.0 ** -20], f32)


def _pair(oracle_api, scene, twin=None, cache={}):
    key = (scene, twin)
    if key not in cache:
        o = oracle_api.OracleScene()
        qc.SCENES[scene](o, rt=True, twin=twin)
        o.set_raytracer(False)
        cache[key] = (o, oracle_api.OracleRenderer(o, 8, 8))
    return cache[key]


def _oracle_batch(oracle_api, scene, grid, lo, hi, mask, tab, O, D, depth, twin=None):
    o, orr = _pair(oracle_api, scene, twin)
    orr.qlearn_enable(grid, lo, hi, 1.0, qc.EPS, qc.Q_INIT, mask)
    if tab is not None:
        orr.qlearn_set_table(tab)
    rgb = orr.trace_rays(1, O, D, depth, (1, 1, 1), qc.SEED_BASE)
    s, c, _ = orr.qlearn_state()
    return rgb, s, c


def test_round_trip_and_its_edges(oracle_api):
    """patch_of(direction(i, j, u1, u2)) == 8 i + j inside every patch, and on the sector's first edge u2 = 0; not at the pole (u1 = 0 in
    band 0: s = 0, sector 0) and not for u within 2^-23 of 1, where i + u rounds up to the next band or sector"""
    i, j, u1, u2 = np.meshgrid(np.arange(8), np.arange(8), US, np.concatenate([US, [f32(0)]]).astype(f32), indexing="ij")
    d = qr.direction(i, j, u1, u2).reshape(-1, 3)
    assert sp.same(d, oracle_api.qlearn_direction(i, j, u1, u2))
    assert np.array_equal(qr.patch_of(d), (8 * i + j).ravel())
    assert np.array_equal(oracle_api.qlearn_patch_of(d), (8 * i + j).ravel())
    # the documented edges
    assert np.array_equal(qr.patch_of(qr.direction(0, np.arange(8), f32(0), f32(0.5))), np.zeros(8, int))   # the pole
    near1 = f32(1 - 2.0 ** -24)
    assert np.array_equal(qr.patch_of(qr.direction(np.arange(7), 3, near1, f32(0.5))), 8 * (np.arange(7) + 1) + 3)   # the next band
    assert qr.patch_of(qr.direction(7, 3, near1, f32(0.5)))[0] == 56   # ... and above the last one the upper pole: z = 1
    # the next sector, around -- but sector 0 keeps such a draw: 0 + u is u
    assert np.array_equal(qr.patch_of(qr.direction(3, np.arange(8), f32(0.5), near1)), 24 + np.array([0, 2, 3, 4, 5, 6, 7, 0]))
    for fn in (oracle_api.qlearn_patch_of,):
        assert np.array_equal(fn(qr.direction(np.arange(7), 3, near1, f32(0.5))), 8 * (np.arange(7) + 1) + 3)
    assert np.array_equal(qr.patch_of([n for n, _, _ in qc.TILT_PLANES]), [p for _, _, p in qc.TILT_PLANES])
    assert np.array_equal(oracle_api.qlearn_patch_of([n for n, _, _ in qc.TILT_PLANES]), [p for _, _, p in qc.TILT_PLANES])


def test_patch_of_on_the_boundaries(oracle_api):
    rng = np.random.default_rng(5)
    n = rng.normal(size=(4000, 3)).astype(f32)
    n[:100, 0] = 0
    n[100:200, 1] = -0.0
    n[200:300, 1] = 0.0
    n[300:400, 1] = n[300:400, 0]
    n[400:500, 1] = -n[400:500, 0]
    n[500:520, :2] = 0
    n[520:530] = np.nan
    n[530:540, 2] = (-1.0, 1.0, -2.0, 2.0, -0.75, 0.75, 0.0, -0.0, np.inf, -np.inf)
    assert np.array_equal(qr.patch_of(n), oracle_api.qlearn_patch_of(n))
    assert set(qr.patch_of(n)) == set(range(64))


@pytest.mark.parametrize("kind", ["face", "lo"])
@pytest.mark.parametrize("grid", qc.GRIDS)
def test_cells_of_the_crafted_points(grid, kind, oracle_api):
    """every point of floor_points lands in the cell written down for it, by the restatement and by the oracle"""
    lo, hi = qc.box(grid, kind)
    o, orr = _pair(oracle_api, "floor")
    if grid < 64:   # (the oracle's enable is a 64 x 64 product per cell: 262144 of them are the GPU file's to pay, once)
        orr.qlearn_enable(grid, lo, hi, 1.0, qc.EPS, qc.Q_INIT, 0)
    iy = qc.expected_cell_y(grid, kind)
    for name, (x, z) in qc.floor_points(grid, kind).items():
        ix, iz = qc.expected_cell_xz(grid, kind, name)
        want = (iz * grid + iy) * grid + ix
        assert qr.cell(grid, lo, hi, [[x, 0.0, z]])[0] == want, name
        if grid < 64:
            assert orr.qlearn_cell([[x, 0.0, z]])[0] == want, name
    rng = np.random.default_rng(grid)
    x = (rng.uniform(-1, 2, (2000, 3)) * (hi - lo) + lo).astype(f32)
    x[:8] = np.array([np.nan, np.inf, -np.inf, 0, -0.0, 1e38, -1e38, 1e-45], f32)[:, None]
    if grid < 64:
        assert np.array_equal(qr.cell(grid, lo, hi, x), orr.qlearn_cell(x))


@pytest.mark.parametrize("alpha", qc.ALPHAS)
@pytest.mark.parametrize("grid", [1, 2, 5])
def test_apply_and_derive(grid, alpha, oracle_api):
    """the fold of the crafted sums, twice, then five more times towards the floor; the V rows and centres after it"""
    o, orr = _pair(oracle_api, "floor")
    lo, hi = qc.box(grid, "face")
    orr.qlearn_enable(grid, lo, hi, alpha, qc.EPS, qc.Q_INIT, 0)
    tab = qc.table("random", grid ** 3)
    orr.qlearn_set_table(tab)
    sums, counts, at = qc.crafted_sums(grid ** 3)
    for rep in range(7):
        orr.qlearn_set_sums(sums, counts)
        orr.qlearn_apply()
        tab2, s2, c2 = qr.apply(tab, sums, counts, alpha)
        so, co, to = orr.qlearn_state()
        assert sp.same(to, tab2) and np.array_equal(so, s2) and np.array_equal(co, c2), rep
        cells = np.arange(grid ** 3)
        assert sp.same(tab2[cells, at["unpaid"]], tab[cells, at["unpaid"]]) and np.all(s2[cells, at["unpaid"]] == 12345)
        assert np.all(tab2[cells, at["negative"]] == qr.Q_MIN)
        orr.qlearn_apply()   # nothing pending but the unpaid sums: nothing changes
        assert sp.same(orr.qlearn_state()[2], tab2)
        tab = tab2
    if alpha == 1.0:
        assert np.all(tab[cells, at["zero"]] == qr.Q_MIN) and np.all(tab[cells, at["full"]] == 64)
    v, c = orr.qlearn_v()
    assert sp.same(v, qr.derive(tab)[1]) and sp.same(c, qr.centres()) and sp.same(orr.qlearn_weights(), qr.weights())


def test_reward_rounding(oracle_api):
    rng = np.random.default_rng(2)
    ties = (np.arange(1, 64, dtype=np.float64) + 0.5) / 65536
    R = np.concatenate([rng.uniform(-1, 70, 2000), ties, [np.nan, np.inf, -np.inf, 64, 63.999996, 0.0, -0.0, 1e-9]]).astype(f32)
    got = qr.reward_fixed(R)
    assert np.array_equal(got, oracle_api.qlearn_reward_fixed(R))
    assert np.array_equal(qr.reward_fixed(ties.astype(f32)) % 2, np.zeros(63, int))   # ties to even
    assert got.min() == 0 and got.max() == 64 << 16


def _state_before(s, steps):
    """the xorshift32 state 'steps' draws before s"""
    def unshift(x, k, left):
        y, sh = x, k
        while sh < 32:
            y = x ^ ((y << k) & 0xFFFFFFFF if left else y >> k)
            sh += k
        return y
    for _ in range(steps):
        s = unshift(unshift(unshift(s, 5, True), 17, False), 13, True)
    return s


@pytest.mark.parametrize("name", qc.TABLES)
def test_sample_against_the_restatement(name, oracle_api):
    """one pick per (cell, state): patch, P, direction and the state after it, bit for bit, on every crafted table, with eps 0, 0.2 and 1;
    among the states some whose pick draw is 1.0 (the last cumulative sum does not take it either) and some whose mixture draw is it"""
    grid = 3
    o, orr = _pair(oracle_api, "floor")
    tab = qc.table(name, grid ** 3)
    rng = np.random.default_rng(11)
    states = rng.integers(1, 1 << 32, 6000, dtype=np.uint64).astype(np.uint32)
    for k in range(64):
        states[k] = _state_before(0xFFFFFFFF - k, 2)       # the second draw rounds to 1.0
        states[64 + k] = _state_before(0xFFFFFFFF - k, 1)  # the first
    assert np.all(qr.random_float(qr.random_float(states[:64])[0])[1] == 1.0)
    cells = rng.integers(0, grid ** 3, len(states))
    for eps in (0.0, qc.EPS, 1.0):
        orr.qlearn_enable(grid, *qc.box(grid, "face"), 1.0, eps, qc.Q_INIT, 0)
        orr.qlearn_set_table(tab)
        p, P, d, after = orr.qlearn_sample(cells, states)
        r = qr.sample(tab[cells], eps, states)
        assert np.array_equal(p, r["patch"]) and sp.same(P, r["P"]) and sp.same(d, r["dir"]) and np.array_equal(after, r["state"]), eps
        if eps == 0.0:
            assert r["past_end"][:64].all() and np.all(r["patch"][:64] % 8 == 7) and (r["branch"] == "cdf").all()
        if eps == 1.0:
            assert np.all(r["patch"][:64] == 63)   # 1.0 * 64 is held at the last patch
    if name == "peak":   # (1 - eps) of the picks go to the one patch that is not on the floor
        r = qr.sample(tab[cells], 0.0, states)
        assert (r["patch"] == (cells * 11 + 37) % 64)[128:].mean() > 0.99


# ---- non-vacuity of the GPU tier's inputs, on the oracle alone --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["face", "lo"])
@pytest.mark.parametrize("grid", [1, 3])
def test_floor_cases_reach_their_branches(grid, kind, oracle_api):
    """part C: the oracle's sums and counts are the prediction's at depths 0 and 1 under every mask; every crafted point pays into the
    cell written down for it; the picks show the epsilon pick, the pick by the table with both fall-throughs, and the dead sample; only
    the dead pay at depth 0 and every learner pays once at depth 1; the twin (another floor colour changes nothing a sky reward sees, so:
    another depth) differs"""
    lo, hi = qc.box(grid, kind)
    O, D, where = qc.rays_of(qc.floor_points(grid, kind))
    o, orr = _pair(oracle_api, "floor")
    tab = qc.table("random", grid ** 3)
    seen = {}
    for mask in qc.MASKS:
        for depth in (0, 1):
            _, s, c = _oracle_batch(oracle_api, "floor", grid, lo, hi, mask, tab, O, D, depth)
            ps, pc, first = qc.predict(tab, grid, lo, hi, mask, o, {0: (qc.FLOOR_ALBEDO, qc.FLOOR_COL)}, O, D, depth)
            assert np.array_equal(s, ps) and np.array_equal(c, pc), (mask, depth)
            seen[mask, depth] = (s, c)
            L = first["learner"]
            assert c.sum() == (L & first["dead"]).sum() if depth == 0 else c.sum() == L.sum()
            below = np.arange(64) % 8 >= 4   # phi in [pi, 2 pi): y <= 0, below the floor
            assert np.all(s[:, below] == 0)
            if depth == 0:
                assert np.all(s == 0)
    s0, c0 = seen[0, 1]
    assert seen[0xFFFFFFFF, 1][1].sum() == 0 and 0 < seen[3, 1][1].sum() < c0.sum() and s0.sum() > 0
    assert not np.array_equal(seen[0, 0][1], c0)
    _, _, first = qc.predict(tab, grid, lo, hi, 0, o, {0: (qc.FLOOR_ALBEDO, qc.FLOOR_COL)}, O, D, 1)
    iy = qc.expected_cell_y(grid, kind)
    for name, at in where.items():
        ix, iz = qc.expected_cell_xz(grid, kind, name)
        assert np.all(first["cell"][at] == (iz * grid + iy) * grid + ix), name
    assert {"eps", "cdf"} == set(first["branch"]) and first["last_band"].any() and first["last_sector"].any()
    assert first["dead"].any() and not first["dead"].all()


def test_tilt_cases_reach_every_normal(oracle_api):
    """part C, the tilted planes: the oracle's sums are the prediction's, whose reward patch is qlearn_ref.patch_of(normal); every
    plane is met by a learner's child; with the normals nudged off their boundaries the sums differ"""
    lo, hi = qc.TILT_BOX
    O, D, where = qc.rays_of(qc.TILT_POINTS, qc.TILT_REPS)
    o, orr = _pair(oracle_api, "tilt")
    tab = qc.table("random", qc.TILT_GRID ** 3)
    _, s, c = _oracle_batch(oracle_api, "tilt", qc.TILT_GRID, lo, hi, 0, tab, O, D, 1)
    ps, pc, first = qc.predict(tab, qc.TILT_GRID, lo, hi, 0, o, qc.TILT_MATS, O, D, 1)
    assert np.array_equal(s, ps) and np.array_equal(c, pc)
    up = ~first["dead"]
    hit = o.find_nearest(O[up], first["dir"][up], t_min=0.001)
    assert set(range(1, 1 + len(qc.TILT_PLANES))) <= set(hit["obj"].tolist()), sorted(set(hit["obj"].tolist()))
    _, st, ct = _oracle_batch(oracle_api, "tilt", qc.TILT_GRID, lo, hi, 0, tab, O, D, 1, twin="nudge")
    assert not np.array_equal(s, st)


def test_kind_cases_reach_every_hit_kind(oracle_api):
    """part D: the guided children of each stretch of floor meet what stands above it; a light's disk pays exactly 64; with everything
    lifted away the sums differ in every stretch's cells"""
    lo, hi = qc.KIND_BOX
    O, D, where = qc.kind_rays()
    o, orr = _pair(oracle_api, "kinds")
    tab = qc.table("random", qc.KIND_GRID ** 3)
    _, s, c = _oracle_batch(oracle_api, "kinds", qc.KIND_GRID, lo, hi, 0, tab, O, D, 1)
    _, st, ct = _oracle_batch(oracle_api, "kinds", qc.KIND_GRID, lo, hi, 0, tab, O, D, 1, twin="away")
    full = (c > 0) & (s == c.astype(np.int64) << 22)
    assert full.any() and not ((ct > 0) & (st == ct.astype(np.int64) << 22)).any()
    orr.qlearn_enable(qc.KIND_GRID, lo, hi, 1.0, qc.EPS, qc.Q_INIT, 0)
    for name, at in where.items():
        cell = orr.qlearn_cell(O[at] * f32([1, 0, 1]))[0]
        assert c[cell].sum() >= len(O[at]) // 2, name
        if name != "sky":
            assert not np.array_equal(s[cell], st[cell]), name
