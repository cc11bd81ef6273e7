"""Conditions on the inputs of tests/test_gpu_spill.py, on the oracle and the host-only layout builder alone: every ray group of
tests/spill_cases.py reaches exactly the stack depth it is named for (OracleScene.stack_peaks: a tally beside the oracle's walks), the
row counts of the instance chains are the ones the cases are built around, a deep set holds both rays that end in a hit and rays that pop
the whole stack and miss, and the render chain has lit, dark and directly lit rays.  Every figure is printed before it is asserted.
Also here: the rays of tests/test_gpu_parity.py::test_deep_tree_uses_the_spill_stack as they were (no push at all) and as they are."""
import numpy as np
import pytest

import spill_cases as sp

F32 = np.float32


def _scene(name, oracle_api, host_api):
    o = oracle_api.OracleScene()
    sp.fill(name, o, host_api)
    return o


def _peaks_by_group(o, R, any_hit, scope=0, index=0):
    pk = o.stack_peaks(R["O"], R["D"], any_hit=any_hit, scope=scope, index=index)
    return {k: {w: np.unique(pk[w][R["group"] == i]).tolist() for w in ("blas", "tlas", "stacked")} for i, k in enumerate(R["names"])}


def _check_set(name, o, R, expect, rows, what):
    for any_hit in (False, True):
        got = _peaks_by_group(o, R, any_hit)
        for k, v in got.items():
            print("%-12s %-8s %-8s %-8s stacked %s  blas %s  tlas %s  (rows %d)" % (name, what, "any-hit" if any_hit else "nearest", k, v["stacked"], v["blas"], v["tlas"], rows))
        for k, v in got.items():
            assert v["stacked"] == (list(expect[k]) if isinstance(expect[k], tuple) else [expect[k]]), (name, k, any_hit, v)
    deep = R["group"] == R["names"].index("deep")
    near = o.find_nearest(R["O"], R["D"])
    hit = near["obj"] != -1
    occ = o.is_occluded(R["O"], R["D"])["occluded"].astype(bool)
    print("%-12s %-8s deep rays: hit %.3f, miss %.3f; whole set occluded %.3f" % (name, what, hit[deep].mean(), 1 - hit[deep].mean(), occ.mean()))
    assert hit[deep].mean() >= 0.2 and (~hit[deep]).mean() >= 0.2
    assert 0.1 <= occ.mean() <= 0.9
    assert np.isfinite(near["t"][hit]).all()


@pytest.mark.parametrize("name", list(sp.CASES))
def test_every_group_peaks_where_it_is_named_for(name, oracle_api, host_api):
    """scene level, nearest-hit and any-hit: the peak of every ray of a group is the group's; a deep set mixes hits and misses"""
    rows, lds = sp.rows_of(name, host_api)
    expect = sp.expected_peaks(name, host_api)
    o = _scene(name, oracle_api, host_api)
    R = sp.rays(name)
    assert len(R["O"]) % 64 != 0
    _check_set(name, o, R, expect, rows, "scene")
    # what the deep rays are for: on both sides of the scene's rows, and of the general kernels' 16 where the chain is named for it
    assert expect["deep"] > rows or name in ("chain_p13", "chain_p14")
    if sp.CASES[name]["kind"] == "tlas":
        # BLAS scope, in the deep mesh's own space: the same rays peak at the mesh's depth
        got = _peaks_by_group(o, R, False, scope=2, index=0)
        print("%-12s BLAS 0 scope: deep %s" % (name, got["deep"]["blas"]))
        assert got["deep"]["blas"] == [sp.CASES[name]["n"] - 1]
        assert expect["over"] == rows + 1 and expect["edge"] == rows and expect["under"] == rows - 1
        tl = o.tlas_dump().view(F32)[:, [0, 1, 2, 4, 5, 6]]
        assert np.isfinite(tl).all() and np.abs(tl).max() < 1e30
    o.close()


def test_the_chains_sit_on_both_sides_of_the_rows(host_api):
    """13 and 14 stay in the LDS rows, 15 is the first spill entry, 17 is past the general kernels' 16 rows, 23 and 61 are deep"""
    peaks = [sp.expected_peaks(k, host_api)["deep"] for k in sp.CHAINS]
    assert peaks == [13, 14, 15, 17, 23, 61, 23]
    for k in sp.CHAINS:
        rows, lds = sp.rows_of(k, host_api)
        assert lds == 0
        assert [p - rows for p in peaks[:3]] == [-1, 0, 1]           # the last LDS row and the first spill entry of trace_persistent
    assert peaks[2] < sp.GENERAL_ROWS < peaks[3]                      # ... and of the general kernels


def test_instance_chains_cover_the_row_counts(host_api):
    """from rt_layout_build: the largest row count a TLAS copy leaves, one in the middle, RT_STACK_ROWS_MIN at the largest instance count
    that still has a copy, and one count above it, whose TLAS stays in global memory"""
    from instances_ref import ROWS_MIN, smallest_n_without_lds
    rows = {k: sp.rows_of(k, host_api) for k in sp.TLAS}
    for k, v in rows.items():
        print("%-12s m %2d  rows %2d  tlasLds %d" % (k, sp.CASES[k]["m"], v[0], v[1]))
    # the row counts of every instance count that has a copy, from the builder itself (a two-triangle probe scene per count)
    every = {}
    for m in range(2, smallest_n_without_lds() + 1):
        h = host_api.HostScene()
        mesh = h.mesh_raw(1, h.diffuse(0.8, (1, 1, 1)), sp.chain_tris(2))
        h.build_tlas(sp.SPLIT, [(mesh, sp.translation(16.0 * 2.0 ** i)) for i in range(m)])
        L = host_api.layout(h.describe())
        h.close()
        every[m] = (L["stackRows"], L["tlasLds"])
    with_copy = [m for m, v in every.items() if v[1]]
    assert max(with_copy) == smallest_n_without_lds() - 1 == sp.CASES["tlas_last"]["m"] and every[max(with_copy) + 1][1] == 0
    assert rows["tlas_first"] == (max(every[m][0] for m in with_copy), 1)
    assert rows["tlas_last"] == (ROWS_MIN, 1) == (min(every[m][0] for m in with_copy), 1)
    assert rows["tlas_first"][0] > rows["tlas_mid"][0] > rows["tlas_last"][0] and rows["tlas_mid"][1] == 1
    assert rows["tlas_global"][1] == 0 and sp.CASES["tlas_global"]["m"] > max(with_copy)
    for k in sp.TLAS:
        assert rows[k] == every[sp.CASES[k]["m"]] if sp.CASES[k]["m"] in every else rows[k][1] == 0


def test_the_deepest_case(oracle_api, host_api):
    """one case stacks 100 entries or more, below RT_STACK_MAX, deeper than either of the reference's own stacks"""
    deep = sp.expected_peaks(sp.DEEPEST, host_api)["deep"]
    print("deepest stacked peak: %d (%s)" % (deep, sp.DEEPEST))
    assert 100 <= deep < sp.STACK_MAX and deep > 64


def test_large_set(oracle_api, host_api):
    R = sp.large_rays()
    n = len(R["O"])
    assert n > sp.GRID_LANES and n % 64 != 0 and (n - sp.GRID_LANES) % 256 != 0
    o = _scene(sp.LARGE_SCENE, oracle_api, host_api)
    _check_set("large", o, R, sp.expected_peaks(sp.LARGE_SCENE, host_api), sp.rows_of(sp.LARGE_SCENE, host_api)[0], "scene")
    assert (R["group"] == R["names"].index("deep")).mean() >= 0.5
    o.close()


@pytest.mark.parametrize("mode,flag", [(0, True), (1, False), (0, False), (1, True)], ids=["Trace", "Sample", "Trace-flag_clear", "Sample-flag_set"])
def test_render_chain(mode, flag, oracle_api):
    """both functions at depths 1 and 4: the walks peak at 23; lit and dark rays are each a fifth of the finite ones at least, the rays
    that see the light directly a quarter at most and the only non-finite ones"""
    o = oracle_api.OracleScene()
    sp.render_chain(o)
    o.set_raytracer(flag)
    orr = oracle_api.OracleRenderer(o, 8, 8)
    O, D = sp.render_rays()
    direct = o.find_nearest(O, D)["obj"] == 11
    for depth in sp.RENDER_DEPTHS:
        rgb, pk = orr.trace_rays_peaks(mode, O, D, depth, sp.ENERGY, seed_base=sp.SEED_BASE)
        fin = np.isfinite(rgb).all(1)
        v = rgb[fin].max(1)
        lit, dark = (v > 0.05).mean(), (v == 0).mean()
        print("render chain mode %d flag %d depth %d: peak %d, non-finite %.3f, lit %.3f, dark %.3f, median lit value %.3g, largest %.3g"
              % (mode, flag, depth, pk["stacked"].max(), (~fin).mean(), lit, dark, np.median(v[v > 0.05]), v.max()))
        assert pk["stacked"].max() == sp.RENDER_PEAK == pk["blas"].max() and (pk["stacked"] == sp.RENDER_PEAK).mean() > 0.7
        assert lit >= 0.2 and dark >= 0.2
        assert np.array_equal(~fin, direct) and (~fin).mean() <= 0.25 and np.isposinf(rgb[~fin]).all()
        assert 0.1 < np.median(v[v > 0.05]) < 10      # O(1)
    orr.close()
    o.close()


def test_overflow_chain_is_past_the_limit_and_fits_f32():
    """the 136-triangle chain by its construction alone (it is never handed to the oracle's walk): finite, below 1e30, extents below the
    smallest x so that x stays every node's longest axis, one triangle more per level than RT_STACK_MAX + 1"""
    t = sp.chain_tris(sp.OVERFLOW_N, sp.OVERFLOW_X0, sp.OVERFLOW_W)
    assert np.isfinite(t).all() and np.abs(t).max() < 1e30 and t[:, 0].min() > sp.OVERFLOW_W and np.all(np.diff(t[:, 0]) > 0)
    assert sp.OVERFLOW_N - 1 > sp.STACK_MAX
    O, D = sp.overflow_rays()
    assert (O[:, 0] < t[:, 0].min()).all() and (D[:, 0] == 1).all() and (D[:, 1:] == 0).all()
    assert ((O[:, 1:] > 0) & (O[:, 1:] < sp.OVERFLOW_W)).all()

    class Walks:
        stack_peaks = None
    with pytest.raises(AssertionError):
        sp.overflow_chain(Walks())


def test_the_old_deep_tree_rays_never_push(oracle_api):
    """The reason for tests/spill_cases.py: the 4,000 rays test_deep_tree_uses_the_spill_stack had alone until now run along z through
    triangles that are flat in z, and the two children of every node are disjoint in x: at most one child is hit, nothing is pushed.
    The +x rays it has gained, on the 24-triangle chain, peak above RT_STACK_ROWS_MAX."""
    import test_gpu_parity as tp
    o = oracle_api.OracleScene()
    tp.deep_tree_fill(o)
    O, D = tp.deep_tree_rays_along_z()
    assert o.bvh_dump(-1)["max_depth"] > 20
    for any_hit in (False, True):
        pk = o.stack_peaks(O, D, any_hit=any_hit)
        print("old deep-tree rays, %s: peak %d" % ("any-hit" if any_hit else "nearest", pk["stacked"].max()))
        assert pk["stacked"].max() == 0
    o.close()
    o = oracle_api.OracleScene()
    sp.fill("chain_p23", o)
    R = sp.rays("chain_p23")
    for any_hit in (False, True):
        pk = o.stack_peaks(R["O"], R["D"], any_hit=any_hit)
        print("chain_p23 rays, %s: peak %d" % ("any-hit" if any_hit else "nearest", pk["stacked"].max()))
        assert pk["stacked"].max() == 23 > tp.STACK_ROWS_MAX
    o.close()


def test_the_scan_case_walks_deep(oracle_api, scenes):
    """tests/scan_cases.py 'deep_chain', the case that holds deep walks to the tree-free rule: its rays peak at 23 on the oracle"""
    import scan_cases
    o = oracle_api.OracleScene()
    rec = scan_cases.fill("deep_chain", o, scenes)
    O, D = scan_cases.make_rays("deep_chain", o, rec)
    assert len(O) % 64 != 0
    for any_hit in (False, True):
        pk = o.stack_peaks(O, D, any_hit=any_hit, scope=1)["stacked"]
        print("scan case deep_chain, %s: peak %d on %.3f of the rays" % ("any-hit" if any_hit else "nearest", pk.max(), (pk == pk.max()).mean()))
        assert pk.max() == 23 and (pk == 23).mean() > 0.7
    o.close()
