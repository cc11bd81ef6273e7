"""The traversal stack's spill half (csrc/rt_scene_dev.h Stack: the top 'rows' entries of a lane in LDS, the rest in the grid's spill
buffer, RT_STACK_MAX = 130 entries) held to the oracle on walks that are deep: the chains and instance chains of tests/spill_cases.py,
whose peak stack pointers tests/test_spill_cpu.py pins on the oracle (13 .. 61 without a TLAS around the 14 LDS rows and the general
kernels' 16; 45 .. 107 stacked, and rows - 1 / rows / rows + 1, under every row split a TLAS copy leaves).
  a  rt_intersect_batch, rt_occluded_batch and the *_scope forms at scene, accelerator, BLAS and instance scope: ids, t bits, normals and
     flags bit for bit under the default walk, RT_WIDE=0 / 1, RT_WIDE8=1 and RT_TLAS_LDS=0; in counting mode the tallies of the walk are
     the oracle's, so the device took the same pushes;
  b  the same on more rays than a full grid has lanes: every block's spill columns;
  c  rt_trace_batch on the render chain against Renderer::Trace / Sample under every schedule of the wavefronts and through both general
     kernels (bar: 1e-4 relative, floor 1e-3, non-finite values by class, a reference that is not all zero); the path schedules agree
     bit for bit;
  d  one entry past RT_STACK_MAX: RT_E_OVERFLOW that names the limit, and a context that goes on answering with the oracle's bits.
The hit record of the C ABI carries the object id, the material, t and the normal; primitive and instance numbers are not part of it."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_cases as dc  # noqa: E402
import spill_cases as sc  # noqa: E402
import support as sp  # noqa: E402
from conftest import rel_err  # noqa: E402
from test_gpu_parity import RADIANCE_TOL, make_pair  # noqa: E402

pytestmark = pytest.mark.gpu

WALK_ENVS = [{}, {"RT_WIDE": "0"}, {"RT_WIDE": "1"}, {"RT_WIDE8": "1"}]
TLAS_ENVS = WALK_ENVS + [{"RT_TLAS_LDS": "0"}]
NEAREST_TALLIES = ("inner_visits", "prim_tests", "tlas_inner", "instance_visits", "rays_nearest", "brute_tests", "light_tests")
OCCLUDED_TALLIES = ("inner_visits", "prim_tests", "tlas_inner", "instance_visits", "rays_occluded")

_REF = {}


def _scopes(name):
    """(scope, index): the accelerator, every BLAS, and of an instance chain its first and last instance"""
    if sc.CASES[name]["kind"] == "chain":
        return [(1, 0), (2, 0)]
    return [(1, 0), (2, 0), (2, 1), (3, 0), (3, sc.CASES[name]["m"] - 1)]


def _reference(name, key, R, oracle_api, host_api):
    """the oracle's answers for the ray set R of the case's scene, computed once"""
    if key not in _REF:
        o = oracle_api.OracleScene()
        sc.fill(name, o, host_api)
        O, D = R["O"], R["D"]
        ref = dict(nearest=o.find_nearest(O, D), occluded=o.is_occluded(O, D))
        if key != "large":
            for s in _scopes(name):
                ref[s] = (o.scope_nearest(s[0], s[1], O, D), o.scope_occluded(s[0], s[1], O, D))
        o.close()
        _REF[key] = ref
    return _REF[key]


def _same_hits(got, ref, what, everywhere):
    assert np.array_equal(got["obj"], ref["obj"]), what
    on = np.ones(len(ref["obj"]), bool) if everywhere else ref["obj"] != -1
    assert sp.same(got["t"][on], ref["t"][on]), what
    hit = ref["obj"] != -1
    assert hit.any() and not hit.all(), what
    assert sp.same(got["normal"][hit], ref["normal"][hit]), what
    assert np.array_equal(got["mat"][hit], ref["mat"][hit]), what


def _device(name, env, host_api, monkeypatch):
    """a context under env with the case's scene; its row split is the layout builder's"""
    sp.clean_env(monkeypatch, env)
    r = host_api.HostRenderer(8, 8)
    sc.fill(name, r.scene, host_api)
    r.commit()
    L = host_api.layout(r.scene.describe(), *sp.layout_knobs(env))
    info = r.build_info()
    assert "tlas_lds=%d stack_rows=%d " % (L["tlasLds"], L["stackRows"]) in info, info
    if not env:
        assert (L["stackRows"], L["tlasLds"]) == sc.rows_of(name, host_api)
    if env.get("RT_TLAS_LDS") == "0":
        assert L["tlasLds"] == 0
    return r


def _queries(r, R, ref, what, scopes):
    O, D = R["O"], R["D"]
    for counting in (False, True):
        r.set_counting(counting)
        r.counters()
        _same_hits(r.find_nearest(O, D), ref["nearest"], "%s find_nearest counting=%d" % (what, counting), True)
        cnt = r.counters()
        if counting:
            for k in NEAREST_TALLIES:
                assert cnt[k] == ref["nearest"]["counters"][k], (what, k, cnt[k], ref["nearest"]["counters"][k])
        occ = r.is_occluded(O, D)
        cnt = r.counters()
        assert np.array_equal(occ, ref["occluded"]["occluded"]), "%s is_occluded counting=%d" % (what, counting)
        if counting:
            for k in OCCLUDED_TALLIES:
                assert cnt[k] == ref["occluded"]["counters"][k], (what, k, cnt[k], ref["occluded"]["counters"][k])
        for s in scopes:
            near, flags = ref[s]
            _same_hits(r.scope_nearest(s[0], s[1], O, D), near, "%s scope %s counting=%d" % (what, s, counting), False)
            assert np.array_equal(r.scope_occluded(s[0], s[1], O, D), flags), "%s scope %s occluded counting=%d" % (what, s, counting)
    r.set_counting(False)


# ---- a: queries -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,env", [(n, e) for n in sc.CHAINS for e in WALK_ENVS] + [(n, e) for n in sc.TLAS for e in TLAS_ENVS],
                         ids=lambda v: v if isinstance(v, str) else sp.env_id(v))
def test_deep_walks_answer_as_the_oracle(name, env, oracle_api, host_api, monkeypatch):
    """Every query form on the case's interleaved ray set, bit for bit, counting off and on (the tallies are the oracle's: the same
    visits, so the same pushes).  The nearest-hit walk and the counting walks are the reference's binary walk under every knob; the
    any-hit walk of a scene BVH is the 4-wide one by default (its stack stays shallow on a chain: the far inner node is pushed first),
    the binary one under RT_WIDE=0 and with a TLAS."""
    R = sc.rays(name)
    ref = _reference(name, name, R, oracle_api, host_api)
    r = _device(name, env, host_api, monkeypatch)
    _queries(r, R, ref, "%s [%s]" % (name, sp.env_id(env)), _scopes(name))
    r.close()


# ---- b: more rays than lanes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"RT_WIDE": "1"}, {"RT_WIDE": "0"}], ids=sp.env_id)
def test_every_blocks_spill_columns(env, oracle_api, host_api, monkeypatch):
    """256 * 8 * 256 + 12,345 rays, half of them nine entries into the spill: the whole grid runs, the last blocks' columns of the
    spill buffer ([entry][global lane], sized for gridBlocks * RT_BLOCK lanes) are written and read back"""
    R = sc.large_rays()
    ref = _reference(sc.LARGE_SCENE, "large", R, oracle_api, host_api)
    r = _device(sc.LARGE_SCENE, env, host_api, monkeypatch)
    _queries(r, R, ref, "large [%s]" % sp.env_id(env), [])
    r.close()


# ---- c: rt_trace_batch on the render chain --------------------------------------------------------------------------------------------------
PATH_ENVS = dc.PATH_ENVS + [{"RT_WIDE": "0"}, {"RT_WIDE": "1"}, {"RT_WIDE8": "1"}, {"RT_MIXED_MAX": "100"}, {"RT_STREAM": "0", "RT_SLOTS": "100"}]
_RENDER_REF, _PATH_FIRST = {}, {}


def _render_ref(oracle_api, mode, flag):
    if (mode, flag) not in _RENDER_REF:
        o = oracle_api.OracleScene()
        sc.render_chain(o)
        o.set_raytracer(flag)
        orr = oracle_api.OracleRenderer(o, 8, 8)
        O, D = sc.render_rays()
        _RENDER_REF[(mode, flag)] = {d: orr.trace_rays(mode, O, D, d, sc.ENERGY, seed_base=sc.SEED_BASE) for d in sc.RENDER_DEPTHS}
        orr.close()
        o.close()
    return _RENDER_REF[(mode, flag)]


def _hold(got, ref, what):
    err, cls_ok = rel_err(got, ref)
    fin = np.isfinite(ref)
    print("%s: max relative error %.3g, %d non-finite values" % (what, err.max(), int((~fin).sum())))
    assert cls_ok, what
    assert err.max() <= RADIANCE_TOL, (what, err.max())
    assert np.abs(ref[fin]).sum() > 0, what


def _render_device(host_api, monkeypatch, env):
    sp.clean_env(monkeypatch, env)
    r = host_api.HostRenderer(8, 8)
    sc.render_chain(r.scene)
    r.commit()
    return r


@pytest.mark.parametrize("env", PATH_ENVS, ids=sp.env_id)
def test_sample_on_the_render_chain(env, oracle_api, host_api, monkeypatch):
    """Renderer::Sample as Tick calls it, depths 1 and 4: the extend walk of every ray and the shadow walk of every hit run the chain
    to the bottom (peak 23).  RT_FUSE=2 walks dense.sideSpill on the second stream, RT_FUSE=1 and the default below RT_MIXED_MAX
    k_traverse_s, RT_MIXED_MAX=100 the split launches, RT_STREAM=0 the slot kernels (with fewer slots than rays under RT_SLOTS);
    RT_WIDE=0 sends the shadow rays down the binary walk.  Every schedule within the bar of the oracle, and the same bits."""
    assert all(len(sc.render_rays()[0]) > int(v) for e in PATH_ENVS for k, v in e.items() if k in ("RT_SLOTS", "RT_MIXED_MAX"))
    ref = _render_ref(oracle_api, dc.SAMPLE, False)
    r = _render_device(host_api, monkeypatch, env)
    O, D = sc.render_rays()
    got = {d: r.trace_batch(host_api.RT_MODE_PATH, O, D, depth=d, seed_base=sc.SEED_BASE, energy=sc.ENERGY) for d in sc.RENDER_DEPTHS}
    first = _PATH_FIRST.setdefault("sample", got)
    for d in sc.RENDER_DEPTHS:
        _hold(got[d], ref[d], "render chain [%s] Sample depth %d" % (sp.env_id(env), d))
        assert sp.same(got[d], first[d]), (env, d)
    r.close()


@pytest.mark.parametrize("env", dc.WHITTED_ENVS + [{"RT_WIDE": "0"}], ids=sp.env_id)
def test_trace_on_the_render_chain(env, oracle_api, host_api, monkeypatch):
    """Renderer::Trace as Tick calls it under the three Whitted schedules (and with binary shadow walks), depths 1 and 4"""
    ref = _render_ref(oracle_api, dc.TRACE, True)
    r = _render_device(host_api, monkeypatch, env)
    O, D = sc.render_rays()
    for d in sc.RENDER_DEPTHS:
        got = r.trace_batch(host_api.RT_MODE_WHITTED, O, D, depth=d, seed_base=sc.SEED_BASE, energy=sc.ENERGY)
        _hold(got, ref[d], "render chain [%s] Trace depth %d" % (sp.env_id(env), d))
    r.close()


@pytest.mark.parametrize("mode,flag", [(dc.TRACE, False), (dc.SAMPLE, True)], ids=["Trace-flag_clear", "Sample-flag_set"])
def test_general_kernels_on_the_render_chain(mode, flag, oracle_api, host_api, monkeypatch):
    """k_trace_general and k_sample_general keep RT_STACK_LDS = 16 entries in LDS: 23 is seven into the spill"""
    assert sc.RENDER_PEAK > sc.GENERAL_ROWS
    ref = _render_ref(oracle_api, mode, flag)
    r = _render_device(host_api, monkeypatch, {})
    r.set_scene_raytracer(1 if flag else 0)
    O, D = sc.render_rays()
    for d in sc.RENDER_DEPTHS:
        got = r.trace_batch(mode, O, D, depth=d, seed_base=sc.SEED_BASE, energy=sc.ENERGY)
        _hold(got, ref[d], "render chain general %s depth %d" % ("Sample" if mode == dc.SAMPLE else "Trace", d))
    r.close()


# ---- d: past the limit ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"RT_WIDE": "0"}], ids=sp.env_id)
def test_a_walk_past_the_limit_is_reported(env, oracle_api, host_api, monkeypatch):
    """136 triangles, 135 entries wanted: the push at RT_STACK_MAX stores nothing, raises the status word and empties the lane's stack
    (Stack::push), the ray ends at a pop of the empty stack, and the call returns RT_E_OVERFLOW naming the limit -- from the nearest-hit
    and the any-hit query, counting or not (these axis-parallel rays are not clean: the default 4-wide walk hands them to the binary
    one).  The status word does not leak: the same context then takes a legal scene and answers with the oracle's bits."""
    sp.clean_env(monkeypatch, env)
    r = host_api.HostRenderer(8, 8)
    sc.overflow_chain(r.scene)  # the host's builder only: never the oracle's walk
    r.commit()
    O, D = sc.overflow_rays()
    for counting in (False, True):
        r.set_counting(counting)
        for call in (lambda: r.find_nearest(O, D), lambda: r.is_occluded(O, D), lambda: r.scope_nearest(1, 0, O, D), lambda: r.scope_occluded(2, 0, O, D)):
            with pytest.raises(RuntimeError) as ei:
                call()
            last = r.rt.rt_last_error(r.ctx).decode()
            for text in (str(ei.value), last):
                assert re.search(r"traversal stack deeper than %d entries" % sc.STACK_MAX, text), text
            assert "error -6:" in str(ei.value)  # RT_E_OVERFLOW (include/rt_amd.h)
    r.set_counting(False)
    # a shallow ray on the same scene is answered: the word was reset
    assert r.is_occluded(O[:5] * np.float32(-1), D[:5]).tolist() == [0] * 5
    name = "chain_p15"
    legal = host_api.HostScene()
    sc.fill(name, legal, host_api)
    r.upload_desc(legal.describe())
    R = sc.rays(name)
    _queries(r, R, _reference(name, name, R, oracle_api, host_api), "%s after the overflow" % name, _scopes(name))
    legal.close()
    r.close()
