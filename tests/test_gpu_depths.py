"""The start depth of Renderer::Trace / Renderer::Sample as a tested axis, on the device through host_api: rt_trace_batch_energy and
rt_render(..., max_depth) against the oracle at every depth the pipelines shape themselves by, not at 4 alone.
  A  Sample as Tick calls it on the round pipelines (csrc/rt_stream.h run_rounds_stream: rounds = depth + 1, the one-round form of
     generate, last / lastNext, the counts' rotation; the slot pipeline's knownRounds), depths -1 .. 7 under every schedule;
  B  the general kernels (k_trace_general, k_sample_general) at depths 1 .. 7 -- from depth 5 on the first hit draws no roulette number
     -- and on 'hall' up to the last depth that fits their call-frame stacks;
  C  Whitted frames and caller rays against the oracle at depths 1, 2, 3, 5 and 7 under the three Whitted schedules;
  D  one level past the call-frame stacks: RT_E_OVERFLOW that names the stack and its limit, and a context that goes on working.
tests/depth_cases.py holds the inputs, tests/test_depths_cpu.py shows on the oracle that neighbouring depths differ on enough rays.
Bar: radiance within 1e-4 relative (BASELINE.json north star), non-finite values equal by class, a reference that is not all zero."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_cases as dc  # noqa: E402
import support as sp  # noqa: E402
from conftest import rel_err  # noqa: E402
from test_gpu_parity import RADIANCE_TOL, make_pair  # noqa: E402

pytestmark = pytest.mark.gpu


def _pair(scenes, oracle_api, host_api, name, w=dc.W, h=dc.H):
    fn, kw = dc.scene_fn(scenes, name)
    return make_pair(fn, oracle_api, host_api, w, h, **kw)


def _hold(got, ref, what):
    """the project's radiance bar; the figure is printed before it is asserted"""
    err, cls_ok = rel_err(got, ref)
    fin = np.isfinite(ref)
    print("%s: max relative error %.3g, %d non-finite values" % (what, err.max(), int((~fin).sum())))
    assert cls_ok, what
    assert err.max() <= RADIANCE_TOL, (what, err.max())
    assert np.abs(ref[fin]).sum() > 0, what


# ---- A: path mode on the round pipelines ----------------------------------------------------------------------------------------------
_PATH_FIRST = {}  # scene -> {depth: the values of the first environment that ran}


@pytest.mark.parametrize("env", dc.PATH_ENVS, ids=sp.env_id)
@pytest.mark.parametrize("name", dc.PATH_SCENES)
def test_sample_on_the_round_pipelines_at_every_depth(name, env, scenes, oracle_api, host_api, monkeypatch):
    """Renderer::Sample with the flag clear at start depths -1 .. 7: zero to eight rounds (depth -1 is 0.05 from the host, depth 0 the
    one-round form, 1 and 2 the loop's other edges, 5 .. 7 more rounds than any frame runs).  Every depth within the bar of the oracle,
    and the same bits under every schedule; on the default schedule the batches of the first 1 and 65 rays give the bits those rays
    have in the full batch (a ray's stream is StreamSeed(seed_base + index): nothing depends on the batch around it)."""
    ref = dc.oracle_values(scenes, oracle_api, name, dc.SAMPLE, False, dc.PATH_DEPTHS)
    sp.clean_env(monkeypatch, env)
    o, orr, r, d = _pair(scenes, oracle_api, host_api, name)
    O, D = orr.primary_rays()
    got = {depth: r.trace_batch(host_api.RT_MODE_PATH, O, D, depth=depth, seed_base=dc.SEED_BASE, energy=dc.ENERGY) for depth in dc.PATH_DEPTHS}
    first = _PATH_FIRST.setdefault(name, got)
    for depth in dc.PATH_DEPTHS:
        _hold(got[depth], ref[depth], "%s [%s] Sample depth %d" % (name, sp.env_id(env), depth))
        assert sp.same(got[depth], first[depth]), (name, env, depth)
    assert np.all(got[-1] == np.float32(0.05))
    if not env:
        for depth in dc.PREFIX_DEPTHS:
            for n in dc.PREFIX_SIZES:
                part = r.trace_batch(host_api.RT_MODE_PATH, O[:n], D[:n], depth=depth, seed_base=dc.SEED_BASE, energy=dc.ENERGY)
                assert sp.same(part, got[depth][:n]), (name, depth, n)
    r.close()


# ---- B: the general kernels ---------------------------------------------------------------------------------------------------------------
def _general_id(case):
    name, mode, flag, _ = case
    return "%s-%s-flag_%s" % (name, "Sample" if mode == dc.SAMPLE else "Trace", "set" if flag else "clear")


@pytest.mark.parametrize("case", dc.GENERAL_CASES, ids=_general_id)
def test_general_kernels_at_every_depth(case, scenes, oracle_api, host_api):
    """k_trace_general (Trace with the flag clear) and k_sample_general (Sample with the flag set, and Sample with it clear where the
    wavefront cannot replay the scene) against the oracle.  Both kernels draw the first hit's roulette number only when depth < 5: at
    depths 5, 6 and 7 every later draw of the tree sits one place earlier (tests/test_depths_cpu.py: 39 to 45 % of the rays change
    from 4 to 5).  'hall' nests a frame per level: depth 5 of Sample and depth 12 of Trace fill the kernels' frame stacks exactly."""
    name, mode, flag, depths = case
    ref = dc.oracle_values(scenes, oracle_api, name, mode, flag, depths)
    o, orr, r, d = _pair(scenes, oracle_api, host_api, name)
    O, D = orr.primary_rays()
    r.set_scene_raytracer(1 if flag else 0)
    for depth in depths:
        got = r.trace_batch(mode, O, D, depth=depth, seed_base=dc.SEED_BASE, energy=dc.ENERGY)
        _hold(got, ref[depth], "%s depth %d" % (_general_id(case), depth))
        if mode == dc.SAMPLE and depth < 0:
            assert np.all(got == np.float32(0.05))
    r.close()


@pytest.mark.parametrize("path,flag", [(False, False), (True, True)], ids=["Trace-flag_clear", "Sample-flag_set"])
def test_general_kernels_through_the_host_surface_at_depth_5(path, flag, scenes, oracle_api, host_api):
    """rapt::Renderer::Trace / Sample take the flag from their Scene: one ray at depth 5, where the first hit draws no roulette number"""
    o, orr, r, d = _pair(scenes, oracle_api, host_api, "mixed_small_rt0")
    O, D = orr.primary_rays()
    i = dc.ONE_RAY
    o.set_raytracer(flag)
    r.scene.set_raytracer(flag)
    one = r.trace_one(O[i], D[i], dc.ONE_DEPTH, path=path, energy=dc.ENERGY)
    ref = orr.trace_rays(dc.SAMPLE if path else dc.TRACE, O[i:i + 1], D[i:i + 1], dc.ONE_DEPTH, dc.ENERGY, seed_base=dc.ONE_SEED)[0]
    # the ray must be one the roulette's gate matters for: depth 4 gives it another value
    assert not np.array_equal(ref, orr.trace_rays(dc.SAMPLE if path else dc.TRACE, O[i:i + 1], D[i:i + 1], 4, dc.ENERGY, seed_base=dc.ONE_SEED)[0])
    _hold(one, ref, "trace_one path=%d depth %d" % (path, dc.ONE_DEPTH))
    r.close()


# ---- C: Whitted against the oracle ------------------------------------------------------------------------------------------------------
_WHITTED_REF = {}


def _whitted_ref(scenes, oracle_api, name):
    """depth -> the oracle's frame [h][w][3] (rendered once per session)"""
    if name not in _WHITTED_REF:
        w, h, depths = dc.WHITTED_CASES[name]
        o, orr = dc.oracle_pair(scenes, oracle_api, name, w, h)
        o.set_raytracer(True)
        frames = {}
        for depth in depths:
            orr.clear()
            orr.render(0, 1, max_depth=depth)
            frames[depth] = orr.accumulator()[..., :3].copy()
            frames[depth].setflags(write=False)
        orr.close()
        o.close()
        _WHITTED_REF[name] = frames
    return _WHITTED_REF[name]


@pytest.mark.parametrize("env", dc.WHITTED_ENVS, ids=sp.env_id)
@pytest.mark.parametrize("name", list(dc.WHITTED_CASES))
def test_whitted_against_the_oracle_at_every_depth(name, env, scenes, oracle_api, host_api, monkeypatch):
    """Renderer::Trace with the flag set under the default schedule, the wavefront rounds (RT_MEGA=0) and the tree levels
    (RT_MEGA_LEVELS=1): frames of an odd size through rt_render(max_depth) and the caller rays through rt_trace_batch, each against the
    oracle.  The three share their shading code (childTraces = depth > 0, the pending branches), so agreeing with each other, as
    test_whitted_levels_depths_and_batches has them do, says nothing about an error they share."""
    w, h, depths = dc.WHITTED_CASES[name]
    frames = _whitted_ref(scenes, oracle_api, name)
    rays = dc.oracle_values(scenes, oracle_api, name, dc.TRACE, True, depths)
    sp.clean_env(monkeypatch, env)
    o, orr, r, d = _pair(scenes, oracle_api, host_api, name, w, h)
    o48, orr48 = dc.oracle_pair(scenes, oracle_api, name)
    O, D = orr48.primary_rays()
    for depth in depths:
        r.clear()
        r.render(host_api.RT_MODE_WHITTED, 0, 1, max_depth=depth)
        _hold(r.accumulator()[..., :3], frames[depth], "%s [%s] %d x %d frame, max_depth %d" % (name, sp.env_id(env), w, h, depth))
        got = r.trace_batch(host_api.RT_MODE_WHITTED, O, D, depth=depth, seed_base=dc.SEED_BASE, energy=dc.ENERGY)
        _hold(got, rays[depth], "%s [%s] Trace depth %d" % (name, sp.env_id(env), depth))
    r.close()
    orr48.close()
    o48.close()


# ---- D: the call-frame stacks, reported for what they are ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,fits,overflows,limit", [(dc.SAMPLE, dc.HALL_SAMPLE_FITS, dc.HALL_SAMPLE_OVERFLOWS, dc.SAMPLE_FRAMES),
                                                       (dc.TRACE, dc.HALL_TRACE_FITS, dc.HALL_TRACE_OVERFLOWS, dc.TRACE_FRAMES)], ids=["Sample", "Trace"])
def test_full_frame_stack_is_reported_as_such(mode, fits, overflows, limit, scenes, oracle_api, host_api):
    """On 'hall' every level nests a frame.  Sample (flag clear) holds RT_SAMPLE_FRAMES = 6 suspended light loops: depth 5 fits, depth 6
    is the smallest that does not.  Trace (flag clear) holds RT_TRACE_FRAMES = 12: depth 12 fits, 13 is the smallest that does not.  The
    push past the limit is dropped behind a bounds check and raises the status word; the call returns RT_E_OVERFLOW with a message that
    names the call-frame stack and its limit, rt_last_error keeps it, and the status word is reset: the next call at the last depth
    that fits returns the bits it returned before."""
    o, orr, r, d = _pair(scenes, oracle_api, host_api, "hall")
    O, D = orr.primary_rays()
    r.set_scene_raytracer(0)
    before = r.trace_batch(mode, O, D, depth=fits, seed_base=dc.SEED_BASE, energy=dc.ENERGY)
    with pytest.raises(RuntimeError) as ei:
        r.trace_batch(mode, O, D, depth=overflows, seed_base=dc.SEED_BASE, energy=dc.ENERGY)
    last = r.rt.rt_last_error(r.ctx).decode()
    for text in (str(ei.value), last):
        assert "call-frame stack" in text and re.search(r"\b%d nested call frames" % limit, text) and "lower depth" in text, text
        assert ("Trace" if mode == dc.TRACE else "Sample") in text and "traversal stack" not in text, text
    assert "error -6:" in str(ei.value)  # RT_E_OVERFLOW (include/rt_amd.h)
    after = r.trace_batch(mode, O, D, depth=fits, seed_base=dc.SEED_BASE, energy=dc.ENERGY)
    assert sp.same(after, before)
    _hold(after, dc.oracle_values(scenes, oracle_api, "hall", mode, False, (fits,))[fits], "hall after the overflow, depth %d" % fits)
    r.close()
