"""The shade step (csrc/rt_shade.h) on crafted hits, on the device through HostRenderer.trace_batch: every pipeline that calls it against
the oracle on the cases of tests/shade_cases.py -- glass by index of refraction on both sides of the critical angle, the diffuse exponents
and the retention branch, metal under an energy, area and directional lights on every branch of their intensity, 0 to 32 lights, the
roulette, scaled instances.  tests/test_shade_cpu.py shows on the oracle alone that every case reaches its branch.
  Sample as Tick calls it   the dense and the slot wavefront under every schedule of depth_cases.PATH_ENVS, the dense one with the
                            material and light tables read from memory (RT_SHADE_LDS=0, a switch of the dense kernels alone), and the
                            slot one under a budget of 24 slots, below every batch: refilled slots, samples stored by the finish pass;
  Trace as Tick calls it    the three Whitted schedules of depth_cases.WHITTED_ENVS;
  the general kernels       Trace with the flag clear, Sample with it set, and Sample with it clear on materials built with it clear.
One context per (scene, environment); all cases of a scene that share a function and a depth are one trace_batch call.
Bar: the project's -- radiance within 1e-4 relative (floor 1e-3), non-finite values equal by class; the schedules of one function agree
with each other under the same bar, and those of the path wavefront bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_cases as dc  # noqa: E402
import shade_cases as sc  # noqa: E402
import support as sp  # noqa: E402
from conftest import rel_err  # noqa: E402
from test_gpu_parity import RADIANCE_TOL  # noqa: E402

pytestmark = pytest.mark.gpu


def _device(host_api, scene, rt, monkeypatch, env):
    """a context reads its switches when it is created (csrc/rt_ctx.h Knobs)"""
    sp.clean_env(monkeypatch, env)
    r = host_api.HostRenderer(8, 8)
    sc.SCENES[scene](r.scene, rt=rt)
    r.commit()
    return r


def _run(r, oracle_api, scene, pipeline, what):
    """every batch of (scene, pipeline) on the device, each case held to the oracle; {depth: the device's values}.  The figures are
    printed before they are asserted."""
    mode, flag, rt = sc.PIPELINES[pipeline]
    out, bad = {}, []
    for depth, O, D, where, ref in sc.reference(oracle_api, scene, pipeline):
        got = r.trace_batch(mode, O, D, depth=depth, seed_base=sc.SEED_BASE, energy=sc.energy_of(scene))
        out[depth] = got
        for name, at in where.items():
            err, cls_ok = rel_err(got[at], ref[at])
            fin = np.isfinite(ref[at])
            print("shade-err family=%d pipeline=%s [%s] case=%s depth=%d err=%.3g nonfinite=%d" % (sc.BY_NAME[name].family, pipeline, what, name, depth, err.max(), int((~fin).sum())))
            if not cls_ok or err.max() > RADIANCE_TOL:
                bad.append((name, depth, float(err.max()), bool(cls_ok)))
            assert sc.BY_NAME[name].expect == "direct" or np.abs(ref[at][fin]).sum() > 0, name
    assert not bad, (scene, pipeline, what, bad)
    return out


def _agree(got, first, what, exact):
    for depth in got:
        same = sp.same(got[depth], first[depth])
        err, cls_ok = rel_err(got[depth], first[depth])
        print("%s depth %d against the first schedule: %s, max relative difference %.3g" % (what, depth, "same bits" if same else "other bits", err.max()))
        assert cls_ok and err.max() <= RADIANCE_TOL, (what, depth, err.max())
        if exact:
            assert same, (what, depth)


_FIRST = {}


@pytest.mark.parametrize("env", dc.PATH_ENVS + sc.OWN_ENVS, ids=sp.env_id)
@pytest.mark.parametrize("scene", sc.SAMPLE_SCENES)
def test_sample_on_the_wavefronts(scene, env, oracle_api, host_api, monkeypatch):
    """Renderer::Sample with the flag clear: k_shade_s / k_light_s (dense) under the fuse modes, with the producer-side decisions off and
    with the tables from memory; k_shade / k_light (slot) with a slot per sample (RT_SLOTS unset, 777, and once more under RT_SHADE_LDS=0,
    which the slot kernels do not read) and with 24 slots for batches of 32 to 528 samples -- the same bits under all of them"""
    if env.get("RT_SLOTS") == str(sc.SLOT_BUDGET):
        assert env.get("RT_STREAM") == "0" and all(len(O) > sc.SLOT_BUDGET for _, O, _, _ in sc.batches(scene, "sample"))  # fewer slots than samples in every batch
    r = _device(host_api, scene, True, monkeypatch, env)
    got = _run(r, oracle_api, scene, "sample", sp.env_id(env))
    _agree(got, _FIRST.setdefault(("sample", scene), got), "%s Sample [%s]" % (scene, sp.env_id(env)), exact=True)
    r.close()


@pytest.mark.parametrize("env", dc.WHITTED_ENVS, ids=sp.env_id)
@pytest.mark.parametrize("scene", sc.TRACE_SCENES)
def test_trace_on_the_whitted_schedules(scene, env, oracle_api, host_api, monkeypatch):
    """Renderer::Trace with the flag set: the Whitted policies of rt_mega.h under the default schedule, the wavefront rounds (RT_MEGA=0)
    and the tree levels (RT_MEGA_LEVELS=1); 'shiny' adds the mirror branch of a diffuse hit"""
    r = _device(host_api, scene, True, monkeypatch, env)
    got = _run(r, oracle_api, scene, "trace", sp.env_id(env))
    _agree(got, _FIRST.setdefault(("trace", scene), got), "%s Trace [%s]" % (scene, sp.env_id(env)), exact=False)
    r.close()


@pytest.mark.parametrize("scene", sc.GENERAL_SCENES)
def test_general_kernels(scene, oracle_api, host_api, monkeypatch):
    """k_trace_general (Trace with the flag clear) and k_sample_general (Sample with the flag set; Sample with it clear where the
    materials were built with it clear or shine) on the same cases, and family 7 -- the roulette -- where only these two play it"""
    r = _device(host_api, scene, False, monkeypatch, {})
    ran = 0
    for pipeline in ("trace_g", "sample_g", "sample_g0"):
        if not sc.batches(scene, pipeline):
            continue
        r.set_scene_raytracer(1 if sc.PIPELINES[pipeline][1] else 0)
        ran += len(_run(r, oracle_api, scene, pipeline, "general"))
    assert ran > 0
    r.close()


def test_every_case_runs_somewhere():
    """the three tests above, between them, run every (case, pipeline) of tests/shade_cases.py"""
    ran = set()
    for scenes, pipelines in ((sc.SAMPLE_SCENES, ("sample",)), (sc.TRACE_SCENES, ("trace",)), (sc.GENERAL_SCENES, ("trace_g", "sample_g", "sample_g0"))):
        for scene in scenes:
            for p in pipelines:
                for _, _, _, where in sc.batches(scene, p):
                    ran |= {(name, p) for name in where}
    assert ran == {(c.name, p) for c in sc.CASES for p in c.pipelines}
    sizes = [len(O) for scene in sc.SAMPLE_SCENES for _, O, _, _ in sc.batches(scene, "sample")]
    assert sc.SLOT_BUDGET < min(sizes) and 8 * sc.SLOT_BUDGET < max(sizes) < 777  # the budget of this tier refills its slots in every batch, many times in the large ones; depth_cases' 777 in none
    assert {"RT_STREAM": "0", "RT_SLOTS": str(sc.SLOT_BUDGET)} in sc.OWN_ENVS
    assert len(dc.PATH_ENVS + sc.OWN_ENVS) * len(sc.SAMPLE_SCENES) + len(dc.WHITTED_ENVS) * len(sc.TRACE_SCENES) + len(sc.GENERAL_SCENES) <= 80  # contexts
