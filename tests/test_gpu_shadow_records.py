"""The dense pipeline's shadow records (csrc/rt_stream.h StreamState::shI / shX) hold the hit point, the RNG state before the
light loop and two entry indices; light rebuilds every sampled light position by replaying light_position's draws from that
state (connect reads them from shP), and reads the hit's normal, direction, weight and material from its round's entry.  Held here: the
dense pipeline renders the slot pipeline's frames bit for bit on scenes whose light lists mix lights that draw (area lights:
two draws each) with lights that do not (directional lights), in both orders, with one light and with the most lights a
scene may have, on every schedule of the round loop (one traversal launch per round, two streams, one kernel at a time --
the schedule of batches of 100 M samples and more), through the 2-, 4- and 8-wide occlusion walks, and with the
Q-learning sampler (which always takes the dense pipeline: its schedules must agree with one another and with the oracle)."""
import numpy as np
import pytest

import support as sp
from lit_scene import lit_scene
from test_gpu_parity import RADIANCE_TOL, rel_err

pytestmark = pytest.mark.gpu

SCHEDULES = (("one_launch_per_round", {"RT_FUSE": "1"}), ("two_streams", {"RT_FUSE": "2"}), ("one_kernel_at_a_time", {"RT_FUSE": "0"}))


def _frame(host_api, kinds, env, monkeypatch, w, h, frames, qlearn=False):
    sp.clean_env(monkeypatch, env)
    r = host_api.HostRenderer(w, h)
    lit_scene(r.scene, kinds)
    r.commit()
    if qlearn:
        r.qlearn_enable(8, (-4, -1, -4), (4, 5, 6), 0.3, 0.2, 1.0, 0)
    r.clear()
    r.render(host_api.RT_MODE_PATH, 0, frames)
    if qlearn:
        r.qlearn_apply()
        r.render(host_api.RT_MODE_PATH, frames, frames)
    out = r.accumulator().copy()
    table = r.qlearn_table().copy() if qlearn else None
    r.close()
    return out, table


@pytest.mark.parametrize("kinds", ["A", "D", "AD", "DA", "ADDA", "DAAD", "A" * 32, ("AD" * 16)])
def test_stream_shadow_records_equal_slot_pipeline(kinds, host_api, monkeypatch):
    """every schedule of the dense pipeline against the slot pipeline (RT_STREAM=0, which stores every sampled position)"""
    w, h, frames = (64, 40, 3) if len(kinds) > 4 else (96, 54, 4)
    ref, _ = _frame(host_api, kinds, {"RT_STREAM": "0"}, monkeypatch, w, h, frames)
    fin = np.isfinite(ref[..., :3])
    assert fin.mean() > 0.5 and (ref[..., :3][fin] > 0).mean() > 0.2  # lit: a light's disk seen directly is +inf or NaN (Q7)
    for key, env in SCHEDULES:
        got, _ = _frame(host_api, kinds, env, monkeypatch, w, h, frames)
        assert sp.same(ref, got), (kinds, key)


@pytest.mark.parametrize("walk", [{"RT_WIDE": "1"}, {"RT_WIDE8": "1"}])
@pytest.mark.parametrize("kinds", ["ADA", "DAD"])
def test_stream_shadow_records_wide_walks(kinds, walk, host_api, monkeypatch):
    """the 4-wide walk with its leftover list and the 8-wide walk read the same records: the binary walk's frames, every schedule"""
    w, h, frames = 80, 48, 3
    ref, _ = _frame(host_api, kinds, {"RT_STREAM": "0"}, monkeypatch, w, h, frames)
    for key, env in SCHEDULES:
        got, _ = _frame(host_api, kinds, dict(env, **walk), monkeypatch, w, h, frames)
        assert sp.same(ref, got), (kinds, walk, key)


def test_stream_shadow_records_larger_batch(host_api, monkeypatch):
    """a batch of 1.2 M samples, above the one-launch-per-round limit (RT_MIXED_MAX lowered to reach it at an affordable size), on
    the default schedule and one kernel at a time (the schedule of the largest batches)"""
    w, h, frames, kinds = 320, 240, 16, "ADAD"
    ref, _ = _frame(host_api, kinds, {"RT_STREAM": "0"}, monkeypatch, w, h, frames)
    for key, env in (("default", {"RT_MIXED_MAX": "100000"}), ("one_kernel_at_a_time", {"RT_FUSE": "0"})):
        got, _ = _frame(host_api, kinds, env, monkeypatch, w, h, frames)
        assert sp.same(ref, got), key


@pytest.mark.parametrize("kinds", ["AD", "DA"])
def test_stream_shadow_records_with_sampler(kinds, host_api, oracle_api, monkeypatch):
    """the Q-learning sampler (k_shade_s<true>): the same frame and table on every schedule, the oracle's table bit for bit and its
    frame within the radiance tolerance"""
    w, h, frames = 64, 40, 3
    out = {}
    for key, env in SCHEDULES:
        out[key] = _frame(host_api, kinds, env, monkeypatch, w, h, frames, qlearn=True)
    first = out[SCHEDULES[0][0]]
    for key, _ in SCHEDULES[1:]:
        assert sp.same(first[0], out[key][0]) and sp.same(first[1], out[key][1]), (kinds, key)
    o = oracle_api.OracleScene()
    lit_scene(o, kinds)
    orr = oracle_api.OracleRenderer(o, w, h)
    orr.scene.set_raytracer(False)
    orr.qlearn_enable(8, (-4, -1, -4), (4, 5, 6), 0.3, 0.2, 1.0, 0)
    orr.clear()
    orr.render(0, frames, nthreads=0); orr.qlearn_apply()
    orr.render(frames, frames, nthreads=0)
    assert sp.same(orr.qlearn_state()[2], first[1])
    err, cls_ok = rel_err(first[0][..., :3], orr.accumulator()[..., :3])
    assert cls_ok and err.max() <= RADIANCE_TOL, err.max()
