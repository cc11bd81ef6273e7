"""numpy restatement of rt_reproject_motion (include/rt_amd.h): rt_reproject with the point and the normal of a moved instance's pixel taken
back through the instance's own motion first.  Built on tests/reproject_ref.py, which does the projection, the acceptance tests and the
gather; this module adds what the header adds:

  k = inst_p;  moved_k = k >= 0 && any of instance k's 24 words (T rows 0..2, invT rows 0..2) differs BITWISE from the capture's
  !moved_k:  x_h = x_p;  n_h = n_p                                   (the bits are kept: no arithmetic)
   moved_k:  x_h = xform_pos(T'_k, xform_pos(invT_k, x_p));  n_h = normalize(xform_vec(T'_k, xform_vec(invT_k, n_p)))
  xform_pos(c, a).x = ((c0 a.x + c1 a.y) + c2 a.z) + c3 * 1.0f   (rows 1, 2 alike);  xform_vec: c3 * 0.0f
  normalize(v) = v * (1.0f / sqrtf((v.x v.x + v.y v.y) + v.z v.z))
  carried = rt_reproject's conditions on (x_h, n_h, t_p) && inst'_q == inst_p

all f32, one rounding per operation.  A G-buffer is reproject_ref's dict plus inst (i32 (H, W), -1: no instance); a transform table is a
dict T, invT of (n, 12) f32 arrays (rows 0..2 of the row-major 4 x 4 matrices; n may be 0), or None for a scene without a TLAS."""
from unittest import mock

import numpy as np

import reproject_ref as ref

F32 = np.float32


def table(T=None, invT=None):
    """a transform table from (n, 12) or (n, 16) arrays (16: the 4 x 4 matrices, whose first 12 floats are rows 0..2)"""
    T = np.zeros((0, 12), F32) if T is None else np.asarray(T, F32).reshape(len(T), -1)[:, :12]
    invT = np.zeros((0, 12), F32) if invT is None else np.asarray(invT, F32).reshape(len(invT), -1)[:, :12]
    return dict(T=np.ascontiguousarray(T), invT=np.ascontiguousarray(invT))


def moved(cur_xf, hist_xf):
    """per instance: does any of its 24 words differ bitwise from the capture's?"""
    if cur_xf is None or hist_xf is None:
        return np.zeros(0, bool)
    a = np.concatenate([cur_xf["T"], cur_xf["invT"]], 1).view(np.uint32)
    b = np.concatenate([hist_xf["T"], hist_xf["invT"]], 1).view(np.uint32)
    return (a != b).any(1)


def _xform(c, a, w):
    """xform_pos (w = 1) / xform_vec (w = 0): c (..., 12), a a tuple of three (...) arrays"""
    out = []
    with np.errstate(all="ignore"):
        for r in range(3):
            s = ((c[..., 4 * r] * a[0]).astype(F32) + (c[..., 4 * r + 1] * a[1]).astype(F32)).astype(F32)
            s = (s + (c[..., 4 * r + 2] * a[2]).astype(F32)).astype(F32)
            out.append((s + (c[..., 4 * r + 3] * F32(w)).astype(F32)).astype(F32))
    return tuple(out)


def _normalize(v):
    with np.errstate(all="ignore"):
        d = (((v[0] * v[0]).astype(F32) + (v[1] * v[1]).astype(F32)).astype(F32) + (v[2] * v[2]).astype(F32)).astype(F32)
        inv = (F32(1) / np.sqrt(d).astype(F32)).astype(F32)
        return tuple((x * inv).astype(F32) for x in v)


def take_back(cur, cur_xf, hist_xf, wrong_normal=False):
    """the current G-buffer with pos and normal as the capture saw them (x_h, n_h); wrong_normal: n_h = n_p even where the instance
    moved (what a gather that forgot the normal would do: the CPU tier shows the tests can tell)"""
    inst = np.asarray(cur["inst"], np.int32)
    mv = moved(cur_xf, hist_xf)
    k = np.where(inst >= 0, inst, 0)
    on = (inst >= 0) & (mv[np.minimum(k, len(mv) - 1)] if len(mv) else np.zeros(inst.shape, bool))
    pos, nrm = np.asarray(cur["pos"], F32), np.asarray(cur["normal"], F32)
    out = dict(cur)
    if not on.any():
        return out
    invT, Tc = cur_xf["invT"][k], hist_xf["T"][k]
    x = _xform(Tc, _xform(invT, ref._c(pos), 1), 1)
    n = _normalize(_xform(Tc, _xform(invT, ref._c(nrm), 0), 0))
    out["pos"] = np.where(on[..., None], np.stack(x, -1), pos).astype(F32)
    if not wrong_normal:
        out["normal"] = np.where(on[..., None], np.stack(n, -1), nrm).astype(F32)
    return out


def source(cur, hist, hist_count, hist_camera, cur_xf, hist_xf, mat_type, mat_shinieness, wrong_normal=False, **params):
    """(src, eligible) as reproject_ref.source, under rt_reproject_motion's definition"""
    P = dict(ref.DEFAULTS, **params)
    back = take_back(cur, cur_xf, hist_xf, wrong_normal)
    src, el = ref.source(back, hist, hist_count, hist_camera, mat_type, mat_shinieness, **P)
    q = np.where(src >= 0, src, 0)
    same = np.asarray(hist["inst"], np.int32).reshape(-1)[q] == np.asarray(cur["inst"], np.int32)
    return np.where(same, src, -1), el


def reproject(cur, hist, hist_acc, hist_count, hist_sum_y, hist_sum_yy, hist_camera, cur_xf, hist_xf, mat_type, mat_shinieness, wrong_normal=False, **params):
    """rt_reproject_motion: (acc, count, sum_y, sum_yy, n_carried, src, eligible) as reproject_ref.reproject, whose gather and
    max_history rescale this runs on the sources chosen above"""
    P = dict(ref.DEFAULTS, **params)
    chosen = source(cur, hist, hist_count, hist_camera, cur_xf, hist_xf, mat_type, mat_shinieness, wrong_normal, **P)
    # reproject_ref.reproject calls the module-level name 'source' once, first thing, and does the gather and the rescale on what it returns; it
    # is reused here, not copied, by handing it the sources chosen above.  The patch lasts for this one call, which is synchronous and calls
    # nothing of this module; tests/test_reproject_motion_cpu.py's unmoved case (bit-equal to the unpatched function) fails if that ever changes.
    with mock.patch.object(ref, "source", lambda *a, **k: chosen):
        return ref.reproject(cur, hist, hist_acc, hist_count, hist_sum_y, hist_sum_yy, hist_camera, mat_type, mat_shinieness, **P)
