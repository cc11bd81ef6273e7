"""numpy restatement of rt_reproject_deform (include/rt_amd.h): rt_reproject_motion with the point of a DEFORMED triangle's pixel taken back
through its barycentric coordinates first.  Built on tests/reproject_motion_ref.py (the motion's way back, the instance test) and, through
it, tests/reproject_ref.py (the projection, the acceptance, the gather); this module adds what the header adds:

  k = inst_p;  s = prim_p;  R_s the current record at slot s, R'_s the capture's (the current one where the BLAS of s has no kept copy)
  deformed_p = s >= 0 && R_s is a triangle record && any of the 12 words v0, v1, v2, N of R_s differs BITWISE from R'_s
  !deformed_p:  x_h, n_h as rt_reproject_motion defines them
   deformed_p:  x_o = k >= 0 ? xform_pos(invT_k, x_p) : x_p
                e1 = v1 - v0;  e2 = v2 - v0;  w = x_o - v0
                d11 = dot(e1,e1); d12 = dot(e1,e2); d22 = dot(e2,e2); w1 = dot(w,e1); w2 = dot(w,e2)
                den = d11 d22 - d12 d12;  bu = (d22 w1 - d12 w2) / den;  bv = (d11 w2 - d12 w1) / den
                x_o' = (v0' + bu e1') + bv e2'
                x_h = k >= 0 ? xform_pos(T'_k, x_o') : x_o';  n_h = k >= 0 ? normalize(xform_vec(T'_k, N')) : N'

all f32, one rounding per operation.  A G-buffer is reproject_motion_ref's dict plus prim (i32 (H, W), -1: no record); the records are
(slots, 16) f32 arrays as rt_blas_array(..., RT_LAYOUT_PRIMS) returns them, all BLASes in order: {v0, N.x} {v1, N.y} {v2, N.z}
{d, obj, mat, kind | flags}."""
from unittest import mock

import numpy as np

import reproject_motion_ref as rm
import reproject_ref as ref

F32 = np.float32
RT_KIND_TRI = 0


def capture_records(cur, captured, kept_slots):
    """R' for every slot: the records downloaded at the capture where the slot's BLAS has been rewritten since (kept_slots: a bool per
    slot), the current ones elsewhere -- a BLAS nothing rewrote has no kept copy, and its current records are the capture's"""
    cur, captured = np.asarray(cur, F32).reshape(-1, 16), np.asarray(captured, F32).reshape(-1, 16)
    return np.where(np.asarray(kept_slots, bool)[:, None], captured, cur).astype(F32)


def deformed_slots(cur_prims, cap_prims):
    """per slot: a triangle record one of whose 12 words differs bitwise from the capture's"""
    a = np.ascontiguousarray(cur_prims, F32).reshape(-1, 16).view(np.uint32)
    b = np.ascontiguousarray(cap_prims, F32).reshape(-1, 16).view(np.uint32)
    return ((a[:, 15] & 3) == RT_KIND_TRI) & (a[:, :12] != b[:, :12]).any(1)


def barycentric(x, v0, v1, v2):
    """(bu, bv) of the point x (a tuple of three arrays) in the triangle v0 v1 v2, as the definition computes them"""
    with np.errstate(all="ignore"):
        e1, e2, w = ref.sub(v1, v0), ref.sub(v2, v0), ref.sub(x, v0)
        d11, d12, d22, w1, w2 = ref.dot(e1, e1), ref.dot(e1, e2), ref.dot(e2, e2), ref.dot(w, e1), ref.dot(w, e2)
        den = ((d11 * d22).astype(F32) - (d12 * d12).astype(F32)).astype(F32)
        bu = (((d22 * w1).astype(F32) - (d12 * w2).astype(F32)).astype(F32) / den).astype(F32)
        bv = (((d11 * w2).astype(F32) - (d12 * w1).astype(F32)).astype(F32) / den).astype(F32)
    return bu, bv


def at(bu, bv, v0, v1, v2):
    """(v0 + bu e1) + bv e2 per component"""
    with np.errstate(all="ignore"):
        e1, e2 = ref.sub(v1, v0), ref.sub(v2, v0)
        return tuple(((a + (bu * b).astype(F32)).astype(F32) + (bv * c).astype(F32)).astype(F32) for a, b, c in zip(v0, e1, e2))


def _verts(rec):
    """v0, v1, v2, N of (..., 16) records as tuples of three arrays"""
    return tuple(tuple(rec[..., 4 * j + c] for c in range(3)) for j in range(3)) + ((rec[..., 3], rec[..., 7], rec[..., 11]),)


def take_back(cur, cur_xf, hist_xf, cur_prims, cap_prims):
    """(the current G-buffer with pos and normal as the capture saw them, the mask of the pixels that went through the barycentric path)"""
    back = rm.take_back(cur, cur_xf, hist_xf)
    cur_prims, cap_prims = np.asarray(cur_prims, F32).reshape(-1, 16), np.asarray(cap_prims, F32).reshape(-1, 16)
    prim, inst = np.asarray(cur["prim"], np.int32), np.asarray(cur["inst"], np.int32)
    if len(cur_prims) == 0:
        return back, np.zeros(prim.shape, bool)
    s = np.where(prim >= 0, prim, 0)
    on = (prim >= 0) & deformed_slots(cur_prims, cap_prims)[s]
    if not on.any():
        return back, on
    pos, nrm = np.asarray(cur["pos"], F32), np.asarray(cur["normal"], F32)
    under = inst >= 0
    k = np.where(under, inst, 0)
    x = ref._c(pos)
    if under.any():
        xo = rm._xform(cur_xf["invT"][k], x, 1)
        x = tuple(np.where(under, a, b).astype(F32) for a, b in zip(xo, x))
    v0, v1, v2, _ = _verts(cur_prims[s])
    h0, h1, h2, N = _verts(cap_prims[s])
    bu, bv = barycentric(x, v0, v1, v2)
    xh, nh = at(bu, bv, h0, h1, h2), N
    if under.any():
        Tc = hist_xf["T"][k]
        xw, nw = rm._xform(Tc, xh, 1), rm._normalize(rm._xform(Tc, N, 0))
        xh = tuple(np.where(under, a, b).astype(F32) for a, b in zip(xw, xh))
        nh = tuple(np.where(under, a, b).astype(F32) for a, b in zip(nw, nh))
    out = dict(back)
    out["pos"] = np.where(on[..., None], np.stack(xh, -1), np.asarray(back["pos"], F32)).astype(F32)
    out["normal"] = np.where(on[..., None], np.stack(nh, -1), np.asarray(back["normal"], F32)).astype(F32)
    return out, on


def source(cur, hist, hist_count, hist_camera, cur_xf, hist_xf, cur_prims, cap_prims, mat_type, mat_shinieness, **params):
    """(src, eligible, deformed) under rt_reproject_deform's definition"""
    P = dict(ref.DEFAULTS, **params)
    back, on = take_back(cur, cur_xf, hist_xf, cur_prims, cap_prims)
    src, el = ref.source(back, hist, hist_count, hist_camera, mat_type, mat_shinieness, **P)
    q = np.where(src >= 0, src, 0)
    same = np.asarray(hist["inst"], np.int32).reshape(-1)[q] == np.asarray(cur["inst"], np.int32)
    return np.where(same, src, -1), el, on


def reproject(cur, hist, hist_acc, hist_count, hist_sum_y, hist_sum_yy, hist_camera, cur_xf, hist_xf, cur_prims, cap_prims, mat_type, mat_shinieness, **params):
    """rt_reproject_deform: (acc, count, sum_y, sum_yy, n_carried, src, eligible, deformed); the gather and the max_history rescale are
    reproject_ref.reproject's, run on the sources chosen above (as reproject_motion_ref.reproject does, and for its reason)"""
    P = dict(ref.DEFAULTS, **params)
    src, el, on = source(cur, hist, hist_count, hist_camera, cur_xf, hist_xf, cur_prims, cap_prims, mat_type, mat_shinieness, **P)
    with mock.patch.object(ref, "source", lambda *a, **k: (src, el)):
        return ref.reproject(cur, hist, hist_acc, hist_count, hist_sum_y, hist_sum_yy, hist_camera, mat_type, mat_shinieness, **P) + (on,)
