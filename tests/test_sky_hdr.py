"""The host's Radiance .hdr -> 8-bit skydome loader (Scene::LoadSkyHDR, the stbi_load(..., 3) call of
template/scene.h:792) against the reference's OWN vendored stb_image.h, built from where it lies
(oracle/ref -> oracle/_ref/libstb_ref.so).  This is the one input of the path for which the real
reference code builds in this image without stand-ins, so here parity is pinned, bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libstb_ref.so")


def stb_load(path):
    L = C.CDLL(REF_SO)
    L.ref_stbi_load.restype = C.POINTER(C.c_ubyte)
    w, h, n = C.c_int(), C.c_int(), C.c_int()
    p = L.ref_stbi_load(path.encode(), C.byref(w), C.byref(h), C.byref(n), 3)
    assert p, "stb_image could not load " + path
    out = np.ctypeslib.as_array(p, shape=(h.value, w.value, 3)).copy()
    L.ref_stbi_free(p)
    return out, n.value


# stbi_load's answers for the test's files, recorded with the library above (tests/golden/make_sky_hdr_golden.py): the files'
# bytes, the 8-bit RGB and the component count.  The pin holds without the library; where it is built, it is checked live too.
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "sky_hdr_stb.npz"))


@pytest.mark.parametrize("w,h,rle", [(256, 128, True), (256, 128, False), (64, 33, True), (7, 5, True), (9, 3, False)])
def test_hdr_loader_matches_reference_stb_image(w, h, rle, tmp_path, host_api):
    key = "%dx%d_%s" % (w, h, "rle" if rle else "flat")
    path = str(tmp_path / "sky.hdr")
    with open(path, "wb") as f:
        f.write(GOLD[key + "_file"].tobytes())
    ref, comps = GOLD[key + "_rgb"], int(GOLD[key + "_n"])
    if os.path.exists(REF_SO):
        live, live_comps = stb_load(path)
        assert live_comps == comps and np.array_equal(live, ref)
    s = host_api.HostScene()
    got = s.sky_hdr(path)
    assert comps == 3 and got.shape == ref.shape == (h, w, 3)
    assert np.array_equal(got, ref)
    if w >= 64:
        assert len(np.unique(ref)) > 20 and ref.max() == 255 and ref.min() == 0  # the image exercises the range
    s.close()


def test_hdr_loader_rejects_bad_files(tmp_path, host_api):
    s = host_api.HostScene()
    bad = tmp_path / "bad.hdr"
    bad.write_bytes(b"P6\n1 1\n255\n\0\0\0")
    with pytest.raises(RuntimeError, match="Radiance"):
        s.sky_hdr(str(bad))
    trunc = tmp_path / "trunc.hdr"
    trunc.write_bytes(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 4 +X 16\n\2\2\0\20\x90")
    with pytest.raises(RuntimeError):
        s.sky_hdr(str(trunc))
    with pytest.raises(RuntimeError, match="open"):
        s.sky_hdr(str(tmp_path / "missing.hdr"))
    s.close()
