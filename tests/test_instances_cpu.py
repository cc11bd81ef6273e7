"""CPU tier for rt_set_instances (include/rt_amd.h): the rules the device follows, restated in tests/instances_ref.py and held against the
host mirror; the numbering of tlas::build's nodes that the device's commit relies on (csrc/rt_instances.h, fact 1); and the guard of the
refactor that made pack_reach's per-instance part a function (csrc/rt_layout.h instance_reach)."""
import hashlib

import numpy as np
import pytest

import instances_ref as ir

f32 = np.float32


def _local_box(scene, blas):
    nodes = scene.bvh_dump(blas)["nodes"]
    return np.concatenate([nodes[0, 0:3], nodes[0, 4:7]]).view(f32)


@pytest.mark.parametrize("mesh", ["triangles", "lowBigB"])
def test_fresh_bounds_rule_equals_the_host_mirror(mesh, host_api, scenes):
    """bvhInstance(blas) + one SetTransform on the host mirror leaves exactly instances_ref.fresh_bounds(local box, T): identity, a TRS with
    rotations about all three axes, and a negative scale."""
    h = host_api.HostScene()
    Ts = [np.eye(4, dtype=f32).reshape(16), h.trs((1.5, -0.25, 3.0), 2.5, 0.3, 1.1, -0.7), h.trs((-2.0, 0.5, 1.0), -1.5, 0.0, 0.4, 0.0)]
    if mesh == "triangles":
        ir.triangles_scene(h, Ts)
    else:
        assets = __import__("importlib").import_module("ray-and-pathtracer_amd.assets")
        m = h.mesh_obj(1, assets.obj_path("lowBigB"), h.diffuse(0.8, (1, 0, 0)), (0, 0.5, 0), 1)
        h.build_tlas(0, [(m, T) for T in Ts])
    for i, T in enumerate(Ts):
        d = h.instance_dump(i)
        want = ir.fresh_bounds(_local_box(h, d["blas"]), T)
        assert np.array_equal(d["bounds"].view(np.uint32), want.view(np.uint32)), (mesh, i)
        assert np.all(want[:3] <= _local_box(h, d["blas"])[:3]) and np.all(want[3:] >= _local_box(h, d["blas"])[3:])  # the union with the local box
    assert not np.array_equal(h.instance_dump(1)["bounds"], h.instance_dump(0)["bounds"])
    h.close()


def _random_transforms(h, n, seed):
    rng = np.random.default_rng(seed)
    Ts = [h.trs(tuple(rng.uniform(-20, 20, 3)), float(rng.uniform(0.2, 5)), *[float(a) for a in rng.uniform(-3, 3, 3)]) for _ in range(n)]
    if n >= 3:
        Ts[n - 1] = Ts[0].copy()  # two identical boxes: a tie in FindBestMatch
    return Ts


@pytest.mark.parametrize("n", [1, 2, 3, 8, 17])
def test_tlas_build_numbering_does_not_depend_on_the_boxes(n, host_api):
    """tlas::build through the host mirror over random finite boxes (two of them identical from n = 3 on): leaves 1..n, inner nodes
    n+1..2n-1 with their children below them, node 0 the last node; and so the layout has n TLAS pair records, none at n = 1."""
    for seed in (1, 2):
        h = host_api.HostScene()
        ir.triangles_scene(h, _random_transforms(h, n, 10 * n + seed), two_meshes=False)
        nodes = h.tlas_dump()
        b6 = np.stack([h.instance_dump(i)["bounds"] for i in range(n)])
        if n >= 3:
            assert np.array_equal(b6[0], b6[n - 1])
        ir.check_numbering(nodes, n)
        assert np.array_equal(nodes, ir.tlas_build(b6)), "instances_ref.tlas_build restates the host mirror's tlas::build"
        L = host_api.layout(h.describe())
        assert L["tlasPairs"] == (n if n >= 2 else 0) and L["nInst"] == n
        assert L["root"] == (0x40000000 if n == 1 else L["tlasBase"]) and L["tlasBase"] == (len(L["pairs"]) // 16 - n if n >= 2 else 0)
        assert len(L["reach"]) == L["tlasPairs"] * 12 + 16
        h.close()


def test_lds_split_sides():
    n = ir.smallest_n_without_lds()
    assert ir.lds_rows(n - 1, n - 1) >= ir.ROWS_MIN > ir.lds_rows(n, n) and n == 38


def test_layout_bytes_equal_the_parent_commit(host_api, scenes):
    """rt_layout_build of tlas_test2 and pretty_tlas (8) gives the bytes of the commit before pack_reach's loop body became a function.  The
    table below is the first 16 hex digits of sha256(array.tobytes()) of every array of host_api.layout(scene.describe(), *knobs),
    knobs = (RT_WIDE, RT_WIDE8, RT_TLAS_LDS); it was printed by that loop run on a build of the PARENT commit's sources (before
    csrc/rt_layout.h was touched), never by the code under test.  (tests/test_layout_cpu.py::test_layout_equals_parent guards the same
    bytes against the commit before that one, for every scene.)

    scene       knobs   array           sha256[:16]
    tlas_test2  -1,0,1  pairs           9d5c83b2b0a03fd6
    tlas_test2  -1,0,1  prims           76fb6a11e118f47d
    tlas_test2  -1,0,1  wide            e3b0c44298fc1c14
    tlas_test2  -1,0,1  wide8           e3b0c44298fc1c14
    tlas_test2  -1,0,1  leafBox         e3b0c44298fc1c14
    tlas_test2  -1,0,1  reach           f29794b508da31c6
    tlas_test2  -1,0,1  brute           6bb51fd31c31a267
    tlas_test2  -1,0,1  inst            204f7860c6e38cad
    tlas_test2  -1,0,1  lights          309032110a95ae63
    tlas_test2  -1,0,1  mats            0fc493878ee8f042
    tlas_test2  -1,0,1  refitOrder      e3b0c44298fc1c14
    tlas_test2  -1,0,1  refitLevelStart e3b0c44298fc1c14
    tlas_test2  -1,0,1  rootLink        67abdd721024f0ff
    tlas_test2  -1,0,1  rootWide        df3f619804a92fdb
    tlas_test2  -1,0,1  rootWide8       df3f619804a92fdb
    tlas_test2  -1,0,1  scalars         fb9a1ff597d02ed3
    tlas_test2  1,1,0   pairs           9d5c83b2b0a03fd6
    tlas_test2  1,1,0   prims           76fb6a11e118f47d
    tlas_test2  1,1,0   wide            69e76d2b3c22fac3
    tlas_test2  1,1,0   wide8           f93cae9b5a17ae04
    tlas_test2  1,1,0   leafBox         05e3696fcc014294
    tlas_test2  1,1,0   reach           f29794b508da31c6
    tlas_test2  1,1,0   brute           6bb51fd31c31a267
    tlas_test2  1,1,0   inst            933d7b27bb68ae6e
    tlas_test2  1,1,0   lights          309032110a95ae63
    tlas_test2  1,1,0   mats            0fc493878ee8f042
    tlas_test2  1,1,0   refitOrder      e3b0c44298fc1c14
    tlas_test2  1,1,0   refitLevelStart e3b0c44298fc1c14
    tlas_test2  1,1,0   rootLink        67abdd721024f0ff
    tlas_test2  1,1,0   rootWide        df3f619804a92fdb
    tlas_test2  1,1,0   rootWide8       df3f619804a92fdb
    tlas_test2  1,1,0   scalars         256d5e1b42f66b4f
    pretty_tlas -1,0,1  pairs           5b9b2590cc86c941
    pretty_tlas -1,0,1  prims           b427f72ebf3f7368
    pretty_tlas -1,0,1  wide            e3b0c44298fc1c14
    pretty_tlas -1,0,1  wide8           e3b0c44298fc1c14
    pretty_tlas -1,0,1  leafBox         e3b0c44298fc1c14
    pretty_tlas -1,0,1  reach           2dc080b88c4fecc7
    pretty_tlas -1,0,1  brute           98424963f43ba53a
    pretty_tlas -1,0,1  inst            b67499f9388ab26e
    pretty_tlas -1,0,1  lights          7aaeb70f8e34c211
    pretty_tlas -1,0,1  mats            7c7996873b342f2e
    pretty_tlas -1,0,1  refitOrder      e3b0c44298fc1c14
    pretty_tlas -1,0,1  refitLevelStart e3b0c44298fc1c14
    pretty_tlas -1,0,1  rootLink        df0e1081279154e3
    pretty_tlas -1,0,1  rootWide        af5570f5a1810b7a
    pretty_tlas -1,0,1  rootWide8       af5570f5a1810b7a
    pretty_tlas -1,0,1  scalars         f8ec816f02189bdc
    pretty_tlas 1,1,0   pairs           5b9b2590cc86c941
    pretty_tlas 1,1,0   prims           b427f72ebf3f7368
    pretty_tlas 1,1,0   wide            127a28512d1a107a
    pretty_tlas 1,1,0   wide8           d454d1be4d53e72a
    pretty_tlas 1,1,0   leafBox         6134348f1be7c67f
    pretty_tlas 1,1,0   reach           2dc080b88c4fecc7
    pretty_tlas 1,1,0   brute           98424963f43ba53a
    pretty_tlas 1,1,0   inst            8abc4c6ae690c6f9
    pretty_tlas 1,1,0   lights          7aaeb70f8e34c211
    pretty_tlas 1,1,0   mats            7c7996873b342f2e
    pretty_tlas 1,1,0   refitOrder      e3b0c44298fc1c14
    pretty_tlas 1,1,0   refitLevelStart e3b0c44298fc1c14
    pretty_tlas 1,1,0   rootLink        df0e1081279154e3
    pretty_tlas 1,1,0   rootWide        9f5bbdadc1df4b9f
    pretty_tlas 1,1,0   rootWide8       0f4a0f679e3f8e84
    pretty_tlas 1,1,0   scalars         1db070d70fd5e078
    """
    want = {}
    for line in test_layout_bytes_equal_the_parent_commit.__doc__.splitlines():
        w = line.split()
        if len(w) == 4 and len(w[3]) == 16 and w[0] in ("tlas_test2", "pretty_tlas"):
            want[(w[0], w[1], w[2])] = w[3]
    assert len(want) == 2 * 2 * len(host_api.LAYOUT_ARRAYS)
    for name, kw in (("tlas_test2", {}), ("pretty_tlas", {"n_instances": 8})):
        for knobs in ((-1, 0, 1), (1, 1, 0)):
            h = host_api.HostScene()
            scenes.REGISTRY[name](h, **kw)
            L = host_api.layout(h.describe(), *knobs)
            for arr, _ in host_api.LAYOUT_ARRAYS:
                assert hashlib.sha256(L[arr].tobytes()).hexdigest()[:16] == want[(name, "%d,%d,%d" % knobs, arr)], (name, knobs, arr)
            h.close()
