"""Writes tests/golden/ref_leaf.npz: the inputs of tests/ref_leaf_cases.py and what the REFERENCE'S OWN COMPILED CODE answers to them
(oracle/ref/ref_leaf.cpp -> oracle/_ref/libref_leaf.so, built by oracle/ref/Makefile where the reference's sources are present), all
floats as raw bits.  The file is data the reference's code wrote while it ran; it holds no program text.

Three builds of the same harness are run:
  libref_leaf.so       -O2, the float transcendentals bound to the project's definition (f64, rounded once)   -- the record
  libref_leaf_O0.so    -O0, otherwise the same -- must answer bit for bit like the first (checked here; this replaces the two-compiler check
                       of the oracle's own vectors, since g++ cannot parse the reference's headers)
  libref_leaf_libm.so  -O2 with libm's float transcendentals -- information only: how many answers the definition moves
The one place the two optimisation levels may differ is Triangle::IsOccluding where it runs off its end without a return statement
(template/scene.h:236-237: the edge tests pass, t is outside the range): those cases are found here from the reference alone -- the two builds
disagree, or IsOccluding says true where Intersect missed -- and recorded as tri_occ_undefined.

Run from the repository root:  python tests/golden/make_ref_leaf_golden.py"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_leaf_cases as rc  # noqa: E402


def main():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle", "ref"), "-s"])
    ref = os.path.join(ROOT, "oracle", "_ref")
    cs = rc.all_cases()
    A = {k: rc.answers(C.CDLL(os.path.join(ref, f)), "ref_", cs) for k, f in (("O2", "libref_leaf.so"), ("O0", "libref_leaf_O0.so"), ("libm", "libref_leaf_libm.so"))}
    undefined = (A["O2"]["tri_occ"] != A["O0"]["tri_occ"]) | (A["O2"]["tri_occ"] & ~A["O2"]["tri_hit"]) | (A["O0"]["tri_occ"] & ~A["O0"]["tri_hit"])
    print("-O0 against -O2, answers that differ:")
    total = 0
    for k in A["O2"]:
        d = ~rc.same_bits(A["O2"][k], A["O0"][k])
        if k == "tri_occ":
            d &= ~undefined
        total += int(d.sum())
        print("  %-16s %6d of %6d" % (k, d.sum(), d.size))
    print("  Triangle::IsOccluding ran off its end in %d of %d cases (%.2f %%): recorded as undefined" % (undefined.sum(), undefined.size, 100 * undefined.mean()))
    assert total == 0, "the reference's answers depend on the optimisation level"
    print("libm's float transcendentals against the f64-rounded-once definition, answers that differ (information only):")
    for k in A["O2"]:
        d = ~rc.same_bits(A["O2"][k], A["libm"][k])
        if d.any():
            print("  %-16s %6d of %6d" % (k, d.sum(), d.size))
    out = {k: rc.bits(v) for k, v in rc.flat_inputs(cs).items()}
    out.update({"out_" + k: rc.bits(v) for k, v in A["O2"].items()})
    out["out_tri_occ"] = A["O2"]["tri_occ"] & ~undefined
    out["out_tri_occ_undefined"] = undefined
    path = os.path.join(HERE, "ref_leaf.npz")
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes" % (os.path.relpath(path, ROOT), len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
