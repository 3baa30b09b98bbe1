"""-m gpu: mutation tests of the parity suite (trap A2 / A4).

The HIP library is rebuilt with one deliberate indexing bug at a time (tests/mutation.py,
-DCELESTE_MUTANT=k in csrc/elbo_kernels.h): iota read by column instead of by row, the sky plane read transposed,
one star stamp for every patch.  On the variable-field golden (varying sky plane, per-row calibration, per-patch
stamps: tests/golden/field_72x88_9src_variable.npz) every mutant must break parity with the committed oracle
outputs; on a constant-template golden the first two cannot be seen at all -- which is exactly why round 1's
fixtures, all constant, did not cover the trap."""
import os
import sys

import pytest

from mutation import ROOT, SUITES, run_child

pytestmark = pytest.mark.gpu
SUITE = SUITES["engine"]

CHECK = r"""
import json, sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import golden_util as gu
from parity_util import RTOL, rel_err, fp32_errors, norm_scaled_fp32_errors, FP32_T_V, FP32_T_D, FP32_T_H
import celeste_jl_amd as cel
z = np.load(gu.path(sys.argv[1]))
# fp32 criterion: "norm" = the mode's stated 1e-4, norm-scaled (SURVEY.md 8(d) config 5); "entry" = parity_util's entry-wise
# criterion; "both"; "fp64" = the fp64 launches only
mode = sys.argv[2] if len(sys.argv) > 2 else "both"
f = gu.arrays_to_field(z)
ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
tg = list(range(len(f.catalog)))
ref = (z["v7"], z["d7"], z["h7"])
worst, report = 0.0, {}
def count(e, tol):      # a NaN error fails (Python's max() would skip it)
    global worst
    worst = max(worst, e / tol) if np.isfinite(e) else np.inf
for flags in ((7, 7 | 16) if mode == "fp64" else (7, 7 | 16, 7 | 8, 5 | 8, 7 | 8 | 16)):
    v, d, h, cnt, st = ctx.eval_batch(f.vp, tg, flags)
    if flags & 8:   # fp32 component loop
        e = norm_scaled_fp32_errors((v, d, h), ref)
        report["norm %%d" %% flags] = e
        if mode in ("norm", "both"):
            for x in e.values():
                count(x, 1e-4)
        # ("entry" alone is the entry-wise criterion by itself, to show what it catches; it is meant to be used with "norm":
        # its Hessian threshold is loose on the largest entries, parity_util.py)
        x = fp32_errors((v, d, h), ref, z["h7"])
        ex = {k: float(x[k].max()) for k in x if x[k] is not None}
        report["entry %%d" %% flags] = ex
        if mode in ("entry", "both"):
            for k, tol in (("v", FP32_T_V), ("d", FP32_T_D), ("h", FP32_T_H)):
                if k in ex:
                    count(ex[k], tol)
    else:
        e = [float(np.max(np.abs(v - z["v7"]) / np.abs(z["v7"])))] + [rel_err(d[t], z["d7"][t]) for t in tg] + \
            [rel_err(h[t], z["h7"][t]) for t in tg]
        report["fp64 %%d" %% flags] = max(e) if np.isfinite(e).all() else float("inf")
        for x in e:
            count(x, RTOL)
print("worst error / tolerance: %%.3g" %% worst)
print("REPORT " + json.dumps(report))   # (inf prints as Infinity, which json.loads reads back)
sys.exit(0 if worst <= 1.0 else 3)
"""


def _parity(lib_path, case, mode="both"):
    """CHECK in a child (tests/mutation.py's runner: exit status 0 or 3, anything else stops every later child)"""
    status, text = run_child([sys.executable, "-c", CHECK % {"root": ROOT}, case, mode], SUITE,
                             lib_path, "%s %s %s" % (os.path.basename(lib_path or "product"), case, mode), normal=(0, 3), timeout=600)
    return status == 0, text.strip()


@pytest.fixture(scope="module")
def mutants():
    libs = SUITE.build()
    return [libs["engine", macro, k] for macro, k, _ in SUITE.mutants]


def test_product_library_holds_parity_on_both_goldens():
    for case in ("field_72x88_9src_variable", "field_64x80_8src_nan"):
        ok, msg = _parity(None, case)
        assert ok, (case, msg)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_mutant_is_caught_by_the_variable_field(mutants, k):
    ok, msg = _parity(mutants[k], "field_72x88_9src_variable")
    print(os.path.basename(mutants[k]), "on the variable field:", msg)
    assert not ok, "the mutated kernel still passes parity: the fixture has no power against this bug"


@pytest.mark.parametrize("k", [0, 1])
def test_constant_template_fixtures_cannot_see_plane_indexing_bugs(mutants, k):
    """documentation of the round-1 hole: with one sky and one calibration per band, iota[w] == iota[h] and
    sky[w, h] == sky[h, w]"""
    ok, msg = _parity(mutants[k], "field_64x80_8src_nan")
    print(os.path.basename(mutants[k]), "on the constant template:", msg)
    assert ok


# Mutants in code only the single-precision mode runs (CELESTE_MUTANT 4 .. 7: galaxy_sums_px2's Hessian and gradient modes,
# the neighbours' float light, galaxy_sums_pk of the fp32 split variant).  Indices into the `mutants` fixture.  Before this
# check no test ran the gradient-only or split fp32 launches on a golden, so 5 and 7 went unseen; on these goldens the old
# norm-scaled criterion flags all four too once those launches run (profiles/fp32_entry_errors_mi355x.json, "mutants").
FP32_ONLY = [3, 4, 5, 6]
FP32_CASE = "field_72x88_9src_variable"


@pytest.mark.parametrize("k", FP32_ONLY)
def test_fp32_mutant_is_caught_by_the_entry_wise_criterion(mutants, k):
    ok, msg = _parity(mutants[k], FP32_CASE, "entry")
    print(os.path.basename(mutants[k]), "entry-wise:", msg)
    assert not ok, "the mutated single-precision kernel still passes the entry-wise fp32 criterion"


@pytest.mark.parametrize("k", FP32_ONLY)
def test_fp32_mutant_holds_fp64_parity(mutants, k):
    """the mutation sits in single-precision code only: the fp64 launches are untouched"""
    ok, msg = _parity(mutants[k], FP32_CASE, "fp64")
    assert ok, (os.path.basename(mutants[k]), msg)

