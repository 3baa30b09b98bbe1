"""Mutation tests of the fit, phot and mcmc libraries' parity suites (the engine's own are tests/test_mutants.py).

Each library is rebuilt with one deliberate bug at a time (tests/mutants/build_mutants.py: SATELLITE; the switches are
CELESTE_CLIENT_MUTANT in csrc/engine_client.h, CELESTE_FIT_MUTANT, CELESTE_PHOT_MUTANT and CELESTE_MCMC_MUTANT at the head of
each library's source), and the library's own parity tests -- those that compare the device with the numpy restatements -- run
against it in a child process, the mutant selected through CELESTE_MI355X_{FIT,PHOT,MCMC}_LIB.  A child that fails (exit status
1) has killed its mutant; one that passes shows a bug the suite cannot see.  Any other end of a child (a signal, its time limit,
pytest's statuses 2 to 5) is an error of the harness, not a kill: the test fails with the child's tail and nothing more is
started on the device.

The catalogue test (not -m gpu) keeps SATELLITE and the `<MACRO> == k` switches of the four sources in step.

With CELESTE_SATELLITE_REPORT=<file> every child's outcome, the test that failed in it and its wall time are appended to
<file>, one JSON object per line (profiles/satellite_mutants_mi355x.json is made of them)."""
import json
import os
import re
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "mutants"))
import build_mutants  # noqa: E402

CSRC = os.path.join(ROOT, "celeste.jl_amd", "csrc")
SOURCES = {"CELESTE_CLIENT_MUTANT": "engine_client.h", "CELESTE_FIT_MUTANT": "fit/celeste_fit.hip",
           "CELESTE_PHOT_MUTANT": "phot/celeste_phot.hip", "CELESTE_MCMC_MUTANT": "mcmc/celeste_mcmc.hip"}
# the parity tests of each library (not infer_box, not the refusals): what compares the device with a restatement, and the
# bit-for-bit comparisons of a library's two paths
SUITES = {
    "fit": ("CELESTE_MI355X_FIT_LIB", "tests/test_gpu_fit.py", "restatement or non_finite_row or multifield"),
    "phot": ("CELESTE_MI355X_PHOT_LIB", "tests/test_gpu_phot.py",
             "restatement or same_bits or capacity_of_lds or non_finite_row or multifield or max_iters"),
    "mcmc": ("CELESTE_MI355X_MCMC_LIB", "tests/test_gpu_mcmc.py", "restatement or replay"),
}
CHILD_TIMEOUT = 300        # seconds; a child needs a small fraction of it
_ABNORMAL = []             # the first child that ended with neither 0 nor 1: nothing is started after it


def _ident(entry):
    macro, k, name, lib = entry
    return "%s-%s-%d-%s" % (lib, macro.split("_")[1].lower(), k, name)


# ---- catalogue against sources (no GPU) --------------------------------------------------------------------------------------
def test_catalogue_and_sources_agree():
    """every `<MACRO> == k` of the four sources is in the catalogue and the reverse; names are unique per library; client
    mutants 1 to 6 go into fit, 1 and 2 into phot as well; each of the other macros goes into its own library"""
    in_source = set()
    for macro, rel in SOURCES.items():
        text = open(os.path.join(CSRC, rel)).read()
        found = {int(k) for k in re.findall(r"\b%s\s*==\s*(\d+)" % macro, text)}
        assert found and 0 not in found, (macro, found)
        in_source |= {(macro, k) for k in found}
        assert not any(other in text for other in SOURCES if other != macro), rel      # one macro per file
    cat = build_mutants.SATELLITE
    assert {(m, k) for m, k, _, _ in cat} == in_source
    assert len({(lib, name) for _, _, name, lib in cat}) == len(cat) == len({(m, k, lib) for m, k, _, lib in cat}) == 25
    assert len({build_mutants.satellite_path(e) for e in cat}) == 25
    libs = {}
    for m, k, _, lib in cat:
        libs.setdefault(m, set()).add((k, lib))
    assert libs["CELESTE_CLIENT_MUTANT"] == {(k, "fit") for k in range(1, 7)} | {(1, "phot"), (2, "phot")}
    for m, lib in (("CELESTE_FIT_MUTANT", "fit"), ("CELESTE_PHOT_MUTANT", "phot"), ("CELESTE_MCMC_MUTANT", "mcmc")):
        assert {l for _, l in libs[m]} == {lib}, m
    assert all(lib in SUITES for _, _, _, lib in cat)


# ---- the children ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mutants():
    return dict(zip(build_mutants.SATELLITE, build_mutants.build_satellite()))


def _child(lib, lib_path, what):
    """runs the library's parity tests in a child; (exit status, output, seconds).  Refuses once a child has ended abnormally."""
    if _ABNORMAL:
        pytest.fail("not started: an earlier child ended abnormally (%s)" % _ABNORMAL[0])
    var, path, select = SUITES[lib]
    env = dict(os.environ)
    env.pop(var, None)
    if lib_path:
        env[var] = lib_path
    cmd = [sys.executable, "-m", "pytest", path, "-q", "-x", "-p", "no:cacheprovider", "-k", select]
    t0 = time.time()
    try:
        out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        status, text = out.returncode, out.stdout + out.stderr
    except subprocess.TimeoutExpired as e:
        status = "time limit of %d s" % CHILD_TIMEOUT
        text = "".join(x.decode(errors="replace") if isinstance(x, bytes) else (x or "") for x in (e.stdout, e.stderr))
    dt = time.time() - t0
    failed = re.findall(r"^FAILED (\S+)", text, flags=re.M)
    report = os.environ.get("CELESTE_SATELLITE_REPORT")
    if report:
        with open(report, "a") as fh:
            fh.write(json.dumps({"what": what, "library": lib, "status": status, "failed": failed[:1], "seconds": round(dt, 2),
                                 "summary": text.strip().splitlines()[-1:]}) + "\n")
    print("%s: status %s in %.1f s%s" % (what, status, dt, (", failed " + failed[0]) if failed else ""))
    if status not in (0, 1):
        _ABNORMAL.append("%s: %s" % (what, status))
        pytest.fail("the child of %s ended with %s, neither passed nor failed:\n%s" % (what, status, text[-3000:]))
    return status, text, dt


@pytest.mark.gpu
@pytest.mark.parametrize("lib", sorted(SUITES))
def test_product_library_passes_the_selection(lib):
    status, text, _ = _child(lib, None, "product-" + lib)
    assert status == 0, text[-3000:]
    assert re.search(r"\b\d+ passed", text) and "skipped" not in text.splitlines()[-1], text[-500:]


@pytest.mark.gpu
@pytest.mark.parametrize("entry", build_mutants.SATELLITE, ids=_ident)
def test_mutant_is_killed_by_the_parity_tests(mutants, entry):
    status, text, _ = _child(entry[3], mutants[entry], _ident(entry))
    assert status == 1, "the mutated library still passes its parity tests: the fixture has no power against this bug"
