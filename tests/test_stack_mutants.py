"""Mutation tests of the stack's parity suite, after tests/test_resid_mutants.py.

The resid library is rebuilt with one deliberate bug of the stack at a time (-DCELESTE_STACK_MUTANT=k; the head of
csrc/resid/resid_stack.h lists them) into tests/mutants/ (git-ignored build artefacts), and the parity tests of
tests/test_gpu_stack.py -- those that compare the device with the numpy restatement, and culling off against on -- run against
it in a child process, the mutant selected through CELESTE_MI355X_RESID_LIB.  A child that fails (exit status 1) has killed its
mutant; one that passes shows a bug the suite cannot see.  Any other end of a child (a signal, its time limit, pytest's
statuses 2 to 5) is an error of the harness, not a kill: the test fails with the child's tail and nothing more is started on
the device.

The catalogue test (not -m gpu) keeps MUTANTS and the `CELESTE_STACK_MUTANT == k` switches of the header in step."""
import os
import re
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "celeste.jl_amd", "csrc", "resid")
SOURCE = os.path.join(DIR, "celeste_resid.hip")
HEADER = os.path.join(DIR, "resid_stack.h")
OUT = os.path.join(ROOT, "tests", "mutants")
MUTANTS = {1: "d_weighted_by_s", 2: "truncation_for_rint", 3: "gather_transposed", 4: "masked_pixel_not_skipped",
           5: "min_images_strict", 6: "cull_without_margin"}
# what compares the device with the restatement, and culling off against on
SELECT = "edge_scene_against or tan_scene_against or culling_changes"
CHILD_TIMEOUT = 300        # seconds; a child needs a small fraction of it
_ABNORMAL = []             # the first child that ended with neither 0 nor 1: nothing is started after it


def _path(k):
    return os.path.join(OUT, "libceleste_resid_stack_mutant_%d_%s.so" % (k, MUTANTS[k]))


def test_catalogue_and_header_agree():
    text = open(HEADER).read()
    found = {int(k) for k in re.findall(r"\bCELESTE_STACK_MUTANT\s*[!=]=\s*(\d+)", text)}
    assert found == set(MUTANTS) and 0 not in found
    head = text[:text.index("#ifndef CELESTE_STACK_MUTANT")]
    for k in MUTANTS:
        assert re.search(r"^//\s+%d = " % k, head, flags=re.M), k
    assert len(set(MUTANTS.values())) == len(MUTANTS) and "CELESTE_RESID_MUTANT ==" not in text
    assert "CELESTE_STACK_MUTANT" not in open(SOURCE).read()          # the library's own switches keep their numbers to themselves


@pytest.fixture(scope="module")
def mutants():
    """the mutated libraries: the library's own command line (the product's), one -D"""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    os.makedirs(OUT, exist_ok=True)
    newest = max(os.path.getmtime(s) for s in ge.sources("resid"))
    stale = [k for k in MUTANTS if not os.path.exists(_path(k)) or os.path.getmtime(_path(k)) < newest]
    cmds = [ge.compile_command("resid", out=_path(k), defines=["CELESTE_STACK_MUTANT=%d" % k]) for k in stale]
    procs = [subprocess.Popen(argv, cwd=cwd) for argv, cwd in cmds]
    if [p.wait() for p in procs].count(0) != len(procs):
        pytest.fail("a mutant did not build")
    return {k: _path(k) for k in MUTANTS}


def _child(lib_path, what):
    """runs the parity tests in a child; (exit status, output).  Refuses once a child has ended abnormally."""
    if _ABNORMAL:
        pytest.fail("not started: an earlier child ended abnormally (%s)" % _ABNORMAL[0])
    env = dict(os.environ)
    env.pop("CELESTE_MI355X_RESID_LIB", None)
    if lib_path:
        env["CELESTE_MI355X_RESID_LIB"] = lib_path
    cmd = [sys.executable, "-m", "pytest", "tests/test_gpu_stack.py", "-q", "-x", "-p", "no:cacheprovider", "-k", SELECT]
    t0 = time.time()
    try:
        out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        status, text = out.returncode, out.stdout + out.stderr
    except subprocess.TimeoutExpired as e:
        status = "time limit of %d s" % CHILD_TIMEOUT
        text = "".join(x.decode(errors="replace") if isinstance(x, bytes) else (x or "") for x in (e.stdout, e.stderr))
    failed = re.findall(r"^FAILED (\S+)", text, flags=re.M)
    print("%s: status %s in %.1f s%s" % (what, status, time.time() - t0, (", failed " + failed[0]) if failed else ""))
    if status not in (0, 1):
        _ABNORMAL.append("%s: %s" % (what, status))
        pytest.fail("the child of %s ended with %s, neither passed nor failed:\n%s" % (what, status, text[-3000:]))
    return status, text


@pytest.mark.gpu
def test_product_library_passes_the_selection():
    status, text = _child(None, "product")
    assert status == 0, text[-3000:]
    assert re.search(r"\b\d+ passed", text) and "skipped" not in text.splitlines()[-1], text[-500:]


@pytest.mark.gpu
@pytest.mark.parametrize("k", sorted(MUTANTS), ids=lambda k: "%d-%s" % (k, MUTANTS[k]))
def test_mutant_is_killed_by_the_parity_tests(mutants, k):
    status, text = _child(mutants[k], "mutant %d %s" % (k, MUTANTS[k]))
    assert status == 1, "the mutated library still passes its parity tests: the fixture has no power against this bug"
