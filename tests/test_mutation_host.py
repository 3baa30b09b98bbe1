"""tests/mutation.py's child runner and builder, driven with stand-in children that never touch a device; and its catalogue
against the sources, every macro of it."""
import json
import subprocess
import sys

import pytest

import mutation

STANDIN = mutation.Suite("standin", "standin", "CELESTE_STANDIN_LIB", [], None, {"CELESTE_STANDIN_MUTANT": {1: "a_bug"}})


def _py(code, *args):
    return [sys.executable, "-c", code] + list(args)


@pytest.fixture(autouse=True)
def fresh(monkeypatch):
    monkeypatch.setattr(mutation, "ABNORMAL", [])
    monkeypatch.delenv("CELESTE_MUTANT_REPORT", raising=False)
    monkeypatch.setenv(STANDIN.env, "/set/by/the/caller")      # the runner must not pass this on to a product child


def test_every_macro_agrees_with_the_sources():
    for macro in mutation.SOURCES:
        mutation.check_macro(macro)
    used = {m for s in mutation.SUITES.values() for m, _, _ in s.mutants}
    assert used == set(mutation.SOURCES) and sum(len(s.mutants) for s in mutation.SUITES.values()) == 87
    assert len({s.path(m, k) for s in mutation.SUITES.values() for m, k, _ in s.mutants}) == 87


def test_normal_statuses_come_back():
    assert mutation.run_child(_py("print('fine')"), STANDIN, None, "zero") == (0, "fine\n")
    status, text = mutation.run_child(_py("import sys; print('FAILED a::b - x'); sys.exit(1)"), STANDIN, None, "one")
    assert status == 1 and "FAILED a::b" in text
    assert mutation.run_child(_py("import sys; sys.exit(3)"), STANDIN, None, "three", normal=(0, 3))[0] == 3
    assert not mutation.ABNORMAL


@pytest.mark.parametrize("what, code, timeout, status", [
    ("exit 2", "import sys; print('the tail'); sys.exit(2)", 300, "2"),
    ("signal", "import os, signal; print('the tail', flush=True); os.kill(os.getpid(), signal.SIGKILL)", 300, "-9"),
    ("time limit", "import time; print('the tail', flush=True); time.sleep(60)", 1, "time limit of 1 s"),
])
def test_an_abnormal_end_fails_the_caller_and_refuses_every_later_child(tmp_path, what, code, timeout, status):
    with pytest.raises(pytest.fail.Exception) as first:
        mutation.run_child(_py(code), STANDIN, None, what, timeout=timeout)
    assert "the tail" in str(first.value) and "ended with %s," % status in str(first.value)
    marker = tmp_path / "started"
    other = mutation.Suite("other", "other", "CELESTE_OTHER_LIB", [], None, {"CELESTE_OTHER_MUTANT": {1: "a_bug"}})
    with pytest.raises(pytest.fail.Exception) as later:       # another suite's child: the latch is the module's
        mutation.run_child(_py("import sys; open(sys.argv[1], 'w')", str(marker)), other, None, "next")
    assert not marker.exists()
    assert "not started" in str(later.value) and "standin %s: %s" % (what, status) in str(later.value)


def test_a_status_normal_for_pytest_is_abnormal_for_the_engine_script():
    with pytest.raises(pytest.fail.Exception):
        mutation.run_child(_py("import sys; sys.exit(1)"), STANDIN, None, "one", normal=(0, 3))
    assert mutation.ABNORMAL


def test_report_lines(tmp_path, monkeypatch):
    report = tmp_path / "report.jsonl"
    monkeypatch.setenv("CELESTE_MUTANT_REPORT", str(report))
    killed = "import sys; print('FAILED a::b - assert 1 == 2'); print('FAILED c::d'); sys.exit(1)"
    mutation.run_child(_py(killed), STANDIN, "/some/lib.so", "mutant 1 a_bug")
    mutation.run_child(_py("print('0.25s call     a::b'); print('1 passed')"), STANDIN, None, "product")
    mutant, product = [json.loads(line) for line in report.read_text().splitlines()]
    assert mutant == dict(library="standin", child="mutant 1 a_bug", status=1, killed_by="a::b", wall_s=mutant["wall_s"])
    assert product == dict(library="standin", child="product", status=0, killed_by=None, wall_s=product["wall_s"],
                           test_wall_s={"a::b": 0.25})


def test_selecting_variable_is_removed_for_the_product_and_set_for_a_mutant():
    show = _py("import os; print(os.environ.get(%r))" % STANDIN.env)
    assert mutation.run_child(show, STANDIN, None, "product")[1] == "None\n"
    assert mutation.run_child(show, STANDIN, "/some/lib.so", "mutant")[1] == "/some/lib.so\n"


class _CountingPopen(subprocess.Popen):
    made = []

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.alive_at_start = 1 + sum(p.poll() is None for p in self.made)
        self.made.append(self)


def test_builder_runs_at_most_16_compilers_and_fails_without_leaving_one_behind(monkeypatch):
    monkeypatch.setattr(_CountingPopen, "made", [])
    monkeypatch.setattr(mutation.subprocess, "Popen", _CountingPopen)
    mutation.run_compilers([(_py("import time; time.sleep(0.3)"), None)] * 40)
    made = _CountingPopen.made
    assert len(made) == 40 and 2 <= max(p.alive_at_start for p in made) <= 16 == mutation.MAX_COMPILERS
    del made[:]
    commands = [(_py("import sys, time; time.sleep(0.3); sys.exit(%d)" % (i == 3)), None) for i in range(40)]
    with pytest.raises(RuntimeError):
        mutation.run_compilers(commands)
    assert 16 <= len(made) < 40 and all(p.returncode is not None for p in made)      # none started after the failure was seen
