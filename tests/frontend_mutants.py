"""What tests/test_detect_mutants.py and tests/test_prep_mutants.py share, after tests/test_resid_mutants.py: the catalogue
check, the mutated builds (at most MAX_COMPILERS compilers at a time) and the child process that runs a selection of the parity
tests against one library.  Test infrastructure: one process on the device at a time, every child a fresh process.

With CELESTE_FRONTEND_REPORT=<file> every child appends one JSON line: the library, the mutant, its exit status, the test that
failed first (the killer) and its wall time; a product child adds the wall time of each test of the selection."""
import json
import os
import re
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "mutants")
CHILD_TIMEOUT = 300        # seconds; a child needs a small fraction of it
MAX_COMPILERS = 16         # compiler processes at a time


class Driver:
    def __init__(self, lib, macro, env, files, mutants, select, sources):
        self.lib, self.macro, self.env, self.files, self.mutants, self.select = lib, macro, env, files, mutants, select
        self.sources = sources     # the files that carry the switches; the first one's head defines the macro
        self.abnormal = []         # the first child that ended with neither 0 nor 1: nothing is started after it

    def path(self, k):
        return os.path.join(OUT, "libceleste_%s_mutant_%d_%s.so" % (self.lib, k, self.mutants[k]))

    def check_catalogue(self):
        """MUTANTS, the `MACRO == k` switches and the `k = what` lines of the heads are the same set"""
        texts = [open(s).read() for s in self.sources]
        found, listed = set(), set()
        for text in texts:
            found |= {int(k) for k in re.findall(r"\b%s\s*==\s*(\d+)" % self.macro, text)}
            head = text[:text.index("#include" if "#include" in text else "#pragma once")]
            listed |= {int(k) for k in re.findall(r"(?:^//|  )\s+(\d+) = ", head, flags=re.M)}
        assert found == set(self.mutants) == listed and 0 not in found, (sorted(found), sorted(listed))
        assert len(set(self.mutants.values())) == len(self.mutants)
        assert re.search(r"#ifndef %s\n#define %s 0\n#endif" % (self.macro, self.macro), texts[0])

    def build(self):
        """the mutated libraries: the library's own command line (the product's), one -D"""
        sys.path.insert(0, ROOT)
        import __graft_entry__ as ge
        os.makedirs(OUT, exist_ok=True)
        newest = max(os.path.getmtime(s) for s in ge.sources(self.lib))
        todo = [k for k in sorted(self.mutants) if not os.path.exists(self.path(k)) or os.path.getmtime(self.path(k)) < newest]
        running, failed = [], False
        while todo or running:
            while todo and not failed and len(running) < MAX_COMPILERS:
                k = todo.pop(0)
                argv, cwd = ge.compile_command(self.lib, out=self.path(k), defines=["%s=%d" % (self.macro, k)])
                running.append(subprocess.Popen(argv, cwd=cwd))
            failed = running.pop(0).wait() != 0 or failed
            if failed and not running:
                pytest.fail("a mutant did not build")
        return {k: self.path(k) for k in self.mutants}

    def child(self, lib_path, what, select=None):
        """runs the selection in a child; (exit status, output).  Refuses once a child has ended abnormally."""
        if self.abnormal:
            pytest.fail("not started: an earlier child ended abnormally (%s)" % self.abnormal[0])
        env = dict(os.environ)
        env.pop(self.env, None)
        if lib_path:
            env[self.env] = lib_path
        cmd = [sys.executable, "-m", "pytest"] + list(self.files) + ["-q", "-x", "-p", "no:cacheprovider", "--durations=0",
                                                                     "--durations-min=0", "-k", select or self.select]
        t0 = time.time()
        try:
            out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
            status, text = out.returncode, out.stdout + out.stderr
        except subprocess.TimeoutExpired as e:
            status = "time limit of %d s" % CHILD_TIMEOUT
            text = "".join(x.decode(errors="replace") if isinstance(x, bytes) else (x or "") for x in (e.stdout, e.stderr))
        wall = time.time() - t0
        failed = re.findall(r"^(?:FAILED|ERROR) (\S+)", text, flags=re.M)
        print("%s: status %s in %.1f s%s" % (what, status, wall, (", failed " + failed[0]) if failed else ""))
        report = os.environ.get("CELESTE_FRONTEND_REPORT")
        if report:
            line = dict(library=self.lib, child=what, status=status, killed_by=failed[0] if failed else None, wall_s=round(wall, 1))
            if not lib_path:
                calls = re.findall(r"^\s*([0-9.]+)s call\s+(\S+)", text, flags=re.M)
                line["test_wall_s"] = {name: float(s) for s, name in calls}
            with open(report, "a") as f:
                f.write(json.dumps(line) + "\n")
        if status not in (0, 1):
            self.abnormal.append("%s: %s" % (what, status))
            pytest.fail("the child of %s ended with %s, neither passed nor failed:\n%s" % (what, status, text[-3000:]))
        return status, text

    def product_passes(self):
        status, text = self.child(None, "product")
        assert status == 0, text[-3000:]
        assert re.search(r"\b\d+ passed", text) and "skipped" not in text.splitlines()[-1], text[-500:]

    def mutant_is_killed(self, libs, k):
        status, text = self.child(libs[k], "mutant %d %s" % (k, self.mutants[k]))
        assert status == 1, "the mutated library still passes its parity tests: the fixtures have no power against this bug"
