#!/usr/bin/env python3
"""Mutation testing: the one catalogue, builder, child runner, report and catalogue check behind the seven test_*_mutants.py files.

Each product library is rebuilt with one deliberate bug at a time (-D<MACRO>=k: the head of the file that defines the macro lists
the bugs) into tests/mutants/ (git-ignored build artefacts), and a selection of that library's own parity tests runs against it in
a child process, the mutant selected through the library's environment variable.  A child that fails (exit status 1) has killed
its mutant; one that passes shows a bug the suite cannot see.  Any other end of a child (a signal, its time limit, pytest's
statuses 2 to 5) is an error of the harness, not a kill: the test fails with the child's tail, and no child of any suite is
started on the device after it in this process.  One process on the device at a time, every child a fresh process.

With CELESTE_MUTANT_REPORT=<file> every child appends one JSON line: the library, the child, its exit status, the test that failed
first (the killer) and its wall time; a product child adds the wall time of each test of the selection.

usage: python tests/mutation.py [--force] [suite ...]     builds the mutated libraries (of every suite by default)"""
import functools
import json
import os
import re
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "celeste.jl_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "mutants")
CHILD_TIMEOUT = 300        # seconds; a pytest child needs a small fraction of it
MAX_COMPILERS = 16         # compiler processes at a time
ABNORMAL = []              # the first child that ended abnormally, of whichever suite: nothing is started after it

# macro -> the files under csrc that carry its switches; the first one's head defines it
SOURCES = {
    "CELESTE_MUTANT": ["elbo_kernels.h", "fused_kernels.h", "eval_fused.h"],
    "CELESTE_CLIENT_MUTANT": ["engine_client.h"],
    "CELESTE_FIT_MUTANT": ["fit/celeste_fit.hip"],
    "CELESTE_PHOT_MUTANT": ["phot/celeste_phot.hip"],
    "CELESTE_MCMC_MUTANT": ["mcmc/celeste_mcmc.hip"],
    "CELESTE_RESID_MUTANT": ["resid/celeste_resid.hip"],
    "CELESTE_STACK_MUTANT": ["resid/resid_stack.h"],
    "CELESTE_ASTROM_MUTANT": ["astrom/celeste_astrom.hip"],
    "CELESTE_DETECT_MUTANT": ["detect/celeste_detect.hip"],
    "CELESTE_PREP_MUTANT": ["prep/celeste_prep.hip", "prep/prep_detected.h"],
}
# The client mutants (engine_client.h's pixel walk) go into fit, whose stamps show m + B pixel by pixel; 1 and 2 go into phot as
# well, which uses m and B apart (a = iota m, b = iota (eps + B)).
_CLIENT = {1: "own_light_in_last_column", 2: "neighbour_light_in_its_last_column", 3: "neighbour_bitmap_ignored",
           4: "bitmap_transposed", 5: "iota_by_column", 6: "neighbour_with_target_stamp"}


class Suite:
    """One library (as keyed in __graft_entry__.LIBRARIES), the variable that selects its file, the test files and the -k
    selection of its children, and its mutants: {macro: {k: name}}."""

    def __init__(self, name, lib, env, files, select, mutants):
        self.name, self.lib, self.env, self.files, self.select = name, lib, env, files, select
        self.mutants = [(macro, k, names[k]) for macro, names in mutants.items() for k in sorted(names)]
        self.names = {(macro, k): name for macro, k, name in self.mutants}
        self.macro = None if len(mutants) > 1 else next(iter(mutants))      # what `k` alone means in this suite

    @property
    def each_mutant(self):
        """parametrises a test over `k`, for a suite with one macro"""
        return pytest.mark.parametrize("k", [k for _, k, _ in self.mutants], ids=["%d-%s" % m[1:] for m in self.mutants])

    def path(self, macro, k):
        return os.path.join(OUT, "libceleste_%s_%s_%d_%s.so" % (self.lib, macro[len("CELESTE_"):].lower(), k, self.names[macro, k]))

    def check_catalogue(self):
        for macro in {m for m, _, _ in self.mutants}:
            check_macro(macro)
        assert len({name for _, _, name in self.mutants}) == len(self.mutants)     # names are unique per library

    def build(self, force=False):
        return build([self.name], force)

    def child(self, lib_path, what, select=None):
        """runs the selection in a pytest child; (exit status, output)"""
        cmd = [sys.executable, "-m", "pytest"] + list(self.files) + ["-q", "-x", "-p", "no:cacheprovider", "--durations=0",
                                                                     "--durations-min=0", "-k", select or self.select]
        return run_child(cmd, self, lib_path, what)

    def product_passes(self):
        status, text = self.child(None, "product")
        assert status == 0, text[-3000:]
        assert re.search(r"\b\d+ passed", text) and "skipped" not in text.splitlines()[-1], text[-500:]

    def mutant_is_killed(self, libs, k, macro=None):
        macro = macro or self.macro
        status, text = self.child(libs[self.name, macro, k], "mutant %s=%d %s" % (macro, k, self.names[macro, k]))
        assert status == 1, "the mutated library still passes its parity tests: the fixtures have no power against this bug"


SUITES = {s.name: s for s in (
    # (tests/test_mutants.py runs its own script on two goldens, not a selection of pytest files)
    Suite("engine", "engine", "CELESTE_MI355X_LIB", [], None, {"CELESTE_MUTANT": {
        1: "iota_by_column", 2: "sky_transposed", 3: "one_stamp_for_all",
        # single-precision code only (CELESTE_FLAG_FP32)
        4: "px2_h4c_dropped_term", 5: "px2_grad_nu_low_half", 6: "value_f2_p12_low_half", 7: "pk_h4b_m3p11"}}),
    Suite("fit", "fit", "CELESTE_MI355X_FIT_LIB", ["tests/test_gpu_fit.py"], "restatement or non_finite_row or multifield", {
        "CELESTE_CLIENT_MUTANT": _CLIENT,
        "CELESTE_FIT_MUTANT": {1: "self_ignores_neighbours", 2: "unvisited_stamp_not_nan", 3: "max_z_added", 4: "first_tile_dropped",
                               5: "bad_flag_not_reported"}}),
    Suite("phot", "phot", "CELESTE_MI355X_PHOT_LIB", ["tests/test_gpu_phot.py"],
          "restatement or same_bits or capacity_of_lds or non_finite_row or multifield or max_iters", {
        "CELESTE_CLIENT_MUTANT": {k: _CLIENT[k] for k in (1, 2)},
        "CELESTE_PHOT_MUTANT": {1: "round_offset_dropped", 2: "b_without_neighbours", 3: "at_bound_never_reached",
                                4: "summary_weight_inverse_sigma", 5: "tolerance_not_scaled_by_sigma",
                                6: "sigma_without_square_root"}}),
    Suite("mcmc", "mcmc", "CELESTE_MI355X_MCMC_LIB", ["tests/test_gpu_mcmc.py"], "restatement or replay", {
        "CELESTE_MCMC_MUTANT": {1: "source_light_not_rounded_to_float", 2: "iota_by_column", 3: "nan_pixel_subtracts_rate",
                                4: "lgamma_sum_not_subtracted", 5: "angle_up_to_two_pi", 6: "scale_prior_without_log_scale"}}),
    Suite("resid", "resid", "CELESTE_MI355X_RESID_LIB", ["tests/test_gpu_resid.py"],
          "frame_model or explicit_bitmaps or filter_maps or find_peaks", {
        "CELESTE_RESID_MUTANT": {1: "light_in_last_column", 2: "bitmap_ignored", 3: "phi_transposed", 4: "iota_by_column",
                                 5: "tie_rule_not_strict"}}),
    # the stack's kernels are part of the resid library, under a macro of their own
    Suite("stack", "resid", "CELESTE_MI355X_RESID_LIB", ["tests/test_gpu_stack.py"],
          "edge_scene_against or tan_scene_against or culling_changes", {
        "CELESTE_STACK_MUTANT": {1: "d_weighted_by_s", 2: "truncation_for_rint", 3: "gather_transposed", 4: "masked_pixel_not_skipped",
                                 5: "min_images_strict", 6: "cull_without_margin"}}),
    Suite("astrom", "astrom", "CELESTE_MI355X_ASTROM_LIB", ["tests/test_gpu_astrom.py"], "sample_star or linear_motion_scene", {
        "CELESTE_ASTROM_MUTANT": {1: "star_shift_sign", 2: "alpha_missing_from_d", 3: "j_transposed_in_w", 4: "last_column_lit",
                                  5: "likelihood_test_inverted"}}),
    Suite("detect", "detect", "CELESTE_MI355X_DETECT_LIB", ["tests/test_gpu_detect_edges.py", "tests/test_gpu_detect.py"],
          "detect_edges or device_equals_restatement or deblending_splits or large_parent", {
        "CELESTE_DETECT_MUTANT": {
            1: "nelec_by_column", 2: "mesh_median_upper", 3: "good_cell_strict", 4: "sigma_n_minus_1", 5: "fill_tie_last_cell",
            6: "thresh_default", 7: "nan_centre_in_mask", 8: "filter_ge", 9: "antidiagonal_dropped", 10: "keep_gt_minarea",
            11: "parent_batch_index", 12: "split_ignores_minarea", 13: "level_exponent_ahead", 14: "tie_to_higher_core",
            15: "children_in_core_order", 16: "twelfth_rule_unconditional", 17: "segmap_batch_index"}}),
    Suite("prep", "prep", "CELESTE_MI355X_PREP_LIB",
          ["tests/test_gpu_prep.py", "tests/test_gpu_detected_table.py", "tests/test_gpu_wcs.py"],
          "patch_table or neighbour_lists or world_center or stamps or sky_flags or column_major or join_rules or more_entries "
          "or boxes_dense or boxes_sparse or rotated_scaled or against_mpmath or detected_table_is_build or needs_pivoting or exact_ties", {
        "CELESTE_PREP_MUTANT": {
            1: "round_half_away", 2: "box_last_column_short", 3: "tried_lower_bound_sign", 4: "radius_max_for_min",
            5: "radius_without_width_scale", 6: "no_pivoting", 7: "jacobian_smaller_step", 8: "active_counts_nan",
            9: "overlap_strict_rows", 10: "row_window_one_short", 11: "unique_keeps_repeats", 12: "stamp_tx_without_minus_one",
            13: "stamp_cmat_transposed", 14: "sky_median_upper", 15: "sky_le", 16: "sky_nelec_by_column", 17: "match_le_radius",
            18: "match_tie_highest", 19: "append_reversed", 20: "shape_last_band_on_tie", 21: "detection_box_replaces_minimum",
            22: "angular_half_separation"}}),
)}


# ---- the catalogue against the sources (no GPU) ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _csrc_code():
    """{path relative to csrc: its text without comments}"""
    code = {}
    for d, _, names in os.walk(CSRC):
        for n in names:
            if not n.endswith((".so", ".o")):
                p = os.path.join(d, n)
                code[os.path.relpath(p, CSRC)] = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(p).read(), flags=re.S)
    return code


def check_macro(macro):
    """The numbers the catalogue gives `macro` (in every suite), the `MACRO == k` and `MACRO != k` switches of its files and the
    `k = what` lines of those files' heads are the same set; no other file under csrc uses the macro (a comment may speak of
    it); the first file defines it as 0."""
    catalogue = {k for s in SUITES.values() for m, k, _ in s.mutants if m == macro}
    found, listed = set(), set()
    for rel in SOURCES[macro]:
        text = open(os.path.join(CSRC, rel)).read()
        found |= {int(k) for k in re.findall(r"\b%s\s*[!=]=\s*(\d+)" % macro, text)}
        # the head: up to the macro's definition where the file has one (engine_client.h's list sits after an #include)
        end = re.search(r"^#ifndef %s$" % macro, text, flags=re.M) or re.search(r"^#(include|pragma once)", text, flags=re.M)
        listed |= {int(k) for k in re.findall(r"\b(\d+) = ", text[:end.start()], flags=re.M)}
    assert found == catalogue == listed - {0} and 0 not in found, (macro, sorted(found), sorted(catalogue), sorted(listed))
    elsewhere = [rel for rel, code in _csrc_code().items() if rel not in SOURCES[macro] and re.search(r"\b%s\b" % macro, code)]
    assert not elsewhere, (macro, elsewhere)
    assert re.search(r"#ifndef %s\n#define %s 0\n#endif" % (macro, macro), open(os.path.join(CSRC, SOURCES[macro][0])).read())


# ---- the mutated libraries -------------------------------------------------------------------------------------------------------
def run_compilers(commands):
    """runs (argv, working directory) commands, at most MAX_COMPILERS at a time; after one fails it starts no more, waits for
    those running and raises"""
    todo, running, failed = list(commands), [], False
    while todo or running:
        while todo and not failed and len(running) < MAX_COMPILERS:
            argv, cwd = todo.pop(0)
            running.append(subprocess.Popen(argv, cwd=cwd))
        failed = running.pop(0).wait() != 0 or failed
        if failed and not running:
            raise RuntimeError("a mutant did not build")


def build(names=None, force=False):
    """The mutated libraries of the named suites (all by default): each library's own command line (the product's), one -D.  A
    library is rebuilt when it is missing or older than one of its sources.  {(suite, macro, k): path}"""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    os.makedirs(OUT, exist_ok=True)
    libs, commands = {}, []
    for s in [SUITES[n] for n in names or SUITES]:
        newest = max(os.path.getmtime(f) for f in ge.sources(s.lib))
        for macro, k, _ in s.mutants:
            p = libs[s.name, macro, k] = s.path(macro, k)
            if force or not os.path.exists(p) or os.path.getmtime(p) < newest:
                commands.append(ge.compile_command(s.lib, out=p, defines=["%s=%d" % (macro, k)]))
    run_compilers(commands)
    return libs


# ---- the children ----------------------------------------------------------------------------------------------------------------
def run_child(cmd, suite, lib_path, what, normal=(0, 1), timeout=CHILD_TIMEOUT):
    """Runs `cmd` in a fresh process, the suite's selecting variable removed from its environment, or set to `lib_path` for a
    mutant; (exit status, output).  A status outside `normal`, a signal or the time limit fails the calling test with the child's
    tail, and every later call, of any suite, is refused."""
    if ABNORMAL:
        pytest.fail("not started: an earlier child ended abnormally (%s)" % ABNORMAL[0])
    env = dict(os.environ)
    env.pop(suite.env, None)
    if lib_path:
        env[suite.env] = lib_path
    t0 = time.time()
    try:
        out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
        status, text = out.returncode, out.stdout + out.stderr
    except subprocess.TimeoutExpired as e:
        status = "time limit of %d s" % timeout
        text = "".join(x.decode(errors="replace") if isinstance(x, bytes) else (x or "") for x in (e.stdout, e.stderr))
    wall = time.time() - t0
    failed = re.findall(r"^(?:FAILED|ERROR) (\S+)", text, flags=re.M)
    print("%s %s: status %s in %.1f s%s" % (suite.name, what, status, wall, (", failed " + failed[0]) if failed else ""))
    report = os.environ.get("CELESTE_MUTANT_REPORT")
    if report:
        line = dict(library=suite.name, child=what, status=status, killed_by=failed[0] if failed else None, wall_s=round(wall, 1))
        if not lib_path:
            calls = re.findall(r"^\s*([0-9.]+)s call\s+(\S+)", text, flags=re.M)
            line["test_wall_s"] = {name: float(s) for s, name in calls}
        with open(report, "a") as f:
            f.write(json.dumps(line) + "\n")
    if status not in normal:
        ABNORMAL.append("%s %s: %s" % (suite.name, what, status))
        pytest.fail("the child of %s %s ended with %s, not one of %s:\n%s" % (suite.name, what, status, normal, text[-3000:]))
    return status, text


if __name__ == "__main__":
    print("\n".join(build([a for a in sys.argv[1:] if a != "--force"], "--force" in sys.argv).values()))
