"""Mutation tests of the prep library's parity suites, after tests/test_resid_mutants.py.

The library is rebuilt with one deliberate bug at a time (-DCELESTE_PREP_MUTANT=k; the heads of csrc/prep/celeste_prep.hip
and csrc/prep/prep_detected.h list them) into tests/mutants/ (git-ignored build artefacts), and the tests of
tests/test_gpu_prep.py, tests/test_gpu_detected_table.py and tests/test_gpu_wcs.py that compare the device with the host's
functions run against it in a child process, the mutant selected through CELESTE_MI355X_PREP_LIB.  A child that fails (exit
status 1) has killed its mutant; one that passes shows a bug the suite cannot see.  Any other end of a child (a signal, its
time limit, pytest's statuses 2 to 5) is an error of the harness, not a kill: the test fails with the child's tail and nothing
more is started on the device.

The catalogue test (not -m gpu) keeps MUTANTS, the `CELESTE_PREP_MUTANT == k` switches and the heads' lists in step."""
import os

import pytest

from frontend_mutants import ROOT, Driver

MUTANTS = {1: "round_half_away", 2: "box_last_column_short", 3: "tried_lower_bound_sign", 4: "radius_max_for_min",
           5: "radius_without_width_scale", 6: "no_pivoting", 7: "jacobian_smaller_step", 8: "active_counts_nan",
           9: "overlap_strict_rows", 10: "row_window_one_short", 11: "unique_keeps_repeats", 12: "stamp_tx_without_minus_one",
           13: "stamp_cmat_transposed", 14: "sky_median_upper", 15: "sky_le", 16: "sky_nelec_by_column", 17: "match_le_radius",
           18: "match_tie_highest", 19: "append_reversed", 20: "shape_last_band_on_tie", 21: "detection_box_replaces_minimum",
           22: "angular_half_separation"}
# what compares the device with the host's functions; not infer_box, the contexts' evaluations, the refusals
SELECT = ("patch_table or neighbour_lists or world_center or stamps or sky_flags or column_major or join_rules or more_entries "
          "or boxes_dense or boxes_sparse or rotated_scaled or against_mpmath or detected_table_is_build or needs_pivoting or exact_ties")
_PREP = os.path.join(ROOT, "celeste.jl_amd", "csrc", "prep")
DRIVER = Driver("prep", "CELESTE_PREP_MUTANT", "CELESTE_MI355X_PREP_LIB",
                ["tests/test_gpu_prep.py", "tests/test_gpu_detected_table.py", "tests/test_gpu_wcs.py"], MUTANTS, SELECT,
                [os.path.join(_PREP, "celeste_prep.hip"), os.path.join(_PREP, "prep_detected.h")])


def test_catalogue_and_source_agree():
    DRIVER.check_catalogue()
    assert len(MUTANTS) >= 14


@pytest.fixture(scope="module")
def mutants():
    return DRIVER.build()


@pytest.mark.gpu
def test_product_library_passes_the_selection():
    DRIVER.product_passes()


@pytest.mark.gpu
@pytest.mark.parametrize("k", sorted(MUTANTS), ids=lambda k: "%d-%s" % (k, MUTANTS[k]))
def test_mutant_is_killed_by_the_parity_tests(mutants, k):
    DRIVER.mutant_is_killed(mutants, k)
