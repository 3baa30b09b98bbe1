"""Mutation tests of the detect library's parity suite, after tests/test_resid_mutants.py.

The library is rebuilt with one deliberate bug at a time (-DCELESTE_DETECT_MUTANT=k; the head of
csrc/detect/celeste_detect.hip lists them) into tests/mutants/ (git-ignored build artefacts), and the tests that compare the
device with the numpy restatement (tests/detect_reference.py) run against it in a child process, the mutant selected through
CELESTE_MI355X_DETECT_LIB: the hand-made edge scenes of tests/test_gpu_detect_edges.py first, then the synthetic fields of
tests/test_gpu_detect.py.  A child that fails (exit status 1) has killed its mutant; one that passes shows a bug the suite
cannot see.  Any other end of a child (a signal, its time limit, pytest's statuses 2 to 5) is an error of the harness, not a
kill: the test fails with the child's tail and nothing more is started on the device.

The catalogue test (not -m gpu) keeps MUTANTS, the `CELESTE_DETECT_MUTANT == k` switches and the head's list in step."""
import os

import pytest

from frontend_mutants import ROOT, Driver

MUTANTS = {1: "nelec_by_column", 2: "mesh_median_upper", 3: "good_cell_strict", 4: "sigma_n_minus_1", 5: "fill_tie_last_cell",
           6: "thresh_default", 7: "nan_centre_in_mask", 8: "filter_ge", 9: "antidiagonal_dropped", 10: "keep_gt_minarea",
           11: "parent_batch_index", 12: "split_ignores_minarea", 13: "level_exponent_ahead", 14: "tie_to_higher_core",
           15: "children_in_core_order", 16: "twelfth_rule_unconditional", 17: "segmap_batch_index"}
# what compares the device with the restatement; not infer_box, recall and precision, the refusals
SELECT = "detect_edges or device_equals_restatement or deblending_splits or large_parent"
DRIVER = Driver("detect", "CELESTE_DETECT_MUTANT", "CELESTE_MI355X_DETECT_LIB",
                ["tests/test_gpu_detect_edges.py", "tests/test_gpu_detect.py"], MUTANTS, SELECT,
                [os.path.join(ROOT, "celeste.jl_amd", "csrc", "detect", "celeste_detect.hip")])


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
