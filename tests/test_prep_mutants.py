"""Mutation tests of the prep library's parity suites (tests/mutation.py has the catalogue and the mechanism).

CELESTE_PREP_MUTANT, 22 mutants; the heads of csrc/prep/celeste_prep.hip and csrc/prep/prep_detected.h list them.  The selection
is what compares the device with the host's functions in tests/test_gpu_prep.py, tests/test_gpu_detected_table.py and
tests/test_gpu_wcs.py; not infer_box, the contexts' evaluations, the refusals."""
import pytest

from mutation import SUITES

SUITE = SUITES["prep"]


def test_catalogue_and_source_agree():
    SUITE.check_catalogue()
    assert len(SUITE.mutants) >= 14


@pytest.fixture(scope="module")
def mutants():
    return SUITE.build()


@pytest.mark.gpu
def test_product_library_passes_the_selection():
    SUITE.product_passes()


@pytest.mark.gpu
@SUITE.each_mutant
def test_mutant_is_killed_by_the_parity_tests(mutants, k):
    SUITE.mutant_is_killed(mutants, k)
