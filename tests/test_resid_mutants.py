"""Mutation tests of the resid library's parity suite (tests/mutation.py has the catalogue and the mechanism).

CELESTE_RESID_MUTANT, 5 mutants; the head of csrc/resid/celeste_resid.hip lists them.  The selection is what compares the device
with the numpy restatement in tests/test_gpu_resid.py: the frame model, the filter maps, the peak rule."""
import pytest

from mutation import SUITES

SUITE = SUITES["resid"]


def test_catalogue_and_source_agree():
    SUITE.check_catalogue()


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
