"""Mutation tests of the astrometry's parity suite (tests/mutation.py has the catalogue and the mechanism).

CELESTE_ASTROM_MUTANT, 5 mutants; the head of csrc/astrom/celeste_astrom.hip lists them.  The selection of
tests/test_gpu_astrom.py is the star fixture against the restatement (mutants 1, 2, 4, 5: its row is perturbed by most of a pixel
and its scales are far from 1) and the linear motion under a rotated WCS, whose Jacobian is not symmetric (mutant 3)."""
import pytest

from mutation import SUITES

SUITE = SUITES["astrom"]


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
