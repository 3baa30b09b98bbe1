"""Mutation tests of the stack's parity suite (tests/mutation.py has the catalogue and the mechanism).

CELESTE_STACK_MUTANT, 6 mutants of the resid library, under a macro of their own; the head of csrc/resid/resid_stack.h lists
them.  The selection is what compares the device with the numpy restatement in tests/test_gpu_stack.py, and culling off against
on."""
import pytest

from mutation import SUITES

SUITE = SUITES["stack"]


def test_catalogue_and_header_agree():
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
