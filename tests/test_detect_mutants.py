"""Mutation tests of the detect library's parity suite (tests/mutation.py has the catalogue and the mechanism).

CELESTE_DETECT_MUTANT, 17 mutants; the head of csrc/detect/celeste_detect.hip lists them.  The selection is what compares the
device with the numpy restatement (tests/detect_reference.py): the hand-made edge scenes of tests/test_gpu_detect_edges.py first,
then the synthetic fields of tests/test_gpu_detect.py; not infer_box, recall and precision, the refusals."""
import pytest

from mutation import SUITES

SUITE = SUITES["detect"]


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
