"""Mutation tests of the fit, phot and mcmc libraries' parity suites (tests/mutation.py has the catalogue and the mechanism).

CELESTE_FIT_MUTANT, CELESTE_PHOT_MUTANT and CELESTE_MCMC_MUTANT each go into their own library; the heads of the libraries'
sources list them.  CELESTE_CLIENT_MUTANT (csrc/engine_client.h's pixel walk) goes into fit, 1 and 2 into phot as well.  Each
library's selection is its parity tests (not infer_box, not the refusals): what compares the device with a restatement, and the
bit-for-bit comparisons of a library's two paths."""
import pytest

from mutation import SUITES, build

LIBS = ("fit", "phot", "mcmc")
# (macro, k, name, library): the client mutants first, then each library's own
SATELLITE = [m + (lib,) for own in (False, True) for lib in LIBS for m in SUITES[lib].mutants
             if (m[0] != "CELESTE_CLIENT_MUTANT") == own]


def _ident(entry):
    macro, k, name, lib = entry
    return "%s-%s-%d-%s" % (lib, macro.split("_")[1].lower(), k, name)


def test_catalogue_and_sources_agree():
    """every switch of the four sources is in the catalogue and the reverse; names are unique per library; client mutants 1 to 6
    go into fit, 1 and 2 into phot as well; each of the other macros goes into its own library"""
    for lib in LIBS:
        SUITES[lib].check_catalogue()
    cat = SATELLITE
    assert len({(lib, name) for _, _, name, lib in cat}) == len(cat) == len({(m, k, lib) for m, k, _, lib in cat}) == 25
    assert len({SUITES[lib].path(m, k) for m, k, _, lib in cat}) == 25
    libs = {}
    for m, k, _, lib in cat:
        libs.setdefault(m, set()).add((k, lib))
    assert libs["CELESTE_CLIENT_MUTANT"] == {(k, "fit") for k in range(1, 7)} | {(1, "phot"), (2, "phot")}
    for m, lib in (("CELESTE_FIT_MUTANT", "fit"), ("CELESTE_PHOT_MUTANT", "phot"), ("CELESTE_MCMC_MUTANT", "mcmc")):
        assert {l for _, l in libs[m]} == {lib}, m
    assert len(libs) == 4


@pytest.fixture(scope="module")
def mutants():
    return build(LIBS)


@pytest.mark.gpu
@pytest.mark.parametrize("lib", sorted(LIBS))
def test_product_library_passes_the_selection(lib):
    SUITES[lib].product_passes()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", SATELLITE, ids=_ident)
def test_mutant_is_killed_by_the_parity_tests(mutants, entry):
    macro, k, _, lib = entry
    SUITES[lib].mutant_is_killed(mutants, k, macro)
