"""Source detection on the MI355X against the numpy restatement (tests/detect_reference.py) on the hand-made planes of
tests/detect_scenes.py: the edges that the synthetic fields of tests/test_gpu_detect.py leave to chance.  What each plane
holds is asserted on the restatement alone in tests/test_detect_scenes_host.py.

The restatement is given nothing of the device's: its own rms gives its own threshold, and the device's rms and threshold
are compared with them bit for bit (test_gpu_detect._compare), then the mask, the labels, the objects and their pixels."""
import functools

import numpy as np
import pytest

import detect_scenes as D
from celeste_jl_amd import detect
from test_gpu_detect import _compare

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _restated(name, *args):
    return D.restate(getattr(D, name)(*args))


def _device_equals_restatement(name, *args):
    cat = detect.extract([getattr(D, name)(*args)], want_maps=True)[0]
    ref = _restated(name, *args)
    assert cat.rms == ref["rms"] or (np.isnan(cat.rms) and np.isnan(ref["rms"])), (cat.rms, ref["rms"])
    _compare(cat, ref)
    return cat


def test_hand_painted_components():
    """the anti-diagonal link, minarea and minarea - 1 pixels, 2 minarea - 1, 2 minarea and 2 minarea + 1 pixels, a leaf that
    splits again, pixels on the bisector of two equal cores, a NaN inside a plateau, a convolved value equal to the threshold,
    children whose order is not their cores'"""
    cat = _device_equals_restatement("painted")
    assert sorted(cat.npix.tolist()) == [5, 5, 6, 9, 10, 19, 22, 26, 28, 37, 212]


def test_an_even_count_takes_the_mean_of_its_two_middle_values():
    cat = _device_equals_restatement("median_gap")
    assert cat.rms == D.S


def test_a_cell_with_exactly_half_its_pixels_is_good_and_one_fewer_is_bad():
    good = _device_equals_restatement("half_valid", 0)
    bad = _device_equals_restatement("half_valid", 1)
    assert len(good) == 1 and np.isnan(bad.rms) and np.isnan(bad.thresh) and len(bad) == 0 and not bad.mask.any()


@pytest.mark.parametrize("transposed", [False, True], ids=["520x24", "24x520"])
def test_a_bad_cell_between_two_good_ones_takes_the_lower_index(transposed):
    _device_equals_restatement("fill_tie", transposed)


def test_a_batch_of_differently_shaped_images():
    batch = D.mixed_batch()
    cats = detect.extract(list(batch), want_maps=True)
    refs = [D.restate(p) for p in batch]
    for cat, ref in zip(cats, refs):
        _compare(cat, ref)
    assert [len(c) for c in cats] == [1, 5, 0, 2] and cats[3].parent.tolist() == [0, 0]
    # and an image's catalog does not depend on its place in the batch
    last = detect.extract([batch[3]], want_maps=True)[0]
    for f in ("npix", "parent", "x", "y", "x2", "y2", "xy", "a", "b", "theta", "flux", "peak"):
        assert np.array_equal(getattr(last, f), getattr(cats[3], f)), f
    assert np.array_equal(last.segmap, cats[3].segmap) and last.thresh == cats[3].thresh


def test_parameters_other_than_the_defaults():
    p = D.parameters_plane()
    kw = D.OTHER
    cat = detect.extract([p], want_maps=True, thresh=kw["thresh"], minarea=kw["minarea"], deblend_nthresh=kw["nthresh"],
                         deblend_cont=kw["cont"])[0]
    _compare(cat, D.restate(p, **kw), thresh=kw["thresh"])
    # one parameter at a time back at its default: the device follows the restatement there too (each of these catalogs
    # differs from the one above, tests/test_detect_scenes_host.py)
    for name in kw:
        one = dict(kw)
        one[name] = D.DEFAULTS[name]
        cat = detect.extract([p], want_maps=True, thresh=one["thresh"], minarea=one["minarea"], deblend_nthresh=one["nthresh"],
                             deblend_cont=one["cont"])[0]
        _compare(cat, D.restate(p, **one), thresh=one["thresh"])
