"""The hand-made planes of tests/detect_scenes.py hold what they were built for: asserted on the restatement
(tests/detect_reference.py) alone, without a device.  tests/test_gpu_detect_edges.py compares the device with the same
restatement on the same planes, so each property named here is an edge the device is shown to get right."""
import numpy as np
import pytest
from scipy import ndimage

import detect_reference as R
import detect_scenes as D


def _signature(r):
    return [(o["npix"], o["parent"], o["xmin"], o["xmax"], o["ymin"], o["ymax"]) for o in r["objects"]]


def _cells(cal, transposed):
    c = cal.T if transposed else cal
    return [c[:256], c[256:512], c[512:]]


@pytest.mark.parametrize("transposed", [False, True])
def test_fill_tie_has_one_bad_cell_between_two_good_ones_of_different_rms(transposed):
    p = D.fill_tie(transposed)
    cal = R.calibrate(*p)
    assert cal.shape == ((24, 520) if transposed else (520, 24))
    cells = _cells(cal, transposed)
    valid = [int((~np.isnan(c)).sum()) for c in cells]
    assert [2 * v >= c.size for v, c in zip(valid, cells)] == [True, False, True] and valid[1] > 0
    r0, r2 = R.cell_rms(cells[0]), R.cell_rms(cells[2])
    assert r2 > 2.5 * r0
    # cells 0 and 2 are equally near: the lower index gives the bad cell's value, and the median of the filtered mesh
    # [r0, r0, (r0 + r2) / 2] is r0; with the last cell instead it would be r2
    r = D.restate(p)
    assert r["rms"] == float(np.float32(r0)) != float(np.float32(r2))
    # and the tie decides a detection: the blob of cell 0 is one under 1.3 r0 and none under 1.3 r2
    at = (12, 100) if transposed else (100, 12)
    assert r["segmap"][at] > 0 and r["conv"][at] < 1.3 * r2


def test_half_valid_is_the_boundary_of_the_good_cell_rule():
    good, bad = D.half_valid(0), D.half_valid(1)
    cg, cb = R.calibrate(*good), R.calibrate(*bad)
    assert cg.shape == (16, 12) and 2 * int((~np.isnan(cg)).sum()) == cg.size and 2 * int((~np.isnan(cb)).sum()) == cg.size - 2
    rg, rb = D.restate(good), D.restate(bad)
    assert np.isfinite(rg["rms"]) and len(rg["objects"]) == 1
    assert np.isnan(rb["rms"]) and len(rb["objects"]) == 0 and not rb["mask"].any()


def test_median_gap_has_an_even_count_whose_middle_values_differ():
    cal = R.calibrate(*D.median_gap())
    v = np.sort(cal.reshape(-1))
    assert v.size == 192 and v[95] == 0.0 and v[96] == 2 * D.S and not np.isnan(v).any()
    # the mean of the two gives the board's own rms, the upper one another
    assert R.cell_rms(cal) == D.S
    upper = R.cell_rms(cal, median=lambda s: np.sort(s)[s.size // 2])
    assert abs(upper - D.S) > 0.05 * D.S
    assert D.restate(D.median_gap())["rms"] == D.S


@pytest.fixture(scope="module")
def painted():
    trace = []
    p = D.painted()
    return p, R.calibrate(*p), D.restate(p, trace=trace), trace


def _object_at(r, at):
    k = int(r["segmap"][at])
    assert k > 0, at
    return r["objects"][k - 1]


def test_painted_plane_margins(painted):
    p, cal, r, trace = painted
    assert cal.shape == (64, 48) and np.nanmin(cal) >= 0.0
    # the threshold lies between what is meant to be outside the mask and what is meant to be inside, with a margin
    above = (r["thresh"] - D.S) / D.Q
    assert 1.125 + 0.02 < above < 1.375 - 0.02, above
    # no convolved value other than the one made for it is within 0.5 % of the threshold (the device's rms is the
    # restatement's to a float32 rounding: 6e-8)
    near = np.abs(r["conv"] - r["thresh"]) < 0.005 * r["thresh"]
    assert np.argwhere(near).tolist() == [list(D.EXACT)]


def test_painted_anti_diagonal_link(painted):
    p, cal, r, trace = painted
    a, b = D.ANTI
    o = _object_at(r, (a, b))
    assert o is _object_at(r, (a + 2, b - 2)) and o["npix"] == 10
    # the only links between its two halves are (+1, -1) steps: under 4-connectivity, and with the three other
    # neighbours of the device's union step alone, it is two components of minarea pixels each
    sub = r["segmap"] == r["segmap"][a, b]
    assert ndimage.label(sub)[1] == 2
    no_anti = np.array([[1, 1, 0], [1, 1, 1], [0, 1, 1]])       # (i - 1, j - 1) and (i + 1, j + 1) stay, the anti-diagonal goes
    lab, n = ndimage.label(sub, structure=no_anti)
    assert n == 2 and sorted(np.bincount(lab[sub]).tolist()[1:]) == [5, 5]
    assert np.isnan(cal[a + 1, b - 1]) and r["conv"][a + 1, b - 1] > r["thresh"]


def test_painted_sizes_around_minarea(painted):
    p, cal, r, trace = painted
    assert _object_at(r, D.FIVE)["npix"] == 5                                     # = minarea: kept
    a, b = D.FOUR
    assert r["mask"][a:a + 2, b:b + 2].all() and r["mask"][a - 1:a + 3, b - 1:b + 3].sum() == 4 and not r["segmap"][a:a + 2, b:b + 2].any()
    assert _object_at(r, D.NINE)["npix"] == 9                                     # = 2 minarea - 1: never deblended
    # 2 minarea pixels with two peaks (the anti-diagonal pair): the level loop runs and cannot split it, since two pieces
    # of minarea pixels would be the whole component; 2 minarea + 1 is the smallest parent that splits
    a, b = D.ANTI
    assert _object_at(r, (a, b))["npix"] == 10
    for c in ((a, b), (a + 2, b - 2)):                                            # both centres are peaks
        around = r["conv"][c[0] - 1:c[0] + 2, c[1] - 1:c[1] + 2]
        assert (around < r["conv"][c]).sum() == 8
    a, b = D.PAIR
    left, right = _object_at(r, (a, b)), _object_at(r, (a, b + 4))
    assert left is not right and left["parent"] == right["parent"] and left["npix"] + right["npix"] == 11


def test_painted_bisector_pixel_is_an_exact_tie(painted):
    p, cal, r, trace = painted
    a, b = D.PAIR
    t = [t for t in trace if t["first"] == (a, b - 1)]
    assert len(t) == 1 and list(t[0]["amps"]) == [(a, b + 2)]
    amps = t[0]["amps"][(a, b + 2)]
    assert len(amps) == 2 and amps[0] == amps[1] > 0                              # equal to the last bit
    # the lower core takes it
    assert r["segmap"][a, b + 2] == r["segmap"][a, b] != r["segmap"][a, b + 4]
    assert _object_at(r, (a, b))["npix"] == 6 and _object_at(r, (a, b + 4))["npix"] == 5


def test_painted_triple_splits_at_two_levels(painted):
    p, cal, r, trace = painted
    a, b = D.TRIPLE
    t = [t for t in trace if r["segmap"][t["first"]] == r["segmap"][a, b]]
    assert len(t) == 1
    levels = t[0]["split_levels"]
    assert len(levels) == 2 and levels[0][0] < levels[1][0] and levels[0][1] == 0 and levels[1][1] > 0     # a new leaf splits again
    kids = [_object_at(r, (a, c)) for c in (b, b + 5, b + 9)]
    assert len({id(k) for k in kids}) == 3 and len({k["parent"] for k in kids}) == 1
    ties = [v for v in t[0]["amps"].values() if sorted(v)[-1] == sorted(v)[-2]]
    assert len(ties) == 6                                                         # the column between the last two cores


def test_painted_nan_inside_a_plateau_and_the_exact_threshold(painted):
    p, cal, r, trace = painted
    a, b = D.PLATEAU
    hole = (a + 2, b + 1)
    assert np.isnan(cal[hole]) and r["conv"][hole] > 2 * r["thresh"] and not r["mask"][hole] and r["segmap"][hole] == 0
    assert r["mask"][hole[0] - 1:hole[0] + 2, hole[1] - 1:hole[1] + 2].sum() == 8
    # the filter takes the lone pixel at EXACT to the threshold itself, bit for bit: conv > thresh leaves it out
    assert r["conv"][D.EXACT] == r["thresh"] and not r["mask"][D.EXACT]
    assert not r["mask"][D.EXACT[0] - 1:D.EXACT[0] + 2, D.EXACT[1] - 1:D.EXACT[1] + 2].any()


def test_painted_children_are_not_in_core_order(painted):
    p, cal, r, trace = painted
    a, b = D.LOPSIDED
    big, bump = _object_at(r, (a, b)), _object_at(r, (a + 5, b - 5))
    assert big is not bump and big["parent"] == bump["parent"]
    t = [t for t in trace if r["segmap"][t["first"]] == r["segmap"][a, b]][0]
    # the bump's core comes first in raster order, the pyramid's child does: it owns the parent's first pixel
    core_of_first = t["core"][t["core"] >= 0][0]
    assert t["owner"][0] != core_of_first
    assert r["objects"].index(big) < r["objects"].index(bump)


def test_no_object_of_a_scene_leaves_its_angle_or_its_twelfth_rule_to_a_rounding():
    """theta = atan2(2 xy, x2 - y2) / 2, and pi / 4 when x2 = y2 bit for bit: an object with x2 = y2 in exact arithmetic gets
    whichever the summation order gives.  The moments are compared with a tolerance, so the scenes keep away from that,
    and from x2 y2 - xy^2 = 1 / 144."""
    scenes = [D.painted(), D.fill_tie(False), D.fill_tie(True), D.half_valid(0), D.parameters_plane()] + list(D.mixed_batch())
    catalogs = [D.restate(p) for p in scenes] + [D.restate(D.parameters_plane(), **D.OTHER)]
    for r in catalogs:
        for o in r["objects"]:
            x2, y2, xy = o["x2"], o["y2"], o["xy"]
            if x2 == 0 and y2 == 0 and xy == 0:                                   # one pixel carries all the weight: exact
                continue
            det = x2 * y2 - xy * xy
            assert abs(det - 1.0 / 144.0) > 1e-9
            assert abs(x2 - y2) > 1e-9 * (x2 + y2 + 1.0 / 6.0), (o["npix"], o["xmin"], o["ymin"])


def test_mixed_batch_shapes_and_blends():
    batch = D.mixed_batch()
    shapes = [p.pixels.shape for p in batch]
    assert len(set(shapes)) == len(shapes) >= 3 and all(h != w for h, w in shapes)
    rs = [D.restate(p) for p in batch]
    counts = [len(r["objects"]) for r in rs]
    assert counts == [1, 5, 0, 2]
    # from the second image on, an image's object and parent indices differ from their batch-wide ones; two images hold
    # deblended parents
    assert [o["parent"] for o in rs[1]["objects"]] == [0, 0, 1, 1, 2] and [o["parent"] for o in rs[3]["objects"]] == [0, 0]
    for p in batch:
        assert len(set(p.nelec_per_nmgy.tolist())) == 3                           # the calibration changes from row to row


def test_each_parameter_changes_the_catalog():
    p = D.parameters_plane()
    other = _signature(D.restate(p, **D.OTHER))
    assert other != _signature(D.restate(p, **D.DEFAULTS))
    for name in D.OTHER:
        kw = dict(D.OTHER)
        kw[name] = D.DEFAULTS[name]
        assert _signature(D.restate(p, **kw)) != other, name
