"""Host-side pieces of source detection (celeste_jl_amd.detect): the geometry of detect_sources, the ellipse rules
the device follows (restated in tests/detect_reference.py), and the C ABI of libceleste_detect.so."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import detect_reference as R
from celeste_jl_amd import detect, model
from celeste_jl_amd.model import Image, ConstantPSFMap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gaussian_blob(H, W, cov, center, flux=1000.0):
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.stack([ii - center[0], jj - center[1]], axis=-1)
    q = np.einsum("...i,ij,...j->...", d, np.linalg.inv(cov), d)
    return flux * np.exp(-0.5 * q) / (2 * np.pi * math.sqrt(np.linalg.det(cov)))


@pytest.mark.parametrize("cov", [np.diag([9.0, 4.0]), np.array([[6.0, 2.5], [2.5, 4.0]]), np.array([[3.0, -1.2], [-1.2, 5.0]])])
def test_moments_of_a_gaussian_blob(cov):
    img = _gaussian_blob(81, 81, cov, (40.0, 40.0))
    ii, jj = np.nonzero(img > 0)
    o = R.moments(ii, jj, img[ii, jj])
    assert abs(o["x"] - 40.0) < 1e-9 and abs(o["y"] - 40.0) < 1e-9
    # a fine pixel grid integrates a smooth Gaussian almost exactly
    np.testing.assert_allclose([o["x2"], o["y2"], o["xy"]], [cov[0, 0], cov[1, 1], cov[0, 1]], rtol=1e-6, atol=1e-6)
    ev = np.linalg.eigvalsh(cov)
    assert abs(o["a"] - math.sqrt(ev[1])) < 1e-6 and abs(o["b"] - math.sqrt(ev[0])) < 1e-6
    if cov[0, 1] != 0:
        w, v = np.linalg.eigh(cov)
        major = v[:, 1]
        th = math.atan2(major[1], major[0])
        d = (o["theta"] - th + math.pi / 2) % math.pi - math.pi / 2   # an axis: defined modulo pi
        assert abs(d) < 1e-6
    else:
        assert abs(o["theta"]) < 1e-9


def test_one_pixel_object_takes_the_one_twelfth_rule():
    o = R.moments(np.array([5]), np.array([7]), np.array([3.0]))
    assert o["x2"] == 0 and o["y2"] == 0
    assert abs(o["a"] - math.sqrt(1 / 12)) < 1e-15 and abs(o["b"] - math.sqrt(1 / 12)) < 1e-15
    assert o["theta"] == math.pi / 4


def test_dilate_box_rounds_halves_to_even():
    # length 5: 0.2 * 5 / 2 = 0.5 -> 0 ; length 15: 1.5 -> 2 ; length 25: 2.5 -> 2 ; length 10: 1.0 -> 1
    assert detect.dilate_box(((3, 7), (0, 14)), 0.2) == ((3, 7), (-2, 16))
    assert detect.dilate_box(((10, 34), (1, 10)), 0.2) == ((8, 36), (0, 11))


@pytest.mark.parametrize("J,expected", [
    (np.eye(2), -math.pi / 2),
    (np.array([[0.0, 1.0], [1.0, 0.0]]), 0.0),                 # det < 0: the sign flips both arguments
    (np.array([[2.0, 0.0], [0.0, -2.0]]), math.pi / 2),
    (np.array([[0.0, -1.0], [1.0, 0.0]]), None),
])
def test_x_vs_n_angle(J, expected):
    cd = np.linalg.inv(J)
    s = np.sign(np.linalg.det(cd))
    want = -(math.atan2(s * cd[0, 1], s * cd[0, 0]) + math.pi / 2)
    got = detect.x_vs_n_angle(J)
    assert got == want
    if expected is not None:
        assert abs(got - expected) < 1e-15


def test_matching_rule():
    w0 = np.array([[10.0, 10.0], [50.0, 50.0]])
    w1 = np.array([[10.2, 10.1], [30.0, 30.0], [50.0, 53.0]])
    w2 = np.array([[30.1, 30.0]])
    joined, dets = detect.match_detections([w0, w1, w2], match_radius=1.0)
    np.testing.assert_array_equal(joined[:2], w0)                 # image 1 seeds the list
    assert dets[0] == [(0, 0), (1, 0)]                            # inside the radius: joins
    assert dets[1] == [(0, 1)]
    assert dets[2] == [(1, 1), (2, 0)]                            # outside: a new entry, later images may join it
    assert dets[3] == [(1, 2)]
    assert len(joined) == 4


def _img(H, W, b, J=None):
    return Image(pixels=np.zeros((H, W), np.float32), b=b, psf=np.zeros((2, 6)), sky=np.zeros((H, W), np.float32),
                 nelec_per_nmgy=np.ones(H, np.float32), psfmap=ConstantPSFMap(np.ones((51, 51)) / 51 ** 2),
                 wcs_jacobian=np.eye(2) if J is None else J)


def _cat(**kw):
    n = len(kw["npix"])
    base = dict(rms=1.0, thresh=1.3, parent=np.arange(n), pixels=[])
    for k in ("x2", "y2", "xy", "peak"):
        base[k] = np.ones(n)
    base.update({k: np.asarray(v) for k, v in kw.items()})
    return detect.Catalog(**base)


def test_catalog_entry_and_patch_boxes():
    images = [_img(60, 60, 1), _img(60, 60, 3), _img(60, 60, 3)]
    c0 = _cat(npix=[12], xmin=[10], xmax=[19], ymin=[20], ymax=[24], x=[15.0], y=[23.0], a=[3.0], b=[1.5], theta=[0.3],
              flux=[7.0])
    c1 = _cat(npix=[30], xmin=[9], xmax=[20], ymin=[19], ymax=[26], x=[15.1], y=[23.0], a=[4.0], b=[2.0], theta=[0.1],
              flux=[9.0])
    c2 = _cat(npix=[20], xmin=[9], xmax=[20], ymin=[19], ymax=[26], x=[15.0], y=[23.2], a=[4.0], b=[1.0], theta=[0.2],
              flux=[5.0])
    cats = [c0, c1, c2]
    catalog, patches = detect.build_detection_output(images, cats, match_radius=1.0)
    assert len(catalog) == 1
    ce = catalog[0]
    np.testing.assert_array_equal(ce.gal_fluxes, [7.0, 0.0, 9.0, 0.0, 0.0])    # bands 2, 4, 5: no detection
    np.testing.assert_array_equal(ce.star_fluxes, ce.gal_fluxes)
    assert ce.gal_axis_ratio == 0.5 and not ce.is_star and ce.gal_frac_dev == 0.5
    assert ce.gal_angle == 0.1 + detect.x_vs_n_angle(np.eye(2))
    assert abs(ce.gal_radius_px - math.sqrt(8.0) * math.sqrt(2 * math.log(2))) < 1e-15
    # image 1's box: 0-based bounds used as 1-based ranges, dilated by 0.2, enclosed with the 5-pixel box
    wc = ce.pos
    assert tuple(wc) == (15.0, 23.0)
    want = detect.enclose_boxes(((9, 20), (19, 25)), model.box_around_point(images[0], wc, 5.0))
    assert patches[0][0].box == model.clamp_box(want, (60, 60))
    assert patches[0][0].box == ((9, 20), (18, 28))
    # the restatement agrees
    rc = [dict(objects=[dict(npix=int(c.npix[0]), flux=float(c.flux[0]), a=float(c.a[0]), b=float(c.b[0]),
                             theta=float(c.theta[0]), x=float(c.x[0]) - 1, y=float(c.y[0]) - 1, xmin=int(c.xmin[0]),
                             xmax=int(c.xmax[0]), ymin=int(c.ymin[0]), ymax=int(c.ymax[0]))]) for c in cats]
    entries, boxes = R.detect_sources(images, rc, 1.0)
    assert len(entries) == 1
    np.testing.assert_array_equal(entries[0][2], ce.gal_fluxes)
    for n in range(3):
        assert patches[0][n].box == model.clamp_box(boxes[0][n], (60, 60))


def test_image_without_detection_gets_the_five_pixel_box():
    images = [_img(40, 40, 1), _img(40, 40, 2)]
    c0 = _cat(npix=[12], xmin=[10], xmax=[14], ymin=[10], ymax=[14], x=[13.0], y=[13.0], a=[1.0], b=[1.0], theta=[0.0],
              flux=[1.0])
    c1 = _cat(npix=[], xmin=[], xmax=[], ymin=[], ymax=[], x=[], y=[], a=[], b=[], theta=[], flux=[])
    catalog, patches = detect.build_detection_output(images, [c0, c1], match_radius=1.0)
    assert patches[0][1].box == model.clamp_box(model.box_around_point(images[1], catalog[0].pos, 5.0), (40, 40))


def _prototypes(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(celeste_detect_[a-z_]+)\s*\(", src)))


def test_exports_equal_the_header():
    import __graft_entry__ as g
    if not os.path.exists(g.DETECT_LIB):
        g.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", g.DETECT_LIB], text=True)
    syms = sorted(l.split()[-1] for l in out.splitlines() if l.split()[1] == "T")
    assert syms == _prototypes(os.path.join(ROOT, "include", "celeste_detect.h")) == sorted(detect.EXPORTED_SYMBOLS)


def test_no_device_status():
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except ImportError:
        pass
    import __graft_entry__ as g
    if not os.path.exists(g.DETECT_LIB):
        g.build()
    with pytest.raises(detect.DetectError) as e:
        detect.extract([_img(16, 16, 1)])
    assert e.value.status == detect.ERR_NO_DEVICE
