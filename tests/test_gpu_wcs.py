"""-m gpu: tangent-plane (TAN) images through the device's input preparation (libceleste_prep.so after
celeste_prep_images_set_wcs) against the host functions, on the scene of tests/wcs_scene.py: three fields at dec 60 that
straddle RA 0, turned by 0, 30 and 90 degrees, one with flipped parity.  Integers (sources, images, boxes, counts, neighbour
lists, flags, detection lists) are compared exactly; world centres, positions and Jacobians within the bounds measured for the
host against mpmath (tests/test_wcs_host.py), which hold the device against mpmath too."""
import math

import numpy as np
import pytest

import mp_wcs
import wcs_scene
from wcs_scene import BOUND_DEG, BOUND_JAC, OVERRIDE

pytestmark = pytest.mark.gpu

MATCH_RADIUS = 1.0 / 3600.0


@pytest.fixture(scope="module")
def field():
    f = wcs_scene.tan_multifield()
    assert wcs_scene.scene_ok(f)          # the precondition of exact boxes: no pc -/+ r within 1e-6 of a rounding tie
    return f


@pytest.fixture(scope="module")
def field_prep(field):
    from celeste_jl_amd import prep
    with prep.PrepImages(field.images, 0) as pi:
        assert pi.has_tan_wcs
        yield pi


def jac_error(got, want):
    """largest |difference| of [E, 2, 2] Jacobians relative to the largest element of each"""
    if len(got) == 0:
        return 0.0
    return float((np.abs(got - want).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2))).max())


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("override", [math.nan, OVERRIDE])
def test_patch_table_is_the_hosts(field, field_prep, sparse, override):
    from celeste_jl_amd import model, prep
    images, catalog = field.images, field.catalog
    want = model.patch_table(images, catalog, radius_override_pix=override, sparse=sparse)
    got = prep.patch_table(images, catalog, radius_override_pix=override, sparse=sparse, prep_images=field_prep)
    assert (got.n_sources, got.n_images, got.dense) == (want.n_sources, want.n_images, want.dense)
    for name in ("source", "image", "box", "pixel_center", "active_pixels"):      # no entry is left out
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    assert got.neighbors() == want.neighbors() and got.neighbor_lists == want.neighbors()
    e_deg = float(np.abs(got.world_center - want.world_center).max())
    e_jac = jac_error(got.wcs_jacobian, want.wcs_jacobian)
    print("device against host: world centres %.3e degrees, Jacobians %.3e relative" % (e_deg, e_jac))
    assert e_deg <= BOUND_DEG and e_jac <= BOUND_JAC
    E = len(want.source)
    assert (E == len(images) * len(catalog)) == (not sparse) and (want.H2 * want.W2 > 0).sum() >= 40
    if sparse:
        off = wcs_scene.placement(images, catalog)[0]
        assert off and not np.isin(want.source, off).any()


def test_the_device_against_mpmath(field, field_prep):
    """the device's own error: world centres and Jacobians of the sparse table against the 50-digit projection and recipe"""
    from celeste_jl_amd import prep
    images, catalog = field.images, field.catalog
    got = prep.patch_table(images, catalog, sparse=True, prep_images=field_prep)
    e_deg = e_jac = 0.0
    mps = {}
    for e in range(len(got.source)):
        w = images[got.image[e]].wcs
        m = mps.setdefault(id(w), mp_wcs.MpTan(w.crval, w.crpix, w.cd))
        pc = got.pixel_center[e]
        e_deg = max(e_deg, mp_wcs.pix_error(got.world_center[e], m.pix_to_world(pc[0], pc[1])))
        mj = m.jacobian(pc[0], pc[1])
        scale = max(abs(float(x)) for r in mj for x in r)
        e_jac = max(e_jac, max(abs(float(mp_wcs._m(got.wcs_jacobian[e, i, j]) - mj[i][j])) for i in range(2) for j in range(2)) / scale)
    print("device against mpmath: world centres %.3e degrees, Jacobians %.3e relative" % (e_deg, e_jac))
    assert e_deg <= BOUND_DEG and e_jac <= BOUND_JAC


def test_sky_flags_are_the_hosts(field, field_prep):
    import copy
    from celeste_jl_amd import infer, prep
    from celeste_jl_amd.params import CatalogEntry
    images, catalog = field.images, list(field.catalog)
    ce = catalog[0]
    behind = CatalogEntry(np.array([179.9995, -60.0]), ce.is_star, ce.star_fluxes, ce.gal_fluxes, ce.gal_frac_dev, ce.gal_axis_ratio,
                          ce.gal_angle, ce.gal_radius_px)
    catalog.append(behind)
    want = [infer.bad_sky(c, images) for c in catalog]
    assert prep.bad_sky_flags(catalog, images, prep_images=field_prep) == want and want[-1] is False
    # a band-4 image whose lower half is brighter than its claimed sky: both values occur
    bright = [copy.copy(im) for im in images]
    k = next(n for n, im in enumerate(bright) if im.b == 4)
    bright[k].pixels = bright[k].pixels.copy()
    bright[k].pixels[32:] += 40.0
    want = [infer.bad_sky(c, bright) for c in catalog]
    assert True in want and False in want
    assert prep.bad_sky_flags(catalog, bright) == want


@pytest.fixture(scope="module")
def detections(field):
    from celeste_jl_amd import detect
    return detect.extract(field.images)


def test_detected_table_is_build_detection_output(field, field_prep, detections):
    from celeste_jl_amd import detect, model, prep
    images, cats = field.images, detections
    worlds = [detect.world_coords(c, im) for c, im in zip(cats, images)]
    joined, lists = detect.match_detections(worlds, MATCH_RADIUS, angular=True)
    hc, patches = detect.build_detection_output(images, cats, MATCH_RADIUS)
    dc, table = prep.detected_table(images, cats, MATCH_RADIUS, prep_images=field_prep)
    assert len(hc) == len(dc) == len(lists) >= 3 and sum(len(c) for c in cats) > len(hc)       # something was joined
    assert table.detections == lists
    e_pos = max(float(np.abs(a.pos - b.pos).max()) for a, b in zip(hc, dc))
    print("joined positions, device against host: %.3e degrees" % e_pos)
    assert e_pos <= BOUND_DEG
    for a, b in zip(hc, dc):
        assert a.gal_fluxes.tobytes() == b.gal_fluxes.tobytes() and a.gal_axis_ratio == b.gal_axis_ratio
        assert a.gal_angle == b.gal_angle and a.gal_radius_px == b.gal_radius_px
    ent = [(s, n, p) for s, row in enumerate(patches) for n, p in row.nonempty()]          # 15 images: sparse rows
    assert table.source.tolist() == [s for s, _, _ in ent] and table.image.tolist() == [n for _, n, _ in ent]
    assert table.box.tolist() == [[p.box[0][0], p.box[0][1], p.box[1][0], p.box[1][1]] for _, _, p in ent]
    assert table.active_pixels.tolist() == [int(p.active_pixel_bitmap.sum()) for _, _, p in ent]
    assert table.neighbors() == model.neighbor_map(patches)
    wc = np.array([p.world_center for _, _, p in ent])
    jac = np.array([p.wcs_jacobian for _, _, p in ent])
    assert np.abs(table.world_center - wc).max() <= BOUND_DEG and jac_error(table.wcs_jacobian, jac) <= BOUND_JAC


@pytest.mark.parametrize("with_catalog", [True, False], ids=["catalog", "detected"])
def test_infer_box_with_device_prep_is_infer_box(field, with_catalog):
    """single_vi, few iterations; the tolerance is tests/test_gpu_prep.py's for a context whose inputs agree within rounding
    (rtol 1e-9; its identity-WCS comparisons are exact because the inputs are).
    Measured on an MI355X: see DESIGN.md section 16."""
    import celeste_jl_amd as cel
    box = cel.BoundingBox(359.9, 360.1, 59.9, 60.1)
    cfg = cel.ElboConfig(max_iters=6)
    kw = dict(method="single_vi", cfg=cfg)
    if with_catalog:
        off, near = wcs_scene.placement(field.images, field.catalog)
        catalog = [ce for s, ce in enumerate(field.catalog) if s not in off + near]      # the sources that lie in an image
        want = cel.infer_box(field.images, box, catalog, prep="host", **kw)
        got = cel.infer_box(field.images, box, catalog, prep="device", **kw)
    else:
        want = cel.infer_box(field.images, box, match_radius=MATCH_RADIUS, prep="host", **kw)
        got = cel.infer_box(field.images, box, match_radius=MATCH_RADIUS, prep="device", **kw)
    assert len(want) == len(got) >= 3
    worst = 0.0
    for a, b in zip(want, got):
        assert a.is_sky_bad == b.is_sky_bad and a.failed == b.failed
        assert abs(a.init_ra - b.init_ra) <= BOUND_DEG and abs(a.init_dec - b.init_dec) <= BOUND_DEG
        nz = a.vs != 0
        worst = max(worst, float((np.abs(a.vs - b.vs)[nz] / np.abs(a.vs)[nz]).max()))
    print("infer_box device against host prep (%s): largest relative parameter difference %.3e" % (
        "catalog" if with_catalog else "detected", worst))
    for a, b in zip(want, got):
        assert np.allclose(b.vs, a.vs, rtol=1e-9, atol=0)


def test_an_affine_scene_with_set_wcs_kind_0_is_bit_equal():
    from celeste_jl_amd import prep, synthetic
    f = synthetic.make_multifield(grid=(1, 2), H=48, W=48, n_sources=12, seed=5, sparse=True)
    names = ("source", "image", "box", "pixel_center", "world_center", "active_pixels")
    with prep.PrepImages(f.images, 0) as pi:
        assert not pi.has_tan_wcs
        before = [prep.patch_table(f.images, f.catalog, sparse=s, prep_images=pi) for s in (False, True)]
        sky = prep.bad_sky_flags(f.catalog, f.images, prep_images=pi)
        arr = prep.wcs_structs(f.images)
        assert all(arr[n].kind == prep.WCS_AFFINE for n in range(len(f.images)))
        with pytest.raises(prep.PrepError) as ei:           # a count that is not the handle's
            pi.set_wcs(arr, n=len(f.images) - 1)
        assert ei.value.status == prep.ERR_INVALID_ARG
        arr[1].kind = 5
        with pytest.raises(prep.PrepError):
            pi.set_wcs(arr)
        arr[1].kind = prep.WCS_AFFINE
        pi.set_wcs(arr)
        after = [prep.patch_table(f.images, f.catalog, sparse=s, prep_images=pi) for s in (False, True)]
        assert prep.bad_sky_flags(f.catalog, f.images, prep_images=pi) == sky
    for a, b in zip(before, after):
        assert a.wcs_jacobian is None and b.wcs_jacobian is None
        for name in names:
            assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
        assert a.neighbor_lists == b.neighbor_lists


def test_make_field_with_a_tan_wcs_on_the_device():
    from celeste_jl_amd import model, synth, synthetic
    t = math.radians(30.0)
    cd = wcs_scene.SCALE * np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]]) @ np.diag([1.0, -1.0])
    w = model.TanWCS(wcs_scene.CRVAL, (30.5, 35.5), cd)
    f = synthetic.make_field(60, 70, 6, seed=3, margin=5, wcs=w, device=0)
    assert all(im.wcs is w and im.pixels.dtype == np.float32 and np.isfinite(im.pixels).all() for im in f.images)
    got = synth.expected_electrons(f.images, f.catalog)
    for n, im in enumerate(f.images):
        want = synthetic.render_expected_image(im, f.catalog) * im.nelec_per_nmgy.astype(np.float64)[:, None]
        err, scale = np.abs(got[n] - want).max(), np.abs(want).max()
        print("image %d: max |got - ref| = %.3e, max |ref| = %.3e" % (n, err, scale))
        assert want.max() > 1.5 * np.median(want)                    # a source is in the picture
        assert err <= 1e-12 * scale                                   # tests/test_gpu_synth.py's tolerance
