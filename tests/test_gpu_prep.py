"""-m gpu: a box's problem built on the device (celeste_jl_amd.prep, libceleste_prep.so) against the host functions of this
repository: model.patch_table, PatchTable.neighbors, model.get_sky_patches / neighbor_map, infer.bad_sky and
SDSSPSFMap.__call__.  Boxes, centres, counts, neighbour lists and flags are compared exactly, stamps and a rotated
Jacobian's world centres against the rounding bounds stated at the tests.  The scenes are small: edges, ties and empties."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
OVERRIDE = 7.5


def _ce(pos, is_star=True, flux=2000.0, radius=4.0):
    from celeste_jl_amd.params import CatalogEntry
    fl = np.full(5, float(flux))
    return CatalogEntry(np.asarray(pos, float), is_star, fl.copy(), fl * 0.5, 0.1, 0.7, math.pi / 4, float(radius))


def geometry_scene():
    """Three images (two of 64 x 48 in bands 1 and 3 on the same grid; one of 40 x 72, band 4, whose pix0 / world0 shift it
    so that it overlaps the others partly) and 62 sources: hand-placed ones (see the comments) and random ones that reach
    30 px outside.  Image 0 has NaN pixels at a fraction of 0.05, and the box sources[8] has there under OVERRIDE is all NaN."""
    from celeste_jl_amd import synthetic
    rng = np.random.Generator(np.random.PCG64(2024))
    b = synthetic.blank_images(64, 48)
    images = [b[0], b[2], synthetic.blank_images(40, 72)[3]]
    images[2].wcs_world0 = np.array([32.0, -12.0])
    images[2].wcs_pix0 = np.array([2.0, -2.0])                   # pc = pos - (30, -10)
    for im in images:
        im.pixels = rng.normal(100.0, 10.0, im.pixels.shape).astype(np.float32)
    cat = []
    # 0-7: centres within half a pixel of every edge and corner of images 0 / 1 (clamped boxes)
    for pos in ((0.7, 24.3), (64.4, 24.2), (32.3, 0.6), (32.2, 48.4), (0.6, 0.8), (0.9, 48.3), (64.3, 0.7), (64.2, 48.1)):
        cat.append(_ce(pos, flux=30.0))
    # 8, 9 (under OVERRIDE): rows 12..28 and 28..43 -- they share exactly row 28; 8's box in image 0 is all NaN
    cat += [_ce((20.0, 10.0), flux=40.0), _ce((35.7, 10.3), flux=40.0)]
    # 10, 11 (under OVERRIDE): rows 12..28 and 29..44, the same columns: not neighbours
    cat += [_ce((20.0, 36.0), flux=40.0), _ce((36.7, 36.2), flux=40.0)]
    # 12, 13 (under OVERRIDE): columns 2..18 and 18..33 -- they share exactly column 18
    cat += [_ce((50.0, 10.0), flux=40.0), _ce((50.3, 25.3), flux=40.0)]
    # 14: a bright star, 15: a large galaxy (both reach max_radius 25); 16: a faint source with a small radius
    cat += [_ce((31.3, 22.8), flux=1.0e36), _ce((40.4, 30.1), False, flux=5.0e5, radius=30.0), _ce((12.6, 40.7), flux=0.02)]
    # 17: alone under OVERRIDE (only in image 2, far from every other source there)
    cat.append(_ce((66.7, 64.3), flux=20.0))
    # 18-21: up to 30 px outside (empty boxes everywhere or nearly)
    cat += [_ce((-28.3, 10.1)), _ce((93.2, 20.7)), _ce((30.4, -29.6)), _ce((101.1, 90.3), False)]
    # 22, 23: rounding ties under OVERRIDE at integer coordinates (7.5 is exact: pc -/+ 7.5 ends in .5)
    cat += [_ce((10.0, 30.0), flux=25.0), _ce((45.0, 3.0), False, flux=25.0, radius=1.5)]
    while len(cat) < 62:
        pos = (rng.uniform(-30.0, 94.0), rng.uniform(-30.0, 78.0))
        star = bool(rng.random() < 0.5)
        cat.append(_ce(pos, star, flux=float(np.exp(rng.normal(4.0, 2.0))), radius=float(np.exp(rng.normal(0.5, 0.6)))))
    images[0].pixels[rng.random(images[0].pixels.shape) < 0.05] = np.nan
    images[0].pixels[11:28, 1:18] = np.nan                       # rows 12..28, columns 2..18: sources[8]'s box under OVERRIDE
    return images, cat


@pytest.fixture(scope="module")
def scene():
    return geometry_scene()


@pytest.fixture(scope="module")
def scene_prep(scene):
    from celeste_jl_amd import prep
    with prep.PrepImages(scene[0], 0) as pi:
        yield pi


def assert_no_near_ties(images, catalog, sparse):
    """the precondition of exact boxes at the default radius: the device's log may differ from libm's in the last place,
    which moves a box only where pc -/+ r lies within rounding of a tie"""
    from celeste_jl_amd import model
    cache = {}
    for img in images:
        for ce in catalog:
            r = model.choose_patch_radius(ce, img, width_scale=1.2, _cache=cache)
            pc = img.world_to_pix(ce.pos)
            for x in (pc[0] - r, pc[0] + r, pc[1] - r, pc[1] + r):
                assert abs((x - math.floor(x)) - 0.5) >= 1e-9, (ce.pos, r, x)


def assert_tables_equal(got, want):
    assert (got.n_sources, got.n_images, got.dense) == (want.n_sources, want.n_images, want.dense)
    assert got.source.dtype == np.int32 and got.image.dtype == np.int32 and got.box.dtype == np.int64
    for name in ("source", "image", "box", "pixel_center", "active_pixels"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    assert np.array_equal(got.costs(), want.costs())


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("override", [math.nan, OVERRIDE])
def test_patch_table_and_neighbours_are_the_hosts(scene, scene_prep, sparse, override):
    from celeste_jl_amd import model, prep
    images, catalog = scene
    if math.isnan(override):
        assert_no_near_ties(images, catalog, sparse)
    want = model.patch_table(images, catalog, radius_override_pix=override, sparse=sparse)
    got = prep.patch_table(images, catalog, radius_override_pix=override, sparse=sparse, prep_images=scene_prep)
    assert_tables_equal(got, want)
    nb = want.neighbors()
    assert got.neighbors() == nb and got.neighbor_lists == nb
    # identity Jacobians: LU is exact, the world centres are LAPACK's bit for bit
    assert np.array_equal(got.world_center, want.world_center)
    assert not hasattr(got, "stamps")                              # no eigen-PSF in this scene
    # the scene holds what it was built for
    E = len(want.source)
    assert (E == len(images) * len(catalog)) == (not sparse)
    h2, w2 = want.H2, want.W2
    if sparse:
        assert (h2 > 0).all() and (w2 > 0).all() and E < len(images) * len(catalog)
    else:
        assert ((h2 == 0) | (w2 == 0)).sum() > 20
    assert (want.active_pixels < h2 * w2).any() and (want.active_pixels == h2 * w2).any()
    if math.isnan(override):
        r = [model.choose_patch_radius(catalog[k], images[0], width_scale=1.2) for k in (14, 15, 16)]
        assert r[0] == 25 and r[1] == 25 and r[2] < 4
    else:
        assert 9 in nb[8] and 8 in nb[9] and 11 not in nb[10] and 10 not in nb[11] and 13 in nb[12] and 12 in nb[13]
        assert nb[17] == [] and want.costs()[17] > 0
        e8 = np.flatnonzero((want.source == 8) & (want.image == 0))[0]
        assert want.box[e8].tolist() == [12, 28, 2, 18] and want.active_pixels[e8] == 0
        e22 = np.flatnonzero((want.source == 22) & (want.image == 1))[0]
        assert want.box[e22].tolist() == [2, 18, 22, 38]                              # 2.5 -> 2, 17.5 -> 18, 22.5 -> 22, 37.5 -> 38
    # a pair that overlaps in two images is one link
    assert all(len(set(r)) == len(r) and r == sorted(r) for r in got.neighbor_lists)


def test_neighbour_lists_are_neighbor_map_of_get_sky_patches(scene, scene_prep):
    """the object path, on the sparse scene"""
    from celeste_jl_amd import model, prep
    images, catalog = scene
    patches = model.get_sky_patches(images, catalog, radius_override_pix=OVERRIDE, sparse=True)
    got = prep.patch_table(images, catalog, radius_override_pix=OVERRIDE, sparse=True, prep_images=scene_prep)
    assert got.neighbors() == model.neighbor_map(patches)
    k = 0
    for s, row in enumerate(patches):
        for n, p in row.nonempty():
            assert (got.source[k], got.image[k]) == (s, n)
            assert got.box[k].tolist() == [p.box[0][0], p.box[0][1], p.box[1][0], p.box[1][1]]
            assert got.active_pixels[k] == p.active_pixel_bitmap.sum()
            k += 1
    assert k == len(got.source)


def test_world_center_under_a_rotated_jacobian(scene):
    """J = rotation(0.3) diag(0.8, 1.3): the device's LU against Image.pix_to_world within the backward-error bound of a
    2 x 2 solve with partial pivoting, 8 eps cond(J) (|pixel_center - pix0|_inf |J^-1|_inf + |world0|_inf) per component
    (the factor 8 covers the different operation order; no bit equality with LAPACK)"""
    _world_centers_under(scene, rotated_image(0.3))


def rotated_image(angle):
    """56 x 60 under J = rotation(angle) diag(0.8, 1.3)"""
    from celeste_jl_amd import synthetic
    img = synthetic.blank_images(56, 60)[1]
    c, s = math.cos(angle), math.sin(angle)
    img.wcs_jacobian = np.array([[c, -s], [s, c]]) @ np.diag([0.8, 1.3])
    img.wcs_world0 = np.array([-3.5, 7.25])
    img.wcs_pix0 = np.array([4.0, -6.0])
    return img


PIVOT_ANGLE = math.pi / 2 - 1.0e-7


def test_world_center_under_a_jacobian_that_needs_pivoting(scene):
    """a rotation 1e-7 short of a quarter turn: |J21| = 0.8 against |J11| = 8e-8, so the rows are exchanged; without the
    exchange the multiplier J21 / J11 is 1e7 and the solve loses seven digits, far outside the same bound"""
    img = rotated_image(PIVOT_ANGLE)
    assert 0 < abs(img.wcs_jacobian[0, 0]) < 1e-6 * abs(img.wcs_jacobian[1, 0])
    _world_centers_under(scene, img)


def _world_centers_under(scene, img):
    from celeste_jl_amd import prep
    images, catalog = scene
    four = list(images) + [img]
    for sparse in (False, True):
        got = prep.patch_table(four, catalog, sparse=sparse)
        e = np.flatnonzero(got.image == 3)
        assert e.size >= (len(catalog) if not sparse else 10)
        J = img.wcs_jacobian
        Ji = np.linalg.inv(J)
        cond = np.linalg.norm(J, np.inf) * np.linalg.norm(Ji, np.inf)
        worst = 0.0
        for k in e:
            pc = got.pixel_center[k]
            want = img.pix_to_world(pc)
            bound = 8 * EPS * cond * (np.abs(pc - img.wcs_pix0).max() * np.linalg.norm(Ji, np.inf) + np.abs(img.wcs_world0).max())
            err = np.abs(got.world_center[k] - want).max()
            worst = max(worst, err / bound)
            assert err <= bound, (k, err, bound)
        print("rotated Jacobian, sparse=%s: largest error / bound = %.3f over %d entries" % (sparse, worst, e.size))
        # the boxes of that image cover the source's pixel position (a box the wrong way round would not)
        for k in e:
            if got.H2[k] > 0 and got.W2[k] > 0 and got.H2[k] < 56 and got.W2[k] < 60:
                p = img.world_to_pix(catalog[got.source[k]].pos)
                assert got.box[k, 0] - 27 <= p[0] <= got.box[k, 1] + 27 and got.box[k, 2] - 27 <= p[1] <= got.box[k, 3] + 27


def test_a_tried_pair_without_a_positive_flux_is_refused(scene, scene_prep):
    from celeste_jl_amd import model, prep
    images, catalog = scene
    for bad in (0.0, math.nan, -1.0):
        cat = list(catalog)
        cat[30] = _ce((30.0, 20.0), flux=bad)
        for sparse in (False, True):
            with pytest.raises(prep.PrepError) as ei:
                prep.patch_table(images, cat, sparse=sparse, prep_images=scene_prep)
            assert ei.value.status == prep.ERR_INVALID_ARG
            with pytest.raises(AssertionError):
                model.patch_table(images, cat, sparse=sparse)
        # (with a radius override no flux is read)
        assert_tables_equal(prep.patch_table(images, cat, radius_override_pix=OVERRIDE, prep_images=scene_prep),
                            model.patch_table(images, cat, radius_override_pix=OVERRIDE))
    # sparse: a source more than `reach` from every image is not tried, its flux not read -- as on the host
    cat = list(catalog)
    cat[30] = _ce((-40.0, 200.0), flux=0.0)
    assert_tables_equal(prep.patch_table(images, cat, sparse=True, prep_images=scene_prep), model.patch_table(images, cat, sparse=True))
    with pytest.raises(prep.PrepError):
        prep.patch_table(images, cat, sparse=False, prep_images=scene_prep)


def stamp_scene():
    from celeste_jl_amd import synthetic
    from celeste_jl_amd.model import SDSSPSFMap
    rng = np.random.Generator(np.random.PCG64(77))
    images = synthetic.blank_images(70, 66)[:4]
    for im, (ni, nj, nk) in zip(images[:3], ((1, 1, 1), (3, 2, 4), (5, 5, 4))):
        im.psfmap = SDSSPSFMap(rng.normal(0.0, 1.0, (51 * 51, nk)), 51, 51, rng.normal(0.0, 1.0, (ni, nj, nk)))
    # under OVERRIDE: (-6.2, -6.2) has the box 1..1 x 1..1, centre x = y = 1 (every higher power is zero);
    # (76.2, 72.2) the far corner 69..70 x 65..66
    cat = [_ce((-6.2, -6.2)), _ce((76.2, 72.2)), _ce((35.3, 33.1)), _ce((-6.2, 40.0), False), _ce((60.7, 12.4)), _ce((200.0, 10.0))]
    return images, cat


@pytest.mark.parametrize("sparse", [False, True])
def test_stamps_are_the_psf_maps_within_the_dot_product_bound(sparse):
    """|stamp - SDSSPSFMap.__call__| <= 2 (nk + ni nj) eps sum_k |w_k| |rrows[:, k]| per pixel (numpy's einsum and BLAS
    orders are unspecified)"""
    from celeste_jl_amd import model, prep
    images, cat = stamp_scene()
    want = model.patch_table(images, cat, radius_override_pix=OVERRIDE, sparse=sparse)
    got = prep.patch_table(images, cat, radius_override_pix=OVERRIDE, sparse=sparse)
    assert_tables_equal(got, want)
    E = len(got.source)
    e0 = np.flatnonzero((got.source == 0) & (got.image == 1))[0]
    e1 = np.flatnonzero((got.source == 1) & (got.image == 2))[0]
    assert got.pixel_center[e0].tolist() == [1.0, 1.0] and got.pixel_center[e1].tolist() == [69.5, 65.5]
    assert got.stamp.shape == (E,) and got.stamps.shape == (int((got.image < 3).sum()), 51 * 51)
    assert (got.stamp[got.image == 3] == -1).all()
    assert got.stamp[got.image < 3].tolist() == list(range(got.stamps.shape[0]))      # one stamp per entry, in entry order
    worst = 0.0
    for e in np.flatnonzero(got.image < 3):
        m = images[got.image[e]].psfmap
        x, y = got.pixel_center[e]
        ref = np.ascontiguousarray(m(x, y).T).reshape(-1)                             # column-major
        ni, nj, nk = m.cmat.shape
        px = (0.001 * (x - 1.0)) ** np.arange(ni)
        py = (0.001 * (y - 1.0)) ** np.arange(nj)
        w = np.einsum("ijk,i,j->k", m.cmat, px, py)
        bound = 2 * (nk + ni * nj) * EPS * (np.abs(m.rrows) @ np.abs(w))
        err = np.abs(got.stamps[got.stamp[e]] - ref)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (e, float((err / bound).max()))
    print("stamps, sparse=%s: largest error / bound = %.3f over %d stamps" % (sparse, worst, got.stamps.shape[0]))


def sky_scene():
    """A 120 x 130 band-4 image over a band-2 one, pixels around the claimed sky with a slope along the rows, and positions:
    boxes clipped at every border, an odd and an even number of valid pixels, a box that is all NaN, an empty box, two whose
    sky was set so that claimed + 5 lies just below and just above the median, three hand-made ones (an even count whose two
    middle values lie 20 apart with claimed + 5 between their mean and the upper one; claimed + 5 equal to the median bit for
    bit; a row whose nelec_per_nmgy differs from that of the row with the column's index), and 64 random ones."""
    from celeste_jl_amd import infer, synthetic
    rng = np.random.Generator(np.random.PCG64(4))
    images = [synthetic.blank_images(120, 130)[1], synthetic.blank_images(120, 130)[3]]
    img = images[1]
    claimed = float(img.sky[0, 0]) * float(img.nelec_per_nmgy[0])
    slope = np.linspace(-12.0, 22.0, 120)[:, None]
    img.pixels = (claimed + slope + rng.normal(0.0, 6.0, (120, 130))).astype(np.float32)
    img.sky = img.sky.copy()
    img.pixels[0:5, 0:5] = np.nan                                 # the box of (-45, -45): rows 1..5, columns 1..5
    img.pixels[rng.random((120, 130)) < 0.01] = np.nan
    pos = [(2.0, 60.0), (119.4, 60.3), (60.2, 1.7), (60.1, 129.6), (1.2, 1.4), (119.8, 129.9),   # clipped at borders and corners
           (60.3, 65.2), (58.4, 64.7),                                                            # interior: 101 x 101
           (-45.0, -45.0),                                                                        # all NaN
           (-80.0, 40.0), (300.0, 300.0),                                                         # empty
           (40.2, 50.3), (80.3, 70.4),                                                            # claimed + 5 just below / above
           (-46.0, 176.0), (166.0, -46.0), (100.3, 30.2)]                                         # 13, 14, 15: see below
    # 13: rows 1..4, columns 126..130: 20 valid pixels, the middle two at claimed - 8 and claimed + 12
    img.pixels[0:4, 125:130] = (claimed + np.concatenate([-8.0 - np.arange(10), 12.0 + np.arange(10)])).reshape(4, 5).astype(np.float32)
    # 14: rows 116..120, columns 1..4: 19 valid pixels whose median is 571.5; the row's nelec_per_nmgy is 512, the sky under the
    # source 566.5 / 512, so that claimed + 5 is 571.5 exactly
    v = (571.5 + np.concatenate([-3.0 - np.arange(9), [0.0], 3.0 + np.arange(9), [np.nan]])).astype(np.float32)
    img.pixels[115:120, 0:4] = v.reshape(5, 4)
    img.nelec_per_nmgy = img.nelec_per_nmgy.copy()
    img.nelec_per_nmgy[119] = 512.0
    img.sky[119, 0] = np.float32(566.5 / 512.0)
    # 15: row 100 has 1.05 times the nelec_per_nmgy of row 30, and the source lies in column 30
    img.nelec_per_nmgy[99] *= np.float32(1.05)
    pos += [(rng.uniform(-20.0, 140.0), rng.uniform(-20.0, 150.0)) for _ in range(64)]
    cat = [_ce(p) for p in pos]
    from celeste_jl_amd.model import box_around_point, clamp_box, julia_round

    def valid_pixels(ce):
        (h0, h1), (w0, w1) = clamp_box(box_around_point(img, ce.pos, 50.0), (img.H, img.W))
        px = img.pixels[h0 - 1:h1, w0 - 1:w1]
        return px[~np.isnan(px)], (h0, h1, w0, w1)
    # an odd and an even count among the two interior boxes: knock one pixel out of the second if need be
    n6, n7 = valid_pixels(cat[6])[0].size, valid_pixels(cat[7])[0].size
    if n6 % 2 == n7 % 2:
        (h0, h1, w0, w1) = valid_pixels(cat[7])[1]
        free = [(h, w) for h in range(h1 - 3, h1) for w in range(w1 - 3, w1) if not np.isnan(img.pixels[h, w])
                and not (valid_pixels(cat[6])[1][0] <= h + 1 <= valid_pixels(cat[6])[1][1]
                         and valid_pixels(cat[6])[1][2] <= w + 1 <= valid_pixels(cat[6])[1][3])]
        img.pixels[free[0]] = np.nan
    assert valid_pixels(cat[6])[0].size % 2 != valid_pixels(cat[7])[0].size % 2
    # claimed + 5 a few Float32 steps below / above the median, by the sky under the source
    for k, sign in ((11, -1.0), (12, +1.0)):
        med = float(np.median(valid_pixels(cat[k])[0]))
        pc = img.world_to_pix(cat[k].pos)
        h, w = julia_round(pc[0]), julia_round(pc[1])
        target = (med - 5.0) * (1.0 + sign * 4.0e-6)
        img.sky[h - 1, w - 1] = np.float32(target / float(img.nelec_per_nmgy[h - 1]))
    img.sky[0, 129] = np.float32((claimed + 2.0) / float(img.nelec_per_nmgy[0]))          # 13: claimed + 5 = claimed_0 + 7
    want = [infer.bad_sky(ce, images) for ce in cat]
    assert want[11] is True and want[12] is False and want[8] is False and want[9] is False
    # the three hand-made cases hold what they were made for
    px13, box13 = valid_pixels(cat[13])
    lo, hi = np.sort(px13)[[9, 10]]
    c13 = float(img.sky[0, 129]) * float(img.nelec_per_nmgy[0]) + 5
    assert box13 == (1, 4, 126, 130) and px13.size == 20 and hi - lo == 20 and float((lo + hi) * np.float32(0.5)) < c13 < float(hi)
    assert want[13] is False
    px14, box14 = valid_pixels(cat[14])
    assert box14 == (116, 120, 1, 4) and px14.size == 19 and float(np.median(px14)) == 571.5
    assert float(img.sky[119, 0]) * float(img.nelec_per_nmgy[119]) + 5.0 == 571.5 and want[14] is False
    med15 = float(np.median(valid_pixels(cat[15])[0]))
    assert float(img.sky[99, 29]) * float(img.nelec_per_nmgy[29]) + 5 < med15 < float(img.sky[99, 29]) * float(img.nelec_per_nmgy[99]) + 5
    assert want[15] is False
    assert 10 < sum(want) < len(want) - 10                         # both values occur among the random ones too
    return images, cat, want


def test_sky_flags_are_bad_sky(scene, scene_prep):
    from celeste_jl_amd import prep
    images, cat, want = sky_scene()
    got = prep.bad_sky_flags(cat, images)
    assert got == want
    with prep.PrepImages(images, 0) as pi:                          # a reused handle; and a column-major plane
        assert prep.bad_sky_flags(cat, images, prep_images=pi) == want
        assert prep.bad_sky_flags(cat[:3], images, prep_images=pi) == want[:3]
    images[1].pixels = np.asfortranarray(images[1].pixels)
    assert prep.bad_sky_flags(cat, images) == want
    # no band-4 image: every flag false
    assert prep.bad_sky_flags(cat, images[:1]) == [False] * len(cat)
    assert prep.bad_sky_flags(scene[1][:5], scene[0][:2], prep_images=None) == [False] * 5
    assert prep.bad_sky_flags([], images) == []


def test_a_column_major_plane_gives_the_same_table(scene, scene_prep):
    from celeste_jl_amd import prep
    images, catalog = scene
    import copy
    imgs = [copy.copy(im) for im in images]
    imgs[0].pixels = np.asfortranarray(imgs[0].pixels)
    a = prep.patch_table(images, catalog, prep_images=scene_prep)
    b = prep.patch_table(imgs, catalog)
    assert_tables_equal(b, a)
    assert b.neighbor_lists == a.neighbor_lists


def _table_bytes(t):
    parts = [t.source, t.image, t.box, t.pixel_center, t.world_center, t.active_pixels]
    if hasattr(t, "stamps"):
        parts += [t.stamp, t.stamps]
    return [np.ascontiguousarray(p).tobytes() for p in parts] + [repr(t.neighbor_lists).encode()]


def test_results_repeat_bit_for_bit_and_do_not_depend_on_the_source_order(scene, scene_prep):
    from celeste_jl_amd import prep
    images, catalog = scene
    for sparse in (False, True):
        a = prep.patch_table(images, catalog, sparse=sparse, prep_images=scene_prep)
        b = prep.patch_table(images, catalog, sparse=sparse, prep_images=scene_prep)
        assert _table_bytes(a) == _table_bytes(b)
        S = len(catalog)
        r = prep.patch_table(images, catalog[::-1], sparse=sparse, prep_images=scene_prep)
        back = np.lexsort((r.image, S - 1 - r.source))               # the reversed table's entries in (source, image) order
        assert np.array_equal(S - 1 - r.source[back], a.source) and np.array_equal(r.image[back], a.image)
        for name in ("box", "pixel_center", "world_center", "active_pixels"):
            assert np.array_equal(getattr(r, name)[back], getattr(a, name)), name
        assert [sorted(S - 1 - t for t in r.neighbor_lists[S - 1 - s]) for s in range(S)] == a.neighbor_lists
    images2, cat2 = stamp_scene()
    a = prep.patch_table(images2, cat2, radius_override_pix=OVERRIDE)
    b = prep.patch_table(images2, cat2, radius_override_pix=OVERRIDE)
    assert _table_bytes(a) == _table_bytes(b)
    r = prep.patch_table(images2, cat2[::-1], radius_override_pix=OVERRIDE)
    S = len(cat2)
    back = np.lexsort((r.image, S - 1 - r.source))
    ea, er = np.flatnonzero(a.stamp >= 0), back[r.stamp[back] >= 0]
    assert np.array_equal(a.stamps[a.stamp[ea]], r.stamps[r.stamp[er]])
    from celeste_jl_amd import infer  # noqa: F401
    imgs, cat, want = sky_scene()
    assert prep.bad_sky_flags(cat[::-1], imgs) == want[::-1]


# ---- plumbing, end to end ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def multifield():
    from celeste_jl_amd import synthetic
    return synthetic.make_multifield(grid=(1, 2), H=48, W=48, n_sources=12, seed=5, sparse=True)


def _eval(ctx, vp, targets):
    v, d, h, cnt, st = ctx.eval_batch(vp, targets)
    return np.array(v), np.array(d), np.array(h), np.array(cnt), np.array(st)


def test_a_context_built_on_the_device_is_the_hosts(multifield):
    import celeste_jl_amd as cel
    f = multifield
    targets = [0, 3, 5, 8, 11]
    host = cel.FieldContext.from_catalog(f.images, f.catalog, sparse=True)
    dev = cel.FieldContext.from_catalog(f.images, f.catalog, sparse=True, prep_device=0)
    try:
        assert dev.problem.neighbors == host.problem.neighbors and np.array_equal(dev.table.box, host.table.box)
        assert dev.problem.stamps.tobytes() == host.problem.stamps.tobytes()
        a, b = _eval(host, f.vp, targets), _eval(dev, f.vp, targets)
        assert (a[4] == 0).all()
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
    finally:
        host.close(); dev.close()


def test_infer_box_with_device_prep_is_infer_box(multifield):
    import celeste_jl_amd as cel
    f = multifield
    box = cel.BoundingBox(5.0, 40.0, 5.0, 80.0)
    cfg = cel.ElboConfig(max_iters=6)
    want = cel.infer_box(f.images, box, f.catalog, method="single_vi", cfg=cfg, prep="host")
    got = cel.infer_box(f.images, box, f.catalog, method="single_vi", cfg=cfg, prep="device")
    assert len(want) == len(got) >= 3
    for a, b in zip(want, got):
        assert a.vs.tobytes() == b.vs.tobytes() and a.is_sky_bad == b.is_sky_bad and a.failed == b.failed
        assert (a.init_ra, a.init_dec) == (b.init_ra, b.init_dec)


def test_a_variable_psf_context_built_on_the_device(multifield):
    """the device-built context against a host-built problem whose stamp table is the device's: the same inputs, the same
    bits (the stamps themselves are bounded above)"""
    import celeste_jl_amd as cel
    from celeste_jl_amd import cabi, model, prep, synthetic
    f = synthetic.make_field(60, 64, 5, seed=3, variable=True)
    dev = cel.FieldContext.from_catalog(f.images, f.catalog, prep_device=0)
    table = model.patch_table(f.images, f.catalog)
    assert_tables_equal(dev.table, table)
    assert dev.table.stamps.shape == (len(table.source), 51 * 51)
    table.stamp, table.stamps = dev.table.stamp, dev.table.stamps
    nb = table.neighbors()
    assert nb == dev.table.neighbor_lists
    host = cel.FieldContext(f.images, None, nb, problem=cabi.problem_from_table(f.images, table, nb))
    plain = cel.FieldContext.from_catalog(f.images, f.catalog)
    try:
        targets = list(range(5))
        a, b, c = _eval(host, f.vp, targets), _eval(dev, f.vp, targets), _eval(plain, f.vp, targets)
        assert (a[4] == 0).all()
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        # against the host's own stamps: the same problem up to the stamps' rounding
        assert np.allclose(b[0], c[0], rtol=1e-9, atol=0) and np.array_equal(b[3], c[3])
    finally:
        host.close(); dev.close(); plain.close()
    assert prep.last_ms().keys() == set(prep.STAGES)
