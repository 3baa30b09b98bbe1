"""CPU: tangent-plane (TAN) sky coordinates on the host -- model.TanWCS against a 50-digit evaluation of the same projection
(tests/mp_wcs.py), the host tables on a TAN multifield, the angular detection join, and the ABI of celeste_prep_wcs_t.

The accuracy bounds are the errors measured for the host against mpmath, times 10 because libm
differs between machines; none may exceed 1e-8 pixels."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import mp_wcs
import wcs_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALE = 0.396 / 3600.0                      # degrees per pixel
FH, FW = 2048, 1489                         # an SDSS frame
RA0 = 359.9995                              # the frame straddles RA 0
BOUND_PX, BOUND_DEG, BOUND_JAC = wcs_scene.BOUND_PX, wcs_scene.BOUND_DEG, wcs_scene.BOUND_JAC


def frame_cd(rot_deg, flip):
    t = math.radians(rot_deg)
    cd = SCALE * np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]])
    return cd @ np.diag([1.0, -1.0]) if flip else cd


def frame_cases():
    for dec0, rot, flip in itertools.product((0.0, 60.0, -85.0), (0.0, 30.0, 90.0), (False, True)):
        yield (RA0, dec0), ((FH + 1) / 2, (FW + 1) / 2), frame_cd(rot, flip)


def frame_points():
    rng = np.random.default_rng(0)
    return np.concatenate([np.array([[1, 1], [1, FW], [FH, 1], [FH, FW], [(FH + 1) / 2, (FW + 1) / 2], [0.5, 0.5]], float),
                           np.stack([rng.uniform(0.5, FH + 0.5, 10), rng.uniform(0.5, FW + 0.5, 10)], axis=1)])


@pytest.fixture(scope="module")
def measured():
    """the host's largest errors against mpmath over every case, computed once"""
    from celeste_jl_amd import model
    pts = frame_points()
    e = {"px": 0.0, "deg": 0.0, "roundtrip": 0.0, "jac": 0.0}
    for crval, crpix, cd in frame_cases():
        w, m = model.TanWCS(crval, crpix, cd), mp_wcs.MpTan(crval, crpix, cd)
        world = w.pix_to_world(pts)
        back = w.world_to_pix(world)
        J = w.jacobian(pts)
        # continuous around crval (the frame spans 0.23 degrees, 1.3 of RA at dec -85), not wrapped into [0, 360)
        assert (np.abs(world[:, 0] - RA0) < 2.0).all() and (world[:, 0] > 360.0).any()
        for k, p in enumerate(pts):
            e["deg"] = max(e["deg"], mp_wcs.pix_error(world[k], m.pix_to_world(p[0], p[1])))
            e["px"] = max(e["px"], mp_wcs.pix_error(back[k], m.world_to_pix(world[k, 0], world[k, 1])))
            e["roundtrip"] = max(e["roundtrip"], float(np.abs(back[k] - p).max()))
            mj = m.jacobian(p[0], p[1])
            scale = max(abs(float(x)) for r in mj for x in r)
            e["jac"] = max(e["jac"], max(abs(float(mp_wcs._m(J[k, i, j]) - mj[i][j])) for i in range(2) for j in range(2)) / scale)
    print("TanWCS against mpmath: %r" % e)
    return e


def test_projection_agrees_with_the_50_digit_projection(measured):
    assert measured["px"] <= BOUND_PX and measured["deg"] <= BOUND_DEG


def test_round_trip_within_the_bound(measured):
    # the world position is within BOUND_DEG of the true one (1 / SCALE pixels per degree), its pixel within BOUND_PX of its own
    assert measured["roundtrip"] <= BOUND_DEG / SCALE + BOUND_PX <= 1e-8


def test_jacobian_is_the_reference_recipe(measured):
    assert measured["jac"] <= BOUND_JAC


def test_known_answers():
    from celeste_jl_amd import model
    for crval, crpix, cd in frame_cases():
        w = model.TanWCS(crval, crpix, cd)
        assert np.array_equal(w.world_to_pix(np.array(crval)), np.array(crpix))
        assert np.array_equal(w.pix_to_world(np.array(crpix)), np.array(crval))
        anti = np.array([crval[0] - 180.0, -crval[1]])
        assert np.isnan(w.world_to_pix(anti)).all()
        # RA as a and a + 360 (values whose sum with 360 is exact in fp64): only sin and cos of ra - ra0 are used
        # (both branches round ra - ra0 by up to half an ulp of 720 degrees: BOUND_DEG / SCALE pixels)
        a = np.array([[0.25, crval[1] + 0.05], [-0.125, crval[1] - 0.03]])
        b = a + np.array([360.0, 0.0])
        pa, pb = w.world_to_pix(a), w.world_to_pix(b)
        assert np.isfinite(pa).all() and np.abs(pa - pb).max() <= BOUND_DEG / SCALE + BOUND_PX
        # vectorised over [..., 2]
        grid = np.stack(np.meshgrid(np.linspace(1, FH, 3), np.linspace(1, FW, 4), indexing="ij"), axis=-1)
        assert w.pix_to_world(grid).shape == (3, 4, 2) and w.jacobian(grid).shape == (3, 4, 2, 2)
        assert np.array_equal(w.pix_to_world(grid)[1, 2], w.pix_to_world(grid[1, 2]))
    with pytest.raises(ValueError):
        model.TanWCS((10.0, 91.0), (1.0, 1.0), np.eye(2))
    with pytest.raises(ValueError):
        model.TanWCS((10.0, 1.0), (1.0, 1.0), np.ones((2, 2)))
    with pytest.raises(ValueError):
        model.TanWCS((math.nan, 1.0), (1.0, 1.0), np.eye(2))


def test_jacobian_at_crpix_on_the_equator_is_inv_cd():
    """there the projection's derivative is inv(cd) exactly; the recipe's one-sided step of about half a pixel leaves a
    truncation error of second order in the step (measured: 4.6e-10 relative; the bound is 10 times that)"""
    from celeste_jl_amd import model
    for rot, flip in ((0.0, False), (30.0, True)):
        w = model.TanWCS((RA0, 0.0), ((FH + 1) / 2, (FW + 1) / 2), frame_cd(rot, flip))
        err = np.abs(w.jacobian(w.crpix) - w.cdinv).max() / np.abs(w.cdinv).max()
        print("recipe against inv(cd) at crpix, dec0 = 0: %.3e" % err)
        assert err <= 4.6e-9


def test_the_linearisation_at_crpix_misplaces_a_corner_source_at_dec_60():
    """why the feature is needed: an affine WCS -- the one with_tan_wcs leaves in the affine fields, or the reference's own
    Jacobian at crpix -- puts a source at the frame's corner more than a pixel from where the projection puts it"""
    from celeste_jl_amd import model
    w = model.TanWCS((RA0, 60.0), ((FH + 1) / 2, (FW + 1) / 2), frame_cd(0.0, False))
    m = mp_wcs.MpTan(w.crval, w.crpix, w.cd)
    corner = w.pix_to_world(np.array([1.0, 1.0]))
    true = m.world_to_pix(corner[0], corner[1])
    img = model.with_tan_wcs(_blank(8, 8)[0], w)
    assert np.array_equal(img.wcs_jacobian, np.linalg.inv(w.cd)) or np.allclose(img.wcs_jacobian, np.linalg.inv(w.cd), rtol=1e-14)
    lin_cd = model.linear_world_to_pix(img.wcs_jacobian, img.wcs_world0, img.wcs_pix0, corner)
    lin_fd = model.linear_world_to_pix(w.jacobian(w.crpix), w.crval, w.crpix, corner)
    e_cd, e_fd = mp_wcs.pix_error(lin_cd, true), mp_wcs.pix_error(lin_fd, true)
    print("corner source misplaced by %.2f px (inv(cd) at crpix) and %.2f px (the recipe's Jacobian at crpix)" % (e_cd, e_fd))
    assert e_cd > 1.0 and e_fd > 1.0
    assert mp_wcs.pix_error(img.world_to_pix(corner), true) <= BOUND_PX


def _blank(h, w):
    from celeste_jl_amd import synthetic
    return synthetic.blank_images(h, w)


# ---- host tables -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def field():
    return wcs_scene.tan_multifield(perturb=False)


def test_the_scene_holds_what_it_was_built_for(field):
    assert wcs_scene.scene_ok(field)
    off, near = wcs_scene.placement(field.images, field.catalog)
    assert len(off) >= 1 and len(near) >= 1
    assert len(field.images) == 15 and all(im.wcs is not None for im in field.images)
    assert field.images[0].wcs is field.images[4].wcs and field.images[0].wcs is not field.images[5].wcs
    dets = [np.linalg.det(field.images[k].wcs.cd) for k in (0, 5, 10)]
    assert dets[0] > 0 and dets[1] > 0 and dets[2] < 0
    pos = np.array([ce.pos for ce in field.catalog])
    assert (pos[:, 0] < 360.0).any() and (pos[:, 0] > 360.0).any()  # both sides of RA 0, continuous around crval
    assert any(im.pixels.max() > 5 * np.median(im.pixels) for im in field.images)


@pytest.mark.parametrize("override", [math.nan, wcs_scene.OVERRIDE])
def test_host_tables_agree_on_a_tan_multifield(field, override):
    from celeste_jl_amd import model
    images, catalog = field.images, field.catalog
    dense = model.get_sky_patches(images, catalog, radius_override_pix=override)
    rows = model.get_sky_patches(images, catalog, radius_override_pix=override, sparse=True)
    td = model.patch_table(images, catalog, radius_override_pix=override)
    ts = model.patch_table(images, catalog, radius_override_pix=override, sparse=True)
    assert len(td.source) == len(images) * len(catalog) and 0 < len(ts.source) < len(td.source)
    assert td.wcs_jacobian.shape == (len(td.source), 2, 2) and ts.wcs_jacobian.shape == (len(ts.source), 2, 2)
    for e in range(len(td.source)):
        p = dense[td.source[e]][td.image[e]]
        assert td.box[e].tolist() == [p.box[0][0], p.box[0][1], p.box[1][0], p.box[1][1]]
        assert np.array_equal(td.pixel_center[e], p.pixel_center) and np.array_equal(td.world_center[e], p.world_center)
        assert np.array_equal(td.wcs_jacobian[e], p.wcs_jacobian) and td.active_pixels[e] == p.active_pixel_bitmap.sum()
        q = model.ImagePatch.from_box(images[td.image[e]], p.box)
        assert np.array_equal(q.wcs_jacobian, p.wcs_jacobian) and np.array_equal(q.world_center, p.world_center)
    ent = [(s, n, p) for s, row in enumerate(rows) for n, p in row.nonempty()]
    assert ts.source.tolist() == [s for s, _, _ in ent] and ts.image.tolist() == [n for _, n, _ in ent]
    for e, (s, n, p) in enumerate(ent):
        assert ts.box[e].tolist() == [p.box[0][0], p.box[0][1], p.box[1][0], p.box[1][1]]
        assert np.array_equal(ts.wcs_jacobian[e], p.wcs_jacobian) and np.array_equal(ts.world_center[e], p.world_center)
    keep = (td.H2 > 0) & (td.W2 > 0)
    assert np.array_equal(td.box[keep], ts.box) and np.array_equal(td.wcs_jacobian[keep], ts.wcs_jacobian)
    assert td.neighbors() == model.neighbor_map(dense) == ts.neighbors() == model.neighbor_map(rows)
    # per-patch Jacobians differ across a frame, and between the turned fields by far more
    j0 = ts.wcs_jacobian[ts.image == 0]
    assert len(j0) >= 2 and np.abs(j0 - j0[0]).max() > 0
    assert np.abs(ts.wcs_jacobian[ts.image == 5][0] - j0[0]).max() > 100.0
    # an empty row's patch is the image's empty patch, with a Jacobian of its own
    off = wcs_scene.placement(images, catalog)[0][0]
    assert rows[off].nonempty().__len__() == 0 and rows[off][3].wcs_jacobian.shape == (2, 2)


def test_the_affine_path_is_untouched():
    """Image.wcs is None: the methods are the affine expressions, a table carries no Jacobians, fields are what they were"""
    from celeste_jl_amd import model, synthetic
    f = synthetic.make_multifield(grid=(1, 2), H=40, W=40, n_sources=6, seed=5, sparse=True)
    img = f.images[5]
    assert img.wcs is None
    pos = np.array([ce.pos for ce in f.catalog])
    assert np.array_equal(img.world_to_pix(pos), (pos - img.wcs_world0) @ img.wcs_jacobian.T + img.wcs_pix0)
    assert np.array_equal(img.world_to_pix(pos[2]), img.wcs_jacobian @ (pos[2] - img.wcs_world0) + img.wcs_pix0)
    assert np.array_equal(img.jacobian_at(np.array([3.0, 4.0])), img.wcs_jacobian)
    assert model.patch_table(f.images, f.catalog, sparse=True).wcs_jacobian is None
    g = synthetic.make_field(60, 64, 3, seed=2)
    assert all(im.wcs is None for im in g.images) and all(26 < ce.pos[0] < 34 for ce in g.catalog)


def test_make_field_with_a_tan_wcs_and_the_location_box():
    from celeste_jl_amd import mcmc, model, synthetic
    w = model.TanWCS((RA0, 60.0), (20.5, 22.5), frame_cd(30.0, True))
    f = synthetic.make_field(40, 44, 3, seed=2, margin=8, wcs=w)
    g = synthetic.make_field(40, 44, 3, seed=2, margin=8)
    for a, b in zip(f.catalog, g.catalog):
        assert np.abs(w.world_to_pix(a.pos) - b.pos).max() <= BOUND_DEG / SCALE + BOUND_PX     # (a round trip)
    assert all(im.wcs is w for im in f.images) and f.patches[0][0].wcs_jacobian.shape == (2, 2)
    box = mcmc.image_location_box(f.images[0], f.catalog[0].pos)
    pix = w.world_to_pix(f.catalog[0].pos)
    lo, hi = w.pix_to_world(pix - 1.0), w.pix_to_world(pix + 1.0)
    assert np.allclose(box, [min(lo[0], hi[0]), max(lo[0], hi[0]), min(lo[1], hi[1]), max(lo[1], hi[1])], rtol=0, atol=1e-12)
    assert box[0] < f.catalog[0].pos[0] < box[1] and box[2] < f.catalog[0].pos[1] < box[3]


# ---- detection join ----------------------------------------------------------------------------------------------------------
def test_angular_separation_known_answers():
    from celeste_jl_amd import detect
    assert detect.angular_separation(10.0, 0.0, 11.0, 0.0) == pytest.approx(1.0, abs=1e-13)
    assert detect.angular_separation(10.0, 60.0, 10.0, 61.5) == pytest.approx(1.5, abs=1e-13)
    assert detect.angular_separation(0.0, 90.0, 123.0, -90.0) == pytest.approx(180.0, abs=1e-12)
    assert detect.angular_separation(359.9999, 0.0, 0.0001, 0.0) == pytest.approx(0.0002, abs=1e-13)
    d = detect.angular_separation(np.array([10.0, 20.0]), 60.0, np.array([10.0, 20.0]) + 1e-3, 60.0)
    assert np.allclose(d, 1e-3 * math.cos(math.radians(60.0)), rtol=1e-6)


def test_angular_join_at_dec_60_and_across_ra_0():
    from celeste_jl_amd import detect
    r = 1.0 / 3600.0
    arc = 1.0 / 3600.0 / math.cos(math.radians(60.0))              # RA difference of one arc second on the sky at dec 60
    a = np.array([[10.0, 60.0], [200.0, 60.0], [359.9999, 60.0]])
    b = np.array([[10.0 + 0.9 * arc, 60.0],                         # 0.9": raw RA difference 1.8 / 3600 > r
                  [200.0 + 1.1 * arc, 60.0],                        # 1.1": separate
                  [359.9999 + 0.9 * arc - 360.0, 60.0]])            # 0.9", on the other side of RA 0
    assert b[0, 0] - a[0, 0] > r and b[2, 0] < 1.0
    sep = detect.angular_separation(a[:, 0], a[:, 1], b[:, 0], b[:, 1]) * 3600.0
    assert np.allclose(sep, [0.9, 1.1, 0.9], rtol=1e-4)
    joined, dets = detect.match_detections([a, b], r, angular=True)
    assert dets == [[(0, 0), (1, 0)], [(0, 1)], [(0, 2), (1, 2)], [(1, 1)]] and len(joined) == 4
    assert np.array_equal(joined[3], b[1])
    # the planar distance gets the first and the third wrong
    joined_p, dets_p = detect.match_detections([a, b], r)
    assert dets_p == [[(0, 0)], [(0, 1)], [(0, 2)], [(1, 0)], [(1, 1)], [(1, 2)]]
    # a tie goes to the lowest index; a later image never joins an entry of its own image
    c = np.array([[50.0, 10.0], [50.0, 10.0]])
    assert detect.match_detections([c, c[:1]], r, angular=True)[1] == [[(0, 0), (1, 0)], [(0, 1)]]
    assert detect.match_detections([c[:1], c], r, angular=True)[1] == [[(0, 0), (1, 0), (1, 1)]]


def test_build_detection_output_joins_by_angle_when_an_image_is_tan(field):
    from celeste_jl_amd import detect
    images = [field.images[2], field.images[7]]                     # the r bands of fields 0 and 1 (turned by 30 degrees)
    arc = 1.0 / 3600.0 / math.cos(math.radians(60.0))
    grid = np.stack(np.meshgrid(np.arange(8.0, 60.0, 4.0), np.arange(8.0, 76.0, 4.0), indexing="ij"), axis=-1).reshape(-1, 2)
    other = images[1].world_to_pix(images[0].pix_to_world(grid))
    both = np.flatnonzero((other[:, 0] > 8) & (other[:, 0] < 56) & (other[:, 1] > 8) & (other[:, 1] < 72))
    sky = images[0].pix_to_world(grid[both[0]] + 0.3)               # a sky position well inside both images
    pix0 = images[0].world_to_pix(sky)
    pix1 = images[1].world_to_pix(sky + np.array([0.9 * arc, 0.0]))
    assert 1 < pix0[0] < 64 and 1 < pix1[0] < 64 and 1 < pix0[1] < 80 and 1 < pix1[1] < 80

    def cat(p):
        one = lambda v, t=np.float64: np.array([v], dtype=t)
        x, y = int(round(p[0])) - 1, int(round(p[1])) - 1
        return detect.Catalog(1.0, 1.0, one(9, np.int64), one(x - 1, np.int64), one(x + 1, np.int64), one(y - 1, np.int64),
                              one(y + 1, np.int64), one(p[0]), one(p[1]), one(1.0), one(1.0), one(0.0), one(1.5), one(1.0),
                              one(0.3), one(100.0), one(30.0), one(-1, np.int64))
    catalog, patches = detect.build_detection_output(images, [cat(pix0), cat(pix1)], 1.0 / 3600.0)
    assert len(catalog) == 1 and np.abs(catalog[0].pos - sky).max() < 1e-9
    assert patches[0][0].active_pixel_bitmap.size > 0 and patches[0][1].active_pixel_bitmap.size > 0
    assert np.abs(patches[0][1].wcs_jacobian - patches[0][0].wcs_jacobian).max() > 100.0


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
SIZES_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "celeste_prep.h"
#define OFF(T, f) printf("offsetof " #T " " #f " %zu\n", offsetof(T, f))
int main(void) {
    printf("sizeof celeste_prep_wcs_t %zu\n", sizeof(celeste_prep_wcs_t));
    OFF(celeste_prep_wcs_t, kind); OFF(celeste_prep_wcs_t, crval); OFF(celeste_prep_wcs_t, crpix); OFF(celeste_prep_wcs_t, cd);
    printf("kinds %d %d version %d\n", CELESTE_PREP_WCS_AFFINE, CELESTE_PREP_WCS_TAN, CELESTE_PREP_ABI_VERSION);
    return 0;
}
"""


@pytest.fixture(scope="module")
def plib(lib):
    import __graft_entry__ as g
    if not os.path.exists(g.PREP_LIB):
        g.build()
    from celeste_jl_amd import prep
    return prep.load_library()


def test_wcs_struct_has_the_layout_a_c_compiler_gives_the_header(tmp_path):
    from celeste_jl_amd import prep
    src, exe = tmp_path / "wcs_sizes.c", tmp_path / "wcs_sizes"
    src.write_text(SIZES_C)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    assert int(re.search(r"sizeof celeste_prep_wcs_t (\d+)", out).group(1)) == C.sizeof(prep.PrepWcsT) == 72
    offs = re.findall(r"offsetof (\w+) (\w+) (\d+)", out)
    assert {f for _, f, _ in offs} == {f for f, _ in prep.PrepWcsT._fields_} - {"reserved"}
    for _, f, n in offs:
        assert getattr(prep.PrepWcsT, f).offset == int(n), f
    assert "kinds %d %d version %d" % (prep.WCS_AFFINE, prep.WCS_TAN, prep.ABI_VERSION) in out


def test_set_wcs_refusals_without_a_device(plib, field):
    from celeste_jl_amd import prep
    INV = prep.ERR_INVALID_ARG
    images = field.images[:3]
    arr = prep.wcs_structs(images)
    assert arr[0].kind == prep.WCS_TAN and arr[0].crval[0] == images[0].wcs.crval[0] and arr[0].cd[1] == images[0].wcs.cd[0, 1]
    assert plib.celeste_prep_wcs_check(3, arr) == 0
    mixed = prep.wcs_structs([images[0]] + _blank(8, 8)[:1])
    assert mixed[1].kind == prep.WCS_AFFINE and plib.celeste_prep_wcs_check(2, mixed) == 0
    assert plib.celeste_prep_wcs_check(0, arr) == INV and plib.celeste_prep_wcs_check(-1, arr) == INV
    assert plib.celeste_prep_wcs_check(3, None) == INV
    # no handle: refused, whatever the rest holds (a count that is not the handle's needs a handle: tests/test_gpu_wcs.py)
    assert plib.celeste_prep_images_set_wcs(None, 3, arr) == INV
    assert plib.celeste_prep_result_get_jacobians(None, None) == INV

    def broken(change):
        a = prep.wcs_structs(images)
        change(a[1])
        return plib.celeste_prep_wcs_check(3, a)
    for field_name, n in (("crval", 2), ("crpix", 2), ("cd", 4)):
        for k in range(n):
            for bad in (math.nan, math.inf, -math.inf):
                def change(w, f=field_name, k=k, bad=bad):
                    getattr(w, f)[k] = bad
                assert broken(change) == INV, (field_name, k, bad)

    def singular(w):
        w.cd[0], w.cd[1], w.cd[2], w.cd[3] = 1e-4, 2e-4, 2e-4, 4e-4
    assert broken(singular) == INV

    def zero(w):
        w.cd[0] = w.cd[1] = w.cd[2] = w.cd[3] = 0.0
    assert broken(zero) == INV
    for dec in (90.0000001, -91.0, 1000.0):
        def pole(w, dec=dec):
            w.crval[1] = dec
        assert broken(pole) == INV, dec

    def at_pole(w):
        w.crval[1] = -90.0
    assert broken(at_pole) == 0
    for kind in (2, -1, 7):
        def unknown(w, kind=kind):
            w.kind = kind
        assert broken(unknown) == INV, kind

    def affine_ignores(w):          # the other fields of an AFFINE entry are not read
        w.kind = prep.WCS_AFFINE
        w.cd[0] = math.nan
    assert broken(affine_ignores) == 0
