"""-m gpu: detections joined, and their catalog and patch table built, on the device (prep.detected_table,
detect.detect_table, infer_box(..., prep="device") without a catalog) against the host path as it stands:
detect.match_detections, detect.catalog_entry, detect.build_detection_output and model.neighbor_map.

Under an identity or offset-only WCS everything is compared exactly, integers and doubles bit for bit.  The join can differ
from the host's only where a distance lies within rounding of match_radius or of the runner-up's distance (the host takes
np.hypot, the device sqrt(dx dx + dy dy)), so every scene keeps separations of 0.01 or more and `assert_join_margin` asserts,
over all detections of later images, min(|d1 - match_radius|, d2 - d1) > 1e-9 with the host's own distances: no detection is
left out of any comparison."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


# ---- scenes (host only) ------------------------------------------------------------------------------------------------
def make_catalog(rows):
    """a detect.Catalog from (x, y, npix, (xmin, xmax, ymin, ymax) or None, a, b, theta, flux) rows; bounds default to the
    3 x 3 pixels around the centroid (0-based, as SEP leaves them)"""
    from celeste_jl_amd.detect import Catalog
    n = len(rows)
    z = np.zeros(n)
    f = {k: [] for k in ("x", "y", "npix", "xmin", "xmax", "ymin", "ymax", "a", "b", "theta", "flux")}
    for x, y, npix, bounds, a, b, theta, flux in rows:
        if bounds is None:
            bounds = (int(round(x)) - 2, int(round(x)), int(round(y)) - 2, int(round(y)))
        for k, v in zip(("x", "y", "npix", "xmin", "xmax", "ymin", "ymax", "a", "b", "theta", "flux"),
                        (x, y, npix) + tuple(bounds) + (a, b, theta, flux)):
            f[k].append(v)
    ints = {k: np.array(f[k], dtype=np.int64) for k in ("npix", "xmin", "xmax", "ymin", "ymax")}
    dbl = {k: np.array(f[k], dtype=np.float64) for k in ("x", "y", "a", "b", "theta", "flux")}
    return Catalog(rms=1.0, thresh=1.3, x2=z, y2=z, xy=z, peak=z, parent=np.full(n, -1), **ints, **dbl)


def _row(k, x, y, npix, bounds=None):
    """a detection whose shape and flux are its own (k numbers it)"""
    return (x, y, npix, bounds, 2.0 + 0.13 * k, 1.0 + 0.07 * k, 0.1 * k - 0.7, 50.0 + 3.5 * k)


def _images(bands, H, W, seed):
    from celeste_jl_amd import synthetic
    rng = np.random.Generator(np.random.PCG64(seed))
    images = []
    for b in bands:
        im = synthetic.blank_images(H, W)[b - 1]
        im.pixels = rng.normal(100.0, 10.0, (H, W)).astype(np.float32)
        images.append(im)
    return images


JOIN_RADIUS = 2.0


def join_scene():
    """Five 60 x 60 images in bands 4, 3, 1, 3, 2 on one grid; match_radius 2.
    image 0: no detection, so the list starts from image 1: entries 0, 1, 2.  image 2: empty, in the middle.
    image 3 (band 3, as image 1): detections 0 and 1 both join entry 0 at distance 0.5 (the box comes from 1; 0 has entry
      0's npix in band 3: image 1's wins); 2 and 3 lie 1.17 apart, far from every entry: both are appended (entries 3, 4);
      4 joins entry 1 with the npix entry 1 has in band 3.
    image 4 (band 2): 0 lies between entries 3 and 4 and joins the nearer, 3; 1 joins entry 1 with the npix that entry has in
      band 3 (equal best npix in two bands: band 2 gives the shape); 2 joins entry 2; 3 is new (entry 5: band 2 only)."""
    images = _images((4, 3, 1, 3, 2), 60, 60, 11)
    cats = [make_catalog([]),
            make_catalog([_row(1, 10.0, 10.0, 20), _row(2, 30.0, 30.0, 12), _row(3, 50.0, 12.0, 9)]),
            make_catalog([]),
            make_catalog([_row(4, 10.3, 10.4, 20, (7, 13, 8, 12)), _row(5, 9.6, 9.7, 15, (2, 20, 5, 15)), _row(6, 40.0, 45.0, 8),
                          _row(7, 41.0, 45.6, 30), _row(8, 30.2, 30.1, 12)]),
            make_catalog([_row(9, 40.4, 45.1, 11), _row(10, 30.0, 30.3, 12), _row(11, 50.2, 12.1, 7), _row(12, 20.0, 50.0, 6)])]
    return images, cats


TIE_RADIUS = 6.0


def tie_scene():
    """Three 60 x 60 images in bands 3, 2, 1 on one grid, every coordinate an integer, so that both the host's np.hypot and the
    device's sqrt(dx dx + dy dy) are exact; match_radius 6.
    image 0: entries 0 (10, 10), 1 (16, 18), 2 (40, 40).
    image 1: detection 0 at (13, 14) lies exactly 5 from entries 0 and 1: the lower index takes it; detection 1 at (40, 46) lies
      exactly 6 = match_radius from entry 2: not closer than the radius, so it is appended (entry 3).
    image 2: detection 0 at (40, 43) lies 3 from entries 2 and 3 alike: entry 2 takes it."""
    images = _images((3, 2, 1), 60, 60, 15)
    cats = [make_catalog([_row(1, 10.0, 10.0, 20), _row(2, 16.0, 18.0, 12), _row(3, 40.0, 40.0, 9)]),
            make_catalog([_row(4, 13.0, 14.0, 15), _row(5, 40.0, 46.0, 8)]),
            make_catalog([_row(6, 40.0, 43.0, 11)])]
    return images, cats


def rotate(images):
    c, s = math.cos(0.3), math.sin(0.3)
    for im in images:
        im.wcs_jacobian = np.array([[c, -s], [s, c]]) @ np.diag([0.8, 1.3])
        im.wcs_world0 = np.array([-3.5, 7.25])
        im.wcs_pix0 = np.array([4.0, -6.0])
    return images


def lattice_scene():
    """More joined entries than one LDS tile and more detections in a later image than one workgroup: image 0 holds a jittered
    lattice of more than MATCH_TILE detections (spacing 11.5, jitter 2), image 1 more than MATCH_BLOCK detections -- two out of
    three next to an entry (within 0.7), among them entries of the second tile, the others at cell centres (appended) --,
    image 2 detections next to appended entries and new ones."""
    from celeste_jl_amd import prep
    rng = np.random.Generator(np.random.PCG64(5))
    side = int(math.ceil(math.sqrt(prep.MATCH_TILE + 76)))
    W = int(side * 11.5 + 10)
    images = _images((3, 2, 3), W, W, 12)
    base = np.array([(6.0 + 11.5 * i, 6.0 + 11.5 * j) for i in range(side) for j in range(side)])
    p0 = base + np.round(rng.uniform(-2.0, 2.0, base.shape), 2)
    n1 = prep.MATCH_BLOCK + 44
    pick = rng.permutation(len(p0))[:n1]
    pick[:8] = len(p0) - 1 - np.arange(8)              # the last entries of the list: the second tile
    rows1, rows2 = [], []
    for k, i in enumerate(pick):
        if k % 3 < 2:
            pos = p0[i] + np.round(rng.uniform(0.05, 0.5, 2), 2) * rng.choice([-1.0, 1.0], 2)
        else:
            pos = base[i] + 5.75 + np.round(rng.uniform(-0.5, 0.5, 2), 2)
        rows1.append(_row(k % 40, float(pos[0]), float(pos[1]), 5 + k % 9))
    pos1 = np.array([(r[0], r[1]) for r in rows1])
    for k in range(60):
        if k % 2 == 0:
            i = 2 + 3 * (k // 2)                       # an appended detection of image 1
            pos = pos1[i] + np.round(rng.uniform(0.05, 0.4, 2), 2)
        else:
            pos = p0[rng.integers(len(p0))] + np.round(rng.uniform(0.05, 0.4, 2), 2) * np.array([1.0, -1.0])
        rows2.append(_row(k % 17, float(pos[0]), float(pos[1]), 4 + k % 5))
    cats = [make_catalog([_row(k % 31, float(x), float(y), 5 + k % 13) for k, (x, y) in enumerate(p0)]),
            make_catalog(rows1), make_catalog(rows2)]
    return images, cats


def box_scene():
    """Dense: three 60 x 60 images, bands 1, 2, 3; image 2 without detections (the 5-pixel box everywhere).
    0, 1, 2: row ranges of 5, 15 and 25 pixels (half-dilations 0.5, 1.5, 2.5: 0, 2, 2 -- ties to even), the 25 one larger than
       the 5-pixel box, the others inside it or not; 3: a 3 x 3 detection, smaller than the 5-pixel box
    4 .. 7: clamped at the first row, the last row, the first column, the last column (bounds that run over the edge)
    8, 9: rows 15 .. 25 and 25 .. 35 in the same columns: they touch; 10, 11: rows 15 .. 25 and 26 .. 36: they do not
    12: its box in image 0 holds NaN pixels; 13: its box in image 0 is all NaN"""
    images = _images((1, 2, 3), 60, 60, 13)
    rows0 = [_row(0, 12.2, 30.4, 9, (10, 14, 28, 32)), _row(1, 30.3, 30.2, 40, (23, 37, 28, 32)), _row(2, 45.4, 30.1, 70, (33, 57, 20, 44)),
             _row(3, 22.4, 41.3, 9, None),
             _row(4, 2.3, 20.2, 12, (0, 6, 18, 22)), _row(5, 59.2, 22.3, 12, (55, 59, 20, 24)), _row(6, 33.1, 1.6, 12, (30, 35, 0, 3)),
             _row(7, 40.3, 59.4, 12, (38, 42, 54, 59)),
             _row(8, 20.0, 10.0, 9, None), _row(9, 30.0, 10.0, 9, None), _row(10, 20.0, 52.0, 9, None), _row(11, 31.0, 52.0, 9, None),
             _row(12, 50.3, 8.2, 9, None), _row(13, 8.3, 48.4, 9, (6, 9, 46, 50))]
    # image 1 sees some of them again, a little off, with bounds of its own (the later detection's box is image 1's own)
    rows1 = [_row(14, 12.4, 30.3, 11, (9, 15, 27, 33)), _row(15, 45.2, 30.2, 50, (30, 54, 25, 39)), _row(16, 2.1, 20.4, 12, (0, 4, 17, 23)),
             _row(17, 20.1, 10.1, 9, (18, 20, 8, 10)), _row(18, 55.0, 55.0, 9, None)]
    images[0].pixels[47:52, 4:9] = np.nan
    images[0].pixels[0:16, 40:56] = np.nan               # 13: rows 3 .. 13, columns 43 .. 53 at the least
    return images, [make_catalog(rows0), make_catalog(rows1), make_catalog([])]


def sparse_scene():
    """Nine 40 x 40 images on a 3 x 3 grid of world offsets (step 30: neighbours overlap by 10), bands cycling; world points
    over the whole area, each detected in every image that holds it (with a small per-image shift), so that most 5-pixel boxes
    fall off most images and those pairs have no entry."""
    rng = np.random.Generator(np.random.PCG64(14))
    images = _images(tuple(1 + (k % 5) for k in range(9)), 40, 40, 15)
    for k, im in enumerate(images):
        im.wcs_world0 = np.array([30.0 * (k // 3), 30.0 * (k % 3)])
        im.wcs_pix0 = np.array([0.0, 0.0])
    images[4].pixels[rng.random((40, 40)) < 0.1] = np.nan
    pts = np.array([(6.0 + 9.0 * i, 5.0 + 9.5 * j) for i in range(10) for j in range(10)])
    pts = pts + np.round(rng.uniform(-1.5, 1.5, pts.shape), 2)
    cats = []
    for k, im in enumerate(images):
        rows = []
        for t, w in enumerate(pts):
            p = w - im.wcs_world0 + np.array([0.02 * k, -0.03 * k])
            if 1.5 <= p[0] <= 39.5 and 1.5 <= p[1] <= 39.5 and (t + k) % 7 != 0:
                hw = 1 + (t + k) % 4
                rows.append(_row((t + 3 * k) % 23, float(p[0]), float(p[1]), 5 + (t * 7 + k) % 11,
                                 (int(p[0]) - hw, int(p[0]) + hw, int(p[1]) - 2, int(p[1]) + hw)))
        cats.append(make_catalog(rows))
    return images, cats


# ---- the yardstick: the host path ------------------------------------------------------------------------------------
def assert_join_margin(worlds, joined, detections, match_radius):
    """over all detections of later images: min(|d1 - match_radius|, d2 - d1) > 1e-9, distances as the host takes them"""
    first_image = np.array([d[0][0] for d in detections], dtype=np.int64)
    checked = 0
    for i in range(1, len(worlds)):
        ref = joined[:int((first_image < i).sum())]
        if ref.shape[0] == 0:
            continue
        for w in np.asarray(worlds[i]).reshape(-1, 2):
            d = np.sort(np.hypot(ref[:, 0] - w[0], ref[:, 1] - w[1]))
            d2 = d[1] if d.size > 1 else math.inf
            assert min(abs(d[0] - match_radius), d2 - d[0]) > 1e-9, (i, w, d[:2])
            checked += 1
    return checked


def host_path(images, cats, match_radius, exact_distances=False):
    """exact_distances: the scene's world coordinates are integers, so its distances are exact on both sides and may be equal
    to one another and to match_radius: asserted in place of the margin"""
    from celeste_jl_amd import detect, model
    worlds = [detect.world_coords(c, im) for c, im in zip(cats, images)]
    joined, detections = detect.match_detections(worlds, match_radius)
    if exact_distances:
        assert all((np.asarray(w) == np.rint(w)).all() and np.abs(w).max(initial=0) < 2 ** 20 for w in worlds)
        checked = 0
    else:
        checked = assert_join_margin(worlds, joined, detections, match_radius)
    catalog, patches = detect.build_detection_output(images, cats, match_radius)
    return dict(worlds=worlds, joined=joined, detections=detections, checked=checked, catalog=catalog, patches=patches,
                neighbors=model.neighbor_map(patches) if patches else [])


def host_entries(images, patches):
    """(source, image, patch) in (source, image) order: every pair of a dense row, the stored pairs of a sparse one"""
    from celeste_jl_amd.model import PatchRow
    out = []
    for s, row in enumerate(patches):
        if isinstance(row, PatchRow):
            out += [(s, n, p) for n, p in row.nonempty()]
        else:
            out += [(s, n, row[n]) for n in range(len(images))]
    return out


def assert_no_box_ties(images, joined):
    """the precondition of equal boxes under a Jacobian that is not the identity: the joined positions differ from the host's
    in the last places, which moves a box only where pc -/+ 5 lies within rounding of a tie"""
    for im in images:
        for w in joined:
            pc = im.world_to_pix(w)
            for x in (pc[0] - 5.0, pc[0] + 5.0, pc[1] - 5.0, pc[1] + 5.0):
                assert abs((x - math.floor(x)) - 0.5) >= 1e-9, (w, x)


def world_bound(im, pix):
    """the backward-error bound of a 2 x 2 solve with partial pivoting that tests/test_gpu_prep.py uses for world_center"""
    J = np.asarray(im.wcs_jacobian)
    Ji = np.linalg.inv(J)
    cond = np.linalg.norm(J, np.inf) * np.linalg.norm(Ji, np.inf)
    return 8 * EPS * cond * (np.abs(np.asarray(pix) - im.wcs_pix0).max() * np.linalg.norm(Ji, np.inf) + np.abs(im.wcs_world0).max())


def assert_is_host_path(images, cats, match_radius, catalog, table, want, exact=True):
    """everything the device returned against the host path `want` (host_path)"""
    S = len(want["catalog"])
    assert len(catalog) == S == table.n_sources and table.n_images == len(images)
    assert table.dense == (len(images) <= 8)
    # the join: lists and positions
    assert table.detections == [[(int(i), int(j)) for i, j in d] for d in want["detections"]]
    pos = np.array([ce.pos for ce in catalog]).reshape(-1, 2)
    if exact:
        assert pos.tobytes() == np.ascontiguousarray(want["joined"]).tobytes()
    else:
        for s in range(S):
            i, j = want["detections"][s][0]
            assert np.abs(pos[s] - want["joined"][s]).max() <= world_bound(images[i], (cats[i].x[j], cats[i].y[j])), s
    # the entries
    for s, (g, w) in enumerate(zip(catalog, want["catalog"])):
        assert g.is_star is False and g.gal_frac_dev == 0.5
        assert np.asarray(g.gal_fluxes).tobytes() == np.asarray(w.gal_fluxes).tobytes(), s
        assert np.asarray(g.star_fluxes).tobytes() == np.asarray(w.star_fluxes).tobytes(), s
        assert (g.gal_axis_ratio, g.gal_angle, g.gal_radius_px) == (w.gal_axis_ratio, w.gal_angle, w.gal_radius_px), s
    # the table
    ent = host_entries(images, want["patches"])
    assert table.source.dtype == np.int32 and table.image.dtype == np.int32 and table.box.dtype == np.int64
    assert table.source.tolist() == [e[0] for e in ent] and table.image.tolist() == [e[1] for e in ent]
    box = np.array([[p.box[0][0], p.box[0][1], p.box[1][0], p.box[1][1]] for _, _, p in ent], dtype=np.int64).reshape(-1, 4)
    assert np.array_equal(table.box, box)
    pc = np.array([p.pixel_center for _, _, p in ent]).reshape(-1, 2)
    assert table.pixel_center.tobytes() == pc.tobytes()
    assert table.active_pixels.tolist() == [int(p.active_pixel_bitmap.sum()) for _, _, p in ent]
    wc = np.array([p.world_center for _, _, p in ent]).reshape(-1, 2)
    if exact:
        assert table.world_center.tobytes() == wc.tobytes()
    else:
        for k, (_, n, p) in enumerate(ent):
            assert np.abs(table.world_center[k] - wc[k]).max() <= world_bound(images[n], p.pixel_center), k
    assert table.neighbor_lists == want["neighbors"] and table.neighbors() == want["neighbors"]


def _table_bytes(catalog, t):
    parts = [t.source, t.image, t.box, t.pixel_center, t.world_center, t.active_pixels]
    if hasattr(t, "stamps"):
        parts += [t.stamp, t.stamps]
    for ce in catalog:
        parts += [ce.pos, ce.gal_fluxes, ce.star_fluxes, np.array([ce.gal_axis_ratio, ce.gal_angle, ce.gal_radius_px])]
    return [np.ascontiguousarray(p).tobytes() for p in parts] + [repr(t.neighbor_lists).encode(), repr(t.detections).encode()]


# ---- 1: the join rules and the entries -------------------------------------------------------------------------------------
def test_join_rules_and_catalog_entries_on_hand_made_catalogs():
    from celeste_jl_amd import prep
    images, cats = join_scene()
    want = host_path(images, cats, JOIN_RADIUS)
    assert want["checked"] == 9
    # the scene holds what it was built for
    assert want["detections"] == [[(1, 0), (3, 0), (3, 1)], [(1, 1), (3, 4), (4, 1)], [(1, 2), (4, 2)], [(3, 2), (4, 0)], [(3, 3)],
                                  [(4, 3)]]
    assert np.hypot(*(want["worlds"][3][2] - want["worlds"][3][3])) < JOIN_RADIUS
    e = want["catalog"]
    assert e[0].gal_fluxes[2] == cats[1].flux[0]                                        # equal npix in band 3: image 1's wins
    assert e[5].gal_fluxes.tolist() == [0.0, cats[4].flux[3], 0.0, 0.0, 0.0]            # bands without a detection
    assert e[1].gal_axis_ratio == cats[4].b[1] / cats[4].a[1] and e[1].gal_fluxes[2] == cats[1].flux[1]   # band 2 gives the shape
    catalog, table = prep.detected_table(images, cats, JOIN_RADIUS)
    assert_is_host_path(images, cats, JOIN_RADIUS, catalog, table, want)
    # two detections of image 3 joined entry 0: the box in image 3 comes from the later one, (2 .. 20) dilated by 2
    k = np.flatnonzero((table.source == 0) & (table.image == 3))[0]
    assert table.box[k].tolist() == [1, 22, 4, 16]
    assert prep.detected_last_ms().keys() == set(prep.DETECTED_STAGES) and prep.detected_last_ms()["join"] > 0
    # no detection at all: zero objects, an empty table
    catalog, table = prep.detected_table(images, [make_catalog([]) for _ in images], JOIN_RADIUS)
    assert catalog == [] and table.n_sources == 0 and len(table.source) == 0 and table.neighbor_lists == [] and table.detections == []


def test_exact_ties_of_the_join():
    """equal distances go to the lower index; a distance equal to match_radius does not join"""
    from celeste_jl_amd import prep
    images, cats = tie_scene()
    want = host_path(images, cats, TIE_RADIUS, exact_distances=True)
    # the scene holds what it was built for
    w = want["worlds"]
    assert np.hypot(*(w[1][0] - w[0][0])) == np.hypot(*(w[1][0] - w[0][1])) == 5.0 < TIE_RADIUS
    assert np.hypot(*(w[1][1] - w[0][2])) == TIE_RADIUS
    assert np.hypot(*(w[2][0] - w[0][2])) == np.hypot(*(w[2][0] - w[1][1])) == 3.0
    assert want["detections"] == [[(0, 0), (1, 0)], [(0, 1)], [(0, 2), (2, 0)], [(1, 1)]]
    catalog, table = prep.detected_table(images, cats, TIE_RADIUS)
    assert_is_host_path(images, cats, TIE_RADIUS, catalog, table, want)


# ---- 2: past one tile, past one workgroup ------------------------------------------------------------------------------------
def test_more_entries_than_a_tile_and_more_detections_than_a_workgroup():
    from celeste_jl_amd import prep
    images, cats = lattice_scene()
    assert len(cats[0]) > prep.MATCH_TILE and len(cats[1]) > prep.MATCH_BLOCK
    want = host_path(images, cats, JOIN_RADIUS)
    assert want["checked"] == len(cats[1]) + len(cats[2])
    d = want["detections"]
    joined_far = [k for k in range(prep.MATCH_TILE, len(cats[0])) if any(i == 1 for i, _ in d[k])]
    assert len(joined_far) >= 4                                                         # entries of the second tile were joined
    late = [j for k in range(len(cats[0])) for i, j in d[k] if i == 1 and j >= prep.MATCH_BLOCK]
    assert late and any(i == 1 and j >= prep.MATCH_BLOCK for k in range(len(cats[0]), len(d)) for i, j in d[k][:1])
    assert any(len(x) >= 2 and x[0][0] == 1 and x[1][0] == 2 for x in d)                # image 2 joined an entry image 1 appended
    assert len(d) > len(cats[0]) + 80
    catalog, table = prep.detected_table(images, cats, JOIN_RADIUS)
    assert_is_host_path(images, cats, JOIN_RADIUS, catalog, table, want)


# ---- 3: boxes ----------------------------------------------------------------------------------------------------------------
def test_boxes_dense():
    from celeste_jl_amd import prep
    images, cats = box_scene()
    want = host_path(images, cats, 1.0)
    assert len(want["catalog"]) == 15 and want["checked"] == 5
    catalog, table = prep.detected_table(images, cats, 1.0)
    assert_is_host_path(images, cats, 1.0, catalog, table, want)

    def box(s, n):
        return table.box[s * 3 + n].tolist()
    # half-dilations 0.5, 1.5, 2.5 round to 0, 2, 2; the 5-pixel box of 0 is rows 7 .. 17, of 1 rows 25 .. 35
    assert box(0, 2) == [7, 17, 25, 35] and box(1, 2)[:2] == [25, 35]
    assert box(1, 0)[:2] == [21, 39] and box(2, 0)[:2] == [31, 59] and box(3, 0) == [17, 27, 36, 46]
    assert box(0, 1) == [7, 17, 25, 35]                                                  # image 1's own (9 .. 15) + 1 lies inside
    # clamped at each edge
    assert box(4, 0)[0] == 1 and box(5, 0)[1] == 60 and box(6, 0)[2] == 1 and box(7, 0)[3] == 60
    nb = want["neighbors"]
    assert 9 in nb[8] and 8 in nb[9] and 11 not in nb[10] and 10 not in nb[11]
    assert box(8, 2)[:2] == [15, 25] and box(9, 2)[:2] == [25, 35] and box(10, 2)[:2] == [15, 25] and box(11, 2)[:2] == [26, 36]
    a = table.active_pixels.reshape(-1, 3)
    h2w2 = (table.H2 * table.W2).reshape(-1, 3)
    assert 0 < a[12, 0] < h2w2[12, 0] and a[13, 0] == 0 and h2w2[13, 0] > 0 and (a[:, 1] == h2w2[:, 1]).all()


def test_boxes_sparse():
    from celeste_jl_amd import prep
    images, cats = sparse_scene()
    want = host_path(images, cats, 1.0)
    S = len(want["catalog"])
    assert S >= 80 and want["checked"] > 60 and sum(len(d) > 1 for d in want["detections"]) > 15
    catalog, table = prep.detected_table(images, cats, 1.0)
    assert not table.dense
    assert_is_host_path(images, cats, 1.0, catalog, table, want)
    assert S < len(table.source) < 4 * S and (table.H2 > 0).all() and (table.W2 > 0).all()
    assert (table.active_pixels < table.H2 * table.W2).any()
    # sparse on request, for fewer images than nine: the same rows, restricted to the first three images' detections
    c3, t3 = prep.detected_table(images[:3], cats[:3], 1.0, sparse=True)
    d3, td = prep.detected_table(images[:3], cats[:3], 1.0)
    assert not t3.dense and td.dense and len(t3.source) < len(td.source)
    keep = np.flatnonzero((td.H2 > 0) & (td.W2 > 0))
    assert np.array_equal(td.box[keep], t3.box) and np.array_equal(td.source[keep], t3.source) and t3.neighbor_lists == td.neighbor_lists


# ---- 4: a rotated, scaled Jacobian ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["join", "box"])
def test_a_rotated_scaled_jacobian(scene):
    from celeste_jl_amd import prep
    images, cats = join_scene() if scene == "join" else box_scene()
    rotate(images)
    want = host_path(images, cats, 1.5)
    assert want["checked"] >= 5
    assert_no_box_ties(images, want["joined"])
    catalog, table = prep.detected_table(images, cats, 1.5)
    assert_is_host_path(images, cats, 1.5, catalog, table, want, exact=False)
    assert abs(catalog[0].gal_angle - cats[1 if scene == "join" else 0].theta[0]) > 0.1      # x_vs_n_angle is in it


# ---- 5: an image with an eigen-PSF ---------------------------------------------------------------------------------------------
def test_stamps_of_an_eigen_psf_image():
    """|stamp - SDSSPSFMap.__call__| <= 2 (nk + ni nj) eps sum_k |w_k| |rrows[:, k]| per pixel, the dot-product bound of
    tests/test_gpu_prep.py"""
    from celeste_jl_amd import model, prep, synthetic
    images, cats = join_scene()
    var = synthetic.variable_images(60, 60, seed=2)
    var[2].pixels = images[1].pixels
    images[1] = var[2]                                                                  # band 3, with an SDSSPSFMap
    assert isinstance(images[1].psfmap, model.SDSSPSFMap) and not isinstance(images[3].psfmap, model.SDSSPSFMap)
    want = host_path(images, cats, JOIN_RADIUS)
    catalog, table = prep.detected_table(images, cats, JOIN_RADIUS)
    assert_is_host_path(images, cats, JOIN_RADIUS, catalog, table, want)
    e1 = np.flatnonzero(table.image == 1)
    assert table.stamp.shape == (len(table.source),) and table.stamps.shape == (len(e1), 51 * 51)
    assert (table.stamp[table.image != 1] == -1).all() and table.stamp[e1].tolist() == list(range(len(e1)))
    m = images[1].psfmap
    ni, nj, nk = m.cmat.shape
    ent = host_entries(images, want["patches"])
    for e in e1:
        x, y = table.pixel_center[e]
        ref = np.ascontiguousarray(ent[e][2].stamp.T).reshape(-1)                       # the host patch's own stamp, column-major
        w = np.einsum("ijk,i,j->k", m.cmat, (0.001 * (x - 1.0)) ** np.arange(ni), (0.001 * (y - 1.0)) ** np.arange(nj))
        bound = 2 * (nk + ni * nj) * EPS * (np.abs(m.rrows) @ np.abs(w))
        assert (np.abs(table.stamps[table.stamp[e]] - ref) <= bound).all(), e


# ---- 6: through the wiring -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def field():
    from celeste_jl_amd import synthetic
    return synthetic.make_field(200, 200, 12, seed=31, stars_only=True)


def assert_same_catalog_and_table(images, host, dev):
    (hc, patches), (dc, table) = host, dev
    from celeste_jl_amd import model
    assert len(hc) == len(dc) > 0
    for a, b in zip(hc, dc):
        assert a.pos.tobytes() == b.pos.tobytes() and a.gal_fluxes.tobytes() == b.gal_fluxes.tobytes()
        assert a.star_fluxes.tobytes() == b.star_fluxes.tobytes() and a.is_star == b.is_star and a.gal_frac_dev == b.gal_frac_dev
        assert (a.gal_axis_ratio, a.gal_angle, a.gal_radius_px) == (b.gal_axis_ratio, b.gal_angle, b.gal_radius_px)
    ent = host_entries(images, patches)
    assert table.source.tolist() == [e[0] for e in ent] and table.image.tolist() == [e[1] for e in ent]
    assert table.box.tolist() == [[p.box[0][0], p.box[0][1], p.box[1][0], p.box[1][1]] for _, _, p in ent]
    assert table.pixel_center.tobytes() == np.array([p.pixel_center for _, _, p in ent]).tobytes()
    assert table.world_center.tobytes() == np.array([p.world_center for _, _, p in ent]).tobytes()
    assert table.active_pixels.tolist() == [int(p.active_pixel_bitmap.sum()) for _, _, p in ent]
    assert table.neighbors() == model.neighbor_map(patches)


def test_detect_table_is_detect_sources_and_its_context_evaluates_alike(field):
    import celeste_jl_amd as cel
    from celeste_jl_amd import cabi, detect, model
    from celeste_jl_amd.params import init_source_table
    f = field
    host = detect.detect_sources(f.images, match_radius=2.5)
    dev = detect.detect_table(f.images, match_radius=2.5)
    assert_same_catalog_and_table(f.images, host, dev)
    catalog, patches = host
    table = dev[1]
    nb = model.neighbor_map(patches)
    a = cel.FieldContext(f.images, patches, nb)
    b = cel.FieldContext(f.images, None, table.neighbors(), problem=cabi.problem_from_table(f.images, table, table.neighbors()))
    try:
        targets = list(range(len(catalog)))
        vp = init_source_table(catalog, targets)
        ra, rb = a.eval_batch(vp, targets), b.eval_batch(vp, targets)
        assert (np.array(ra[4]) == 0).all()
        for x, y in zip(ra, rb):
            assert np.array(x).tobytes() == np.array(y).tobytes()
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("kw", [{"method": "joint_vi"}, {"method": "single_vi"}, {"method": "single_vi", "devices": [0]}],
                         ids=["joint_vi", "single_vi", "group"])
def test_infer_box_without_a_catalog_with_device_prep(field, kw):
    import celeste_jl_amd as cel
    box = cel.BoundingBox(20.0, 180.0, 20.0, 180.0)
    cfg = cel.ElboConfig(max_iters=8)
    want = cel.infer_box(field.images, box, cfg=cfg, match_radius=2.5, n_iters=1, prep="host", **kw)
    got = cel.infer_box(field.images, box, cfg=cfg, match_radius=2.5, n_iters=1, prep="device", **kw)
    assert len(want) == len(got) >= 5
    for a, b in zip(want, got):
        assert a.vs.tobytes() == b.vs.tobytes() and a.is_sky_bad == b.is_sky_bad and a.failed == b.failed
        assert (a.init_ra, a.init_dec) == (b.init_ra, b.init_dec)


def test_infer_box_mcmc_without_a_catalog_with_device_prep(field):
    import celeste_jl_amd as cel
    from celeste_jl_amd import detect, mcmc
    catalog, _ = detect.detect_table(field.images, match_radius=2.5)
    t = next(i for i, ce in enumerate(catalog) if 20.0 < ce.pos[0] < 180.0 and 20.0 < ce.pos[1] < 180.0)
    p = catalog[t].pos
    box = cel.BoundingBox(p[0] - 0.5, p[0] + 0.5, p[1] - 0.5, p[1] + 0.5)
    cfg = mcmc.MCMCConfig(num_ais_temperatures=3, num_ais_samples=2, num_samples_per_chain=5, num_bootstrap=100, seed=11)
    want = cel.infer_box(field.images, box, method="mcmc", match_radius=2.5, mcmc_config=cfg, prep="host")
    got = cel.infer_box(field.images, box, method="mcmc", match_radius=2.5, mcmc_config=cfg, prep="device")
    assert len(want) == len(got) == 1 and want[0].source == got[0].source == t
    for name in ("star_samples", "star_lls", "gal_samples", "gal_lls", "ais_weights", "type_samples", "status"):
        assert getattr(want[0], name).tobytes() == getattr(got[0], name).tobytes(), name
    assert (want[0].star_lnZ, want[0].gal_lnZ, want[0].ave_pstar) == (got[0].star_lnZ, got[0].gal_lnZ, got[0].ave_pstar)


def test_a_multifield_gives_the_same_sparse_rows():
    from celeste_jl_amd import detect, synthetic
    f = synthetic.make_multifield((2, 2), n_sources=60, seed=5)
    assert len(f.images) == 20
    cats = detect.extract(f.images)
    host = detect.build_detection_output(f.images, cats, 1.0)
    worlds = [detect.world_coords(c, im) for c, im in zip(cats, f.images)]
    joined, dets = detect.match_detections(worlds, 1.0)
    assert_join_margin(worlds, joined, dets, 1.0)
    dev = detect.detect_table(f.images, match_radius=1.0)
    assert not dev[1].dense and dev[1].detections == dets
    assert_same_catalog_and_table(f.images, host, dev)


# ---- 7: a second call repeats the first ----------------------------------------------------------------------------------------
def test_a_second_call_repeats_the_first_bit_for_bit():
    from celeste_jl_amd import prep
    for images, cats, r in (join_scene() + (JOIN_RADIUS,), sparse_scene() + (1.0,), tuple(lattice_scene()) + (JOIN_RADIUS,)):
        with prep.PrepImages(images, 0) as pi:
            a = prep.detected_table(images, cats, r, prep_images=pi)
            b = prep.detected_table(images, cats, r, prep_images=pi)
        c = prep.detected_table(images, cats, r)
        assert _table_bytes(*a) == _table_bytes(*b) == _table_bytes(*c)
