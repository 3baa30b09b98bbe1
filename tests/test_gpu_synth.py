"""MI355X: synthetic images on the device (libceleste_synth.so) -- the expected electrons against the host function
synthetic.render_expected_image, the Poisson pixels against the numpy restatement of tests/synth_reference.py pixel for
pixel, their independence of batch, tiling and launch split, their statistics, and the public face
synthetic.make_field(..., device=0) down to an inference on a device-made field."""
import copy
import math

import numpy as np
import pytest

import synth_reference as ref
import celeste_jl_amd as cel
from celeste_jl_amd import synth, synthetic
from celeste_jl_amd.params import CatalogEntry

pytestmark = pytest.mark.gpu
SEED = 0x5EED0123456789AB      # both key words in use


def _ce(pos, is_star, flux=60.0, dev=0.3, ab=0.6, angle=0.7, radius=2.5):
    fl = flux * np.array([0.4, 0.8, 1.0, 1.3, 1.7])
    return CatalogEntry(np.asarray(pos, float), is_star, fl.copy(), 0.9 * fl, dev, ab, angle, radius)


def hand_catalog():
    return [_ce((1.2, 1.7), True),                                   # a corner: clamped on two sides
            _ce((96.6, 122.4), False, flux=150.0),                   # the opposite corner
            _ce((48.5, 61.5), True, flux=200.0),                     # box edges on rounding ties (23.5, 73.5, 36.5, 86.5)
            _ce((50.0, 63.0), False, flux=300.0, radius=4.0),        # a galaxy over it
            _ce((20.3, 100.2), True, flux=40.0), _ce((20.3, 100.2), True, flux=55.0),   # two stars at one position
            _ce((-10.0, 60.0), True, flux=500.0),                    # half off the image
            _ce((-40.0, 60.0), False, flux=500.0),                   # no entry
            _ce((70.0, 30.0), False, flux=2000.0, ab=0.05, radius=20.0, angle=2.1),
            _ce((30.0, 25.0), False, flux=80.0, radius=0.2),
            _ce((80.0, 90.0), False, dev=0.0), _ce((60.0, 100.0), False, dev=1.0)]


def host_electrons(images, catalog):
    return [synthetic.render_expected_image(im, catalog) * im.nelec_per_nmgy.astype(np.float64)[:, None] for im in images]


@pytest.fixture(scope="module")
def scenes():
    """the hand-made catalog on constant and on variable images: host planes and device planes, computed once"""
    out = {}
    cat = hand_catalog()
    for name, images in (("blank", synthetic.blank_images(97, 123)), ("variable", synthetic.variable_images(97, 123, seed=5))):
        out[name] = (images, cat, host_electrons(images, cat), synth.expected_electrons(images, cat))
    return out


def _assert_planes(got, want):
    assert len(got) == len(want)
    for n, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == np.float64
        err, scale = np.abs(g - w).max(), np.abs(w).max()
        print("image %d: max |got - ref| = %.3e, max |ref| = %.3e, ratio %.2e" % (n, err, scale, err / scale))
        assert err <= 1e-12 * scale, (n, err, scale)


@pytest.mark.parametrize("name", ["blank", "variable"])
def test_expected_electrons_match_the_host_function(scenes, name):
    images, cat, want, got = scenes[name]
    entries, stamps = synth.entry_table(images, cat)
    assert len(entries) == 5 * 11 and len(stamps) == (5 if name == "blank" else 5 * 5)
    _assert_planes(got, want)
    assert all(np.abs(w - w[::-1]).max() > 0 for w in want)          # (the planes are not symmetric: a transpose would show)


def test_expected_electrons_on_overlapping_fields():
    f = synthetic.make_multifield(grid=(2, 2), H=64, W=64, n_sources=30, seed=5)
    entries, _ = synth.entry_table(f.images, f.catalog)
    assert len(f.images) == 20 and 0 < len(entries) < 20 * 30 * 2 // 3   # every source is absent from some images
    _assert_planes(synth.expected_electrons(f.images, f.catalog), host_electrons(f.images, f.catalog))


def test_no_entry_gives_sky_times_iota():
    images = synthetic.variable_images(97, 123, seed=5)[:2]
    for cat in ([], [_ce((-40.0, 60.0), False)]):
        for im, lam in zip(images, synth.expected_electrons(images, cat)):
            assert np.array_equal(lam, im.sky.astype(np.float64) * im.nelec_per_nmgy.astype(np.float64)[:, None])


def ramp():
    r = np.concatenate([[0.0, -1.0, np.nan, np.inf, 1e-3, 9.999, 10.0, 10.001], np.logspace(-3, 6, 3064), np.full(1024, 492.0)])
    assert r.size == 4096
    return r


def _assert_same_pixels(got, lam, seed, stream, first_index=0, what=""):
    want, used, capped, trial = ref.sample(lam, seed, stream=stream, first_index=first_index, details=True)
    assert not capped.any()
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        g, w, l = (x.reshape(-1, order="F") for x in (got, want, np.asarray(lam)))
        bad = np.flatnonzero(~same.reshape(-1, order="F"))
        lines = ["pixel %d: lambda %r, device %r, restatement %r (its last log test: k %r, lhs %r, rhs %r)"
                 % (i + first_index, l[i], g[i], w[i], trial[i, 0], trial[i, 1], trial[i, 2]) for i in bad[:8]]
        raise AssertionError("%s: %d of %d pixels differ\n%s" % (what, bad.size, g.size, "\n".join(lines)))


def test_pixels_replay_the_restatement_exactly(scenes):
    images, cat, _, lams = scenes["variable"]
    images = [copy.copy(images[1]), copy.copy(images[4])]      # (the fixture's images keep their pixels)
    lams = [lams[1], lams[4]]
    capped = synth.gen_images(images, cat, SEED, streams=[1, 4])
    assert capped == 0
    for im, lam, stream in zip(images, lams, (1, 4)):
        assert im.pixels.dtype == np.float32 and im.pixels.shape == lam.shape
        _assert_same_pixels(im.pixels, lam, SEED, stream, what="gen_images, stream %d" % stream)
        px, cap = synth.sample_poisson(lam, SEED, stream=stream, return_capped=True)
        assert cap == 0
        _assert_same_pixels(px, lam, SEED, stream, what="sample_poisson, stream %d" % stream)
    r = ramp()
    px, cap = synth.sample_poisson(r, SEED, stream=7, first_index=12345, return_capped=True)
    assert cap == 0 and px[0] == 0 and px[1] == 0 and np.isnan(px[2]) and np.isnan(px[3])
    _assert_same_pixels(px, r, SEED, 7, first_index=12345, what="the ramp")
    # the ramp's float32 values as a sky plane with no source: the fused kernel's sampler on the same edge values
    im = synthetic.blank_images(64, 64)[0]
    im.sky = r.astype(np.float32).reshape(64, 64, order="F")
    im.nelec_per_nmgy = np.ones(64, dtype=np.float32)
    assert synth.gen_images([im], [], SEED, streams=[9]) == 0
    _assert_same_pixels(im.pixels, im.sky.astype(np.float64), SEED, 9, what="the ramp as a sky plane")


def test_pixels_do_not_depend_on_batch_tiling_or_split(scenes):
    images, cat, _, lams = scenes["blank"]
    images = [copy.copy(im) for im in images]
    synth.gen_images(images, cat, SEED)
    first = [im.pixels.copy() for im in images]
    synth.gen_images(images, cat, SEED)
    assert all(np.array_equal(a, im.pixels, equal_nan=True) for a, im in zip(first, images))            # a repeated call
    synth.gen_images(images, cat, SEED, chunk_tiles=1)
    assert all(np.array_equal(a, im.pixels, equal_nan=True) for a, im in zip(first, images))            # one tile per launch
    alone = [images[3]]
    synth.gen_images(alone, cat, SEED, streams=[3])
    assert np.array_equal(first[3], alone[0].pixels)                                                    # image 3 on its own
    lam = lams[2]
    flat = lam.reshape(-1, order="F")
    half = flat.size // 2 + 7
    whole = synth.sample_poisson(lam, SEED, stream=2)
    assert np.array_equal(whole, first[2])                                                              # the plane, resampled
    parts = np.concatenate([synth.sample_poisson(flat[:half], SEED, stream=2),
                            synth.sample_poisson(flat[half:], SEED, stream=2, first_index=half)])
    assert np.array_equal(parts, whole.reshape(-1, order="F"))                                          # in two halves
    const = np.full(1 << 14, 492.0)
    base = synth.sample_poisson(const, SEED, stream=0)
    assert np.mean(synth.sample_poisson(const, SEED + 1, stream=0) != base) > 0.9                       # another seed
    assert np.mean(synth.sample_poisson(const, SEED + (1 << 32), stream=0) != base) > 0.9               # (its high word)
    assert np.mean(synth.sample_poisson(const, SEED, stream=1) != base) > 0.9                           # another stream


@pytest.mark.parametrize("k,lam", [(0, 9.99), (1, 10.0), (2, 492.0)])
def test_device_statistics(k, lam):
    n = 1 << 18
    plane = np.full(n, lam)
    x, cap = synth.sample_poisson(plane, 4242 + k, stream=k, return_capped=True)
    want = ref.sample(plane, 4242 + k, stream=k)
    assert cap == 0
    for name, y in (("device", x.astype(np.float64)), ("restatement", want.astype(np.float64))):
        zm = (y.mean() - lam) / math.sqrt(lam / n)
        zv = (y.var() - lam) / (lam * math.sqrt((2 + 1 / lam) / n))
        print("%s, lambda %g: z(mean) %.2f, z(var) %.2f" % (name, lam, zm, zv))
        assert abs(zm) <= 4 and abs(zv) <= 4, name
    assert np.array_equal(x, want)


def test_public_face():
    host = synthetic.make_field(96, 120, 12, seed=9)
    dev = synthetic.make_field(96, 120, 12, seed=9, device=0)
    assert np.array_equal(host.vp, dev.vp) and host.neighbors == dev.neighbors
    for a, b in zip(host.catalog, dev.catalog):
        assert np.array_equal(a.pos, b.pos) and a.is_star == b.is_star and np.array_equal(a.gal_fluxes, b.gal_fluxes)
    for ra, rb in zip(host.patches, dev.patches):
        assert [p.box for p in ra] == [p.box for p in rb]
    lams = synth.expected_electrons(dev.images, dev.catalog)
    z = np.concatenate([((im.pixels.astype(np.float64) - l) / np.sqrt(l)).ravel() for im, l in zip(dev.images, lams)])
    assert all(im.pixels.dtype == np.float32 and im.pixels.shape == (96, 120) for im in dev.images)
    assert not any(np.array_equal(a.pixels, b.pixels) for a, b in zip(host.images, dev.images))        # (its own random stream)
    n = z.size
    se_var = math.sqrt(np.mean(2.0 + 1.0 / np.concatenate([l.ravel() for l in lams])) / n)
    print("pull over %d pixels: mean %.4f (se %.4f), variance %.4f (se %.4f)" % (n, z.mean(), 1 / math.sqrt(n), z.var(), se_var))
    assert abs(z.mean()) <= 4 / math.sqrt(n) and abs(z.var() - 1.0) <= 4 * se_var
    # expectation: Float32 of the expected electrons, through both faces
    imgs = synthetic.blank_images(96, 120)
    synth.gen_images(imgs, dev.catalog, 9, expectation=True)
    assert all(np.array_equal(im.pixels, l.astype(np.float32)) for im, l in zip(imgs, lams))
    imgs = synthetic.blank_images(96, 120)
    synthetic.gen_images(imgs, dev.catalog, np.random.default_rng(0), expectation=True, device=0)
    assert all(np.array_equal(im.pixels, l.astype(np.float32)) for im, l in zip(imgs, lams))
    # nan_fraction masks what the device drew
    masked = synthetic.make_field(96, 120, 12, seed=9, device=0, nan_fraction=0.05)
    nan = np.concatenate([np.isnan(im.pixels).ravel() for im in masked.images])
    assert abs(nan.mean() - 0.05) <= 4 * math.sqrt(0.05 * 0.95 / nan.size)
    for a, b in zip(masked.images, dev.images):
        keep = ~np.isnan(a.pixels)
        assert np.array_equal(a.pixels[keep], b.pixels[keep])
    mf = synthetic.make_multifield(grid=(1, 2), H=64, W=64, n_sources=6, seed=5, device=0)
    mh = synthetic.make_multifield(grid=(1, 2), H=64, W=64, n_sources=6, seed=5)
    assert np.array_equal(mf.vp, mh.vp) and all(im.pixels.dtype == np.float32 and np.isfinite(im.pixels).all() for im in mf.images)


def test_end_to_end_on_a_device_made_field():
    """the body of test_end_to_end_recovers_the_synthetic_truth (tests/test_gpu_optimizer.py) with its thresholds, on the
    field the device draws for the same seed"""
    from celeste_jl_amd.catalog import catalog_entry_to_row, celeste_to_rows, score_predictions
    f = synthetic.make_field(300, 340, 40, seed=77, margin=26, device=0)
    box = cel.BoundingBox(0.0, 300.0, 0.0, 340.0)
    res = cel.infer_box(f.images, box, f.catalog, method="joint_vi")
    rows = celeste_to_rows(res)
    assert len(res) == 40 and len(rows) >= 34
    truth = {(ce.pos[0], ce.pos[1]): ce for ce in f.catalog}
    n_bright = n_type = 0
    flux_err, col_err = [], []
    for r, row in zip([x for x in res if not x.is_sky_bad], rows):
        ce = truth[(r.init_ra, r.init_dec)]
        fl = ce.star_fluxes if ce.is_star else ce.gal_fluxes
        if fl[2] < 2.0:        # faint: the posterior is broad, nothing to assert
            continue
        n_bright += 1
        n_type += int((row["is_star"] > 0.5) == ce.is_star)
        flux_err.append(abs(row["flux_r_nmgy"] / fl[2] - 1.0))
        col_err.append(abs(row["color_gr"] - np.log(fl[2] / fl[1])))
        assert abs(row["ra"] - ce.pos[0]) <= 1e-4 + 1e-9
    print("bright sources %d, type right %d, median |flux err| %.3f, median |g-r err| %.3f"
          % (n_bright, n_type, np.median(flux_err), np.median(col_err)))
    assert n_bright >= 8 and n_type >= 0.8 * n_bright
    assert np.median(flux_err) <= 0.10 and np.median(col_err) <= 0.15
    good = [x for x in res if not x.is_sky_bad]
    scores = score_predictions([catalog_entry_to_row(truth[(r.init_ra, r.init_dec)]) for r in good], rows)
    print({k: (v["N"], round(v["first"], 3)) for k, v in scores.items()})
    assert scores["position"]["first"] <= 1.5e-4
    assert scores["flux_r_mag"]["first"] <= 0.25
    assert scores["missed_stars"]["first"] <= 0.35 and scores["missed_galaxies"]["first"] <= 0.35
