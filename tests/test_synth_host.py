"""CPU: the host side of device image generation (celeste_jl_amd.synth, libceleste_synth.so's ABI) and the numpy
restatement of its sampler (tests/synth_reference.py): the restatement is a Poisson sampler, the library exports its header,
refuses invalid arguments before it touches a device, the entry table is the geometry of render_expected_image, and
device=None leaves the host generator as it was."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from scipy import stats

import synth_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_DRAWS = 100_000


@pytest.fixture(scope="module")
def slib(lib):
    import __graft_entry__ as g
    if not os.path.exists(g.SYNTH_LIB):
        g.build()
    from celeste_jl_amd import synth
    return synth.load_library()


def test_vector_philox_is_the_scalar_one():
    b = ref.philox_blocks(np.array([5, 7, 0xffffffff]), 3, np.array([2, 0, 63]), ref.TAG, 0x1234567890abcdef)
    for i, (c0, c2) in enumerate(((5, 2), (7, 0), (0xffffffff, 63))):
        want = ref.philox4x32_10((c0, 3, c2, ref.TAG), (0x90abcdef, 0x12345678))
        assert [int(x[i]) for x in b] == want
        assert ref.u53_array(b[0], b[1])[i] == ref.u53(want[0], want[1])
    assert ref.TAG == int.from_bytes(b"SYNT", "big")


def moment_z(x, lam):
    """(z of the mean, z of the variance): standard errors sqrt(lam / N) and lam sqrt((2 + 1 / lam) / N)"""
    n = x.size
    return ((x.mean() - lam) / math.sqrt(lam / n), (x.var() - lam) / (lam * math.sqrt((2 + 1 / lam) / n)))


def chi_square_p(x, lam, bins=30):
    """chi-square against scipy.stats.poisson over about `bins` equal-probability bins (fewer where the distribution has
    fewer values; bins with an expected count under 5 are merged into their neighbour)"""
    d = stats.poisson(lam)
    edges = np.unique(d.ppf(np.linspace(0, 1, bins + 1)[1:-1]))
    cdf = np.concatenate([[0.0], d.cdf(edges), [1.0]])
    expect = x.size * np.diff(cdf)
    got = np.bincount(np.searchsorted(edges, x, side="left"), minlength=expect.size).astype(float)
    e2, g2 = [], []
    for e, g in zip(expect, got):
        if e2 and e2[-1] < 5:
            e2[-1] += e; g2[-1] += g
        else:
            e2.append(e); g2.append(g)
    if len(e2) > 1 and e2[-1] < 5:
        e2[-2] += e2.pop(); g2[-2] += g2.pop()
    e2, g2 = np.array(e2), np.array(g2)
    return float(stats.chi2.sf(np.sum((g2 - e2) ** 2 / e2), len(e2) - 1)), len(e2)


@pytest.mark.parametrize("k,lam", list(enumerate((0.3, 3.0, 9.99, 10.0, 50.0, 1000.0, 1e5))))
def test_the_restatement_is_a_poisson_sampler(k, lam):
    x, used, capped, _ = ref.sample(np.full(N_DRAWS, lam), seed=2024 + k, stream=k, details=True)
    x = x.astype(np.float64)
    zm, zv = moment_z(x, lam)
    p, nb = chi_square_p(x, lam)
    print("lambda %g: z(mean) %.2f, z(var) %.2f, chi-square p %.3f over %d bins, at most %d uniforms" % (lam, zm, zv, p, nb, used.max()))
    assert not capped.any() and np.all(x >= 0) and np.all(x == np.floor(x))
    assert abs(zm) <= 4 and abs(zv) <= 4
    assert p > 1e-4
    assert used.max() <= 64


def test_restatement_edge_values_and_cap():
    lam = np.array([0.0, -1.0, np.nan, np.inf, -np.inf, 1e-3])
    x, used, capped, _ = ref.sample(lam, seed=1, details=True)
    assert x[0] == 0 and x[1] == 0 and np.isnan(x[2:5]).all() and x[5] in (0.0, 1.0)
    assert not capped.any() and list(used[:5]) == [0] * 5
    # a pixel's value depends on its own index, not on its place in the call
    a = ref.sample(np.full(50, 30.0), seed=9, stream=2, first_index=100)
    b = ref.sample(np.full(20, 30.0), seed=9, stream=2, first_index=130)
    assert np.array_equal(a[30:], b)
    assert not np.array_equal(a, ref.sample(np.full(50, 30.0), seed=9, stream=3, first_index=100))


def test_header_symbols_are_exported_and_build_loads_the_library(slib):
    import __graft_entry__ as g
    from celeste_jl_amd import synth
    hdr = open(os.path.join(ROOT, "include", "celeste_synth.h")).read()
    declared = set(re.findall(r"\b(celeste_synth_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(synth.EXPORTED_SYMBOLS), declared ^ set(synth.EXPORTED_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", g.SYNTH_LIB], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[1] in "TDBR"}
    assert exported == declared, exported ^ declared
    assert slib.celeste_synth_version() == synth.ABI_VERSION
    assert "#define CELESTE_SYNTH_ABI_VERSION %d" % synth.ABI_VERSION in hdr
    assert "0x%08X" % synth.PHILOX_TAG in hdr.upper().replace("0X", "0x") and "#define CELESTE_SYNTH_MAX_BLOCKS %d" % synth.MAX_BLOCKS in hdr
    assert slib.celeste_synth_strerror(0) == b"ok" and b"CPU fallback" in slib.celeste_synth_strerror(synth.ERR_NO_DEVICE)
    entry = g.LIBRARIES["synth"]     # build() compiles and loads what its table lists
    assert os.path.basename(entry["source"]) == "celeste_synth.hip" and os.path.isfile(entry["source"])
    assert sys.modules["celeste_jl_amd." + entry["module"]] is synth
    assert C.sizeof(synth.SynthImageT) == 16 + 5 * 8 and synth.ENTRY_DTYPE.itemsize == 8 * 4 + 7 * 8


def _small_call():
    from celeste_jl_amd import synth, synthetic
    images = synthetic.blank_images(70, 40)[:2]
    catalog = [synthetic.sample_ce([10.2, 12.1], True), synthetic.sample_ce([60.0, 30.5], False)]
    entries, stamps = synth.entry_table(images, catalog)
    return images, entries, stamps


def _status(images, entries, stamps, **kw):
    from celeste_jl_amd import synth
    try:
        synth.generate_raw(images, entries, stamps, **kw)
    except synth.SynthError as e:
        return e.status
    return 0


def test_invalid_arguments_are_refused_without_a_device(slib):
    from celeste_jl_amd import synth
    images, entries, stamps = _small_call()
    assert len(entries) == 4 and list(entries["image"]) == [0, 0, 1, 1] and len(stamps) == 2
    INV = synth.ERR_INVALID_ARG
    assert _status(images, entries, stamps) in (0, synth.ERR_NO_DEVICE)       # the call itself is well formed

    def changed(field, k, value):
        e = entries.copy()
        e[field][k] = value
        return e
    assert _status(images, changed("h1", 0, 71), stamps) == INV               # a box outside its image
    assert _status(images, changed("w0", 1, 0), stamps) == INV
    assert _status(images, changed("h0", 1, entries["h1"][1] + 1), stamps) == INV   # an empty box
    assert _status(images, changed("stamp", 0, 2), stamps) == INV             # stamp index out of range
    assert _status(images, changed("stamp", 2, -1), stamps) == INV
    assert _status(images, changed("stamp", 1, 99), stamps) in (0, synth.ERR_NO_DEVICE)   # (a galaxy's is ignored)
    assert _status(images, entries[[1, 0, 2, 3]], stamps) == INV              # not sorted by (image, source)
    assert _status(images, entries[[2, 3, 0, 1]], stamps) == INV
    assert _status(images, entries[[0, 0, 2, 3]], stamps) == INV              # a pair twice
    assert _status(images, changed("image", 3, 2), stamps) == INV             # an image that is not there
    for K in (0, 5):                                                          # K outside 1..4
        arr = (synth.SynthImageT * 1)()
        sky, iota, psf, px = np.zeros((8, 8), np.float32), np.ones(8, np.float32), np.ones((5, 6)), np.zeros((8, 8), np.float32)
        arr[0].H, arr[0].W, arr[0].psf_K = 8, 8, K
        arr[0].sky, arr[0].nelec_per_nmgy = sky.ctypes.data_as(C.POINTER(C.c_float)), iota.ctypes.data_as(C.POINTER(C.c_float))
        arr[0].psf, arr[0].pixels_out = psf.ctypes.data_as(C.POINTER(C.c_double)), px.ctypes.data_as(C.POINTER(C.c_float))
        assert slib.celeste_synth_generate(0, 1, arr, 0, None, 0, None, 0, 0, 0, None) == INV
    assert slib.celeste_synth_generate(0, 0, None, 0, None, 0, None, 0, 0, 0, None) == INV
    assert _status(images, entries, stamps, want_pixels=False, want_lambda=False) == INV    # nothing asked for
    assert _status(images, entries, stamps, chunk_tiles=-1) == INV
    assert slib.celeste_synth_sample(0, 4, None, 0, 0, 0, None, None) == INV
    assert slib.celeste_synth_sample(-1, 0, None, 0, 0, 0, None, None) == INV
    assert slib.celeste_synth_last_ms(None) == INV


def test_entry_table_is_the_geometry_of_render_expected_image():
    """boxes, positions and fluxes against ImagePatch.from_box, source by source: rounding ties, clamped and empty boxes,
    world offsets and a variable PSF map's stamps"""
    from celeste_jl_amd import synth, synthetic
    from celeste_jl_amd.model import ImagePatch, box_around_point
    images = synthetic.variable_images(97, 123, seed=5)[:2] + synthetic.blank_images(97, 123)[2:3]
    images[2].wcs_world0 = np.array([30.0, -20.0])
    catalog = [synthetic.sample_ce(p, s) for p, s in (([1.2, 1.7], True), ([96.6, 122.4], False), ([48.5, 61.5], True),
                                                      ([-10.0, 60.0], True), ([-40.0, 60.0], False), ([126.5, 50.5], True))]
    entries, stamps = synth.entry_table(images, catalog)
    k = 0
    for n, img in enumerate(images):
        for s, ce in enumerate(catalog):
            p = ImagePatch.from_box(img, box_around_point(img, ce.pos, 25))
            (h0, h1), (w0, w1) = p.box
            if h1 < h0 or w1 < w0:
                continue
            e = entries[k]; k += 1
            assert (e["image"], e["source"], e["h0"], e["h1"], e["w0"], e["w1"]) == (n, s, h0, h1, w0, w1)
            m = p.wcs_jacobian @ (np.asarray(ce.pos, float) - p.world_center) + p.pixel_center
            np.testing.assert_allclose(e["m"], m, rtol=0, atol=1e-12)
            assert e["flux"] == (ce.star_fluxes if ce.is_star else ce.gal_fluxes)[img.b - 1] and bool(e["is_star"]) == ce.is_star
            if ce.is_star:
                np.testing.assert_allclose(stamps[e["stamp"]].reshape(51, 51).T, p.stamp, rtol=0, atol=1e-15)
    assert k == len(entries) and k < len(images) * len(catalog)
    assert synth.entry_table(images, [])[0].size == 0


def test_device_none_leaves_the_host_generator_as_it_was():
    """gen_images and make_field with device=None against a direct restatement of the host path: the catalog draws, then one
    rng.poisson per image from the same generator"""
    from celeste_jl_amd import synthetic
    f = synthetic.make_field(60, 64, 3, seed=3, device=None)
    g = synthetic.make_field(60, 64, 3, seed=3)
    rng = np.random.Generator(np.random.PCG64(3))
    prior = synthetic.load_prior()
    catalog = []
    for _ in range(3):
        pos = (rng.uniform(26, 60 - 26), rng.uniform(26, 64 - 26))
        catalog.append(synthetic.draw_source(prior, rng, pos))
    for n, img in enumerate(synthetic.blank_images(60, 64)):
        el = synthetic.render_expected_image(img, catalog) * img.nelec_per_nmgy.astype(np.float64)[:, None]
        want = rng.poisson(el).astype(np.float64).astype(np.float32)
        assert f.images[n].pixels.dtype == np.float32
        assert np.array_equal(f.images[n].pixels, want) and np.array_equal(g.images[n].pixels, want)
    for a, b in zip(catalog, f.catalog):
        assert np.array_equal(a.pos, b.pos) and a.is_star == b.is_star
    imgs = synthetic.blank_images(60, 64)
    synthetic.gen_images(imgs, catalog, np.random.Generator(np.random.PCG64(11)), device=None)
    r2 = np.random.Generator(np.random.PCG64(11))
    for img in imgs:
        el = synthetic.render_expected_image(img, catalog) * img.nelec_per_nmgy.astype(np.float64)[:, None]
        assert np.array_equal(img.pixels, r2.poisson(el).astype(np.float32))
    m = synthetic.make_multifield(grid=(1, 2), H=40, W=40, n_sources=4, seed=5, device=None)
    m2 = synthetic.make_multifield(grid=(1, 2), H=40, W=40, n_sources=4, seed=5)
    assert all(np.array_equal(a.pixels, b.pixels) for a, b in zip(m.images, m2.images))
