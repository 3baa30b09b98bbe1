"""The tangent-plane scene of tests/test_wcs_host.py and tests/test_gpu_wcs.py: three overlapping fields of 64 x 80 pixels x 5
bands around (ra, dec) = (359.9995, 60) -- the fields straddle RA 0 -- turned by 0, 30 and 90 degrees, the third with flipped
parity, and 12 sources drawn up to 30 pixels outside the mosaic.  Test infrastructure, not product code."""
import math

import numpy as np

# model.TanWCS against mpmath, measured by tests/test_wcs_host.py on an SDSS-sized frame (glibc's libm): 1.48e-12 px, 2.83e-14
# degrees (half an ulp of an RA near 360), 8.55e-10 relative for the Jacobian (the recipe divides that half ulp, 2.6e-10 px, by
# its half-pixel step); the bounds are 10 times that (libm differs between machines), at most 1e-8
BOUND_PX, BOUND_DEG, BOUND_JAC = 10 * 1.48e-12, 10 * 2.83e-14, 10 * 8.55e-10
assert BOUND_PX <= 1e-8 and BOUND_JAC <= 1e-8

CRVAL = (359.9995, 60.0)
SCALE = 0.396 / 3600.0            # degrees per pixel
ROTATIONS = [0.0, 30.0, (90.0, True)]
H, W, N_SOURCES, MARGIN = 64, 80, 12, -30
OVERRIDE = 6.3
# chosen on the CPU by find_seed(): one source off every image, one outside an image but within reach of its edge, and no
# pc -/+ r of the host table within 1e-6 of a rounding tie in either radius mode
SEED = 16


def tan_multifield(seed=SEED, **kw):
    from celeste_jl_amd import synthetic
    return synthetic.make_multifield(grid=(1, 3), H=H, W=W, overlap=0.25, n_sources=N_SOURCES, seed=seed, margin=MARGIN, wcs="tan",
                                     crval=CRVAL, pixel_scale_deg=SCALE, rotations=ROTATIONS, **kw)


def tie_distance(images, catalog, override):
    """the smallest distance of a pc -/+ r of a tried pair from a rounding tie (x.5), over the pairs whose pixel coordinates
    are finite; r as get_sky_patches chooses it"""
    from celeste_jl_amd import model
    cache, best = {}, math.inf
    reach = (25.0 if math.isnan(override) else override) + 1.0
    for img in images:
        for ce in catalog:
            pc = img.world_to_pix(ce.pos)
            if not np.isfinite(pc).all():
                continue
            if not (-reach < pc[0] < img.H + 1 + reach and -reach < pc[1] < img.W + 1 + reach):
                continue      # (a dense table keeps such a pair too: its box is empty by a wide margin)
            r = override if not math.isnan(override) else model.choose_patch_radius(ce, img, width_scale=1.2, _cache=cache)
            for x in (pc[0] - r, pc[0] + r, pc[1] - r, pc[1] + r):
                best = min(best, abs((x - math.floor(x)) - 0.5))
    return best


def placement(images, catalog, reach=26.0):
    """(sources off every image and beyond reach of all, sources outside some image but within reach of its edge)"""
    off, near = [], []
    for s, ce in enumerate(catalog):
        inside = within = edge = False
        for img in images:
            pc = img.world_to_pix(ce.pos)
            i = 0.5 <= pc[0] <= img.H + 0.5 and 0.5 <= pc[1] <= img.W + 0.5
            w = -reach < pc[0] < img.H + 1 + reach and -reach < pc[1] < img.W + 1 + reach
            inside |= i
            within |= w
            edge |= (w and not i)
        if not within:
            off.append(s)
        elif not inside and edge:
            near.append(s)
    return off, near


def scene_ok(f):
    off, near = placement(f.images, f.catalog)
    return bool(off) and bool(near) and tie_distance(f.images, f.catalog, math.nan) > 1e-6 and \
        tie_distance(f.images, f.catalog, OVERRIDE) > 1e-6


def find_seed(limit=200):
    for seed in range(limit):
        if scene_ok(tan_multifield(seed, perturb=False)):
            return seed
    return None
