"""Small hand-made planes for the edges of source detection that random fields leave to chance (test infrastructure).

tests/test_detect_scenes_host.py states what each plane holds, on the restatement (tests/detect_reference.py) alone;
tests/test_gpu_detect_edges.py compares the device with the restatement on them.  A plane is a (pixels, sky, nelec_per_nmgy)
triple with named fields, which detect.extract accepts.  nelec_per_nmgy is a power of two that changes from row to row and
the sky is 0.5 (0 under the painted plane), so the planes calibrate exactly to the values written here.
"""
import collections
import functools

import numpy as np

import detect_reference as R

Plane = collections.namedtuple("Plane", "pixels sky nelec_per_nmgy")
S = 2.0 ** -6             # the amplitude of the painted plane's background
Q = 11 * S / 32           # the unit of what is painted on it


def plane(cal, sky=0.5):
    """the plane that calibrates to `cal` (float32 values with a few spare bits, or any float32 values with sky=0)"""
    cal = np.asarray(cal, np.float32)
    H, W = cal.shape
    nelec = (2.0 ** (np.arange(H) % 3)).astype(np.float32)
    sky = np.full((H, W), sky, np.float32)
    px = ((cal.astype(np.float64) + sky) * nelec[:, None].astype(np.float64)).astype(np.float32)
    p = Plane(px, sky, nelec)
    got = R.calibrate(px, sky, nelec)
    assert np.array_equal(got, cal, equal_nan=True)
    return p


def noise(H, W, sigma, seed):
    """Gaussian noise on a grid of 2^-10, so that a plane of it calibrates exactly"""
    v = np.random.default_rng(seed).normal(0.0, sigma, (H, W))
    return (np.round(v * 1024.0) / 1024.0).astype(np.float32)


def blob(cal, ci, cj, flux, sigma):
    H, W = cal.shape
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    v = flux * np.exp(-0.5 * ((ii - ci) ** 2 + (jj - cj) ** 2) / sigma ** 2) / (2 * np.pi * sigma ** 2)
    cal += (np.round(v * 1024.0) / 1024.0).astype(np.float32)


# ---- the background mesh ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fill_tie(transposed=False):
    """520 x 24: three mesh cells in a row.  The middle one is more than half NaN, so it takes the value of the nearest
    good cell: cells 0 and 2 are equally near, and their noise differs by a factor of 3.  A bright blob in cell 0 is a
    detection under cell 0's rms and none under cell 2's."""
    cal = np.empty((520, 24), np.float32)
    cal[:256] = noise(256, 24, 1.0, 1)
    cal[256:512] = noise(256, 24, 2.0, 2)
    cal[512:] = noise(8, 24, 3.0, 3)
    cal[256:512].reshape(-1)[np.random.default_rng(4).permutation(256 * 24)[:256 * 24 // 2 + 40]] = np.nan
    blob(cal, 100.0, 12.0, 100.0, 2.0)
    return plane(cal.T.copy() if transposed else cal)


@functools.lru_cache(maxsize=None)
def half_valid(extra_nan):
    """16 x 12, one cell: exactly half of its pixels NaN (a good cell), or one more (a bad one: no rms, no detection)"""
    cal = noise(16, 12, 1.0, 5)
    blob(cal, 5.0, 4.0, 300.0, 1.2)
    order = np.random.default_rng(6).permutation(16 * 12)
    order = order[~np.isin(order, [i * 12 + j for i in range(2, 9) for j in range(1, 8)])]     # (the blob stays)
    cal.reshape(-1)[order[:96 + extra_nan]] = np.nan
    return plane(cal)


@functools.lru_cache(maxsize=None)
def median_gap():
    """16 x 12, one cell: a checkerboard of 0 and 2 S with two pixels at -2.5 S and two at 4.5 S.  The count is even and the two
    middle values are 0 and 2 S: around their mean S the first pass clips all four, around the upper one only the low two."""
    ii, jj = np.meshgrid(np.arange(16), np.arange(12), indexing="ij")
    cal = np.where((ii + jj) % 2 == 0, 2 * S, 0.0)
    cal[3, 3] = cal[10, 7] = -2.5 * S          # (one on each colour of the board)
    cal[5, 8] = cal[12, 4] = 4.5 * S
    return plane(cal)


# ---- hand-painted components --------------------------------------------------------------------------------------
# The background is a checkerboard of 0 and 2 S, which the 3 x 3 filter takes to exactly S away from the border.  What is
# painted on top is a multiple of Q / 2, so every convolved value is exact and known: a lone pixel of 16 Q adds 4 Q at its
# centre, 2 Q at its four edge neighbours and 1 Q at its corners.  The faint paint stays inside the clipping range, so the
# rms is 1.075 S, and Q is chosen so that the threshold lies 1.157 Q above the filtered background: what adds 1.125 Q or
# less is outside the mask, what adds 1.375 Q or more is inside (tests/test_detect_scenes_host.py asserts the margin).
# No calibrated value is negative, so every moment is proper.
ANTI = (8, 11)            # centre of the upper right plus of the anti-diagonal pair; the lower left one is at (+2, -2)
FIVE = (8, 22)            # a lone plus: 5 = minarea pixels
FOUR = (8, 32)            # a 2 x 2 block: 4 = minarea - 1 pixels
NINE = (8, 40)            # a lone 3 x 3: 9 = 2 minarea - 1 pixels
PAIR = (20, 8)            # two pluses four columns apart and the pixel between them: 11 = 2 minarea + 1 pixels
TRIPLE = (33, 8)          # three 6 x 5 blobs in a row, the valley between the first two lower than between the last two
PLATEAU = (22, 30)        # a 6 x 7 plateau with a NaN pixel inside
EXACT = (22, 43)          # a lone pixel whose convolved value is the threshold itself
LOPSIDED = (50, 24)       # a broad pyramid with a bump on its lower left corner: the children's order is not the cores'


def _painted_cal(exact_value, q=Q):
    H, W = 64, 48
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    bg = np.where((ii + jj) % 2 == 0, 2 * S, 0.0)
    p = np.zeros((H, W))
    a, b = ANTI
    p[a, b] = p[a + 2, b - 2] = 16
    p[a - 1, b] = 0.5                                       # (no component is symmetric: x2 = y2 would leave theta to a rounding)
    p[FIVE] = 16
    a, b = FOUR
    p[a:a + 2, b:b + 2] = 4
    p[NINE] = 24
    p[NINE[0], NINE[1] + 1] = 1
    a, b = PAIR
    p[a, b] = p[a, b + 4] = 12
    p[a, b + 2] = 5.5
    a, b = TRIPLE
    for c in (b, b + 5, b + 9):
        p[a - 1:a + 3, c - 1:c + 2] = 16
    a, b = PLATEAU
    p[a:a + 4, b:b + 5] = 8
    a, b = LOPSIDED
    for r in range(7):                                      # a pyramid of 13 x 14 paints, and a bump on its corner
        p[a - 6 + r:a + 7 - r, b - 6 + r:b + 8 - r] += 6
    p[a + 4:a + 7, b - 6:b - 4] += 40
    cal = bg + p * q
    cal[ANTI[0] + 1, ANTI[1] - 1] = np.nan                  # the pixel both pluses would light: the link stays diagonal
    cal[PLATEAU[0] + 2, PLATEAU[1] + 1] = np.nan
    cal[EXACT] = exact_value
    return cal.astype(np.float32)


@functools.lru_cache(maxsize=None)
def painted():
    """64 x 48 with the components above.  The lone pixel at EXACT (background 0, its neighbours convolve to S) is
    4 thr - 4 S, which the filter takes to thr itself; it is inside the clipping range, so thr is found by iteration."""
    assert sum(EXACT) % 2 == 1
    v = np.float32(S)
    for _ in range(4):
        thr = np.float32(np.float32(1.3) * np.float32(R.global_rms(_painted_cal(v))))
        v = np.float32(np.float32(4.0) * thr - np.float32(4 * S))
    return plane(_painted_cal(v), sky=0.0)


# ---- batches and parameters ---------------------------------------------------------------------------------------

def _stars(H, W, centres, seed, flux=60.0, sigma=2.0):
    cal = noise(H, W, 0.03, seed)
    for ci, cj in centres:
        blob(cal, ci, cj, flux, sigma)
    return plane(cal)


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """four planes of different shapes, H != W: a lone star; two blended pairs and a lone star; nothing; a blended pair"""
    return (_stars(40, 56, [(20.0, 30.3)], 11),
            _stars(72, 48, [(15.0, 20.0), (24.0, 20.3), (50.0, 12.0), (50.3, 21.0), (60.0, 38.0)], 12),
            _stars(24, 31, [], 13),
            _stars(33, 47, [(16.0, 14.0), (16.3, 23.0)], 14))


DEFAULTS = dict(thresh=1.3, minarea=5, nthresh=32, cont=0.005)
OTHER = dict(thresh=2.0, minarea=3, nthresh=8, cont=0.05)


@functools.lru_cache(maxsize=None)
def parameters_plane():
    """60 x 52 on which each of the four parameters decides something: a faint star that shrinks under the higher threshold; a
    2 x 2 block that convolves to 4 pixels (minarea 3 keeps it, 5 does not); an equal pair 6 pixels apart whose valley lies
    between the two highest of 8 levels but below some of 32; a pair whose fainter member holds 3 % of the flux (a child at
    deblend_cont 0.005, none at 0.05)"""
    cal = noise(60, 52, 0.03, 21)
    blob(cal, 29.0, 10.0, 1.2, 1.6)
    cal[28:30, 40:42] += np.float32(0.15625)
    blob(cal, 44.0, 14.0, 60.0, 2.0)
    blob(cal, 44.3, 20.0, 60.0, 2.0)
    blob(cal, 14.0, 14.0, 60.0, 2.0)
    blob(cal, 14.3, 23.0, 2.4, 1.5)
    return plane(cal)


def restate(p, trace=None, **kw):
    return R.extract(p.pixels, p.sky, p.nelec_per_nmgy, trace=trace, **kw)
