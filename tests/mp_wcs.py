"""The tangent-plane (TAN) projection in 50-digit arithmetic (mpmath): what model.TanWCS and the prep library's TAN branch
are measured against.  Written from FITS WCS paper II (Calabretta & Greisen 2002, section 5.1.3:
the gnomonic projection and its inverse through the native sphere rotation) and from the reference's finite-difference
recipe (src/model/wcs_utils.jl:36-51), from the same fp64 inputs the code under test gets.

Test infrastructure, not product code."""
import numpy as np
from mpmath import mp, mpf

mp.dps = 50


def _m(x):
    return x if isinstance(x, mpf) else mpf(float(x))


class MpTan:
    def __init__(self, crval, crpix, cd):
        self.ra0, self.dec0 = _m(crval[0]), _m(crval[1])
        self.p0 = [_m(crpix[0]), _m(crpix[1])]
        cd = np.asarray(cd, dtype=np.float64).reshape(2, 2)
        self.cd = [[_m(cd[0, 0]), _m(cd[0, 1])], [_m(cd[1, 0]), _m(cd[1, 1])]]
        self.d2r = mp.pi / 180

    def world_to_pix(self, ra, dec):
        """(h, w), or None behind the tangent plane"""
        da = (_m(ra) - self.ra0) * self.d2r
        d, d0 = _m(dec) * self.d2r, self.dec0 * self.d2r
        l = mp.cos(d) * mp.sin(da)
        m = mp.sin(d) * mp.cos(d0) - mp.cos(d) * mp.sin(d0) * mp.cos(da)
        n = mp.sin(d) * mp.sin(d0) + mp.cos(d) * mp.cos(d0) * mp.cos(da)
        if n <= 0:
            return None
        x, y = l / n / self.d2r, m / n / self.d2r
        (a, b), (c, e) = self.cd
        det = a * e - b * c
        return (self.p0[0] + (e * x - b * y) / det, self.p0[1] + (-c * x + a * y) / det)

    def pix_to_world(self, h, w):
        """(ra, dec) in degrees, ra within 180 degrees of crval[0]"""
        u, v = _m(h) - self.p0[0], _m(w) - self.p0[1]
        x = (self.cd[0][0] * u + self.cd[0][1] * v) * self.d2r
        y = (self.cd[1][0] * u + self.cd[1][1] * v) * self.d2r
        d0 = self.dec0 * self.d2r
        den = mp.cos(d0) - y * mp.sin(d0)
        num = mp.sin(d0) + y * mp.cos(d0)
        return (self.ra0 + mp.atan2(x, den) / self.d2r, mp.atan2(num, mp.sqrt(x * x + den * den)) / self.d2r)

    def jacobian(self, h, w, pixel_delt=0.5):
        """pixel_world_jacobian, the recipe itself (step rule and all) in 50 digits: [[J11, J12], [J21, J22]]"""
        h, w, dl = _m(h), _m(w), _m(pixel_delt)
        ra, dec = self.pix_to_world(h, w)
        ra2, dec2 = self.pix_to_world(h + dl, w + dl)
        t = max(abs(ra2 - ra), abs(dec2 - dec))
        a = self.world_to_pix(ra + t, dec)
        b = self.world_to_pix(ra, dec + t)
        return [[(a[0] - h) / t, (b[0] - h) / t], [(a[1] - w) / t, (b[1] - w) / t]]

    def analytic_jacobian(self, h, w):
        """d pix / d world by 50-digit differentiation (what the recipe approximates)"""
        ra, dec = self.pix_to_world(_m(h), _m(w))
        f = lambda i, j: mp.diff(lambda t: self.world_to_pix(*((t, dec) if j == 0 else (ra, t)))[i], ra if j == 0 else dec)
        return [[f(0, 0), f(0, 1)], [f(1, 0), f(1, 1)]]


def pix_error(got, want):
    """largest |difference| of an fp64 (h, w) against the 50-digit pair"""
    return float(max(abs(_m(got[0]) - want[0]), abs(_m(got[1]) - want[1])))
