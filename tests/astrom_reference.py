"""The per-exposure astrometry of include/celeste_astrom.h, restated in numpy / torch (fp64, sums in np.longdouble) -- test
infrastructure.

Written from the header's text, not from the kernel: whole-patch arrays; the densities of tests/torch_value_model.py evaluated
on the shifted grid (fit_reference._Light's expression at hh - d1, ww - d2) with their derivatives from torch.autograd, never
from hand-written derivative code; B and the visited masks from fit_reference.expected_nmgy.  It holds
  the header's iteration, restated (iterate), with the margins of its decisions;
  an independent root theta* (root): Newton on the OBSERVED information, the Hessian of -l from autograd;
  the contraction r = rho(I - inv(F) J) of Fisher scoring at that root (contraction);
  the summaries (summarise).
For every sum it also returns sum |term|, which conditions a comparison of the sums.
"""
from dataclasses import dataclass, field

import numpy as np
import torch

import fit_reference as FR
import torch_value_model as tvm
from celeste_jl_amd import cabi

DT = torch.float64
LD = np.longdouble
OK, NO_LIGHT, TOO_FAINT, OUT_OF_RANGE, STALLED, NOT_CONVERGED, BAD_MODEL = range(7)
NO_EPOCHS, NO_MOTION = 1, 2
MAX_STEP_PX, LS_MIN_DEC, MAX_HALVINGS = 0.5, 1e-3, 8
TRI = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
DEFAULTS = dict(tol_sigma=1e-6, max_iters=50, max_sigma_px=0.2, max_shift_px=2.0)


def full3(p):
    out = np.empty((3, 3), dtype=np.asarray(p).dtype)
    for q, (k, l) in enumerate(TRI):
        out[k, l] = out[l, k] = p[q]
    return out


def pack3(M):
    return np.array([M[k, l] for k, l in TRI])


@dataclass
class Pass:
    l: float
    U: np.ndarray            # [3]
    F: np.ndarray            # [6] packed
    chi2: float
    sound: bool
    light: bool
    abs_l: float = 0.0
    abs_U: np.ndarray = None
    abs_F: np.ndarray = None
    abs_chi2: float = 0.0
    sum_a: float = 0.0


@dataclass
class Step:
    ok: bool
    p: np.ndarray = None
    dec: float = np.nan
    cov: np.ndarray = None   # [6] packed inv(F)


def step_of(F, U) -> Step:
    """the header's step of a pass, in extended precision"""
    F, U = np.asarray(F, dtype=LD), np.asarray(U, dtype=LD)
    M = full3(F)
    d = np.array([M[0, 0], M[1, 1], M[2, 2]])
    if not (np.isfinite(d).all() and (d > 0).all()):
        return Step(False)
    s = np.sqrt(d)
    R = M / np.outer(s, s)
    L = np.zeros((3, 3), dtype=LD)
    for j in range(3):
        piv = LD(1) - sum(L[j, k] ** 2 for k in range(j))          # R's diagonal is 1
        if not (np.isfinite(piv) and piv > 0):
            return Step(False)
        L[j, j] = np.sqrt(piv)
        for i in range(j + 1, 3):
            L[i, j] = (R[i, j] - sum(L[i, k] * L[j, k] for k in range(j))) / L[j, j]
    v = U / s
    z = np.zeros(3, dtype=LD)
    for i in range(3):
        z[i] = (v[i] - sum(L[i, k] * z[k] for k in range(i))) / L[i, i]
    y = np.zeros(3, dtype=LD)
    for i in (2, 1, 0):
        y[i] = (z[i] - sum(L[k, i] * y[k] for k in range(i + 1, 3))) / L[i, i]
    Li = np.zeros((3, 3), dtype=LD)
    for j in range(3):
        e = np.zeros(3, dtype=LD); e[j] = 1
        for i in range(3):
            Li[i, j] = (e[i] - sum(L[i, k] * Li[k, j] for k in range(i))) / L[i, i]
    cov = (Li.T @ Li) / np.outer(s, s)
    return Step(True, y / s, float(np.sqrt((z * z).sum())), pack3(cov))


class Entry:
    """one (target, image) pair: whole-patch arrays and the shifted light as a torch function of delta"""

    def __init__(self, light, images, patches, vp, s, n, visited, B):
        self.image, self.band = n, images[n].b - 1
        img, pa = images[n], patches[s][n]
        self.patch = pa
        H2, W2 = visited.shape
        h0, w0 = pa.bitmap_offset
        self.visited = visited
        self.n_pix = int(visited.sum())
        self.own = visited & (np.arange(1, W2 + 1)[None, :] < W2)
        self.iota = np.broadcast_to(img.nelec_per_nmgy[h0:h0 + H2].astype(np.float64)[:, None], (H2, W2))
        sky = img.sky[h0:h0 + H2, w0:w0 + W2].astype(np.float64)
        self.b = self.iota * (sky + B)
        self.x = np.where(visited, img.pixels[h0:h0 + H2, w0:w0 + W2].astype(np.float64), 0.0)
        self.J = np.asarray(pa.wcs_jacobian, dtype=np.float64)
        self.finite = bool(light.finite[s])
        hh = torch.arange(h0 + 1, h0 + H2 + 1, dtype=DT)[:, None].expand(H2, W2)
        ww = torch.arange(w0 + 1, w0 + W2 + 1, dtype=DT)[None, :].expand(H2, W2)
        vs = light.vp[s]
        if self.finite:
            Jt = torch.tensor(self.J, dtype=DT)
            m = Jt @ (vs[0:2] - torch.tensor(np.asarray(pa.world_center), dtype=DT)) + torch.tensor(np.asarray(pa.pixel_center), dtype=DT)
            coef = light.coef(pa.stamp)
            c = [vs[26 + i] * tvm.brightness(vs, i, self.band)[0] for i in range(2)]

            def shifted(d):
                f0 = tvm.star_density(coef, hh - d[0] - m[0] + 26, ww - d[1] - m[1] + 26)
                f1 = tvm.galaxy_density(pa.psf, m, vs[2], vs[3], vs[4], vs[5], hh - d[0], ww - d[1])
                return c[0] * f0 + c[1] * f1
            self._shifted = shifted
        self.result = None

    # -- the model --------------------------------------------------------------------------------------------------------
    def light(self, delta):
        """m(delta) [H2, W2] and dm / d delta [2, H2, W2] from autograd; 0 where the own light does not count.  A pixel's light
        depends on delta through its own shifted coordinates only, so one reverse pass over per-pixel copies of delta yields
        every pixel's gradient."""
        if not self.finite:
            z = np.full(self.visited.shape, np.nan)
            return np.where(self.own, z, 0.0), np.where(self.own[None], np.stack([z, z]), 0.0)
        shape = self.visited.shape
        D = [torch.full(shape, float(delta[k]), dtype=DT, requires_grad=True) for k in range(2)]
        val = self._shifted(D)
        g = torch.autograd.grad(val.sum(), D)
        m, dm = val.detach().numpy(), np.stack([g[0].numpy(), g[1].numpy()])
        return np.where(self.own, m, 0.0), np.where(self.own[None], dm, 0.0)

    def evaluate(self, theta) -> Pass:
        """one pass at theta = (d1, d2, alpha), sums in extended precision"""
        theta = np.asarray(theta, dtype=np.float64)
        m, dm = self.light(theta[:2])
        v = self.visited
        a, g0, g1 = (self.iota * m)[v].astype(LD), (self.iota * dm[0])[v].astype(LD), (self.iota * dm[1])[v].astype(LD)
        b, x = self.b[v].astype(LD), self.x[v].astype(LD)
        al = LD(theta[2])
        lam = b + al * a
        with np.errstate(invalid="ignore"):
            good = np.isfinite(lam) & (lam > 0)
        sound = bool(good.all())
        light = bool((a > 0).any())
        a, g0, g1, b, x, lam = (t[good] for t in (a, g0, g1, b, x, lam))
        D = [al * g0, al * g1, a]
        r = x / lam - 1
        tl = x * np.log(lam) - lam
        tU = [Dk * r for Dk in D]
        tF = [D[k] * D[l] / lam for k, l in TRI]
        tc = (x - lam) ** 2 / lam
        f = lambda t: float(t.sum())
        return Pass(f(tl), np.array([t.sum() for t in tU]), np.array([t.sum() for t in tF]), f(tc), sound, light,
                    f(np.abs(tl)), np.array([np.abs(t).sum() for t in tU]), np.array([np.abs(t).sum() for t in tF]),
                    f(np.abs(tc)), f(a))

    def b_sound(self):
        bv = self.b[self.visited]
        with np.errstate(invalid="ignore"):
            return bool(np.isfinite(bv).all() and (bv > 0).all())

    # -- autograd of the whole likelihood: the observed information ------------------------------------------------------------
    def _loglik_torch(self, th):
        v = torch.tensor(self.visited)
        own = torch.tensor(self.own)
        m = torch.where(own, self._shifted(th[:2]), torch.zeros((), dtype=DT))
        lam = torch.tensor(self.b, dtype=DT) + th[2] * torch.tensor(np.array(self.iota), dtype=DT) * m
        lam = torch.where(v, lam, torch.ones((), dtype=DT))
        x = torch.tensor(self.x, dtype=DT)
        return torch.where(v, x * torch.log(lam) - lam, torch.zeros((), dtype=DT)).sum()

    def score_and_observed(self, theta):
        """(grad l [3], J = -Hessian of l [3, 3]) from autograd"""
        th = torch.tensor(np.asarray(theta, dtype=np.float64), dtype=DT, requires_grad=True)
        g = torch.autograd.functional.jacobian(self._loglik_torch, th)
        H = torch.autograd.functional.hessian(self._loglik_torch, th)
        return g.numpy(), -H.numpy()

    def root(self, start, max_steps=60):
        """theta*: Newton on the observed information from `start`, until the step is below 1e-13 standard errors (or it stops
        shrinking); returns (theta*, last step length in standard errors)"""
        th = np.asarray(start, dtype=np.float64).copy()
        last = np.inf
        for _ in range(max_steps):
            g, J = self.score_and_observed(th)
            p = np.linalg.solve(J, g)
            size = float(np.sqrt(abs(p @ J @ p)))
            th = th + p
            if size < 1e-13 or size >= last and size < 1e-10:
                return th, size
            last = size
        return th, last

    def contraction(self, theta):
        """r = rho(I - inv(F) J) at theta: the linear rate of Fisher scoring near its fixed point"""
        F = full3(self.evaluate(theta).F).astype(np.float64)
        _, J = self.score_and_observed(theta)
        return float(np.abs(np.linalg.eigvals(np.eye(3) - np.linalg.solve(F, J))).max())


@dataclass
class Result:
    flag: int
    iters: int
    theta: np.ndarray                   # (d1, d2, alpha), NaN where the header says so
    F: np.ndarray                       # [6]
    cov: np.ndarray                     # [6]
    chi2: float
    loglik: float
    margin: float = np.inf              # the smallest |log ratio| of a decision of the iteration (gate, dec tests, range)
    halvings: int = 0
    decs: list = field(default_factory=list)


def _lr(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        v = abs(float(np.log(LD(a) / LD(b))))
    return v if np.isfinite(v) else np.inf


def iterate(e: Entry, tol_sigma=1e-6, max_iters=50, max_sigma_px=0.2, max_shift_px=2.0) -> Result:
    """the header's iteration, restated"""
    nan3, nan6 = np.full(3, np.nan), np.full(6, np.nan)
    if not e.finite or not e.b_sound():
        return Result(BAD_MODEL, 0, nan3, nan6, nan6, np.nan, np.nan)
    theta = np.array([0.0, 0.0, 1.0])
    cur = e.evaluate(theta)
    iters = 1
    if not cur.sound:
        return Result(BAD_MODEL, 1, nan3, nan6, nan6, np.nan, np.nan)
    if not cur.light:
        return Result(NO_LIGHT, 1, nan3, nan6, nan6, cur.chi2, cur.l)
    st = step_of(cur.F, cur.U)
    if not st.ok:
        return Result(TOO_FAINT, 1, nan3, cur.F, nan6, cur.chi2, cur.l)
    sig = float(np.sqrt(max(st.cov[0], st.cov[3])))
    margin = _lr(sig, max_sigma_px)
    if sig > max_sigma_px:
        return Result(TOO_FAINT, 1, nan3, cur.F, np.asarray(st.cov, dtype=np.float64), cur.chi2, cur.l, margin)
    halv, decs = 0, []

    def done(flag, cov=None):
        return Result(flag, iters, theta.copy(), cur.F, np.asarray(st.cov if cov is None else cov, dtype=np.float64), cur.chi2,
                      cur.l, margin, halv, decs)
    while True:
        decs.append(st.dec)
        margin = min(margin, _lr(st.dec, tol_sigma), _lr(st.dec, LS_MIN_DEC))
        if st.dec <= tol_sigma:
            return done(OK)
        if iters >= max_iters:
            return done(NOT_CONVERGED)
        p = np.asarray(st.p, dtype=np.float64)
        big = max(abs(p[0]), abs(p[1]))
        if big > 0:
            margin = min(margin, _lr(big, MAX_STEP_PX))
        if big > MAX_STEP_PX:
            p = p * (MAX_STEP_PX / big)
        t, h = 1.0, 0
        while True:
            trial = theta + t * p
            tp = e.evaluate(trial)
            iters += 1
            if st.dec > LS_MIN_DEC and tp.sound:
                # how far the likelihood test is from depending on rounding: the difference against the sums' rounding
                margin = min(margin, abs(tp.l - cur.l) / (1e-12 * max(cur.abs_l, 1e-300)) if abs(tp.l - cur.l) < 1e-12 * cur.abs_l else np.inf)
            reject = (not tp.sound) or (st.dec > LS_MIN_DEC and tp.l < cur.l)
            if not reject:
                break
            if h == MAX_HALVINGS:
                return done(STALLED)
            if iters >= max_iters:
                return done(NOT_CONVERGED)
            h += 1
            halv += 1
            t *= 0.5
        theta, cur = trial, tp
        st = step_of(cur.F, cur.U)
        if not st.ok:
            return done(STALLED, nan6)
        margin = min(margin, _lr(max(abs(theta[0]), 1e-300), max_shift_px), _lr(max(abs(theta[1]), 1e-300), max_shift_px))
        if abs(theta[0]) > max_shift_px or abs(theta[1]) > max_shift_px:
            return done(OUT_OF_RANGE)


# ---- summaries ---------------------------------------------------------------------------------------------------------------
def entry_weight(J, delta, F6):
    """Delta_n [2] and W_n [2, 2] of an entry"""
    J, F = np.asarray(J, dtype=np.float64), full3(np.asarray(F6, dtype=np.float64))
    S = F[:2, :2] - np.outer(F[:2, 2], F[2, :2]) / F[2, 2]
    return np.linalg.solve(J, np.asarray(delta, dtype=np.float64)), J.T @ S @ J


def summarise(rows, epochs=None):
    """rows: [(image, flag, delta [2], F [6], J [2, 2])] of one target in image order -> (n_epochs, summary_flag, summary [22])"""
    out = np.full(22, np.nan)
    ok = [r for r in rows if r[1] == OK]
    n = len(ok)
    if n == 0:
        return 0, NO_EPOCHS | NO_MOTION, out
    t = np.array([float(r[0]) if epochs is None else float(epochs[r[0]]) for r in ok])
    DW = [entry_weight(r[4], r[2], r[3]) for r in ok]
    SW = sum(W for _, W in DW)
    try:
        np.linalg.cholesky(SW)
    except np.linalg.LinAlgError:
        return n, NO_EPOCHS | NO_MOTION, out
    mean = np.linalg.solve(SW, sum(W @ D for D, W in DW))
    mc = np.linalg.inv(SW)
    out[0:2], out[2:5] = mean, [mc[0, 0], mc[0, 1], mc[1, 1]]
    out[5] = sum((D - mean) @ W @ (D - mean) for D, W in DW)
    tref = t.sum() / n
    tau = t - tref
    N4 = sum(np.kron(np.array([[1.0, tk], [tk, tk * tk]]), W) for tk, (_, W) in zip(tau, DW))
    r4 = sum(np.concatenate([W @ D, tk * (W @ D)]) for tk, (D, W) in zip(tau, DW))
    out[21] = tref
    if len(set(t.tolist())) < 2:
        return n, NO_MOTION, out
    try:
        np.linalg.cholesky(N4)
    except np.linalg.LinAlgError:
        return n, NO_MOTION, out
    beta, bc = np.linalg.solve(N4, r4), np.linalg.inv(N4)
    out[6:10] = beta
    out[10:20] = [bc[k, l] for k in range(4) for l in range(k, 4)]
    out[20] = sum((D - beta[:2] - beta[2:] * tk) @ W @ (D - beta[:2] - beta[2:] * tk) for tk, (D, W) in zip(tau, DW))
    return n, 0, out


# ---- whole calls -------------------------------------------------------------------------------------------------------------
def entries_of(images, patches, neighbors, vp, target, expected=None):
    """the entries of one target in image order, not yet iterated"""
    light = FR._Light(images, patches, vp)
    visits = expected if expected is not None else FR.expected_nmgy(images, patches, neighbors, vp, target)
    return [Entry(light, images, patches, vp, target, n, visited, B) for n, visited, E, m, B in visits]


@dataclass
class AstromReference:
    entries: list            # per target: [Entry], each with .result
    n_epochs: np.ndarray     # [T]
    summary_flag: np.ndarray
    summary: np.ndarray      # [T, 22]
    status: np.ndarray       # [T]
    flat: list = field(default_factory=list)

    @property
    def offsets(self):
        return np.concatenate([[0], np.cumsum([len(r) for r in self.entries])]).astype(np.int64)


def astrom_reference(images, patches, neighbors, vp, targets, epochs=None, **params) -> AstromReference:
    vp = np.asarray(vp, dtype=np.float64)
    kw = dict(DEFAULTS, **params)
    rows, ne, sf, sm, status = [], [], [], [], np.zeros(len(targets), dtype=np.int32)
    for ti, s in enumerate(targets):
        row = entries_of(images, patches, neighbors, vp, s)
        for e in row:
            e.result = iterate(e, **kw)
        if not np.isfinite(vp[s]).all():
            status[ti] = cabi.ERR_NONFINITE_INPUT
        elif any(e.result.flag == BAD_MODEL for e in row):
            status[ti] = cabi.ERR_NONFINITE_RESULT
        n, fl, out = summarise([(e.image, e.result.flag, e.result.theta[:2], e.result.F, e.J) for e in row], epochs)
        rows.append(row); ne.append(n); sf.append(fl); sm.append(out)
    T = len(targets)
    return AstromReference(rows, np.array(ne, dtype=np.int32).reshape(T), np.array(sf, dtype=np.int32).reshape(T),
                           np.array(sm).reshape(T, 22), status, [e for r in rows for e in r])


# ---- scenes shared by the host and the device tests -----------------------------------------------------------------------------
_SCENES = {}
MOVED_SEED = 5
MOVED_SHIFT = (0.4, -0.3)


def _brightest(catalog):
    return int(np.argmax([ce.star_fluxes[2] if ce.is_star else ce.gal_fluxes[2] for ce in catalog]))


def moved_scene(seed=MOVED_SEED):
    """Three exposures of five bands (15 images: image 5 e + band) of one 64 x 80 region with 6 prior-drawn sources; the
    brightest one in r is rendered MOVED_SHIFT pixels (rows, columns) away in the second exposure only.  Returns (Field, index
    of that source)."""
    if ("moved", seed) not in _SCENES:
        import copy
        from celeste_jl_amd import synthetic
        from celeste_jl_amd.model import get_sky_patches, neighbor_map
        f0 = synthetic.make_field(64, 80, 6, seed=seed, margin=12, perturb=False)
        catalog = f0.catalog
        mv = _brightest(catalog)
        moved = copy.deepcopy(catalog)
        img0 = f0.images[0]
        pix = np.asarray(img0.world_to_pix(catalog[mv].pos), dtype=np.float64) + np.array(MOVED_SHIFT)
        moved[mv].pos = np.asarray(img0.pix_to_world(pix), dtype=np.float64)
        images = list(f0.images)
        for e, cat in ((1, moved), (2, catalog)):
            more = synthetic.blank_images(64, 80)
            synthetic.gen_images(more, cat, np.random.Generator(np.random.PCG64([seed, e])))
            images += more
        patches = get_sky_patches(images, catalog)
        _SCENES["moved", seed] = (synthetic.Field(images, catalog, patches, neighbor_map(patches), f0.vp.copy(), "moved"), mv)
    return _SCENES["moved", seed]
