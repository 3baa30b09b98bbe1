"""Independent numpy / scipy restatement of source detection (DESIGN.md "Detection", steps 1-7) and of
detect_sources (detection.jl:39-171).  Test infrastructure: the product never imports it.

Coordinates follow SEP as the reference calls it: x = row index (axis 0), y = column index, raster order column-major
(index i + H*j).  Sums whose order the device fixes serially (deblending) are taken sequentially here as well
(np.cumsum); the per-object moments are compared with a tolerance.
"""
import math

import numpy as np
from scipy import ndimage

MESH = 256
EIGHT = np.ones((3, 3), dtype=int)


def calibrate(pixels, sky, nelec):
    """calibrated_pixels (image_model.jl:56): float32, one rounding per operation"""
    return (np.asarray(pixels, np.float32) / np.asarray(nelec, np.float32)[:, None]) - np.asarray(sky, np.float32)


def cell_rms(vals, median=np.median):
    """kappa-sigma clipping at 3 sigma around the median until no value leaves (at most 100 passes); fp64.  `median`: for
    the scenes' own tests, which show that another median rule gives another rms"""
    v = vals[~np.isnan(vals)].astype(np.float64)
    lo, hi = -np.inf, np.inf
    s = v
    sigma = float("nan")
    for it in range(100):
        med = float(median(s))
        mean = s.sum() / s.size
        sigma = math.sqrt(((s - mean) ** 2).sum() / s.size)
        nlo, nhi = max(lo, med - 3.0 * sigma), min(hi, med + 3.0 * sigma)
        ns = v[(v >= nlo) & (v <= nhi)]
        if ns.size == s.size:
            break
        lo, hi, s = nlo, nhi, ns
        if it == 99:
            mean = s.sum() / s.size
            sigma = math.sqrt(((s - mean) ** 2).sum() / s.size)
    return sigma


def global_rms(cal):
    H, W = cal.shape
    nx, ny = -(-H // MESH), -(-W // MESH)
    rms = np.full(nx * ny, np.nan)
    good = np.zeros(nx * ny, bool)
    for cy in range(ny):
        for cx in range(nx):
            blk = cal[cx * MESH:(cx + 1) * MESH, cy * MESH:(cy + 1) * MESH]
            nvalid = int((~np.isnan(blk)).sum())
            c = cx + nx * cy
            if nvalid > 0 and 2 * nvalid >= blk.size:
                good[c] = True
                rms[c] = cell_rms(blk)
    if not good.any():
        return float("nan")
    fixed = rms.copy()
    gidx = np.nonzero(good)[0]
    for c in np.nonzero(~good)[0]:
        d = (gidx % nx - c % nx) ** 2 + (gidx // nx - c // nx) ** 2
        fixed[c] = rms[gidx[int(np.argmin(d))]]
    filt = np.empty_like(fixed)
    for c in range(nx * ny):
        cx, cy = c % nx, c // nx
        win = [fixed[x + nx * y] for y in range(cy - 1, cy + 2) for x in range(cx - 1, cx + 2) if 0 <= x < nx and 0 <= y < ny]
        filt[c] = np.median(np.array(win))
    return float(np.float32(np.median(filt)))


def convolve(cal):
    """[1 2 1; 2 4 2; 1 2 1] / 16 in fp64, taps in the device's order (j outer, i inner); NaN and outside = 0"""
    H, W = cal.shape
    pad = np.zeros((H + 2, W + 2))
    pad[1:-1, 1:-1] = np.where(np.isnan(cal), 0.0, cal.astype(np.float64))
    acc = np.zeros((H, W))
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            w = (2 if di == 0 else 1) * (2 if dj == 0 else 1) / 16.0
            acc = acc + w * pad[1 + di:1 + di + H, 1 + dj:1 + dj + W]
    return acc


def seqsum(a):
    a = np.asarray(a, np.float64)
    return float(np.cumsum(a)[-1]) if a.size else 0.0


def _ellipse_coeffs(x2, y2, xy):
    det = x2 * y2 - xy * xy
    if det < 1.0 / 144.0:
        x2 += 1.0 / 12.0
        y2 += 1.0 / 12.0
        det = x2 * y2 - xy * xy
    return y2 / det, x2 / det, -2.0 * xy / det


def _pieces(ii, jj, sel):
    """8-connected pieces of the selected pixels (given by coordinates): a label per selected pixel"""
    i0, j0 = ii[sel].min(), jj[sel].min()
    m = np.zeros((ii[sel].max() - i0 + 1, jj[sel].max() - j0 + 1), bool)
    m[ii[sel] - i0, jj[sel] - j0] = True
    lab, _ = ndimage.label(m, structure=EIGHT)
    return lab[ii[sel] - i0, jj[sel] - j0]


def deblend(ii, jj, c, thr, nthresh=32, cont=0.005, minarea=5, trace=None):
    """multi-threshold deblending of one component; pixels in raster order.  Returns the child index of every pixel
    (children ordered by their smallest raster index).  trace: a list that receives what the scenes' own tests ask about a
    parent that splits: the levels at which a leaf split, each pixel's core (-1: none), its owner among the cores, and the
    Gaussian amplitudes of every pixel outside the cores."""
    n = c.size
    leaf = np.zeros(n, int)
    F = seqsum(c)
    peak = float(c.max())
    next_id = 1
    split_levels = []
    if n >= 2 * minarea:
        for lev in range(1, nthresh):
            t = float(thr) * (peak / float(thr)) ** (lev / nthresh)
            new_leaf = leaf.copy()
            for L in np.unique(leaf[leaf >= 0]):
                sel = (leaf == L) & (c > t)
                if not sel.any():
                    continue
                lab = _pieces(ii, jj, sel)
                idx = np.nonzero(sel)[0]
                sig = []
                for q in np.unique(lab):
                    members = idx[lab == q]
                    if seqsum(c[members]) >= cont * F and members.size >= minarea:
                        sig.append(members)
                if len(sig) >= 2:
                    split_levels.append((lev, int(L)))
                    new_leaf[leaf == L] = -1
                    for members in sorted(sig, key=lambda m: m[0]):
                        new_leaf[members] = next_id
                        next_id += 1
            leaf = new_leaf
    ids = []
    for L in leaf:
        if L >= 0 and L not in ids:
            ids.append(L)
    if len(ids) <= 1:
        return np.zeros(n, int)
    core = np.array([ids.index(L) if L >= 0 else -1 for L in leaf])
    gauss = []
    for k in range(len(ids)):
        m = core == k
        v, x, y = c[m], ii[m].astype(float), jj[m].astype(float)
        f = seqsum(v)
        xm, ym = seqsum(v * x) / f, seqsum(v * y) / f
        dx, dy = x - xm, y - ym
        cxx, cyy, cxy = _ellipse_coeffs(seqsum(v * dx * dx) / f, seqsum(v * dy * dy) / f, seqsum(v * dx * dy) / f)
        gauss.append((xm, ym, cxx, cyy, cxy, float(v.max())))
    owner = core.copy()
    all_amps = {}
    for k in np.nonzero(core < 0)[0]:
        amps = []
        for (xm, ym, cxx, cyy, cxy, pk) in gauss:
            dx, dy = ii[k] - xm, jj[k] - ym
            amps.append(pk * math.exp(-0.5 * (cxx * dx * dx + cyy * dy * dy + cxy * dx * dy)))
        owner[k] = int(np.argmax(amps))
        all_amps[(int(ii[k]), int(jj[k]))] = amps
    if trace is not None:
        trace.append(dict(first=(int(ii[0]), int(jj[0])), split_levels=split_levels, core=core, owner=owner.copy(), amps=all_amps))
    order = []
    for o in owner:
        if o not in order:
            order.append(o)
    return np.array([order.index(o) for o in owner])


def moments(ii, jj, v):
    v = v.astype(np.float64)
    f = v.sum()
    xm, ym = (v * ii).sum() / f, (v * jj).sum() / f
    dx, dy = ii - xm, jj - ym
    x2, y2, xy = (v * dx * dx).sum() / f, (v * dy * dy).sum() / f, (v * dx * dy).sum() / f
    mx2, my2 = x2, y2
    if mx2 * my2 - xy * xy < 1.0 / 144.0:
        mx2 += 1.0 / 12.0
        my2 += 1.0 / 12.0
    tmp = mx2 - my2
    theta = math.atan2(2.0 * xy, tmp) / 2.0 if abs(tmp) > 0 else math.pi / 4.0
    tmp = math.sqrt(0.25 * tmp * tmp + xy * xy)
    pm = 0.5 * (mx2 + my2)
    return dict(x=xm, y=ym, x2=x2, y2=y2, xy=xy, a=math.sqrt(pm + tmp), b=math.sqrt(max(pm - tmp, 0.0)), theta=theta,
                flux=f, peak=float(v.max()))


def extract(pixels, sky, nelec, thresh=1.3, minarea=5, nthresh=32, cont=0.005, thr=None, trace=None):
    """one image; thr (the absolute threshold) overrides the one derived from this restatement's rms; trace: see deblend"""
    cal = calibrate(pixels, sky, nelec)
    H, W = cal.shape
    rms = global_rms(cal)
    if thr is None:
        thr = float(np.float32(np.float32(thresh) * np.float32(rms)))
    conv = convolve(cal)
    mask = ~np.isnan(cal) & (conv > thr)
    lab, nlab = ndimage.label(mask, structure=EIGHT)
    objs = []
    segmap = np.zeros((H, W), np.int32)
    comps = ndimage.find_objects(lab)
    parents = []
    for q in range(1, nlab + 1):
        sl = comps[q - 1]
        sub = lab[sl] == q
        ii, jj = np.nonzero(sub)
        ii, jj = ii + sl[0].start, jj + sl[1].start
        if ii.size < minarea:
            continue
        cm = ii + H * jj
        order = np.argsort(cm, kind="stable")
        parents.append((int(cm[order[0]]), ii[order], jj[order]))
    parents.sort(key=lambda p: p[0])
    for p, (_, ii, jj) in enumerate(parents):
        child = deblend(ii, jj, conv[ii, jj], thr, nthresh, cont, minarea, trace)
        for r in range(child.max() + 1):
            m = child == r
            o = moments(ii[m], jj[m], cal[ii[m], jj[m]])
            o.update(npix=int(m.sum()), xmin=int(ii[m].min()), xmax=int(ii[m].max()), ymin=int(jj[m].min()),
                     ymax=int(jj[m].max()), parent=p, pixels=np.stack([ii[m], jj[m]], axis=1))
            objs.append(o)
            segmap[ii[m], jj[m]] = len(objs)
    return dict(rms=rms, thresh=thr, mask=mask, segmap=segmap, objects=objs, conv=conv)


# ---- detect_sources ----------------------------------------------------------------------------------------------

def detect_sources(images, cats, match_radius):
    """detection.jl:61-171 from per-image restated catalogs (dicts of extract()): (entries, boxes) where entries are
    (world position, star fluxes, gal fluxes, axis ratio, angle, radius) and boxes[i][n] the unclamped box of entry i
    in image n."""
    def world(img, o):
        pix = np.array([o["x"] + 1.0, o["y"] + 1.0])
        return np.linalg.inv(img.wcs_jacobian) @ (pix - img.wcs_pix0) + img.wcs_world0

    def jround(v):
        return int(np.rint(v))

    def around(img, wc, r):
        pc = img.wcs_jacobian @ (wc - img.wcs_world0) + img.wcs_pix0
        return ((jround(pc[0] - r), jround(pc[0] + r)), (jround(pc[1] - r), jround(pc[1] + r)))

    def angle(img):
        cd = np.linalg.inv(img.wcs_jacobian)
        s = np.sign(np.linalg.det(cd))
        return -(math.atan2(s * cd[0, 1], s * cd[0, 0]) + math.pi / 2)

    pos, dets = [], []
    for n, (img, cat) in enumerate(zip(images, cats)):
        w = [world(img, o) for o in cat["objects"]]
        base = np.array(pos) if pos else None
        for j, wj in enumerate(w):
            if n > 0 and base is not None:
                d = np.sqrt(((base - wj) ** 2).sum(axis=1))
                k = int(np.argmin(d))
                if d[k] < match_radius:
                    dets[k].append((n, j))
                    continue
            pos.append(wj)
            dets.append([(n, j)])
    entries, boxes = [], []
    for wc, dl in zip(pos, dets):
        best, npix = [None] * 5, [0] * 5
        for n, j in dl:
            b = images[n].b - 1
            if cats[n]["objects"][j]["npix"] > npix[b]:
                best[b], npix[b] = (n, j), cats[n]["objects"][j]["npix"]
        fl = np.array([cats[bb[0]]["objects"][bb[1]]["flux"] if bb is not None else 0.0 for bb in best])
        n, j = best[int(np.argmax(npix))]
        o = cats[n]["objects"][j]
        entries.append((wc, fl, fl, o["b"] / o["a"], o["theta"] + angle(images[n]), math.sqrt(o["a"] * o["b"]) * math.sqrt(2 * math.log(2))))
        row = []
        found = dict(dl)
        for m, img in enumerate(images):
            mb = around(img, wc, 5.0)
            if m in found:
                o = cats[m]["objects"][found[m]]
                box = ((o["xmin"], o["xmax"]), (o["ymin"], o["ymax"]))
                dil = []
                for r in box:
                    dlt = jround(0.2 * (r[1] - r[0] + 1) / 2)
                    dil.append((r[0] - dlt, r[1] + dlt))
                mb = ((min(dil[0][0], mb[0][0]), max(dil[0][1], mb[0][1])), (min(dil[1][0], mb[1][0]), max(dil[1][1], mb[1][1])))
            row.append(mb)
        boxes.append(row)
    return entries, boxes
