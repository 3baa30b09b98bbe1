"""Node-level inference loops on top of the device optimiser.

  reference (src/ParallelRun.jl)                              here
  ----------------------------------------------------------  -----------------------------------------
  one_node_single_infer  (:546-607) -> process_source (:468)  one_node_single_infer
  one_node_joint_infer   (:135-196): setup_vecs, Cyclades     one_node_joint_infer
  infer_box / _infer_box (:610-672), OptimizedSource, bad_sky  infer_box, OptimizedSource, bad_sky
      batches, num_joint_vi_iters sweeps, process_sources_kernel!
      (:372-397) = sequential maximize! inside a connected component

Single inference: every target starts from generic_init_source and sees its neighbours frozen at
catalog_init_source (DeterministicVI.init_sources, DeterministicVI.jl:94-103).
Joint inference: all targets share one parameter table (setup_vecs: generic_init_source for targets,
catalog_init_source for the rest); inside a Cyclades batch the connected components are independent, and the
sources of one component are optimised one after another.  On the GPU the j-th sources of all components of a
batch form one launch ("layer"): no two of them are neighbours, so optimising them simultaneously is exactly
the reference's schedule.
"""
import logging
from dataclasses import dataclass, replace
from typing import Callable, List, Optional, Sequence

import numpy as np

from .elbo import ElboConfig, FieldContext
from .params import catalog_init_source, generic_init_source, init_source_table  # noqa: F401
from .parallel import sharded_maximize
from .partition import color_classes, partition_cyclades_dynamic

NUM_JOINT_VI_ITERS = 3   # Config.num_joint_vi_iters (src/config.jl:17-25)
log = logging.getLogger("celeste_jl_amd.infer")


def default_infer_config() -> ElboConfig:
    """The optimiser settings of the node-level loops when the caller gives none: ElboConfig's defaults with the
    trust-region multiplier iteration capped at 5 steps, as Optim.jl's solve_tr_subproblem! does (converged or not) --
    the reference's production behaviour (ElboMaximize.jl:228-242 -> Optim.optimize).  ElboConfig() itself keeps
    tr_secular_iters = 0 (run to convergence, <= 20 steps), the setting the optimiser tests pin against a 60-digit
    solution of the sub-problem; the two differ only on boundary steps whose multiplier needs more than 5 Newton steps."""
    return ElboConfig(tr_secular_iters=5)


def _report_failures(targets, status, where: str, failed: Optional[set]):
    """A source whose ELBO turned non-finite is logged and skipped -- the reference's production / multi-thread
    behaviour (Log.exception in process_sources_kernel! and one_node_single_infer, ParallelRun.jl:389-396, 582-597):
    its row stays where it was, every other source of the batch keeps its result."""
    status = np.asarray(status)
    for k in np.flatnonzero(status):
        t = targets[int(k)]
        log.warning("%s: source %d skipped (status %d)", where, int(t), int(status[k]))
        if failed is not None:
            failed.add(int(t))


def one_node_single_infer(ctx: FieldContext, catalog, target_sources: Sequence[int],
                          cfg: Optional[ElboConfig] = None, failed: Optional[set] = None) -> np.ndarray:
    """Returns the optimised parameters, one row per target (OptimizedSource.vs).  Targets that failed are logged,
    keep their initial row and are added to `failed` (the reference drops them from its result list)."""
    vp_nbr = init_source_table(catalog)
    vp = init_source_table(catalog, target_sources)
    cfg = cfg or default_infer_config()
    new, _, _, _, st = ctx.maximize_batch(vp, list(target_sources), cfg, vp_neighbors=vp_nbr, raise_on_error=False)
    _report_failures(target_sources, st, "one_node_single_infer", failed)
    return new[list(target_sources)]


def joint_infer_sweeps(maximize_layer: Callable, vp: np.ndarray, targets: Sequence[int], neighbors: List[List[int]],
                       batch_size: int = 400, n_iters: int = NUM_JOINT_VI_ITERS,
                       rng: Optional[np.random.Generator] = None, rank: int = 0, world: int = 1,
                       costs: Optional[Sequence[float]] = None, all_gather: Optional[Callable] = None,
                       schedule: str = "cyclades", device: Optional[int] = None) -> np.ndarray:
    """The joint-inference schedule, independent of who optimises a layer.

    schedule = "cyclades": the reference's randomly drawn batches, connected components processed source by source
    (ParallelRun.jl:302-397).  schedule = "coloring": the colour classes of a greedy colouring of the neighbour graph,
    one launch per colour and sweep -- the same conflict-freedom with far fewer, larger launches (2.3x faster on
    the 2000-source bench field).  The sweep order differs, as it does between two Cyclades seeds; with most sources in
    the first colour class a sweep is closer to a Jacobi step, so crowded scenes may want more sweeps.

    maximize_layer(vp, layer, pos_centers) -> [len(layer), 44] optimises the sources of `layer` (no two of them are
    neighbours) against the shared table `vp` and returns their new rows.  With world > 1 every rank holds the
    whole table, optimises its cost-balanced shard of each layer and the updated rows are all-gathered (352 B per
    target and layer: SURVEY.md 8(e)) -- the only exchange of the path.  vp is updated in place and returned."""
    targets = list(targets)
    centers = {t: vp[t, 0:2].copy() for t in targets}        # boxes stay at the initial positions
    for layer in joint_layers(targets, neighbors, batch_size, n_iters, rng, schedule):

        def run(local):
            pc = np.stack([centers[t] for t in local])
            return maximize_layer(vp, list(local), pc)
        if world == 1:
            vp[layer] = run(layer)
        else:
            lc = [1.0 if costs is None else costs[t] for t in layer]
            vp[layer] = sharded_maximize(run, layer, lc, rank, world, all_gather, device)
    return vp


def joint_layers(targets: Sequence[int], neighbors: List[List[int]], batch_size: int = 400,
                 n_iters: int = NUM_JOINT_VI_ITERS, rng: Optional[np.random.Generator] = None,
                 schedule: str = "cyclades") -> List[List[int]]:
    """The joint-inference schedule as a flat list of layers (lists of source ids no two of which are neighbours), in the
    order they are optimised: for every sweep, for every batch, the j-th sources of all its connected components
    (j = 0, 1, ...).  This is what celeste_joint_infer consumes."""
    targets = list(targets)
    tset = set(targets)
    nmap = {t: [n for n in neighbors[t] if n in tset] for t in targets}
    if schedule == "coloring":
        batches = [[[i] for i in cls] for cls in color_classes(targets, nmap)]   # one layer per colour
    else:
        assert schedule == "cyclades"
        batches = partition_cyclades_dynamic(targets, nmap, batch_size=batch_size,
                                             rng=rng or np.random.default_rng(42))   # srand(42), ParallelRun.jl:143
    layers = []
    for _ in range(n_iters):
        for components in batches:
            depth = max(len(c) for c in components)
            for j in range(depth):
                layers.append([targets[c[j]] for c in components if len(c) > j])
    return layers


def one_node_joint_infer(ctx: FieldContext, catalog, target_sources: Sequence[int], neighbors: List[List[int]],
                         cfg: Optional[ElboConfig] = None, batch_size: int = 400, n_iters: int = NUM_JOINT_VI_ITERS,
                         rng: Optional[np.random.Generator] = None, rank: int = 0, world: int = 1,
                         costs: Optional[Sequence[float]] = None, all_gather: Optional[Callable] = None,
                         schedule: str = "cyclades", failed: Optional[set] = None) -> np.ndarray:
    """Cyclades-batched joint inference; returns the optimised parameters, one row per target.  rank / world > 1:
    one process per GPU, images replicated (every rank builds the same FieldContext), layers sharded.
    A source that fails in some layer keeps the row it had before that layer (logged, added to `failed`)."""
    targets = list(target_sources)
    vp = init_source_table(catalog, targets)
    cfg = cfg or default_infer_config()
    if world == 1:
        # the whole schedule in one call: the parameter table stays in HBM across all layers (celeste_joint_infer)
        layers = joint_layers(targets, neighbors, batch_size, n_iters, rng, schedule)
        centers = [vp[layer, 0:2].copy() for layer in layers]      # boxes stay at the initial positions
        vp, _, _, _, st = ctx.joint_infer(vp, layers, cfg, pos_centers=centers)
        _report_failures([t for layer in layers for t in layer], st, "one_node_joint_infer", failed)
        return vp[targets]
    if all_gather is None:
        # one process per GPU: every rank optimises its shard of each layer against its own device-resident table and
        # the optimised rows (+ status) are all-gathered on the device after every layer (RCCL; gloo: through the host)
        from .parallel import DeviceJointInfer
        dj = DeviceJointInfer(ctx, vp, rank, world, cfg)
        centers = {t: vp[t, 0:2].copy() for t in targets}
        for layer in joint_layers(targets, neighbors, batch_size, n_iters, rng, schedule):
            lc = [1.0 if costs is None else costs[t] for t in layer]
            st = dj.layer(layer, lc, np.stack([centers[t] for t in layer]))
            _report_failures(layer, st, "one_node_joint_infer", failed)
        return dj.table()[targets]

    def maximize_layer(table, layer, pc):
        new, _, _, _, st = ctx.maximize_batch(table, layer, cfg, pos_centers=pc, raise_on_error=False)
        _report_failures(layer, st, "one_node_joint_infer", failed)
        return new[layer]
    vp = joint_infer_sweeps(maximize_layer, vp, targets, neighbors, batch_size, n_iters, rng, rank, world, costs,
                            all_gather, schedule, device=ctx.device)
    return vp[targets]


# ---- box-level driver (ParallelRun.infer_box, ParallelRun.jl:610-672) ------------------------------------------------

@dataclass
class BoundingBox:
    """src/dataset.jl:1-13"""
    ramin: float
    ramax: float
    decmin: float
    decmax: float

    def __post_init__(self):
        assert self.ramax > self.ramin, "ramax must be greater than ramin"
        assert self.decmax > self.decmin, "decmax must be greater than decmin"

    def contains(self, pos) -> bool:
        return self.ramin < pos[0] < self.ramax and self.decmin < pos[1] < self.decmax


@dataclass
class OptimizedSource:
    """ParallelRun.jl:425-430"""
    init_ra: float
    init_dec: float
    vs: np.ndarray
    is_sky_bad: bool
    failed: bool = False   # the optimiser reported a non-finite ELBO for this source; vs is its last good row
    fit: Optional[object] = None   # infer_box(..., diagnostics=True): this source's fit.FitStats at the final parameters
    light_curve: Optional[object] = None   # infer_box(..., light_curves=True): this source's phot.LightCurves (one target)
    uncertainty: Optional[object] = None   # infer_box(..., uncertainties=True): this source's info.InfoBounds (one target)
    astrometry: Optional[object] = None   # infer_box(..., astrometry=True): this source's astrom.Astrometry (one target)
    refined: Optional[int] = None   # infer_box(..., refine=k): the round of the residual search that added this source; None: it was there from the start


def bad_sky(ce, images) -> bool:
    """ParallelRun.jl:437-460: is the claimed sky of the i-band image 5 photons per pixel below the median of the
    pixels in a 50-pixel box around the object?"""
    from .model import box_around_point, clamp_box, julia_round
    img = next((im for im in images if im.b == 4), None)
    if img is None:
        return False
    pc = img.world_to_pix(ce.pos)
    if img.wcs is not None and not np.isfinite(pc).all():
        return False           # behind the tangent plane: the empty box
    h = max(1, min(julia_round(pc[0]), img.H))
    w = max(1, min(julia_round(pc[1]), img.W))
    claimed_sky = float(img.sky[h - 1, w - 1]) * float(img.nelec_per_nmgy[h - 1])
    (h0, h1), (w0, w1) = clamp_box(box_around_point(img, ce.pos, 50.0), (img.H, img.W))
    px = img.pixels[h0 - 1:h1, w0 - 1:w1]
    px = px[~np.isnan(px)]
    if px.size == 0:
        return False
    # median(px) by selection (what np.median does, without its per-call overhead: 2000 sources took 0.3 s)
    k = px.size // 2
    if px.size % 2:
        med = float(np.partition(px, k)[k])
    else:
        part = np.partition(px, [k - 1, k])
        med = float((part[k - 1] + part[k]) * px.dtype.type(0.5))
    return (claimed_sky + 5) < med


def bad_sky_flags(entries, images, device=None, force_torch: bool = False) -> List[bool]:
    """bad_sky for many catalog entries at once: the 101 x 101 boxes of all sources are gathered and sorted on the GPU
    (torch: device memory and a sort -- plumbing), the median taken from the sorted rows exactly as np.median takes it.
    Used when torch's CUDA runtime is already up in this process (its first use costs ~0.8 s, more than the per-entry
    loop takes for a whole field); otherwise, and for a handful of sources, the per-entry function is used."""
    entries = list(entries)
    img = next((im for im in images if im.b == 4), None)
    if img is None or not entries:
        return [False] * len(entries)
    try:
        import torch
        use = force_torch or (torch.cuda.is_available() and torch.cuda.is_initialized() and len(entries) >= 64)
    except ImportError:       # pragma: no cover
        use = False
    if not use:
        return [bad_sky(ce, images) for ce in entries]
    dev = torch.device("cuda", device or 0) if torch.cuda.is_available() else torch.device("cpu")
    H, W = img.H, img.W
    pos = np.array([ce.pos for ce in entries], dtype=np.float64).reshape(-1, 2)
    pc = img.world_to_pix(pos)                                                           # row by row
    if img.wcs is not None:
        pc = np.where(np.isfinite(pc).all(axis=1)[:, None], pc, -1.0e9)                  # behind the tangent plane: the empty box
    hc = np.clip(np.rint(pc[:, 0]).astype(np.int64), 1, H)
    wc = np.clip(np.rint(pc[:, 1]).astype(np.int64), 1, W)
    claimed = img.sky[hc - 1, wc - 1].astype(np.float64) * np.asarray(img.nelec_per_nmgy)[hc - 1].astype(np.float64)
    # clamp_box(box_around_point(img, pos, 50), (H, W)): inclusive 1-based ranges, possibly empty
    h0 = np.clip(np.rint(pc[:, 0] - 50.0).astype(np.int64), 1, H + 1); h1 = np.clip(np.rint(pc[:, 0] + 50.0).astype(np.int64), 0, H)
    w0 = np.clip(np.rint(pc[:, 1] - 50.0).astype(np.int64), 1, W + 1); w1 = np.clip(np.rint(pc[:, 1] + 50.0).astype(np.int64), 0, W)
    px = torch.from_numpy(np.ascontiguousarray(img.pixels, dtype=np.float32)).to(dev)
    out = np.zeros(len(entries), dtype=bool)
    B = 102                                                                              # a box has at most 102 rows / columns
    off = torch.arange(B, device=dev)
    for lo in range(0, len(entries), 4096):
        sl = slice(lo, min(len(entries), lo + 4096))
        th0 = torch.from_numpy(h0[sl]).to(dev); th1 = torch.from_numpy(h1[sl]).to(dev)
        tw0 = torch.from_numpy(w0[sl]).to(dev); tw1 = torch.from_numpy(w1[sl]).to(dev)
        rows = th0[:, None] + off[None, :]; cols = tw0[:, None] + off[None, :]           # 1-based
        okr = rows <= th1[:, None]; okc = cols <= tw1[:, None]
        vals = px[(rows.clamp(1, H) - 1)[:, :, None], (cols.clamp(1, W) - 1)[:, None, :]]
        vals = torch.where(okr[:, :, None] & okc[:, None, :], vals, torch.full_like(vals, float("nan"))).reshape(vals.shape[0], -1)
        n = (~torch.isnan(vals)).sum(dim=1)
        srt = torch.sort(vals, dim=1).values                                             # NaNs last
        k = torch.div(n, 2, rounding_mode="floor")
        hi = srt.gather(1, k.clamp(max=srt.shape[1] - 1)[:, None])[:, 0]
        lo_ = srt.gather(1, (k - 1).clamp(min=0)[:, None])[:, 0]
        med = torch.where(n % 2 == 1, hi, (lo_ + hi) * 0.5)                              # float32, like np.median
        res = (torch.from_numpy(claimed[sl] + 5.0).to(dev) < med.double()) & (n > 0)
        out[sl] = res.cpu().numpy()
    return [bool(x) for x in out]


def group_single_infer(group, catalog, target_sources: Sequence[int], cfg: Optional[ElboConfig] = None,
                       failed: Optional[set] = None) -> np.ndarray:
    """one_node_single_infer (ParallelRun.jl:546-607) over the devices of a `group.FieldGroup`: the N workers of the
    reference's loop are the group's members (celeste_group_maximize_batch)."""
    vp_nbr = init_source_table(catalog)
    vp = init_source_table(catalog, target_sources)
    new, _, _, _, st = group.maximize_batch(vp, list(target_sources), cfg or default_infer_config(), vp_neighbors=vp_nbr,
                                            raise_on_error=False)
    _report_failures(target_sources, st, "one_node_single_infer", failed)
    return new[list(target_sources)]


def group_joint_infer(group, catalog, target_sources: Sequence[int], neighbors: List[List[int]],
                      cfg: Optional[ElboConfig] = None, batch_size: int = 400, n_iters: int = NUM_JOINT_VI_ITERS,
                      rng: Optional[np.random.Generator] = None, failed: Optional[set] = None) -> np.ndarray:
    """one_node_joint_infer (ParallelRun.jl:135-196) over the devices of a `group.FieldGroup`: the connected components of
    every Cyclades batch are sharded over the members, and rows are exchanged in front of every batch in which a member reads a
    row another member wrote since the last exchange -- at most once per batch, once in all for a group of one
    (celeste_group_joint_infer).  Same table as one_node_joint_infer on one device, bit for bit.
    batch_size is the reference's (Config: 400 sources per Cyclades batch, sized for CPU threads); several devices want batches
    of thousands -- between two exchanges a member's launch ends on its slowest component."""
    from .group import cyclades_schedule
    targets = list(target_sources)
    vp = init_source_table(catalog, targets)
    b_off, c_off, flat = cyclades_schedule(targets, neighbors, batch_size=batch_size, rng=rng)
    pos = vp[flat, 0:2].copy()                                   # boxes stay at the initial positions
    vp, _, _, _, st, _ = group.joint_infer(vp, b_off, c_off, flat, n_iters, cfg or default_infer_config(), pos_centers=pos)
    for sweep in st:
        _report_failures([int(t) for t in flat], sweep, "one_node_joint_infer", failed)
    return vp[targets]


def infer_box(images, box: BoundingBox, catalog=None, method: str = "joint_vi", cfg: Optional[ElboConfig] = None,
              n_iters: int = NUM_JOINT_VI_ITERS, device: int = 0, schedule: str = "cyclades",
              devices: Optional[Sequence[int]] = None, match_radius: float = 1.0 / 3600.0,
              mcmc_config=None, prep: str = "host", diagnostics: bool = False, light_curves: bool = False,
              uncertainties: bool = False, refine: int = 0, refine_threshold: float = 5.0,
              refine_stack: bool = False, astrometry: bool = False, epochs=None) -> list:
    """infer_box / _infer_box (ParallelRun.jl:610-672): targets = catalog entries strictly inside the box, neighbours
    may lie outside it, then joint or single variational inference on the device (method in {joint_vi, single_vi}:
    one OptimizedSource per target) or MCMC (method = "mcmc": process_source_mcmc, ParallelRun.jl:504-543, with
    mcmc_config, an mcmc.MCMCConfig; one mcmc.MCMCResult per target, in target order; one device only).  catalog=None: the catalog and the patches come from source detection on the device
    (detect.detect_sources, detection.jl:39-171), as the reference's infer_box does without a catalog; otherwise
    patches for every catalog entry (get_sky_patches).  match_radius: the world distance under which detections of
    different images are one object (detection.jl's 1 arcsec; used only without a catalog).
    devices: HIP ordinals of a device group (celeste_group_*: one process, the reference's N workers = N devices, RCCL
    inside the library); None = the one `device`.
    prep: "host" builds the patch table, the neighbour lists, the stamps of a variable PSF and the sky flags of a catalog on
    the host (model.patch_table, infer.bad_sky_flags); "device" builds them on the device (prep.patch_table,
    prep.bad_sky_flags: one upload of the planes serves both).  Without a catalog, "host" joins the detections and builds the
    catalog and the patches on the host (detect.detect_sources), "device" on the device (detect.detect_table: the patch table,
    the neighbour lists and the sky flags from one upload of the planes).
    diagnostics: after variational inference every result also carries `fit`, the goodness of fit of its source
    (fit.FitStats: chi-square, residual flux, purity, flux misfit per band; include/celeste_fit.h) at the final table --
    the targets at their optimised rows, every other source at catalog_init_source -- computed on the first device.  Not
    available with method="mcmc" (there is no parameter table to evaluate).  The default loads nothing and changes nothing.
    light_curves: after variational inference every result also carries `light_curve`, the per-exposure forced photometry of
    its source (phot.LightCurves of one target: per image the scale of its light, its error, a flag; per band the weighted mean
    and the variability chi-square; include/celeste_phot.h) at the same table.  Not available with method="mcmc".  The default
    loads nothing and changes nothing.
    uncertainties: after variational inference every result also carries `uncertainty`, the Cramer-Rao bounds of its source's
    position and shape from the pixels' Fisher information (info.InfoBounds of one target: per type the sums, the covariance
    and its flags; include/celeste_info.h) at the same table.  Not available with method="mcmc".  The default loads nothing
    and changes nothing.
    refine: after variational inference, up to `refine` rounds of: search the frames' residuals at the final table for sources the
    catalog missed (resid.ResidContext.search with threshold refine_threshold, resid.missed_sources; include/celeste_resid.h),
    append those strictly inside the box to the catalog as stars, and run the catalog path again over the extended catalog with
    targets = the old targets followed by the new ones; it stops early when a round adds nothing.  Every result carries
    `refined`: the round that added its source, None for the others.  On the first device of a device group.  Not available
    with method="mcmc".  The default loads nothing and changes nothing.
    refine_stack: each refinement round also adds the search's maps across images on a sky grid that covers the searched frames
    within the box (resid.grid_covering, ResidualSearch.stack at refine_threshold with flat weights) and takes the stacked
    peaks that are neither catalog sources nor what the round's single-image search already found (resid.stacked_sources):
    the sources too faint for every single image.  Needs refine >= 1.  The default loads nothing and changes nothing.
    astrometry: after variational inference every result also carries `astrometry`, the per-exposure offsets of its source
    (astrom.Astrometry of one target: per image the offset and scale of its light, their covariance, a flag; per target the
    weighted mean offset and a linear motion over `epochs`, one time per image, None: the image index;
    include/celeste_astrom.h) at the final table, on the first device.  Not available with method="mcmc".  The default loads
    nothing and changes nothing."""
    if refine_stack and not refine:
        raise ValueError("refine_stack=True needs refine >= 1: the stack is a step of a refinement round")
    if astrometry and method == "mcmc":
        raise ValueError("astrometry=True needs a parameter table: method='mcmc' returns samples, not parameters")
    if refine and method == "mcmc":
        raise ValueError("refine needs a parameter table: method='mcmc' returns samples, not parameters")
    state: Optional[dict] = {} if (refine or astrometry) else None
    results = _infer_box_round(images, box, catalog, method, cfg, n_iters, device, schedule, devices, match_radius, mcmc_config,
                               prep, diagnostics, light_curves, uncertainties, state)
    if refine:
        results = _refine(images, box, results, state, int(refine), float(refine_threshold), method, cfg, n_iters, device, schedule,
                          devices, mcmc_config, prep, diagnostics, light_curves, uncertainties, bool(refine_stack))
    if astrometry:
        results = _with_astrometry(results, state, epochs)
    return results


def _refine(images, box, results, state, rounds, threshold, method, cfg, n_iters, device, schedule, devices, mcmc_config, prep,
            diagnostics, light_curves, uncertainties, stack=False) -> list:
    """infer_box(..., refine=rounds): the loop of residual search and renewed inference.  state: what the first inference left
    (_with_fit: problem, catalog, targets, device); empty when the box held no target."""
    if not results or not state:
        return results
    from . import resid
    final = state                      # the caller's dict: receives what the last round saw
    catalog, targets, problem, dev = list(state["catalog"]), list(state["targets"]), state["problem"], state["device"]
    added = {}
    for k in range(1, rounds + 1):
        vp = init_source_table(catalog)
        vp[targets] = np.stack([r.vs for r in results])
        with resid.ResidContext(problem, dev) as rc:
            search = rc.search(vp, threshold=threshold)
            _, entries = resid.missed_sources(search, images, catalog)
            if stack and search.images:
                # (the stack sees what the single-image search saw too: those count as catalog sources here, so a source is added once)
                stacked = search.stack(resid.grid_covering(images, search.images, box), threshold=threshold)
                entries = entries + resid.stacked_sources(stacked, search, images, list(catalog) + entries)[1]
        new = [ce for ce in entries if box.contains(ce.pos)]
        if not new:
            break
        for i in range(len(new)):
            added[len(catalog) + i] = k
        targets = targets + list(range(len(catalog), len(catalog) + len(new)))
        # (a detection's entry has flux 0 in a band without a detection, which the catalog path's patch radius refuses
        # (imaged_sources.jl:205): such bands get the floor the new entries get; a given catalog has none)
        catalog = [ce if (np.asarray(ce.star_fluxes) > 0).all() and (np.asarray(ce.gal_fluxes) > 0).all() else
                   replace(ce, star_fluxes=np.maximum(ce.star_fluxes, resid.DEFAULT_FLUX_FLOOR_NMGY),
                           gal_fluxes=np.maximum(ce.gal_fluxes, resid.DEFAULT_FLUX_FLOOR_NMGY)) for ce in catalog] + new
        state = {}
        results = _infer_box_round(images, box, catalog, method, cfg, n_iters, device, schedule, devices, 0.0, mcmc_config, prep,
                                   diagnostics, light_curves, uncertainties, state, targets=targets)
        problem = state["problem"]
    for r, t in zip(results, targets):
        r.refined = added.get(t)
    final.update(problem=problem, catalog=catalog, targets=list(targets), device=dev)
    return results


def _infer_box_round(images, box, catalog, method, cfg, n_iters, device, schedule, devices, match_radius, mcmc_config, prep,
                     diagnostics, light_curves, uncertainties, state, targets=None) -> list:
    """one inference over a box (infer_box without its refinement).  state (a dict or None) receives what _with_fit saw;
    targets: the target list of the catalog path when it is not "every entry inside the box" (a refinement round)"""
    if prep not in ("host", "device"):
        raise ValueError("prep must be 'host' or 'device', not %r" % (prep,))
    if diagnostics and method == "mcmc":
        raise ValueError("diagnostics=True needs a parameter table: method='mcmc' returns samples, not parameters")
    if light_curves and method == "mcmc":
        raise ValueError("light_curves=True needs a parameter table: method='mcmc' returns samples, not parameters")
    if uncertainties and method == "mcmc":
        raise ValueError("uncertainties=True needs a parameter table: method='mcmc' returns samples, not parameters")
    if method == "mcmc" and devices is not None:
        raise ValueError("method='mcmc' runs on one device: pass device=..., not devices=... (device groups run VI only)")
    if catalog is None:
        if prep == "device":
            return _infer_box_detected_table(images, box, method, cfg, n_iters, device, schedule, devices, match_radius, mcmc_config,
                                             diagnostics, light_curves, uncertainties, state)
        return _infer_box_detected(images, box, method, cfg, n_iters, device, schedule, devices, match_radius, mcmc_config,
                                   diagnostics, light_curves, uncertainties, state)
    if targets is None:
        targets = [i for i, ce in enumerate(catalog) if box.contains(ce.pos)]
    if not targets:
        return []
    if prep == "device":
        from .prep import PrepImages
        with PrepImages(images, devices[0] if devices is not None else device) as pi:
            return _infer_box_catalog(images, catalog, targets, method, cfg, n_iters, device, schedule, devices, mcmc_config, pi,
                                      diagnostics, light_curves, uncertainties, state)
    return _infer_box_catalog(images, catalog, targets, method, cfg, n_iters, device, schedule, devices, mcmc_config, None,
                              diagnostics, light_curves, uncertainties, state)


def _with_astrometry(results: list, state: dict, epochs) -> list:
    """infer_box(..., astrometry=True): every result gets the per-exposure offsets of its source (astrom.AstromContext.offsets)
    at the table that holds the targets' optimised rows and catalog_init_source for every other source.  state: what _with_fit
    (or the last refinement round) saw; empty when the box held no target."""
    if not results or not state:
        return results
    from .astrom import AstromContext
    catalog, targets = state["catalog"], list(state["targets"])
    vp = init_source_table(catalog)
    vp[targets] = np.stack([r.vs for r in results])
    with AstromContext(state["problem"], state["device"]) as ac:
        am = ac.offsets(vp, targets, epochs=epochs)
    for k, r in enumerate(results):
        r.astrometry = am[k]
    return results


def _with_fit(results: list, diagnostics: bool, problem, catalog, targets, device: int, light_curves: bool = False,
              uncertainties: bool = False, state: Optional[dict] = None) -> list:
    """infer_box(..., diagnostics=True): every result gets the fit statistics of its source (fit.FitContext.stats) at the
    table that holds the targets' optimised rows and catalog_init_source for every other source; light_curves=True: its
    per-exposure photometry (phot.PhotContext.light_curves) at the same table; uncertainties=True: the bounds of its position
    and shape (info.InfoContext.bounds) at the same table.  state (infer_box(..., refine=k)): receives the problem, the catalog,
    the targets and the device"""
    if state is not None:
        state.update(problem=problem, catalog=catalog, targets=list(targets), device=device)
    if not (diagnostics or light_curves or uncertainties) or not results:
        return results
    vp = init_source_table(catalog)
    vp[list(targets)] = np.stack([r.vs for r in results])
    if diagnostics:
        from .fit import FitContext
        with FitContext(problem, device) as fc:
            st = fc.stats(vp, list(targets))
        for k, r in enumerate(results):
            r.fit = st[k]
    if light_curves:
        from .phot import PhotContext
        with PhotContext(problem, device) as pc:
            lc = pc.light_curves(vp, list(targets))
        for k, r in enumerate(results):
            r.light_curve = lc[k]
    if uncertainties:
        from .info import InfoContext
        with InfoContext(problem, device) as ic:
            ub = ic.bounds(vp, list(targets))
        for k, r in enumerate(results):
            r.uncertainty = ub[k]
    return results


def _infer_box_catalog(images, catalog, targets, method, cfg, n_iters, device, schedule, devices, mcmc_config, pi,
                       diagnostics: bool = False, light_curves: bool = False,
                       uncertainties: bool = False, state: Optional[dict] = None) -> list:
    """infer_box with a catalog.  pi: a prep.PrepImages over `images` (the table, neighbour lists, stamps and sky flags come
    from the device) or None (from the host)."""
    def sky_flags(dev):
        if pi is not None:
            from . import prep
            return prep.bad_sky_flags([catalog[t] for t in targets], images, prep_images=pi)
        return bad_sky_flags([catalog[t] for t in targets], images, dev)
    if method == "mcmc":
        # the MCMC library's own context over the problem of FieldContext.from_catalog (no VI context is created)
        from . import cabi, model
        from .mcmc import MCMCContext, run_ais_batch
        table = model.table_for(images, catalog, len(images) > 5, prep_images=pi)
        mc = MCMCContext(cabi.problem_from_table(images, table, table.neighbors()), device)
        try:
            return run_ais_batch(mc, catalog, targets, mcmc_config)
        finally:
            mc.close()
    if devices is not None:
        from .group import FieldGroup
        if schedule != "cyclades":
            raise ValueError("a device group runs the reference's Cyclades schedule")
        group = FieldGroup.from_catalog(images, catalog, devices=list(devices), sparse=len(images) > 5, prep_images=pi)
        failed = set()
        try:
            if method == "joint_vi":
                vs = group_joint_infer(group, catalog, targets, group.problem.neighbors, cfg, n_iters=n_iters, failed=failed)
            elif method == "single_vi":
                vs = group_single_infer(group, catalog, targets, cfg, failed=failed)
            else:
                raise ValueError("unknown method: %s" % method)
        finally:
            group.close()
        flags = sky_flags(devices[0])
        return _with_fit([OptimizedSource(float(catalog[t].pos[0]), float(catalog[t].pos[1]), vs[k].copy(), flags[k], t in failed)
                          for k, t in enumerate(targets)], diagnostics, group.problem, catalog, targets, devices[0], light_curves,
                          uncertainties, state)
    # patches and neighbour lists as arrays (model.patch_table: the geometry of get_sky_patches / find_neighbors
    # without a Python object per patch); several fields: sources see a few images each -> sparse patch list
    ctx = FieldContext.from_catalog(images, catalog, device=device, sparse=len(images) > 5, prep_images=pi)
    neighbors = ctx.problem.neighbors
    failed: set = set()
    try:
        if method == "joint_vi":
            vs = one_node_joint_infer(ctx, catalog, targets, neighbors, cfg, n_iters=n_iters, schedule=schedule,
                                      failed=failed)
        elif method == "single_vi":
            vs = one_node_single_infer(ctx, catalog, targets, cfg, failed=failed)
        else:
            raise ValueError("unknown method: %s" % method)
    finally:
        ctx.close()
    flags = sky_flags(device)
    return _with_fit([OptimizedSource(float(catalog[t].pos[0]), float(catalog[t].pos[1]), vs[k].copy(), flags[k], t in failed)
                      for k, t in enumerate(targets)], diagnostics, ctx.problem, catalog, targets, device, light_curves,
                      uncertainties, state)


def _infer_box_detected(images, box: BoundingBox, method, cfg, n_iters, device, schedule, devices,
                        match_radius, mcmc_config=None, diagnostics: bool = False, light_curves: bool = False,
                        uncertainties: bool = False, state: Optional[dict] = None) -> list:
    """_infer_box with the catalog and patches of detect_sources (ParallelRun.jl:661-665): targets strictly inside the
    box, neighbours from the detection patches, the context (or device group) over those patches."""
    from .detect import detect_sources
    from .model import neighbor_map
    catalog, patches = detect_sources(images, device=devices[0] if devices is not None else device,
                                      match_radius=match_radius)
    targets = [i for i, ce in enumerate(catalog) if box.contains(ce.pos)]
    if not targets:
        return []
    neighbors = neighbor_map(patches)
    failed: set = set()
    if method == "mcmc":
        from . import cabi
        from .mcmc import MCMCContext, run_ais_batch
        mc = MCMCContext(cabi.Problem(images, patches, neighbors), device)
        try:
            return run_ais_batch(mc, catalog, targets, mcmc_config)
        finally:
            mc.close()
    if devices is not None:
        from .group import FieldGroup
        if schedule != "cyclades":
            raise ValueError("a device group runs the reference's Cyclades schedule")
        group = FieldGroup(images, patches, neighbors, devices=list(devices))
        problem = group.problem
        try:
            if method == "joint_vi":
                vs = group_joint_infer(group, catalog, targets, neighbors, cfg, n_iters=n_iters, failed=failed)
            elif method == "single_vi":
                vs = group_single_infer(group, catalog, targets, cfg, failed=failed)
            else:
                raise ValueError("unknown method: %s" % method)
        finally:
            group.close()
        flag_device = devices[0]
    else:
        ctx = FieldContext(images, patches, neighbors, device=device)
        problem = ctx.problem
        try:
            if method == "joint_vi":
                vs = one_node_joint_infer(ctx, catalog, targets, neighbors, cfg, n_iters=n_iters, schedule=schedule,
                                          failed=failed)
            elif method == "single_vi":
                vs = one_node_single_infer(ctx, catalog, targets, cfg, failed=failed)
            else:
                raise ValueError("unknown method: %s" % method)
        finally:
            ctx.close()
        flag_device = device
    flags = bad_sky_flags([catalog[t] for t in targets], images, flag_device)
    return _with_fit([OptimizedSource(float(catalog[t].pos[0]), float(catalog[t].pos[1]), vs[k].copy(), flags[k], t in failed)
                      for k, t in enumerate(targets)], diagnostics, problem, catalog, targets, flag_device, light_curves,
                      uncertainties, state)


def _infer_box_detected_table(images, box: BoundingBox, method, cfg, n_iters, device, schedule, devices,
                              match_radius, mcmc_config=None, diagnostics: bool = False, light_curves: bool = False,
                              uncertainties: bool = False, state: Optional[dict] = None) -> list:
    """_infer_box_detected with the join, the catalog, the patch table, the neighbour lists and the sky flags from the device
    (detect.detect_table, prep.bad_sky_flags over one prep.PrepImages); the problem is cabi.problem_from_table's."""
    from . import cabi, prep
    from .detect import detect_table
    if method not in ("joint_vi", "single_vi", "mcmc"):
        raise ValueError("unknown method: %s" % method)
    if devices is not None and schedule != "cyclades":
        raise ValueError("a device group runs the reference's Cyclades schedule")
    first = devices[0] if devices is not None else device
    with prep.PrepImages(images, first) as pi:
        catalog, table = detect_table(images, device=first, match_radius=match_radius, prep_images=pi)
        targets = [i for i, ce in enumerate(catalog) if box.contains(ce.pos)]
        if not targets:
            return []
        neighbors = table.neighbors()
        problem = cabi.problem_from_table(images, table, neighbors)
        failed: set = set()
        if method == "mcmc":
            from .mcmc import MCMCContext, run_ais_batch
            mc = MCMCContext(problem, device)
            try:
                return run_ais_batch(mc, catalog, targets, mcmc_config)
            finally:
                mc.close()
        if devices is not None:
            from .group import FieldGroup
            group = FieldGroup(images, None, neighbors, devices=list(devices), problem=problem)
            try:
                if method == "joint_vi":
                    vs = group_joint_infer(group, catalog, targets, neighbors, cfg, n_iters=n_iters, failed=failed)
                else:
                    vs = group_single_infer(group, catalog, targets, cfg, failed=failed)
            finally:
                group.close()
        else:
            ctx = FieldContext(images, None, neighbors, device=device, problem=problem)
            try:
                if method == "joint_vi":
                    vs = one_node_joint_infer(ctx, catalog, targets, neighbors, cfg, n_iters=n_iters, schedule=schedule,
                                              failed=failed)
                else:
                    vs = one_node_single_infer(ctx, catalog, targets, cfg, failed=failed)
            finally:
                ctx.close()
        flags = prep.bad_sky_flags([catalog[t] for t in targets], images, prep_images=pi)
    return _with_fit([OptimizedSource(float(catalog[t].pos[0]), float(catalog[t].pos[1]), vs[k].copy(), flags[k], t in failed)
                      for k, t in enumerate(targets)], diagnostics, problem, catalog, targets, first, light_curves,
                      uncertainties, state)
