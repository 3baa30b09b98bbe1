"""Input preparation of a box on the device (celeste_jl_amd.prep) beside the host functions it replaces, in one process on
the same inputs: the median of 5 calls after a warm-up, on
  * the bench field: 2048 x 1489 x 5, 2000 prior-drawn sources (the catalog make_field draws for seed 1), with the constant
    PSF template and with `variable_images` (an SDSSPSFMap stamp per patch), pixels generated on the device;
  * config 5: 80 images of 2048 x 1489 on the 4 x 4 grid with 30 000 sources (the catalog make_multifield draws for seed 5),
    sparse tables, blank pixels (the host functions once: they take seconds there).
Per scene: the upload of the planes (PrepImages), device milliseconds per stage (HIP events: celeste_prep_last_ms) and wall
time of prep.patch_table and prep.bad_sky_flags with a reused PrepImages and with one of their own, and the wall time of
model.patch_table, PatchTable.neighbors, the per-entry infer.bad_sky loop and infer.bad_sky_flags (torch).  On the bench
field also FieldContext.from_catalog plus the sky flags as infer_box runs them, host path against device path (upload
included), and infer_box end to end with prep="host" and prep="device".
The prep library uploads its own copy of the planes (celeste_ctx_create uploads its own as before): `upload_s` is that cost.
Writes profiles/prep_time_mi355x.json (and prints it).  --small: a 256 x 256 x 5 field only (a rehearsal of the script).
--wcs tan: only the bench field's geometry (dense table, constant PSF, blank pixels) with the affine WCS and, in the same run,
with a tangent-plane WCS at dec 60 turned by 30 degrees (model.TanWCS; the same pixel positions): device milliseconds per stage,
the medians of 21 calls each, taken in turn; the result is added to the JSON file under "wcs_tan" (the rest of the file stays)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import celeste_jl_amd as cel  # noqa: E402
from celeste_jl_amd import infer, model, prep, synthetic  # noqa: E402

REPS = 5


def catalog_of(H, W, n_sources, seed, margin):
    """the catalog make_field / make_multifield draw for this seed (positions uniform in [margin, extent - margin])"""
    rng = np.random.Generator(np.random.PCG64(seed))
    prior = synthetic.load_prior()
    out = []
    for _ in range(n_sources):
        pos = (rng.uniform(margin, H - margin), rng.uniform(margin, W - margin))
        out.append(synthetic.draw_source(prior, rng, pos))
    return out


def grid_images(grid, H, W, overlap=0.10):
    images = []
    step_h, step_w = int(round(H * (1 - overlap))), int(round(W * (1 - overlap)))
    for gi in range(grid[0]):
        for gj in range(grid[1]):
            for im in synthetic.blank_images(H, W):
                im.wcs_world0 = np.array([float(gi * step_h), float(gj * step_w)])
                images.append(im)
    return images, step_h * (grid[0] - 1) + H, step_w * (grid[1] - 1) + W


def sync():
    import torch
    torch.cuda.synchronize()


def timed(fn, reps=REPS, warm=1):
    """(median wall seconds, last result) of fn(), every call ending in a device synchronise"""
    out = None
    for _ in range(warm):
        out = fn()
        sync()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        sync()
        walls.append(time.perf_counter() - t0)
    return float(np.median(walls)), out


def time_scene(name, images, catalog, sparse, host_reps=REPS, contexts=True, infer_reps=3):
    print("%s: %d images, %d sources" % (name, len(images), len(catalog)), flush=True)
    out = dict(n_images=len(images), n_sources=len(catalog), sparse=bool(sparse),
               plane_bytes=int(sum(im.pixels.nbytes for im in images)))
    warm = 1 if host_reps > 1 else 0
    # ---- the device path
    def upload():
        prep.PrepImages(images, 0).close()
    out["upload_s"], _ = timed(upload)
    with prep.PrepImages(images, 0) as pi:
        stages = []

        def table_reused():
            t = prep.patch_table(images, catalog, sparse=sparse, prep_images=pi)
            stages.append(prep.last_ms())
            return t
        out["patch_table_reused_s"], table = timed(table_reused)
        med = {k: float(np.median([s[k] for s in stages[1:]])) for k in prep.STAGES if k != "sky"}
        out["patch_table_device_ms"] = med
        out["entries"], out["neighbor_links"] = int(len(table.source)), int(sum(len(r) for r in table.neighbor_lists))
        out["stamps"] = int(table.stamps.shape[0]) if hasattr(table, "stamps") else 0
        sky_ms = []

        def sky_reused():
            f = prep.bad_sky_flags(catalog, images, prep_images=pi)
            sky_ms.append(prep.last_ms()["sky"])
            return f
        out["bad_sky_flags_reused_s"], flags = timed(sky_reused)
        out["bad_sky_device_ms"] = float(np.median(sky_ms[1:]))
        del table
    out["patch_table_own_upload_s"], table = timed(lambda: prep.patch_table(images, catalog, sparse=sparse, device=0))
    out["bad_sky_flags_own_upload_s"], _ = timed(lambda: prep.bad_sky_flags(catalog, images, device=0))
    # ---- the host functions, same process, same inputs
    out["host_patch_table_s"], htable = timed(lambda: model.patch_table(images, catalog, sparse=sparse), host_reps, warm)
    out["host_neighbors_s"], hnb = timed(htable.neighbors, host_reps, warm)
    out["host_bad_sky_loop_s"], hflags = timed(lambda: [infer.bad_sky(ce, images) for ce in catalog], host_reps, warm)
    out["host_bad_sky_flags_torch_s"], tflags = timed(lambda: infer.bad_sky_flags(catalog, images, 0), host_reps, warm)
    same = (np.array_equal(table.box, htable.box) and np.array_equal(table.source, htable.source) and
            np.array_equal(table.image, htable.image) and np.array_equal(table.active_pixels, htable.active_pixels) and
            table.neighbor_lists == hnb and flags == hflags)
    out["device_results_equal_host"] = bool(same)
    out["host_over_device"] = dict(
        patch_table_and_neighbors=(out["host_patch_table_s"] + out["host_neighbors_s"]) / out["patch_table_reused_s"],
        bad_sky=min(out["host_bad_sky_loop_s"], out["host_bad_sky_flags_torch_s"]) / out["bad_sky_flags_reused_s"])
    del table, htable
    if contexts:
        # ---- from_catalog plus the sky flags, as infer_box runs them (the host path's flags: infer.bad_sky_flags)
        def host_path():
            ctx = cel.FieldContext.from_catalog(images, catalog, sparse=sparse)
            ctx.close()
            return infer.bad_sky_flags(catalog, images, 0)

        def device_path():
            with prep.PrepImages(images, 0) as p2:
                ctx = cel.FieldContext.from_catalog(images, catalog, sparse=sparse, prep_images=p2)
                ctx.close()
                return prep.bad_sky_flags(catalog, images, prep_images=p2)
        out["from_catalog_plus_sky_host_s"], a = timed(host_path, host_reps, warm)
        out["from_catalog_plus_sky_device_s"], b = timed(device_path)
        out["from_catalog_plus_sky_host_over_device"] = out["from_catalog_plus_sky_host_s"] / out["from_catalog_plus_sky_device_s"]
        assert a == b
        # ---- infer_box end to end
        box = cel.BoundingBox(-1e9, 1e9, -1e9, 1e9)
        res = {}
        for mode in ("host", "device"):
            out["infer_box_joint_vi_prep_%s_s" % mode], res[mode] = timed(
                lambda: cel.infer_box(images, box, catalog, method="joint_vi", prep=mode), infer_reps)
        out["infer_box_host_over_device"] = out["infer_box_joint_vi_prep_host_s"] / out["infer_box_joint_vi_prep_device_s"]
        out["infer_box_flags_equal"] = [r.is_sky_bad for r in res["host"]] == [r.is_sky_bad for r in res["device"]]
        # (an eigen-PSF: the device's stamps differ from numpy's in the last bits, which the optimiser's iterations amplify)
        out["infer_box_vs_max_abs_difference"] = float(max(np.abs(x.vs - y.vs).max() for x, y in zip(res["host"], res["device"])))
    print(json.dumps({name: out}, indent=1), flush=True)
    return out


def bench_field(H, W, n, variable):
    catalog = catalog_of(H, W, n, 1, 26)
    images = synthetic.variable_images(H, W, 1) if variable else synthetic.blank_images(H, W)
    synthetic.gen_images(images, catalog, np.random.Generator(np.random.PCG64(1)), seed=1, device=0)
    return images, catalog


def time_wcs(H, W, n, reps=21):
    """device milliseconds per stage of prep.patch_table on the same pixel positions under an affine and a TAN WCS"""
    import math
    affine_cat = catalog_of(H, W, n, 1, 26)
    t = math.radians(30.0)
    scale = 0.396 / 3600.0
    wcs = model.TanWCS((359.9995, 60.0), ((H + 1) / 2.0, (W + 1) / 2.0),
                       scale * np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]]))
    tan_cat = []
    for ce in affine_cat:
        tan_cat.append(synthetic.CatalogEntry(wcs.pix_to_world(ce.pos), ce.is_star, ce.star_fluxes, ce.gal_fluxes, ce.gal_frac_dev,
                                              ce.gal_axis_ratio, ce.gal_angle, ce.gal_radius_px))
    scenes = {"affine": (synthetic.blank_images(H, W), affine_cat),
              "tan": ([model.with_tan_wcs(im, wcs) for im in synthetic.blank_images(H, W)], tan_cat)}
    handles = {k: prep.PrepImages(v[0], 0) for k, v in scenes.items()}
    ms = {k: [] for k in scenes}
    tables = {}
    try:
        for r in range(reps + 1):
            for k, (images, catalog) in scenes.items():
                tables[k] = prep.patch_table(images, catalog, prep_images=handles[k])
                sync()
                if r:
                    ms[k].append(prep.last_ms())
    finally:
        for h in handles.values():
            h.close()
    out = {"n_images": 5, "n_sources": n, "reps": reps, "entries": int(len(tables["tan"].source))}
    for k in scenes:
        out[k] = {"device_ms": {s: float(np.median([m[s] for m in ms[k]])) for s in prep.STAGES if s != "sky"},
                  "geometry_ms_min_max": [float(min(m["geometry"] for m in ms[k])), float(max(m["geometry"] for m in ms[k]))]}
    out["tan_over_affine_geometry"] = out["tan"]["device_ms"]["geometry"] / out["affine"]["device_ms"]["geometry"]
    out["boxes_equal"] = bool(np.array_equal(tables["affine"].box, tables["tan"].box))   # (may differ at a rounding tie)
    return out


def main():
    import torch
    assert torch.cuda.is_available(), "this tool measures on the device"
    out = {"reps": REPS, "device": torch.cuda.get_device_name(0)}
    if "--wcs" in sys.argv:
        if sys.argv[sys.argv.index("--wcs") + 1:][:1] != ["tan"]:
            raise SystemExit("--wcs tan")
        small = "--small" in sys.argv
        res = time_wcs(256, 256, 60) if small else time_wcs(2048, 1489, 2000)
        print(json.dumps({"wcs_tan": res}, indent=1))
        if not small:
            path = os.path.join(ROOT, "profiles", "prep_time_mi355x.json")
            with open(path) as f:
                doc = json.load(f)
            doc["wcs_tan"] = res
            with open(path, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
            print("wrote", path)
        return
    if "--small" in sys.argv:
        for variable in (False, True):
            images, catalog = bench_field(256, 256, 60, variable)
            out["small_256x256x5_60_sources_%s_psf" % ("variable" if variable else "constant")] = time_scene(
                "small", images, catalog, False, infer_reps=1)
        print(json.dumps(out, indent=1))
        return
    for variable in (False, True):
        images, catalog = bench_field(2048, 1489, 2000, variable)
        out["bench_field_2048x1489x5_2000_sources_%s_psf" % ("variable" if variable else "constant")] = time_scene(
            "bench field, %s PSF" % ("variable" if variable else "constant"), images, catalog, False)
        del images
    if "--no-config5" not in sys.argv:
        images, th, tw = grid_images((4, 4), 2048, 1489)
        out["config5_grid_4x4_80_images_2048x1489_30000_sources"] = time_scene(
            "config 5", images, catalog_of(th, tw, 30000, 5, 8), True, host_reps=1, contexts=False)
    path = os.path.join(ROOT, "profiles", "prep_time_mi355x.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
