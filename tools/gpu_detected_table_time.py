"""The detection path of input preparation on the device (prep.detected_table: join, catalog entries, boxes, patch table)
beside the host functions it replaces, in one process on the same inputs: the median of 5 calls after a warm-up, on
  * the bench field: 2048 x 1489 x 5, pixels generated on the device from the 2000 prior-drawn sources make_field draws for
    seed 1, with the constant PSF template and with `variable_images`; the per-image catalogs are detect.extract's;
  * an 80-image field: the 4 x 4 grid of config 5 with blank pixels and synthetic per-image catalogs (every one of 30 000
    drawn sources is detected, a little off, in every image that holds it); the host functions run once there.
match_radius is 2.5 (the synthetic WCS counts pixels).  Per scene: device milliseconds per stage (HIP events inside the
library: celeste_prep_detected_last_ms), the wall time of prep.detected_table with a reused PrepImages and with its own
upload and of cabi.problem_from_table, and the wall time of detect.match_detections, detect.build_detection_output,
model.neighbor_map and cabi.Problem.  On the bench field also infer_box(images, box) end to end with prep="host" and
prep="device".  Every timed call ends in a device synchronise.
Writes profiles/detected_table_time_mi355x.json after every scene (and prints it).  --small: a 256 x 256 x 5 field and a
2 x 2 grid of 128 x 128 images (a rehearsal of the script); --no-80: without the 80-image field."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
import celeste_jl_amd as cel  # noqa: E402
from celeste_jl_amd import cabi, detect, model, prep  # noqa: E402
from gpu_prep_time import REPS, bench_field, catalog_of, grid_images, timed  # noqa: E402

RADIUS = 2.5


def synthetic_catalogs(images, catalog, seed):
    """one detect.Catalog per image: every source of `catalog` that lies 3 pixels inside the image, shifted by N(0, 0.1)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pos = np.array([ce.pos for ce in catalog]).reshape(-1, 2)
    out = []
    for im in images:
        p = pos - im.wcs_world0 + im.wcs_pix0
        p = p[(p[:, 0] > 3) & (p[:, 0] < im.H - 3) & (p[:, 1] > 3) & (p[:, 1] < im.W - 3)]
        p = p + rng.normal(0.0, 0.1, p.shape)
        n = len(p)
        hw = rng.integers(1, 9, (n, 2))
        z = np.zeros(n)
        a = rng.uniform(1.0, 4.0, n)
        out.append(detect.Catalog(rms=1.0, thresh=1.3, npix=rng.integers(5, 200, n), xmin=p[:, 0].astype(np.int64) - hw[:, 0],
                                  xmax=p[:, 0].astype(np.int64) + hw[:, 0], ymin=p[:, 1].astype(np.int64) - hw[:, 1],
                                  ymax=p[:, 1].astype(np.int64) + hw[:, 1], x=p[:, 0], y=p[:, 1], x2=z, y2=z, xy=z, a=a,
                                  b=a * rng.uniform(0.3, 1.0, n), theta=rng.uniform(-1.5, 1.5, n), flux=rng.uniform(1.0, 500.0, n),
                                  peak=z, parent=np.full(n, -1)))
    return out


def same_as_host(images, catalog, table, hcatalog, patches, hneighbors):
    ent = []
    for s, row in enumerate(patches):
        ent += [(s, n, p) for n, p in row.nonempty()] if isinstance(row, model.PatchRow) else [(s, n, row[n]) for n in range(len(images))]
    return bool(len(catalog) == len(hcatalog) and
                all(a.pos.tobytes() == b.pos.tobytes() and a.gal_fluxes.tobytes() == b.gal_fluxes.tobytes() and
                    (a.gal_axis_ratio, a.gal_angle, a.gal_radius_px) == (b.gal_axis_ratio, b.gal_angle, b.gal_radius_px)
                    for a, b in zip(catalog, hcatalog)) and
                table.source.tolist() == [e[0] for e in ent] and table.image.tolist() == [e[1] for e in ent] and
                table.box.tolist() == [[p.box[0][0], p.box[0][1], p.box[1][0], p.box[1][1]] for _, _, p in ent] and
                table.active_pixels.tolist() == [int(p.active_pixel_bitmap.sum()) for _, _, p in ent] and
                table.neighbor_lists == hneighbors)


def time_scene(name, images, cats, host_reps=REPS, end_to_end=True, infer_reps=3):
    print("%s: %d images, %d detections" % (name, len(images), sum(len(c) for c in cats)), flush=True)
    out = dict(n_images=len(images), n_detections=int(sum(len(c) for c in cats)), match_radius=RADIUS)
    warm = 1 if host_reps > 1 else 0
    # ---- the device path
    with prep.PrepImages(images, 0) as pi:
        stages = []

        def reused():
            r = prep.detected_table(images, cats, RADIUS, prep_images=pi)
            stages.append(prep.detected_last_ms())
            return r
        out["detected_table_reused_s"], (catalog, table) = timed(reused)
        out["device_ms"] = {k: float(np.median([s[k] for s in stages[1:]])) for k in prep.DETECTED_STAGES}
    out["n_objects"], out["entries"], out["sparse"] = len(catalog), int(len(table.source)), not table.dense
    out["neighbor_links"] = int(sum(len(r) for r in table.neighbor_lists))
    out["detected_table_own_upload_s"], _ = timed(lambda: prep.detected_table(images, cats, RADIUS, device=0))
    out["problem_from_table_s"], _ = timed(lambda: cabi.problem_from_table(images, table, table.neighbors()))
    # ---- the host functions, same process, same inputs
    worlds = [detect.world_coords(c, im) for c, im in zip(cats, images)]
    out["host_match_detections_s"], _ = timed(lambda: detect.match_detections(worlds, RADIUS), host_reps, warm)
    print("  host match_detections: %.3f s" % out["host_match_detections_s"], flush=True)
    out["host_build_detection_output_s"], (hcatalog, patches) = timed(lambda: detect.build_detection_output(images, cats, RADIUS),
                                                                     host_reps, warm)
    print("  host build_detection_output: %.3f s" % out["host_build_detection_output_s"], flush=True)
    out["host_neighbor_map_s"], hnb = timed(lambda: model.neighbor_map(patches), host_reps, warm)
    out["host_cabi_problem_s"], _ = timed(lambda: cabi.Problem(images, patches, hnb), host_reps, warm)
    out["host_runs"] = host_reps
    out["device_results_equal_host"] = same_as_host(images, catalog, table, hcatalog, patches, hnb)
    ms = out["device_ms"]
    out["host_over_device"] = dict(
        join=out["host_match_detections_s"] / (ms["join"] * 1e-3),
        entries_and_patches=(out["host_build_detection_output_s"] - out["host_match_detections_s"]) /
        ((ms["entries"] + ms["geometry"] + ms["active_pixels"] + ms["stamps"]) * 1e-3),
        neighbors=out["host_neighbor_map_s"] / (ms["neighbors"] * 1e-3),
        problem=out["host_cabi_problem_s"] / out["problem_from_table_s"],
        whole=(out["host_build_detection_output_s"] + out["host_neighbor_map_s"] + out["host_cabi_problem_s"]) /
        (out["detected_table_own_upload_s"] + out["problem_from_table_s"]))
    del patches, table
    if end_to_end:
        box = cel.BoundingBox(-1e9, 1e9, -1e9, 1e9)
        res = {}
        for mode in ("host", "device"):
            out["infer_box_joint_vi_prep_%s_s" % mode], res[mode] = timed(
                lambda: cel.infer_box(images, box, method="joint_vi", match_radius=RADIUS, prep=mode), infer_reps)
        out["infer_box_host_over_device"] = out["infer_box_joint_vi_prep_host_s"] / out["infer_box_joint_vi_prep_device_s"]
        out["infer_box_targets"] = len(res["host"])
        out["infer_box_results_equal"] = bool(len(res["host"]) == len(res["device"]) and all(
            a.vs.tobytes() == b.vs.tobytes() and a.is_sky_bad == b.is_sky_bad for a, b in zip(res["host"], res["device"])))
        out["infer_box_vs_max_abs_difference"] = float(max(np.abs(a.vs - b.vs).max() for a, b in zip(res["host"], res["device"])))
    print(json.dumps({name: out}, indent=1), flush=True)
    return out


def main():
    import torch
    assert torch.cuda.is_available(), "this tool measures on the device"
    small = "--small" in sys.argv
    out = {"reps": REPS, "device": torch.cuda.get_device_name(0)}
    path = os.path.join(ROOT, "profiles", "detected_table_time_small.json" if small else "detected_table_time_mi355x.json")

    def save():
        if not small:
            with open(path, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
    H, W, n = (256, 256, 60) if small else (2048, 1489, 2000)
    for variable in (False, True):
        images, _ = bench_field(H, W, n, variable)
        cats = detect.extract(images, want_pixels=False)
        key = "%s_%dx%dx5_%d_sources_%s_psf" % ("small" if small else "bench_field", H, W, n, "variable" if variable else "constant")
        out[key] = time_scene(key, images, cats, infer_reps=1 if small else 3)
        save()
        del images
    if "--no-80" not in sys.argv:
        grid, (H, W), n = ((2, 2), (128, 128), 300) if small else ((4, 4), (2048, 1489), 30000)
        images, th, tw = grid_images(grid, H, W)
        cats = synthetic_catalogs(images, catalog_of(th, tw, n, 5, 8), 7)
        key = "grid_%dx%d_%d_images_%dx%d_%d_sources" % (grid + (len(images), H, W, n))
        out[key] = time_scene(key, images, cats, host_reps=1, end_to_end=False)
        save()
    print(json.dumps(out, indent=1))
    print("wrote", path if not small else "nothing (--small)")


if __name__ == "__main__":
    main()
