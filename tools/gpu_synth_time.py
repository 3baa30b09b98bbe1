"""Device time of synthetic image generation (celeste_synth_generate: HIP events around the stamp prefilter, the galaxy
tables and the pixel kernel), the median of 5 calls after a warm-up, on
  * the bench field: 2048 x 1489 x 5, 2000 prior-drawn sources (the catalog make_field draws for seed 1);
  * 80 images of 2048 x 1489 on the 4 x 4 grid with 30 000 sources (the catalog make_multifield draws for seed 5),
and, beside each, the wall time of the host function synthetic.gen_images for ONE image of the same field on the same
machine.  Per kernel: milliseconds, pixels per second, the algorithmic bytes (8 B per pixel: the sky read and the pixel
written, plus the entry, stamp-coefficient and galaxy-component tables) over the time against the HBM peak, an estimate of
the fp64 operations over the time against the fp64 vector peak, and which of the two bounds is the larger.
Writes profiles/synth_time_mi355x.json (and prints it).  --small: a 256 x 256 x 5 field only (a rehearsal of the script)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from celeste_jl_amd import synth, synthetic  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s (MI355X, HBM3E specification)
FP64_PEAK = 78.6e12        # FLOP / s, fp64 vector (DESIGN.md section 5's nominal figure)
# fp64 operations per unit of work, counted from the kernels' source (an FMA = 2): a galaxy component of one pixel (3 FMA for
# the exponent, the table-driven exp's 16 instructions, 1 FMA), a star's 4 x 4 spline with its weights, a PTRS draw
# (sqrt, 2 logs, 3 divisions and the transform; the integer Philox rounds are not fp64 work)
OPS_GAL_COMP, OPS_STAR, OPS_SAMPLE = 30, 110, 120


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


def work_of(images, entries, stamps):
    px = sum(im.H * im.W for im in images)
    area = (entries["h1"] - entries["h0"] + 1).astype(np.int64) * (entries["w1"] - entries["w0"] + 1)
    star = entries["is_star"] != 0
    nc = np.array([14 * np.asarray(im.psf).shape[0] for im in images])[entries["image"]]
    n_gal = int((~star).sum())
    table_bytes = 48 * len(entries) + 8 * 53 * 53 * len(stamps) + 64 * int(nc[~star].sum())
    ops = 2 * (OPS_GAL_COMP * int((area[~star] * nc[~star]).sum()) + OPS_STAR * int(area[star].sum()) + OPS_SAMPLE * px)
    return dict(pixels=px, entries=int(len(entries)), star_entries=int(star.sum()), galaxy_entries=n_gal, stamps=int(len(stamps)),
                box_pixels=int(area.sum()), algorithmic_bytes=8 * px + table_bytes, table_bytes=table_bytes, fp64_ops_estimate=ops)


def time_scene(name, images, catalog, reps=5):
    t0 = time.perf_counter()
    entries, stamps = synth.entry_table(images, catalog)
    table_s = time.perf_counter() - t0
    work = work_of(images, entries, stamps)
    print("%s: %d images, %d entries; warm-up" % (name, len(images), len(entries)), flush=True)
    synth.generate_raw(images, entries, stamps, seed=1)
    ms, walls, capped = [], [], 0
    for r in range(reps):
        t0 = time.perf_counter()
        _, _, cap = synth.generate_raw(images, entries, stamps, seed=2 + r)
        walls.append(time.perf_counter() - t0)
        ms.append(synth.last_ms())
        capped += cap
        print("  call %d: device ms %s, wall %.3f s" % (r, ["%.3f" % x for x in ms[-1]], walls[-1]), flush=True)
    med = [float(x) for x in np.median(np.array(ms), axis=0)]
    # the same call without the sampler (pixels = Float32 of the expected electrons): what of the pixel kernel is rendering
    ems = []
    for r in range(reps):
        synth.generate_raw(images, entries, stamps, seed=2 + r, expectation=True)
        ems.append(synth.last_ms()[2])
    print("  expectation only: pixel kernel ms %s" % ["%.3f" % x for x in ems], flush=True)
    kern = {}
    for k, label in enumerate(("spline_prefilter_kernel", "syn_tables_kernel", "syn_pixel_kernel")):
        kern[label] = dict(ms=med[k])
    t = med[2] * 1e-3
    t_hbm, t_fp64 = work["algorithmic_bytes"] / HBM_PEAK, work["fp64_ops_estimate"] / FP64_PEAK
    kern["syn_pixel_kernel"].update(
        ms_without_sampling=float(np.median(ems)),
        pixels_per_s=work["pixels"] / t, algorithmic_bytes_per_s=work["algorithmic_bytes"] / t,
        share_of_hbm_peak=work["algorithmic_bytes"] / t / HBM_PEAK, fp64_ops_per_s_estimate=work["fp64_ops_estimate"] / t,
        share_of_fp64_vector_peak_estimate=work["fp64_ops_estimate"] / t / FP64_PEAK,
        least_ms_hbm=t_hbm * 1e3, least_ms_fp64_estimate=t_fp64 * 1e3, bound="fp64 vector" if t_fp64 > t_hbm else "HBM")
    # the host function on one image of the same field (the middle band), on this machine
    img = images[2]
    t0 = time.perf_counter()
    synthetic.gen_images([img], catalog, np.random.Generator(np.random.PCG64(3)))
    host_s = time.perf_counter() - t0
    device_ms = float(sum(med))
    out = dict(work, entry_table_host_s=table_s, kernels=kern, device_ms=device_ms, call_wall_s=float(np.median(walls)),
               n_capped=int(capped), host_gen_images_one_image_s=host_s, host_s_per_image_over_device_s_per_image=host_s / (
                   device_ms * 1e-3 / len(images)), host_s_per_image_over_call_wall_s_per_image=host_s / (np.median(walls) / len(images)))
    print(json.dumps({name: out}, indent=1), flush=True)
    return out


def main():
    out = {"hbm_peak_bytes_per_s": HBM_PEAK, "fp64_vector_peak_flops": FP64_PEAK, "reps": 5,
           "ops_per_unit": dict(galaxy_component=OPS_GAL_COMP, star=OPS_STAR, sample=OPS_SAMPLE)}
    if "--small" in sys.argv:
        out["small_256x256x5_60_sources"] = time_scene("small", synthetic.blank_images(256, 256), catalog_of(256, 256, 60, 1, 26))
        print(json.dumps(out, indent=1))
        return
    out["bench_field_2048x1489x5_2000_sources"] = time_scene("bench field", synthetic.blank_images(2048, 1489),
                                                             catalog_of(2048, 1489, 2000, 1, 26))
    images, th, tw = grid_images((4, 4), 2048, 1489)
    out["grid_4x4_80_images_2048x1489_30000_sources"] = time_scene("4 x 4 grid", images, catalog_of(th, tw, 30000, 5, 8))
    path = os.path.join(ROOT, "profiles", "synth_time_mi355x.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
