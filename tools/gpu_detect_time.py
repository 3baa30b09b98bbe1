"""Device time of each detection stage (HIP events inside celeste_detect_run) and Mpx/s, on a 2048 x 1489 x 5 field
(the size of configs[2]) and on 80 images of 1024 x 1024 (the image count of configs[4]), plus the numpy restatement
(tests/detect_reference.py) on the CPU for one image.  Images: sky + Poisson-like noise + Gaussian sources (numpy,
seeded); detection's cost does not depend on how the sources were rendered.  Writes JSON to stdout."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from celeste_jl_amd import detect  # noqa: E402
from celeste_jl_amd.model import Image, ConstantPSFMap  # noqa: E402


def image(H, W, n_src, seed):
    rng = np.random.default_rng(seed)
    cal = rng.normal(0.0, 0.03, (H, W))
    for _ in range(n_src):
        ci, cj, s, f = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1.2, 4.0), rng.lognormal(1.0, 1.2)
        i0, i1, j0, j1 = int(max(ci - 5 * s, 0)), int(min(ci + 5 * s + 1, H)), int(max(cj - 5 * s, 0)), int(min(cj + 5 * s + 1, W))
        ii, jj = np.meshgrid(np.arange(i0, i1), np.arange(j0, j1), indexing="ij")
        cal[i0:i1, j0:j1] += f * np.exp(-0.5 * ((ii - ci) ** 2 + (jj - cj) ** 2) / s ** 2) / (2 * np.pi * s * s)
    sky = np.full((H, W), 0.1, np.float32)
    nelec = np.full(H, 150.0, np.float32)
    px = ((cal + sky) * nelec[:, None]).astype(np.float32)
    return Image(pixels=px, b=3, psf=np.zeros((2, 6)), sky=sky, nelec_per_nmgy=nelec,
                 psfmap=ConstantPSFMap(np.zeros((51, 51))))


def time_device(images, reps=5):
    detect.extract(images)                                     # warm-up (module load, allocations)
    stages, walls = [], []
    for _ in range(reps):
        st = {}
        t0 = time.perf_counter()
        cats = detect.extract(images, stage_ms=st)
        walls.append((time.perf_counter() - t0) * 1e3)
        stages.append(st)
    med = {k: float(np.median([s[k] for s in stages])) for k in detect.STAGES}
    px = sum(im.H * im.W for im in images)
    dev = sum(med.values())
    return dict(images=len(images), pixels=px, objects=sum(len(c) for c in cats), stage_ms=med, device_ms=dev,
                wall_ms=float(np.median(walls)), device_mpx_per_s=px / dev / 1e3, wall_mpx_per_s=px / np.median(walls) / 1e3)


def main():
    out = {}
    field = [image(2048, 1489, 1500, 100 + b) for b in range(5)]
    out["configs2_field_2048x1489x5"] = time_device(field)
    many = [image(1024, 1024, 400, 200 + n) for n in range(80)]
    out["configs4_80_images_1024x1024"] = time_device(many, reps=3)
    import detect_reference as R
    t0 = time.perf_counter()
    R.extract(field[0].pixels, field[0].sky, field[0].nelec_per_nmgy)
    cpu = (time.perf_counter() - t0) * 1e3
    out["cpu_restatement_one_2048x1489_image"] = dict(ms=cpu, threads=1, mpx_per_s=2048 * 1489 / cpu / 1e3)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
