"""Time of ResidContext.search on one GPU, beside the two things it is measured against in the same process: the engine's
expected image (five celeste_render_expected calls on the bench field's images) and source detection (celeste_detect_run) on the
same images.

Scenes: the bench field (2048 x 1489 x 5, 2000 sources) and 80 images of 1024 x 1024 (a 4 x 4 grid of overlapping fields, the
image count of gpu_detect_time.py's second scene, here with a catalog: a search needs a model).  Pixels are drawn on the device.
Per scene one warm-up search, then `--repeats` searches; reported: the median device time per stage (celeste_resid_last_ms:
per-visit tables, frame model, filter, peaks) and of their sum, and the median wall time of the call (uploads, launches, the
download of summaries and candidates; no plane is copied).  celeste_render_expected has no stage clock: its wall time per call is
reported, which includes the copy of the plane to the host that every call makes.

    python tools/gpu_resid_time.py --out profiles/resid_time_mi355x.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import celeste_jl_amd as cel  # noqa: E402
from celeste_jl_amd import cabi, detect, resid, synthetic  # noqa: E402

STAGES = ("tables", "frame_model", "filter", "peaks")


def med(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def measure(name, f, repeats, render):
    problem = cabi.Problem(f.images, f.patches, f.neighbors)
    px = sum(im.H * im.W for im in f.images)
    rec = {"scene": name, "sources": len(f.catalog), "images": len(f.images), "pixels": px}
    with resid.ResidContext(problem) as rc:
        rc.search(f.vp)                                              # warm-up (module load, allocations, the tile table)
        wall, dev = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            s = rc.search(f.vp)
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(rc.last_ms())
        d = np.asarray(dev)
        rec["search"] = {"wall_ms": med(wall), "device_ms": med(d.sum(axis=1)),
                         "device_ms_by_stage": {k: med(d[:, i]) for i, k in enumerate(STAGES)},
                         "device_mpx_per_s": px / med(d.sum(axis=1)) / 1e3, "candidates": int(s.n_found),
                         "frames_ok": int((s.frames["status"] == 0).sum()), "chi2_per_px": float(s.frames["chi2"].sum() / s.frames["n_px"].sum())}
    print(json.dumps(rec), flush=True)
    if render:
        ctx = cel.FieldContext(f.images, None, f.neighbors, problem=problem)
        try:
            for n in range(len(f.images)):
                ctx.render_expected(f.vp, n)                         # warm-up
            walls = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                for n in range(len(f.images)):
                    ctx.render_expected(f.vp, n)
                walls.append((time.perf_counter() - t0) * 1e3)
            rec["render_expected_all_images"] = {"wall_ms": med(walls), "calls": len(f.images)}
        finally:
            ctx.close()
    st_all, walls = [], []
    detect.extract(f.images)                                         # warm-up
    for _ in range(repeats):
        st = {}
        t0 = time.perf_counter()
        cats = detect.extract(f.images, stage_ms=st)
        walls.append((time.perf_counter() - t0) * 1e3)
        st_all.append(sum(st[k] for k in detect.STAGES))
    rec["detect_run"] = {"wall_ms": med(walls), "device_ms": med(st_all), "objects": int(sum(len(c) for c in cats))}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resid_time_mi355x.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bench-sources", type=int, default=2000)
    ap.add_argument("--many-sources", type=int, default=4000)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    t0 = time.perf_counter()
    f = synthetic.make_field(2048, 1489, a.bench_sources, seed=3, name="bench field", device=0)
    print("bench field made in %.1f s" % (time.perf_counter() - t0), flush=True)
    scenes = [measure("bench field 2048x1489x5", f, a.repeats, render=True)]
    del f
    t0 = time.perf_counter()
    g = synthetic.make_multifield((4, 4), 1024, 1024, 0.10, a.many_sources, seed=5, sparse=True, device=0)
    print("80 images made in %.1f s" % (time.perf_counter() - t0), flush=True)
    scenes.append(measure("80 images 1024x1024", g, a.repeats, render=False))
    out = {"device": "MI355X", "repeats": a.repeats, "warmup": 1, "scenes": scenes,
           "note": "device ms: HIP events per stage; wall ms: host clock around the call.  Median of the repeats after one warm-up "
                   "call, all in one process.  render_expected: wall only (no stage clock), plane copies included."}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
