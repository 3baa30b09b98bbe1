"""Time of FitContext.stats on one GPU, beside the engine's value-only sweep (flags = 0) of the same targets in the same process.

Two scenes: the bench field (2048 x 1489 x 5, 2000 sources, all of them targets) and a config-5-shaped sparse scene of
overlapping fields (make_multifield, 2 x 4 fields of 400 x 400, 1500 sources, all of them targets).  Per scene and case one
warm-up call, then `--repeats` calls; reported: median, min and max of
  - the device time per stage (celeste_fit_last_ms: per-visit tables, pixel kernel, per-target sums; the engine's
    celeste_ctx_last_kernel_ms: tables, pixel kernel with the neighbours' rendering, lift),
  - the wall time of the call (host clock around a call that ends in a stream synchronise: uploads, launches, downloads).
The statistics evaluate a neighbour's light once per (target, pixel) link; the engine renders it once per neighbour pixel and
gathers it.  The scene's pixel visits and neighbour links (celeste_ctx_work_stats) are recorded beside the times.

    python tools/gpu_fit_time.py --out profiles/fit_time_mi355x.json
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
from celeste_jl_amd import fit, synthetic  # noqa: E402


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def measure(name, f, repeats):
    S = len(f.catalog)
    targets = np.arange(S, dtype=np.int32)
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    fc = fit.FitContext(ctx.problem)
    rec = {"scene": name, "sources": S, "images": len(f.images), "targets": S}
    try:
        ctx.enable_timing(True)
        ws = ctx.work_stats(targets)
        rec["active_pixel_visits"] = int(ws["active_pixel_visits"])
        rec["neighbor_links"] = int(ws["neighbor_links"])
        cases = (("value_only_sweep", lambda: ctx.eval_batch(f.vp, targets, 0), ctx.last_kernel_ms, ("tables", "pixel", "lift")),
                 ("fit_stats", lambda: fc.stats(f.vp, targets), fc.last_ms, ("tables", "pixel", "sums")),
                 ("fit_stats_with_stamps", lambda: fc.stats(f.vp, targets, stamps=True), fc.last_ms, ("tables", "pixel", "sums")))
        for case, call, last_ms, stages in cases:
            out = call()                                           # warm-up
            wall, dev = [], []
            for _ in range(repeats):
                t0 = time.perf_counter()
                out = call()
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(list(last_ms()))
            dev = np.asarray(dev)
            rec[case] = {"wall_ms": stats(wall), "device_ms": stats(dev.sum(axis=1)),
                         "device_ms_by_stage": {s: stats(dev[:, k]) for k, s in enumerate(stages)}}
            if case == "fit_stats":
                assert (out.status == 0).all()
                rec["n_pix"] = int(out.n_pix.sum())
                _, total = out.reduced_chi2()
                rec["median_reduced_chi2"] = float(np.median(total))
            if case == "fit_stats_with_stamps":
                rec["stamp_values"] = int(sum(s.size for row in out.stamps for _, s in row))
        rec["fit_over_value_only_device"] = rec["fit_stats"]["device_ms"]["median"] / rec["value_only_sweep"]["device_ms"]["median"]
        rec["fit_over_value_only_wall"] = rec["fit_stats"]["wall_ms"]["median"] / rec["value_only_sweep"]["wall_ms"]["median"]
    finally:
        fc.close()
        ctx.close()
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_time_mi355x.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bench-sources", type=int, default=2000)
    ap.add_argument("--multifield-sources", type=int, default=1500)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    scenes = []
    f = synthetic.make_field(2048, 1489, a.bench_sources, seed=3, name="bench field")
    scenes.append(measure("bench field 2048x1489x5", f, a.repeats))
    del f
    f = synthetic.make_multifield(grid=(2, 4), H=400, W=400, overlap=0.10, n_sources=a.multifield_sources, seed=5, sparse=True)
    scenes.append(measure("config-5-shaped sparse scene, 2x4 fields of 400x400", f, a.repeats))
    out = {"device": "MI355X", "repeats": a.repeats, "scenes": scenes,
           "note": "device ms: HIP events per stage, summed; wall ms: host clock around the call (uploads of the table, launches, "
                   "downloads of the results; with stamps also one double per patch pixel).  Median of the repeats after one "
                   "warm-up call, both libraries in one process."}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
