"""Time of PhotContext.light_curves on one GPU, beside FitContext.stats of the same targets in the same process -- the existing
pass over the same pixels with the same densities, and the only comparison that means anything.

Two scenes: the bench field (2048 x 1489 x 5, 2000 sources, all of them targets) and a config-5-shaped sparse scene of
overlapping fields (make_multifield, 2 x 4 fields of 400 x 400, 1500 sources, all of them targets).  Per scene and case one
warm-up call, then `--repeats` calls; reported: median, min and max of
  - the device time per stage (celeste_phot_last_ms: per-visit tables, pixel pass, solve pass, band summaries;
    celeste_fit_last_ms: per-visit tables, pixel kernel, per-target sums),
  - the wall time of the call (host clock around a call that ends in a stream synchronise: uploads, launches, downloads),
and the mean and the largest number of Newton iterations, the flags, and the split of the entries between the two solve paths.
A third case forces every patch of more than one tile onto the streaming path (lds_max_pixels = 64).

    python tools/gpu_phot_time.py --out profiles/phot_time_mi355x.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from celeste_jl_amd import cabi, fit, phot, synthetic  # noqa: E402


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def measure(name, f, repeats):
    S = len(f.catalog)
    targets = np.arange(S, dtype=np.int32)
    problem = cabi.Problem(f.images, f.patches, f.neighbors)
    fc = fit.FitContext(problem)
    pc = phot.PhotContext(problem)
    rec = {"scene": name, "sources": S, "images": len(f.images), "targets": S}
    try:
        cases = (("fit_stats", lambda: fc.stats(f.vp, targets), fc.last_ms, ("tables", "pixel", "sums")),
                 ("light_curves", lambda: pc.light_curves(f.vp, targets), pc.last_ms, ("tables", "pixel", "solve", "summaries")),
                 ("light_curves_streamed", lambda: pc.light_curves(f.vp, targets, lds_max_pixels=64), pc.last_ms,
                  ("tables", "pixel", "solve", "summaries")))
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
                rec["n_pix"] = int(out.n_pix.sum())
            if case == "light_curves":
                npx = np.array([h2 * w2 for s in range(S) for _, h2, w2 in fit.patch_shapes(problem)[s]])
                rec["entries"] = int(len(out.alpha))
                rec["entries_streamed"] = int((npx > phot.LDS_PIXELS).sum())
                rec["largest_patch_pixels"] = int(npx.max())
                rec["flags"] = {k: int((out.flag == v).sum()) for k, v in (("ok", phot.OK), ("no_light", phot.NO_LIGHT),
                                ("at_bound", phot.AT_BOUND), ("not_converged", phot.NOT_CONVERGED), ("bad_model", phot.BAD_MODEL))}
                it = out.iters[out.iters > 0]
                rec["newton_iterations"] = {"mean": float(it.mean()), "max": int(it.max())}
                base = out
            if case == "light_curves_streamed":
                rec["streamed_equals_lds_bit_for_bit"] = bool(all(
                    np.array_equal(getattr(out, k), getattr(base, k), equal_nan=True) for k in ("alpha", "sigma", "chi2", "iters", "flag", "summary")))
        for k in ("device_ms", "wall_ms"):
            rec["light_curves_over_fit_stats_" + k] = rec["light_curves"][k]["median"] / rec["fit_stats"][k]["median"]
        st = rec["light_curves"]["device_ms_by_stage"]
        rec["solve_over_pixel_pass"] = st["solve"]["median"] / st["pixel"]["median"]
    finally:
        pc.close()
        fc.close()
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phot_time_mi355x.json"))
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
                   "downloads of the results).  Median of the repeats after one warm-up call, both libraries in one process."}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
