"""Time of InfoContext.bounds on one GPU, beside FitContext.stats and the engine's value-only sweep (flags = 0) of the same
targets in the same process.

The bench field (2048 x 1489 x 5, 2000 sources, all of them targets).  Per case `--warmup` calls that are not reported except
the first (a call on the chip's clock ramp is not a steady-state figure: the first call's device time is recorded beside the
median so that the ramp shows), then `--repeats` calls; reported: median, min and max of
  - the device time per stage (celeste_info_last_ms: per-visit tables, pixel kernel, per-target sums, solve; celeste_fit_last_ms;
    the engine's celeste_ctx_last_kernel_ms: tables, pixel kernel with the neighbours' rendering, lift),
  - the wall time of the call (host clock around a call that ends in a stream synchronise: uploads, launches, downloads).
The cases alternate inside every repeat, so that a drift of the clock touches all of them alike.

    python tools/gpu_info_time.py --out profiles/info_time_mi355x.json
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
from celeste_jl_amd import fit, info, synthetic  # noqa: E402


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def measure(name, f, repeats, warmup):
    S = len(f.catalog)
    targets = np.arange(S, dtype=np.int32)
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    fc = fit.FitContext(ctx.problem)
    ic = info.InfoContext(ctx.problem)
    rec = {"scene": name, "sources": S, "images": len(f.images), "targets": S}
    try:
        ctx.enable_timing(True)
        ws = ctx.work_stats(targets)
        rec["active_pixel_visits"] = int(ws["active_pixel_visits"])
        rec["neighbor_links"] = int(ws["neighbor_links"])
        cases = (("value_only_sweep", lambda: ctx.eval_batch(f.vp, targets, 0), ctx.last_kernel_ms, ("tables", "pixel", "lift")),
                 ("fit_stats", lambda: fc.stats(f.vp, targets), fc.last_ms, ("tables", "pixel", "sums")),
                 ("info_bounds", lambda: ic.bounds(f.vp, targets), ic.last_ms, ("tables", "pixel", "sums", "solve")))
        wall = {c[0]: [] for c in cases}
        dev = {c[0]: [] for c in cases}
        first = {}
        for r in range(warmup + repeats):
            for case, call, last_ms, _ in cases:
                t0 = time.perf_counter()
                out = call()
                w = (time.perf_counter() - t0) * 1e3
                d = list(last_ms())
                if r == 0:
                    first[case] = float(sum(d))
                if r >= warmup:
                    wall[case].append(w)
                    dev[case].append(d)
                if case == "info_bounds" and r == warmup + repeats - 1:
                    rec["n_pix"] = int(out.n_pix.sum())
                    rec["status_ok"] = int((out.status == 0).sum())
                    rec["flag_counts"] = {str(k): int(((out.flag & k) != 0).sum()) for k in (1, 2, 4, 8)}
                    ok = (out.flag[:, 0] == 0)
                    rec["median_star_pos_stderr_px"] = float(np.median(out.pos_stderr(0)[ok]))
        for case, _, _, stages in cases:
            d = np.asarray(dev[case])
            rec[case] = {"wall_ms": stats(wall[case]), "device_ms": stats(d.sum(axis=1)), "first_call_device_ms": first[case],
                         "device_ms_by_stage": {s: stats(d[:, k]) for k, s in enumerate(stages)}}
        rec["info_over_fit_device"] = rec["info_bounds"]["device_ms"]["median"] / rec["fit_stats"]["device_ms"]["median"]
        rec["info_over_value_only_device"] = rec["info_bounds"]["device_ms"]["median"] / rec["value_only_sweep"]["device_ms"]["median"]
        rec["info_pixel_ns_per_visit"] = 1e6 * rec["info_bounds"]["device_ms_by_stage"]["pixel"]["median"] / rec["active_pixel_visits"]
    finally:
        ic.close()
        fc.close()
        ctx.close()
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "info_time_mi355x.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bench-sources", type=int, default=2000)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    f = synthetic.make_field(2048, 1489, a.bench_sources, seed=3, name="bench field")
    scenes = [measure("bench field 2048x1489x5", f, a.repeats, a.warmup)]
    out = {"device": "MI355X", "repeats": a.repeats, "warmup": a.warmup, "scenes": scenes,
           "note": "device ms: HIP events per stage, summed; wall ms: host clock around the call (uploads of the table, launches, "
                   "downloads of the results).  Median of the repeats after the warm-up calls, the three libraries in one process, "
                   "the cases alternating inside every repeat; first_call_device_ms is the first warm-up call (clock ramp, "
                   "first launches)."}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
