"""Time of AstromContext.offsets on one GPU, beside PhotContext.light_curves and InfoContext.bounds of the same targets in the
same process.

Two scenes: the bench field (2048 x 1489 x 5, 2000 sources, all of them targets) and phot's sparse multifield scene
(make_multifield, 2 x 4 fields of 400 x 400, 1500 sources, all of them targets).  Per scene one warm-up round that is not
reported except its device time (a call on the chip's clock ramp is not a steady-state figure), then `--repeats` rounds;
reported: median, min and max of
  - the device time per stage (celeste_astrom_last_ms: per-visit tables, pixel pass, solve pass, summaries; celeste_phot_last_ms;
    celeste_info_last_ms),
  - the wall time of the call (host clock around a call that ends in a stream synchronise: uploads, launches, downloads),
and of the astrometry itself the mean and the largest number of passes per iterated entry and the share of entries per flag.
The cases alternate inside every round, so that a drift of the clock touches all of them alike.

    python tools/gpu_astrom_time.py --out profiles/astrom_time_mi355x.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from celeste_jl_amd import astrom, cabi, info, phot, synthetic  # noqa: E402


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def measure(name, f, repeats, warmup):
    S = len(f.catalog)
    targets = np.arange(S, dtype=np.int32)
    problem = cabi.Problem(f.images, f.patches, f.neighbors)
    ac, pc, ic = astrom.AstromContext(problem), phot.PhotContext(problem), info.InfoContext(problem)
    rec = {"scene": name, "sources": S, "images": len(f.images), "targets": S}
    try:
        cases = (("phot_light_curves", lambda: pc.light_curves(f.vp, targets), pc.last_ms, ("tables", "pixel", "solve", "summary")),
                 ("info_bounds", lambda: ic.bounds(f.vp, targets), ic.last_ms, ("tables", "pixel", "sums", "solve")),
                 ("astrom_offsets", lambda: ac.offsets(f.vp, targets), ac.last_ms, ("tables", "pixel", "solve", "summary")))
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
                if case == "astrom_offsets" and r == warmup + repeats - 1:
                    rec["entries"] = int(len(out.flag))
                    rec["n_pix"] = int(out.n_pix.sum())
                    rec["status_ok"] = int((out.status == 0).sum())
                    rec["flag_share"] = {astrom.FLAG_NAMES[k]: float((out.flag == k).mean()) for k in range(7)}
                    it = out.iters[~np.isin(out.flag, [astrom.NO_LIGHT, astrom.TOO_FAINT, astrom.BAD_MODEL])]
                    rec["passes_per_iterated_entry"] = {"mean": float(it.mean()) if it.size else 0.0, "max": int(it.max()) if it.size else 0}
                    rec["passes_per_entry_mean"] = float(out.iters.mean())
                    rec["pixel_passes"] = int((out.iters.astype(np.int64) * out.n_pix).sum())
                    ok = out.flag == astrom.OK
                    rec["median_pos_stderr_px_of_ok"] = float(np.median(out.pos_stderr_px()[ok])) if ok.any() else None
                    rec["targets_with_motion"] = int((out.summary_flag == 0).sum())
        for case, _, _, stages in cases:
            d = np.asarray(dev[case])
            rec[case] = {"wall_ms": stats(wall[case]), "device_ms": stats(d.sum(axis=1)), "first_call_device_ms": first[case],
                         "device_ms_by_stage": {s: stats(d[:, k]) for k, s in enumerate(stages)}}
        a = rec["astrom_offsets"]
        rec["astrom_over_phot_device"] = a["device_ms"]["median"] / rec["phot_light_curves"]["device_ms"]["median"]
        rec["astrom_over_info_device"] = a["device_ms"]["median"] / rec["info_bounds"]["device_ms"]["median"]
        rec["astrom_solve_ns_per_pixel_pass"] = 1e6 * a["device_ms_by_stage"]["solve"]["median"] / max(rec["pixel_passes"], 1)
        rec["info_pixel_ns_per_pixel"] = 1e6 * rec["info_bounds"]["device_ms_by_stage"]["pixel"]["median"] / max(rec["n_pix"], 1)
        rec["dominant_stage"] = max(a["device_ms_by_stage"], key=lambda s: a["device_ms_by_stage"][s]["median"])
    finally:
        ic.close()
        pc.close()
        ac.close()
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "astrom_time_mi355x.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bench-sources", type=int, default=2000)
    ap.add_argument("--multifield-sources", type=int, default=1500)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    scenes = []
    f = synthetic.make_field(2048, 1489, a.bench_sources, seed=3, name="bench field")
    scenes.append(measure("bench field 2048x1489x5", f, a.repeats, a.warmup))
    del f
    f = synthetic.make_multifield(grid=(2, 4), H=400, W=400, overlap=0.10, n_sources=a.multifield_sources, seed=5, sparse=True)
    scenes.append(measure("multifield 2x4 of 400x400x5, sparse", f, a.repeats, a.warmup))
    out = {"device": "MI355X", "repeats": a.repeats, "warmup": a.warmup, "scenes": scenes,
           "note": "device ms: HIP events per stage, summed; wall ms: host clock around the call (uploads of the table, launches, "
                   "downloads of the results).  Median of the repeats after the warm-up round, the three libraries in one process, "
                   "the cases alternating inside every round; first_call_device_ms is the warm-up call (clock ramp, first launches)."}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
