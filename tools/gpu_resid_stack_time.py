"""Time of ResidualSearch.stack on one GPU, beside the search it follows, in the same process (a sibling of gpu_resid_time.py,
with its scenes).

Scenes and passes:
  the bench field (2048 x 1489 x 5, 2000 sources), five aligned images, on the grid of its first image: 1 channel (flat), and 6
      channels (five one-band channels and a flat one);
  80 images of 1024 x 1024 (a 4 x 4 grid of overlapping fields) on resid.grid_covering of all of them, 1 channel: culling on, and
      culling off (CELESTE_STACK_NO_CULL=1).
Per pass one warm-up call, then `--repeats` calls; reported: the median device time of the two stages (celeste_resid_stack_last_ms:
the gather with the z ranges; the peaks with their world positions), the median wall time of the call, and the bytes the gather
must move: 24 per added (cell, image) sample (N, D, z of the image; a masked sample reads z alone and is not counted) and 28 per
(cell, channel) written (N, D, z, count).  "share_of_hbm_rate" divides those bytes by the gather's device time and by the 6.29 TB/s
a float4 copy reaches on this part; it counts the bytes that must move, not the bytes that moved (no counter was read).

    python tools/gpu_resid_stack_time.py --out profiles/resid_stack_time_mi355x.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from celeste_jl_amd import cabi, resid, synthetic  # noqa: E402

HBM_COPY_RATE = 6.29e12      # bytes per second: a float4 copy on an MI355X
FLAT = [1.0] * 5
ONE = [[1.0 if b == k else 0.0 for b in range(5)] for k in range(5)]


def med(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def one_pass(rc, s, grid, weights, repeats, cull):
    if cull:
        os.environ.pop("CELESTE_STACK_NO_CULL", None)
    else:
        os.environ["CELESTE_STACK_NO_CULL"] = "1"
    try:
        s.stack(grid, weights)                                       # warm-up (allocations)
        wall, dev = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            st = s.stack(grid, weights)
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(rc.stack_last_ms())
        samples = int(sum(st.map(k, "count").sum() for k in range(len(weights))))
    finally:
        os.environ.pop("CELESTE_STACK_NO_CULL", None)
    d = np.asarray(dev)
    cells = int(grid.H) * int(grid.W)
    moved = 24 * samples + 28 * cells * len(weights)
    return {"channels": len(weights), "culling": bool(cull), "grid": [int(grid.H), int(grid.W)], "wall_ms": med(wall),
            "device_ms": med(d.sum(axis=1)), "device_ms_by_stage": {"gather": med(d[:, 0]), "peaks": med(d[:, 1])},
            "samples_added": samples, "bytes_that_must_move": moved,
            "share_of_hbm_rate": moved / (med(d[:, 0]) * 1e-3) / HBM_COPY_RATE, "candidates": int(st.n_found),
            "cells_with_z": [int(x) for x in st.frames["n_cells"]]}


def measure(name, f, repeats, passes):
    problem = cabi.Problem(f.images, f.patches, f.neighbors)
    rec = {"scene": name, "sources": len(f.catalog), "images": len(f.images), "pixels": sum(im.H * im.W for im in f.images), "stack": []}
    with resid.ResidContext(problem) as rc:
        rc.search(f.vp)                                              # warm-up
        dev = []
        for _ in range(repeats):
            s = rc.search(f.vp)
            dev.append(sum(rc.last_ms()))
        rec["search_device_ms"] = med(dev)
        for grid, weights, cull in passes(f):
            rec["stack"].append(one_pass(rc, s, grid, weights, repeats, cull))
            print(json.dumps({"scene": name, **rec["stack"][-1]}), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resid_stack_time_mi355x.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bench-sources", type=int, default=2000)
    ap.add_argument("--many-sources", type=int, default=4000)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    f = synthetic.make_field(2048, 1489, a.bench_sources, seed=3, name="bench field", device=0)
    scenes = [measure("bench field 2048x1489x5", f, a.repeats,
                      lambda f: [(resid.StackGrid.of_image(f.images[0]), [FLAT], True), (resid.StackGrid.of_image(f.images[0]), ONE + [FLAT], True)])]
    del f
    g = synthetic.make_multifield((4, 4), 1024, 1024, 0.10, a.many_sources, seed=5, sparse=True, device=0)

    def many(g):
        grid = resid.grid_covering(g.images, list(range(len(g.images))))
        return [(grid, [FLAT], True), (grid, [FLAT], False)]
    scenes.append(measure("80 images 1024x1024", g, a.repeats, many))
    out = {"device": "MI355X", "repeats": a.repeats, "warmup": 1, "scenes": scenes,
           "note": "device ms: HIP events per stage; wall ms: host clock around the call.  Median of the repeats after one warm-up call, "
                   "all in one process.  bytes_that_must_move and share_of_hbm_rate: see the tool's docstring; no counter was read."}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
