"""Time of celeste_blend_maximize per Newton iteration on one GPU, split into evaluation and step, for B = 1, 64, 512 blends
of Sa = 2, 3, 4 sources; beside it, the same evaluations as B sequential celeste_elbo_eval_multi calls.

The field is a grid of identical tiles, each holding one cluster of Sa overlapping sources (one tile rendered and sampled,
then repeated), so that B conflict-free blends exist.  Per case: one warm-up call, then `--repeats` calls of
maximize_blends with max_iters = `--iters`; the device times come from celeste_blend_last_ms (summed over a call's
iterations, divided by its iteration count).  Reported: median, min and max over the repeats.

    python tools/gpu_blend_time.py --out profiles/blend_time_mi355x.json
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
from celeste_jl_amd import synthetic  # noqa: E402
from celeste_jl_amd.params import catalog_init_source, perturb_params  # noqa: E402

TILE = 64


def clustered_field(sa, n_tiles, seed=0):
    """n_tiles (rounded up to a square) copies of one TILE x TILE tile with a cluster of sa sources at its centre"""
    rng = np.random.Generator(np.random.PCG64(seed + sa))
    prior = synthetic.load_prior()
    tile_imgs = synthetic.blank_images(TILE, TILE)
    cat = [synthetic.draw_source(prior, rng, (TILE / 2 + rng.uniform(-3, 3), TILE / 2 + rng.uniform(-3, 3))) for _ in range(sa)]
    synthetic.gen_images(tile_imgs, cat, rng)
    g = int(np.ceil(np.sqrt(n_tiles)))
    images = synthetic.blank_images(TILE * g, TILE * g)
    for img, t in zip(images, tile_imgs):
        img.pixels[:] = np.tile(t.pixels, (g, g))
    catalog = []
    for i in range(g):
        for j in range(g):
            for ce in cat:
                e = type(ce)(**{k: getattr(ce, k) for k in ce.__dataclass_fields__}) if hasattr(ce, "__dataclass_fields__") else ce
                e.pos = np.array([ce.pos[0] + TILE * i, ce.pos[1] + TILE * j])
                catalog.append(e)
    return images, catalog


def conflict_free_clusters(neighbors, sa, n_clusters):
    """the clusters (sources k sa .. k sa + sa - 1) no member of which neighbours a member of a kept cluster"""
    owner, kept = {}, []
    for k in range(n_clusters):
        mem = list(range(k * sa, (k + 1) * sa))
        if any(owner.get(t, k) != k for s in mem for t in neighbors[s]) or any(s in owner for s in mem):
            continue
        for s in mem:
            owner[s] = k
        kept.append(mem)
    return kept


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blend_time_mi355x.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--seq-repeats", type=int, default=3)
    a = ap.parse_args()
    cases = []
    for sa in (2, 3, 4):
        # enough tiles for 512 conflict-free clusters: every other tile (the neighbour lists decide)
        images, catalog = clustered_field(sa, 520)
        ctx = cel.FieldContext.from_catalog(images, catalog)
        nbrs = ctx.table.neighbors()
        sym = [set(x) for x in nbrs]
        for s, x in enumerate(nbrs):
            for t in x:
                sym[t].add(s)
        clusters = conflict_free_clusters(sym, sa, len(catalog) // sa)
        vp = np.stack([catalog_init_source(ce) for ce in catalog])
        perturb_params(vp)
        bc = ctx.blend_context()
        cfg = cel.ElboConfig(max_iters=a.iters)
        for B in (1, 64, 512):
            if len(clusters) < B:
                print("sa %d: only %d conflict-free clusters, skipping B = %d" % (sa, len(clusters), B), flush=True)
                continue
            blends = clusters[:B]
            bc.maximize_blends(vp, blends, cfg)                           # warm-up
            ev, st, wall, its = [], [], [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                _, it, _, _, status = bc.maximize_blends(vp, blends, cfg)
                w = (time.perf_counter() - t0) * 1e3
                e_ms, s_ms, n = bc.last_ms()
                assert (status == 0).all()
                ev.append(e_ms / n); st.append(s_ms / n); wall.append(w / n); its.append(n)
            bc.eval_blends(vp, blends)                                     # warm-up
            batched = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                bc.eval_blends(vp, blends)
                batched.append((time.perf_counter() - t0) * 1e3)
            seq = []
            for _ in range(a.seq_repeats):
                t0 = time.perf_counter()
                for bl in blends:
                    ctx.eval_multi(vp, bl)
                seq.append((time.perf_counter() - t0) * 1e3)
            rec = {"sa": sa, "blends": B, "n_free": 41 * sa, "iterations_per_call": int(np.median(its)),
                   "eval_ms_per_iter_device": stats(ev), "step_ms_per_iter_device": stats(st),
                   "wall_ms_per_iter": stats(wall), "eval_blends_wall_ms": stats(batched),
                   "sequential_eval_multi_wall_ms": stats(seq)}
            print(json.dumps(rec), flush=True)
            cases.append(rec)
        bc.close()
        ctx.close()
    out = {"device": "MI355X", "repeats": a.repeats, "max_iters": a.iters, "tile_px": TILE, "cases": cases,
           "note": "device ms: celeste_blend_last_ms per iteration; wall ms include the host driver and copies"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
