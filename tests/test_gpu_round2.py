"""-m gpu: round-2 boundary features, all through the C ABI.

* BASELINE configs[3]: one field sharded by source across 2 ranks (two processes on the one GPU, gloo staging) equals
  the single-rank sweep bit for bit -- through bench.py itself, and through parallel.DeviceShardedSweep;
* shared image handle (celeste_images_create / celeste_ctx_create_on): 100 per-source contexts on one handle,
  device memory flat, results identical to the whole-field context (ParallelRun.jl:468-488);
* host-pointer sweep: page-locked and pageable outputs, packed Hessians, parts -- all bit-identical;
* optimiser: duplicate targets refused; a failing target does not take the batch down (ParallelRun.jl:582-597).
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = 7


def _free_device_bytes():
    free, total = C.c_size_t(), C.c_size_t()
    assert C.CDLL("libamdhip64.so").hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def _launch_bench(tmp_path, nproc, extra, **more_env):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **more_env)
    port = 29700 + os.getpid() % 200
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
           "--gpus", str(nproc)] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_strong_scaling_two_ranks_on_one_gpu_equals_single_rank(tmp_path):
    """bench.py --gpus 2 --backend gloo: the SAME field on both ranks, targets sharded by estimate_time, (v, d)
    all-gathered; every rank ends up with the single-rank sweep's numbers, bit for bit"""
    import celeste_jl_amd as cel
    sys.path.insert(0, ROOT)
    import bench
    shape = ["--height", "420", "--width", "380", "--sources", "180", "--seed", "7"]
    d = _launch_bench(tmp_path, 2, shape + ["--backend", "gloo", "--steps", "3", "--warmup", "1", "--full", "--no-extras",
                                            "--check-dir", str(tmp_path)])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["gather_backend"] == "gloo"
    # the same run carries the OTHER driver too: rank 0 alone, one process, two group members (here both on the one device,
    # peer copies; on a node: one per device, RCCL inside the library) while rank 1 waits on the rendezvous store
    gd = d["group_driver"]
    assert "error" not in gd, gd
    assert gd["config"]["members"] == 2 and gd["config"]["gather_backend"] == "peer_copy" and gd["value"] > 0
    assert gd["config"]["shard_sizes"] == d["config"]["shard_sizes"] and not gd["config"]["aborted"]
    sizes = d["config"]["shard_sizes"]
    assert sum(sizes) == 180 == d["config"]["sources_per_step"] and len(sizes) == 2 and min(sizes) > 0
    assert d["config"]["catalog_gather_bytes_per_step"] == 2 * max(sizes) * 45 * 8
    pv = d["config"]["shard_pixel_visits"]
    assert abs(pv[0] - pv[1]) <= 0.1 * max(pv), "cost-balanced shards"
    fld = bench.build_field(420, 380, 180, 7)
    ctx = cel.FieldContext(fld.images, fld.patches, fld.neighbors)
    v, dd, h, cnt, st = ctx.eval_batch(fld.vp, np.arange(180), ALL)
    assert (st == 0).all()
    seen = np.zeros(180, dtype=bool)
    for r in range(2):
        z = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        assert np.array_equal(z["v"], v) and np.array_equal(z["d"], dd), "rank %d gathered catalog" % r
        assert np.array_equal(z["h"], h[z["mine"]]), "Hessians stay with the owner"
        seen[z["mine"]] = True
    assert seen.all()


def test_bench_plain_invocation_runs_two_ranks_by_itself(tmp_path):
    """`python bench.py --gpus 2 --backend gloo` with NO launcher and no RANK in the environment: bench.py starts its two
    ranks itself, the line says n_gpus 2 and ranks_seen 2, and both ranks hold the single-rank catalog bit for bit"""
    import celeste_jl_amd as cel
    sys.path.insert(0, ROOT)
    import bench
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--height", "420", "--width", "380",
           "--sources", "180", "--seed", "7", "--steps", "3", "--warmup", "1", "--full", "--check-dir", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_seen"] == 2 and d["config"]["gather_backend"] == "gloo"
    assert sum(d["config"]["shard_sizes"]) == 180 and len(d["config"]["shard_sizes"]) == 2
    per_rank = d["config"]["sweep_ms_without_gather_per_rank"]
    assert len(per_rank) == 2 and min(per_rank) > 0 and max(per_rank) <= d["ms_per_step"] * 1.5
    fld = bench.build_field(420, 380, 180, 7)
    ctx = cel.FieldContext(fld.images, fld.patches, fld.neighbors)
    v, dd, h, cnt, st = ctx.eval_batch(fld.vp, np.arange(180), ALL)
    for r in range(2):
        z = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        assert np.array_equal(z["v"], v) and np.array_equal(z["d"], dd), "rank %d gathered catalog" % r
    # RCCL cannot put two ranks on this box's one device: the plain form must refuse, not print a line for fewer ranks
    import torch
    if torch.cuda.device_count() < 2:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--height", "300", "--width", "260",
                              "--sources", "60", "--steps", "1", "--warmup", "0", "--no-extras"],
                             capture_output=True, text=True, timeout=900, env=env)
        assert out.returncode != 0 and not [ln for ln in out.stdout.splitlines() if ln.strip().startswith("{")]
        assert "RCCL needs one device per rank" in out.stderr


def test_bench_single_rank_under_the_launcher(tmp_path):
    """N = 1 launched the way the driver launches N > 1 (torch.distributed.run, RCCL group of one)"""
    d = _launch_bench(tmp_path, 1, ["--height", "300", "--width", "260", "--sources", "60", "--steps", "3", "--warmup", "1",
                                    "--no-extras"])
    assert d["n_gpus"] == 1 and d["config"]["shard_sizes"] == [60] and d["value"] > 0
    assert d["config"]["catalog_gather_bytes_per_step"] == 0


def test_bench_rccl_gather_path_on_a_group_of_one(tmp_path):
    """the device-side catalog gather exactly as N > 1 runs it -- RCCL all_gather_into_tensor on its own stream, two
    alternating blocks, events both ways -- on a process group of one rank (CELESTE_GATHER_SINGLE=1; RCCL refuses two
    ranks on one device, so this is as close as a one-GPU box gets): the gathered catalog is the host API's"""
    import celeste_jl_amd as cel
    sys.path.insert(0, ROOT)
    import bench
    shape = ["--height", "300", "--width", "260", "--sources", "60", "--seed", "9"]
    d = _launch_bench(tmp_path, 1, shape + ["--steps", "4", "--warmup", "2", "--no-extras", "--check-dir", str(tmp_path)],
                      CELESTE_GATHER_SINGLE="1")
    assert d["n_gpus"] == 1 and d["config"]["gather_backend"] == "nccl"
    assert d["config"]["catalog_gather_bytes_per_step"] == 60 * 45 * 8
    fld = bench.build_field(300, 260, 60, 9)
    ctx = cel.FieldContext(fld.images, fld.patches, fld.neighbors)
    v, dd, h, cnt, st = ctx.eval_batch(fld.vp, np.arange(60), ALL)
    z = np.load(os.path.join(str(tmp_path), "rank0.npz"))
    assert np.array_equal(z["v"], v) and np.array_equal(z["d"], dd) and np.array_equal(z["h"], h[z["mine"]])


def test_device_sharded_sweep_single_process_matches_host_api():
    import torch
    import celeste_jl_amd as cel
    from celeste_jl_amd import synthetic
    from celeste_jl_amd.parallel import DeviceShardedSweep
    from celeste_jl_amd.partition import estimate_time
    f = synthetic.make_field(200, 240, 40, seed=12)
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    tg = np.arange(40)
    sweep = DeviceShardedSweep(ctx, tg, [estimate_time(r) for r in f.patches], 0, 1, ALL)
    d_vp = torch.tensor(f.vp, dtype=torch.float64, device="cuda:0")
    for _ in range(3):     # alternating output blocks
        sweep.step(d_vp.data_ptr())
    v, d, st, cnt = sweep.results()
    rv, rd, rh, rcnt, rst = ctx.eval_batch(f.vp, tg, ALL)
    assert np.array_equal(v, rv) and np.array_equal(d, rd) and np.array_equal(sweep.hessians(), rh)
    assert np.array_equal(cnt, rcnt) and (st == 0).all()


def test_hundred_contexts_on_one_image_handle(oracle):
    """the reference's per-source ElboArgs over shared images (process_source, ParallelRun.jl:468-488): every context
    holds only its patch table; the planes are uploaded once"""
    if os.environ.get("PYTEST_XDIST_WORKER"):
        pytest.skip("free device memory is a property of the whole GPU: other test processes allocate beside this one (run without -n)")
    import celeste_jl_amd as cel
    from celeste_jl_amd import synthetic, cabi
    f = synthetic.make_field(1024, 900, 100, seed=31)
    whole = cel.FieldContext(f.images, f.patches, f.neighbors)
    rv, rd, rh, rcnt, _ = whole.eval_batch(f.vp, np.arange(100), ALL)
    iset = cabi.ImageSet(f.images)
    plane_bytes = sum(im.pixels.size for im in f.images) * (4 + 4)     # pixels + sky, f32
    # (closed contexts leave their streams in the library's pool -- up to 32, about 1 MB of device memory each: stream_retire,
    # celeste_abi.hip -- so the pool is filled before the baseline is taken and holds the same at the end)
    for c_ in [cel.FieldContext(f.images, [f.patches[0]], [[]], image_set=iset) for _ in range(17)]:
        c_.close()
    base = _free_device_bytes()
    ctxs = []
    for t in range(100):
        loc = [t] + list(f.neighbors[t])           # patches[[t; neighbors], :], active source first
        patches = [f.patches[s] for s in loc]
        nbrs = [list(range(1, len(loc)))] + [[] for _ in loc[1:]]
        ctxs.append((cel.FieldContext(f.images, patches, nbrs, image_set=iset), loc))
    used = base - _free_device_bytes()
    # a context costs its patch tables and scratch (a few MB), not a copy of the planes (37 MB here, 122 MB for an
    # SDSS-size field)
    assert used < 100 * 0.1 * plane_bytes, (used, plane_bytes)
    for t, (ctx, loc) in enumerate(ctxs):
        v, d, h, cnt, st = ctx.eval_batch(f.vp[loc], [0], ALL)
        assert st[0] == 0 and np.array_equal(cnt[0], rcnt[t])
        assert v[0] == rv[t] and np.array_equal(d[0], rd[t]) and np.array_equal(h[0], rh[t])
    # one of them against the oracle as well (the local problem is a complete problem of its own)
    ctx, loc = ctxs[17]
    iset_free_before = _free_device_bytes()
    iset.close()                                    # contexts keep the planes alive
    assert abs(_free_device_bytes() - iset_free_before) < (1 << 20)
    v, d, h, cnt, st = ctx.eval_batch(f.vp[loc], [0], ALL)
    pb = cabi.Problem(f.images, [f.patches[s] for s in loc], [list(range(1, len(loc)))] + [[] for _ in loc[1:]])
    ov, od, oh, ocnt, ost = oracle.elbo_batch(pb, f.vp[loc], [0], ALL)
    from parity_util import assert_parity
    assert_parity((v, d, h, cnt, st), (ov, od, oh, ocnt, ost), "context on a shared handle")
    for ctx, _ in ctxs:
        ctx.close()
    assert _free_device_bytes() >= base + int(0.9 * plane_bytes), "planes released with the last context"


def test_image_handle_argument_checks(lib):
    from celeste_jl_amd import synthetic, cabi
    import celeste_jl_amd as cel
    f = synthetic.make_sample_dataset("two_body")
    h = C.c_void_p()
    assert lib.celeste_images_create(0, None, 0, C.byref(h)) == cabi.ERR_INVALID_ARG
    assert lib.celeste_ctx_create_on(None, None, C.byref(h)) == cabi.ERR_INVALID_ARG
    iset = cabi.ImageSet(f.images)
    pb = cabi.Problem(f.images[:3], [row[:3] for row in f.patches], f.neighbors, marshal_images=False)
    assert lib.celeste_ctx_create_on(iset.handle, C.byref(pb.c), C.byref(h)) == cabi.ERR_INVALID_ARG   # 3 images != 5
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors, image_set=iset)
    ref = cel.FieldContext(f.images, f.patches, f.neighbors)
    a, b = ctx.eval_batch(f.vp, [0, 1], ALL), ref.eval_batch(f.vp, [0, 1], ALL)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_host_api_pinned_pageable_packed_and_parts():
    """celeste_elbo_eval_batch: outputs in page-locked or pageable memory, full or packed Hessians, one part or
    several -- the same bits; the packed layout is the column-wise upper triangle"""
    import celeste_jl_amd as cel
    from celeste_jl_amd import synthetic, cabi
    f = synthetic.make_field(512, 512, 420, seed=77)      # > 2 x 192 targets: the batch is cut into parts
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    tg = np.random.default_rng(3).permutation(420)
    a = ctx.eval_batch(f.vp, tg, ALL, pinned=True)
    b = ctx.eval_batch(f.vp, tg, ALL, pinned=False)
    assert (a[4] == 0).all()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    singles = [ctx.eval_batch(f.vp, [int(t)], ALL) for t in tg[[0, 5, 200, 419]]]
    for k, t in enumerate([0, 5, 200, 419]):
        assert singles[k][0][0] == a[0][t] and np.array_equal(singles[k][2][0], a[2][t])
    for pinned in (True, False):
        p = ctx.eval_batch(f.vp, tg, ALL | cabi.FLAG_PACKED_HESS, pinned=pinned)
        assert p[2].shape == (420, cabi.HP)
        assert np.array_equal(p[0], a[0]) and np.array_equal(p[1], a[1]) and np.array_equal(p[3], a[3])
        assert np.array_equal(cabi.unpack_hessian(p[2]), a[2])
    assert a[2][3][2, 7] == p[2][3][7 * 8 // 2 + 2]       # element (i, j), i <= j, at j (j + 1) / 2 + i
    # caller-registered memory (celeste_host_register) behaves like celeste_host_alloc memory
    h = np.zeros((420, 44, 44))
    assert ctx.lib.celeste_host_register(h.ctypes.data_as(C.c_void_p), h.nbytes) == 0
    v = np.zeros(420); d = np.zeros((420, 44)); cnt = np.zeros((420, 2), dtype=np.int64); st = np.zeros(420, dtype=np.int32)
    vp = np.ascontiguousarray(f.vp); t32 = np.ascontiguousarray(tg, dtype=np.int32)
    dp = cabi.c_double_p
    rc = ctx.lib.celeste_elbo_eval_batch(ctx.handle, vp.ctypes.data_as(dp), 420, t32.ctypes.data_as(cabi.c_int32_p), ALL,
                                         v.ctypes.data_as(dp), d.ctypes.data_as(dp), h.ctypes.data_as(dp),
                                         cnt.ctypes.data_as(cabi.c_int64_p), st.ctypes.data_as(cabi.c_int32_p))
    assert rc == 0 and np.array_equal(h, a[2]) and np.array_equal(v, a[0])
    assert ctx.lib.celeste_host_unregister(h.ctypes.data_as(C.c_void_p)) == 0
    # pinned arrays are recycled through the pool without aliasing live results
    keep = a[2].copy()
    del p
    c = ctx.eval_batch(f.vp, tg[::-1].copy(), ALL)
    assert np.array_equal(a[2], keep) and np.array_equal(c[2][::-1], a[2])


def test_optimiser_refuses_duplicate_targets_and_survives_a_failing_target():
    import celeste_jl_amd as cel
    from celeste_jl_amd import synthetic, cabi
    f = synthetic.make_field(160, 200, 24, seed=11)
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    with pytest.raises(cabi.CelesteError) as e:
        ctx.maximize_batch(f.vp, [3, 5, 3], cel.ElboConfig(max_iters=2))
    assert e.value.status == cabi.ERR_INVALID_ARG
    # a neighbour with a non-finite parameter: every target that lists it fails (non-finite result), keeps its row,
    # and the rest of the batch is optimised exactly as it would be alone
    bad = int(np.argmax([len(n) for n in f.neighbors]))
    hit = set(f.neighbors[bad])
    targets = [t for t in range(24) if t != bad]
    nb = f.vp.copy(); nb[bad, 7] = np.nan
    cfg = cel.ElboConfig(max_iters=4)
    with pytest.raises(AssertionError):
        ctx.maximize_batch(f.vp, targets, cfg, vp_neighbors=nb)
    vp, its, evals, el, st = ctx.maximize_batch(f.vp, targets, cfg, vp_neighbors=nb, raise_on_error=False)
    ok = [k for k, t in enumerate(targets) if t not in hit]
    ko = [k for k, t in enumerate(targets) if t in hit]
    assert len(ko) > 0 and len(ok) > 0
    assert np.isin(st[ko], (cabi.ERR_NONFINITE_INPUT, cabi.ERR_NONFINITE_RESULT)).all() and (st[ok] == 0).all()
    for k in ko:
        assert np.array_equal(vp[targets[k]], f.vp[targets[k]]), "a failed target keeps its input row"
    good_targets = [targets[k] for k in ok]
    vp2, its2, _, el2, st2 = ctx.maximize_batch(f.vp, good_targets, cfg)
    assert (st2 == 0).all() and np.array_equal(vp2[good_targets], vp[good_targets]) and np.array_equal(el2, el[ok])
    # the node-level loop logs and skips instead of raising
    from celeste_jl_amd.infer import one_node_single_infer
    failed = set()

    class BadNeighbour:   # the same context, with one catalogued neighbour turned non-finite on the way in
        def maximize_batch(self, vp, tg, cfg=None, vp_neighbors=None, **kw):
            nbrs = np.array(vp_neighbors, dtype=np.float64, copy=True)
            nbrs[bad, 7] = np.nan
            return ctx.maximize_batch(vp, tg, cfg, vp_neighbors=nbrs, **kw)
    vs = one_node_single_infer(BadNeighbour(), f.catalog, targets, cfg, failed=failed)
    assert failed == hit & set(targets) and np.isfinite(vs).all()
    vs_ok = one_node_single_infer(ctx, f.catalog, good_targets, cfg)
    assert np.array_equal(vs[ok], vs_ok)


def test_optimiser_initial_gradient_check_and_secular_cap(oracle):
    """the two Optim.jl details ADVICE r1 asked for: the g_tol test at the starting point, and the cap of the
    multiplier iterations (tr_secular_iters = 5 is Optim's); device and CPU restatement agree in both modes"""
    import celeste_jl_amd as cel
    from celeste_jl_amd import synthetic
    f = synthetic.make_sample_dataset("galaxy")
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    # a gradient tolerance larger than any gradient: converged before the first iteration, one evaluation
    vp, its, evals, el, st = ctx.maximize_batch(f.vp, [0], cel.ElboConfig(gtol=1e30))
    assert its[0] == 0 and evals[0] == 1 and st[0] == 0
    o = oracle.maximize(ctx.problem, f.vp, 0, oracle.OptCfg(gtol=1e30))
    assert o[1] == 0 and o[2] == 1 and abs(o[3] - el[0]) <= 1e-9 * abs(el[0])
    for cap in (5, 0):
        vp, its, evals, el, st = ctx.maximize_batch(f.vp, [0], cel.ElboConfig(max_iters=8, tr_secular_iters=cap))
        o = oracle.maximize(ctx.problem, f.vp, 0, oracle.OptCfg(max_iters=8, tr_secular_iters=cap))
        assert st[0] == 0 and its[0] == o[1] and evals[0] == o[2]
        assert np.max(np.abs(vp[0] - o[0][0]) / np.maximum(np.abs(o[0][0]), 1e-3)) <= 1e-6, cap


def test_variable_sky_calibration_and_psf_map_on_the_device(oracle):
    """SURVEY.md 8(f) row 3 on the device, trap A2 / A4: an SDSSBackground sky plane, a per-row calibration and an
    SDSSPSFMap with 3 eigen-images (every patch its own spline) through the fused, split, fp32, gradient-only and
    multi-active paths against the oracle (SDSSIO.jl:56-99, 239-299; elbo_objective.jl:374-385)"""
    import celeste_jl_amd as cel
    from celeste_jl_amd import synthetic, cabi
    from parity_util import assert_fp32_parity, assert_parity, rel_err
    f = synthetic.make_field(300, 340, 60, seed=41, variable=True, nan_fraction=0.005)
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    assert ctx.problem.c.n_stamps > 200
    tg = list(range(60))
    ref = oracle.elbo_batch(ctx.problem, f.vp, tg, ALL)
    print("fused", assert_parity(ctx.eval_batch(f.vp, tg, ALL), ref, "variable field"))
    print("split", assert_parity(ctx.eval_batch(f.vp, tg, ALL | cabi.FLAG_SPLIT), ref, "variable field, split"))
    v32, d32, h32, c32, s32 = ctx.eval_batch(f.vp, tg, ALL | cabi.FLAG_FP32)
    assert np.array_equal(c32, ref[3]) and np.max(np.abs(v32 - ref[0]) / np.abs(ref[0])) <= 1e-4
    # (the fp32 mode's stated tolerance is norm-scaled: SURVEY.md 8(d) config 5, "1e-4 relative on v and on |d|_inf-scaled d")
    assert max(np.abs(d32[t] - ref[1][t]).max() / np.abs(ref[1][t]).max() for t in tg) <= 1e-4
    assert max(np.abs(h32[t] - ref[2][t]).max() / np.abs(ref[2][t]).max() for t in tg) <= 1e-4
    assert_fp32_parity((v32, d32, h32), ref, ref[2], "variable field, fp32")
    g = ctx.eval_batch(f.vp, tg, 1 | 4)
    assert np.max(np.abs(g[0] - ref[0]) / np.abs(ref[0])) <= 1e-8 and max(rel_err(g[1][t], ref[1][t]) for t in tg) <= 1e-8
    # two overlapping active sources (Sa = 2) on the same planes
    a = int(np.argmax([len(n) for n in f.neighbors])); b = f.neighbors[a][0]
    loc = sorted(set([a, b] + list(f.neighbors[a]) + list(f.neighbors[b])))
    ia, ib = loc.index(a), loc.index(b)
    patches = [f.patches[s] for s in loc]
    nbrs = [[j for j in range(len(loc)) if j != i] if i in (ia, ib) else [] for i in range(len(loc))]
    mctx = cel.FieldContext(f.images, patches, nbrs)
    mv, md, mh, mcnt = mctx.eval_multi(f.vp[loc], [ia, ib], ALL)
    ov, od, oh, ocnt, ost = oracle.elbo_multi(mctx.problem, f.vp[loc], [ia, ib], ALL)
    assert ost == 0 and np.array_equal(mcnt, ocnt) and abs(mv - ov) <= 1e-8 * abs(ov)
    assert rel_err(md.T, od) <= 1e-8 and rel_err(mh, oh) <= 1e-8
    # the optimiser runs on these planes as well (a few iterations against the CPU restatement)
    vp, its, _, el, st = ctx.maximize_batch(f.vp, [a], cel.ElboConfig(max_iters=6))
    o = oracle.maximize(ctx.problem, f.vp, a, oracle.OptCfg(max_iters=6))
    assert st[0] == 0 and its[0] == o[1] and abs(el[0] - o[3]) <= 1e-9 * abs(o[3])


def test_joint_inference_on_the_device_equals_the_cpu_restatement(oracle):
    """the joint-inference schedule (Cyclades batches, components processed source by source,
    position boxes pinned at the initial positions, ParallelRun.jl:135-196, 302-397) driven once by the device
    optimiser and once by the CPU restatement of maximize!: the shared parameter table must come out the same --
    every layer's result feeds the next layers, so this checks the whole chain, not single optimisations"""
    # (eval_batch below evaluates each target's ELBO with its neighbours at the table's values)
    import celeste_jl_amd as cel
    from celeste_jl_amd import synthetic
    from celeste_jl_amd.infer import joint_infer_sweeps
    from celeste_jl_amd.params import catalog_init_source, generic_init_source
    f = synthetic.make_field(110, 120, 12, seed=19, margin=30)       # crowded: every source has neighbours
    assert min(len(n) for n in f.neighbors) >= 2
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    targets = [0, 1, 2, 4, 5, 7, 8, 9, 11]                           # three sources stay frozen neighbours
    vp0 = np.stack([catalog_init_source(ce) for ce in f.catalog])
    for t in targets:
        vp0[t] = generic_init_source(f.catalog[t].pos)
    frozen = [s for s in range(12) if s not in targets]

    def run(max_iters):
        cfg_kw = dict(max_iters=max_iters)
        calls = {"dev": 0, "cpu": 0}

        def layer_dev(vp, layer, pc):
            calls["dev"] += 1
            new, _, _, _, st = ctx.maximize_batch(vp, layer, cel.ElboConfig(**cfg_kw), pos_centers=pc)
            assert (st == 0).all()
            return new[layer]

        def layer_cpu(vp, layer, pc):
            calls["cpu"] += 1
            rows = []
            for t, c in zip(layer, pc):
                r = oracle.maximize(ctx.problem, vp, t, oracle.OptCfg(**cfg_kw), pos_center=c)
                assert r[4] == 0
                rows.append(r[0][t])
            return np.stack(rows)
        out = {}
        for name, fn in (("dev", layer_dev), ("cpu", layer_cpu)):
            out[name] = joint_infer_sweeps(fn, vp0.copy(), targets, f.neighbors, batch_size=5, n_iters=2,
                                           rng=np.random.default_rng(3))
        assert calls["dev"] == calls["cpu"] > 4
        moved = np.abs(out["cpu"][targets] - vp0[targets]).max()
        err = np.abs(out["dev"] - out["cpu"]) / np.maximum(np.abs(out["cpu"]), 1e-3)
        absdiff = np.abs(out["dev"] - out["cpu"])
        worst = np.unravel_index(np.argmax(absdiff), absdiff.shape)
        print("joint inference, 2 sweeps, %d layers, max_iters %d: max |device - CPU| %.2e (source %d parameter %d), median "
              "relative %.1e; parameters moved by up to %.2g" % (calls["dev"], max_iters, absdiff.max(), worst[0], worst[1],
                                                               np.median(err[targets]), moved))
        assert moved > 0.1 and np.array_equal(out["dev"][frozen], vp0[frozen])
        return out, absdiff.max(), np.median(err[targets])

    # (a) the bar of test_randomised_optimiser_against_cpu -- every parameter within 1e-6 -- while the trust-region
    # sub-problems are well conditioned (the first Newton iterations of every layer)
    _, absdiff, med = run(3)
    assert absdiff <= 1e-6 and med <= 1e-9, (absdiff, med)
    # (b) six iterations per layer: some late sub-problems sit next to the hard case (smallest eigenvalue of
    # H + lambda I ~1e-8 of the largest), where rounding-level differences between two eigen-solvers move the step by
    # ~1e-9 and the following iterations amplify that ~1000x each along flat directions (tools/diag_joint.py prints it
    # layer by layer: 1e-12 after four iterations, 1e-7 .. 1e-6 after six).  Measured 9.5e-7; besides the parameters,
    # what must agree is what the optimiser is for: the objective reached.
    out, absdiff, med = run(6)
    tg = np.array(targets, dtype=np.int32)
    e_dev = ctx.eval_batch(out["dev"], tg, 4)[0]
    e_cpu = ctx.eval_batch(out["cpu"], tg, 4)[0]
    rel = np.abs(e_dev - e_cpu) / np.abs(e_cpu)
    print("    ELBO reached, device vs CPU tables: max relative difference %.1e" % rel.max())
    assert absdiff <= 2e-6 and med <= 1e-9 and rel.max() <= 1e-9, (absdiff, med, rel.max())


def test_repeated_device_launches_track_the_parameters():
    """celeste_elbo_eval_batch_device called again and again with the same pointers (an evaluation loop over a resident
    parameter table): every launch must see the CURRENT contents of the parameter table and of the target list, also
    after a larger batch through the same context has moved the scratch buffers"""
    import torch
    import celeste_jl_amd as cel
    from celeste_jl_amd import synthetic
    f = synthetic.make_field(256, 300, 70, seed=23)
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    dev = torch.device("cuda:0")
    n = 40
    d_vp = torch.tensor(f.vp, dtype=torch.float64, device=dev)
    d_tg = torch.arange(n, dtype=torch.int32, device=dev)
    d_v = torch.zeros(n, dtype=torch.float64, device=dev); d_d = torch.zeros(n, 44, dtype=torch.float64, device=dev)
    d_h = torch.zeros(n, 44, 44, dtype=torch.float64, device=dev)
    d_c = torch.zeros(n, 2, dtype=torch.int64, device=dev); d_s = torch.zeros(n, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def launch():
        ctx.eval_batch_device(d_vp.data_ptr(), n, d_tg.data_ptr(), ALL, d_v.data_ptr(), d_d.data_ptr(), d_h.data_ptr(),
                              d_c.data_ptr(), d_s.data_ptr(), stream)
        torch.cuda.synchronize(dev)
        return d_v.cpu().numpy(), d_d.cpu().numpy(), d_h.cpu().numpy()
    rng = np.random.default_rng(1)
    vp = f.vp.copy()
    for it in range(6):
        if it == 3:                         # same pointers, new targets
            d_tg.copy_(torch.arange(20, 20 + n, dtype=torch.int32, device=dev))
        if it == 4:                         # a larger batch through the same context moves the scratch buffers
            ctx.eval_batch(vp, np.arange(70), ALL)
        vp[:, 6:8] += 0.01 * rng.normal(size=(70, 2))
        d_vp.copy_(torch.tensor(vp, dtype=torch.float64, device=dev))
        got = launch()
        tg = d_tg.cpu().numpy()
        ref = ctx.eval_batch(vp, tg, ALL)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]), it
    # repeated targets: the work list is longer than the grid the host can bound without knowing the targets (the
    # chunks of the n chunk-richest sources) -- the pixel kernel's stride loop covers the rest
    big = int(np.argmax([sum(p.active_pixel_bitmap.size for p in row) for row in f.patches]))
    d_tg.copy_(torch.full((n,), big, dtype=torch.int32, device=dev))
    got = launch()
    ref = ctx.eval_batch(vp, [big], ALL)
    assert (got[0] == ref[0][0]).all() and (got[2] == ref[2][0]).all()
