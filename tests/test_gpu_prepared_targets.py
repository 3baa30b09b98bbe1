"""-m gpu: prepared target lists (celeste_targets_t) against the unprepared device entry, bit for bit.

What a sweep derives from its targets alone -- work list, record offsets, visit items, target marks, the tables to fill and
the neighbour items to render -- is made once per list instead of once per sweep; the kernels that do the arithmetic are
the same and see the same records in the same order.  So every comparison here is np.array_equal against
celeste_elbo_eval_batch_device on the same context and vp, over v, d, h, counters and status.  Every case has more than 32
targets or sets CELESTE_EVAL_FUSED=0, so that the pixel + lift path runs (except the one that is about small batches)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 44
ALL = 1 | 2 | 4


@pytest.fixture(scope="module")
def dense():
    import celeste_jl_amd as cel
    from celeste_jl_amd import synthetic
    f = synthetic.make_field(160, 200, 40, seed=11, nan_fraction=0.005)
    assert sum(len(n) for n in f.neighbors) > 0
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    yield f, ctx
    ctx.close()


@pytest.fixture(scope="module")
def sparse():
    import celeste_jl_amd as cel
    from celeste_jl_amd import synthetic
    f = synthetic.make_multifield((2, 3), 160, 160, 0.10, 70, seed=11, sparse=True)
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    yield f, ctx
    ctx.close()


def _perturbed(vp, seed):
    """another parameter table: every unconstrained-looking entry moved a little (positions by a fraction of a pixel)"""
    rng = np.random.default_rng(seed)
    out = np.array(vp, dtype=np.float64).reshape(-1, P).copy()
    out[:, 0:2] += rng.uniform(-0.3, 0.3, (out.shape[0], 2))
    out[:, 5] *= rng.uniform(0.9, 1.1, out.shape[0])
    return out


class _Outputs:
    """device outputs of one call, pre-filled with sentinels so that an entry a call does not write compares equal only
    if neither call wrote it"""

    def __init__(self, torch, dev, n, flags):
        self.v = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
        self.d = torch.full((n, P), -7.0, dtype=torch.float64, device=dev) if flags & 3 else None
        self.h = torch.full((n, P, P), -7.0, dtype=torch.float64, device=dev) if flags & 2 else None
        self.cnt = torch.full((n, 2), -7, dtype=torch.int64, device=dev)
        self.st = torch.full((n,), -7, dtype=torch.int32, device=dev)

    def ptrs(self):
        return (self.v.data_ptr(), self.d.data_ptr() if self.d is not None else 0,
                self.h.data_ptr() if self.h is not None else 0, self.cnt.data_ptr(), self.st.data_ptr())

    def host(self):
        return tuple(None if t is None else t.cpu().numpy() for t in (self.v, self.d, self.h, self.cnt, self.st))


def _device(ctx):
    import torch
    return torch, torch.device("cuda", ctx.device)


def _unprepared(ctx, vp, targets, flags):
    """celeste_elbo_eval_batch_device itself (not FieldContext.eval_batch_device, which looks registered lists up)"""
    from celeste_jl_amd import cabi
    torch, dev = _device(ctx)
    d_vp = torch.tensor(np.ascontiguousarray(vp, dtype=np.float64).reshape(ctx.S, P), device=dev)
    d_tg = torch.tensor(np.asarray(targets, dtype=np.int32), device=dev)
    out = _Outputs(torch, dev, len(targets), flags)
    torch.cuda.synchronize(dev)
    cabi.check(ctx.lib.celeste_elbo_eval_batch_device(ctx.handle, d_vp.data_ptr(), len(targets), d_tg.data_ptr(), flags,
                                                      *out.ptrs(), 0), ctx.lib)
    torch.cuda.synchronize(dev)
    return out.host()


class _List:
    """a prepared list made from a host array through celeste_targets_create"""

    def __init__(self, ctx, targets):
        from celeste_jl_amd import cabi
        self.ctx, self.n = ctx, len(targets)
        tg = np.ascontiguousarray(np.asarray(targets, dtype=np.int32))
        self.h = C.c_void_p()
        cabi.check(ctx.lib.celeste_targets_create(ctx.handle, tg.size, tg.ctypes.data_as(cabi.c_int32_p), C.byref(self.h)), ctx.lib)
        tg[:] = 0                       # the library has its own copy

    def eval(self, vp, flags):
        ctx = self.ctx
        torch, dev = _device(ctx)
        d_vp = torch.tensor(np.ascontiguousarray(vp, dtype=np.float64).reshape(ctx.S, P), device=dev)
        out = _Outputs(torch, dev, self.n, flags)
        torch.cuda.synchronize(dev)
        ctx.eval_targets_device(self.h, d_vp.data_ptr(), flags, *out.ptrs(), 0)
        torch.cuda.synchronize(dev)
        return out.host()

    def close(self):
        if self.h:
            self.ctx.lib.celeste_targets_destroy(self.h)
            self.h = None


def _same(a, b, what):
    for x, y, name in zip(a, b, ("v", "d", "h", "counters", "status")):
        if x is None and y is None:
            continue
        assert np.array_equal(x, y, equal_nan=True), "%s: %s differs" % (what, name)


def _check(ctx, vp, targets, flags, what):
    ref = _unprepared(ctx, vp, targets, flags)
    assert (ref[4] == 0).all(), what
    lst = _List(ctx, targets)
    try:
        _same(ref, lst.eval(vp, flags), what)
    finally:
        lst.close()


@pytest.mark.parametrize("flags", [ALL, 1, 3], ids=["flags7", "flags1", "flags3"])
def test_every_source_as_target(dense, flags):
    f, ctx = dense
    _check(ctx, f.vp, list(range(ctx.S)), flags, "all sources, flags %d" % flags)


def test_single_precision_runs_the_unprepared_path_on_the_lists_targets(dense):
    """lists are made for the fp64 chunks (the header says so): an fp32 call is served by the unprepared path"""
    from celeste_jl_amd import cabi
    f, ctx = dense
    _check(ctx, f.vp, list(range(ctx.S)), ALL | cabi.FLAG_FP32, "fp32")


def test_strict_subset_whose_neighbours_lie_outside_it(dense, monkeypatch):
    """the compact table and value lists must cover the neighbours that are no targets"""
    monkeypatch.setenv("CELESTE_EVAL_FUSED", "0")
    f, ctx = dense
    tg = list(range(1, ctx.S, 3))
    inside = set(tg)
    assert any(q not in inside for t in tg for q in f.neighbors[t])
    _check(ctx, f.vp, tg, ALL, "subset")
    _check(ctx, f.vp, tg[::-1], 1, "subset, reversed, gradient only")


def test_repeated_entry(dense):
    f, ctx = dense
    _check(ctx, f.vp, list(range(ctx.S)) + [3, 3, 17], ALL, "repeated targets")


def test_sparse_context(sparse):
    """a source with no patch in some image: items entries of -1"""
    f, ctx = sparse
    assert ctx.problem.sparse
    per_source = np.bincount(ctx.problem.patch_source, minlength=ctx.S)
    assert per_source.min() < per_source.max()
    _check(ctx, f.vp, list(range(ctx.S)), ALL, "sparse, all sources")
    _check(ctx, f.vp, list(range(0, ctx.S, 2)) + [5], 1, "sparse, subset")


def test_nothing_that_depends_on_vp_is_cached(dense):
    f, ctx = dense
    tg = list(range(ctx.S))
    vp2 = _perturbed(f.vp, 3)
    lst = _List(ctx, tg)
    try:
        _same(_unprepared(ctx, f.vp, tg, ALL), lst.eval(f.vp, ALL), "first vp")
        ref2 = _unprepared(ctx, vp2, tg, ALL)
        assert not np.array_equal(ref2[0], _unprepared(ctx, f.vp, tg, ALL)[0])
        _same(ref2, lst.eval(vp2, ALL), "second vp")
    finally:
        lst.close()


def test_an_unprepared_call_in_between_leaves_the_list_intact(dense):
    f, ctx = dense
    tg = list(range(ctx.S))
    lst = _List(ctx, tg)
    try:
        first = lst.eval(f.vp, ALL)
        _unprepared(ctx, _perturbed(f.vp, 5), list(range(ctx.S - 1, 2, -1)), ALL)
        _same(first, lst.eval(f.vp, ALL), "prepared, unprepared with other targets, prepared")
        _same(first, _unprepared(ctx, f.vp, tg, ALL), "against the unprepared call")
    finally:
        lst.close()


def test_two_lists_alive_on_one_context(dense):
    f, ctx = dense
    ta, tb = list(range(ctx.S)), list(range(ctx.S - 1, -1, -1))[:35]
    ra, rb = _unprepared(ctx, f.vp, ta, ALL), _unprepared(ctx, f.vp, tb, ALL)
    la, lb = _List(ctx, ta), _List(ctx, tb)
    try:
        for k in range(2):
            _same(ra, la.eval(f.vp, ALL), "list a, round %d" % k)
            _same(rb, lb.eval(f.vp, ALL), "list b, round %d" % k)
    finally:
        la.close()
        lb.close()


def test_small_batch_whichever_path_serves_it(dense):
    f, ctx = dense
    _check(ctx, f.vp, [7, 3, 21, 0, 39], ALL, "5 targets")
    _check(ctx, f.vp, [7, 3, 21, 0, 39], 1, "5 targets, gradient only")


def test_handle_of_another_context_is_refused(dense):
    import celeste_jl_amd as cel
    from celeste_jl_amd import cabi
    f, ctx = dense
    other = cel.FieldContext(f.images, f.patches, f.neighbors)
    lst = _List(ctx, list(range(ctx.S)))
    try:
        torch, dev = _device(ctx)
        d_vp = torch.tensor(np.ascontiguousarray(f.vp, dtype=np.float64).reshape(ctx.S, P), device=dev)
        out = _Outputs(torch, dev, lst.n, ALL)
        st = ctx.lib.celeste_elbo_eval_targets_device(other.handle, lst.h, d_vp.data_ptr(), ALL, *out.ptrs(), 0)
        assert st == cabi.ERR_INVALID_ARG
        torch.cuda.synchronize(dev)
        assert (out.host()[4] == -7).all()          # nothing ran
        # an out-of-range target never becomes a list
        bad = np.array([0, ctx.S], dtype=np.int32)
        h = C.c_void_p()
        assert ctx.lib.celeste_targets_create(ctx.handle, 2, bad.ctypes.data_as(cabi.c_int32_p), C.byref(h)) == cabi.ERR_INVALID_ARG
        assert not h.value
    finally:
        lst.close()
        other.close()


def _free_device_bytes():
    free, total = C.c_size_t(), C.c_size_t()
    assert C.CDLL("libamdhip64.so").hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_hundred_lists_created_and_destroyed_release_their_memory(dense):
    if os.environ.get("PYTEST_XDIST_WORKER"):
        pytest.skip("free device memory is a property of the whole GPU: other test processes allocate beside this one (run without -n)")
    import celeste_jl_amd as cel
    f, ctx = dense
    tg = list(range(ctx.S))
    _List(ctx, tg).close()
    base = _free_device_bytes()
    lists = [_List(ctx, tg[k % 5:]) for k in range(100)]
    assert _free_device_bytes() < base
    for lst in lists:
        lst.close()
    assert abs(_free_device_bytes() - base) < (1 << 20)
    # ... and a context that is destroyed frees the lists still alive on it
    # (a closed context leaves its streams in the library's pool: one is put there before the baseline is taken)
    cel.FieldContext(f.images, f.patches, f.neighbors).close()
    base = _free_device_bytes()
    own = cel.FieldContext(f.images, f.patches, f.neighbors)
    kept = [_List(own, tg) for _ in range(100)]
    assert len(kept) == 100 and _free_device_bytes() < base
    own.close()
    assert abs(_free_device_bytes() - base) < (1 << 20)


def test_no_prepared_switch_gives_equal_results(dense, monkeypatch):
    f, ctx = dense
    tg = list(range(ctx.S))
    ref = _unprepared(ctx, f.vp, tg, ALL)
    lst = _List(ctx, tg)
    try:
        monkeypatch.setenv("CELESTE_NO_PREPARED", "1")
        _same(ref, lst.eval(f.vp, ALL), "CELESTE_NO_PREPARED=1")
        monkeypatch.delenv("CELESTE_NO_PREPARED")
        _same(ref, lst.eval(f.vp, ALL), "default")
    finally:
        lst.close()


def test_first_call_on_a_fresh_context_is_a_prepared_one(dense):
    """nothing an earlier unprepared call left in the context (SrcGeo, tables, neighbour light, scratch) is relied on: the
    reference comes from another context over the same problem"""
    import celeste_jl_amd as cel
    f, ctx = dense
    tg = list(range(1, ctx.S))
    ref = _unprepared(ctx, f.vp, tg, ALL)
    fresh = cel.FieldContext(f.images, f.patches, f.neighbors)
    lst = _List(fresh, tg)
    try:
        _same(ref, lst.eval(f.vp, ALL), "first call of a fresh context")
    finally:
        lst.close()
        fresh.close()


def test_sharded_sweep_steps_equal_the_unregistered_entry(dense):
    from celeste_jl_amd.parallel import DeviceShardedSweep
    f, ctx = dense
    torch, dev = _device(ctx)
    tg = list(range(ctx.S))
    costs = [sum(int(p.active_pixel_bitmap.size) for p in f.patches[t]) for t in tg]
    sweep = DeviceShardedSweep(ctx, tg, costs, 0, 1, ALL)
    assert (sweep.d_tg.data_ptr(), sweep.n) in ctx._prepared
    for k, vp in enumerate((f.vp, _perturbed(f.vp, 9))):
        d_vp = torch.tensor(np.ascontiguousarray(vp, dtype=np.float64).reshape(ctx.S, P), device=dev)
        torch.cuda.synchronize(dev)
        sweep.step(d_vp.data_ptr())
        v, d, st, cnt = sweep.results()
        h = sweep.hessians()
        rv, rd, rh, rcnt, rst = _unprepared(ctx, vp, list(sweep.mine), ALL)
        order = np.asarray(sweep.shards[0])
        assert np.array_equal(v[order], rv) and np.array_equal(d[order], rd), "step %d" % k
        assert np.array_equal(h, rh) and np.array_equal(cnt, rcnt) and np.array_equal(st, rst), "step %d" % k
    sweep.close()
    assert not ctx._prepared


@pytest.mark.timeout(600, method="thread")
def test_group_sweep_on_two_members_sharing_one_device(dense):
    from celeste_jl_amd.group import FieldGroup
    f, _ = dense
    g = FieldGroup(f.images, f.patches, f.neighbors, devices=[0, 0])
    try:
        S = len(f.catalog)
        for what, vp, tg, flags in (("every source twice", f.vp, list(range(S)) * 2, ALL),
                                    ("another table, gradient only", _perturbed(f.vp, 13), list(range(S)) + [4, 4], 1)):
            ref = g.eval_batch(vp, tg, flags)
            g.plan(vp, tg, flags)
            for _ in range(2):
                g.sweep()
            g.wait()
            got = g.results()
            _same(ref, got, what)
    finally:
        g.close()
