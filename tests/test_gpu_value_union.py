"""-m gpu: a prepared sweep renders each neighbour pixel once (value_union_kernel over the list's own pixel set,
csrc/value_union.h) instead of once per link -- against the unprepared device entry and against the per-link items
(CELESTE_NO_VALUE_UNION=1), bit for bit over v, d, h, counters and status.

The scene is the one of test_gpu_prepared_targets.py.  Its geometry, counted on the CPU: 59 187 neighbour pixels are wanted
by more than one target; 67 unions are over 256 pixels and no multiple of 64 (items are split, last trips are partly
empty); with targets 0..19, 84 rendered (source, image) pairs belong to sources that are no targets.  40 targets would only
ever take the four-wavefront form of the kernel, so every list also runs under CELESTE_NO_WIDE_VALUE=1: the one-wavefront
items are what a 2000-target sweep runs.

Before every prepared call an unprepared sweep with ANOTHER parameter table overwrites the neighbours' light, so a pixel
the prepared call failed to render would hold a wrong value, not the reference's."""
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
    rng = np.random.default_rng(seed)
    out = np.array(vp, dtype=np.float64).reshape(-1, P).copy()
    out[:, 0:2] += rng.uniform(-0.3, 0.3, (out.shape[0], 2))
    out[:, 5] *= rng.uniform(0.9, 1.1, out.shape[0])
    return out


class _Outputs:
    """device outputs of one call, pre-filled with sentinels"""

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
    """celeste_elbo_eval_batch_device itself"""
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


def _stale_light(ctx, vp):
    """every neighbour pixel any link renders now holds the light of another parameter table"""
    _unprepared(ctx, _perturbed(vp, 101), list(range(ctx.S)), 1)


def _check(ctx, vp, targets, flags, what, monkeypatch):
    """union == unprepared, and union == per-link items on the same list"""
    ref = _unprepared(ctx, vp, targets, flags)
    assert (ref[4] == 0).all(), what
    lst = _List(ctx, targets)
    try:
        _stale_light(ctx, vp)
        got = lst.eval(vp, flags)
        _same(ref, got, what + ": against the unprepared entry")
        _stale_light(ctx, vp)
        monkeypatch.setenv("CELESTE_NO_VALUE_UNION", "1")
        per_link = lst.eval(vp, flags)
        monkeypatch.delenv("CELESTE_NO_VALUE_UNION")
        _same(per_link, got, what + ": against CELESTE_NO_VALUE_UNION=1")
    finally:
        lst.close()


def _lists(S):
    return {"all": list(range(S)), "first20": list(range(20)), "repeated": list(range(S)) + [3, 3, 17]}


@pytest.mark.parametrize("narrow", [False, True], ids=["wide", "one_wavefront"])
@pytest.mark.parametrize("which", ["all", "first20", "repeated"])
@pytest.mark.parametrize("flags", [ALL, 1, 3], ids=["flags7", "flags1", "flags3"])
def test_union_equals_per_link_rendering(dense, monkeypatch, flags, which, narrow):
    # (20 targets: the pixel + lift path, not eval_fused_kernel, which prepared lists do not serve)
    monkeypatch.setenv("CELESTE_EVAL_FUSED", "0")
    if narrow:
        monkeypatch.setenv("CELESTE_NO_WIDE_VALUE", "1")
    f, ctx = dense
    tg = _lists(ctx.S)[which]
    if which == "first20":
        inside = set(tg)
        assert any(q not in inside for t in tg for q in f.neighbors[t])     # rendered sources that are no targets
    _check(ctx, f.vp, tg, flags, "%s, flags %d, %s" % (which, flags, "one wavefront" if narrow else "wide"), monkeypatch)


@pytest.mark.parametrize("narrow", [False, True], ids=["wide", "one_wavefront"])
def test_sparse_context(sparse, monkeypatch, narrow):
    """a source with no patch in some image: its neighbours' visits come from the visit lists"""
    if narrow:
        monkeypatch.setenv("CELESTE_NO_WIDE_VALUE", "1")
    f, ctx = sparse
    assert ctx.problem.sparse
    _check(ctx, f.vp, list(range(ctx.S)), ALL, "sparse, all sources", monkeypatch)
    _check(ctx, f.vp, list(range(0, ctx.S, 2)) + [5], 1, "sparse, subset", monkeypatch)


def test_two_sweeps_with_different_vp(dense, monkeypatch):
    """the pixel set is cached, nothing that depends on the parameters is"""
    monkeypatch.setenv("CELESTE_NO_WIDE_VALUE", "1")
    f, ctx = dense
    tg = list(range(ctx.S))
    vp2 = _perturbed(f.vp, 3)
    ref1, ref2 = _unprepared(ctx, f.vp, tg, ALL), _unprepared(ctx, vp2, tg, ALL)
    assert not np.array_equal(ref1[0], ref2[0])
    lst = _List(ctx, tg)
    try:
        _same(ref1, lst.eval(f.vp, ALL), "first vp")
        _same(ref2, lst.eval(vp2, ALL), "second vp")
        _same(ref1, lst.eval(f.vp, ALL), "first vp again")
    finally:
        lst.close()


def test_an_unprepared_call_between_two_prepared_ones(dense):
    f, ctx = dense
    tg = list(range(ctx.S))
    lst = _List(ctx, tg)
    try:
        first = lst.eval(f.vp, ALL)
        _unprepared(ctx, _perturbed(f.vp, 5), list(range(ctx.S - 1, 2, -1)), ALL)
        _same(first, lst.eval(f.vp, ALL), "prepared, unprepared with other targets and parameters, prepared")
        _same(first, _unprepared(ctx, f.vp, tg, ALL), "against the unprepared call")
    finally:
        lst.close()


def test_targets_without_neighbours_need_no_value_launch(dense, monkeypatch):
    """no link, no pixel set, no items: the sweep runs without a value launch and gives what the unprepared entry gives"""
    import celeste_jl_amd as cel
    f, _ = dense
    own = cel.FieldContext(f.images, f.patches, [[] for _ in f.neighbors])
    try:
        tg = list(range(own.S))
        ref = _unprepared(own, f.vp, tg, ALL)
        assert (ref[4] == 0).all()
        lst = _List(own, tg)
        try:
            got = lst.eval(f.vp, ALL)
            _same(ref, got, "no neighbours")
            monkeypatch.setenv("CELESTE_NO_VALUE_UNION", "1")
            _same(got, lst.eval(f.vp, ALL), "no neighbours, CELESTE_NO_VALUE_UNION=1")
        finally:
            lst.close()
    finally:
        own.close()


def _free_device_bytes():
    free, total = C.c_size_t(), C.c_size_t()
    assert C.CDLL("libamdhip64.so").hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_hundred_lists_created_and_destroyed_release_their_memory(dense):
    if os.environ.get("PYTEST_XDIST_WORKER"):
        pytest.skip("free device memory is a property of the whole GPU: other test processes allocate beside this one (run without -n)")
    f, ctx = dense
    tg = list(range(ctx.S))
    _List(ctx, tg).close()
    base = _free_device_bytes()
    lists = [_List(ctx, tg[k % 5:]) for k in range(100)]
    assert _free_device_bytes() < base
    for lst in lists:
        lst.close()
    assert abs(_free_device_bytes() - base) < (1 << 20)
