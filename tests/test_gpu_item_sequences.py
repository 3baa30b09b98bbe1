"""-m gpu: a prepared list's pixel work items started from their descriptors (csrc/work_sequences.h, pixel_desc_kernel), bit
for bit.

A prepared sweep launches one workgroup of pixel_desc_kernel per work item of the list; the item comes from a 64-byte
descriptor made when the list was created, and the workgroup stages the same tables, runs the same chunk loop and writes
the same records as pixel_kernel.  So every comparison here is np.array_equal over v, d, h, counters and status, against
celeste_elbo_eval_batch_device on the same context and vp AND against the same list under CELESTE_NO_SEQUENCES=1 (pixel_kernel
over the list's work items).  The lists run as they ship: nothing but CELESTE_EVAL_FUSED=0, which keeps small Hessian batches on
the pixel + lift path."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 44
ALL = 1 | 2 | 4


@pytest.fixture(autouse=True)
def pixel_and_lift_path(monkeypatch):
    monkeypatch.setenv("CELESTE_EVAL_FUSED", "0")
    monkeypatch.delenv("CELESTE_NO_SEQUENCES", raising=False)


@pytest.fixture(scope="module")
def field():
    from celeste_jl_amd import synthetic
    f = synthetic.make_field(160, 200, 40, seed=11, nan_fraction=0.005)
    assert sum(len(n) for n in f.neighbors) > 0
    return f


@pytest.fixture(scope="module")
def dense(field):
    import celeste_jl_amd as cel
    ctx = cel.FieldContext(field.images, field.patches, field.neighbors)
    yield field, ctx
    ctx.close()


@pytest.fixture(scope="module")
def sparse():
    import celeste_jl_amd as cel
    from celeste_jl_amd import synthetic
    f = synthetic.make_multifield((2, 3), 160, 160, 0.10, 70, seed=11, sparse=True)
    ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
    yield f, ctx
    ctx.close()


# patch sizes (H2, W2) of the `shaped` context, source s takes entry s % len: one-trip patches (small radii), exact multiples
# of the 256-pixel chunk, one pixel more than a multiple of 64, and a few ordinary ones
SHAPES = [(7, 7), (8, 8), (16, 16), (5, 13), (32, 16), (11, 35), (6, 9), (16, 48), (3, 43), (21, 23), (7, 5), (9, 57)]


@pytest.fixture(scope="module")
def shaped(field):
    """the dense field's images and sources with patches cut to SHAPES around each source"""
    import celeste_jl_amd as cel
    from celeste_jl_amd.model import ImagePatch, neighbor_map
    f = field
    patches = []
    for s, ce in enumerate(f.catalog):
        h2, w2 = SHAPES[s % len(SHAPES)]
        row = []
        for img in f.images:
            pc = img.world_to_pix(ce.pos)
            h0 = min(max(int(round(pc[0])) - h2 // 2, 1), img.H - h2 + 1)
            w0 = min(max(int(round(pc[1])) - w2 // 2, 1), img.W - w2 + 1)
            row.append(ImagePatch.from_box(img, ((h0, h0 + h2 - 1), (w0, w0 + w2 - 1))))
        patches.append(row)
    sizes = {p.active_pixel_bitmap.size for row in patches for p in row}
    assert {49, 64, 256, 65, 512, 385, 768, 129, 513} <= sizes, sizes
    nbrs = neighbor_map(patches)
    assert sum(len(n) for n in nbrs) > 0
    ctx = cel.FieldContext(f.images, patches, nbrs)
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


def _check_list(lst, ctx, vp, targets, flags, monkeypatch, what):
    """the list through the descriptors == the unprepared entry == the list through pixel_kernel (the A/B switch)"""
    ref = _unprepared(ctx, vp, targets, flags)
    assert (ref[4] == 0).all(), what
    _same(ref, lst.eval(vp, flags), what + ": descriptors against the unprepared entry")
    monkeypatch.setenv("CELESTE_NO_SEQUENCES", "1")
    off = lst.eval(vp, flags)
    monkeypatch.delenv("CELESTE_NO_SEQUENCES")
    _same(off, lst.eval(vp, flags), what + ": descriptors against CELESTE_NO_SEQUENCES=1")
    _same(ref, off, what + ": CELESTE_NO_SEQUENCES=1 against the unprepared entry")


def _check(ctx, vp, targets, flags, monkeypatch, what):
    lst = _List(ctx, targets)
    try:
        _check_list(lst, ctx, vp, targets, flags, monkeypatch, what)
    finally:
        lst.close()


@pytest.mark.parametrize("flags", [ALL, 3, 1], ids=["flags7", "flags3", "flags1"])
def test_every_source_as_target(dense, flags, monkeypatch):
    f, ctx = dense
    _check(ctx, f.vp, list(range(ctx.S)), flags, monkeypatch, "all sources, flags %d" % flags)


def test_strict_subset_whose_neighbours_lie_outside_it(dense, monkeypatch):
    f, ctx = dense
    tg = list(range(1, ctx.S, 3))
    inside = set(tg)
    assert any(q not in inside for t in tg for q in f.neighbors[t])
    _check(ctx, f.vp, tg, ALL, monkeypatch, "subset")
    _check(ctx, f.vp, tg[::-1], 1, monkeypatch, "subset, reversed, value only")


def test_list_of_800_entries_runs_groups_of_two_chunks(dense, monkeypatch):
    """>= 768 entries: groups of two chunks (G = 2), the 40 sources twenty times over"""
    f, ctx = dense
    tg = list(range(ctx.S)) * 20
    _check(ctx, f.vp, tg, ALL, monkeypatch, "800 entries")


@pytest.mark.parametrize("flags", [ALL, 1], ids=["flags7", "flags1"])
def test_small_patches_and_exact_multiples(shaped, flags, monkeypatch):
    """one-trip patches; 256, 512 and 768 pixels end exactly at a chunk, 65, 129, 385 and 513 leave a one-pixel trip; with
    800 entries (G = 2) an item's second chunk may not exist"""
    f, ctx = shaped
    _check(ctx, f.vp, list(range(ctx.S)), flags, monkeypatch, "shaped patches, flags %d" % flags)
    _check(ctx, f.vp, list(range(ctx.S)) * 20, flags, monkeypatch, "shaped patches, 800 entries, flags %d" % flags)


def test_sparse_context_with_empty_patches(sparse, monkeypatch):
    """a target without a patch in some image has no work item there, and the rows of nbr_vis come from the descriptor"""
    f, ctx = sparse
    assert ctx.problem.sparse
    per_source = np.bincount(ctx.problem.patch_source, minlength=ctx.S)
    assert per_source.min() < per_source.max()
    _check(ctx, f.vp, list(range(ctx.S)), ALL, monkeypatch, "sparse, all sources")
    _check(ctx, f.vp, list(range(0, ctx.S, 2)) + [5], 3, monkeypatch, "sparse, subset")


def test_two_vp_on_one_list_and_an_unprepared_call_in_between(dense, monkeypatch):
    f, ctx = dense
    tg = list(range(ctx.S))
    vp2 = _perturbed(f.vp, 3)
    lst = _List(ctx, tg)
    try:
        _check_list(lst, ctx, f.vp, tg, ALL, monkeypatch, "first vp")
        first = lst.eval(f.vp, ALL)
        ref2 = _unprepared(ctx, vp2, tg, ALL)
        assert not np.array_equal(ref2[0], first[0])
        _same(ref2, lst.eval(vp2, ALL), "second vp")
        _unprepared(ctx, _perturbed(f.vp, 5), list(range(ctx.S - 1, 2, -1)), ALL)
        _same(first, lst.eval(f.vp, ALL), "prepared, unprepared with other targets, prepared")
    finally:
        lst.close()


def test_two_lists_alive_on_one_context(dense, monkeypatch):
    f, ctx = dense
    ta, tb = list(range(ctx.S)), list(range(ctx.S - 1, -1, -1))[:35]
    ra, rb = _unprepared(ctx, f.vp, ta, ALL), _unprepared(ctx, f.vp, tb, ALL)
    la = _List(ctx, ta)
    lb = _List(ctx, tb)
    try:
        for k in range(2):
            _same(ra, la.eval(f.vp, ALL), "list a, round %d" % k)
            _same(rb, lb.eval(f.vp, ALL), "list b, round %d" % k)
    finally:
        la.close()
        lb.close()


POISON_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(tests)r)
import test_gpu_item_sequences as T
import celeste_jl_amd as cel
from celeste_jl_amd import synthetic

f = synthetic.make_field(160, 200, 40, seed=11, nan_fraction=0.005)
ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
for tg, flags in ((list(range(ctx.S)), 7), (list(range(ctx.S)) * 20, 7), (list(range(1, ctx.S, 3)), 1)):
    ref = T._unprepared(ctx, f.vp, tg, flags)
    lst = T._List(ctx, tg)
    T._same(ref, lst.eval(f.vp, flags), "poisoned allocations, %%d entries" %% len(tg))
    lst.close()
ctx.close()
print("poison ok")
"""


def test_fresh_allocations_poisoned(tmp_path):
    """CELESTE_POISON=1 is read once per process: a child process with every fresh device allocation filled with 0xFF bytes,
    so that a descriptor field the host left unwritten, or a read past the list's arrays, shows as a difference"""
    import os
    import subprocess
    import sys
    tests = os.path.dirname(os.path.abspath(__file__))
    script = tmp_path / "poison_child.py"
    script.write_text(POISON_CHILD % {"tests": tests})
    env = dict(os.environ, CELESTE_POISON="1", CELESTE_EVAL_FUSED="0")
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(tests)] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout + r.stderr
