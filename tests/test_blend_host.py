"""libceleste_blend.so without a GPU: its C ABI (header, exports, Python binding, Julia shim) and the refusal of a
context without a device; the host restatement of the joint optimiser (tests/blend_reference.py) against the oracle's
optimiser at Sa = 1, and its free-space chain rule with cross blocks against torch.autograd at Sa = 2 and 3."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _protos():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "celeste_blend.h")).read(), flags=re.S)
    return {n: (0 if a.strip() in ("", "void") else len(a.split(","))) for n, a in
            re.findall(r"\b(celeste_blend_\w+)\s*\(([^)]*)\)\s*;", hdr)}


def test_the_blend_library_exports_its_c_abi_and_nothing_else(lib):
    from celeste_jl_amd import blend
    protos = _protos()
    assert set(protos) == set(blend.EXPORTED_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", blend.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == sorted(blend.EXPORTED_SYMBOLS)
    b = blend.load_library()
    assert b.celeste_blend_version() == blend.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "celeste_blend.h")).read()
    assert "#define CELESTE_BLEND_ABI_VERSION %d" % blend.ABI_VERSION in hdr
    assert "#define CELESTE_BLEND_SA_MAX %d" % blend.SA_MAX in hdr and blend.SA_MAX >= 4
    assert b"no CPU fallback" in b.celeste_blend_strerror(5)


@pytest.mark.parametrize("name", ["blend", "fit", "phot"])
def test_an_explicit_path_gets_its_own_handle_and_leaves_the_default_alone(lib, name, tmp_path):
    """load_library(path) opens that file; the handle every context gets from load_library() stays the default path's"""
    import importlib
    import shutil
    mod = importlib.import_module("celeste_jl_amd." + name)
    copy = str(tmp_path / os.path.basename(mod.LIB_PATH))
    shutil.copy(mod.LIB_PATH, copy)
    other = mod.load_library(copy)
    assert other._name == copy
    assert getattr(other, "celeste_%s_version" % name)() == mod.ABI_VERSION
    assert len(getattr(other, "celeste_%s_ctx_create" % name).argtypes) == 3          # (declared like the default handle)
    default = mod.load_library()
    assert default._name == os.environ.get("CELESTE_MI355X_%s_LIB" % name.upper(), mod.LIB_PATH)
    assert mod.load_library() is default and mod.load_library(copy) is not other


def test_the_julia_shim_binds_the_header():
    """shim/CelesteMI355XBlend.jl cannot run here (no Julia): every ccall names a prototype of include/celeste_blend.h with
    its argument count, every prototype is bound, and the config mirror lists celeste_optim_config_t's fields in order"""
    protos = _protos()
    jl = open(os.path.join(ROOT, "shim", "CelesteMI355XBlend.jl")).read()
    calls = []
    for m in re.finditer(r"ccall\(\(:(\w+), LIB\), \w+,\s*\(", jl):
        i, depth = m.end(), 1
        while depth:
            depth += {"(": 1, ")": -1}.get(jl[i], 0)
            i += 1
        calls.append((m.group(1), [a for a in jl[m.end():i - 1].split(",") if a.strip()]))
    assert {c for c, _ in calls} == set(protos)
    for name, args in calls:
        assert len(args) == protos[name], name
    hdr = open(os.path.join(ROOT, "include", "celeste_mi355x.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct celeste_optim_config_t \{(.*?)\} celeste_optim_config_t;", hdr,
                                              re.S).group(1), flags=re.S)
    cf = [d.strip().split()[-1] for d in body.split(";") if d.strip()]
    jb = re.search(r"struct OptimConfig\b.*?\n(.*?)\nend", jl, re.S).group(1)
    assert [ln.split("::")[0].strip() for ln in jb.splitlines() if "::" in ln] == cf


def test_no_device_no_fallback(lib):
    """without a device the context refuses (there is no CPU path); on a GPU machine it is created"""
    import torch
    from celeste_jl_amd import blend, cabi, synthetic
    f = synthetic.make_sample_dataset("two_body", seed=1)
    pr = cabi.Problem(f.images, f.patches, f.neighbors)
    if torch.cuda.is_available():
        blend.BlendContext(pr).close()
    else:
        with pytest.raises(RuntimeError, match="no HIP device"):
            blend.BlendContext(pr)


def test_restatement_with_one_member_reproduces_the_oracle_optimiser(oracle):
    """tests/blend_reference.py with Sa = 1 follows the oracle's maximize! iterate for iterate"""
    import blend_reference as BR
    from celeste_jl_amd import cabi, synthetic
    for kind, target in (("galaxy", 0), ("two_body", 1)):
        f = synthetic.make_sample_dataset(kind)
        pb = cabi.Problem(f.images, f.patches, f.neighbors)
        for iters in (3, 8):
            ovp, oit, oev, oel, ost = oracle.maximize(pb, f.vp, target, oracle.OptCfg(max_iters=iters))
            rvp, rit, rev, rel, rst = BR.maximize_blend(oracle, pb, f.vp, [target], max_iters=iters)
            assert ost == 0 and rst == 0
            assert (rit, rev) == (oit, oev), (kind, iters)
            assert abs(rel - oel) <= 1e-10 * abs(oel)
            assert np.abs(rvp - ovp).max() <= 1e-8


def _to_bound_torch(xf, lo, hi):
    import torch
    outs = [torch.sigmoid(xf[:26]) * torch.tensor(hi - lo) + torch.tensor(lo)]
    for f0, n, l in ((26, 2, 0.005), (27, 8, 0.01 / 8), (34, 8, 0.01 / 8)):
        z = torch.cat([xf[f0:f0 + n - 1], torch.zeros(1, dtype=torch.float64)])
        outs.append((1 - n * l) * torch.softmax(z, 0) + l)
    return torch.cat(outs)


@pytest.mark.parametrize("kind,blend", [("two_body", [0, 1]), ("two_body", [1, 0]), ("crowded", [0, 1, 2])])
def test_free_space_cross_blocks_match_autograd(oracle, kind, blend):
    """the restatement's free-space gradient and Hessian (cross blocks J_a' h_ab J_b) against torch.autograd of the
    free-space objective: the blend's ELBO to second order around the point (its bound-space value, gradient and Hessian
    from joint_value_grad_hess), composed with every member's to_bound!"""
    import torch
    import blend_reference as BR
    import joint_objective as JO
    from celeste_jl_amd import synthetic
    if kind == "crowded":
        f = synthetic.make_field(40, 44, 3, seed=5, margin=17)
    else:
        f = synthetic.make_sample_dataset(kind)
    v0, d, h = JO.joint_value_grad_hess(f.images, f.patches, f.vp, blend)
    sa = len(blend)
    cross = max(np.abs(h[44 * a:44 * (a + 1), 44 * b:44 * (b + 1)]).max() for a in range(sa) for b in range(sa) if a != b)
    assert cross > 1e-6 * np.abs(h).max()       # the members overlap: the cross blocks are not empty
    lw = 0.5
    xs, centres, bxs = [], [], []
    for s in blend:
        lo, hi, sc = BR.boxes(f.vp[s, :2], lw)
        vs, x = BR.enforce_to_free(f.vp[s], lo, hi, sc)
        xs.append(x)
        centres.append(f.vp[s, :2].copy())
        bxs.append((lo, hi))
    b0 = torch.tensor(np.concatenate([_to_bound_torch(torch.tensor(x), *bx).numpy() for x, bx in zip(xs, bxs)]))
    dt, ht = torch.tensor(d.reshape(-1)), torch.tensor(h)

    def F(xf):
        b = torch.cat([_to_bound_torch(xf[41 * k:41 * (k + 1)], *bxs[k]) for k in range(sa)]) - b0
        return dt @ b + 0.5 * b @ ht @ b
    x0 = torch.tensor(np.concatenate(xs))
    ga = torch.autograd.functional.jacobian(F, x0).numpy()
    Ha = torch.autograd.functional.hessian(F, x0).numpy()
    g, H = BR.free_derivs(oracle, np.array(xs), centres, d, h, lw)
    assert np.abs(g - ga).max() <= 1e-10 * np.abs(ga).max()
    assert np.abs(H - Ha).max() <= 1e-10 * np.abs(Ha).max()
    for a in range(sa):                          # the cross blocks themselves, on their own scale
        for b in range(sa):
            if a != b:
                blk = slice(41 * a, 41 * (a + 1)), slice(41 * b, 41 * (b + 1))
                assert np.abs(H[blk] - Ha[blk]).max() <= 1e-10 * max(np.abs(Ha[blk]).max(), 1e-300)
