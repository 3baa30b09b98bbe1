#!/usr/bin/env python3
"""The single-precision mode (CELESTE_FLAG_FP32) against fp64, entry by entry, on every fixture the suite checks it on: the
measurement the thresholds of tests/parity_util.py (FP32_F, FP32_T_V / _D / _H) and the split / 256-pixel-chunk bounds of
tests/test_gpu_parity.py rest on.  Needs the GPU.

The suite's own fp32 test bodies are run with assert_fp32_parity replaced by a recorder (and the two variant bounds lifted),
so that what is measured is exactly what the tests compare: the fp32 fuzz seeds, test_fp32_component_loop_within_1e4's
field, the 2 x 2 and 2 x 4 (configs[4]) multifields, the variable fields, the randomised fuzz; then the two goldens against
their committed oracle outputs, and the mutant libraries of tests/mutants (built beforehand: tests/mutation.py) through test_mutants.CHECK.

For each fixture and parameter block (position, star / galaxy flux, colour, shape, type, k) it records the 50th / 99th /
100th percentile of the ratio |fp32 - fp64| / scale for several floors F, and the old norm-scaled errors.
usage: python tools/gpu_fp32_entry_errors.py [--out profiles/fp32_entry_errors_mi355x.json] [--no-mutants]"""
import json
import os
import subprocess
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import parity_util as pu  # noqa: E402

FLOORS = (1e-1, 1e-2, 1e-3, 1e-4)      # worst ratios for each; per-record block percentiles for the first two
RECORDS = []
WORST = {}
VARIANTS = []
CURRENT = {"fixture": None}


def _pct(x):
    x = x[np.isfinite(x)] if np.isfinite(x).any() else x
    if not x.size:
        return None
    return {"p50": float(np.percentile(x, 50)), "p99": float(np.percentile(x, 99)), "max": float(x.max())}


def _summary(gpu, ref, ref_h):
    out = {}
    for F in FLOORS:
        e = pu.fp32_errors(gpu, ref, ref_h, F)     # (non-finite entries come back as inf)
        w = WORST.setdefault("F=%g" % F, {"v": 0.0, "d": 0.0, "h": 0.0})
        for x in ("v", "d", "h"):
            if e[x] is not None and e[x].size:
                w[x] = max(w[x], float(e[x].max()))
        if F not in FLOORS[:2]:
            continue
        s = {"v": float(e["v"].max())}
        for x in ("d", "h"):
            r = e[x]
            if r is None:
                continue
            s[x] = {"all": _pct(r.reshape(-1)), "nonfinite": int((~np.isfinite(r)).sum())}
            for b, idx in pu.FP32_BLOCKS.items():
                s[x][b] = _pct(r[:, idx].reshape(-1))      # (Hessian: the rows of the block)
        out["F=%g" % F] = s
    return out


def recorder(gpu, ref, ref_h, what=""):
    RECORDS.append({"fixture": CURRENT["fixture"], "what": what, "targets": int(len(gpu[0])),
                    "entry": _summary(gpu, ref, ref_h), "norm": pu.norm_scaled_fp32_errors(gpu, ref)})
    return {}


class DeviceTrouble(Exception):
    pass


def _parity_finding(exc):
    """an assertion of a test body itself (a parity mismatch: recorded, the run goes on) -- not a device status, which the
    package raises as AssertionError(celeste_strerror) or CelesteError, and not any other error"""
    if not isinstance(exc, AssertionError):
        return False
    tb = traceback.extract_tb(exc.__traceback__)
    if any(fr.name == "_report_unexpected_statuses" for fr in tb):      # a target's device status, reported by the test
        return False
    return bool(tb) and os.path.dirname(os.path.abspath(tb[-1].filename)) == os.path.join(ROOT, "tests")


def _write(out_path, out):
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(out, fh, indent=1)


def main():
    out_path = os.path.join(ROOT, "profiles", "fp32_entry_errors_mi355x.json")
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
    from oracle import oracle as orc
    orc.lib()
    import test_gpu_parity as tp
    import test_gpu_fullsize as tf
    import test_gpu_round2 as tr2
    import test_mutants as tm
    pu.assert_fp32_parity = recorder
    tp.assert_fp32_parity = recorder
    tf.assert_fp32_parity = recorder
    tp.FP32_SPLIT_VS_FUSED = np.inf
    tp.FP32_CHUNK256_VS_512 = np.inf
    check_variants = tp._check_fp32_variants

    def variants(*a, **k):
        r = check_variants(*a, **k)
        VARIANTS.append(dict(r, fixture=CURRENT["fixture"], what=a[5]))
        return r
    tp._check_fp32_variants = variants
    runs = [("fp32_component_loop_200x240", lambda: tp.test_fp32_component_loop_within_1e4(orc)),
            ("fp32_split_packed_chunk_160x200", lambda: tp.test_fp32_split_packed_and_256_pixel_chunks_against_the_oracle(orc)),
            ("multifield_2x2", lambda: tp.test_multifield_overlapping_images(orc)),
            ("variable_field_300x340", lambda: tr2.test_variable_sky_calibration_and_psf_map_on_the_device(orc)),
            ("config5_multifield_2x4", lambda: tf.test_config5_overlapping_fields_fp32(orc))]
    runs += [("fp32_fuzz_seed_%d" % s, (lambda s=s: tp.test_single_precision_mode_counts_and_masks_like_the_fp64_path(s)))
             for s in range(10)]
    runs += [("randomised_small_seed_%d" % s, (lambda s=s: tp.test_randomised_small_fields(orc, s))) for s in range(16)]
    runs += [("randomised_medium_seed_%d" % s, (lambda s=s: tp.test_randomised_medium_fields(orc, s))) for s in range(4)]
    failures, mut = {}, {}

    def result():
        return {"device": "MI355X", "floors": FLOORS, "worst_over_all_fixtures": WORST,
                "variants_worst": {k: max((r[k] for r in VARIANTS), default=None) for k in ("split_vs_fused", "chunk256_vs_512")},
                "records": RECORDS, "variants": VARIANTS, "mutants": mut, "failures": failures}
    # Anything but a parity finding ends the run at once -- nothing more is started on a device that may have faulted: the
    # partial result is written and the exit status is non-zero.
    try:
        measure(runs, failures, mut, tm)
    except BaseException as e:   # noqa: BLE001
        failures["stopped"] = traceback.format_exc()[-3000:]
        _write(out_path, dict(result(), partial=True))
        print("stopped:", repr(e)[:500], flush=True)
        sys.exit(2)
    _write(out_path, result())
    print(json.dumps({"worst": WORST, "variants_worst": result()["variants_worst"], "failures": list(failures)}))


def measure(runs, failures, mut, tm):
    t0 = time.time()
    for name, fn in runs:
        CURRENT["fixture"] = name
        try:
            fn()
        except AssertionError as e:
            if not _parity_finding(e):
                raise
            failures[name] = traceback.format_exc()[-1500:]      # an old assertion failing is a finding, recorded
        print("%-36s %6.1f s  records %d" % (name, time.time() - t0, len(RECORDS)), flush=True)
    # the goldens against their committed oracle outputs (the mutant tests' fixtures)
    import celeste_jl_amd as cel
    import golden_util as gu
    for case in ("field_72x88_9src_variable", "field_64x80_8src_nan"):
        z = np.load(gu.path(case))
        f = gu.arrays_to_field(z)
        ctx = cel.FieldContext(f.images, f.patches, f.neighbors)
        tg = list(range(len(f.catalog)))
        CURRENT["fixture"] = "golden_" + case
        for flags in (7 | 8, 5 | 8, 7 | 8 | 16):
            v, d, h, cnt, st = ctx.eval_batch(f.vp, tg, flags)
            recorder((v, d, h), (z["v7"], z["d7"], z["h7"]), z["h7"], "golden %s flags %d" % (case, flags))
        ctx.close()
    if "--no-mutants" not in sys.argv:
        import mutation
        engine = mutation.SUITES["engine"]
        libs = {0: None}
        libs.update({k: engine.path(macro, k) for macro, k, _ in engine.mutants})
        for k, lib in libs.items():
            for case in ("field_72x88_9src_variable", "field_64x80_8src_nan"):
                env = dict(os.environ)
                if lib:
                    env["CELESTE_MI355X_LIB"] = lib
                r = subprocess.run([sys.executable, "-c", tm.CHECK % {"root": ROOT}, case, "both"], capture_output=True,
                                   text=True, env=env, timeout=600)
                rep = [ln for ln in r.stdout.splitlines() if ln.startswith("REPORT ")]
                mut["%d %s" % (k, case)] = {"rc": r.returncode, "report": json.loads(rep[0][7:]) if rep else None,
                                           "stderr": r.stderr[-800:] if r.returncode not in (0, 3) else ""}
                print("mutant", k, case, r.returncode, rep[0][:300] if rep else r.stderr[-300:], flush=True)
                if r.returncode not in (0, 3):     # abort, segfault, signal, device error: no further child on this card
                    raise DeviceTrouble("CHECK of mutant %d on %s exited with %d" % (k, case, r.returncode))


if __name__ == "__main__":
    main()
