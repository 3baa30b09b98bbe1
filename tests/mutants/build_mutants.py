#!/usr/bin/env python3
"""Builds the mutated libraries of tests/test_mutants.py: the product source with -DCELESTE_MUTANT=k (see
csrc/elbo_kernels.h), and those of tests/test_satellite_mutants.py: the fit, phot and mcmc libraries with one of
-DCELESTE_CLIENT_MUTANT=k (csrc/engine_client.h), -DCELESTE_FIT_MUTANT=k, -DCELESTE_PHOT_MUTANT=k, -DCELESTE_MCMC_MUTANT=k
(the head of each library's source lists its mutants).  Test infrastructure; the outputs (tests/mutants/*.so) are git-ignored
build artefacts that travel to the GPU box with the snapshot.
usage: python tests/mutants/build_mutants.py [--force] [--satellite]"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
MUTANTS = {1: "iota_by_column", 2: "sky_transposed", 3: "one_stamp_for_all",
           # single-precision code only (CELESTE_FLAG_FP32)
           4: "px2_h4c_dropped_term", 5: "px2_grad_nu_low_half", 6: "value_f2_p12_low_half", 7: "pk_h4b_m3p11"}

# The satellite libraries' mutants: (macro, k, name, library).  The client mutants (engine_client.h's pixel walk) go into fit,
# whose stamps show m + B pixel by pixel; 1 and 2 go into phot as well, which uses m and B apart (a = iota m, b = iota (eps + B)).
SATELLITE = [
    ("CELESTE_CLIENT_MUTANT", 1, "own_light_in_last_column", "fit"),
    ("CELESTE_CLIENT_MUTANT", 2, "neighbour_light_in_its_last_column", "fit"),
    ("CELESTE_CLIENT_MUTANT", 3, "neighbour_bitmap_ignored", "fit"),
    ("CELESTE_CLIENT_MUTANT", 4, "bitmap_transposed", "fit"),
    ("CELESTE_CLIENT_MUTANT", 5, "iota_by_column", "fit"),
    ("CELESTE_CLIENT_MUTANT", 6, "neighbour_with_target_stamp", "fit"),
    ("CELESTE_CLIENT_MUTANT", 1, "own_light_in_last_column", "phot"),
    ("CELESTE_CLIENT_MUTANT", 2, "neighbour_light_in_its_last_column", "phot"),
    ("CELESTE_FIT_MUTANT", 1, "self_ignores_neighbours", "fit"),
    ("CELESTE_FIT_MUTANT", 2, "unvisited_stamp_not_nan", "fit"),
    ("CELESTE_FIT_MUTANT", 3, "max_z_added", "fit"),
    ("CELESTE_FIT_MUTANT", 4, "first_tile_dropped", "fit"),
    ("CELESTE_FIT_MUTANT", 5, "bad_flag_not_reported", "fit"),
    ("CELESTE_PHOT_MUTANT", 1, "round_offset_dropped", "phot"),
    ("CELESTE_PHOT_MUTANT", 2, "b_without_neighbours", "phot"),
    ("CELESTE_PHOT_MUTANT", 3, "at_bound_never_reached", "phot"),
    ("CELESTE_PHOT_MUTANT", 4, "summary_weight_inverse_sigma", "phot"),
    ("CELESTE_PHOT_MUTANT", 5, "tolerance_not_scaled_by_sigma", "phot"),
    ("CELESTE_PHOT_MUTANT", 6, "sigma_without_square_root", "phot"),
    ("CELESTE_MCMC_MUTANT", 1, "source_light_not_rounded_to_float", "mcmc"),
    ("CELESTE_MCMC_MUTANT", 2, "iota_by_column", "mcmc"),
    ("CELESTE_MCMC_MUTANT", 3, "nan_pixel_subtracts_rate", "mcmc"),
    ("CELESTE_MCMC_MUTANT", 4, "lgamma_sum_not_subtracted", "mcmc"),
    ("CELESTE_MCMC_MUTANT", 5, "angle_up_to_two_pi", "mcmc"),
    ("CELESTE_MCMC_MUTANT", 6, "scale_prior_without_log_scale", "mcmc"),
]
MAX_COMPILERS = 16     # compiler processes at a time


def path(k):
    return os.path.join(HERE, "libceleste_mutant_%d_%s.so" % (k, MUTANTS[k]))


def build(force=False):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge     # the product's own command line (exports.map, RCCL)
    newest = max(os.path.getmtime(s) for s in ge.sources("engine"))
    procs = []
    for k in MUTANTS:
        if force or not os.path.exists(path(k)) or os.path.getmtime(path(k)) < newest:
            argv, cwd = ge.compile_command("engine", out=path(k), defines=["CELESTE_MUTANT=%d" % k])
            procs.append(subprocess.Popen(argv, cwd=cwd))
    for p in procs:
        if p.wait() != 0:
            raise SystemExit("mutant build failed")
    return [path(k) for k in MUTANTS]


def satellite_path(entry):
    macro, k, name, lib = entry
    return os.path.join(HERE, "libceleste_%s_mutant_%s_%d_%s.so" % (lib, macro.split("_")[1].lower(), k, name))


def build_satellite(force=False):
    """the libraries of SATELLITE, in its order: each library's own command line (the product's), one -D<macro>=<k>"""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    newest = {lib: max(os.path.getmtime(s) for s in ge.sources(lib)) for lib in {e[3] for e in SATELLITE}}
    todo = [e for e in SATELLITE
            if force or not os.path.exists(satellite_path(e)) or os.path.getmtime(satellite_path(e)) < newest[e[3]]]
    running = []
    while todo or running:
        while todo and len(running) < MAX_COMPILERS:
            macro, k, name, lib = e = todo.pop(0)
            argv, cwd = ge.compile_command(lib, out=satellite_path(e), defines=["%s=%d" % (macro, k)])
            running.append(subprocess.Popen(argv, cwd=cwd))
        if running[0].wait() != 0:
            for p in running[1:]:
                p.wait()
            raise SystemExit("satellite mutant build failed")
        running.pop(0)
    return [satellite_path(e) for e in SATELLITE]


if __name__ == "__main__":
    print("\n".join(build_satellite("--force" in sys.argv) if "--satellite" in sys.argv else build("--force" in sys.argv)))
