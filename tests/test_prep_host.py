"""CPU: the host side of device input preparation (celeste_jl_amd.prep, libceleste_prep.so's ABI): the library exports its
header, the ctypes mirrors have the sizes and offsets a C compiler gives the header's structs, invalid arguments are refused
before the library touches a device, infer_box validates `prep`, and cabi.problem_from_table takes a table's own stamps."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "celeste_prep.h"
#define SZ(T) printf("sizeof " #T " %zu\n", sizeof(T))
#define OFF(T, f) printf("offsetof " #T " " #f " %zu\n", offsetof(T, f))
int main(void) {
    SZ(celeste_prep_image_t); SZ(celeste_prep_source_t); SZ(celeste_prep_table_t);
    OFF(celeste_prep_image_t, H); OFF(celeste_prep_image_t, W); OFF(celeste_prep_image_t, band); OFF(celeste_prep_image_t, pixels);
    OFF(celeste_prep_image_t, stride_h); OFF(celeste_prep_image_t, stride_w); OFF(celeste_prep_image_t, sky);
    OFF(celeste_prep_image_t, sky_stride_h); OFF(celeste_prep_image_t, sky_stride_w); OFF(celeste_prep_image_t, nelec_per_nmgy);
    OFF(celeste_prep_image_t, wcs_jacobian); OFF(celeste_prep_image_t, wcs_world0); OFF(celeste_prep_image_t, wcs_pix0);
    OFF(celeste_prep_image_t, psf_width); OFF(celeste_prep_image_t, epsilon); OFF(celeste_prep_image_t, rnrow);
    OFF(celeste_prep_image_t, rncol); OFF(celeste_prep_image_t, ni); OFF(celeste_prep_image_t, nj); OFF(celeste_prep_image_t, nk);
    OFF(celeste_prep_image_t, rrows); OFF(celeste_prep_image_t, cmat);
    OFF(celeste_prep_source_t, pos); OFF(celeste_prep_source_t, is_star); OFF(celeste_prep_source_t, flux);
    OFF(celeste_prep_source_t, gal_radius_px);
    OFF(celeste_prep_table_t, n_entries); OFF(celeste_prep_table_t, n_sources); OFF(celeste_prep_table_t, n_neighbors);
    OFF(celeste_prep_table_t, n_stamps); OFF(celeste_prep_table_t, source); OFF(celeste_prep_table_t, image);
    OFF(celeste_prep_table_t, box); OFF(celeste_prep_table_t, pixel_center); OFF(celeste_prep_table_t, world_center);
    OFF(celeste_prep_table_t, active_pixels); OFF(celeste_prep_table_t, nbr_offsets); OFF(celeste_prep_table_t, nbr_index);
    OFF(celeste_prep_table_t, stamp); OFF(celeste_prep_table_t, stamps);
    printf("version %d stamp %d stages %d\n", CELESTE_PREP_ABI_VERSION, CELESTE_PREP_STAMP, CELESTE_PREP_N_STAGES);
    return 0;
}
"""


@pytest.fixture(scope="module")
def plib(lib):
    import __graft_entry__ as g
    if not os.path.exists(g.PREP_LIB):
        g.build()
    from celeste_jl_amd import prep
    return prep.load_library()


def test_header_symbols_are_exported_and_build_loads_the_library(plib):
    import __graft_entry__ as g
    from celeste_jl_amd import prep
    hdr = open(os.path.join(ROOT, "include", "celeste_prep.h")).read()
    declared = set(re.findall(r"\b(celeste_prep_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(prep.EXPORTED_SYMBOLS), declared ^ set(prep.EXPORTED_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", g.PREP_LIB], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[1] in "TDBR"}
    assert exported == declared, exported ^ declared
    assert plib.celeste_prep_version() == prep.ABI_VERSION
    assert "#define CELESTE_PREP_ABI_VERSION %d" % prep.ABI_VERSION in hdr
    assert plib.celeste_prep_strerror(0) == b"ok" and b"CPU fallback" in plib.celeste_prep_strerror(prep.ERR_NO_DEVICE)
    entry = g.LIBRARIES["prep"]     # build() compiles and loads what its table lists
    assert os.path.basename(entry["source"]) == "celeste_prep.hip" and os.path.isfile(entry["source"])
    assert sys.modules["celeste_jl_amd." + entry["module"]] is prep


def test_ctypes_mirrors_have_the_layout_a_c_compiler_gives_the_header(tmp_path):
    """a C program compiled against include/celeste_prep.h alone prints the sizes and offsets; the mirrors agree"""
    from celeste_jl_amd import prep
    src, exe = tmp_path / "prep_sizes.c", tmp_path / "prep_sizes"
    src.write_text(SIZES_C)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    mirror = {"celeste_prep_image_t": prep.PrepImageT, "celeste_prep_source_t": prep.PrepSourceT,
              "celeste_prep_table_t": prep.PrepTableT}
    sizes = re.findall(r"sizeof (\w+) (\d+)", out)
    offs = re.findall(r"offsetof (\w+) (\w+) (\d+)", out)
    assert {t for t, _ in sizes} == set(mirror)
    for t, n in sizes:
        assert C.sizeof(mirror[t]) == int(n), t
    for t, f, n in offs:
        assert getattr(mirror[t], f).offset == int(n), (t, f)
    for t, cls in mirror.items():      # every field but the reserved ones was printed
        assert {f for f, _ in cls._fields_} - {"reserved", "reserved2"} == {f for tt, f, _ in offs if tt == t}, t
    assert prep.SOURCE_DTYPE.itemsize == C.sizeof(prep.PrepSourceT)
    for f, _ in prep.PrepSourceT._fields_:
        assert prep.SOURCE_DTYPE.fields[f][1] == getattr(prep.PrepSourceT, f).offset, f
    assert "version %d stamp %d stages %d" % (prep.ABI_VERSION, prep.STAMP, prep.N_STAGES) in out
    assert len(prep.STAGES) == prep.N_STAGES


def _create(plib, arr, n, device=0):
    h = C.c_void_p()
    st = plib.celeste_prep_images_create(device, n, arr, C.byref(h))
    if st == 0:
        plib.celeste_prep_images_destroy(h)
    else:
        assert not h.value
    return st


def test_invalid_arguments_are_refused_without_a_device(plib):
    from celeste_jl_amd import prep, synthetic
    INV = prep.ERR_INVALID_ARG
    images = synthetic.variable_images(24, 20, seed=1)[2:4]      # bands 3 and 4, eigen-PSFs

    def structs():
        keep = []
        return prep.image_structs(images, keep), keep
    arr, keep = structs()
    assert arr[1].band == 4 and arr[1].sky and not arr[0].sky and arr[0].rnrow == 51 and arr[0].nk == 3
    # the call itself is well formed: a compute entry point without a device says so
    assert _create(plib, arr, 2) in (0, prep.ERR_NO_DEVICE)
    import torch
    if not torch.cuda.is_available():
        assert _create(plib, arr, 2) == prep.ERR_NO_DEVICE
    # null pointers
    h = C.c_void_p()
    assert plib.celeste_prep_images_create(0, 2, None, C.byref(h)) == INV
    assert plib.celeste_prep_images_create(0, 2, arr, None) == INV
    assert _create(plib, arr, 0) == INV and _create(plib, arr, 2, device=-1) == INV
    for field in ("pixels", "nelec_per_nmgy", "cmat"):
        arr, keep = structs()
        setattr(arr[0], field, None)
        assert _create(plib, arr, 2) == INV, field
    arr, keep = structs()
    arr[1].sky = None                                            # the band-4 image's sky plane is read
    assert _create(plib, arr, 2) == INV
    # H <= 0, W <= 0; a band outside 1 .. 5; rnrow / rncol != 51; strides that are neither row- nor column-major
    for field, value in (("H", 0), ("H", -3), ("W", 0), ("band", 0), ("band", 6), ("rnrow", 50), ("rncol", 52), ("stride_w", 2),
                         ("stride_h", 21), ("ni", 0), ("nj", 9), ("nk", 17)):
        arr, keep = structs()
        setattr(arr[0], field, value)
        assert _create(plib, arr, 2) == INV, (field, value)
    arr, keep = structs()
    arr[0].wcs_jacobian[0] = math.nan
    assert _create(plib, arr, 2) == INV
    arr, keep = structs()
    for k in range(4):
        arr[0].wcs_jacobian[k] = 1.0                             # singular
    assert _create(plib, arr, 2) == INV
    # the calls on a handle
    rh = C.c_void_p()
    src = prep.source_table([synthetic.sample_ce([5.0, 5.0], True)])
    assert plib.celeste_prep_patches(None, 1, src.ctypes.data_as(C.c_void_p), math.nan, 0, C.byref(rh)) == INV
    assert plib.celeste_prep_result_get(None, None) == INV
    assert plib.celeste_prep_bad_sky(None, 0, None, None) == INV
    assert plib.celeste_prep_last_ms(None) == INV
    plib.celeste_prep_images_destroy(None)
    plib.celeste_prep_result_destroy(None)


def test_planes_are_passed_as_they_are():
    """numpy's row-major float32 planes, and column-major ones, go to the library without a copy; anything else is copied"""
    from celeste_jl_amd import prep
    a = np.zeros((6, 4), dtype=np.float32)
    p, sh, sw = prep._plane(a)
    assert p is a and (sh, sw) == (4, 1)
    f = np.asfortranarray(a)
    p, sh, sw = prep._plane(f)
    assert p is f and (sh, sw) == (1, 6)
    p, sh, sw = prep._plane(np.zeros((12, 8), dtype=np.float32)[::2, ::2])
    assert p.flags.c_contiguous and p.shape == (6, 4) and (sh, sw) == (4, 1)
    p, sh, sw = prep._plane(np.zeros((6, 4)))
    assert p.dtype == np.float32 and (sh, sw) == (4, 1)


def test_infer_box_validates_prep():
    import celeste_jl_amd as cel
    from celeste_jl_amd import synthetic
    images = synthetic.blank_images(20, 23)
    catalog = [synthetic.sample_ce([10.1, 12.2], True)]
    with pytest.raises(ValueError, match="prep"):
        cel.infer_box(images, cel.BoundingBox(0.0, 20.0, 0.0, 23.0), catalog, prep="bogus")
    with pytest.raises(ValueError, match="prep"):
        cel.infer_box(images, cel.BoundingBox(0.0, 20.0, 0.0, 23.0), None, prep="gpu")


def test_model_functions_delegate_only_when_asked():
    """device=None is the host function; PatchTable.neighbors returns the lists a table carries"""
    from celeste_jl_amd import model, synthetic
    images = synthetic.blank_images(40, 30)[:2]
    catalog = [synthetic.sample_ce([10.2, 12.1], True), synthetic.sample_ce([14.0, 16.5], False), synthetic.sample_ce([300.0, 2.0], True)]
    t = model.patch_table(images, catalog)
    t2 = model.patch_table(images, catalog, device=None)
    t3 = model.table_for(images, catalog, False)
    for name in ("source", "image", "box", "pixel_center", "world_center", "active_pixels"):
        assert np.array_equal(getattr(t, name), getattr(t2, name)) and np.array_equal(getattr(t, name), getattr(t3, name))
    assert t.neighbors() == [[1], [0], []]
    t.neighbor_lists = [[2], [], [0]]
    assert t.neighbors() == [[2], [], [0]]


def test_problem_from_table_takes_the_stamps_a_table_brings(lib):
    """a hand-made table.stamp / table.stamps holding the psfmap outputs gives, entry for entry, the stamp bytes of the
    psfmap loop; entries of a constant-map image keep going through the host's table, in front of the table's own"""
    from celeste_jl_amd import cabi, model, synthetic
    images = synthetic.variable_images(60, 50, seed=3)[:2] + synthetic.blank_images(60, 50)[2:3]
    catalog = [synthetic.sample_ce(p, s) for p, s in (([10.2, 12.1], True), ([30.0, 25.5], False), ([55.5, 44.0], True),
                                                      ([30.4, 26.0], True))]
    for sparse in (False, True):
        table = model.patch_table(images, catalog, sparse=sparse)
        host = cabi.problem_from_table(images, table, table.neighbors())
        E = len(table.source)
        stamp = np.full(E, -1, dtype=np.int32)
        rows = []
        for e in range(E):
            m = images[table.image[e]].psfmap
            if isinstance(m, model.SDSSPSFMap):
                stamp[e] = len(rows)
                rows.append(np.ascontiguousarray(m(table.pixel_center[e, 0], table.pixel_center[e, 1]).T).reshape(-1))
        table.stamp, table.stamps = stamp, np.stack(rows)
        got = cabi.problem_from_table(images, table, table.neighbors())
        assert got.c.n_stamps == 1 + len(rows) and got.stamps.shape == (1 + len(rows), 51 * 51)
        for e in range(E):
            a, b = host.c_patches[e], got.c_patches[e]
            assert host.stamps[a.stamp].tobytes() == got.stamps[b.stamp].tobytes(), e
            if stamp[e] >= 0:
                assert b.stamp == 1 + stamp[e]
            else:
                assert b.stamp == 0
            assert (a.off_h, a.off_w, a.H2, a.W2) == (b.off_h, b.off_w, b.H2, b.W2)
        # every image with an eigen-PSF: the table's stamps are the problem's, not a copy
        table2 = model.patch_table(images[:2], catalog, sparse=sparse)
        keep = np.flatnonzero(table.image < 2)
        table2.stamp, table2.stamps = stamp[keep], table.stamps
        got2 = cabi.problem_from_table(images[:2], table2, table2.neighbors())
        assert np.shares_memory(got2.stamps, table2.stamps) and got2.c.n_stamps == len(rows)
        assert [got2.c_patches[k].stamp for k in range(len(keep))] == stamp[keep].tolist()
