"""CPU: the host side of the detection path of device input preparation (prep.detected_table, detect.detect_table,
libceleste_prep.so's celeste_prep_detected): the ctypes mirrors of the new structs have the layout a C compiler gives the
header, every class of invalid argument is refused without a device, and the Python entry points have the stated
signatures."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

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
    SZ(celeste_prep_detection_t); SZ(celeste_prep_catalog_t);
    OFF(celeste_prep_detection_t, npix); OFF(celeste_prep_detection_t, xmin); OFF(celeste_prep_detection_t, xmax);
    OFF(celeste_prep_detection_t, ymin); OFF(celeste_prep_detection_t, ymax); OFF(celeste_prep_detection_t, x);
    OFF(celeste_prep_detection_t, y); OFF(celeste_prep_detection_t, a); OFF(celeste_prep_detection_t, b);
    OFF(celeste_prep_detection_t, theta); OFF(celeste_prep_detection_t, flux);
    OFF(celeste_prep_catalog_t, n_objects); OFF(celeste_prep_catalog_t, n_detections); OFF(celeste_prep_catalog_t, pos);
    OFF(celeste_prep_catalog_t, flux); OFF(celeste_prep_catalog_t, gal_axis_ratio); OFF(celeste_prep_catalog_t, gal_angle);
    OFF(celeste_prep_catalog_t, gal_radius_px); OFF(celeste_prep_catalog_t, det_offsets); OFF(celeste_prep_catalog_t, det_image);
    OFF(celeste_prep_catalog_t, det_object);
    printf("tile %d block %d stages %d\n", CELESTE_PREP_MATCH_TILE, CELESTE_PREP_MATCH_BLOCK, CELESTE_PREP_DETECTED_N_STAGES);
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


def test_ctypes_mirrors_of_the_new_structs_have_the_headers_layout(tmp_path):
    from celeste_jl_amd import prep
    src, exe = tmp_path / "detected_sizes.c", tmp_path / "detected_sizes"
    src.write_text(SIZES_C)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    mirror = {"celeste_prep_detection_t": prep.PrepDetectionT, "celeste_prep_catalog_t": prep.PrepCatalogT}
    sizes = re.findall(r"sizeof (\w+) (\d+)", out)
    offs = re.findall(r"offsetof (\w+) (\w+) (\d+)", out)
    assert {t for t, _ in sizes} == set(mirror)
    for t, n in sizes:
        assert C.sizeof(mirror[t]) == int(n), t
    for t, f, n in offs:
        assert getattr(mirror[t], f).offset == int(n), (t, f)
    for t, cls in mirror.items():
        assert {f for f, _ in cls._fields_} - {"reserved"} == {f for tt, f, _ in offs if tt == t}, t
    assert prep.DETECTION_DTYPE.itemsize == C.sizeof(prep.PrepDetectionT)
    for f, _ in prep.PrepDetectionT._fields_:
        assert prep.DETECTION_DTYPE.fields[f][1] == getattr(prep.PrepDetectionT, f).offset, f
    assert "tile %d block %d stages %d" % (prep.MATCH_TILE, prep.MATCH_BLOCK, prep.DETECTED_N_STAGES) in out
    assert len(prep.DETECTED_STAGES) == prep.DETECTED_N_STAGES
    # what the issue keeps as it is
    hdr = open(os.path.join(ROOT, "include", "celeste_prep.h")).read()
    assert "#define CELESTE_PREP_ABI_VERSION 100" in hdr and "#define CELESTE_PREP_N_STAGES 5 " in hdr


def _catalog(n=3, **over):
    """a hand-made detect.Catalog of n objects"""
    from celeste_jl_amd.detect import Catalog
    z = np.zeros(n)
    f = dict(npix=np.full(n, 9, dtype=np.int64), xmin=np.arange(n) * 10 + 3, xmax=np.arange(n) * 10 + 7, ymin=np.full(n, 4),
             ymax=np.full(n, 9), x=np.arange(n) * 10.0 + 6.0, y=np.full(n, 7.5), a=np.full(n, 2.0), b=np.full(n, 1.5),
             theta=np.full(n, 0.3), flux=np.full(n, 100.0))
    f.update(over)
    return Catalog(rms=1.0, thresh=1.3, x2=z, y2=z, xy=z, peak=z, parent=np.full(n, -1), **f)


def _check(plib, off, det, ang, match_radius=1.0, min_radius=5.0, dilate=0.2, flags=1, n_images=None):
    vp = C.c_void_p
    n_images = len(off) - 1 if n_images is None else n_images
    return plib.celeste_prep_detected_check(n_images, off.ctypes.data_as(vp), det.ctypes.data_as(vp), ang.ctypes.data_as(vp),
                                            match_radius, min_radius, dilate, flags)


def test_every_class_of_invalid_argument_is_refused_without_a_device(plib):
    from celeste_jl_amd import prep
    INV = prep.ERR_INVALID_ARG
    off, det = prep.detection_table([_catalog(3), _catalog(0), _catalog(2)])
    ang = np.array([0.0, 0.1, -0.2])
    assert off.tolist() == [0, 3, 3, 5] and det["xmax"].tolist() == [7, 17, 27, 7, 17] and det["x"][4] == 16.0
    assert _check(plib, off, det, ang) == 0
    assert _check(plib, off, det, ang, match_radius=0.0, min_radius=0.0, dilate=0.0, flags=3) == 0
    assert _check(plib, off, det, ang, match_radius=math.inf) == 0                 # not NaN, not negative
    empty = np.zeros(4, dtype=np.int64)
    assert _check(plib, empty, det[:0], ang) == 0                                   # no detection at all
    # null pointers
    vp = C.c_void_p
    assert plib.celeste_prep_detected_check(3, None, det.ctypes.data_as(vp), ang.ctypes.data_as(vp), 1.0, 5.0, 0.2, 1) == INV
    assert plib.celeste_prep_detected_check(3, off.ctypes.data_as(vp), None, ang.ctypes.data_as(vp), 1.0, 5.0, 0.2, 1) == INV
    assert plib.celeste_prep_detected_check(3, off.ctypes.data_as(vp), det.ctypes.data_as(vp), None, 1.0, 5.0, 0.2, 1) == INV
    rh = C.c_void_p()
    args = (off.ctypes.data_as(vp), det.ctypes.data_as(vp), ang.ctypes.data_as(vp), 1.0, 5.0, 0.2, 1)
    assert plib.celeste_prep_detected(None, *args, C.byref(rh)) == INV and not rh.value
    assert plib.celeste_prep_result_get_catalog(None, None) == INV
    assert plib.celeste_prep_detected_last_ms(None) == INV
    # offsets that do not ascend from 0
    for bad in ([1, 3, 3, 5], [0, 3, 2, 5], [0, -1, 3, 5]):
        assert _check(plib, np.array(bad, dtype=np.int64), det, ang) == INV, bad
    # per detection: npix <= 0, a non-finite x, y, a, b, theta or flux, a <= 0, reversed bounds
    for field, value in (("npix", 0), ("npix", -4), ("x", math.nan), ("y", math.inf), ("a", math.nan), ("b", -math.inf),
                         ("theta", math.nan), ("flux", math.inf), ("a", 0.0), ("a", -1.0), ("xmax", 2), ("ymax", 3)):
        for d in (0, 4):
            bad = det.copy()
            bad[field][d] = value
            assert _check(plib, off, bad, ang) == INV, (field, value, d)
    assert _check(plib, off, det, np.array([0.0, math.nan, 0.0])) == INV            # angle
    assert _check(plib, off, det, np.array([0.0, 0.0, math.inf])) == INV
    # match_radius NaN or negative; min_radius_pix / dilate not finite or negative; an unknown flag
    for kw in ({"match_radius": math.nan}, {"match_radius": -1e-9}, {"min_radius": math.nan}, {"min_radius": math.inf},
               {"min_radius": -1.0}, {"dilate": math.nan}, {"dilate": math.inf}, {"dilate": -0.1}, {"flags": 4}, {"n_images": 0}):
        assert _check(plib, off, det, ang, **kw) == INV, kw


def test_the_compute_entry_reports_a_missing_device(plib):
    """without a device prep.detected_table ends in ERR_NO_DEVICE (there is no CPU path); with one it runs"""
    import torch
    from celeste_jl_amd import prep, synthetic
    images = synthetic.blank_images(40, 40)[:3]
    cats = [_catalog(3), _catalog(0), _catalog(2)]
    if torch.cuda.is_available():
        catalog, table = prep.detected_table(images, cats, 1.0)
        assert len(catalog) == table.n_sources == len(table.detections)
    else:
        with pytest.raises(prep.PrepError) as ei:
            prep.detected_table(images, cats, 1.0)
        assert ei.value.status == prep.ERR_NO_DEVICE
    with pytest.raises(ValueError):
        prep.detected_table(images, cats[:2], 1.0)


def test_python_entry_points_have_the_stated_signatures():
    from celeste_jl_amd import detect, infer, prep
    p = inspect.signature(prep.detected_table).parameters
    assert list(p) == ["images", "catalogs", "match_radius", "sparse", "device", "prep_images"]
    assert p["sparse"].default is None and p["device"].default == 0 and p["prep_images"].default is None
    p = inspect.signature(detect.detect_table).parameters
    assert list(p) == ["images", "device", "match_radius", "prep_images", "extract_kw"]
    assert p["device"].default == 0 and p["match_radius"].default == 1 / 3600 and p["prep_images"].default is None
    assert p["extract_kw"].kind is inspect.Parameter.VAR_KEYWORD
    assert inspect.signature(detect.extract).parameters["want_pixels"].default is True
    assert inspect.signature(infer.infer_box).parameters["prep"].default == "host"
    assert "brings its own patches either way" not in infer.infer_box.__doc__
    assert set(prep.EXPORTED_SYMBOLS) >= {"celeste_prep_detected", "celeste_prep_detected_check", "celeste_prep_result_get_catalog",
                                          "celeste_prep_detected_last_ms"}
