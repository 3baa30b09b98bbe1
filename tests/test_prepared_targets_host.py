"""Host only: the prepared-target-list entry points are declared in the header and exported by the version script."""
import fnmatch
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["celeste_targets_create", "celeste_targets_create_device", "celeste_targets_destroy",
           "celeste_elbo_eval_targets_device"]


def test_symbols_in_header_and_exports_map():
    """the prototypes are in include/celeste_targets.h, which include/celeste_mi355x.h includes (and names them)"""
    main = open(os.path.join(ROOT, "include", "celeste_mi355x.h")).read()
    hdr = open(os.path.join(ROOT, "include", "celeste_targets.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert '#include "celeste_targets.h"' in re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    exports = open(os.path.join(ROOT, "celeste.jl_amd", "csrc", "exports.map")).read()
    global_part = exports[exports.index("global:"):exports.index("local:")]
    patterns = re.findall(r"([A-Za-z_0-9*?]+)\s*;", global_part)
    for name in SYMBOLS:
        assert re.search(r"^\s*(int|void)\s+%s\s*\(" % name, code, re.M), "%s is not declared in the header" % name
        assert re.search(r"\b%s\s*\(" % name, main), "%s is not named in celeste_mi355x.h" % name
        assert any(fnmatch.fnmatchcase(name, pat) for pat in patterns), "%s is not exported by exports.map" % name
    assert "typedef struct celeste_targets celeste_targets_t;" in code


def test_symbols_in_the_python_binding():
    from celeste_jl_amd import cabi
    assert set(SYMBOLS) <= set(cabi.EXPORTED_SYMBOLS)
