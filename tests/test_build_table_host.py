"""CPU: the build table of __graft_entry__.py (LIBRARIES) against the tree and against what it builds: every entry names
files that exist, the table's directories are the directories of csrc/ that hold a .hip file, only the engine compiles a
.hip file of csrc's top level and links RCCL, and the five libraries that compile the engine's context without its
evaluation code (fit, phot, info, resid, astrom) and the one that compiles it with the evaluation launcher (blend) export
their header's functions and nothing else, and ask no library for an RCCL symbol."""
import importlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTEXT_ONLY = ("fit", "phot", "info", "resid", "astrom")


@pytest.fixture(scope="module")
def g(lib):
    import __graft_entry__ as g
    if not all(os.path.exists(e["output"]) for e in g.LIBRARIES.values()):
        g.build()
    return g


def test_every_entry_names_files_that_exist():
    import __graft_entry__ as g
    assert len(g.LIBRARIES) == 11 and set(CONTEXT_ONLY) < set(g.LIBRARIES)
    for name, e in g.LIBRARIES.items():
        assert os.path.isdir(e["dir"]) and os.path.dirname(e["source"]) == e["dir"] == os.path.dirname(e["output"]), name
        assert os.path.isfile(e["source"]) and os.path.isfile(os.path.join(e["dir"], "exports.map")), name
        for h in e["headers"]:
            assert os.path.isfile(os.path.join(ROOT, "include", h)), (name, h)
        assert os.path.isfile(os.path.join(ROOT, "celeste.jl_amd", e["module"] + ".py")), name
        assert all(os.path.isfile(s) for s in g.sources(name)) and e["source"] in g.sources(name), name
        argv, cwd = g.compile_command(name)
        assert cwd == e["dir"] and argv[0] == g.HIPCC and e["source"] in argv and argv[argv.index("-o") + 1] == e["output"], name
    assert len({e["output"] for e in g.LIBRARIES.values()}) == len(g.LIBRARIES)
    assert g.LIB == g.LIBRARIES["engine"]["output"] and g.PREP_LIB == g.LIBRARIES["prep"]["output"]
    assert g.ASTROM_DIR == g.LIBRARIES["astrom"]["dir"]


def test_the_table_lists_every_directory_of_csrc_that_holds_a_hip_file():
    import __graft_entry__ as g
    have = {d for d, _, files in os.walk(g.CSRC) if any(f.endswith(".hip") for f in files)}
    assert have == {e["dir"] for e in g.LIBRARIES.values()}, have ^ {e["dir"] for e in g.LIBRARIES.values()}


def test_only_the_engine_compiles_the_engine_whole_and_links_rccl():
    import __graft_entry__ as g
    for name, e in g.LIBRARIES.items():
        assert (e["csrc"] == "all") == (name == "engine") and ("-lrccl" in e["link"]) == (name == "engine"), name
        text = open(e["source"]).read()
        if name in CONTEXT_ONLY:
            assert '#include "../engine_context.h"\n#include "../engine_client.h"\n' in text and e["link"] == ["-lpthread"], name
        if name == "blend":
            assert '#include "../engine_eval.h"\n#include "../engine_client.h"\n' in text and e["link"] == ["-lpthread"], name
    # no file under csrc includes a .hip file: a library compiles its own and headers
    for d, _, files in os.walk(g.CSRC):
        for f in files:
            if f.endswith((".hip", ".h", ".inc")):
                included = re.findall(r'^\s*#\s*include\s*[<"]([^>"]+)[>"]', open(os.path.join(d, f)).read(), flags=re.M)
                assert not [i for i in included if i.endswith(".hip")], (d, f)


@pytest.mark.parametrize("name", CONTEXT_ONLY + ("blend",))
def test_a_context_only_library_exports_its_header_and_imports_no_rccl_symbol(g, name):
    e = g.LIBRARIES[name]
    module = importlib.import_module("celeste_jl_amd." + e["module"])
    hdr = open(os.path.join(ROOT, "include", "celeste_%s.h" % name)).read()
    declared = set(re.findall(r"\b(celeste_%s_[a-z_0-9]+)\s*\(" % name, hdr))
    assert declared and declared == set(module.EXPORTED_SYMBOLS), declared ^ set(module.EXPORTED_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", e["output"]], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[1] in "TDBR"}
    assert exported == declared, exported ^ declared
    undefined = subprocess.run(["nm", "-D", "--undefined-only", e["output"]], capture_output=True, text=True, check=True).stdout
    assert undefined.strip() and not [ln for ln in undefined.splitlines() if ln.split()[-1].startswith("nccl")]
    needed = subprocess.run(["readelf", "-d", e["output"]], capture_output=True, text=True, check=True).stdout
    assert "librccl" not in needed and "libamdhip64" in needed
