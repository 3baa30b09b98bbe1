"""shim/CelesteMI355XDetect.jl cannot be executed here (no Julia): every `ccall` in it must name a function
include/celeste_detect.h declares and pass as many arguments as the prototype has, and its struct mirrors must list
the header's fields in order."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "celeste_detect.h")).read(), flags=re.S)
    protos = {}
    for name, args in re.findall(r"\b(celeste_detect_\w+)\s*\(([^)]*)\)\s*;", src):
        args = args.strip()
        protos[name] = 0 if args in ("", "void") else len(args.split(","))
    structs = {}
    for body, name in re.findall(r"typedef struct \{(.*?)\}\s*(\w+);", src, flags=re.S):
        fields = []
        for decl in body.split(";"):
            decl = re.sub(r"//.*", "", decl).strip()
            if not decl:
                continue
            decl = re.sub(r"\[.*?\]", "", decl)
            names = decl.split(None, 1)[1] if not decl.startswith("const") else decl.split(None, 2)[2]
            fields += [n.strip().lstrip("*") for n in names.split(",")]
        structs[name] = fields
    return protos, structs


def _shim():
    return open(os.path.join(ROOT, "shim", "CelesteMI355XDetect.jl")).read()


def test_every_ccall_matches_a_prototype():
    protos, _ = _header()
    calls = re.findall(r"ccall\(\(:(\w+), LIB\), \w+, \(([^)]*)\)", _shim())
    assert {c for c, _ in calls} == set(protos)
    for name, args in calls:
        n = len([a for a in args.split(",") if a.strip()])
        assert n == protos[name], (name, n, protos[name])


def test_struct_mirrors_follow_the_header():
    _, structs = _header()
    src = _shim()
    for jl, c in (("DetectImage", "celeste_detect_image_t"), ("DetectParams", "celeste_detect_params_t")):
        body = re.search(r"struct %s\b.*?\n(.*?)\nend" % jl, src, flags=re.S).group(1)
        fields = [l.split("::")[0].strip() for l in body.splitlines() if "::" in l]
        assert fields == structs[c], (jl, fields, structs[c])
