"""What the ctypes bindings of the satellite libraries (blend, fit, phot, mcmc, synth, detect, prep) share: finding and
opening a library, pointers into numpy arrays, status checks, and the context class of the libraries that keep their own
copy of a problem.  cabi (the engine's binding) stands alone."""
import ctypes as C
import os
from typing import Callable, Optional

from . import cabi

_cache: dict = {}


def open_library(name: str, default_path: str, env: str, abi_version: int, version_symbol: str, declare: Callable,
                 path: Optional[str] = None, engine: bool = True) -> C.CDLL:
    """lib<name>.so at `path`, else at the path the environment variable `env` holds, else at `default_path`, its ABI
    version checked and its argtypes set by declare(lib).  The handle of the default path or of the environment override is
    cached; any other `path` gets a handle of its own and leaves the cache alone.  torch's HIP runtime is loaded first,
    through cabi (the engine's library with it) or, with engine=False, on its own."""
    if path is None and name in _cache:
        return _cache[name]
    override = os.environ.get(env)
    path = path or override or default_path
    cached = path == default_path or path == override
    if not os.path.exists(path):
        raise ImportError("HIP extension %s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no CPU fallback." % path)
    if engine:
        cabi.load_library()
    else:
        try:
            import torch  # noqa: F401
            if torch.cuda.is_available():
                torch.cuda.init()
        except (ImportError, RuntimeError):
            pass
    lib = C.CDLL(path)
    version = getattr(lib, version_symbol)
    version.restype = C.c_int
    if version() // 100 != abi_version // 100:
        raise ImportError("%s has ABI version %d, this binding was written against %d" % (path, version(), abi_version))
    declare(lib)
    if cached:
        _cache[name] = lib
    return lib


def ptr(a, ctype):
    """the array's data as a pointer of type `ctype`; None stays None (a null pointer)"""
    return None if a is None else a.ctypes.data_as(ctype)


def checker(name: str, error: Optional[Callable] = None):
    """check(lib, status) of lib<name>.so: a non-zero status raises error(status, text of celeste_<name>_strerror), by
    default RuntimeError("libceleste_<name>: text (status n)")"""
    def check(lib, st: int):
        if st != 0:
            text = getattr(lib, "celeste_%s_strerror" % name)(st).decode()
            if error is not None:
                raise error(st, text)
            raise RuntimeError("libceleste_%s: %s (status %d)" % (name, text, st))
    return check


class Context:
    """A satellite library's copy of a problem (celeste_<name>_ctx_t), built from a marshalled celeste_problem_t.  A
    subclass names its library (_name) and the module-level load_library (_load)."""
    _name = ""
    _load = None

    def __init__(self, problem: "cabi.Problem", device: int = 0):
        self.lib = type(self)._load()
        self.problem = problem
        self.S = problem.n_sources
        self._keep: list = []
        pc = cabi.ProblemT.from_buffer_copy(problem.c)
        if not pc.images:
            pc.images = cabi.marshal_image_structs(problem.images, self._keep)
        self._pc = pc
        h = C.c_void_p()
        create = getattr(self.lib, "celeste_%s_ctx_create" % self._name)
        checker(self._name)(self.lib, create(C.byref(pc), int(device), C.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            getattr(self.lib, "celeste_%s_ctx_destroy" % self._name)(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
