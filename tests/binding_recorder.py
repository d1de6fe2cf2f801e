"""A stand-in for the HIP library that records what the Python binding hands to it, and the canonical form the records are compared in
(tests/test_binding_marshalling_cpu.py; the calls are tests/binding_cases.py's).

The binding calls the library without argtypes, so what reaches C is exactly the ctypes objects the wrappers build: a device pointer that
misses c_void_p is truncated to 32 bits, a double that misses c_double goes out as an int.  `canon` keeps the TYPE next to the value of every
argument, so either shows as a difference.  Nothing here needs a built library or a GPU.
"""
import contextlib
import ctypes as C
import hashlib

import numpy as np

# fake device pointers: distinct, page-spaced, above 2^32 (a truncation shows) and above 2^47, where no host allocation of this process can lie --
# a void* FIELD of a structure outside this range is a host address (Solver.ransac's RansacOut) and is recorded as such, not by value
DEVICE_BASE = 0xD12000000000
DEVICE_SPAN = 4096 * 65536
FAKE_CTX = 0xC0FFEE000


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()[:16]


def _ndarray(a):
    return {"nd": [a.dtype.str, list(a.shape), bool(a.flags["C_CONTIGUOUS"]), _sha(np.ascontiguousarray(a).tobytes())]}


def _structure(x):
    raw = bytearray(bytes(x))
    for name, ftype in x._fields_:
        if ftype is C.c_void_p:
            v = getattr(x, name)
            if v is not None and not (DEVICE_BASE <= v < DEVICE_BASE + DEVICE_SPAN):
                off = getattr(type(x), name).offset
                raw[off:off + 8] = b"HOSTADDR"
    return {"struct": [type(x).__name__, bytes(raw).hex()]}


def canon(x):
    """one argument of a library call (or one value a wrapper returns) as JSON-able data: type and value"""
    if x is None or isinstance(x, (bool, str)):
        return x
    if isinstance(x, (int, float)):
        return {type(x).__name__: repr(x)}
    if isinstance(x, bytes):
        return {"bytes": x.hex()}
    if isinstance(x, np.ndarray):
        return _ndarray(x)
    if isinstance(x, np.generic):
        return {"np." + type(x).__name__: repr(x.item())}
    if isinstance(x, C.Structure):
        return _structure(x)
    if isinstance(x, C.Array):
        if issubclass(x._type_, C.Structure):
            return {"array": [x._type_.__name__, len(x), [_structure(e)["struct"][1] for e in x]]}
        if x._type_ is C.c_char:
            return {"array": ["c_char", len(x), x.raw.hex()]}
        if x._type_ is C.c_void_p:  # device pointers by value, host addresses (deep_flow_seq's frames) as such
            return {"array": ["c_void_p", len(x), [v if v is None or DEVICE_BASE <= v < DEVICE_BASE + DEVICE_SPAN else "HOSTADDR" for v in x]]}
        return {"array": [x._type_.__name__, len(x), [canon(e) for e in x]]}
    if isinstance(x, C._CFuncPtr):
        return {"cfunctype": len(type(x)._argtypes_)}
    if isinstance(x, C._SimpleCData):
        arr = getattr(x, "_arr", None)  # ndarray.ctypes.data_as keeps the array on the pointer it returns
        if arr is not None:
            return {"host": _ndarray(arr)["nd"]}
        v = x.value
        return {type(x).__name__: v.hex() if isinstance(v, bytes) else (repr(v) if isinstance(v, float) else v)}
    if hasattr(x, "_obj"):  # byref(obj)
        return {"byref": canon(x._obj)}
    if isinstance(x, dict):
        return {"dict": [[str(k), canon(x[k])] for k in sorted(x, key=str)]}
    if isinstance(x, (list, tuple)):
        return {type(x).__name__: [canon(e) for e in x]}
    raise TypeError("binding_recorder.canon: no canonical form for %r" % (type(x),))


class _Entry:
    """one entry point: callable, returns 0 (RSDSFM_OK, and a count of 0 where the result is a count) unless the case set another value in
    RecorderLib.returns, takes a restype like a ctypes function"""

    def __init__(self, lib, name):
        self._lib, self._name, self.restype, self.argtypes = lib, name, None, None

    def __call__(self, *args):
        self._lib.calls.append([self._name, [canon(a) for a in args]])
        return self._lib.returns.get(self._name, 0)


class RecorderLib:
    def __init__(self):
        self.calls, self.returns = [], {}

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        fn = _Entry(self, name)
        self.__dict__[name] = fn
        return fn


class Env:
    """what a case gets: the module, a Solver on the recorder, and fake device pointers"""

    def __init__(self, pkg, lib):
        self.m, self.lib, self._next = pkg, lib, 0
        self.s = pkg.Solver.__new__(pkg.Solver)
        self.s.lib, self.s.arith, self.s._ctx = lib, "reference", C.c_void_p(FAKE_CTX)

    def p(self):
        self._next += 1
        return DEVICE_BASE + 4096 * self._next

    def P(self, n):
        return [self.p() for _ in range(n)]


@contextlib.contextmanager
def recording(pkg):
    """the recorder installed as the package's reference library and numpy.empty returning zeros (the wrappers' output buffers then have
    defined bytes), both put back afterwards"""
    lib = RecorderLib()
    had, before, empty = "reference" in pkg._libs, pkg._libs.get("reference"), np.empty
    pkg._libs["reference"] = lib
    np.empty = np.zeros
    try:
        yield Env(pkg, lib)
    finally:
        np.empty = empty
        if had:
            pkg._libs["reference"] = before
        else:
            del pkg._libs["reference"]


def run_case(pkg, fn):
    """-> {"calls": [...], "returns": ...} or, where the wrapper refuses, {"calls": [...], "raises": [type, text]}"""
    with recording(pkg) as env:
        try:
            out = {"returns": canon(fn(env))}
        except (pkg.RsdsfmError, ValueError) as e:
            out = {"raises": [type(e).__name__, str(e)]}
        out["calls"] = list(env.lib.calls)
        env.s._ctx = None  # Solver.__del__ then has nothing to destroy
    return out


# ---------------------------------------------------------------------------------------------------
# the two goldens: every case's calls and result, and the module's surface
# ---------------------------------------------------------------------------------------------------
def dev_methods(pkg):
    return sorted(n for n in vars(pkg.Solver) if n.endswith("_dev"))


def covered(cases):
    """the *_dev methods the table has a case for: a case's name is the method's, with an optional /variant"""
    return {name.split("/")[0] for name, _ in cases}


def source_sha(fn):
    import inspect

    return hashlib.sha256(inspect.getsource(fn).encode()).hexdigest()


def build_calls(pkg, cases, uncovered):
    return {"cases": {name: run_case(pkg, fn) for name, fn in cases}, "uncovered": {n: source_sha(vars(pkg.Solver)[n]) for n in sorted(uncovered)}}


def _describe(pkg, obj, root):
    import inspect
    import os
    import types

    if isinstance(obj, types.ModuleType):
        return ["module", obj.__name__.split(".")[-1]]
    if isinstance(obj, type) and issubclass(obj, C.Structure):
        return ["structure", [[f[0], f[1].__name__] for f in obj._fields_], C.sizeof(obj)]
    if isinstance(obj, type):
        return ["class", [b.__name__ for b in obj.__bases__]]
    if isinstance(obj, property):
        return ["property", _sha((obj.__doc__ or "").encode())]
    if inspect.isfunction(obj):
        return ["function", str(inspect.signature(obj)), _sha((obj.__doc__ or "").encode())]
    if isinstance(obj, str) and os.path.isabs(obj):
        return ["path", os.path.relpath(obj, root).replace(os.sep, "/")]
    if isinstance(obj, (bool, int, float, str, bytes, tuple, list)) or obj is None:
        return ["constant", repr(obj)]
    if isinstance(obj, dict):
        return ["constant", repr(sorted(obj.items(), key=repr)) if not any(callable(v) or hasattr(v, "_handle") for v in obj.values()) else "dict"]
    return ["object", type(obj).__name__]


def build_surface(pkg, private, root):
    """every public name of the module and the listed private ones: kind, signature, fields, value; every attribute of Solver: signature and a
    hash of the docstring.  The parameter-struct builders, Solver's methods and the structures are what callers hold on to."""
    names = sorted(n for n in vars(pkg) if not n.startswith("_") and n != "LIB_PATH") + sorted(private)  # (LIB_PATH follows the environment)
    return {"module": {n: _describe(pkg, getattr(pkg, n), root) for n in names},
            "solver": {n: _describe(pkg, v, root) for n, v in sorted(vars(pkg.Solver).items()) if not n.startswith("_")}}


def dumps(obj):
    import json

    return (json.dumps(obj, sort_keys=True, separators=(",", ":")) + "\n").encode()


def loads(b):
    import json

    return json.loads(b)


def write_gz(path, obj):
    import gzip

    with open(path, "wb") as f, gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0, compresslevel=9) as g:  # no name, no time: the same bytes every run
        g.write(dumps(obj))


def read_gz(path):
    import gzip

    with gzip.open(path, "rb") as g:
        return loads(g.read())
