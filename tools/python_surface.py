"""The Python surface of entropy_coders_amd as plain data, for tests/test_python_surface.py:
    python tools/python_surface.py            # print the dump
    python tools/python_surface.py --write    # (re)write tests/golden/python_surface.json
For every name in the package's __all__: its kind, its signature where it has one and the CRC-32 of its
docstring; for every class among them the same for every attribute `dir()` finds (methods may live in base
classes), dunders other than __init__ left out, with how the attribute is stored (`inspect.getattr_static`):
a plain function, a staticmethod, a classmethod or data.  What a class inherits from the interpreter's own
types (object, Exception, ctypes.Structure) is left out: it is no part of this package's surface and differs
between Python versions.  Needs neither torch nor the built library.

The fixture is written before a change that must leave the surface alone and never from the changed tree."""
import inspect
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "python_surface.json")


def _signature(obj):
    try:
        return str(inspect.signature(obj))
    except (TypeError, ValueError):
        return None


def _doc(obj):
    doc = getattr(obj, "__doc__", None)
    return None if doc is None else zlib.crc32(doc.encode())


def _entry(kind: str, obj) -> dict:
    if kind == "data":  # a constant or a table: its type, and the value of a plain number or string
        e = {"kind": "data", "type": type(obj).__name__}
        if isinstance(obj, (int, str)):
            e["value"] = obj
        return e
    return {"kind": kind, "signature": _signature(obj), "doc": _doc(obj)}


def _owner(cls, attr: str):
    return next(c for c in cls.__mro__ if attr in vars(c))


def _attribute(cls, attr: str) -> dict:
    static = inspect.getattr_static(cls, attr)
    if isinstance(static, staticmethod):
        return _entry("staticmethod", static.__func__)
    if isinstance(static, classmethod):
        return _entry("classmethod", static.__func__)
    if inspect.isfunction(static):
        return _entry("function", static)
    return {"kind": "data", "type": type(static).__name__}


def surface() -> dict:
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import entropy_coders_amd as E

    out = {}
    for name in sorted(E.__all__):
        obj = getattr(E, name)
        if not inspect.isclass(obj):
            out[name] = _entry("function" if inspect.isfunction(obj) else "data", obj)
            continue
        out[name] = _entry("class", obj)
        for attr in dir(obj):
            if attr.startswith("__") and attr.endswith("__") and attr != "__init__":
                continue
            if _owner(obj, attr).__module__ in ("builtins", "_ctypes"):
                continue
            out[f"{name}.{attr}"] = _attribute(obj, attr)
    return out


if __name__ == "__main__":
    text = json.dumps(surface(), indent=0, sort_keys=True) + "\n"
    if "--write" in sys.argv[1:]:
        with open(FIXTURE, "w") as f:
            f.write(text)
        print(f"{FIXTURE}: {len(surface())} entries, {len(text)} bytes")
    else:
        sys.stdout.write(text)
