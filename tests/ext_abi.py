"""What the satellites' *_cpu tests share when they hold a module's table against its header and call the entry points with
bad arguments (which return before any launch).  A plain module, as tests/glue_cases.py."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "float": ctypes.c_float}


def header_text(header_name):
    """include/<header_name> without its /* */ comments."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header_name)).read(), flags=re.S)


def declared(header_name, prefix):
    """{name: (restype, argtypes)} of the header's declarations `int | int64_t <prefix>...(...);`, in ctypes, a pointer of any
    kind as c_void_p: what a module's X_SIGNATURES must equal."""
    found = {}
    for res, name, args in re.findall(r"\b(int|int64_t)\s+(%s\w+)\s*\(([^)]*)\)\s*;" % prefix, header_text(header_name)):
        found[name] = (KINDS[res], [ctypes.c_void_p if "*" in a else KINDS[a.replace("const ", "").split()[0]] for a in args.split(",")])
    return found


def aligned():
    """(keep-alive, a 16-byte aligned host address): the calls of these tests return before anything would read it"""
    buf = np.zeros(4096 + 16, dtype=np.uint8)
    return buf, (buf.ctypes.data + 15) & ~15


def swap(good, i, v):
    """The argument list `good` with argument i replaced by v."""
    return [v if j == i else a for j, a in enumerate(good)]
