"""What does the ctypes binding of libdgg_hip.so marshal?  Dumps, for every function of `_lib.PROTOTYPES`, the return type and the argument
types that `_lib.lib()` has bound, one letter per type (CODES), together with `dgg_abi_version()`:

    python tools/record_abi.py tests/golden/abi_v6.json

The script reads the bound handle, so it runs the same way on a tree whose table is written by hand and on one that derives it from
include/dgg_hip.h.  tests/test_abi_and_host.py requires the working tree to give the same table.  Run it again -- deliberately, under
the new version's file name -- only when a prototype changes and dgg_abi_version is bumped."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CODES = {C.c_void_p: "p", C.c_int: "i", C.c_int64: "l", C.c_uint32: "u", C.c_float: "f", C.c_size_t: "z", C.c_char_p: "s"}


def encode(restype, argtypes):
    return [CODES[restype], "".join(CODES[t] for t in argtypes)]


def table():
    from dgg_amd import _lib
    L = _lib.lib()
    fns = {name: encode(getattr(L, name).restype, getattr(L, name).argtypes) for name in sorted(_lib.PROTOTYPES)}
    return {"abi_version": L.dgg_abi_version(), "functions": fns}


def dump(t, path):
    """one function per line: a change of the fixture shows as the lines that changed"""
    with open(path, "w") as f:
        f.write('{"abi_version": %d,\n"functions": {\n%s\n}}\n'
                % (t["abi_version"], ",\n".join("%s: %s" % (json.dumps(n), json.dumps(v)) for n, v in t["functions"].items())))


if __name__ == "__main__":
    t = table()
    dump(t, sys.argv[1])
    print(len(t["functions"]), "functions, abi_version", t["abi_version"], "->", sys.argv[1])
