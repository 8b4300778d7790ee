"""ctypes binding of libdgg_hip.so.  The prototypes are not written here: PROTOTYPES / RESTYPES are parsed from the public header
include/dgg_hip.h, the one description of the C ABI (the library's definitions are compiled against the same file).  Entry points added
since that ABI version was recorded are declared in include/dgg_hip_next.h (purely additive, folded into dgg_hip.h at the next ABI bump)
and parsed into tables of their own, NEXT_PROTOTYPES / NEXT_RESTYPES (the header's first block) and NEXT_BLOCKS (one table per later
block, by the name on its `==== block NAME ====` line): PROTOTYPES stays the recorded ABI.  include/dgg_hip_adj_loss.h (the adjacency
supervision loss, additive in the same way) is parsed into ADJ_LOSS_PROTOTYPES / ADJ_LOSS_RESTYPES, include/dgg_hip_sampling.h (the
mini-batch sampling entries) into SAMPLING_PROTOTYPES / SAMPLING_RESTYPES, include/dgg_hip_batch_graph.h (the batch edit: noisy edges and
the same-class target) into BATCH_GRAPH_PROTOTYPES / BATCH_GRAPH_RESTYPES.  Fails loudly when the HIP
library or a header is missing: there is no CPU fallback anywhere in this package."""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("DGG_HIP_SO", os.path.join(_HERE, "libdgg_hip.so"))   # override: diagnostic builds only

HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "dgg_hip.h"))
NEXT_HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "dgg_hip_next.h"))     # entry points since the recorded ABI
ADJ_LOSS_HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "dgg_hip_adj_loss.h"))   # the adjacency supervision loss
SAMPLING_HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "dgg_hip_sampling.h"))   # random walks and induced sub-graphs
BATCH_GRAPH_HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "dgg_hip_batch_graph.h"))   # noisy edges and target of a batch

_C_TYPES = {"int": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float, "size_t": C.c_size_t}
_C_RETURNS = {"int": C.c_int, "size_t": C.c_size_t, "const char *": C.c_char_p}
_INFO = ("dgg_last_error", "dgg_abi_version")    # bound like the rest, not listed in PROTOTYPES


class DggHipError(RuntimeError):
    pass


def parse_header(text, where=HEADER):
    """C declarations `ret dgg_name(params);` -> {name: (restype, [argtypes])}.  Any pointer is a c_void_p; a type outside _C_TYPES /
    _C_RETURNS is an error naming the declaration, never a guess."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = "\n".join(line for line in text.split("\n") if not line.lstrip().startswith("#"))
    decls = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s*]*?)\b(dgg_\w+)\s*\(([^()]*)\)\s*;", text):
        decl = " ".join(f"{ret}{name}({params})".split())
        ret = " ".join(ret.split())
        if ret not in _C_RETURNS:
            raise DggHipError(f"{where}: return type {ret!r} has no ctypes mapping: {decl}")
        argtypes = []
        for param in ([] if params.strip() == "void" else params.split(",")):
            words = [w for w in param.split() if w != "const"]             # `type name` or a bare `type`
            if "*" in param:
                argtypes.append(C.c_void_p)
            elif len(words) in (1, 2) and words[0] in _C_TYPES:
                argtypes.append(_C_TYPES[words[0]])
            else:
                raise DggHipError(f"{where}: parameter {' '.join(param.split())!r} has no ctypes mapping: {decl}")
        decls[name] = (_C_RETURNS[ret], argtypes)
    if len(decls) != len(set(re.findall(r"\b(dgg_\w+)\s*\(", text))):
        raise DggHipError(f"{where}: a dgg_* declaration is not of the form `ret dgg_name(params);`")
    return decls


def _read_header(path=HEADER):
    if not os.path.exists(path):
        raise DggHipError(f"{path} is missing: the ctypes prototypes are read from the public header")
    with open(path) as f:
        return parse_header(f.read(), path)


_DECLS = _read_header()
PROTOTYPES = {name: argtypes for name, (_, argtypes) in _DECLS.items() if name not in _INFO}    # name -> argtypes
RESTYPES = {name: restype for name, (restype, _) in _DECLS.items() if name not in _INFO}        # name -> restype


def _read_next_header(path=NEXT_HEADER):
    """dgg_hip_next.h grows one BLOCK of declarations per change, each opened by a line `/* ==== block NAME ==== ... */` (the first block,
    the chunked edge lists, has no such line) -> (declarations of the first block, {NAME: declarations})."""
    if not os.path.exists(path):
        raise DggHipError(f"{path} is missing: the ctypes prototypes are read from the public header")
    with open(path) as f:
        parts = re.split(r"^/\* ==== block (\w+) ====", f.read(), flags=re.M)
    first = parse_header(parts[0], path)
    return first, {name: parse_header("/* " + body, path) for name, body in zip(parts[1::2], parts[2::2])}


_NEXT_DECLS, NEXT_BLOCKS = _read_next_header()
NEXT_PROTOTYPES = {name: argtypes for name, (_, argtypes) in _NEXT_DECLS.items()}               # the same two tables for the entry
NEXT_RESTYPES = {name: restype for name, (restype, _) in _NEXT_DECLS.items()}                   # points of dgg_hip_next.h's first block
_LATER_DECLS = {name: d for block in NEXT_BLOCKS.values() for name, d in block.items()}          # ... and of its later blocks, one table
if set(_NEXT_DECLS) & set(_DECLS) or set(_LATER_DECLS) & (set(_DECLS) | set(_NEXT_DECLS)):
    raise DggHipError(f"{NEXT_HEADER} declares again what {HEADER} or an earlier block of its own declares: "
                      f"{sorted((set(_NEXT_DECLS) | set(_LATER_DECLS)) & set(_DECLS) | set(_LATER_DECLS) & set(_NEXT_DECLS))}")

_ADJ_LOSS_DECLS = _read_header(ADJ_LOSS_HEADER)
ADJ_LOSS_PROTOTYPES = {name: argtypes for name, (_, argtypes) in _ADJ_LOSS_DECLS.items()}       # ... and for dgg_hip_adj_loss.h
ADJ_LOSS_RESTYPES = {name: restype for name, (restype, _) in _ADJ_LOSS_DECLS.items()}
if set(_ADJ_LOSS_DECLS) & (set(_DECLS) | set(_NEXT_DECLS) | set(_LATER_DECLS)):
    raise DggHipError(f"{ADJ_LOSS_HEADER} declares again what {HEADER} or {NEXT_HEADER} declares: "
                      f"{sorted(set(_ADJ_LOSS_DECLS) & (set(_DECLS) | set(_NEXT_DECLS) | set(_LATER_DECLS)))}")

_SAMPLING_DECLS = _read_header(SAMPLING_HEADER)
SAMPLING_PROTOTYPES = {name: argtypes for name, (_, argtypes) in _SAMPLING_DECLS.items()}       # ... and for dgg_hip_sampling.h
SAMPLING_RESTYPES = {name: restype for name, (restype, _) in _SAMPLING_DECLS.items()}
if set(_SAMPLING_DECLS) & (set(_DECLS) | set(_NEXT_DECLS) | set(_LATER_DECLS) | set(_ADJ_LOSS_DECLS)):
    raise DggHipError(f"{SAMPLING_HEADER} declares again what {HEADER}, {NEXT_HEADER} or {ADJ_LOSS_HEADER} declares: "
                      f"{sorted(set(_SAMPLING_DECLS) & (set(_DECLS) | set(_NEXT_DECLS) | set(_LATER_DECLS) | set(_ADJ_LOSS_DECLS)))}")

_BATCH_GRAPH_DECLS = _read_header(BATCH_GRAPH_HEADER)
BATCH_GRAPH_PROTOTYPES = {name: argtypes for name, (_, argtypes) in _BATCH_GRAPH_DECLS.items()}  # ... and for dgg_hip_batch_graph.h
BATCH_GRAPH_RESTYPES = {name: restype for name, (restype, _) in _BATCH_GRAPH_DECLS.items()}
if set(_BATCH_GRAPH_DECLS) & (set(_DECLS) | set(_NEXT_DECLS) | set(_LATER_DECLS) | set(_ADJ_LOSS_DECLS) | set(_SAMPLING_DECLS)):
    raise DggHipError(f"{BATCH_GRAPH_HEADER} declares again what {HEADER}, {NEXT_HEADER}, {ADJ_LOSS_HEADER} or {SAMPLING_HEADER} declares: "
                      f"{sorted(set(_BATCH_GRAPH_DECLS) & (set(_DECLS) | set(_NEXT_DECLS) | set(_LATER_DECLS) | set(_ADJ_LOSS_DECLS) | set(_SAMPLING_DECLS)))}")

_lib = None


def bind(L, names=None):
    """Gives the entry points `names` (default: every declared one, of all five headers) of the CDLL handle L the headers' argtypes and
    restype."""
    decls = {**_DECLS, **_NEXT_DECLS, **_LATER_DECLS, **_ADJ_LOSS_DECLS, **_SAMPLING_DECLS, **_BATCH_GRAPH_DECLS}
    for name in (decls if names is None else names):
        fn = getattr(L, name)      # AttributeError if the library does not export a declared symbol
        fn.restype, fn.argtypes = decls[name]
    return L


def lib():
    """Loads libdgg_hip.so (built by __graft_entry__.build() / csrc/Makefile)."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise DggHipError(
                f"{SO_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  This package has no CPU fallback.")
        _lib = bind(C.CDLL(SO_PATH))
    return _lib


def check(code, what):
    if code != 0:
        raise DggHipError(f"{what} failed (code {code}): {lib().dgg_last_error().decode()}")
