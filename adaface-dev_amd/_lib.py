"""ctypes binding of csrc/libadaface_hip.so, derived from the C ABI's own header (include/adaface_hip.h).

The header is parsed once at import: every ``af_*`` prototype gives the argtypes / restype ``lib()`` sets, the body of ``af_gemm_desc``
gives ``GemmDesc._fields_``, and every ``#define AF_*`` becomes a module attribute.  A new entry point is declared in the header and
defined in a ``.hip`` file; nothing is added here.  The parser reads the small subset of C the header is written in and refuses anything
else: a declaration it cannot read completely stops the import and is named in the error, it is never skipped and no type is guessed.

The product path has NO fallback: if the shared library is missing or a call fails, a
RuntimeError is raised.  ``build()`` (re)compiles the library in-tree with hipcc for gfx950.
"""
import ctypes as C
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "adaface_hip.h")
# AF_LIB: another build of the SAME sources to load instead (measurement only: tools/ab_lib.sh compares two builds of the library, e.g. one compiled
# with other hipcc flags or from the parent commit, in alternating runs on one box).  Unset in every judged run; a missing file fails as loudly as the default path.
LIB_PATH = os.environ.get("AF_LIB") or os.path.join(CSRC, "libadaface_hip.so")


class GemmDesc(C.Structure):
    """af_gemm_desc.  Its _fields_ are the header's struct members, set below."""


# Every type spelling the header may use (one space between words, none before '*') and its ctypes type.
CTYPES = {
    "int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float,
    "void*": C.c_void_p, "const void*": C.c_void_p, "const char*": C.c_char_p,
    "const float*": C.POINTER(C.c_float), "const int*": C.POINTER(C.c_int), "int*": C.POINTER(C.c_int), "double*": C.POINTER(C.c_double),
    "const af_gemm_desc*": C.POINTER(GemmDesc),
}


_DECLARATOR = re.compile(r"(.+?)\b(\w+(?:\s*,\s*\w+)*)")


def _declarator(decl: str, where: str):
    """'const void* a1' -> ('const void*', ['a1']); 'int32_t M, N, K' -> ('int32_t', ['M', 'N', 'K'])."""
    m = _DECLARATOR.fullmatch(decl.strip())
    spelling = " ".join(m.group(1).replace("*", " * ").split()).replace(" *", "*") if m else None
    if spelling not in CTYPES:
        raise RuntimeError(f"adaface_hip.h: cannot read {' '.join(decl.split())!r} in {where!r}: expected '<type> <name>' with a type out of {sorted(CTYPES)}")
    return spelling, [n.strip() for n in m.group(2).split(",")]


def parse_header(text: str):
    """The ABI a header text declares, as spellings: (functions {name: (return type, [parameter types])} in declaration order,
    fields [(member of af_gemm_desc, type)], constants {AF_*: int}).  RuntimeError for anything that is not read completely."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(AF_\w+)(.*)$", text, flags=re.M):
        try:                                                    # an integer, or arithmetic over the constants above it
            if not re.fullmatch(r"[\w\s()*+-]+", value):
                raise ValueError("not integer arithmetic")
            constants[name] = int(eval(value, {"__builtins__": {}}, constants))
        except Exception as e:
            raise RuntimeError(f"adaface_hip.h: cannot read '#define {name}{value}': {e}") from e
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    fields = []
    m = re.search(r"typedef\s+struct\s+af_gemm_desc\s*\{(.*?)\}\s*af_gemm_desc\s*;", text, flags=re.S)
    if m:
        for decl in filter(str.strip, m.group(1).split(";")):
            spelling, names = _declarator(decl, "af_gemm_desc")
            fields += [(n, spelling) for n in names]
        text = text[:m.start()] + text[m.end():]
    functions = {}
    for decl in filter(str.strip, text.split(";")):
        proto = " ".join(decl.split())
        m = re.fullmatch(r"([^()]+)\(([^()]*)\)", proto)
        if not m:
            raise RuntimeError(f"adaface_hip.h: cannot read the declaration {proto!r}")
        ret, names = _declarator(m.group(1), proto)
        if len(names) != 1 or not names[0].startswith("af_") or names[0] in functions:
            raise RuntimeError(f"adaface_hip.h: cannot read the declaration {proto!r}: expected one new af_* function")
        functions[names[0]] = (ret, [] if m.group(2).strip() == "void" else [_declarator(p, proto)[0] for p in m.group(2).split(",")])
    return functions, fields, constants


with open(HEADER) as _f:
    FUNCTIONS, _fields, _constants = parse_header(_f.read())
if not _fields:
    raise RuntimeError("adaface_hip.h: no af_gemm_desc")
GemmDesc._fields_ = [(n, CTYPES[t]) for n, t in _fields]
globals().update(_constants)                                    # AF_OK, AF_E_*, AF_ACT_*, AF_OUT_*, AF_FAM_*, AF_SPLITK_*, ...
EXPORTS = tuple(FUNCTIONS)                                      # every symbol the header declares (tests check the .so exports exactly these)


def _csrc_sha() -> str:
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    files += [os.path.join(CSRC, "Makefile"), HEADER]
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def build(verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 into csrc/libadaface_hip.so (make, in-tree).  The objects are stamped with a hash
    of ALL sources: if the stamp does not match the tree (a stale or foreign .o / .so), everything is rebuilt from scratch;
    otherwise make's incremental rules decide."""
    stamp = os.path.join(CSRC, ".build_sha")
    want = _csrc_sha()
    have = open(stamp).read().strip() if os.path.exists(stamp) else ""
    cmd = ["make", "-C", CSRC, "-j8"] + ([] if have == want and os.path.exists(LIB_PATH) else ["-B"])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libadaface_hip.so failed:\n" + r.stdout + r.stderr)
    with open(stamp, "w") as f:
        f.write(want)
    if verbose:
        print(r.stdout)
    return LIB_PATH


def sources_sha() -> str:
    """Hash of everything that decides what the GEMM family executes (kernel sources + the tuned tile table).  Measurements
    that cannot be taken in-process (PMC traffic) record it, and bench.py reports them only while it still matches."""
    import hashlib
    h = hashlib.sha256()
    for rel in ("csrc/af_common.h", "csrc/af_gemm.hip", "csrc/af_gemm3.hip", "csrc/af_runtime.hip", "tuning/gfx950_gemm.json"):
        with open(os.path.join(_HERE, rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


_lib = None


def lib() -> C.CDLL:
    """Load (once) and return the library; raise loudly if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64; it must be the HIP runtime of this process, so load it
    # first (the .so then binds to the already-loaded runtime instead of a second copy).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback). "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C adaface-dev_amd/csrc`."
        )
    L = C.CDLL(LIB_PATH)
    for name, (ret, params) in FUNCTIONS.items():
        f = getattr(L, name)
        f.restype, f.argtypes = CTYPES[ret], [CTYPES[p] for p in params]
    _lib = L
    return L


def check(rc: int, what: str) -> None:
    if rc < 0:
        msg = lib().af_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")
