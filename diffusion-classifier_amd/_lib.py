"""ctypes binding of libdcamd.so, built from the one declaration of the C-ABI: include/dcamd.h.

The header is read once at import (parse_header: text in, names out; no compiler, no torch, no library load); the struct classes, the
constants, EXPORTS and every function's argtypes / restype come from it.  A new op is declared in the header and nowhere in here.

The product path has NO fallback: if the HIP library is missing or does not load, every
entry point raises.  Nothing here imports `oracle/`.
"""
import collections
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DCAMD_LIB") or os.path.join(_HERE, "libdcamd.so")   # DCAMD_LIB: diagnostic builds only
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "dcamd.h")

i32, i64, u64, f32, vp = C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_void_p
SCALARS = {"int32_t": i32, "int64_t": i64, "uint64_t": u64, "float": f32}
RETURNS = dict(SCALARS, **{"int": C.c_int, "const char*": C.c_char_p, "void": None})

ATTENTION_WIDE_DIMS = (256, 512)     # head widths of dc_attention_wide


class DcamdError(RuntimeError):
    pass


class HeaderError(ValueError):
    """include/dcamd.h holds a declaration outside the grammar parse_header reads."""


# structs: name -> [(field, C type, is_pointer)]; functions: name -> (return type, [parameter types]); enums: name -> {NAME: value};
# defines: NAME -> int | float; handles: the names typedef-ed to a pointer (dc_stream)
Header = collections.namedtuple("Header", "structs functions enums defines handles")


def _ctype(text, what):
    """'const float * x' -> ('const float*', True, 'x'); anything but [const] NAME [*] [declarator] raises."""
    m = re.fullmatch(r"((?:const\s+)?\w+)\s*(\*?)\s*(\w*)", text.strip())
    if not m or m[1] == "const":
        raise HeaderError(f"dcamd.h: cannot read `{text.strip()}` in {what}")
    return " ".join(m[1].split()) + m[2], bool(m[2]), m[3]


def parse_header(text):
    """The declarations of dcamd.h as a Header.  The grammar is what the header uses — `typedef struct { ... } name;` with scalar
    (SCALARS) or pointer fields and comma-separated declarators, `typedef enum { A = n, ... } name;`, `typedef T* name;`,
    `#define NAME literal` and prototypes returning one of RETURNS — and everything else raises HeaderError: nothing is guessed."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^#ifdef __cplusplus\n.*?^#endif[^\n]*$", "", text, flags=re.S | re.M)
    h = Header({}, {}, {}, {}, set())
    for line in re.findall(r"^\s*#[^\n]*", text, flags=re.M):
        m = re.fullmatch(r"\s*#\s*define\s+(\w+)\s+(\S+)\s*", line)
        if m:
            try:
                h.defines[m[1]] = int(m[2], 0) if re.fullmatch(r"-?\w+", m[2]) else float(m[2].rstrip("fF"))
            except ValueError:
                raise HeaderError(f"dcamd.h: #define {m[1]} is no integer or float literal: `{m[2]}`") from None
        elif not re.fullmatch(r"\s*#\s*(include\s*<\w+\.h>|ifndef\s+\w+|define\s+\w+|endif)\s*", line):
            raise HeaderError(f"dcamd.h: cannot read `{line.strip()}`")
    text = re.sub(r"^\s*#[^\n]*", "", text, flags=re.M)
    for decl in re.split(r";(?![^{}]*\})", text):       # the semicolons outside braces
        decl = decl.strip()
        m = re.fullmatch(r"typedef\s+(struct|enum)\s*\{([^{}]*)\}\s*(\w+)", decl)
        if m and m[1] == "enum":
            h.enums[m[3]] = {}
            for item in filter(None, (s.strip() for s in m[2].split(","))):
                e = re.fullmatch(r"(\w+)\s*=\s*(-?\d+)", item)
                if not e:
                    raise HeaderError(f"dcamd.h: enum {m[3]}: cannot read `{item}` (NAME = integer)")
                h.enums[m[3]][e[1]] = int(e[2])
        elif m:
            fields = h.structs[m[3]] = []
            for item in filter(None, (s.strip() for s in m[2].split(";"))):
                first, *more = item.split(",")
                ctype, is_ptr, name = _ctype(first, f"struct {m[3]}")
                names = [name] + [s.strip() for s in more]
                if not all(re.fullmatch(r"\w+", n) for n in names) or (is_ptr and more) or not (is_ptr or ctype in SCALARS):
                    raise HeaderError(f"dcamd.h: struct {m[3]}: cannot read `{item}` (a scalar of {sorted(SCALARS)} or one pointer)")
                fields += [(n, ctype, is_ptr) for n in names]
        elif re.fullmatch(r"typedef\s+\w+\s*\*\s*\w+", decl):
            h.handles.add(decl.split("*")[1].strip())
        elif decl:
            m = re.fullmatch(r"([\w\s]+?\*?)\s*\b(\w+)\s*\((.*)\)", decl, flags=re.S)
            ret = m and re.sub(r"\s*\*", "*", " ".join(m[1].split()))
            if not m or ret not in RETURNS:
                raise HeaderError(f"dcamd.h: cannot read the declaration `{' '.join(decl.split())[:120]}`")
            params = []
            for item in ([] if m[3].strip() == "void" else m[3].split(",")):
                ctype, is_ptr, _ = _ctype(item, f"the prototype of {m[2]}")
                if not (is_ptr or ctype in SCALARS or ctype in h.handles):
                    raise HeaderError(f"dcamd.h: {m[2]}: parameter `{item.strip()}` is neither a scalar nor a pointer")
                params.append(ctype)
            h.functions[m[2]] = (ret, params)
    return h


def _read_header():
    try:
        with open(HEADER_PATH) as fh:
            return parse_header(fh.read())
    except OSError as e:
        raise DcamdError(f"the C-ABI declaration include/dcamd.h was looked for at {HEADER_PATH} and cannot be read ({e}); "
                         "the binding is built from it, the package does not work without its source tree") from None


ABI = _read_header()


def class_name(struct):
    """dc_x_y_params -> XYParams, dc_op -> Op, dc_conv3_pn_tail_op -> Conv3PnTailOp."""
    return "".join(w.capitalize() for w in struct.split("_")[1:])


def _pointer(ctype):
    """A pointer to one of the header's own structs is typed; every other pointer (and dc_stream) is a c_void_p."""
    cls = STRUCTS.get(ctype.replace("const ", "").rstrip("*"))
    return C.POINTER(cls) if cls else vp


STRUCTS = {}        # header name -> ctypes class, also module attributes under class_name()
for _name, _fields in ABI.structs.items():
    STRUCTS[_name] = type(class_name(_name), (C.Structure,), {"_fields_": [(n, _pointer(t) if p else SCALARS[t]) for n, t, p in _fields]})
    globals()[class_name(_name)] = STRUCTS[_name]

# DC_ABI_VERSION -> ABI_VERSION, DC_ACT_SILU -> ACT_SILU, DC_OP_IGEMM -> OP_IGEMM, DC_PASS_GELU_ERF -> PASS_GELU_ERF; the dtypes keep DC_
globals().update(ABI.enums["dc_dtype"])
for _consts in (ABI.defines, ABI.enums["dc_act"], ABI.enums["dc_pass_kind"], ABI.enums["dc_op_kind"]):
    globals().update({k[3:]: v for k, v in _consts.items() if k.startswith("DC_")})

# every symbol include/dcamd.h declares (tests check that the library exports all of them)
EXPORTS = list(ABI.functions)

# The naming rule of the plan ops: DC_OP_FOO is launched by dc_foo on a dc_foo_params.  One exception: DC_OP_CONV3_PN_TAIL points to a
# dc_conv3_pn_tail_op (two structs behind one op record).
OP_ENTRY, OP_PARAMS = {}, {}      # op kind -> entry function name / params class
for _kind, _value in ABI.enums["dc_op_kind"].items():
    _fn = "dc_" + _kind[len("DC_OP_"):].lower()
    _struct = "dc_conv3_pn_tail_op" if _kind == "DC_OP_CONV3_PN_TAIL" else _fn + "_params"
    if _fn not in ABI.functions or _struct not in STRUCTS:
        raise HeaderError(f"dcamd.h: {_kind} needs the function {_fn} and the struct {_struct}")
    OP_ENTRY[_value], OP_PARAMS[_value] = _fn, STRUCTS[_struct]

_lib = None


def lib():
    """Load libdcamd.so once.  Raises (never falls back) when the extension is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DcamdError(
            f"HIP extension {LIB_PATH} is missing — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C diffusion-classifier_amd/csrc`). There is no CPU fallback for the scoring path.")
    L = C.CDLL(LIB_PATH)
    for name, (ret, params) in ABI.functions.items():
        fn = getattr(L, name)
        fn.argtypes = [SCALARS[t] if t in SCALARS else _pointer(t) for t in params]
        fn.restype = RETURNS[ret]
    if L.dc_abi_version() != ABI_VERSION:
        raise DcamdError(f"libdcamd ABI {L.dc_abi_version()} != {ABI_VERSION} (stale libdcamd.so? rebuild with `make -C diffusion-classifier_amd/csrc`)")
    _lib = L
    return L


def check(rc, what=""):
    if rc != 0:
        raise DcamdError(f"{what} failed (status {rc}): {lib().dc_last_error().decode()}")


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise DcamdError("the diffusion-classifier scoring path needs an MI355X (HIP device); no CPU fallback exists")
    return lib()
