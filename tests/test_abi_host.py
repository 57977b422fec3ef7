"""CPU: include/dcamd.h is the one declaration of the C-ABI and _lib builds the ctypes binding from it.  The layout of every derived
struct is held against what the host C compiler makes of the header, the reader refuses what it does not read, and the naming rule of the
plan ops and the constants are pinned to literals."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from diffusion_classifier_amd import _lib as L
from diffusion_classifier_amd import plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "dcamd.h")).read()


def _c_compiler():
    for cc in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang"):
        path = shutil.which(cc)
        if path:
            return path
    pytest.fail("no host C compiler found (cc, gcc, clang, /opt/rocm/llvm/bin/clang): the layout of the binding cannot be checked")


def test_layout_of_every_struct_is_the_host_compilers(tmp_path):
    """sizeof of every struct and offsetof / size of every field, as a C program that includes dcamd.h prints them, against the ctypes
    classes.  Compiled as C: the header stands on its own."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "dcamd.h"', "int main(void) {"]
    for struct, fields in L.ABI.structs.items():
        lines.append(f'  printf("{struct} %zu\\n", sizeof({struct}));')
        for name, _, _ in fields:
            lines.append(f'  printf("{struct}.{name} %zu %zu\\n", offsetof({struct}, {name}), sizeof((({struct}*)0)->{name}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([_c_compiler(), "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    theirs = {key: tuple(map(int, nums)) for key, *nums in (line.split() for line in out.splitlines())}
    ours = {}
    for struct, fields in L.ABI.structs.items():
        cls = L.STRUCTS[struct]
        assert cls is getattr(L, L.class_name(struct))
        assert [n for n, _ in cls._fields_] == [n for n, _, _ in fields]
        ours[struct] = (ctypes.sizeof(cls),)
        for name, _, _ in fields:
            ours[f"{struct}.{name}"] = (getattr(cls, name).offset, getattr(cls, name).size)
    assert len(L.ABI.structs) == 32 and len(ours) == len(theirs)
    assert ours == theirs, {k: (ours.get(k), theirs.get(k)) for k in set(ours) | set(theirs) if ours.get(k) != theirs.get(k)}


def test_field_and_parameter_types():
    """Scalars by their C type; a pointer to one of the header's own structs is typed, every other pointer is a c_void_p."""
    scalar = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}
    for struct, fields in L.ABI.structs.items():
        for (name, ctype, is_ptr), (_, t) in zip(fields, L.STRUCTS[struct]._fields_):
            assert is_ptr == ctype.endswith("*")
            if not is_ptr:
                assert t is scalar[ctype], (struct, name)
            elif struct != "dc_conv3_pn_tail_op":
                assert t is ctypes.c_void_p, (struct, name)
    assert L.Conv3PnTailOp._fields_ == [("conv", ctypes.POINTER(L.IgemmParams)), ("tail", ctypes.POINTER(L.PnTailParams))]
    assert (L.i32, L.i64, L.u64, L.f32, L.vp) == (ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_void_p)
    lib = L.lib()
    assert lib.dc_igemm.argtypes == [ctypes.POINTER(L.IgemmParams), ctypes.c_void_p] and lib.dc_igemm.restype is ctypes.c_int
    assert lib.dc_conv3_pn_tail_ring_floats.argtypes == [ctypes.POINTER(L.IgemmParams), ctypes.POINTER(L.PnTailParams)]
    assert lib.dc_conv3_pn_tail_ring_floats.restype is ctypes.c_int64
    assert lib.dc_igemm_variant.restype is ctypes.c_char_p and lib.dc_last_error.argtypes == []
    assert lib.dc_philox_normal.argtypes == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    assert lib.dc_run_plan.argtypes == [ctypes.POINTER(L.Op), ctypes.c_int32, ctypes.c_void_p]
    assert lib.dc_stage_stop.argtypes[5] is ctypes.c_float
    # int32_t* geom takes a ctypes array or NULL
    geom = (ctypes.c_int32 * 14)(*([-1] * 14))
    assert lib.dc_igemm_instance(L.IgemmParams(), geom) == lib.dc_igemm_instance(L.IgemmParams(), None)


def test_the_real_header_parses_to_its_counts():
    """Update these counts only together with an ABI bump."""
    h = L.parse_header(HDR)
    assert h == L.ABI
    assert (len(h.structs), len(h.functions), len(h.enums["dc_op_kind"])) == (32, 77, 23)
    assert L.EXPORTS == list(h.functions) and len(set(L.EXPORTS)) == 77
    assert h.handles == {"dc_stream"}
    assert h.structs["dc_op"] == [("kind", "int32_t", False), ("pad_", "int32_t", False), ("params", "const void*", True)]
    assert h.functions["dc_igemm_instance"] == ("const char*", ["const dc_igemm_params*", "int32_t*"])
    assert h.functions["dc_pn_timeouts"] == ("int32_t", [])
    assert h.enums["dc_status"] == dict(DC_OK=0, DC_ERR_ARG=-1, DC_ERR_SHAPE=-2, DC_ERR_DTYPE=-3, DC_ERR_ALIGN=-4, DC_ERR_LAUNCH=-5,
                                        DC_ERR_UNSUPPORTED=-6)


OK = "typedef struct { const float* x; int32_t n, m; float* y; } dc_a_params;\nint dc_a(const dc_a_params* p, dc_stream s);\n"
PRE = "typedef void* dc_stream;\n"
REFUSED = {
    "array field": PRE + "typedef struct { int32_t dims[4]; } dc_a_params;",
    "array in a later declarator": PRE + "typedef struct { int32_t n, dims[4]; } dc_a_params;",
    "bit-field": PRE + "typedef struct { int32_t flag : 1; } dc_a_params;",
    "nested struct": PRE + "typedef struct { struct { int32_t a; } in; int32_t b; } dc_a_params;",
    "by-value struct": PRE + "typedef struct { int32_t a; } dc_a_params;\ntypedef struct { dc_a_params in; } dc_b_params;",
    "unknown scalar type": PRE + "typedef struct { double x; } dc_a_params;",
    "unsigned 32-bit scalar": PRE + "typedef struct { uint32_t x; } dc_a_params;",
    "two-word scalar": PRE + "typedef struct { unsigned int x; } dc_a_params;",
    "pointer among several declarators": PRE + "typedef struct { float* x, y; } dc_a_params;",
    "pointer to pointer": PRE + "typedef struct { float** x; } dc_a_params;",
    "function-pointer field": PRE + "typedef struct { void (*cb)(int32_t); } dc_a_params;",
    "function-pointer parameter": PRE + "int dc_a(void (*cb)(int32_t), dc_stream s);",
    "by-value struct parameter": PRE + "typedef struct { int32_t a; } dc_a_params;\nint dc_a(dc_a_params p, dc_stream s);",
    "unknown return type": PRE + "double dc_a(dc_stream s);",
    "struct return type": PRE + "typedef struct { int32_t a; } dc_a_params;\ndc_a_params dc_a(void);",
    "enum without values": "typedef enum { DC_A, DC_B } dc_e;",
    "named struct": "struct dc_a { int32_t a; };",
    "union": "typedef union { int32_t a; float b; } dc_u;",
    "global variable": "extern int32_t dc_count;",
    "define of an expression": "#define DC_N (1 << 4)",
    "define of a name": "#define DC_N DC_M",
    "function-like macro": "#define DC_F(x) 3",
    "unknown directive": "#pragma pack(1)",
}


def test_reader_reads_the_supported_grammar():
    h = L.parse_header("/* c */ #define DC_N 0x10\n#define DC_V 2.5f // tail\n" + PRE + OK + "typedef enum { DC_A = 1, DC_B = -2 } dc_e;\n"
                       "const char* dc_name(void);\nvoid dc_none(int64_t n, float /* unnamed */);\n")
    assert h.defines == dict(DC_N=16, DC_V=2.5) and h.enums == dict(dc_e=dict(DC_A=1, DC_B=-2))
    assert h.structs == dict(dc_a_params=[("x", "const float*", True), ("n", "int32_t", False), ("m", "int32_t", False), ("y", "float*", True)])
    assert h.functions == dict(dc_a=("int", ["const dc_a_params*", "dc_stream"]), dc_name=("const char*", []),
                               dc_none=("void", ["int64_t", "float"]))


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_reader_refuses(what):
    with pytest.raises(L.HeaderError, match="dcamd.h"):
        L.parse_header(REFUSED[what])


def test_a_missing_header_says_where_it_was_looked_for(monkeypatch, tmp_path):
    assert os.path.samefile(L.HEADER_PATH, os.path.join(ROOT, "include", "dcamd.h"))
    monkeypatch.setattr(L, "HEADER_PATH", str(tmp_path / "include" / "dcamd.h"))
    with pytest.raises(L.DcamdError, match=re.escape(str(tmp_path))):
        L._read_header()


def test_every_op_kind_has_its_entry_and_its_struct():
    """DC_OP_FOO <-> dc_foo <-> dc_foo_params; DC_OP_CONV3_PN_TAIL -> dc_conv3_pn_tail_op is the one exception."""
    kinds = L.ABI.enums["dc_op_kind"]
    assert sorted(kinds.values()) == list(range(1, 24)) and set(L.OP_ENTRY) == set(L.OP_PARAMS) == set(kinds.values())
    for name, kind in kinds.items():
        fn = "dc_" + name[len("DC_OP_"):].lower()
        assert L.OP_ENTRY[kind] == fn and fn in L.ABI.functions and hasattr(L.lib(), fn)
        struct = "dc_conv3_pn_tail_op" if name == "DC_OP_CONV3_PN_TAIL" else fn + "_params"
        assert L.OP_PARAMS[kind] is L.STRUCTS[struct]
        if name != "DC_OP_CONV3_PN_TAIL":
            assert L.ABI.functions[fn] == ("int", [f"const {struct}*", "dc_stream"])
    assert L.ABI.functions["dc_conv3_pn_tail"] == ("int", ["const dc_igemm_params*", "const dc_pn_tail_params*", "dc_stream"])
    assert L.OP_PARAMS[L.OP_IGEMM] is L.IgemmParams and L.OP_PARAMS[L.OP_CONV3_PN_TAIL] is L.Conv3PnTailOp


def test_variant_of_names_declared_functions():
    assert plan.VARIANT_OF == {
        L.OP_IGEMM: ("dc_igemm_variant", "family"), L.OP_ATTENTION: ("dc_attention_variant", "variant"),
        L.OP_ATTENTION_WIDE: ("dc_attention_wide_variant", "variant"), L.OP_ATTENTION_CAUSAL: ("dc_attention_causal_variant", "variant"),
        L.OP_ATTENTION_BIAS: ("dc_attention_bias_variant", "variant"), L.OP_CROSS_ATTENTION: ("dc_cross_attention_variant", "variant"),
        L.OP_CROSS_ATTENTION_LEN: ("dc_cross_attention_len_variant", "variant"), L.OP_GROUPNORM: ("dc_groupnorm_variant", "variant"),
        L.OP_LAYERNORM: ("dc_layernorm_variant", "variant")}
    for kind, (fn, _) in plan.VARIANT_OF.items():
        assert L.ABI.functions[fn] == ("const char*", [f"const {L.OP_ENTRY[kind]}_params*"]) and hasattr(L.lib(), fn)


def test_constants_against_literals():
    ops = ("QSAMPLE SINUSOID IGEMM GROUPNORM LAYERNORM ATTENTION EPS_MSE TBLOCK_FRONT CROSS_ATTENTION CROSS_ATTENTION_LEN ATTENTION_BIAS RMSNORM "
           "EMBED_ROWS RELU ATTENTION_CAUSAL LAYERNORM_ROWS EMBED_ROWS_POS ACT_PASS ERR_MAP ATTENTION_WIDE IM2COL_S2 CONV3_PN_TAIL "
           "LATENT_IM2COL").split()
    assert [getattr(L, "OP_" + name) for name in ops] == list(range(1, 24))
    assert sorted(n for n in vars(L) if n.startswith("OP_") and isinstance(getattr(L, n), int)) == sorted("OP_" + name for name in ops)
    assert (L.DC_F32, L.DC_BF16, L.DC_F16) == (0, 1, 2)
    assert (L.ACT_NONE, L.ACT_SILU, L.ACT_GEGLU, L.ACT_GELU_TANH) == (0, 1, 2, 3)
    assert (L.PASS_QUICK_GELU, L.PASS_GELU_ERF) == (1, 2)
    assert (L.ATTENTION_BIAS_MAX_L, L.ATTENTION_CAUSAL_MAX_L) == (512, 512)
    assert (L.EVIDENCE_FRAC_BITS, L.EVIDENCE_VMAX) == (30, 16384.0)
    assert type(L.EVIDENCE_FRAC_BITS) is int and type(L.EVIDENCE_VMAX) is float
    assert L.ABI_VERSION == 5 and L.lib().dc_abi_version() == 5
    assert L.ATTENTION_WIDE_DIMS == (256, 512)
