"""The ctypes binding is derived from include/speechclip_hip.h by speechclip_plus_amd/_header.py: the reader on small synthetic
headers (every form the real header uses, and what it must refuse), then the binding it gives on the real header.  No GPU."""
import ctypes
from ctypes import POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_uint8, c_uint16, c_uint32, c_void_p

import pytest

from speechclip_plus_amd import _header

SEG = "typedef struct { const int32_t* row0; const int32_t* chunk; int32_t B, rows, max_pitch, reserved; } sc_segments;\n"


def test_struct_fields_in_the_three_forms():
    h = _header.parse("""
        typedef uint16_t sc_bf16;
        typedef struct {
            const float *g1, *b1; float *out1, *xhat1;
            int32_t B, rows, max_pitch, reserved;
            void* C; int64_t ldc;
            const sc_bf16* A; sc_bf16 raw; float eps; uint32_t seed;
        } sc_demo_args;""", {"sc_demo_args": "DemoArgs"})
    cls = h.structs["sc_demo_args"]
    assert cls.__name__ == "DemoArgs" and issubclass(cls, ctypes.Structure)
    assert cls._fields_ == [("g1", c_void_p), ("b1", c_void_p), ("out1", c_void_p), ("xhat1", c_void_p),
                            ("B", c_int32), ("rows", c_int32), ("max_pitch", c_int32), ("reserved", c_int32),
                            ("C", c_void_p), ("ldc", c_int64),
                            ("A", c_void_p), ("raw", c_uint16), ("eps", c_float), ("seed", c_uint32)]
    assert cls.ldc.offset == 56 and ctypes.sizeof(cls) == 88          # the C layout: 4 pointers, 4 ints, pointer, int64, ...


def test_prototype_forms_and_return_types():
    h = _header.parse("""
        #ifndef DEMO_H
        #define DEMO_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        typedef uint16_t sc_bf16;
        const char* sc_last_error(void);
        int sc_three_lines(const sc_bf16* x, int64_t ldx,
                           float* y /*[rows, D]*/, double beta,
                           const uint8_t* mask, uint64_t n, int flag, void* stream);
        int64_t sc_bytes(int32_t what, int64_t a);
        uint32_t sc_hash(uint32_t x);
        int32_t sc_count(const float* w0 /*[C,10]*/, float /*device scalar*/ * t);
        #ifdef __cplusplus
        }
        #endif
        #endif""")
    assert list(h.functions) == ["sc_last_error", "sc_three_lines", "sc_bytes", "sc_hash", "sc_count"]      # header order
    assert h.functions["sc_last_error"] == (c_char_p, [])
    assert h.functions["sc_three_lines"] == (c_int32, [c_void_p, c_int64, c_void_p, c_double, c_void_p, ctypes.c_uint64, c_int32, c_void_p])
    assert h.functions["sc_bytes"] == (c_int64, [c_int32, c_int64])
    assert h.functions["sc_hash"] == (c_uint32, [c_uint32])
    assert h.functions["sc_count"] == (c_int32, [c_void_p, c_void_p])
    assert h.defines == {} and h.structs == {}                         # an include guard defines no integer


def test_struct_pointers_as_parameter_and_as_field():
    h = _header.parse(SEG + """
        typedef struct { const float* x; const sc_segments* seg; int32_t n, pad_; } sc_layer_args;
        int sc_run(const float* x, const sc_segments* seg, int32_t n, void* stream);
        int sc_layer(const sc_layer_args* args, void* stream);""", {"sc_segments": "Segments"})
    Segments, Layer = h.structs["sc_segments"], h.structs["sc_layer_args"]
    assert Segments.__name__ == "Segments" and Layer.__name__ == "sc_layer_args"
    assert Segments._fields_ == [("row0", c_void_p), ("chunk", c_void_p), ("B", c_int32), ("rows", c_int32), ("max_pitch", c_int32),
                                 ("reserved", c_int32)]
    assert dict(Layer._fields_)["seg"] is POINTER(Segments)
    assert h.functions["sc_run"][1][1] is POINTER(Segments)
    assert h.functions["sc_layer"][1] == [POINTER(Layer), c_void_p]


def test_host_pointers_are_typed_by_their_scalar():
    h = _header.parse("int sc_stats(const float* x, const int32_t* cols_host, int32_t n, const float* scale_host, const int32_t* hosts);")
    assert h.functions["sc_stats"][1] == [c_void_p, POINTER(c_int32), c_int32, POINTER(c_float), c_void_p]


def test_comments_declare_nothing():
    h = _header.parse("""
        /* a comment with ; and ( and { and a prototype:  int sc_fake(int32_t a);
         * typedef struct { int32_t a; } sc_fake_args;   #define SC_FAKE 3   // nested */
        // int sc_fake2(void);  /* not opened
        #define SC_ROWS 8      /* 8 rows; (a chunk) { */
        #define SC_MASK 0x40   // hex
        int sc_real(int32_t a /* ; ( { int sc_fake3(void); */, void* stream);   /* two
        lines; */ int sc_real2(void);""")
    assert list(h.functions) == ["sc_real", "sc_real2"] and h.structs == {}
    assert h.functions["sc_real"] == (c_int32, [c_int32, c_void_p])
    assert h.defines == {"SC_ROWS": 8, "SC_MASK": 64}


@pytest.mark.parametrize("text, quoted", [
    ("int sc_f(const float* x, size_t n, void* stream);", "size_t n"),                     # a type the header does not use
    ("int sc_f(const sc_nothing_args* args, void* stream);", "const sc_nothing_args* args"),   # a struct nobody declared
    ("typedef struct { const sc_nothing* p; int32_t n; } sc_args;", "const sc_nothing* p"),
    ("int sc_f(void (*cb)(int), int32_t n);", "int sc_f(void (*cb)(int), int32_t n);"),      # a function pointer
    ("int sc_f(void);\nint x", "int x"),                                                      # no ';': residue
    ("int sc_f(void);\nint x\n", "int x"),
    ("int sc_f(int32_t n) { return n; }", "int sc_f(int32_t n) { return n;"),                # a definition
    ("void sc_f(int32_t n);", "void"),                                                        # no such return type in the header
    ("int sc_f(float** p);", "float** p"),
    ("int sc_f(int32_t a[4]);", "int32_t a[4]"),
    ("int sc_f(sc_segments seg);", "sc_segments seg"),                                        # a struct by value
    ("int sc_f(void* p_host);", "void* p_host"),                                              # a host array of what?
    ("int sc_f();", "int sc_f();"),
    ("int sc_f(void);\nint sc_f(void);", "int sc_f(void);"),                                  # declared twice
    ("typedef struct { int32_t n : 3; } sc_args;", "int32_t n : 3"),
    ("typedef struct { int32_t n; float x } sc_args;", "float x"),
    ("typedef unsigned sc_u;", "unsigned"),
    ("struct sc_s { int32_t n; };", "struct sc_s { int32_t n;"),
    ("}", "}"),
    ('extern "C" {\nint sc_f(void);', "never closed"),
    ("#define SC_N (1 << 3)", "#define SC_N (1 << 3)"),
    ("#define SC_F(x) 1", "#define SC_F(x) 1"),
    ("#if 1\nint sc_f(void);\n#else\nint sc_f(int32_t n);\n#endif", "#if 1"),
    ("#pragma once", "#pragma once"),
])
def test_what_the_reader_does_not_understand_raises_and_is_quoted(text, quoted):
    with pytest.raises(_header.HeaderError) as e:
        _header.parse(SEG + text)
    assert quoted in str(e.value), str(e.value)


def test_missing_header_names_the_path(tmp_path):
    with pytest.raises(RuntimeError, match="no_such_header.h"):
        _header.read(str(tmp_path / "no_such_header.h"))


# ---- the real header

NOT_INT = {"sc_last_error": c_char_p, "sc_hash32": c_uint32, "sc_infonce_workspace_floats": c_int64, "sc_workspace_bytes": c_int64,
           "sc_sizeof": c_int64, "sc_supcon_workspace_floats": c_int64}


def test_every_declared_function_is_bound_with_the_headers_types():
    from speechclip_plus_amd import _lib
    fns = _lib.HEADER.functions
    assert len(fns) == 139 and set(_lib.SIGNATURES) | set(NOT_INT) == set(fns) and not set(_lib.SIGNATURES) & set(NOT_INT)
    assert {n: r for n, (r, _) in fns.items() if r is not c_int32} == NOT_INT
    assert type(_lib.SIGNATURES) is dict and all(type(a) is list for a in _lib.SIGNATURES.values())
    lib = _lib.lib()
    for name, (restype, argtypes) in fns.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # spot checks against the header text: a struct pointer, the one _host array, an int64 stride between pointers, doubles
    assert _lib.SIGNATURES["sc_gemm_bf16"] == [POINTER(_lib.GemmArgs), c_void_p]
    assert _lib.SIGNATURES["sc_vq_rowstats"][5] is POINTER(c_int32)
    assert _lib.SIGNATURES["sc_wav_prep"][:7] == [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, POINTER(_lib.Segments)]
    assert _lib.SIGNATURES["sc_adam_f32"][5:8] == [c_float, c_double, c_double]
    assert fns["sc_workspace_bytes"][1] == [c_int32, c_int64, c_int64, c_int64]
    assert _lib.SIGNATURES["sc_image_resample_h_u8"][0] is c_void_p and c_uint8 not in _lib.SIGNATURES["sc_image_resample_h_u8"]


def test_the_six_structs_keep_their_names_and_the_sizeof_order():
    from speechclip_plus_amd import _lib
    names = ["GemmArgs", "HubertLayerArgs", "RtGemmArgs", "RtLnArgs", "RtLnBwdArgs", "Segments"]
    assert [c.__name__ for c in _lib.STRUCTS] == names == list(_lib.STRUCT_NAMES.values())
    assert all(getattr(_lib, n) is c for n, c in zip(names, _lib.STRUCTS))
    lib = _lib.lib()
    assert [lib.sc_sizeof(i) for i in range(6)] == [ctypes.sizeof(c) for c in _lib.STRUCTS] == [312, 312, 208, 152, 104, 32]
    assert dict(_lib.HubertLayerArgs._fields_)["seg"] is POINTER(_lib.Segments)
    g = dict(_lib.GemmArgs._fields_)
    assert (g["drop_p"], g["drop_seed"], g["ldc"], g["M"], g["A"]) == (c_float, c_uint32, c_int64, c_int32, c_void_p)
    assert [n for n, _ in _lib.RtLnArgs._fields_][9:19] == ["g1", "b1", "out1", "xhat1", "rstd1", "g2", "b2", "out2", "xhat2", "rstd2"]


def test_the_defines_and_their_python_twins():
    from speechclip_plus_amd import _lib, clip_image, ops
    assert _lib.DEFINES == {"SC_SEG_ROWS": 8, "SC_ATTN_SLACK": 64, "SC_CONV0_NSTAT": 66, "SC_WS_INFONCE": 0, "SC_WS_HUBERT_LAYER": 1,
                            "SC_SUPCON_MAX_LOGIT_BYTES": 1 << 30}
    assert ops.RowSegments.GRAN == clip_image.SEG_ROWS == _lib.DEFINES["SC_SEG_ROWS"] == 8
    assert ops.ATTN_SLACK == _lib.DEFINES["SC_ATTN_SLACK"] == 64
