"""The C-ABI library builds for gfx950, loads without a GPU and exports every symbol that
include/rc_abi.h declares (no compute calls here)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rc_abi.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rc_[a-z_0-9]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from nrc_amd import rc_ext
    return rc_ext.load_library()


def test_header_symbols_are_exported(lib):
    names = _declared()
    assert "rc_render_rays" in names and "rc_create" in names and len(names) >= 12
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


def test_binding_covers_header(lib):
    from nrc_amd import rc_ext
    assert set(_declared()) == set(rc_ext.EXPORTS)
    assert lib.rc_abi_version() == rc_ext.RC_ABI_VERSION


def _c_class(decl):
    """Width class of one C parameter or return type of the header: ptr, i32, u32, i64, f32 or void."""
    if "*" in decl or "[" in decl:
        return "ptr"
    words = [w for w in decl.split() if w != "const"]
    return {"int": "i32", "int32_t": "i32", "uint32_t": "u32", "int64_t": "i64", "float": "f32", "void": "void"}[words[0]]


def _ctypes_class(t):
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "ptr"
    return {ctypes.c_int32: "i32", ctypes.c_uint32: "u32", ctypes.c_int64: "i64", ctypes.c_float: "f32"}[t]


def _header_prototypes():
    """name -> (class of the return type, [class per parameter]) of every rc_*(...) declaration of the header."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    protos = {}
    for ret, name, params in re.findall(r"^[ \t]*((?:const[ \t]+)?\w+[ \t]*\*?)[ \t]*\b(rc_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", src, flags=re.M):
        params = [p.strip() for p in params.split(",")]
        args = [] if params == ["void"] else [_c_class(p) for p in params]
        assert name not in protos, name
        protos[name] = (_c_class(ret), args)
    return protos


def test_prototype_table_matches_header():
    """Every ctypes prototype of the binding against the header's declaration: the same number of arguments, and per
    position (and for the return value) the same class -- pointer, int32, uint32, int64, float, void.  A wrong width or a
    dropped argument corrupts a call without any error."""
    from nrc_amd import rc_ext
    header = _header_prototypes()
    assert set(header) == set(_declared())                    # the parser saw every declaration
    assert "ptr" == header["rc_last_error"][0] and header["rc_prng_fill"][1][1] == "ptr"       # const char*, key[2]
    for name, (ret, args) in header.items():
        assert name in rc_ext._PROTOTYPES, f"{name}: no row in the prototype table"
        restype, argtypes = rc_ext._PROTOTYPES[name]
        assert _ctypes_class(restype) == ret, (name, "return", ret)
        assert [_ctypes_class(t) for t in argtypes] == args, (name, args)
    assert isinstance(rc_ext.EXPORTS, tuple) and set(rc_ext.EXPORTS) == set(rc_ext._PROTOTYPES)


def test_loaded_library_carries_the_table(lib):
    from nrc_amd import rc_ext
    for name, (restype, argtypes) in rc_ext._PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_struct_layouts_match_c():
    """Every ctypes.Structure of the binding against the header as a C compiler lays it out: sizeof of the struct, offsetof
    and size of each field; and the lengths of the three output tables against RC_OUT_COUNT / RC_MOUT_COUNT /
    RC_TOUT_COUNT."""
    import tempfile
    from nrc_amd import rc_ext
    structs = [v for v in vars(rc_ext).values() if isinstance(v, type) and issubclass(v, ctypes.Structure)
               and v.__module__ == rc_ext.__name__]
    assert len(structs) >= 22 and rc_ext.rc_camera in structs and rc_ext.rc_grad_segment in structs
    lines = ['printf("%d %d %d\\n", (int)RC_OUT_COUNT, (int)RC_MOUT_COUNT, (int)RC_TOUT_COUNT);']
    for s in structs:
        lines.append(f'printf("{s.__name__} %zu\\n", sizeof({s.__name__}));')
        for f, _ in s._fields_:
            lines.append(f'printf("{s.__name__}.{f} %zu %zu\\n", offsetof({s.__name__}, {f}), sizeof((({s.__name__}*)0)->{f}));')
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "rc_abi.h"\nint main(void) {\n  ' + "\n  ".join(lines) + "\n  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, text=True).stdout.splitlines()
    assert [int(x) for x in out[0].split()] == [rc_ext.RC_OUT_COUNT, rc_ext.RC_MOUT_COUNT, rc_ext.RC_TOUT_COUNT]
    c = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out[1:]}
    for s in structs:
        assert c[s.__name__] == [ctypes.sizeof(s)], s.__name__
        for f, _ in s._fields_:
            assert c[f"{s.__name__}.{f}"] == [getattr(s, f).offset, getattr(s, f).size], (s.__name__, f)
    assert len(c) == len(structs) + sum(len(s._fields_) for s in structs)


def test_output_table_matches_header_enum():
    from nrc_amd import rc_ext
    src = open(HEADER).read()
    body = src[src.index("typedef enum {\n  RC_OUT_RGB"):src.index("} rc_output_id;")]
    enum = re.findall(r"RC_OUT_([A-Z_0-9]+)", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    enum = [e for e in enum if e != "COUNT"]
    assert [e.lower() for e in enum] == [n for n, _ in rc_ext.OUTPUTS]


def test_product_fails_loudly_without_library(monkeypatch, tmp_path):
    from nrc_amd import rc_ext
    monkeypatch.setattr(rc_ext, "_LIB", None)
    monkeypatch.setattr(rc_ext, "library_path", lambda: str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rc_ext.load_library()


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "neural-radiance-caching_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "from oracle" not in txt and "import oracle" not in txt, f
