"""The Python binding's prototype table (basevarc_amd.lib.PROTOTYPES) against include/bvc.h, without a device: the same functions, the
same number of parameters, pointers bound as pointers, every integer and double with the header's width and signedness, the same
return types; and bind() resolves every required symbol of the built library."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double,
           "int": C.c_int, "size_t": C.c_size_t}
RETURNS = {"int": C.c_int, "void": None, "const char *": C.c_char_p, "void *": C.c_void_p}


def header_declarations():
    """{name: (return type, [parameter text])} of every `<ret> bvc_name(params);` in include/bvc.h."""
    txt = open(os.path.join(ROOT, "include", "bvc.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)
    decls = {}
    for ret, name, params in re.findall(r"\b((?:const\s+)?\w+\s*\*?)\s*\b(bvc_\w+)\s*\(([^;{}()]*)\)\s*;", txt):
        params = " ".join(params.split())
        assert name not in decls, name
        decls[name] = (re.sub(r"\s*\*", " *", " ".join(ret.split())), [] if params == "void" else [p.strip() for p in params.split(",")])
    return decls


def is_pointer(ctype):
    return ctype in (C.c_void_p, C.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))


def scalar_of(param):
    """The ctypes type of a by-value parameter such as `int64_t n_sites` or `double min_af`."""
    words = [w for w in param.split() if w != "const"]
    assert len(words) == 2 and words[0] in SCALARS, param
    return SCALARS[words[0]]


def test_the_parser_reads_the_header():
    decls = header_declarations()
    assert decls["bvc_version"] == ("const char *", [])
    assert decls["bvc_host_alloc"] == ("void *", ["size_t bytes"])
    assert decls["bvc_host_free"] == ("void", ["void *p"])
    assert decls["bvc_pileup_finish"][1][3] == "const uint8_t carry_in[5]"
    assert len(decls["bvc_pileup_finish_called_stats"][1]) == 19
    assert not any("typedef" in r or "struct" in r for r, _ in decls.values())


def test_the_table_names_what_the_header_declares():
    from basevarc_amd import lib as bl
    declared = set(header_declarations())
    assert len(declared) == 53
    assert len(bl.EXPORTS) == len(set(bl.EXPORTS))
    assert declared == set(bl.EXPORTS)
    assert list(header_declarations()) == bl.EXPORTS             # the table is in the header's order
    assert declared == set(bl.PROTOTYPES) - {"bvc_debug_report"}
    assert "bvc_debug_report" in bl.PROTOTYPES                  # optional: diagnostic builds only export it


def test_every_prototype_matches_its_declaration():
    from basevarc_amd import lib as bl
    for name, (ret, params) in header_declarations().items():
        restype, argtypes = bl.PROTOTYPES[name]
        assert ret in RETURNS, (name, ret)
        assert restype is RETURNS[ret], (name, ret, restype)
        assert len(argtypes) == len(params), (name, argtypes, params)
        for a, prm in zip(argtypes, params):
            if "*" in prm or re.search(r"\[\d+\]$", prm):
                assert is_pointer(a), (name, prm, a)
            else:
                assert not is_pointer(a) and a is scalar_of(prm), (name, prm, a)


def test_a_slip_in_the_table_would_be_seen():
    """The comparison tells widths and signedness apart (ctypes aliases equal types, e.g. c_int and c_int32: those are one ABI)."""
    assert len({C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_double}) == 5
    assert not is_pointer(C.c_int64) and is_pointer(C.POINTER(C.c_int64)) and is_pointer(C.c_char_p)
    assert scalar_of("uint32_t flags") is not C.c_int


def test_bind_resolves_every_required_symbol():
    from basevarc_amd import build as b
    from basevarc_amd import lib as bl
    b.build(force=b.needs_build())
    # (the symbol table only: loading through basevarc_amd.lib would bring the HIP runtime in, which this test does not need)
    L = bl.bind(C.CDLL(bl.library_path(), mode=os.RTLD_LAZY))
    for name in bl.EXPORTS:
        fn = getattr(L, name)
        assert fn.restype is bl.PROTOTYPES[name][0] and list(fn.argtypes) == bl.PROTOTYPES[name][1], name
