"""CPU: the C-ABI library loads and exports every symbol include/mclstexp_hip.h declares (no compute)."""
import os
import re

import pytest

from conftest import ROOT


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "mclstexp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mcl_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_expected_surface():
    syms = declared_symbols()
    for s in ("mcl_gemm", "mcl_layernorm_fwd", "mcl_layernorm_bwd", "mcl_pos_embed_add_fwd", "mcl_infonce_lse",
              "mcl_infonce_dlogits", "mcl_adam_step", "mcl_adam_table_step"):
        assert s in syms


def test_library_loads_and_exports_every_declared_symbol():
    from mclstexp_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.load()
    assert lib.mcl_abi_version() == _lib.ABI_VERSION
    for s in declared_symbols():
        assert hasattr(lib, s), f"{s} declared in include/mclstexp_hip.h but not exported"
        assert s in _lib.PROTOTYPES, f"{s} has no ctypes prototype in mclstexp_amd/_lib.py"
    assert set(_lib.PROTOTYPES) == set(declared_symbols())
    assert b"invalid" in lib.mcl_error_string(-1)


def test_missing_library_fails_loudly(tmp_path):
    from mclstexp_amd import _lib
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.load(str(tmp_path / "nope.so"))


def test_argument_errors_without_gpu():
    """Argument validation happens before any launch, so it is checkable on CPU."""
    import ctypes as C
    from mclstexp_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.load()
    a = _lib.gemm_args()
    assert lib.mcl_gemm(C.byref(a), None) == -1
    assert lib.mcl_layernorm_fwd(None, 0, None, None, None, 0, None, None, 0, 0, 1e-5, None) == -1
    assert lib.mcl_adam_step(None, None, None, None, 0, 1e-4, .9, .999, 1e-8, 1e-3, .1, .001, None) == -1


# ---------------------------------------------------------------- prototypes: header == ctypes table, type by type
_ARG_KIND = {"int32_t": "i32", "int": "i32", "int64_t": "i64", "uint32_t": "u32", "uint64_t": "u64", "float": "f32",
             "double": "f64", "mcl_stream_t": "stream"}


def header_prototypes():
    """{name: (return kind, [argument kinds])} for every function include/mclstexp_hip.h declares.  Kinds: 'ptr', 'i32'
    (int32_t / int), 'i64', 'u32', 'u64', 'f32', 'f64', 'stream'."""
    text = open(os.path.join(ROOT, "include", "mclstexp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)

    def kind(decl, named):
        decl = " ".join(decl.replace("*", " * ").split())
        if "*" in decl:
            return "ptr"
        words = [w for w in decl.split() if w != "const"]
        if named:
            assert len(words) == 2, f"unnamed or unreadable parameter: {decl!r}"
        return _ARG_KIND[words[0]]

    out = {}
    for ret, name, params in re.findall(r"([\w\s\*]+?)\b(mcl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [q for q in (q.strip() for q in params.split(",")) if q and q != "void"]
        assert name not in out, f"{name} is declared twice"
        out[name] = (kind(ret, False), [kind(q, True) for q in params])
    return out


def table_prototypes(prototypes, restypes):
    """The same description read from the ctypes table (``_lib.PROTOTYPES`` / ``_lib._RESTYPES``)."""
    import ctypes as C
    from mclstexp_amd import _lib
    scalar = {C.c_int32: "i32", C.c_int64: "i64", C.c_uint32: "u32", C.c_uint64: "u64", C.c_float: "f32", C.c_double: "f64"}

    def kind(t):
        if t is _lib.c_s:
            return "stream"
        if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
            return "ptr"
        return scalar[t]
    return {name: (kind(restypes.get(name, C.c_int)), [kind(t) for t in argtypes]) for name, argtypes in prototypes.items()}


def prototype_mismatches(prototypes, restypes):
    want, have = header_prototypes(), table_prototypes(prototypes, restypes)
    bad = [f"{n}: only in {'the header' if n in want else 'PROTOTYPES'}" for n in sorted(set(want) ^ set(have))]
    for n in sorted(set(want) & set(have)):
        (wr, wa), (hr, ha) = want[n], have[n]
        if wr != hr:
            bad.append(f"{n}: returns {wr} in the header, {hr} in _RESTYPES")
        if len(wa) != len(ha):
            bad.append(f"{n}: {len(wa)} arguments in the header, {len(ha)} in PROTOTYPES")
        bad += [f"{n}: argument {i} is {a} in the header, {b} in PROTOTYPES" for i, (a, b) in enumerate(zip(wa, ha)) if a != b]
    return bad


def test_every_prototype_matches_the_header_type_by_type():
    """Argument count, every argument's kind and the return type of all entry points: a c_int32 typed where the header says
    int64_t would truncate silently."""
    from mclstexp_amd import _lib
    want = header_prototypes()
    assert len(want) == len(declared_symbols()) >= 180
    kinds = {k for _, a in want.values() for k in a}
    assert kinds == {"ptr", "i32", "i64", "u32", "u64", "f32", "f64", "stream"}           # (the parser tells them all apart)
    assert prototype_mismatches(_lib.PROTOTYPES, _lib._RESTYPES) == []
    # a stream is always the last argument, and only there: _lib.call appends it
    for name, (_, args) in want.items():
        assert "stream" not in args[:-1], name
    # every status-returning entry point enqueues work and takes the stream, no value-returning one does; the stream is
    # always typed mcl_stream_t, never spelt as a bare pointer that call() would not recognise
    takes_stream = {n for n, (_, a) in want.items() if a[-1:] == ["stream"]}
    assert takes_stream == set(_lib.PROTOTYPES) - set(_lib._RESTYPES)
    assert len(takes_stream) >= 182 and len(_lib._RESTYPES) >= 44 and len(want) == len(takes_stream) + len(_lib._RESTYPES)
    # (floors, so that the parser cannot match nothing unnoticed; a new entry point raises them without editing this test)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mclstexp_hip.h")).read(), flags=re.S)
    assert re.search(r"\bvoid\s*\*\s*stream\b", text) is None
    # every value-returning entry point is listed in _RESTYPES (call() returns its result instead of checking a status)
    assert {"mcl_abi_version", "mcl_gemm_auto_ksplit", "mcl_proj_head_ksplit", "mcl_topk_rows_max_k"} <= set(_lib._RESTYPES)
    assert {n for n, (r, _) in want.items() if r != "i32"} <= set(_lib._RESTYPES)


def test_prototype_check_catches_a_swapped_int_width():
    """The check itself: c_i and c_l swapped in one row (same count, both integers) must be reported, as must a dropped
    argument, a pointer typed as an integer and a wrong return type."""
    import ctypes as C
    from mclstexp_amd import _lib
    row = _lib.PROTOTYPES["mcl_add_f32"]                       # (void*, void*, void*, int64_t n, stream)
    assert row[3] is _lib.c_l

    def mutated(name, argtypes):
        table = dict(_lib.PROTOTYPES)
        table[name] = argtypes
        return prototype_mismatches(table, _lib._RESTYPES)
    assert mutated("mcl_add_f32", row[:3] + [_lib.c_i] + row[4:]) == ["mcl_add_f32: argument 3 is i64 in the header, i32 in PROTOTYPES"]
    bn = list(_lib.PROTOTYPES["mcl_dense_bn1_bwd"])            # (..., int32_t C, const void* x, int64_t ldx, ...)
    assert (bn[2], bn[4]) == (_lib.c_i, _lib.c_l)
    bn[2], bn[4] = bn[4], bn[2]
    assert mutated("mcl_dense_bn1_bwd", bn) == ["mcl_dense_bn1_bwd: argument 2 is i32 in the header, i64 in PROTOTYPES",
                                                "mcl_dense_bn1_bwd: argument 4 is i64 in the header, i32 in PROTOTYPES"]
    assert mutated("mcl_add_f32", row[:-2] + row[-1:]) != []
    assert mutated("mcl_add_f32", [_lib.c_l] + row[1:]) == ["mcl_add_f32: argument 0 is ptr in the header, i64 in PROTOTYPES"]
    assert mutated("mcl_add_f32", row[:-1] + [_lib.c_p]) == ["mcl_add_f32: argument 4 is stream in the header, ptr in PROTOTYPES"]
    res = dict(_lib._RESTYPES)
    res["mcl_bn_workspace_floats"] = C.c_int32
    assert prototype_mismatches(_lib.PROTOTYPES, res) == ["mcl_bn_workspace_floats: returns i64 in the header, i32 in _RESTYPES"]


# ---------------------------------------------------------------- struct layouts: header == ctypes binding == INTEGRATION.md
_CTYPES_OF = {"int32_t": "c_int", "uint32_t": "c_uint", "int64_t": "c_long", "float": "c_float", "double": "c_double"}


def header_structs():
    """{name: [(field, kind)]} for every ``typedef struct`` in include/mclstexp_hip.h; kind = a C scalar type or 'ptr'."""
    text = open(os.path.join(ROOT, "include", "mclstexp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\w+\s*;", text, flags=re.S):
        fields = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
            ctype, star, names = m.group(2), m.group(3), m.group(4)
            for n in names.split(","):
                n = n.strip()
                ptr = bool(star) or n.startswith("*")
                fields.append((n.lstrip("* "), "ptr" if ptr else ctype))
        out[name] = fields
    return out


def _ctypes_fields(struct):
    import ctypes as C
    res = []
    for n, t in struct._fields_:
        if t is C.c_void_p or (isinstance(t, type) and issubclass(t, C._Pointer)):
            res.append((n, "ptr"))
        else:
            res.append((n, t.__name__))
    return res


def _snippet_struct(path, class_name):
    """Executes the ``class <class_name>(C.Structure)`` block of a markdown document's python snippet; returns the class."""
    text = open(path).read()
    m = re.search(r"^(class " + class_name + r"\(C\.Structure\):.*?)\n\n", text, flags=re.S | re.M)
    assert m, f"{path} holds no ctypes declaration of {class_name}"
    import ctypes as C
    ns = {"C": C, "vp": C.c_void_p, "i32": C.c_int32, "u32": C.c_uint32, "i64": C.c_int64, "f32": C.c_float}
    exec(m.group(1), ns)
    return ns[class_name]


def test_every_header_struct_matches_its_ctypes_declaration():
    import ctypes as C
    from mclstexp_amd import _lib
    bound = {"mcl_gemm_args": _lib.GemmArgs}
    structs = header_structs()
    assert set(structs) == set(bound), "a struct of include/mclstexp_hip.h has no ctypes declaration in mclstexp_amd/_lib.py"
    for name, fields in structs.items():
        want = [(n, "ptr" if k == "ptr" else _CTYPES_OF[k]) for n, k in fields]
        assert _ctypes_fields(bound[name]) == want, name
    lib = _lib.load()
    assert lib.mcl_gemm_args_size() == C.sizeof(_lib.GemmArgs)
    assert lib.mcl_gemm_args_min_size() == _lib.GemmArgs.workspace.offset + C.sizeof(C.c_void_p)


def test_integration_md_struct_is_the_current_layout():
    """INTEGRATION.md section 2's binding, executed: same fields, order and size as the library's struct."""
    import ctypes as C
    from mclstexp_amd import _lib
    doc = _snippet_struct(os.path.join(ROOT, "INTEGRATION.md"), "GemmArgs")
    assert _ctypes_fields(doc) == _ctypes_fields(_lib.GemmArgs)
    assert C.sizeof(doc) == _lib.load().mcl_gemm_args_size()


def test_gemm_args_struct_size_is_honoured():
    """mcl_gemm reads nothing beyond the caller's struct_size: a struct that ends at `workspace` (the ABI-6 fields) passes the
    argument check with garbage behind it, a shorter or unsized one is MCL_EINVAL.  Argument checks only (no GPU)."""
    import ctypes as C
    from mclstexp_amd import _lib
    lib = _lib.load()
    full = _lib.GemmArgs
    short_fields = full._fields_[:[n for n, _ in full._fields_].index("workspace") + 1]

    class Short(C.Structure):
        _fields_ = short_fields

    class Padded(C.Structure):                      # the short struct followed by bytes a stale binding never initialised
        _fields_ = [("a", Short), ("junk", C.c_ubyte * 64)]

    assert C.sizeof(Short) == lib.mcl_gemm_args_min_size()
    fn = lib.mcl_gemm
    fn_short = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)(("mcl_gemm", lib))
    p = Padded()
    C.memset(C.byref(p, C.sizeof(Short)), 0xAB, 64)                    # flt_thr & co would read as wild pointers
    a = p.a
    a.M, a.N, a.K, a.batch = 4, 4, 4, 1
    a.A = a.B = a.C = 0x1000                                            # never dereferenced: the checks below fail first
    a.sAm, a.sAk, a.sBk, a.sBn, a.ldc = 4, 1, 1, 4, 4
    a.compute = 7                                                       # -> MCL_EUNSUPPORTED, after every pointer / filter check
    a.struct_size = C.sizeof(Short)
    assert fn_short(C.addressof(p), None) == -2, "fields beyond struct_size must read as zero (the filter block is not engaged)"
    a.struct_size = C.sizeof(Short) + 64                                # the caller now CLAIMS the junk: filter block engaged -> EINVAL
    assert fn_short(C.addressof(p), None) == -1
    a.struct_size = C.sizeof(Short) - 8
    assert fn_short(C.addressof(p), None) == -1
    a.struct_size = 0
    assert fn_short(C.addressof(p), None) == -1
    g = _lib.gemm_args()
    assert g.struct_size == C.sizeof(full)
    assert fn(C.byref(g), None) == -1                                   # sized, but null operands


def _nm_tool():
    """llvm-nm of the ROCm toolchain that builds the library (next to hipcc), else binutils' nm."""
    import shutil
    hipcc = shutil.which("hipcc")
    if hipcc:
        cand = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", "llvm-nm")
        if os.path.exists(cand):
            return cand
    return shutil.which("llvm-nm") or shutil.which("nm")


def test_library_reads_no_environment():
    """Kernel choice and experiment switches travel through arguments: the shipped library imports no getenv."""
    import subprocess
    from mclstexp_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    nm = _nm_tool()
    assert nm, "no nm / llvm-nm to read the library's symbols"
    out = subprocess.run([nm, "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    undefined = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip()}
    assert "memcpy" in undefined                     # (the listing was read)
    assert not undefined & {"getenv", "secure_getenv"}, sorted(undefined & {"getenv", "secure_getenv"})
