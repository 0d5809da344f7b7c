"""``_lib.call``: the one checked path from Python into the C ABI.  CPU tests (argument checks happen before the library is
touched), a source test (no module reaches the library another way) and two GPU tests (same launch as raw ctypes; a stage
module's launch follows torch's current stream)."""
import ctypes as C
import glob
import os
import re

import pytest
import torch

from conftest import ROOT
from mclstexp_amd import _lib
from mclstexp_amd._lib import call


@pytest.fixture
def untouched(monkeypatch):
    """The library must not be reached: any load or lookup fails the test."""
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_lib, "load", boom)


def test_cpu_tensor_in_a_pointer_slot_is_refused_before_the_library(untouched):
    a, n = torch.zeros(8), 8
    with pytest.raises(RuntimeError, match=r"mcl_add_f32: argument 0 is on cpu"):
        call("mcl_add_f32", a, a, a, n)
    with pytest.raises(RuntimeError, match=r"mcl_layernorm_fwd: argument 3 is on cpu"):        # behind None and numbers too
        call("mcl_layernorm_fwd", None, 0, 64, torch.zeros(4), None, 0, None, None, 0, 0, 1e-5)
    with pytest.raises(RuntimeError, match=r"mcl_add_f32: argument 2 is on meta"):
        call("mcl_add_f32", None, 64, torch.empty(8, device="meta"), n)


def test_tensor_in_a_non_pointer_slot_is_a_type_error(untouched):
    a = torch.zeros(8)
    with pytest.raises(TypeError, match=r"mcl_add_f32: argument 3 is a tensor \(on cpu\)"):
        call("mcl_add_f32", None, None, None, a)
    with pytest.raises(TypeError, match=r"mcl_bn_workspace_floats: argument 0 is a tensor"):
        call("mcl_bn_workspace_floats", torch.tensor(4), 8, 0)


def test_tensor_in_a_host_array_or_struct_slot_is_a_type_error(untouched):
    """The ``POINTER(...)`` slots are read by the library on the host: a tensor there, even a device tensor's address, would
    be dereferenced as a host address."""
    a = torch.zeros(8)
    assert _lib.PROTOTYPES["mcl_gemm"][0] is not C.c_void_p and _lib.PROTOTYPES["mcl_colred_group"][1] is not C.c_void_p
    with pytest.raises(TypeError, match=r"mcl_gemm: argument 0 is a tensor"):
        call("mcl_gemm", a)
    with pytest.raises(TypeError, match=r"mcl_gemm_group: argument 0 is a tensor"):
        call("mcl_gemm_group", a, 1)
    for slot in range(1, 11):
        args = [1] + [None] * 10 + [8]
        args[slot] = a
        with pytest.raises(TypeError, match=rf"mcl_colred_group: argument {slot} is a tensor"):
            call("mcl_colred_group", *args)


def test_wrong_argument_count_names_the_entry_point_and_both_counts(untouched):
    with pytest.raises(TypeError, match=r"mcl_add_f32 takes 4 arguments \(the stream is appended\), 3 given"):
        call("mcl_add_f32", None, None, None)
    with pytest.raises(TypeError, match=r"mcl_add_f32 takes 4 arguments \(the stream is appended\), 5 given"):
        call("mcl_add_f32", None, None, None, 8, None)                      # (passing the stream by hand is one too many)
    with pytest.raises(TypeError, match=r"mcl_edge_agreement takes 8 arguments \(the stream is appended\), 9 given"):
        call("mcl_edge_agreement", None, 1, 4, None, None, None, 2, None, None)     # (so it is for a stage's entry point)
    with pytest.raises(RuntimeError, match=r"mcl_edge_agreement: argument 3 is on cpu"):      # eight pass the count
        call("mcl_edge_agreement", None, 1, 4, torch.zeros(4, dtype=torch.int32), None, None, 2, None)
    with pytest.raises(TypeError, match=r"mcl_bn_workspace_floats takes 3 arguments, 2 given"):
        call("mcl_bn_workspace_floats", 4, 8)
    with pytest.raises(RuntimeError, match="no entry point mcl_nope"):
        call("mcl_nope")


def test_signatures_follow_the_table():
    for name, argtypes in _lib.PROTOTYPES.items():
        nargs, pointer, stream, returns_value = _lib._SIGNATURES[name]
        assert stream == (bool(argtypes) and argtypes[-1] is _lib.c_s) and nargs == len(argtypes) - stream
        assert _lib.c_s not in argtypes[:-1]
        assert returns_value == (name in _lib._RESTYPES)
        assert len(pointer) == nargs
        assert pointer == tuple(t is C.c_void_p for t in argtypes[:nargs]), name
    # every status-returning entry point enqueues work and is handed the stream; no value-returning one is
    streamed = {name for name, s in _lib._SIGNATURES.items() if s[2]}
    assert streamed == set(_lib.PROTOTYPES) - set(_lib._RESTYPES)
    assert len(streamed) >= 182 and len(_lib._RESTYPES) >= 44          # (floors: neither set is quietly empty)


@pytest.fixture
def built():
    """The library, built first where a clean checkout has none yet."""
    if not os.path.exists(_lib.LIB_PATH):
        from mclstexp_amd import build
        build.build(verbose=False)
    return _lib.lib()


class _StubStream:
    cuda_stream, device_index = 0, 0


def test_error_is_raised_under_the_entry_points_own_name(built, monkeypatch):
    """A null-operand call returns MCL_EINVAL before any launch (as in test_argument_errors_without_gpu); the stream handle is
    stubbed because this machine may have no GPU to ask for one."""
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: _StubStream())
    with pytest.raises(RuntimeError, match=r"mclstexp_hip mcl_layernorm_fwd failed: \[-1\] invalid argument"):
        call("mcl_layernorm_fwd", None, 0, None, None, None, 0, None, None, 0, 0, 1e-5)
    with pytest.raises(RuntimeError, match=r"mclstexp_hip mcl_avgpool2_nhwc_bf16 failed: \[-1\]"):
        call("mcl_avgpool2_nhwc_bf16", None, None, 0, 0, 0, 0, 0)
    with pytest.raises(RuntimeError, match=r"mclstexp_hip mcl_gemm failed: \[-1\]"):
        call("mcl_gemm", C.byref(_lib.gemm_args()))                          # ctypes objects pass through


def test_value_returning_entry_points_return_and_reject_in_one_place(built):
    assert call("mcl_abi_version") == _lib.ABI_VERSION
    assert call("mcl_gemm_args_size") == C.sizeof(_lib.GemmArgs)
    assert call("mcl_bn_workspace_floats", 4096, 64, 1) > 0
    assert call("mcl_gemm_auto_ksplit", 0, 0, 0, 0) == 1                        # (documented answer for a degenerate problem)
    assert call("mcl_harmony_workspace_doubles", 0, 0, 0, 0) == 0               # (0, not an error, by this entry point's contract)
    assert b"invalid" in call("mcl_error_string", -1)
    with pytest.raises(RuntimeError, match=r"mcl_bn_workspace_floats rejected its arguments \(0, 64, 1\)"):
        call("mcl_bn_workspace_floats", 0, 64, 1)
    with pytest.raises(RuntimeError, match=r"mcl_infonce_fused_workspace_bytes rejected"):
        call("mcl_infonce_fused_workspace_bytes", 8, 8, 7)


def test_no_module_reaches_the_library_around_call():
    """Every module of the package goes through ``_lib.call``: no direct ``<lib>.mcl_*(`` call, no ``check(``, and the names
    that stay for the tests (``ops._stream``, ``densenet_fused._stream``, ``vit_fused._st``) are the one shared helper."""
    srcs = sorted(p for p in glob.glob(os.path.join(ROOT, "mclstexp_amd", "*.py")) if os.path.basename(p) != "_lib.py")
    assert len(srcs) >= 25
    offenders = {}
    for p in srcs:
        text = re.sub(r"#[^\n]*", "", open(p).read())                      # (comments may speak of a check)
        hits = re.findall(r"\.\s*mcl_\w+\s*\(", text) + re.findall(r"(?<![\w.])(?<!def )check\(|_lib\s*\.\s*check\s*\(", text)
        hits += re.findall(r"def\s+_st(?:ream)?\s*\(", text) + re.findall(r"getattr\([^)]*mcl_", text)
        if hits:
            offenders[os.path.basename(p)] = hits
    assert not offenders, "call the C ABI through mclstexp_amd._lib.call"
    from mclstexp_amd import densenet_fused, ops, vit_fused
    assert ops._stream is densenet_fused._stream is vit_fused._st is _lib.current_stream


@pytest.mark.gpu
def test_call_launches_exactly_what_raw_ctypes_launches():
    n = 1000 + 3
    g = torch.Generator(device="cuda").manual_seed(5)
    a = torch.randn(n, device="cuda", generator=g)
    b = torch.randn(n, device="cuda", generator=g)
    raw, via = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    with _lib.AbiTimer(["mcl_add_f32"]) as t:
        rc = _lib.lib().mcl_add_f32(a.data_ptr(), b.data_ptr(), raw.data_ptr(), n, _lib.current_stream())
        assert call("mcl_add_f32", a, b, via, n) is None
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(raw, a + b) and raw.view(torch.int32).equal(via.view(torch.int32))
    (_, _, raw_args), (_, _, via_args) = t.records["mcl_add_f32"]
    assert raw_args == (a.data_ptr(), b.data_ptr(), raw.data_ptr(), n, _lib.current_stream())
    assert via_args == (a.data_ptr(), b.data_ptr(), via.data_ptr(), n, _lib.current_stream())
    assert [type(v) for v in via_args] == [type(v) for v in raw_args]
    # the same on a side stream: the stream appended is the current one at the time of the call
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), _lib.AbiTimer(["mcl_add_f32"]) as t2:
        call("mcl_add_f32", a, b, via, n)
    assert t2.records["mcl_add_f32"][0][2][-1] == side.cuda_stream
    torch.cuda.current_stream().wait_stream(side)
    # a host tensor among device tensors is refused, not launched
    with pytest.raises(RuntimeError, match="mcl_add_f32: argument 1 is on cpu"):
        call("mcl_add_f32", a, b.cpu(), via, n)
    torch.cuda.synchronize()
    assert raw.view(torch.int32).equal(via.view(torch.int32))


@pytest.mark.gpu
def test_a_stage_entry_point_follows_the_current_stream():
    """``hmrf.edge_agreement`` passes no stream: ``call`` hands ``mcl_edge_agreement`` torch's current one.  One slide of 4
    spots on a ring, 2 neighbour slots of weight 1, labels 0 0 1 1: every spot agrees with one of its two neighbours."""
    import numpy as np
    from mclstexp_amd import hmrf
    graph = {"nbr": np.array([[3, 1], [0, 2], [1, 3], [2, 0]], dtype=np.int32), "w": np.ones((4, 2)), "offsets": [0, 4]}
    labels = np.array([0, 0, 1, 1], dtype=np.int32)
    default = hmrf.edge_agreement(labels, graph)
    assert default.shape == (1,) and default[0] == 0.5
    side = torch.cuda.Stream()
    with torch.cuda.stream(side), _lib.AbiTimer(["mcl_edge_agreement"]) as t:
        on_side = hmrf.edge_agreement(labels, graph)
    (_, _, args), = t.records["mcl_edge_agreement"]
    assert len(args) == 9 and args[-1] == side.cuda_stream != torch.cuda.current_stream().cuda_stream
    assert on_side.tobytes() == default.tobytes()
    torch.cuda.synchronize()
