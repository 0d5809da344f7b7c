"""CPU: the device types and helpers of csrc/device.h are defined there once, not copied into a kernel file (no compute)."""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "mclstexp_amd", "csrc")


def _strip(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return re.sub(r"__attribute__\s*\(\((?:[^()]|\([^()]*\))*\)\)", "", text)


def defined_names(text):
    """Type, function, lambda and macro names a C++ source defines."""
    text = _strip(text)
    names = {re.findall(r"\w+", t)[-1] for t in re.findall(r"\btypedef\b([^;]*);", text)}
    names |= set(re.findall(r"__device__[^;{}()=]*?\b(\w+)\s*\(", text))
    names |= set(re.findall(r"\bauto\s+(\w+)\s*=\s*\[", text))
    names |= set(re.findall(r"^\s*#\s*define\s+(\w+)", text, flags=re.M))
    return names


def test_device_header_defines_the_shared_helpers():
    names = defined_names(open(os.path.join(CSRC, "device.h")).read())
    for n in ("bf16_t", "bf16x2_t", "bf16x8", "v4s", "f32x2", "f32x4", "f32x16", "u32x2", "u32x4", "u64", "bf_lo",
              "bf_hi", "bf2f", "pack_bf16", "f2bf", "round_bf16", "pack8", "unpack8", "ldd", "lanes_below", "half_wave_sum",
              "opaque_lane", "glds16", "glds16s", "glds4", "buffer_lds16", "bn_relu_chunk", "MCL_LDSP", "MCL_GLBP"):
        assert n in names, n
    assert '#include "device.h"' in open(os.path.join(CSRC, "common.h")).read()


def test_no_kernel_file_redefines_a_device_header_name():
    shared = defined_names(open(os.path.join(CSRC, "device.h")).read())
    srcs = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    assert len(srcs) > 20
    copies = {os.path.basename(p): sorted(defined_names(open(p).read()) & shared) for p in srcs}
    assert not {k: v for k, v in copies.items() if v}, "defined in csrc/device.h, use it from there"
