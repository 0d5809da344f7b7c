"""CPU: the device types and helpers of csrc/device.h and the statistics of csrc/stats.h are defined there once, not copied
into a kernel file (no compute)."""
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
              "opaque_lane", "wave_sync", "glds16", "glds16s", "glds4", "buffer_lds16", "bn_relu_chunk", "MCL_LDSP", "MCL_GLBP",
              "wave_sum", "wave_max", "wave_min", "block_sum4", "order_key", "key_value", "mix64", "segment_rows",
              "segment_span", "segment_entries", "valid_weight", "clamp_index"):
        assert n in names, n
    assert '#include "device.h"' in open(os.path.join(CSRC, "common.h")).read()


def test_stats_header_defines_the_shared_statistics():
    text = open(os.path.join(CSRC, "stats.h")).read()
    names = defined_names(text)
    for n in ("normal_tail", "before", "bh_stage", "bh_adjust", "top_select"):
        assert n in names, n
    for n in ("LN10", "LN2", "SQRT2", "TOP_SAMPLE", "TOP_CAP"):
        assert re.search(r"^constexpr \w+ %s = " % n, text, flags=re.M), n
    assert re.search(r"^struct top_lds\b", text, flags=re.M)
    assert '#include "stats.h"' not in open(os.path.join(CSRC, "common.h")).read()      # the training kernels do without it


def test_no_kernel_file_redefines_a_device_header_name():
    shared = defined_names(open(os.path.join(CSRC, "device.h")).read() + open(os.path.join(CSRC, "stats.h")).read())
    srcs = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    assert len(srcs) > 20
    copies = {os.path.basename(p): sorted(defined_names(open(p).read()) & shared) for p in srcs}
    assert not {k: v for k, v in copies.items() if v}, "defined in csrc/device.h or csrc/stats.h, use it from there"


# a helper that differs from device.h's keeps a name of its own; (file, name): the difference, stated at the definition too
LOCAL_FORMS = {
    ("spatial.hip", "sp_slide_rows"): "tests r1 < r0 ahead of the subtraction, terms in another order: segment_rows changes "
                                      "the code of the file's kernels",
}
COPY_NAMES = re.compile(r"\w+_wave_(sum|total|count|max|min)\w*|wave_(min|max)_f64|\w+_slide_rows|\w+_(mix|mix64)|"
                        r"\w+_valid_weight|\w+_ceil")


def defined_functions(text):
    """Names of the functions, host or device, that a C++ source defines at file scope."""
    return set(re.findall(r"^[A-Za-z_][^;{}()=#\n]*?[\s*&](\w+)\s*\(", _strip(text), flags=re.M))


def test_no_kernel_file_keeps_a_copy_of_a_lane_segment_or_hash_helper():
    srcs = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    found = {}
    for p in srcs:
        name, text = os.path.basename(p), open(p).read()
        assert "9e3779b97f4a7c15" not in text.lower(), f"{name}: the splitmix64 step is device.h's mix64"
        for fn in defined_functions(text):
            if COPY_NAMES.fullmatch(fn):
                found[(name, fn)] = text
    assert set(found) == set(LOCAL_FORMS), "a copy of a csrc/device.h helper (or an entry of LOCAL_FORMS that is gone)"
    for (name, fn), text in found.items():      # the reason stands at the definition: a comment right above it
        lines = text.splitlines()
        at = next(i for i, l in enumerate(lines) if re.match(r"[A-Za-z_].*\b%s\s*\(" % fn, l))
        assert lines[at - 1].startswith("//") and "device.h" in "".join(lines[max(0, at - 3):at]), (name, fn)


# the copies that csrc/stats.h (and device.h's wave_sync) replaced.  (file, name): the difference, stated at the definition too;
# a counting loop against an LDS tile that is written out goes by the name of its kernel
LOCAL_STATS = {
    ("eval_metrics.hip", "heg_beats"): "with HEG_SAMPLE / HEG_CAP the top-n of expr_summary_kernel: top_select changes the "
                                       "kernel's code and mcl_expr_metrics measures outside the spread of two runs",
    ("eval_metrics.hip", "HEG_SAMPLE"): "as heg_beats",
    ("eval_metrics.hip", "HEG_CAP"): "as heg_beats",
    # the counting loop against an LDS tile: stats.h holds no shared form and says why (a call changes the kernels' code and
    # their entry points measure slower); a kernel that gains such a loop is decided there and listed here
    ("markers.hip", "marker_prank_kernel"): "the loop", ("markers.hip", "marker_order_kernel"): "the loop",
    ("spatial.hip", "sp_prank_kernel"): "the loop", ("gene_significance.hip", "gene_order_kernel"): "the loop",
}
STAT_COPY_NAMES = re.compile(r"\w+_normal_tail|(\w+_)?beats|\w+_top_genes|\w+_wave_sync")
STAT_COPY_CONSTANTS = re.compile(r"\bconst(?:expr)?\s+\w+\s+(\w+_(?:LN10|LN2|SQRT2|SAMPLE|CAP))\s*=")
TILE_LOOP = re.compile(r"rank \+= [^;\n]*\btile\[")


def test_no_kernel_file_keeps_a_copy_of_a_statistic():
    found = {}
    for p in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        name, text = os.path.basename(p), open(p).read()
        for literal, what in (("2.302585092994046", "LN10"), ("1.4142135623730951", "SQRT2")):
            assert literal not in text, f"{name}: {literal} is stats.h's {what}"
        code = _strip(text)
        copies = {fn for fn in defined_functions(text) if STAT_COPY_NAMES.fullmatch(fn)}
        copies |= set(STAT_COPY_CONSTANTS.findall(code))
        for m in TILE_LOOP.finditer(code):      # the kernel that holds the loop
            copies.add(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", code[:m.start()])[-1])
        for fn in copies:
            found[(name, fn)] = text
    assert set(found) == set(LOCAL_STATS), "a copy of a csrc/stats.h statistic (or an entry of LOCAL_STATS that is gone)"
    for (name, fn), text in found.items():      # the reason stands at the definition: a comment right above it
        lines = text.splitlines()
        at = next(i for i, l in enumerate(lines) if re.match(r"[A-Za-z_].*\b%s\b" % fn, l))
        while STAT_COPY_CONSTANTS.search(lines[at - 1]):      # constants that stand together share one comment
            at -= 1
        above = "".join(lines[max(0, at - 6):at])
        assert lines[at - 1].startswith("//") and ("stats.h" in above or "device.h" in above), (name, fn)
