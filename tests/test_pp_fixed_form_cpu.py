"""The fixed-form persistent GEMMs (memvul_amd/csrc/gemm_pp_fixed.hip, libmemvul_pp_fixed.so), the parts that need no GPU: the build, the kernel maps, the
switch and the counter's binding.  tests/test_pp_fixed_form_gpu.py compares the two forms' bits."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rank_kit as kit  # noqa: E402
from memvul_amd import binding, build  # noqa: E402

CSRC = os.path.join(ROOT, "memvul_amd", "csrc")


@pytest.fixture(scope="module")
def libs():
    return build.build_all(verbose=False)


def test_side_libs_lists_the_library_with_its_sources(libs):
    assert build.SIDE_LIBS["pp"] == (build.PP_LIB_NAME, build.PP_SOURCES, build.PP_HEADERS) == (
        "libmemvul_pp_fixed.so", ["gemm_pp_fixed.hip"], ["gemm_pp_fixed.h", "gemm_pp.h", "gemm.h", "common.h"])
    # the stamp covers every project header the source includes, directly or through gemm_pp.h
    seen, todo = set(), ["gemm_pp_fixed.hip"]
    while todo:
        name = todo.pop()
        for inc in re.findall(r'#include\s+"([^"]+)"', open(os.path.join(CSRC, name)).read()):
            if inc not in seen:
                seen.add(inc)
                todo.append(inc)
    assert seen == set(build.PP_HEADERS)
    assert os.path.exists(build.LIB_PATH_PP) and not build.pp_is_stale() and build.build_pp(verbose=False) == build.LIB_PATH_PP
    assert "gemm_pp_fixed.h" in build.KERNEL_HEADERS  # the header libmemvul_hip.so calls the library through is part of ITS stamp


def test_both_builds_link_against_it_and_it_against_nothing_of_the_tree(libs):
    def needed(path):
        out = subprocess.run([kit.llvm_tool("llvm-readelf"), "-d", path], capture_output=True, text=True, check=True).stdout
        return "".join(ln for ln in out.splitlines() if "NEEDED" in ln)

    for path in libs:
        assert "libmemvul_pp_fixed.so" in needed(path) and "libmemvul_tok_u8.so" in needed(path), path
    assert "libmemvul" not in needed(build.LIB_PATH_PP)
    exported = subprocess.run([kit.llvm_tool("llvm-readelf"), "--dyn-syms", build.LIB_PATH_PP], capture_output=True, text=True, check=True).stdout
    assert {"pp_fixed_launch", "pp_fixed_lds_opt_in"} <= set(re.findall(r"\b(pp_fixed_\w+)", exported))
    assert not re.search(r"\bmv_[a-z]", exported)


def test_the_kernels_are_the_recorded_ones(libs):
    """Three kernel kinds at two padded lengths, under a name of their own, and the bytes recorded in profiles/kernel_fingerprints_pp.json (a kernel edit of
    gemm_pp.h moves this map together with the two of libmemvul_hip.so: python scripts/kernel_fingerprints.py --pp --out profiles/kernel_fingerprints_pp.json)."""
    with open(os.path.join(ROOT, "profiles", "kernel_fingerprints_pp.json")) as f:
        want = json.load(f)
    got = build.kernel_fingerprints(build.LIB_PATH_PP)
    changed = sorted(set(want) ^ set(got)) + sorted(k for k in set(want) & set(got) if want[k] != got[k])
    assert not changed, changed
    kernels = sorted(k[:-3] for k in got if k.endswith(".kd"))
    assert len(kernels) == 6 and all(re.match(r"_Z20gemm_pp_fixed_kernelILi(1ELi1|3ELi1|8ELi0)ELi1ELi(256|512)EEv8GemmArgs$", k) for k in kernels), kernels
    main = build.kernel_fingerprints(build.LIB_PATH)
    assert main and not set(got) & set(main)  # no symbol of the product library's map, which stays the recorded one
    with open(os.path.join(ROOT, "profiles", "kernel_fingerprints.json")) as f:
        assert json.load(f) == main
    with open(os.path.join(ROOT, "profiles", "kernel_fingerprints_dev.json")) as f:
        assert json.load(f) == build.kernel_fingerprints(build.LIB_PATH_DEV)


def test_the_run_time_form_is_the_header_as_it_stands():
    """gemm_pp.h alone defines every accessor with its GemmArgs field, so a translation unit that overrides none compiles the kernels it always did; the side
    library's source overrides them BEFORE the include and is the only file that does."""
    hdr = open(os.path.join(CSRC, "gemm_pp.h")).read()
    defaults = dict(re.findall(r"#ifndef (PP_[A-Z0-9_]+)[^\n]*\n#define \1(?:\(a(?:, tm)?\))? ?([^\n]*)", hdr))
    assert defaults["PP_KERNEL_NAME"] == "gemm_pp_kernel" and defaults["PP_EXTRA_TPARAMS"] == ""
    for macro, field in (("PP_X8_TERMS", "x8_terms"), ("PP_ASIDE_MASK", "x8_aside_mask"), ("PP_OUT8_HI_ONLY", "out8_hi_only"), ("PP_VT_LO", "vt_lo"),
                         ("PP_RASTER_MODE", "raster_mode"), ("PP_S", "S"), ("PP_N", "N")):
        assert defaults[macro] == "((a).%s)" % field, macro
    assert "sload_i32((a).tile_both + (tm))" in defaults["PP_SHORT_TILE"]  # the per-tile flag keeps going through the scalar cache
    src = open(os.path.join(CSRC, "gemm_pp_fixed.hip")).read()
    assert src.index("#define PP_KERNEL_NAME gemm_pp_fixed_kernel") < src.index('#include "gemm_pp.h"')
    assert re.search(r"#define PP_SHORT_TILE\(a, tm\) false\n", src) and "tile_both" not in re.sub(r"//[^\n]*", "", src)  # the fixed form never reads the flag
    for name in os.listdir(CSRC):
        if name not in ("gemm_pp.h", "gemm_pp_fixed.hip"):
            assert "#define PP_" not in open(os.path.join(CSRC, name)).read() or name == "gemm_pp.h", name


def test_the_switch_is_parsed_strictly_and_the_counter_is_bound(libs):
    from stage_kit import host_source

    src = host_source()
    m = re.search(r'getenv\("MEMVUL_PP_FORM"\)\) \{(.*?)\n  \}\n', src, flags=re.S)
    assert m, "read_switches does not read MEMVUL_PP_FORM"
    body = m.group(1)
    assert '!strcmp(e, "fixed")' in body and '!strcmp(e, "runtime")' in body
    assert re.search(r'else \{\s*g_create_error = [^;]*expected \\"fixed\\" or \\"runtime\\"";\s*return MV_ERR_INVALID;', body)  # anything else fails mv_create
    assert re.search(r"bool pp_fixed = true;", src)  # the default
    hdr = open(os.path.join(ROOT, "include", "memvul_hip.h")).read()
    assert "MEMVUL_PP_FORM" in hdr and re.search(r"\bint64_t mvpp_fixed_launches\(mv_handle\* h, int reset\);", hdr)
    for dev in (False, True):
        lib = binding.load_library(dev=dev)
        assert lib.mvpp_fixed_launches.restype == C.c_int64 and lib.mvpp_fixed_launches.argtypes == [C.c_void_p, C.c_int]
        assert lib.mvpp_fixed_launches(None, 0) == -1
    assert "mvpp_fixed_launches" not in binding.ABI_SYMBOLS and hasattr(binding.Engine, "pp_fixed_launches")
    # the predicate, next to pp_selected, and the one place that calls the side library's launcher
    assert re.search(r"bool pp_fixed_form\(const mv_handle\* h, const PassPlan& p, int min_len\) \{\n  return h->pp_fixed && p\.big && p\.x8 && p\.cls_as && "
                     r"p\.one_seq_tiles && min_len >= h->cls_min_len && !p\.two_plane && !p\.safe && p\.qkv_mask == 0;", src)
    assert src.count("pp_fixed_launch(") == 1 and src.count("pp_fixed_lds_opt_in()") == 1
