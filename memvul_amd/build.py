"""Build libmemvul_hip.so (product and development build) and the side libraries of SIDE_LIBS — libmemvul_tok_u8.so, libmemvul_pp_fixed.so, libmemvul_retrieve.so,
libmemvul_claims.so, libmemvul_bank.so and libmemvul_rank.so — for gfx950, in-tree with hipcc.  The last four share csrc/kept_index.h and csrc/kept_terms.h, which no other library
includes.  No torch involved."""
from __future__ import annotations

from functools import partial
import os
import shutil
import subprocess
from struct import error as struct_error
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libmemvul_hip.so")
# the same sources with -DMEMVUL_DEV_SWITCHES: the development A/B knobs (MEMVUL_GEMM_TILE, MEMVUL_SHORT_VLO, MEMVUL_RASTER, MEMVUL_GN_MAX,
# MEMVUL_NUM_CU; engine.hip read_switches) exist only in this build — GPU tests that force a kernel path at test sizes and the A/B scripts load it
LIB_PATH_DEV = os.path.join(LIB_DIR, "libmemvul_hip_dev.so")
# -Bsymbolic: a test process loads this build NEXT TO the product library, which binding.load_library opens RTLD_GLOBAL.  Both define the same interposable
# symbols (mv_destroy, mv_comm_destroy, mv_handle's implicit constructor and destructor, the kernels' host handles), and without it the dynamic linker binds this
# build's own references to them to the product's definitions when that was loaded first — host code compiled for ANOTHER mv_handle layout (the development
# members of the struct).  With it every reference of this build is bound to its own definition at link time; the product's link line is untouched
DEV_FLAGS = ("-DMEMVUL_DEV_SWITCHES", "-Wl,-Bsymbolic")
# the side libraries, each with sources, headers and a stamp of its own: key -> (library name, sources, headers).
#   tok       the UTF-8 tokenise kernel and its launch function, a library and a code object of its own (csrc/wordpiece_u8.hip says why); the two libraries above link
#             against it and find it beside themselves ($ORIGIN), so it is built before them
#   pp        the fixed-form persistent GEMMs of MV_F16X8 and their launch function (csrc/gemm_pp_fixed.hip says why they are not kernels of libmemvul_hip.so); linked
#             against and found like tok, so built before the two libraries above as well.  It is built from csrc/gemm_pp.h — a kernel edit there moves both maps
#   retrieve  per-anchor retrieval over a kept corpus (csrc/retrieve.hip, csrc/report_topk.h, include/memvul_retrieve.h)
#   claims    per-anchor claims over a kept corpus (csrc/claims.hip, csrc/claim_sweep.h, include/memvul_claims.h)
#   bank      the anchor-bank audit over a kept corpus (csrc/bank.hip, csrc/bank_cover.h, include/memvul_bank.h)
#   rank      per-anchor ranking quality over a kept corpus (csrc/rank.hip, csrc/rank_sort.h, include/memvul_rank.h)
# The four kept-corpus libraries stand alone — nothing links against them and they link against nothing of this tree, so neither the source fingerprint nor the
# kernel map of the libraries above moves with them — and share two headers, which only they include: csrc/kept_index.h (the host side of an index over a kept corpus)
# and csrc/kept_terms.h (the device functions of the row and vector terms)
KEPT_HEADERS = ["kept_index.h", "kept_terms.h"]
SIDE_LIBS = {
    "tok": ("libmemvul_tok_u8.so", ["wordpiece_u8.hip"], ["wordpiece.h"]),
    "pp": ("libmemvul_pp_fixed.so", ["gemm_pp_fixed.hip"], ["gemm_pp_fixed.h", "gemm_pp.h", "gemm.h", "common.h"]),
    "retrieve": ("libmemvul_retrieve.so", ["retrieve.hip"], ["report_topk.h", *KEPT_HEADERS, os.path.join(ROOT, "include", "memvul_retrieve.h")]),
    "claims": ("libmemvul_claims.so", ["claims.hip"], ["claim_sweep.h", *KEPT_HEADERS, os.path.join(ROOT, "include", "memvul_claims.h")]),
    "bank": ("libmemvul_bank.so", ["bank.hip"], ["bank_cover.h", *KEPT_HEADERS, os.path.join(ROOT, "include", "memvul_bank.h")]),
    "rank": ("libmemvul_rank.so", ["rank.hip"], ["rank_sort.h", *KEPT_HEADERS, os.path.join(ROOT, "include", "memvul_rank.h")]),
}
TOK_LIB_NAME, TOK_SOURCES, TOK_HEADERS = SIDE_LIBS["tok"]
PP_LIB_NAME, PP_SOURCES, PP_HEADERS = SIDE_LIBS["pp"]
RETRIEVE_LIB_NAME, RETRIEVE_SOURCES, RETRIEVE_HEADERS = SIDE_LIBS["retrieve"]
CLAIMS_LIB_NAME, CLAIMS_SOURCES, CLAIMS_HEADERS = SIDE_LIBS["claims"]
BANK_LIB_NAME, BANK_SOURCES, BANK_HEADERS = SIDE_LIBS["bank"]
RANK_LIB_NAME, RANK_SOURCES, RANK_HEADERS = SIDE_LIBS["rank"]
LIB_PATH_TOK, LIB_PATH_RETRIEVE, LIB_PATH_CLAIMS, LIB_PATH_BANK, LIB_PATH_RANK = (os.path.join(LIB_DIR, SIDE_LIBS[k][0]) for k in ("tok", "retrieve", "claims", "bank", "rank"))
LIB_PATH_PP = os.path.join(LIB_DIR, PP_LIB_NAME)
SOURCES = ["engine.hip"]
KERNEL_HEADERS = ["common.h", "gemm.h", "gemm_pp.h", "gemm_pp_fixed.h", "attention.h", "attention_v2.h", "misc_kernels.h", "match_topk.h", "ref_f32.h", "sink_census.h", "route.h", "wordpiece.h"]
# the host code of the library: engine.hip includes each of these parts once, in this order
HOST_PARTS = ["host_base.h", "weights.h", "workspace.h", "encoder_pass.h", "batch_flow.h", "corpus.h", "comm.h", "records_format.h", "tokenizer_object.h"]
HEADERS = KERNEL_HEADERS + HOST_PARTS + [os.path.join(ROOT, "include", "memvul_hip.h")]
ARCH = "gfx950"


def hipcc_path() -> str:
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (need ROCm at /opt/rocm)")


STAMP_PATH = LIB_PATH + ".stamp"


def _paths(dev: bool):
    lib = LIB_PATH_DEV if dev else LIB_PATH
    return lib, lib + ".stamp"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-shared", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function", "-Wno-unused-value"]


def _compiler_id():
    try:
        return subprocess.run([hipcc_path(), "--version"], capture_output=True, check=True).stdout
    except Exception:  # no compiler here (a GPU box without the ROCm dev tools)
        return None


def source_fingerprint(extra_flags=(), sources=None, headers=None) -> str:
    """sha256 of the flags and the CONTENT of every source / header (not mtimes — a checkout or a copy to another box
    rewrites those).  sources / headers: those of another library than libmemvul_hip.so."""
    import hashlib

    h = hashlib.sha256()
    h.update(" ".join([ARCH, *FLAGS, *extra_flags]).encode())
    deps = [os.path.join(CSRC, s) for s in (sources or SOURCES)] + [h_ if os.path.isabs(h_) else os.path.join(CSRC, h_) for h_ in (headers or HEADERS)]
    for d in deps:
        h.update(os.path.basename(d).encode())
        with open(d, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def build_fingerprint(extra_flags=()) -> str:
    """What the binary depends on, as the two lines of the stamp file: `src <sha256 of flags + sources>` and
    `cc <sha256 of the compiler's --version>`.  bench.py keys its counter figures on the whole stamp."""
    import hashlib

    cc = _compiler_id()
    return "src %s\ncc %s" % (source_fingerprint(extra_flags), hashlib.sha256(cc).hexdigest() if cc is not None else "unknown")


def device_code_objects(lib_path: str = None) -> list:
    """The gfx950 code object(s) embedded in the shared library (the clang offload bundle inside .hip_fatbin), as bytes: what the GPU executes."""
    import struct

    data = open(lib_path or LIB_PATH, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    found = []
    i = data.find(magic)
    while i >= 0:
        if i + 32 > len(data):
            raise RuntimeError("truncated offload bundle header")
        (n,) = struct.unpack_from("<Q", data, i + 24)
        off = i + 32
        if n > 64:  # a handful of targets at most: anything else is not a bundle header we understand (e.g. a compressed one)
            raise RuntimeError(f"offload bundle with {n} entries: not a plain clang offload bundle")
        for _ in range(n):
            if off + 24 > len(data):
                raise RuntimeError("truncated offload bundle entry table")
            o, size, tsz = struct.unpack_from("<QQQ", data, off)
            off += 24
            if tsz > 256 or off + tsz > len(data) or i + o + size > len(data):  # never trust offsets read from the file
                raise RuntimeError("offload bundle entry points outside the file")
            triple = data[off:off + tsz]
            off += tsz
            if ARCH.encode() in triple:
                found.append(data[i + o:i + o + size])
        i = data.find(magic, i + len(magic))
    if not found:
        raise RuntimeError(f"no {ARCH} code object found in {lib_path or LIB_PATH}")
    return found


def device_code_fingerprint(lib_path: str = None) -> str:
    """sha256 of the gfx950 code object(s) embedded in the shared library: what the GPU executes.  Any kernel change moves it — bench.py keys the counter
    figures of profiles/pmc_current.json on this line of the stamp.  A host-only edit of engine.hip or of a part it includes leaves the KERNELS unchanged (kernel_fingerprints
    below compares them one by one), but this hash — the stamp's `dev` line — may still move: the kernels are laid out in the code object in the order
    in which the host code first uses them."""
    import hashlib

    h = hashlib.sha256()
    for co in device_code_objects(lib_path):
        h.update(co)
    return h.hexdigest()


STT_OBJECT, STT_FUNC, STB_GLOBAL = 1, 2, 1


def code_object_symbols(co: bytes):
    """The defined FUNC and OBJECT symbols of one code object (ELF64, little endian) as (name, type, binding, bytes), read from its section and symbol
    tables; symbols of sections without file contents (.bss) are left out."""
    import struct

    def need(off, size, what):  # never trust offsets read from the file
        if off < 0 or size < 0 or off + size > len(co):
            raise RuntimeError(f"code object: {what} points outside the file")

    need(0, 64, "ELF header")
    if co[:6] != b"\x7fELF\x02\x01":
        raise RuntimeError("code object: not a little-endian ELF64 file")
    (shoff,) = struct.unpack_from("<Q", co, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", co, 0x3A)
    if shentsize < 64:
        raise RuntimeError("code object: section headers shorter than ELF64's")
    need(shoff, shentsize * shnum, "section header table")
    # (type, address, file offset, size, link, entry size) per section
    secs = [struct.unpack_from("<4xI8xQQQI4x8xQ", co, shoff + i * shentsize) for i in range(shnum)]
    out = []
    for typ, _, off, size, link, entsize in secs:
        if typ != 2:  # SHT_SYMTAB
            continue
        need(off, size, "symbol table")
        if entsize < 24 or link >= shnum:
            raise RuntimeError("code object: malformed symbol table header")
        _, _, stroff, strsize, _, _ = secs[link]
        need(stroff, strsize, "string table")
        for s in range(off, off + size - entsize + 1, entsize):
            name, info, shndx, value, nbytes = struct.unpack_from("<IBxHQQ", co, s)
            if (info & 15) not in (STT_OBJECT, STT_FUNC) or shndx == 0 or shndx >= shnum or nbytes == 0:
                continue
            styp, saddr, soff, ssize, _, _ = secs[shndx]
            if styp == 8:  # SHT_NOBITS
                continue
            if value < saddr or value - saddr + nbytes > ssize:
                raise RuntimeError("code object: a symbol lies outside its section")
            need(soff + value - saddr, nbytes, "symbol")
            end = co.find(b"\0", stroff + name, stroff + strsize) if name < strsize else -1
            if end < 0:
                raise RuntimeError("code object: a symbol name lies outside the string table")
            out.append((co[stroff + name:end].decode(), info & 15, info >> 4, co[soff + value - saddr:soff + value - saddr + nbytes]))
    return out


def kernel_fingerprints(lib_path: str = None) -> dict:
    """The device code of the library kernel by kernel: {symbol: sha256}, for every function (its instruction bytes) and every kernel descriptor
    `<kernel>.kd` (its 64 bytes with bytes 16 .. 23 zeroed: the offset from the descriptor to the kernel's entry, the one field that depends on where
    the kernel lies in the code object).  Unlike device_code_fingerprint it does not move with the ORDER of the kernels, so it is equal before and
    after a host-only edit of engine.hip or its parts, and between the product and the development build of one tree.  No external tool is called (a GPU box may have
    none)."""
    import hashlib

    out = {}
    for co in device_code_objects(lib_path):
        for name, typ, _, data in code_object_symbols(co):
            if typ == STT_FUNC:
                out[name] = hashlib.sha256(data).hexdigest()
            elif name.endswith(".kd") and len(data) == 64:
                out[name] = hashlib.sha256(data[:16] + bytes(8) + data[24:]).hexdigest()
    return out


def read_stamp(dev: bool = False) -> dict:
    """The stamp next to the library as a dict: src / cc (what it was built from) and dev (the device code it contains)."""
    with open(_paths(dev)[1]) as f:
        return dict(line.split(" ", 1) for line in f.read().strip().splitlines() if " " in line)


def is_stale(extra_flags=(), dev: bool = False) -> bool:
    """True when the library must be rebuilt: no binary / stamp, other sources or flags, or — where a compiler exists to
    compare with — another compiler.  On a box WITHOUT hipcc only the source line is compared (the binary that travelled with
    the tree is then the one to use; ADVICE r2: the old single-hash stamp could never match there)."""
    lib_path, stamp_path = _paths(dev)
    if dev:
        extra_flags = tuple(extra_flags) + DEV_FLAGS
    if not os.path.exists(lib_path) or not os.path.exists(stamp_path):
        return True
    with open(stamp_path) as f:
        have = dict(line.split(" ", 1) for line in f.read().strip().splitlines() if " " in line)
    want = dict(line.split(" ", 1) for line in build_fingerprint(extra_flags).splitlines())
    if have.get("src") != want["src"]:
        return True
    return want["cc"] != "unknown" and have.get("cc") != want["cc"]


def side_lib_path(key: str) -> str:
    return os.path.join(LIB_DIR, SIDE_LIBS[key][0])


def _side_stamp(key: str) -> str:
    import hashlib

    _, sources, headers = SIDE_LIBS[key]
    cc = _compiler_id()
    return "src %s\ncc %s\n" % (source_fingerprint((), sources, headers), hashlib.sha256(cc).hexdigest() if cc is not None else "unknown")


def side_is_stale(key: str) -> bool:
    """is_stale for a side library (SIDE_LIBS[key]): its own stamp, over its own sources and headers."""
    lib_path = side_lib_path(key)
    if not os.path.exists(lib_path) or not os.path.exists(lib_path + ".stamp"):
        return True
    with open(lib_path + ".stamp") as f:
        have = dict(line.split(" ", 1) for line in f.read().strip().splitlines() if " " in line)
    want = dict(line.split(" ", 1) for line in _side_stamp(key).splitlines())
    if have.get("src") != want["src"]:
        return True
    return want["cc"] != "unknown" and have.get("cc") != want["cc"]


def build_side(key: str, force: bool = False, verbose: bool = True) -> str:
    """Compile a side library (SIDE_LIBS[key]) for gfx950; returns its path."""
    lib_name, sources, _ = SIDE_LIBS[key]
    lib_path = side_lib_path(key)
    if not force and not side_is_stale(key):
        return lib_path
    os.makedirs(LIB_DIR, exist_ok=True)
    cmd = [hipcc_path(), f"--offload-arch={ARCH}", *FLAGS, f"-Wl,-soname,{lib_name}", *[os.path.join(CSRC, s) for s in sources], "-o", lib_path + ".tmp"]
    if verbose:
        print("[memvul_amd.build]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    with open(lib_path + ".stamp.tmp", "w") as f:
        f.write(_side_stamp(key))
    os.replace(lib_path + ".tmp", lib_path)
    os.replace(lib_path + ".stamp.tmp", lib_path + ".stamp")
    return lib_path


tok_is_stale, retrieve_is_stale, claims_is_stale, bank_is_stale, rank_is_stale = (partial(side_is_stale, k) for k in ("tok", "retrieve", "claims", "bank", "rank"))
build_tok, build_retrieve, build_claims, build_bank, build_rank = (partial(build_side, k) for k in ("tok", "retrieve", "claims", "bank", "rank"))
pp_is_stale, build_pp = partial(side_is_stale, "pp"), partial(build_side, "pp")


def build(force: bool = False, verbose: bool = True, extra_flags=(), dev: bool = False) -> str:
    """Compile the HIP library for gfx950; returns the .so path.  dev: the -DMEMVUL_DEV_SWITCHES build (libmemvul_hip_dev.so).  libmemvul_tok_u8.so and
    libmemvul_pp_fixed.so, which both link against, are brought up to date first."""
    tok = build_tok(False, verbose)  # (forced by build_all, once for both)
    build_pp(False, verbose)
    if not force and not is_stale(extra_flags, dev):
        return _paths(dev)[0]
    lib_path, stamp_path = _paths(dev)
    if dev:
        extra_flags = tuple(extra_flags) + DEV_FLAGS
    os.makedirs(LIB_DIR, exist_ok=True)
    cmd = [
        hipcc_path(), f"--offload-arch={ARCH}", *FLAGS,  # -Wno-unused-value: hipError_t of calls checked by launch_check
        *extra_flags,
        *[os.path.join(CSRC, s) for s in SOURCES],
        "-L" + os.path.dirname(tok), "-l:" + TOK_LIB_NAME, "-l:" + PP_LIB_NAME, "-Wl,-rpath,$ORIGIN",  # (found beside this library wherever the tree lies)
        "-o", lib_path + ".tmp",
    ]
    if verbose:
        print("[memvul_amd.build]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    # the stamp describes the NEW binary and is written from it before either file is moved into place; a fatbin this parser does
    # not understand (compressed bundle, no gfx950 entry) yields `dev unknown` — bench.load_pmc then compares whole stamps — instead
    # of a successful compile left without a stamp (and rebuilt, and failing again, on every load)
    try:
        code = device_code_fingerprint(lib_path + ".tmp")
    except (RuntimeError, OSError, ValueError, struct_error) as e:
        code = "unknown"
        if verbose:
            print(f"[memvul_amd.build] device-code fingerprint unavailable ({e}); stamp carries `dev unknown`", flush=True)
    with open(stamp_path + ".tmp", "w") as f:
        f.write(build_fingerprint(extra_flags) + "\ndev " + code + "\n")
    os.replace(lib_path + ".tmp", lib_path)
    os.replace(stamp_path + ".tmp", stamp_path)
    return lib_path


def build_all(force: bool = False, verbose: bool = True):
    """Both builds, compiled side by side (two hipcc processes), after the two libraries both link against; libmemvul_retrieve.so, libmemvul_claims.so,
    libmemvul_bank.so and libmemvul_rank.so, which stand alone, beside them.  Returns the paths of the two builds of libmemvul_hip.so (LIB_PATH_RETRIEVE,
    LIB_PATH_CLAIMS, LIB_PATH_BANK and LIB_PATH_RANK are where the other four lie)."""
    from concurrent.futures import ThreadPoolExecutor

    build_tok(force, verbose)
    build_pp(force, verbose)
    with ThreadPoolExecutor(6) as ex:
        sides = [ex.submit(build_side, key, force, verbose) for key in ("retrieve", "claims", "bank", "rank")]
        futs = [ex.submit(build, force, verbose, (), d) for d in (False, True)]
        for side in sides:
            side.result()
        return [f.result() for f in futs]


if __name__ == "__main__":
    print("\n".join(build_all(force="--force" in sys.argv) + [LIB_PATH_TOK, LIB_PATH_PP, LIB_PATH_RETRIEVE, LIB_PATH_CLAIMS, LIB_PATH_BANK, LIB_PATH_RANK]))
