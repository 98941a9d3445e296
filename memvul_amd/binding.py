"""ctypes binding of libmemvul_hip.so (include/memvul_hip.h) and a thin ``Engine`` wrapper.

The product path has no CPU fallback: if the library cannot be loaded, or a call fails, a
``RuntimeError`` is raised.  Nothing here imports torch or anything under ``oracle/``.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import warnings
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmemvul_hip.so")
LIB_PATH_DEV = os.path.join(_HERE, "lib", "libmemvul_hip_dev.so")  # the -DMEMVUL_DEV_SWITCHES build (memvul_amd/build.py): tests and A/B scripts only
DEV_SWITCHES = ("MEMVUL_GEMM_TILE", "MEMVUL_SHORT_VLO", "MEMVUL_RASTER", "MEMVUL_GN_MAX", "MEMVUL_NUM_CU", "MEMVUL_DEBUG_STOP", "MEMVUL_DEBUG_TAIL")  # read by that build alone

MV_F32, MV_F16, MV_BF16, MV_I32, MV_I64 = 0, 1, 2, 3, 4
MV_F16X8 = 6  # compute dtype only ("precise"): fp16 MFMA sweep + one fp8 (e4m3) correction sweep per GEMM (include/memvul_hip.h)
COMPUTE_DTYPES = {"f16": MV_F16, "fast": MV_F16, "f16x8": MV_F16X8, "precise": MV_F16X8, "safe": MV_F16X8, "guarded": MV_F16X8,
                  # the reference form: the encoder in fp32 on the fp32-input MFMA — what memvul_amd/audit.py measures the other dtypes against; 1/16 of the
                  # 16-bit matrix rate, for audits and envelope work, not for throughput
                  "f32": MV_F32, "reference": MV_F32}
# the three forms of MV_F16X8 (include/memvul_hip.h mv_set_form).  "safe" as a compute dtype name = MV_F16X8 + the safe form set after finalize: both first-order
# correction terms in every row and two fp16 planes through attention at every length — the form that holds 1e-3 with an attention sink on an ordinary token
# ("guarded" likewise: the default form, and the safe form again for the sequences whose own monitor items report an ordinary-token sink)
MV_FORM_DEFAULT, MV_FORM_SAFE, MV_FORM_GUARDED = 0, 1, 2
FORMS = {"default": MV_FORM_DEFAULT, "safe": MV_FORM_SAFE, "guarded": MV_FORM_GUARDED}
# the guarded form costs the default form's time x (1 + 1.34 f) at a rescored share f (14.65 / 10.95 k issue reports/s: DESIGN.md section 2): above this share
# the safe form is the cheaper one, and Engine says so once
GUARDED_WARN_SHARE = 0.25
# The product's default is the compute dtype that holds the reference's 1e-3 logit tolerance on trained-like weights
# (model_memory.py:133-147 at config_memory.json:38's temperature): MV_F16X8.  MV_F16 ("fast") is an explicit opt-in:
# ~1.7x the rate, logits within 1e-3 only on small-logit models (measured 3.0-5.6e-3 at |logit| ~ 3).
DEFAULT_COMPUTE = "precise"


def default_compute() -> str:
    """$MEMVUL_COMPUTE (f16 | fast | f16x8 | precise | safe | guarded | f32 | reference) or the contract-holding default."""
    return os.environ.get("MEMVUL_COMPUTE", DEFAULT_COMPUTE)


def compute_dtype_of(name_or_code) -> int:
    """"f16" (alias "fast") | "f16x8" (alias "precise") | "f32" (alias "reference") or the numeric mv_dtype -> the code mv_finalize_weights takes; None = the
    default (default_compute()); anything else raises."""
    if name_or_code is None:
        name_or_code = default_compute()
    if isinstance(name_or_code, str):
        if name_or_code.lower() not in COMPUTE_DTYPES:
            raise ValueError(f"unknown compute dtype {name_or_code!r}: expected one of {sorted(COMPUTE_DTYPES)}")
        return COMPUTE_DTYPES[name_or_code.lower()]
    if int(name_or_code) not in (MV_F16, MV_F16X8, MV_F32):
        raise ValueError(f"unknown compute dtype code {name_or_code!r}: MV_F16 = {MV_F16}, MV_F16X8 = {MV_F16X8} or MV_F32 = {MV_F32}")
    return int(name_or_code)


def _strict(value, source: str, allowed):
    """A switch that takes one of a few spellings and nothing else: `value` when it is one of `allowed`, else the ValueError that names `source` and them."""
    if value not in allowed:
        names = [repr(a) for a in allowed]
        raise ValueError(f"{source}={value!r}: expected {' or '.join(names) if len(names) == 2 else 'one of ' + ', '.join(names)}")
    return value


def on_sink_policy() -> str:
    """$MEMVUL_ON_SINK = warn (default) | safe, parsed strictly: what an MV_F16X8 engine does when the concentration monitor reports attention sinks on ordinary
    tokens — warn once and go on in the default form, or switch to the safe form (Engine._on_sink_trip)."""
    return _strict(os.environ.get("MEMVUL_ON_SINK", "warn"), "MEMVUL_ON_SINK", ("warn", "safe"))


def sink_census_policy() -> bool:
    """$MEMVUL_SINK_CENSUS = 0 (default) | 1, parsed strictly: whether an MV_F16X8 engine keeps the sink census from construction on (Engine.sink_census)."""
    return _strict(os.environ.get("MEMVUL_SINK_CENSUS", "0"), "MEMVUL_SINK_CENSUS", ("0", "1")) == "1"


MAX_SINK_TOKENS = 64  # include/memvul_hip.h MV_MAX_SINK_TOKENS


def parse_sink_tokens(text: str) -> List[int]:
    """"1012,1010" -> [1012, 1010]: comma-separated decimal token ids and nothing else (no spaces, no signs, no empty field); anything else raises."""
    if not isinstance(text, str) or not re.fullmatch(r"[0-9]+(,[0-9]+)*", text):
        raise ValueError(f"MEMVUL_SINK_TOKENS={text!r}: expected comma-separated decimal token ids, e.g. '1012,1010'")
    ids = [int(t) for t in text.split(",")]
    if len(ids) > MAX_SINK_TOKENS:
        raise ValueError(f"MEMVUL_SINK_TOKENS: {len(ids)} ids, the list holds at most {MAX_SINK_TOKENS}")
    return ids


def sink_tokens_policy() -> Optional[List[int]]:
    """$MEMVUL_SINK_TOKENS = ID[,ID...], parsed strictly (parse_sink_tokens), or None when it is not set: the sink-token list a guarded engine gets after
    mv_finalize_weights (Engine.set_sink_tokens).  Set while the engine's form is not "guarded" it raises there: a switch that would do nothing is a typo."""
    v = os.environ.get("MEMVUL_SINK_TOKENS")
    return None if v is None else parse_sink_tokens(v)


TOKENIZE_MODES = ("host", "gpu", "gpu-utf8")


def tokenize_policy(option=None) -> str:
    """engine_options["tokenize"] or $MEMVUL_TOKENIZE = host (default) | gpu | gpu-utf8, parsed strictly: where the drivers tokenise the issue reports — "gpu"
    attaches the reader's tokenizer to the model's device (tokenizer.PretrainedTransformerTokenizer.attach_device: ASCII rows through DeviceWordPiece, every
    other row through the tokenizer it already has); "gpu-utf8" attaches it with unicode=True (every row goes to the device in UTF-8; the rows its code-point
    table does not cover come back and go through the tokenizer it already has).  The option wins over the environment; an unknown value raises."""
    if option is not None:
        return _strict(option, 'engine_options["tokenize"]', TOKENIZE_MODES)
    return _strict(os.environ.get("MEMVUL_TOKENIZE", "host"), "MEMVUL_TOKENIZE", TOKENIZE_MODES)


def _sink_token_list(ids) -> List[int]:
    """engine_options["sink_tokens"] / Engine.set_sink_tokens: a sequence of integer token ids (a string is MEMVUL_SINK_TOKENS' syntax), checked as strictly."""
    if isinstance(ids, str):
        return parse_sink_tokens(ids)
    out = []
    for t in ids:
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)):
            raise ValueError(f"sink_tokens: expected integer token ids, got {t!r}")
        out.append(int(t))
    return out


def wants_safe_form(name_or_code) -> bool:
    """True when the compute dtype asked for (None = default_compute()) is the name "safe": MV_F16X8 in the safe form."""
    return wanted_form(name_or_code) == "safe"


def wanted_form(name_or_code) -> Optional[str]:
    """The form a compute dtype NAME stands for ("safe" / "guarded": MV_F16X8 in that form), None for every other name or code."""
    if name_or_code is None:
        name_or_code = default_compute()
    if isinstance(name_or_code, str) and name_or_code.lower() in ("safe", "guarded"):
        return name_or_code.lower()
    return None


NUM_KERNEL_CLASSES = 14

class MvConfig(C.Structure):
    _fields_ = [
        ("vocab_size", C.c_int32), ("hidden", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32),
        ("intermediate", C.c_int32), ("max_pos", C.c_int32), ("type_vocab", C.c_int32), ("proj_dim", C.c_int32),
        ("ln_eps", C.c_float), ("max_tokens", C.c_int32), ("max_batch", C.c_int32), ("max_anchors", C.c_int32),
        ("same_idx", C.c_int32),
    ]


# every entry include/memvul_hip.h declares (ABI_SYMBOLS: tests check the header and the .so against them): name -> (result type, argument types)
_vp, _i32p, _P = C.c_void_p, C.POINTER(C.c_int32), C.POINTER
_SIGNATURES = {
    "mv_create": (C.c_int, [C.c_int, _P(MvConfig), _P(_vp)]),
    "mv_destroy": (None, [_vp]),
    "mv_last_error": (C.c_char_p, [_vp]),
    "mv_sync": (C.c_int, [_vp]),
    "mv_load_tensor": (C.c_int, [_vp, C.c_char_p, _vp, C.c_int, _P(C.c_int64), C.c_int]),
    "mv_finalize_weights": (C.c_int, [_vp, C.c_int]),
    "mv_anchor_reset": (C.c_int, [_vp]),
    "mv_anchor_append": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int]),
    "mv_anchor_count": (C.c_int, [_vp]),
    "mv_anchor_get": (C.c_int, [_vp, _vp]),
    "mv_anchor_set": (C.c_int, [_vp, _vp, C.c_int]),
    "mv_forward": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "mv_forward_ragged": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "mv_forward_ragged_begin": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_int)]),
    "mv_forward_ragged_end": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "mv_encode": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp]),
    "mv_match": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp, _vp]),
    "mv_topk": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _vp]),
    "mv_corpus_upload": (C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_int]),
    "mv_corpus_run": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "mv_corpus_run_len": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int]),
    "mv_corpus_results": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp, _vp, _vp]),
    "mv_corpus_keep": (C.c_int, [_vp, C.c_int, C.c_int]),
    "mv_corpus_rematch": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "mv_corpus_embeddings": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp]),
    "mv_corpus_topk": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp, _vp]),
    "mv_x8_saturation": (C.c_int, [_vp, C.POINTER(C.c_int64), C.c_int]),
    "mv_attention_concentration": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int]),
    "mv_sink_census_enable": (C.c_int, [_vp, C.c_int]),
    "mv_sink_census_read": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, C.c_int, C.c_int]),
    "mv_set_streams": (C.c_int, [_vp, C.c_int]),
    "mv_set_form": (C.c_int, [_vp, C.c_int]),
    "mv_get_form": (C.c_int, [_vp]),
    "mv_form_stats": (C.c_int, [_vp, _P(C.c_int64), _P(C.c_int64), C.c_int]),
    "mv_last_row_forms": (C.c_int, [_vp, _vp, C.c_int]),
    "mv_corpus_row_forms": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp]),
    "mv_set_sink_tokens": (C.c_int, [_vp, _i32p, C.c_int]),
    "mv_get_sink_tokens": (C.c_int, [_vp, _i32p, C.c_int]),
    "mv_route_stats": (C.c_int, [_vp, _P(C.c_int64), C.c_int]),
    "mv_route_scan": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _i32p, C.c_int, C.c_int, _vp]),
    "mv_corpus_route_flags": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp]),
    "mv_profile_enable": (C.c_int, [_vp, C.c_int]),
    "mv_profile_select": (C.c_int, [_vp, C.c_uint32]),
    "mv_profile_read": (C.c_int, [_vp, _P(C.c_double), _P(C.c_int64), C.c_int]),
    "mv_kernel_class_name": (C.c_char_p, [C.c_int]),
    "mv_debug_encode": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    "mv_debug_read": (C.c_int, [_vp, C.c_int, _vp, C.c_int64]),
    "mv_test_gemm": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _P(C.c_float)]),
    "mv_test_gemm_pp": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, _P(C.c_float)]),
    "mv_test_gemm_f32": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, _P(C.c_float)]),
    "mv_test_e4m3": (C.c_int, [_vp, _vp, C.c_int64]),
    "mv_format_records": (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, C.c_int64, C.c_char_p, _vp, _vp, C.c_int64, _P(C.c_int64)]),
    "mv_comm_prepare": (C.c_int, [_vp]),
    "mv_comm_unique_id": (C.c_int, [_vp, _vp, C.c_int]),
    "mv_comm_init": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int]),
    "mv_comm_allgather": (C.c_int, [_vp, _vp, _vp, C.c_int64]),
    "mv_comm_destroy": (C.c_int, [_vp]),
    "mv_comm_info": (C.c_int, [_vp, _P(C.c_int), C.c_int]),
    "mv_device_count": (C.c_int, []),
    "mv_tok_create": (C.c_int, [C.c_int, _vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P(_vp)]),
    "mv_tok_encode": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]),
    "mv_tok_encode_host": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]),
    "mv_tok_kernel_ms": (C.c_int, [_vp, _P(C.c_float)]),
    "mv_tok_set_unicode": (C.c_int, [_vp, _vp, C.c_int]),
    "mv_tok_encode_u8": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]),
    "mv_tok_encode_u8_host": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]),
    "mv_tok_destroy": (None, [_vp]),
    "mv_tok_last_error": (C.c_char_p, [_vp]),
}
ABI_SYMBOLS = list(_SIGNATURES)
PP_FORM_SIGNATURE = (C.c_int64, [_vp, C.c_int])  # mvpp_fixed_launches(handle, reset)


_libs = {}


def load_library(path: Optional[str] = None, dev: bool = False):
    """dlopen the HIP library and declare the prototypes.  Raises RuntimeError if it is missing —
    there is deliberately no other implementation to fall back to.  dev: the development build (the same kernels, plus the
    A/B knobs of DEV_SWITCHES at mv_create); the product never asks for it."""
    path = path or (LIB_PATH_DEV if dev else (os.environ.get("MEMVUL_HIP_LIB") or LIB_PATH))
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError(f"libmemvul_hip.so not found at {path}: build it with `python -m memvul_amd.build` "
                           "(hipcc --offload-arch=gfx950); the MemVul hot path has no CPU fallback")
    try:
        # the product library as always (RTLD_GLOBAL); the development build, which a test process may load NEXT TO it, privately — RTLD_LOCAL keeps its
        # symbols from others, and its -Bsymbolic link (build.DEV_FLAGS) keeps the product's from it
        lib = C.CDLL(path, mode=C.RTLD_LOCAL if path == LIB_PATH_DEV else C.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover
        raise RuntimeError(f"cannot load {path}: {e}") from e
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    # the fixed-form launch counter (include/memvul_hip.h mvpp_fixed_launches): a figure for tests and A/B scripts, outside the mv_ names of ABI_SYMBOLS
    lib.mvpp_fixed_launches.restype, lib.mvpp_fixed_launches.argtypes = PP_FORM_SIGNATURE
    # the three tiny getters the hot loop calls once per batch, bound a second time WITHOUT releasing the interpreter lock around the call (PyDLL): next to other
    # Python threads every release costs the scoring thread a wait for the lock that is far longer than these calls (profiles/r06_*_e2e_dropin.txt)
    quick = C.PyDLL(path)
    for name in ("mv_anchor_count", "mv_x8_saturation", "mv_attention_concentration"):
        fn = getattr(quick, name)
        fn.restype, fn.argtypes = _SIGNATURES[name]
    lib.quick = quick
    _libs[path] = lib
    return lib


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _as(a, dtype) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=dtype)


def _outputs(B: int, G: int, P: int, want_logits: bool, want_probs: bool, want_embed: bool) -> Dict[str, Optional[np.ndarray]]:
    """The result arrays of the forward entry points, in the order those take them (None = not asked for; best / best_idx always)."""
    return {"logits": np.empty((B, G, 2), np.float32) if want_logits else None, "probs": np.empty((B, G, 2), np.float32) if want_probs else None,
            "best": np.empty((B, 2), np.float32), "best_idx": np.empty((B,), np.int32), "embed": np.empty((B, P), np.float32) if want_embed else None}


def _row_forms(f: np.ndarray) -> list:
    """uint8 form codes, one per row (mv_last_row_forms / mv_corpus_row_forms) -> "default" / "safe"."""
    return ["safe" if x == MV_FORM_SAFE else "default" for x in f]


class _Redo(NamedTuple):  # what a ticket begun in the default form under MEMVUL_ON_SINK=safe keeps: its batch, scored again if the form has switched by collection
    ids: np.ndarray
    lens: np.ndarray
    min_tokens: Optional[int]


class Ticket(NamedTuple):  # what forward_by_length_begin hands out; [0] is the state, [1] what it holds, [-1] the redo record
    state: str                     # "pending": the library has the batch; "done": it was scored at once
    held: object                   # pending: the library's ticket (int); done: the results (_outputs)
    B: int                         # pending: rows, and ...
    G: int                         # ... the anchors the batch began with: what the library scatters
    want: Tuple[bool, bool, bool]  # want_logits, want_probs, want_embed
    redo: Optional[_Redo]


@dataclass
class _KeptSweep:  # the last bucketed_sweep(keep= / topk=): its row order, and the bank its stored results cover
    n: int
    inv: np.ndarray  # original row -> row of the length-sorted upload
    embed: bool      # the corpus keeps its embeddings (rematch_sweep needs them)
    epoch: int       # Engine._bank_epoch when the stored results were computed
    covered: int     # the anchors they were computed against


class Engine:
    """One handle <-> one GPU <-> one stream (see include/memvul_hip.h)."""

    def __init__(self, device: int = 0, *, vocab_size: int = 30522, layers: int = 12, max_pos: int = 512,
                 type_vocab: int = 2, ln_eps: float = 1e-12, max_tokens: int = 65536, max_batch: int = 512,
                 max_anchors: int = 1024, same_idx: int = 0, proj_dim: int = 512, dev: bool = False, sink_tokens=None):
        """proj_dim: width of the embedding the matcher runs on — 512 (the header output: use_header=True, every reference
        config) or 768 (use_header=False: the pooler output, no ``_projector_single`` in the state dict).  dev: load the development
        build (tests / A/B scripts: the only one that reads DEV_SWITCHES).  sink_tokens: the sink-token list of the guarded form (what MEMVUL_SINK_TOKENS sets; it wins
        over the environment), applied by load_state_dict — it raises there unless the form is "guarded"."""
        for policy in (on_sink_policy, sink_census_policy, sink_tokens_policy):  # (a malformed switch raises before anything is created)
            policy()
        wanted = None if sink_tokens is None else _sink_token_list(sink_tokens)
        self._lib = load_library(dev=dev)
        self.P = int(proj_dim)
        self.cfg = MvConfig(vocab_size, 768, layers, 12, 3072, max_pos, type_vocab, self.P, ln_eps, max_tokens,
                            max_batch, max_anchors, same_idx)
        self._h, h = None, C.c_void_p()
        self._check(self._lib.mv_create(device, C.byref(self.cfg), C.byref(h)), "mv_create")
        self._h = h
        self.device = device
        self._init_sink_state(precise=False, sink_tokens=wanted)

    def _init_sink_state(self, precise: Optional[bool] = None, sink_tokens: Optional[List[int]] = None):
        """Every attribute Engine keeps on the host besides _lib, _h, P, cfg and device, declared once (no library call: a stand-in engine calls it too; the name is
        from when the MEMVUL_ON_SINK fall-back was all of it).  The methods below only assign to these.  precise None: a stand-in, which has no load_state_dict,
        has said before this call whether it is."""
        self._tickets = []            # forward_by_length_begin: the library's tickets in flight, oldest first
        self._sink_tokens_wanted = sink_tokens  # the constructor's sink_tokens, applied by load_state_dict
        if precise is not None:
            self._precise = precise   # the compute dtype is MV_F16X8: the only one the monitors below speak of (load_state_dict)
        self._dbg = None              # debug_encode: (rows, padded length, lens) of the taps debug_read hands back
        self.comm_rank, self.comm_world = 0, 1  # comm_world: the ranks comm_allgather gathers over (comm_init)
        # the resident corpus
        self._corpus_k = 0            # corpus_keep's topk: the width of corpus_topk (an upload resets it)
        self._sweep_kept: Optional[_KeptSweep] = None
        self._bank_epoch = 0          # bumped by whatever rewrites anchors the bank already holds (anchor_reset, anchor_set, the MEMVUL_ON_SINK=safe switch), not by anchor_append
        # the monitors (_monitors)
        self._conc_warned = self._guard_warned = self._sat_warned = False  # _sink_monitor has tripped (warned, or switched the form); the other two have warned
        self._census = False          # the sink census is on (sink_census_enable / MEMVUL_SINK_CENSUS=1): the sink warning names its top tokens
        self._last_rows = 0           # rows of the last call last_row_forms() speaks of
        # the MEMVUL_ON_SINK fall-back
        self._on_sink = on_sink_policy()  # "warn" | "safe", read once
        self._form = "default"        # the form the passes enqueued now run in (set_form; load_state_dict)
        self._anchor_log = []         # the (ids, lens) of every anchor_append since the last reset: what a switch of form re-encodes the bank from
        self._bank_replayable = True  # False once anchor_set installed embeddings the binding cannot re-encode
        self._corpus_runs = []        # the corpus_run calls since the last corpus_upload: what a switch of form sweeps once more

    # -- plumbing
    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self._lib.mv_last_error(self._h)
            raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mv_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._check(self._lib.mv_sync(self._h), "mv_sync")

    # -- weights
    def load_tensor(self, name: str, arr: np.ndarray):
        dt = {np.dtype(np.float16): MV_F16, np.dtype(np.int64): MV_I64, np.dtype(np.int32): MV_I32}.get(arr.dtype, MV_F32)
        arr = _as(arr, np.float32 if dt == MV_F32 else arr.dtype)  # (every other dtype is loaded as fp32)
        shape = (C.c_int64 * arr.ndim)(*arr.shape)
        self._check(self._lib.mv_load_tensor(self._h, name.encode(), _ptr(arr), dt, shape, arr.ndim), f"mv_load_tensor({name})")

    def load_state_dict(self, sd: Dict[str, np.ndarray], compute_dtype=None):
        """``sd``: reference ``state_dict`` keys -> arrays (torch tensors are converted by the caller)."""
        for k, v in sd.items():
            a = np.asarray(v)
            if a.ndim == 0:
                continue
            self.load_tensor(k, a)
        self._check(self._lib.mv_finalize_weights(self._h, compute_dtype_of(compute_dtype)), "mv_finalize_weights")
        self._precise = compute_dtype_of(compute_dtype) == MV_F16X8
        self._sat_warned = False
        if self._precise and sink_census_policy():  # (the census reads the planes of MV_F16X8: on another compute dtype the switch has nothing to switch on)
            self.sink_census_enable(True)
        if wanted_form(compute_dtype):
            self.set_form(wanted_form(compute_dtype))
        else:
            self._form = {v: k for k, v in FORMS.items()}.get(self._get_form(), "default")  # (MEMVUL_FORM, read by mv_create)
        want, src = self._sink_tokens_wanted, "sink_tokens"
        if want is None:
            want, src = sink_tokens_policy(), "MEMVUL_SINK_TOKENS"
        if want is not None:  # (once, after mv_finalize_weights and after the form is known)
            if self._form != "guarded":
                raise ValueError(f"{src} is set, but this engine's form is {self._form!r}: the sink-token list is acted on in the guarded form only "
                                 "(compute dtype \"guarded\" / MEMVUL_FORM=guarded); it would do nothing here")
            self.set_sink_tokens(want)

    # -- the three forms of MV_F16X8
    def _get_form(self) -> int:
        return int(self._lib.mv_get_form(self._h))

    def _set_form(self, code: int):
        self._check(self._lib.mv_set_form(self._h, code), "mv_set_form")

    @property
    def form(self) -> str:
        """"default", "safe" or "guarded" (include/memvul_hip.h mv_set_form)."""
        return self._form

    def set_form(self, form: str):
        """The form the passes enqueued from now on run in: "default" | "safe" | "guarded" (work in flight keeps its own).  "safe" and "guarded" on an MV_F16
        engine raise."""
        if form not in FORMS:
            raise ValueError(f"unknown form {form!r}: expected one of {sorted(FORMS)}")
        self._set_form(FORMS[form])
        self._form = form

    def form_stats(self, reset: bool = False):
        """(sequences, rescored) of mv_form_stats: the sequences encoded in the guarded form so far and how many of them were encoded again in the safe form."""
        n, r = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.quick.mv_form_stats(self._h, C.byref(n), C.byref(r), int(bool(reset))), "mv_form_stats")
        return int(n.value), int(r.value)

    def last_row_forms(self) -> list:
        """The form ("default" / "safe") that produced each row of the last forward / forward_by_length / forward_by_length_end / encode / anchor_append, in
        that call's row order (mv_last_row_forms)."""
        f = np.empty((self._last_rows,), np.uint8)
        self._check(self._lib.mv_last_row_forms(self._h, _ptr(f), len(f)), "mv_last_row_forms")
        return _row_forms(f)

    def corpus_row_forms(self, first: int, count: int) -> list:
        """The same for rows [first, first + count) of the resident corpus, valid after corpus_results (mv_corpus_row_forms).  After bucketed_sweep the rows are
        those of the length-sorted upload: ``np.argsort(lens, kind="stable")``."""
        f = np.empty((count,), np.uint8)
        self._check(self._lib.mv_corpus_row_forms(self._h, first, count, _ptr(f)), "mv_corpus_row_forms")
        return _row_forms(f)

    # -- the sink-token list of the guarded form
    def set_sink_tokens(self, ids):
        """Replace the sink-token list (mv_set_sink_tokens; [] clears it): in the guarded form a sequence that carries one of these ids at positions 1 .. len - 2
        goes straight into the safe-form pass instead of being encoded twice.  Typically the top rows of sink_census().  MV_F16X8 only; kept in every form,
        acted on in the guarded form; at most MAX_SINK_TOKENS ids inside the vocabulary (the library raises otherwise and keeps the list it had)."""
        ids = _sink_token_list(ids)
        a = (C.c_int32 * max(len(ids), 1))(*ids)
        self._check(self._lib.mv_set_sink_tokens(self._h, a if ids else None, len(ids)), "mv_set_sink_tokens")

    def sink_tokens(self) -> List[int]:
        """The list as the handle holds it (mv_get_sink_tokens)."""
        a = (C.c_int32 * MAX_SINK_TOKENS)()
        n = int(self._lib.mv_get_sink_tokens(self._h, a, MAX_SINK_TOKENS))
        if n < 0:
            self._check(n, "mv_get_sink_tokens")
        return [int(a[i]) for i in range(n)]

    def route_stats(self, reset: bool = False) -> int:
        """Sequences sent directly to the safe form by the list so far (mv_route_stats); form_stats()[1] counts only the sequences encoded twice."""
        n = C.c_int64(0)
        self._check(self._lib.mv_route_stats(self._h, C.byref(n), int(bool(reset))), "mv_route_stats")
        return int(n.value)

    @staticmethod
    def route_scan(ids, lens, tokens, vocab_size: int = 30522, lib=None) -> np.ndarray:
        """The routing rule on the host (mv_route_scan, no GPU): bool [B], True where a row of ids [B, S] carries one of `tokens` at positions 1 .. len - 2."""
        ids, lens = _as(ids, np.int32), _as(lens, np.int32)
        if ids.ndim != 2 or lens.shape != (ids.shape[0],):
            raise ValueError("route_scan: ids [B, S] and lens [B]")
        tokens = _sink_token_list(tokens)
        t = (C.c_int32 * max(len(tokens), 1))(*tokens)
        flags = np.zeros((ids.shape[0],), np.uint8)
        rc = (lib or load_library()).mv_route_scan(_ptr(ids), _ptr(lens), ids.shape[0], ids.shape[1], t if tokens else None, len(tokens), int(vocab_size), _ptr(flags))
        if rc != 0:
            raise RuntimeError(f"mv_route_scan failed ({rc}): bad shape, more than {MAX_SINK_TOKENS} tokens or a token outside [0, {int(vocab_size)})")
        return flags.astype(bool)

    def corpus_route_flags(self, first: int, count: int) -> np.ndarray:
        """bool [count]: what the device kernel flags for rows [first, first + count) of the resident corpus under the current list (mv_corpus_route_flags)."""
        f = np.zeros((count,), np.uint8)
        self._check(self._lib.mv_corpus_route_flags(self._h, first, count, _ptr(f)), "mv_corpus_route_flags")
        return f.astype(bool)

    def x8_saturation(self, reset: bool = False) -> int:
        """MV_F16X8: activation elements (raw stream, attention context, GELU output) that fell outside the +-112 range of the fp8
        correction planes since the engine was created / last reset (mv_x8_saturation; synchronises).  Such an element keeps fp16
        accuracy and loses its correction term."""
        n = C.c_int64(0)
        self._check(self._lib.quick.mv_x8_saturation(self._h, C.byref(n), int(bool(reset))), "mv_x8_saturation")
        return int(n.value)

    def pp_fixed_launches(self, reset: bool = False) -> int:
        """MV_F16X8: kernel launches of this engine that took a fixed-form persistent GEMM (MEMVUL_PP_FORM=fixed, the default; libmemvul_pp_fixed.so) since it was
        created / last reset; always 0 under MEMVUL_PP_FORM=runtime.  A host counter (mvpp_fixed_launches): it does not synchronise."""
        n = int(self._lib.mvpp_fixed_launches(self._h, int(bool(reset))))
        if n < 0:
            raise RuntimeError("mvpp_fixed_launches: no handle")
        return n

    def attention_concentration(self, reset: bool = False):
        """MV_F16X8: (max_collision, items_over, items_total) of mv_attention_concentration — the largest sum_{j >= 2} p[CLS row][j]^2 over every (sequence,
        head, layer) processed so far, the number of them above 0.25 — more than half of a head's [CLS]-row attention on one token that is neither [CLS] nor
        [SEP]: the regime outside the measured envelope of the default form (include/memvul_hip.h) — and the number looked at."""
        m, n, t = C.c_float(0), C.c_int64(0), C.c_int64(0)
        self._check(self._lib.quick.mv_attention_concentration(self._h, C.byref(m), C.byref(n), C.byref(t), int(bool(reset))), "mv_attention_concentration")
        return float(m.value), int(n.value), int(t.value)

    # -- the sink census
    def sink_census_enable(self, on: bool = True):
        """Keep (or stop keeping) the sink census for the passes enqueued from now on (mv_sink_census_enable; MV_F16X8 only, raises otherwise)."""
        self._check(self._lib.mv_sink_census_enable(self._h, int(bool(on))), "mv_sink_census_enable")
        self._census = bool(on)

    def sink_census_read(self, reset: bool = False):
        """The raw histograms of mv_sink_census_read (waits for the work in flight): items uint32 [vocab], share_q20 uint64 [vocab], by_head uint32 [layers, 12]."""
        V, L = int(self.cfg.vocab_size), int(self.cfg.layers)
        items, share, by_head = np.zeros(V, np.uint32), np.zeros(V, np.uint64), np.zeros((L, 12), np.uint32)
        self._check(self._lib.mv_sink_census_read(self._h, _ptr(items), _ptr(share), V, _ptr(by_head), L * 12, int(bool(reset))), "mv_sink_census_read")
        return items, share, by_head

    def sink_census(self, top: int = 10, reset: bool = False, vocab=None):
        """Which tokens the flagged heads sit on: {"tokens": the `top` token ids by flagged items, most first (ties: the lower id), each {token_id, items,
        mean_share (of the [CLS] row's attention, over its items), share_of_flagged_items}, "by_head": uint32 [layers, 12], "flagged_items": their total}.
        vocab: a tokenizer or vocabulary (convert_ids_to_tokens, an id -> string mapping or a sequence of strings): each row also gets "token"."""
        items, share, by_head = self.sink_census_read(reset)
        total = int(items.sum())
        order = np.argsort(-items.astype(np.int64), kind="stable")[:max(int(top), 0)]
        rows = []
        for t in order:
            n = int(items[t])
            if n == 0:
                break
            row = {"token_id": int(t), "items": n, "mean_share": float(share[t]) / n / float(1 << 20), "share_of_flagged_items": n / total}
            if vocab is not None:
                row["token"] = _token_string(vocab, int(t))
            rows.append(row)
        return {"tokens": rows, "by_head": by_head, "flagged_items": total}

    def _census_note(self) -> str:
        """What the one-time sink warning appends with the census on: the top three tokens ("" with it off — the text then stays as it always was)."""
        rows = self.sink_census(top=3)["tokens"] if self._census else []
        if not rows:
            return ""
        return "; sink census, token id (share of the flagged items): " + ", ".join(f"{r['token_id']} ({r['share_of_flagged_items']:.0%})" for r in rows)

    def _monitors(self, level: int = 3) -> bool:
        """Called after the host-synchronous entry points of the precise mode: the three monitors below in this order, each saying its piece ONCE.  Returns True
        when the first of them switched the engine to the safe form (MEMVUL_ON_SINK=safe): the caller redoes its call.  level: the stacklevel that attributes a
        warning to whoever called the public method: 3 when that method calls this itself, 4 through _redo_on_switch."""
        if not self._precise:
            return False
        form = self._form
        for monitor in (self._sink_monitor, self._guard_monitor, self._saturation_monitor):
            text = monitor()
            if text:
                warnings.warn(text, RuntimeWarning, stacklevel=level)
        return self._form != form

    def _sink_monitor(self) -> Optional[str]:
        """The concentration monitor in the default form (the safe form keeps counting, trips nothing; the guarded form answers per sequence): attention sinks
        on ordinary tokens, systematic, not the odd head of the odd sequence, warn or, under MEMVUL_ON_SINK=safe, switch the form (_on_sink_trip)."""
        m, n, t = (0.0, 0, 0) if self._conc_warned or self._form != "default" else self.attention_concentration()
        if t < 100 or n <= 0.02 * t:
            return None
        self._conc_warned = True
        seen = (f"MV_F16X8: in {n} of {t} (sequence, head, layer) items the [CLS] row puts more than half of a head's attention on ONE ordinary token "
                f"(collision mass up to {m:.2f})")
        if self._on_sink == "safe":
            return seen + self._on_sink_trip()
        return (seen + ": the 1e-3 logit tolerance of the default form is backed by measurement for diffuse attention and "
                "for attention sinks on [CLS] / [SEP] only (profiles/r06_n_sink_envelope.txt: 0.8 - 2.7e-3 for such a sink); "
                "MEMVUL_CLS_ASIDE=0 MEMVUL_QKV_ASIDE=qkv is the most conservative form (include/memvul_hip.h mv_attention_concentration)"
                + self._census_note())

    def _guard_monitor(self) -> Optional[str]:
        """The guarded form's rescored share: above GUARDED_WARN_SHARE the safe form is the cheaper one."""
        seqs, resc = (0, 0) if self._form != "guarded" or self._guard_warned else self.form_stats()
        if seqs < 100 or resc <= GUARDED_WARN_SHARE * seqs:
            return None
        self._guard_warned = True
        return (f"MV_F16X8, guarded form: {resc} of {seqs} sequences were encoded again in the safe form — above a share of {GUARDED_WARN_SHARE} the safe "
                "form (compute dtype \"safe\" / set_form(\"safe\") / MEMVUL_FORM=safe) scores the same corpus faster: a guarded sequence costs "
                "1 + 1.34 x that share of a default-form one, a safe-form one 1.34 (include/memvul_hip.h mv_set_form).  If the sinks sit on a few tokens "
                "(sink_census() names them), set_sink_tokens / MEMVUL_SINK_TOKENS sends the sequences that carry them straight to the safe form "
                "instead of encoding them twice")

    def _saturation_monitor(self) -> Optional[str]:
        """The fp8 correction planes clamped something."""
        n = 0 if self._sat_warned else self.x8_saturation()
        if not n:
            return None
        self._sat_warned = True
        return (f"MV_F16X8: {n} activation element(s) exceeded the +-112 range of the fp8 correction planes and were "
                "computed at fp16 accuracy; the 1e-3 logit tolerance is not backed by measurement for this model "
                "(include/memvul_hip.h mv_x8_saturation; Engine.x8_saturation())")

    def _on_sink_trip(self) -> str:
        """MEMVUL_ON_SINK=safe, the monitor has tripped: the safe form for the rest of the engine's life, the counters reset, the anchor bank encoded again in
        that form from the ids anchor_append was given (a bank installed with anchor_set is kept: there is nothing to encode it from); returns what the one warning goes on to say."""
        self.set_form("safe")
        self.attention_concentration(reset=True)
        self._bank_epoch += 1  # (the bank is encoded again below: results stored against it are stale row for row)
        n_bank = self.n_anchors
        if self._bank_replayable:
            self._anchor_reset()
            for ids, lens in self._anchor_log:
                self._anchor_append(ids, lens)
            bank = f"the anchor bank ({n_bank} anchors) was encoded again in the safe form"
        else:
            bank = (f"the anchor bank ({n_bank} anchors) holds embeddings installed with anchor_set and was KEPT as it is: install a bank encoded in the safe form "
                    "to have both sides of the match in it") if n_bank else "the anchor bank is empty"
        return (", outside the measured envelope of the default form: MEMVUL_ON_SINK=safe switched this engine to the SAFE form "
                f"(include/memvul_hip.h mv_set_form) for the rest of its life; {bank}; the call that tripped is redone in the safe form")

    # -- anchors
    def _anchor_reset(self):
        self._check(self._lib.mv_anchor_reset(self._h), "mv_anchor_reset")

    def _anchor_append(self, ids: np.ndarray, lens: np.ndarray):
        self._check(self._lib.mv_anchor_append(self._h, _ptr(ids), _ptr(lens), ids.shape[0], ids.shape[1]), "mv_anchor_append")

    def anchor_reset(self):
        self._anchor_reset()
        self._anchor_log, self._bank_replayable = [], True
        self._bank_epoch += 1

    def anchor_append(self, ids: np.ndarray, lens: np.ndarray):
        ids, lens = _as(ids, np.int32), _as(lens, np.int32)
        self._anchor_append(ids, lens)
        self._last_rows = ids.shape[0]
        if self._on_sink == "safe" and not self._conc_warned:  # (kept only while a switch of form may still need them)
            self._anchor_log.append((ids.copy(), lens.copy()))
        self._monitors()  # (a trip here encodes the whole bank again, these anchors included)

    @property
    def n_anchors(self) -> int:
        return int(self._lib.quick.mv_anchor_count(self._h))

    def anchor_get(self) -> np.ndarray:
        out = np.empty((self.n_anchors, self.P), np.float32)
        self._check(self._lib.mv_anchor_get(self._h, _ptr(out)), "mv_anchor_get")
        return out

    def _check_width(self, a: np.ndarray, what: str):
        if a.ndim != 2 or a.shape[1] != self.P:
            raise ValueError(f"{what}: expected [n, {self.P}] embeddings (mv_config.proj_dim), got {a.shape}")

    def anchor_set(self, v: np.ndarray):
        v = _as(v, np.float32)
        self._check_width(v, "anchor_set")
        self._check(self._lib.mv_anchor_set(self._h, _ptr(v), v.shape[0]), "mv_anchor_set")
        self._anchor_log, self._bank_replayable = [], False
        self._bank_epoch += 1

    # -- hot loop
    def _redo_on_switch(self, rows: int, call):
        """One host-synchronous scoring call, `call` (it allocates its results and hands them back), of `rows` rows, and the monitors after it; when they
        switched the engine to the safe form (MEMVUL_ON_SINK=safe) the call once more, in that form."""
        out = call()
        self._last_rows = rows
        if self._monitors(level=4):
            out = call()
            self._monitors(level=4)  # (the safe form trips nothing: what is left to read is the saturation count)
        return out

    def _scoring(self, entry: str, ids: np.ndarray, lens: np.ndarray, want, *extra):
        """The `call` of forward / forward_by_length: the library's `entry` (mv_forward, or mv_forward_ragged with its min_tokens) on one batch."""
        def call():
            out = _outputs(ids.shape[0], self.n_anchors, self.P, *want)
            self._check(getattr(self._lib, entry)(self._h, _ptr(ids), _ptr(lens), *ids.shape, *extra, *map(_ptr, out.values())), entry)
            return out
        return call

    def forward(self, ids: np.ndarray, lens: np.ndarray, want_logits=True, want_probs=True, want_embed=False):
        ids, lens = _as(ids, np.int32), _as(lens, np.int32)
        return self._redo_on_switch(ids.shape[0], self._scoring("mv_forward", ids, lens, (want_logits, want_probs, want_embed)))

    # tokens below which one pad-to-longest pass is kept as it is (a pass of a few thousand tokens leaves most of the 256 persistent workgroups idle)
    BY_LENGTH_MIN_TOKENS = 16384

    def forward_by_length(self, ids: np.ndarray, lens: np.ndarray, want_logits=True, want_probs=True, want_embed=False, min_tokens: Optional[int] = None):
        """``forward`` on a pad-to-longest batch of UNSORTED issue reports (the reference's collation, predict_memory.py:97-101) without paying for the
        padding, in ONE library call (mv_forward_ragged: one release of the interpreter lock per batch): the rows are grouped by the padded length of their
        OWN token count (64 .. 256 in steps of 64, 384, 512: engine.hip padded_len), every group runs at its own length, and the results go back to the rows'
        places.  A group of fewer than ``min_tokens`` tokens travels with the next longer one (a pass that small leaves most of the chip idle).  Same per-row
        arithmetic as ``forward`` at a different padded length (what Engine.bucketed_sweep does to a resident corpus); a batch whose rows share one padded
        length is bit for bit ``forward`` at that length."""
        ids, lens = _as(ids, np.int32), _as(lens, np.int32)
        B, S = ids.shape
        min_tokens = self.BY_LENGTH_MIN_TOKENS if min_tokens is None else min_tokens
        if B == 0 or B * S < 2 * min_tokens:
            return self.forward(ids, lens, want_logits, want_probs, want_embed)
        return self._redo_on_switch(B, self._scoring("mv_forward_ragged", ids, lens, (want_logits, want_probs, want_embed), int(min_tokens)))

    def forward_by_length_begin(self, ids: np.ndarray, lens: np.ndarray, want_logits=True, want_probs=True, want_embed=False, min_tokens: Optional[int] = None):
        """``forward_by_length`` handed over without waiting for it (mv_forward_ragged_begin): returns a ticket for ``forward_by_length_end``.  One batch per
        workspace set may be in flight (two by default); collect in the order of the calls.  A batch the asynchronous entry cannot take (too small to be
        worth grouping, more than max_batch rows, every workspace set busy: the library's MV_ERR_CAPACITY) is scored at once and its ticket holds the results.
        MEMVUL_ON_SINK=safe: while the engine is in the default form a ticket remembers that and keeps its ``ids`` / ``lens`` — collected after the engine has
        switched to the safe form, it is scored again (``forward_by_length_end``)."""
        ids, lens = _as(ids, np.int32), _as(lens, np.int32)
        B, S = ids.shape
        mt = self.BY_LENGTH_MIN_TOKENS if min_tokens is None else min_tokens
        want = (bool(want_logits), bool(want_probs), bool(want_embed))
        redo = _Redo(ids, lens, min_tokens) if self._on_sink == "safe" and self._form == "default" else None
        if B > 0 and B * S >= 2 * mt:
            t = C.c_int(-1)
            rc = self._lib.mv_forward_ragged_begin(self._h, _ptr(ids), _ptr(lens), B, S, int(mt), int(want_logits), int(want_probs), int(want_embed), C.byref(t))
            if rc == 0:
                self._tickets.append(t.value)
                return Ticket("pending", t.value, B, self.n_anchors, want, redo)
            if rc != -5:  # (MV_ERR_CAPACITY: below)
                self._check(rc, "mv_forward_ragged_begin")
        out = self.forward_by_length(ids, lens, want_logits, want_probs, want_embed, min_tokens)
        return Ticket("done", out, B, 0, want, None if self._form == "safe" else redo)  # (a trip inside that call: the results are the safe form's already)

    def _rescore(self, ticket: Ticket):
        """A ticket begun in the default form, collected after the switch: its batch once more, synchronously, in the safe form."""
        return self.forward_by_length(ticket.redo.ids, ticket.redo.lens, *ticket.want, ticket.redo.min_tokens)

    def forward_by_length_end(self, ticket: Ticket):
        """The results of a ``forward_by_length_begin`` ticket.  Collecting consumes the ticket, also when this call raises.  MEMVUL_ON_SINK=safe: the monitor is
        read at EVERY collection while the engine is in the default form (that read waits for the batch in flight behind this one: the price of the guarantee
        that no result handed out after the trip comes from the default form), and a ticket begun in the default form is scored again after the switch."""
        redo = ticket.redo
        if ticket.state == "done":
            return self._rescore(ticket) if redo is not None and self._form == "safe" else ticket.held
        t = ticket.held
        if not self._tickets or self._tickets[0] != t:
            raise RuntimeError("forward_by_length_end: tickets are collected in the order they were issued")
        out = _outputs(ticket.B, ticket.G, self.P, *ticket.want)
        self._tickets.pop(0)
        self._check(self._lib.mv_forward_ragged_end(self._h, t, *map(_ptr, out.values())), "mv_forward_ragged_end")
        self._last_rows = ticket.B
        stale = redo is not None and self._form == "safe"  # begun before the switch: its results are the default form's
        if not self._tickets or (redo is not None and not stale):  # (the counters are read after a synchronisation of EVERY stream: with the next batch in flight that would wait for it — holding the lock)
            stale = self._monitors() or stale
        return self._rescore(ticket) if stale and redo is not None else out

    def encode(self, ids: np.ndarray, lens: np.ndarray) -> np.ndarray:
        ids, lens = _as(ids, np.int32), _as(lens, np.int32)

        def call():
            out = np.empty((ids.shape[0], self.P), np.float32)
            self._check(self._lib.mv_encode(self._h, _ptr(ids), _ptr(lens), ids.shape[0], ids.shape[1], _ptr(out)), "mv_encode")
            return out
        return self._redo_on_switch(ids.shape[0], call)

    def match(self, u: np.ndarray):
        u = _as(u, np.float32)
        self._check_width(u, "match")
        out = _outputs(u.shape[0], self.n_anchors, self.P, True, True, False)
        del out["embed"]  # (the matcher has none to hand back)
        self._check(self._lib.mv_match(self._h, _ptr(u), u.shape[0], *map(_ptr, out.values())), "mv_match")
        return out

    def topk(self, u: np.ndarray, k: int):
        u = _as(u, np.float32)
        self._check_width(u, "topk")
        p, i = np.empty((u.shape[0], k), np.float32), np.empty((u.shape[0], k), np.int32)
        self._check(self._lib.mv_topk(self._h, _ptr(u), u.shape[0], k, _ptr(p), _ptr(i)), "mv_topk")
        return p, i

    # -- resident corpus
    def corpus_upload(self, ids: np.ndarray, lens: np.ndarray):
        ids, lens = _as(ids, np.int32), _as(lens, np.int32)
        self._check(self._lib.mv_corpus_upload(self._h, _ptr(ids), _ptr(lens), ids.shape[0], ids.shape[1]), "mv_corpus_upload")
        self._corpus_runs, self._corpus_k, self._sweep_kept = [], 0, None  # (an upload resets mv_corpus_keep)

    def corpus_run(self, first: int, count: int, batch: int, keep_probs: bool = False, s_eff: int = 0):
        """Enqueue IRs [first, first+count) of the resident corpus in batches of `batch` (asynchronous).  s_eff > 0:
        process only the first s_eff tokens of each row (length-bucketed sweeps, see bucketed_sweep)."""
        self._check(self._lib.mv_corpus_run_len(self._h, first, count, batch, int(keep_probs), int(s_eff)), "mv_corpus_run_len")
        if self._on_sink == "safe" and self._form == "default":
            self._corpus_runs.append((first, count, batch, keep_probs, s_eff))

    def corpus_keep(self, embed: bool = True, topk: int = 0):
        """What the sweeps of the corpus just uploaded keep besides best / best_idx (mv_corpus_keep; after corpus_upload, before its first corpus_run): the rows'
        embeddings — what corpus_rematch matches again against a changed anchor bank, without the encoder — and / or their ``topk`` best anchors."""
        self._check(self._lib.mv_corpus_keep(self._h, int(bool(embed)), int(topk)), "mv_corpus_keep")
        self._corpus_k = int(topk)

    def corpus_rematch(self, first: int, count: int, g_first: int = 0, keep_probs: bool = False):
        """The matcher alone over the kept embeddings of rows [first, first + count) against the bank as it is now (mv_corpus_rematch; it waits).  g_first = 0
        rewrites the stored results; 0 < g_first < n_anchors: the caller states that they were computed against a bank whose first g_first anchors are the
        present ones, and only the anchors from g_first on are matched and merged in (same bytes).  rematch_sweep chooses g_first by itself."""
        self._check(self._lib.mv_corpus_rematch(self._h, first, count, int(g_first), int(bool(keep_probs))), "mv_corpus_rematch")

    def corpus_embeddings(self, first: int, count: int) -> np.ndarray:
        """fp32 [count, P]: the kept embeddings of rows [first, first + count) (mv_corpus_embeddings)."""
        out = np.empty((count, self.P), np.float32)
        self._check(self._lib.mv_corpus_embeddings(self._h, first, count, _ptr(out)), "mv_corpus_embeddings")
        return out

    def corpus_topk(self, first: int, count: int):
        """(P(same) fp32 [count, k], anchor index int32 [count, k]) of rows [first, first + count), k as given to corpus_keep (mv_corpus_topk)."""
        p, i = np.empty((count, self._corpus_k), np.float32), np.empty((count, self._corpus_k), np.int32)
        self._check(self._lib.mv_corpus_topk(self._h, first, count, _ptr(p), _ptr(i)), "mv_corpus_topk")
        return p, i

    def bucketed_sweep(self, ids: np.ndarray, lens: np.ndarray, batch: int, with_probs: bool = False, keep: bool = False, topk: int = 0):
        """Score a ragged corpus with each batch padded to ITS longest member (the reference's pad-to-longest collation,
        predict_memory.py:97-101) instead of the corpus-wide S: rows are sorted by length, uploaded once, swept batch by
        batch at that batch's length (rounded up to 64 tokens), and the results are returned in the ORIGINAL order.
        keep / topk: the corpus keeps its embeddings / the k best anchors of every row (corpus_keep), and the engine remembers the order of the upload:
        rematch_sweep() then scores the same rows against a changed bank without encoding them again, sweep_topk() returns the top-k lists."""
        ids, lens = _as(ids, np.int32), _as(lens, np.int32)
        n = ids.shape[0]
        order = np.argsort(lens, kind="stable")
        self.corpus_upload(ids[order], lens[order])
        if keep or topk:
            self.corpus_keep(embed=bool(keep), topk=topk)
        sl = lens[order]
        for s0 in range(0, n, batch):
            nb = min(batch, n - s0)
            self.corpus_run(s0, nb, nb, keep_probs=with_probs, s_eff=int(sl[s0 + nb - 1]))
        best, idx, ps = self.corpus_results(0, n, with_probs=with_probs)
        inv = np.empty(n, np.int64)
        inv[order] = np.arange(n)
        if keep or topk:  # (after corpus_results: a MEMVUL_ON_SINK=safe trip in there swept again, against the bank it encoded again)
            self._sweep_kept = _KeptSweep(n, inv, bool(keep), self._bank_epoch, self.n_anchors)
        return best[inv], idx[inv], (ps[inv] if ps is not None else None)

    def rematch_sweep(self, with_probs: bool = False):
        """The rows of the last ``bucketed_sweep(..., keep=True)`` against the anchor bank as it is NOW, by the matcher alone: ``(best, idx, p_same | None)`` in
        the ORIGINAL row order, the bytes sweeping again would give.  When the bank has only been appended to since the stored results were computed (no
        anchor_reset, anchor_set or switch of form in between) and P(same) is not asked for, only the new anchors are matched and merged in."""
        st = self._sweep_kept
        if st is None or not st.embed:
            raise RuntimeError("rematch_sweep: the resident corpus keeps no embeddings — sweep it with bucketed_sweep(..., keep=True) first")
        G = self.n_anchors
        appended = st.epoch == self._bank_epoch and G >= st.covered and not with_probs
        self.corpus_rematch(0, st.n, st.covered if appended else 0, keep_probs=with_probs)
        best, idx, ps = self.corpus_results(0, st.n, with_probs=with_probs)
        st.epoch, st.covered = self._bank_epoch, self.n_anchors
        return best[st.inv], idx[st.inv], (ps[st.inv] if ps is not None else None)

    def sweep_topk(self):
        """(P(same) [n, k], anchor index [n, k]) of the last ``bucketed_sweep(..., topk=k)``, in the ORIGINAL row order."""
        st = self._sweep_kept
        if st is None or not self._corpus_k:
            raise RuntimeError("sweep_topk: the resident corpus keeps no top-k lists — sweep it with bucketed_sweep(..., topk=k) first")
        p, i = self.corpus_topk(0, st.n)
        return p[st.inv], i[st.inv]

    def sweep_embeddings(self, first: int = 0, count: Optional[int] = None, chunk: int = 65536) -> np.ndarray:
        """fp32 [count, P]: the kept embeddings of rows [first, first + count) of the last ``bucketed_sweep(..., keep=True)``, in the ORIGINAL row order.  The
        upload is sorted by length, so the rows asked for lie scattered over it: the span that holds them is downloaded ``chunk`` rows at a time (corpus_embeddings)
        and the wanted rows are picked out — one pass over the corpus when all rows are asked for."""
        st = self._sweep_kept
        if st is None or not st.embed:
            raise RuntimeError("sweep_embeddings: the resident corpus keeps no embeddings — sweep it with bucketed_sweep(..., keep=True) first")
        count = st.n - first if count is None else count
        if first < 0 or count < 0 or first + count > st.n or chunk < 1:
            raise ValueError(f"sweep_embeddings: rows [{first}, {first} + {count}) of {st.n}, chunk {chunk}")
        out = np.empty((count, self.P), np.float32)
        if count == 0:
            return out
        pos = st.inv[first:first + count]
        lo, hi = int(pos.min()), int(pos.max()) + 1
        where = np.full(hi - lo, -1, np.int64)  # row of the upload -> row of `out`
        where[pos - lo] = np.arange(count)
        for s0 in range(lo, hi, chunk):
            w = where[s0 - lo:s0 - lo + chunk]
            take = w >= 0
            if take.any():
                out[w[take]] = self.corpus_embeddings(s0, len(w))[take]
        return out

    def corpus_results(self, first: int, count: int, with_probs: bool = False):
        best = np.empty((count, 2), np.float32)
        idx = np.empty((count,), np.int32)
        ps = np.empty((count, self.n_anchors), np.float32) if with_probs else None
        self._check(self._lib.mv_corpus_results(self._h, first, count, _ptr(best), _ptr(idx), _ptr(ps)), "mv_corpus_results")
        if self._monitors():  # MEMVUL_ON_SINK=safe tripped: the sweeps over the resident corpus once more, in the safe form
            runs, self._corpus_runs = self._corpus_runs, []
            for r in runs:
                self.corpus_run(*r)
            self._check(self._lib.mv_corpus_results(self._h, first, count, _ptr(best), _ptr(idx), _ptr(ps)), "mv_corpus_results")
        return best, idx, ps

    # -- multi-GPU exchange (RCCL bound inside the library; no torch in the process)
    def comm_prepare(self):
        """dlopen librccl.so and resolve its entry points (raises if RCCL is not usable in this process)."""
        self._check(self._lib.mv_comm_prepare(self._h), "mv_comm_prepare")

    def comm_unique_id(self) -> bytes:
        """Rank 0: the 128-byte ncclUniqueId every rank passes to comm_init."""
        buf = C.create_string_buffer(128)
        n = self._lib.mv_comm_unique_id(self._h, buf, 128)
        if n <= 0:
            self._check(n, "mv_comm_unique_id")
        return buf.raw[:n]

    def comm_init(self, rank: int, world: int, unique_id: Optional[bytes] = None):
        uid = None if unique_id is None else C.c_char_p(bytes(unique_id))
        self._check(self._lib.mv_comm_init(self._h, int(rank), int(world), uid, 0 if unique_id is None else len(unique_id)), "mv_comm_init")
        self.comm_world = int(world)

    def comm_allgather(self, block: np.ndarray) -> np.ndarray:
        """Every rank contributes a same-shape array; returns ``[world, *block.shape]`` in rank order."""
        block = np.ascontiguousarray(block)
        out = np.empty((self.comm_world,) + block.shape, block.dtype)
        if block.nbytes:
            self._check(self._lib.mv_comm_allgather(self._h, _ptr(block), _ptr(out), block.nbytes), "mv_comm_allgather")
        return out

    def comm_destroy(self):
        self._check(self._lib.mv_comm_destroy(self._h), "mv_comm_destroy")
        self.comm_rank, self.comm_world = 0, 1

    def comm_info(self) -> Dict[str, int]:
        """What RCCL itself says about the live communicator: its rank count (0 = none), this rank, the RCCL version code, and
        the world mv_comm_allgather gathers over."""
        info = (C.c_int * 4)()
        self._check(self._lib.mv_comm_info(self._h, info, 4), "mv_comm_info")
        return {"rccl_ranks": int(info[0]), "rccl_rank": int(info[1]), "rccl_version": int(info[2]), "world": int(info[3])}

    # -- measurement / debug
    def set_streams(self, n: int):
        """Batches of the resident sweep in flight at once (1 or 2)."""
        self._check(self._lib.mv_set_streams(self._h, int(n)), "mv_set_streams")

    def profile_enable(self, on: bool = True):
        self._check(self._lib.mv_profile_enable(self._h, int(on)), "mv_profile_enable")

    def profile_select(self, names=None):
        """Restrict HIP-event recording to the named kernel classes (None = all)."""
        all_names = names and [self._lib.mv_kernel_class_name(i).decode() for i in range(NUM_KERNEL_CLASSES)]
        mask = 0xFFFFFFFF if names is None else sum({1 << all_names.index(nm) for nm in names})
        self._check(self._lib.mv_profile_select(self._h, mask), "mv_profile_select")

    def profile_read(self) -> Dict[str, Tuple[float, int]]:
        ms = (C.c_double * NUM_KERNEL_CLASSES)()
        n = (C.c_int64 * NUM_KERNEL_CLASSES)()
        self._check(self._lib.mv_profile_read(self._h, ms, n, NUM_KERNEL_CLASSES), "mv_profile_read")
        return {self._lib.mv_kernel_class_name(i).decode(): (float(ms[i]), int(n[i])) for i in range(NUM_KERNEL_CLASSES)}

    def debug_encode(self, ids, lens, n_layers: int):
        ids, lens = _as(ids, np.int32), _as(lens, np.int32)
        self._check(self._lib.mv_debug_encode(self._h, _ptr(ids), _ptr(lens), ids.shape[0], ids.shape[1], n_layers), "mv_debug_encode")
        S = ids.shape[1]
        self._dbg = (ids.shape[0], (S + 63) // 64 * 64 if S <= 256 else (S + 127) // 128 * 128, lens.copy())  # engine.hip padded_len

    def tail_encode(self, ids, lens) -> np.ndarray:
        """encode(ids, lens) — the ordinary, pruned forward — on a development-build engine created with MEMVUL_DEBUG_TAIL=1: the embeddings, and debug_read then
        hands back the tail taps 22 - 34 of that pass beside the taps of the tail's inputs (0, 1, 3, 4, 8, 9, 12, 13, 18, 19: the pruned layer overwrites none)."""
        ids, lens = _as(ids, np.int32), _as(lens, np.int32)
        u = self.encode(ids, lens)
        S = ids.shape[1]
        self._dbg = (ids.shape[0], (S + 63) // 64 * 64 if S <= 256 else (S + 127) // 128 * 128, lens.copy())  # engine.hip padded_len
        return u

    def debug_read(self, buffer: int, pad_rows: bool = False) -> np.ndarray:
        """pad_rows (the per-token raw planes 11, 13 - 15, 17, 19 only): the rows PAST the pass' B * Sp tokens, up to the end of its last 256-row tile, as
        [rows, width] in the engine's order — rows no token lives in, which the persistent GEMMs compute like any other."""
        B, Sp, lens = self._dbg
        if pad_rows:
            width, dt = {11: (2 * 768, np.uint8), 13: (6, np.float32), 14: (6, np.float32), 15: (2 * 768, np.uint8), 17: (2 * 3072, np.uint8), 19: (768, np.float16)}[buffer]
            T = B * Sp
            full = np.empty(((T + 255) // 256 * 256, width), dt)
            self._check(self._lib.mv_debug_read(self._h, buffer, _ptr(full), full.nbytes), "mv_debug_read")
            return full[T:]
        shapes = {
            0: ((B, Sp, 768), np.float32), 1: ((B, Sp, 768), np.float16), 2: ((B, 12, Sp, 64), np.float16),
            3: ((B, 12, Sp, 64), np.float16), 4: ((B, 12, 64, Sp), np.float16), 5: ((B, Sp, 768), np.float16),
            6: ((B, Sp, 3072), np.float16), 7: ((B, 12, Sp, 64), np.float16), 8: ((B, 12, Sp, 64), np.float16), 9: ((B, 12, 64, Sp), np.float16),
            10: ((B, self.P), np.float32),
            # the raw planes of the persistent path (include/memvul_hip.h; what a pass stopped by MEMVUL_DEBUG_STOP leaves).  Per-token planes come back in token
            # order like 0 - 9; the COMPACT special-row buffers 12, 16, 18, 20 stay in the engine's [2 b + row] order: row 0 = the [CLS] token, row 1 = the LAST
            # token of sequence b (token 1 when the sequence has fewer than 3).  16 and 20 are flat: their row pitch is the N of the launch that wrote them
            # (768 / 2304 / 3072), so rows are x[:2 * B * N].reshape(2 * B, N)
            11: ((B, Sp, 2 * 768), np.uint8), 12: ((2 * B, 768), np.float16), 13: ((B, Sp, 3, 2), np.float32), 14: ((B, Sp, 3, 2), np.float32),
            15: ((B, Sp, 2 * 768), np.uint8), 16: ((2 * B * 3072,), np.float16), 17: ((B, Sp, 2 * 3072), np.uint8), 18: ((B, 12, 64, 2), np.float16),
            19: ((B, Sp, 768), np.float16), 20: ((2 * B * 3072,), np.float32), 21: (((B * Sp + 255) // 256,), np.int32),
            # the tail taps (development build, MEMVUL_DEBUG_TAIL=1; tail_encode): what each launch of the pruned last layer's [CLS] tail wrote, B rows each —
            # 22 / 23 the gathered c32 / c16, 24 the [CLS] query, 25 the context (fp32 in MV_F16X8, fp16 in MV_F16), 26 c32 after the output projection, 27 / 28
            # c32 / c16 after LayerNorm 1, 29 the FFN intermediate (fp32 / fp16 likewise), 30 c32 after FFN-2, 31 c32 after LayerNorm 2, 32 the pooler output,
            # 33 the embedding u; 34 int32 [3] = (pruned passes tapped since the engine was created, rows and padded length of the last pass)
            22: ((B, 768), np.float32), 23: ((B, 768), np.float16), 24: ((B, 768), np.float32), 25: ((B, 768), np.float32 if self._precise else np.float16),
            26: ((B, 768), np.float32), 27: ((B, 768), np.float32), 28: ((B, 768), np.float16), 29: ((B, 3072), np.float32 if self._precise else np.float16),
            30: ((B, 768), np.float32), 31: ((B, 768), np.float32), 32: ((B, 768), np.float32), 33: ((B, self.P), np.float32), 34: ((3,), np.int32),
            # the fp32 planes of the reference form (MV_F32 handles only): 35 Q (1/8 folded) | K | V, 36 the attention context, 37 the GELU output; token order
            # (this compute dtype swaps no special rows)
            35: ((B, Sp, 3 * 768), np.float32), 36: ((B, Sp, 768), np.float32), 37: ((B, Sp, 3072), np.float32),
        }
        shape, dt = shapes[buffer]
        out = np.empty(shape, dt)
        self._check(self._lib.mv_debug_read(self._h, buffer, _ptr(out), out.nbytes), "mv_debug_read")
        if self._precise and buffer in self._TOKEN_AXIS:
            # MV_F16X8 keeps the LAST token of every sequence in row 1 and token 1 in the last token's row (the "special rows" of
            # misc_kernels.h embed_ln_kernel; only the [CLS] row's result leaves the encoder): hand the taps back in token order
            ax = self._TOKEN_AXIS[buffer]
            for b in range(B):
                n = int(lens[b])
                if n >= 3:
                    rows = np.moveaxis(out[b], ax - 1, 0)  # (a view: the token axis of sequence b first)
                    rows[[1, n - 1]] = rows[[n - 1, 1]]
        return out

    # debug buffer -> its token axis (7 - 9: the lo planes of 2 - 4; 11, 13 - 15, 17: the per-token raw planes)
    _TOKEN_AXIS = {0: 1, 1: 1, 2: 2, 3: 2, 4: 3, 5: 1, 6: 1, 7: 2, 8: 2, 9: 3, 11: 1, 13: 1, 14: 1, 15: 1, 17: 1}

    def _timed(self, entry: str, *args) -> float:
        """A mv_test_gemm* entry: it runs its kernel `iters` times and says what one run took, in milliseconds."""
        ms = C.c_float(0)
        self._check(getattr(self._lib, entry)(self._h, *args, C.byref(ms)), entry)
        return float(ms.value)

    def test_gemm(self, A16: np.ndarray, W16: np.ndarray, bias: Optional[np.ndarray], variant: int = 0, iters: int = 1):
        A16, W16 = _as(A16, np.float16), _as(W16, np.float16)
        M, K = A16.shape
        N = W16.shape[0]
        bias = None if bias is None else _as(bias, np.float32)
        out = np.empty((M, N), np.float32)
        return out, self._timed("mv_test_gemm", variant, M, N, K, _ptr(A16), _ptr(W16), _ptr(bias), _ptr(out), iters)

    def test_gemm_pp(self, A: np.ndarray, W: np.ndarray, bias: np.ndarray, x8=False, iters: int = 1):
        """The persistent FFN-1 kernel on fp32 operands (unit row statistics): fp16 gelu(A W^T + bias) [M][N]; x8: the MV_F16X8
        build (True / 1: both correction terms, 2: the weight-side term A_hi8 W_lo8 only, the QKV projection's form), also returning
        the [lo8 | hi8] e4m3 planes of the output as uint8 [M][2 N]."""
        A, W, bias = _as(A, np.float32), _as(W, np.float32), _as(bias, np.float32)
        M, K = A.shape
        N = W.shape[0]
        out = np.empty((M, N), np.float16)
        out8 = np.empty((M, 2 * N), np.uint8) if x8 else None
        return out, out8, self._timed("mv_test_gemm_pp", int(x8), M, N, K, _ptr(A), _ptr(W), _ptr(bias), _ptr(out), _ptr(out8), iters)

    GEMM_F32_ACTS = {"bias": 0, "gelu": 1, "res": 2}

    def test_gemm_f32(self, A: np.ndarray, W: np.ndarray, bias: Optional[np.ndarray], res: Optional[np.ndarray] = None, act: str = "bias", iters: int = 1):
        """The MV_F32 GEMM on fp32 operands: act(A W^T + bias) (+ res) [M][N] fp32; act "bias" | "gelu" | "res" (M, N % 128, K % 32)."""
        A, W = _as(A, np.float32), _as(W, np.float32)
        M, K = A.shape
        N = W.shape[0]
        bias = None if bias is None else _as(bias, np.float32)
        res = None if res is None else _as(res, np.float32)
        out = np.empty((M, N), np.float32)
        return out, self._timed("mv_test_gemm_f32", self.GEMM_F32_ACTS[act], M, N, K, _ptr(A), _ptr(W), _ptr(bias), _ptr(res), _ptr(out), iters)


def _token_string(vocab, token_id: int) -> str:
    """The string of a token id from a tokenizer (convert_ids_to_tokens), a mapping id -> string, or a sequence of strings; "" where it has none."""
    if hasattr(vocab, "convert_ids_to_tokens"):
        t = vocab.convert_ids_to_tokens([token_id])
        return str(t[0]) if t else ""
    if hasattr(vocab, "get"):
        return str(vocab.get(token_id, ""))
    return str(vocab[token_id]) if 0 <= token_id < len(vocab) else ""


def device_count() -> int:
    """GPUs visible to this process (0 without one)."""
    return max(0, int(load_library().mv_device_count()))


def e4m3_bits(x: np.ndarray) -> np.ndarray:
    """OCP e4m3fn bits of fp32 values through the library's host-side encoder (the one that builds the MV_F16X8 weight planes)."""
    x = _as(x, np.float32)
    out = np.empty(x.shape, np.uint8)
    if load_library().mv_test_e4m3(_ptr(x), _ptr(out), x.size) != 0:
        raise RuntimeError("mv_test_e4m3 failed")
    return out


def e4m3_decode(b: np.ndarray) -> np.ndarray:
    """fp32 value of OCP e4m3fn bits (0x7f / 0xff = NaN)."""
    b = np.asarray(b, np.uint8).astype(np.int32)
    e, m = (b >> 3) & 15, b & 7
    v = np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e - 10))
    v = np.where((e == 15) & (m == 7), np.nan, v)
    return (np.where(b & 0x80, -v, v)).astype(np.float32)


def _packed(strings) -> Tuple[bytes, np.ndarray]:
    """Byte strings back to back + int64 offsets [n + 1]."""
    off = np.zeros(len(strings) + 1, np.int64)
    if len(strings):
        np.cumsum(np.fromiter((len(b) for b in strings), np.int64, len(strings)), out=off[1:])
    return b"".join(strings), off


# one entry of the code-point table of mv_tok_set_unicode (include/memvul_hip.h; memvul_amd/csrc/wordpiece.h WpCp)
CODE_POINT_DTYPE = np.dtype([("out", np.uint8, 12), ("nbytes", np.uint8), ("cls", np.uint8), ("covered", np.uint8), ("nchars", np.uint8)])
CODE_POINTS = 0x20000


class DeviceWordPiece:
    """The device WordPiece tokenizer (include/memvul_hip.h mv_tok_*): ASCII text -> the ids BertTokenizerFast's backend gives it.  ``vocab``: the pieces
    as bytes, index = id (b"" for an unused id); ``literals``: the tokenizer's added tokens as bytes — a row that holds one, or a byte >= 0x80, comes back with
    status 1, length 0 and a zero id row, for the caller to encode with the tokenizer it has.  ``device=None``: the table only; such an object serves
    ``encode_host`` (the rule on the CPU: tests and reference) and needs no GPU.  After ``set_unicode`` (a code-point table: tokenizer.code_point_table)
    ``encode_u8`` / ``encode_u8_host`` take text in UTF-8 and hand back only what the table does not cover (status 2).  Its own object in the library: usable from one thread while another drives
    an ``Engine`` of the same device; not re-entrant itself."""

    def __init__(self, vocab, literals, unk_id: int, cls_id: int, sep_id: int, max_chars_per_word: int = 100, lowercase: bool = True,
                 device: Optional[int] = 0, lib=None):
        self._lib = lib or load_library()
        self._t = None
        vb, vo = _packed(list(vocab))
        lb, lo = _packed(list(literals))
        t = C.c_void_p()
        self.device = -1 if device is None else int(device)
        self._check(self._lib.mv_tok_create(self.device, vb, _ptr(vo), len(vo) - 1, lb, _ptr(lo), len(lo) - 1, int(unk_id), int(cls_id), int(sep_id),
                                            int(max_chars_per_word), 1 if lowercase else 0, C.byref(t)), "mv_tok_create")
        self._t = t

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self._lib.mv_tok_last_error(self._t)  # (None while mv_tok_create runs: the library's own last error)
            raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "_t", None):
            self._lib.mv_tok_destroy(self._t)
            self._t = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _run(self, fn, name: str, packed: bytes, offsets, max_length: int, add_special: bool):
        off = _as(offsets, np.int64)
        n = len(off) - 1
        if n < 0:
            raise ValueError(f"{name}: offsets must hold n + 1 values")
        ids, lens, status = np.zeros((n, int(max_length)), np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
        self._check(fn(self._t, packed, _ptr(off), n, int(max_length), 1 if add_special else 0, _ptr(ids), _ptr(lens), _ptr(status)), name)
        return ids, lens, status

    def encode(self, packed: bytes, offsets, max_length: int, add_special: bool = True):
        """The kernel: text i = packed[offsets[i]:offsets[i + 1]] -> (ids int32 [n, max_length] zero-padded, lens int32 [n], status uint8 [n])."""
        return self._run(self._lib.mv_tok_encode, "mv_tok_encode", packed, offsets, max_length, add_special)

    def kernel_ms(self) -> float:
        """The kernel's own time of the last ``encode`` (HIP events around each chunk's launch), in milliseconds."""
        ms = C.c_float()
        rc = self._lib.mv_tok_kernel_ms(self._t, C.byref(ms))
        if rc != 0:
            raise RuntimeError(f"mv_tok_kernel_ms failed ({rc})")
        return float(ms.value)

    def encode_host(self, packed: bytes, offsets, max_length: int, add_special: bool = True):
        """The same rule, single-threaded on the CPU (mv_tok_encode_host)."""
        return self._run(self._lib.mv_tok_encode_host, "mv_tok_encode_host", packed, offsets, max_length, add_special)

    def set_unicode(self, entries):
        """Attach a code-point table (mv_tok_set_unicode): uint8 [n, 16], row i for code point i, laid out as include/memvul_hip.h says (CODE_POINT_DTYPE).
        ``encode_u8`` / ``encode_u8_host`` need one; ``encode`` / ``encode_host`` do not change."""
        e = np.ascontiguousarray(entries)
        if e.dtype == CODE_POINT_DTYPE:
            e = e.view(np.uint8).reshape(-1, 16)
        if e.dtype != np.uint8 or e.ndim != 2 or e.shape[1] != 16:
            raise ValueError("set_unicode: entries must be uint8 [n, 16] or CODE_POINT_DTYPE [n]")
        self._check(self._lib.mv_tok_set_unicode(self._t, _ptr(e), len(e)), "mv_tok_set_unicode")

    def encode_u8(self, packed: bytes, offsets, max_length: int, add_special: bool = True):
        """The UTF-8 kernel (mv_tok_encode_u8): as ``encode`` for text in UTF-8; status 0 tokenised, 1 an added-token literal, 2 malformed or not covered."""
        return self._run(self._lib.mv_tok_encode_u8, "mv_tok_encode_u8", packed, offsets, max_length, add_special)

    def encode_u8_host(self, packed: bytes, offsets, max_length: int, add_special: bool = True):
        """The UTF-8 rule, single-threaded on the CPU (mv_tok_encode_u8_host)."""
        return self._run(self._lib.mv_tok_encode_u8_host, "mv_tok_encode_u8_host", packed, offsets, max_length, add_special)
