"""The index over a kept corpus that per-anchor retrieval (retrieve.py), per-anchor claims (claims.py), the anchor-bank audit (bank.py) and per-anchor ranking
quality (rank.py) share: the rows of a corpus on one GPU, appended as they arrive, and the calls that are the same in all four libraries (csrc/kept_index.h is the
C++ side).  Each of the four derives its class from KeptIndex and adds only its questions."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _check_array(a, what: str, width: int) -> np.ndarray:
    """float32, C-contiguous, [n, width]: checked, never converted (a silent copy of a 2.5 GB corpus is not a service)."""
    if not isinstance(a, np.ndarray):
        raise TypeError(f"{what}: a numpy array, not {type(a).__name__}")
    if a.dtype != np.float32:
        raise TypeError(f"{what}: float32, not {a.dtype}")
    if a.ndim != 2 or a.shape[1] != width:
        raise ValueError(f"{what}: shape [n, {width}], not {list(a.shape)}")
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError(f"{what}: must be C-contiguous")
    return a


def _int(x, what: str) -> int:
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
        raise TypeError(f"{what}: an integer, not {type(x).__name__}")
    return int(x)


_libs = {}


def load_side_library(path: str, name: str, signatures: dict, what: str):
    """dlopen the library ``name`` at ``path`` and declare the prototypes.  Raises RuntimeError if it is missing: there is no other implementation to fall back to
    (``what``: the clause that says so)."""
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError(f"{name} not found at {path}: build it with `python -m memvul_amd.build` (hipcc --offload-arch=gfx950); {what}")
    try:
        lib = C.CDLL(path, mode=C.RTLD_LOCAL)
    except OSError as e:  # pragma: no cover
        raise RuntimeError(f"cannot load {path}: {e}") from e
    for sym, (res, args) in signatures.items():
        fn = getattr(lib, sym)  # AttributeError if the .so does not export a declared symbol
        fn.restype, fn.argtypes = res, args
    _libs[path] = lib
    return lib


class KeptIndex:
    """One index <-> one GPU <-> one stream; one thread uses it at a time.  ``matcher_weight``: ``_projector.weight`` of the state dict, fp32 [2, 3 * proj_dim].

    A subclass names its library by class attributes: PREFIX (of the entry points, looked up on ``self._lib`` by name), MAX_VECTORS and VECTORS (how a refusal
    calls them), MAX_ROWS, and ``_load`` (its module's load_library)."""

    PREFIX = ""
    VECTORS = "vectors"
    MAX_VECTORS = 4096
    MAX_ROWS = 2 ** 31 - 2
    _load = None

    def __init__(self, device: int, proj_dim: int, matcher_weight, same_idx: int, lib=None):
        self._h = None
        device, proj_dim, same_idx = _int(device, "device"), _int(proj_dim, "proj_dim"), _int(same_idx, "same_idx")
        if proj_dim not in (512, 768):
            raise ValueError(f"proj_dim = {proj_dim}: the matcher runs on 512 or 768 features")
        if same_idx not in (0, 1):
            raise ValueError(f"same_idx = {same_idx}: 0 or 1")
        if device < 0:
            raise ValueError(f"device = {device}")
        w = np.asarray(matcher_weight)
        if w.dtype != np.float32 or w.shape != (2, 3 * proj_dim):
            raise ValueError(f"matcher_weight: float32 [2, {3 * proj_dim}], not {w.dtype} {list(w.shape)}")
        w = np.ascontiguousarray(w)
        self._lib = lib if lib is not None else type(self)._load()
        self.P, self.same_idx, self.device = proj_dim, same_idx, device
        self._dropped()
        h = C.c_void_p()
        rc = self._fn("create")(device, proj_dim, _ptr(w), same_idx, C.byref(h))
        if rc != 0:
            msg = self._fn("last_error")(None)
            raise RuntimeError(f"{self.PREFIX}create failed ({rc}): {msg.decode() if msg else ''}")
        self._h = h

    # -- plumbing
    def _fn(self, name: str):
        return getattr(self._lib, self.PREFIX + name)

    def _call(self, name: str, *args):
        """The entry point PREFIX + name on the open handle; a non-zero return raises with the library's message."""
        self._check(self._fn(name)(self._handle(), *args), self.PREFIX + name)

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self._fn("last_error")(self._h)
            raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def _handle(self):
        if self._h is None:
            raise RuntimeError(f"the {type(self).__name__} is closed")
        return self._h

    def _dropped(self):
        """What a subclass forgets whenever the rows, their classes or the plan change (the library drops its held state on the same calls)."""

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
        self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    # -- the rows
    def add(self, embed: np.ndarray):
        """Append rows: float32 [n, proj_dim], C-contiguous.  Rows are numbered in order of arrival (where rows have a class, it is 0 until set_classes says
        otherwise)."""
        self._handle()
        embed = _check_array(embed, "embed", self.P)
        if len(self) + embed.shape[0] > self.MAX_ROWS:
            raise ValueError("the index would hold more than 2^31 - 2 rows")
        self._dropped()
        self._call("add", _ptr(embed), embed.shape[0])

    def reset(self):
        """Forget the rows (and their classes), keep the weights."""
        self._dropped()
        self._call("reset")

    def __len__(self) -> int:
        return int(self._fn("count")(self._handle()))

    def _range(self, first, count):
        n = len(self)
        first = _int(first, "first")
        count = n - first if count is None else _int(count, "count")
        if first < 0 or count < 0 or first + count > n:
            raise ValueError(f"rows [{first}, {first} + {count}) are not within the {n} rows of the index")
        return first, count

    def _vectors(self, vectors) -> np.ndarray:
        vectors = _check_array(vectors, "vectors", self.P)
        if not 1 <= vectors.shape[0] <= self.MAX_VECTORS:
            raise ValueError(f"{vectors.shape[0]} {self.VECTORS}: 1 <= Q <= {self.MAX_VECTORS}")
        return vectors

    def kernel_ms(self) -> float:
        """HIP-event time of the last call's launches, in milliseconds."""
        ms = C.c_float()
        self._call("kernel_ms", C.byref(ms))
        return float(ms.value)

    @classmethod
    def _from_sweep(cls, engine, matcher_weight, same_idx, chunk, index_factory, classes):
        chunk = _int(chunk, "chunk")
        if chunk < 1:
            raise ValueError(f"chunk = {chunk}")
        embed = engine.sweep_embeddings(0, None, chunk)  # (raises unless the last sweep kept its embeddings; host memory: the whole corpus once, n * P * 4 bytes)
        index = (index_factory or cls)(engine.device, engine.P, matcher_weight, same_idx)
        try:
            for s0 in range(0, embed.shape[0], chunk):
                index.add(np.ascontiguousarray(embed[s0:s0 + chunk], dtype=np.float32))
            if classes is not None:
                index.set_classes(np.ascontiguousarray(classes, dtype=np.uint8))
        except Exception:
            index.close()
            raise
        return index

    @classmethod
    def from_sweep(cls, engine, matcher_weight, same_idx: int, chunk: int = 65536, index_factory=None):
        """An index over the kept embeddings of the engine's last ``bucketed_sweep(..., keep=True)``, in the ORIGINAL row order, downloaded ``chunk`` rows at a time
        (one download and one upload per kept sweep: the engine's ABI has no entry that hands its resident embeddings over on the device; a further device copy of
        the embeddings, 2 KB per row at 512 features)."""
        return cls._from_sweep(engine, matcher_weight, same_idx, chunk, index_factory, None)


class ClassedKeptIndex(KeptIndex):
    """A KeptIndex whose rows carry a class (0 or 1)."""

    def set_classes(self, cls, first: int = 0):
        """The class (0 or 1; bool or uint8, one per row) of rows [first, first + len(cls))."""
        self._handle()
        if not isinstance(cls, np.ndarray):
            raise TypeError(f"cls: a numpy array, not {type(cls).__name__}")
        if cls.dtype not in (np.dtype(np.uint8), np.dtype(bool)):
            raise TypeError(f"cls: uint8 or bool, not {cls.dtype}")
        if cls.ndim != 1 or not cls.flags["C_CONTIGUOUS"]:
            raise ValueError(f"cls: one C-contiguous dimension, not shape {list(cls.shape)}")
        first = _int(first, "first")
        if first < 0 or first + cls.shape[0] > len(self):
            raise ValueError(f"rows [{first}, {first} + {cls.shape[0]}) are not within the {len(self)} rows of the index")
        cls = cls.view(np.uint8)
        if cls.size and int(cls.max()) > 1:
            raise ValueError("cls: a class is 0 or 1")
        self._dropped()
        self._call("set_classes", _ptr(cls), first, cls.shape[0])

    @classmethod
    def from_sweep(cls, engine, matcher_weight, same_idx: int, chunk: int = 65536, index_factory=None, classes=None):
        """KeptIndex.from_sweep; classes: one class per row."""
        return cls._from_sweep(engine, matcher_weight, same_idx, chunk, index_factory, classes)
