"""What the tests of the tools over a kept corpus share (retrieve / claims / bank, and for rank the checks of the shared headers; CPU and GPU files alike; nothing
here needs a GPU at import): the recording stub library, the numpy stand-in indexes, the oracle-backed keeping engines and the model on them, the checks of the two shared headers, and the GPU files' names."""
import ctypes as C
import json
import os
import re
import shutil

import numpy as np
import pytest

from memvul_amd import build, claims, kept_sweep, model_memory

import bank_kit
import claims_kit
import plumbing_util as pu
import report_index_kit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "memvul_amd", "csrc")
W512 = np.zeros((2, 3 * 512), np.float32)


# ---- the two headers the four kept-corpus libraries share (csrc/kept_index.h, csrc/kept_terms.h) ------------------------------------------------------------------

KEPT_SHARED = ("kept_index.h", "kept_terms.h")
KEPT_OWN = {"retrieve": ("retrieve.hip", "report_topk.h"), "claims": ("claims.hip", "claim_sweep.h"), "bank": ("bank.hip", "bank_cover.h"),
            "rank": ("rank.hip", "rank_sort.h")}  # (source, kernel header)


def opened_by_fingerprint(monkeypatch, sources=None, headers=None) -> set:
    """The files build.source_fingerprint opens for a library (default: libmemvul_hip.so, either build)."""
    opened = []
    real_open = open

    def spy(path, *a, **kw):
        opened.append(os.path.abspath(path) if isinstance(path, str) else path)
        return real_open(path, *a, **kw)

    monkeypatch.setattr("builtins.open", spy)
    build.source_fingerprint((), sources, headers)
    monkeypatch.undo()
    assert opened
    return set(opened)


def own_and_shared(key: str):
    """The files of a kept-corpus library as build.py lists them: (its own, the two it shares), as paths."""
    _, sources, headers = build.SIDE_LIBS[key]
    files = [os.path.join(CSRC, s) for s in sources] + [h if os.path.isabs(h) else os.path.join(CSRC, h) for h in headers]
    shared = [p for p in files if os.path.basename(p) in KEPT_SHARED]
    assert sorted(os.path.basename(p) for p in shared) == sorted(KEPT_SHARED), key
    return [p for p in files if p not in shared], shared


def check_the_shared_headers_belong_to_the_four_kept_libraries(monkeypatch):
    """Opened by exactly the four kept-corpus libraries' fingerprints — never by libmemvul_hip.so's or the tokeniser library's, whose stamps bench.py keys on — and
    included by no file under csrc/ outside those libraries' own sources."""
    shared = {os.path.join(CSRC, h) for h in KEPT_SHARED}
    assert sorted(k for k, (_, _, headers) in build.SIDE_LIBS.items() if set(KEPT_SHARED) & set(headers)) == sorted(KEPT_OWN)
    for key in KEPT_OWN:
        assert shared <= opened_by_fingerprint(monkeypatch, *build.SIDE_LIBS[key][1:]), key
    assert not shared & opened_by_fingerprint(monkeypatch)
    assert not shared & opened_by_fingerprint(monkeypatch, build.TOK_SOURCES, build.TOK_HEADERS)
    assert not set(KEPT_SHARED) & set(build.HEADERS + build.KERNEL_HEADERS + build.TOK_HEADERS + build.SOURCES + build.TOK_SOURCES)
    theirs = {f for pair in KEPT_OWN.values() for f in pair} | set(KEPT_SHARED)
    includes = {}
    for name in os.listdir(CSRC):
        text = open(os.path.join(CSRC, name)).read()
        includes[name] = re.findall(r'#include\s+"([^"]+)"', text)
        if name not in theirs:
            assert not any(h in text for h in KEPT_SHARED), name
    for source, header in KEPT_OWN.values():  # the host side goes into the .hip file, the device side into its kernel header, and neither shared header includes anything of this tree
        assert "kept_index.h" in includes[source] and "kept_terms.h" not in includes[source], source
        assert "kept_terms.h" in includes[header] and "kept_index.h" not in includes[header], header
    assert includes["kept_index.h"] == [] and includes["kept_terms.h"] == []


PLUMBING = ("on_exception", "fail", "hipchk", "launched", "need", "grow", "reserve_rows", "struct Refusal", "struct StateError", "g_err")


def _definitions(text: str, name: str) -> int:
    """How often ``text`` DEFINES ``name`` (a use does not count): a struct with a base or a body, a variable declared with its type, or a function — a return type,
    the name and a parameter list at the start of a line, closed by the brace of its body."""
    text = re.sub(r"//[^\n]*", "", text)
    if name.startswith("struct "):
        return len(re.findall(rf"\b{name}\b\s*[:{{]", text))
    if name == "g_err":
        return len(re.findall(r"^[ \t]*(?:static\s+|thread_local\s+)*std::string\s+g_err\b", text, flags=re.M))
    return len(re.findall(rf"^[ \t]*(?:template\s*<[^>]*>\s*)?(?:static\s+|inline\s+)*[A-Za-z_][\w:<>]*[\s*&]+{name}\s*\([^;{{}}]*\)\s*(?:noexcept\s*)?\{{", text, flags=re.M))


def check_the_index_plumbing_is_defined_once():
    """The error plumbing of the C boundary and the rows' growth are defined by kept_index.h, each exactly once, and by none of the four libraries' sources."""
    shared = open(os.path.join(CSRC, "kept_index.h")).read()
    for name in PLUMBING:
        assert _definitions(shared, name) == 1, name
        for source, _ in KEPT_OWN.values():
            assert _definitions(open(os.path.join(CSRC, source)).read(), name) == 0, (source, name)
    restated = ("thread_local std::string g_err;\nstruct Refusal : std::runtime_error {\n};\nstruct StateError : std::runtime_error {\n};\n"
                "int fail(mvk_index* h, int code, const std::string& msg) {\n  return code;\n}\nint on_exception(mvk_index* h) noexcept {\n  return fail(h, 1, g_err);\n}\n"
                "void hipchk(hipError_t e, const char* what) {\n}\nvoid launched(const char* what) { hipchk(hipGetLastError(), what); }\nvoid need(bool ok, const std::string& msg) {\n}\n"
                "template <typename T>\nvoid grow(T*& p, size_t& have, size_t want) {  // (contents are not kept)\n}\nstatic void reserve_rows(mvk_index* h, int64_t want) {\n  need(true, g_err);\n}\n")
    assert [_definitions(restated, name) for name in PLUMBING] == [1] * len(PLUMBING)  # (a library that restated them would be seen)


def check_kernels_are_the_recorded_ones(lib_path: str, flag: str):
    """build.kernel_fingerprints of a side library against the map recorded under profiles/: a refactor of the shared headers must leave every kernel's bytes alone."""
    recorded = os.path.join(ROOT, "profiles", f"kernel_fingerprints_{flag}.json")
    with open(recorded) as f:
        want = json.load(f)
    got = build.kernel_fingerprints(lib_path)
    changed = sorted(set(want) ^ set(got)) + sorted(k for k in set(want) & set(got) if want[k] != got[k])
    assert not changed, (f"{len(changed)} symbols of {os.path.basename(lib_path)} differ from {recorded}: {changed[:4]}; if the kernels were meant to change, re-record with "
                         f"`python scripts/kernel_fingerprints.py --{flag} --out profiles/kernel_fingerprints_{flag}.json`")


# ---- the recording stub library ------------------------------------------------------------------------------------------------------------------------------------

class StubLib:
    """Records every call; holds `n` rows.  The entries every kept-corpus library has, looked up under PREFIX; a subclass names its PREFIX and adds its own."""
    PREFIX = ""

    def __init__(self):
        self.log, self.n, self.th = [], 0, None

    def __getattr__(self, name):  # (only for what is not found otherwise: mvX_add -> add)
        if not self.PREFIX or not name.startswith(self.PREFIX):
            raise AttributeError(name)
        return getattr(self, name[len(self.PREFIX):])

    def _thresholds(self, th, n):
        self.th = np.ctypeslib.as_array(C.cast(th, C.POINTER(C.c_float)), (n,)).copy()

    def create(self, device, P, w, same_idx, out):
        self.log.append(("create", device, P, same_idx))
        C.cast(out, C.POINTER(C.c_void_p))[0] = 1
        return 0

    def destroy(self, h):
        self.log.append(("destroy",))

    def last_error(self, h):
        return b"stub"

    def add(self, h, e, n):
        self.log.append(("add", n))
        self.n += n
        return 0

    def reset(self, h):
        self.log.append(("reset",))
        self.n = 0
        return 0

    def count(self, h):
        return self.n

    def set_classes(self, h, c, first, n):
        self.log.append(("classes", first, n))
        return 0

    def kernel_ms(self, h, ms):
        return -1

    def test_plan(self, h, *plan):
        self.log.append(("plan",) + plan)
        return 0


# ---- the numpy stand-in indexes (index_factory of the CPU tests) -------------------------------------------------------------------------------------------------------

class _NumpyKept:
    """The rows, their classes and the oracle's P(same); every instance is listed in its class's ``made``."""

    def __init__(self, device, P, w, same_idx):
        self.w, self.same_idx, self.u, self.cls, self.closed = np.asarray(w), same_idx, np.zeros((0, P), np.float32), np.zeros(0, np.uint8), False
        type(self).made.append(self)

    def add(self, e):
        self.u = np.concatenate([self.u, e])
        self.cls = np.concatenate([self.cls, np.zeros(len(e), np.uint8)])

    def set_classes(self, cls, first=0):
        assert cls.dtype == np.uint8
        self.cls[first:first + len(cls)] = cls

    def _p(self, v):
        from oracle import memvul_oracle as orc

        _, p, _, _ = orc.match(self.u, np.asarray(v, np.float32), self.w, self.same_idx)
        return p[:, :, self.same_idx].astype(np.float32)

    def close(self):
        self.closed = True


class _NumpyIndex(_NumpyKept):
    """Ranks P(same) with reference_topk."""
    made = []
    queries = 0

    def query(self, v, k, first=0, count=None):
        self.queries += 1
        return report_index_kit.reference_topk(self._p(v), k)


class _NumpyClaims(_NumpyKept):
    """P(same) met with the rule of claims_kit."""
    made = []

    def counts(self, v, thresholds, first=0, count=None):
        return claims_kit.reference_counts(self._p(v), self.cls, claims.up32(thresholds))

    def select(self, v, thres, first=0, count=None, order="prob"):
        off, rows, p = claims_kit.reference_select(self._p(v), claims.up32(np.broadcast_to(thres, (len(v),))))
        return (off,) + (tuple(claims_kit.by_prob(off, rows, p)) if order == "prob" else (rows, p))


class _NumpyBank(_NumpyKept):
    """P(same) met with the definitions of bank_kit."""
    made = []
    B, marks = None, 0

    def mark(self, v, thres, first=0, count=None):
        self.B = bank_kit.marking(self._p(v), claims.up32(np.broadcast_to(thres, (len(v),))))
        self.marks += 1

    def totals(self):
        return bank_kit.totals(self.B, self.cls)

    def multiplicity(self, per_row=False):
        out = bank_kit.multiplicity(self.B, self.cls)
        return out if per_row else out[:2]

    def overlap(self):
        return bank_kit.overlap(self.B, self.cls)

    def greedy(self, w_pos=1, w_neg=1, fixed=None, max_rounds=None):
        return bank_kit.greedy(self.B, self.cls, w_pos, w_neg, fixed, max_rounds)[:2]


# ---- the engines and the model on them -----------------------------------------------------------------------------------------------------------------------------------

class _KeepingEngine(pu.OracleEngine):
    """The oracle-backed stand-in plus what a keeping sweep needs."""
    created = []

    def __init__(self, device=0, **kw):
        super().__init__(device, **kw)
        self.device, self.kept = device, None
        _KeepingEngine.created.append(self)

    def bucketed_sweep(self, ids, lens, batch, with_probs=False, keep=False, topk=0):
        self.kept = self.encode(ids, lens) if keep else None
        return super().bucketed_sweep(ids, lens, batch, with_probs)

    def sweep_embeddings(self, first=0, count=None, chunk=65536):
        if self.kept is None:
            raise RuntimeError("sweep_embeddings: the resident corpus keeps no embeddings — sweep it with bucketed_sweep(..., keep=True) first")
        return self.kept[first:None if count is None else first + count]


class _CountingEngine(_KeepingEngine):
    """The keeping stand-in, counting the downloads of the kept embeddings."""
    downloads = 0

    def sweep_embeddings(self, first=0, count=None, chunk=65536):
        out = super().sweep_embeddings(first, count, chunk)
        _CountingEngine.downloads += 1
        return out


@pytest.fixture()
def standin_model(monkeypatch):
    """(model, arrays, fixture): a ModelMemory of a small archive on a _CountingEngine, its bank filled from the golden file; the stand-ins' records start empty."""
    from memvul_amd.archive import load_archive

    fx = pu.make_fixture(n_irs=23, n_anchors=4, layers=2)
    root, arch, golden, test_path, w, dims = fx
    monkeypatch.setattr(model_memory, "Engine", _CountingEngine)
    archive = load_archive(arch, cuda_device=0, overrides=pu.TEST_CONFIG, engine_options=dict(max_tokens=16 * 256, max_batch=16, max_anchors=16))
    model = archive.model
    model.eval()
    model._golden_instances_embeddings = None
    model._golden_instances_labels = None
    model.forward_on_instances(list(archive.validation_dataset_reader.read(golden)))
    arrays = archive.dataset_reader.read_arrays(test_path)
    _NumpyIndex.made, _NumpyClaims.made, _NumpyBank.made, _CountingEngine.downloads = [], [], [], 0
    yield model, arrays, fx
    shutil.rmtree(root, ignore_errors=True)


def _inputs(arch, golden, test_path):
    """(ids, lens, the reader's arrays) of the command line's inputs."""
    from memvul_amd import archive, audit

    _, config, _ = audit._read_archive(arch)
    ids, lens, _, _ = audit._read_inputs(config, golden, test_path)
    reader = archive._build_reader(config.get("validation_dataset_reader")) or archive._build_reader(config.get("dataset_reader"))
    return np.asarray(ids), np.asarray(lens), reader.read_arrays(test_path)


# ---- what the GPU files share --------------------------------------------------------------------------------------------------------------------------------------------

L2 = dict(layers=2, vocab_size=2048)
WK = dict(qk_scale=4.0, match_scale=6.0)
WK768 = dict(qk_scale=4.0, match_scale=6.0, use_header=False)


class _Vocab:
    def get_token_index(self, token, namespace=None):
        return {"same": 0, "diff": 1}[token]


def _engine_matrix(eng, U, V):
    """probs [N, G, 2] of the engine's matcher for every (row of U, row of V)."""
    eng.anchor_set(V)
    mb = eng.cfg.max_batch
    return np.concatenate([eng.match(np.ascontiguousarray(U[s0:s0 + mb]))["probs"] for s0 in range(0, len(U), mb)])


def _same_bytes(got, want, what):
    """Byte equality, with the figures printed first."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        bits = np.dtype("i4") if got.dtype == np.float32 else got.dtype
        diff = got.view(bits) != want.view(bits)
        ulp = np.abs(got.view(bits).astype(np.int64) - want.view(bits).astype(np.int64))
        print(f"{what}: {int(diff.sum())} of {diff.size} values differ; largest bit-pattern distance {int(ulp.max())}; first at {np.argwhere(diff)[0].tolist()}")
    assert got.tobytes() == want.tobytes(), what


def bare_model(eng, matcher_weight, n_labels: int):
    """A ModelMemory around a live engine, without an archive: the engine, the matcher weight and the labels CWE-0 .. are all it knows; its metrics go nowhere."""
    m = model_memory.ModelMemory.__new__(model_memory.ModelMemory)
    m.__dict__.update(_engine=eng, vocab=_Vocab(), _label_namespace="labels", _same_idx=0, _kept=kept_sweep.KeptSweepState(matcher_weight),
                      _golden_labels=[f"CWE-{i}" for i in range(n_labels)], _counts=lambda best, lab: None,
                      _siamese_metric=type("M", (), {"add_arrays": lambda self, a, b: None})())
    return m
