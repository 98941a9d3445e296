// libmemvul_hip.so — C ABI (include/memvul_hip.h) over the gfx950 kernels in this directory.
// Host side: weight staging/packing, workspace ownership, launch sequencing on one HIP stream,
// HIP-event profiling per kernel class, error translation.  No torch, no exceptions across the ABI.
// One translation unit, cut into parts by subsystem: this file holds the state — the structs a handle is made of and mv_handle itself — includes each
// part once, and ends with read_switches, mv_create / mv_destroy, the anchor / encode / forward / match entries, the accessors and the debug and test hooks.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>  // types and prototypes only: librccl.so is opened at run time (mv_comm_init), never linked
#include <unistd.h>

#include <algorithm>
#include <charconv>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/memvul_hip.h"
#include "common.h"
#include "gemm.h"
#include "gemm_pp.h"
#include "gemm_pp_fixed.h"
#include "attention.h"
#include "attention_v2.h"
#include "misc_kernels.h"
#include "match_topk.h"
#include "ref_f32.h"
#include "sink_census.h"
#include "route.h"
#include "wordpiece.h"

namespace {

enum KernelClass {
  KC_EMBED_LN = 0, KC_GEMM_QKV, KC_ATTENTION, KC_GEMM_OUT, KC_LN, KC_GEMM_FFN1, KC_GEMM_FFN2,
  KC_POOL_HEAD, KC_MATCH, KC_TOPK, KC_TEST_GEMM, KC_CLS_ROW_TERM, KC_GEMM_KV_LAST, KC_CLS_TAIL
};
const char* kKernelClassNames[MV_NUM_KERNEL_CLASSES] = {
    "embed_ln", "gemm_qkv", "attention", "gemm_attn_out", "layernorm", "gemm_ffn1_gelu", "gemm_ffn2",
    "pool_head", "match", "topk", "test_gemm", "cls_row_term", "gemm_kv_last", "cls_tail"};

thread_local std::string g_create_error;

struct HostTensor {
  std::vector<float> data;
  std::vector<int64_t> shape;
};

struct LayerW {
  half_t *wqkv = nullptr, *wo = nullptr, *w1 = nullptr, *w2 = nullptr;
  float *bqkv = nullptr, *bo = nullptr, *b1 = nullptr, *b2 = nullptr;
  // virtual LayerNorm (gemm_pp.h): the preceding LayerNorm folded in: W'' = rowcentre(W gamma), b' = b + W beta
  half_t *wqkv_f = nullptr, *w1_f = nullptr;
  float *bqkv_f = nullptr, *b1_f = nullptr;
  // MV_F16X8 (gemm_pp.h): fp8 planes [hi8 | lo8] of the four GEMM weights the persistent path uses, rows of 2 K bytes, and the
  // E8M0 scale word of each GEMM's correction sweep (2^-(11 + MV_X8_ACT_SHIFT + the matrix' own shift))
  uint8_t *wqkv_f8 = nullptr, *wo8 = nullptr, *w1_f8 = nullptr, *w28 = nullptr;
  int sc_qkv = 0, sc_o = 0, sc_1 = 0, sc_2 = 0;
  // MV_F16X8, last layer only: fp32 transposed ([k][n]) weights of the [CLS] tail (misc_kernels.h dense768_kernel)
  float *wqT32 = nullptr, *woT32 = nullptr, *w1T32 = nullptr, *w2T32 = nullptr;
  // MV_F32 (ref_f32.h): the four GEMM weights as loaded, [n][k] fp32, no LayerNorm folded in (packed QKV with the 1/8 on the Q block: exact)
  float *wqkv32 = nullptr, *wo32 = nullptr, *w132 = nullptr, *w232 = nullptr;
  float *ln1g = nullptr, *ln1b = nullptr, *ln2g = nullptr, *ln2b = nullptr;
};

struct ProfRec {
  int cls;
  hipEvent_t e0, e1;
};

}  // namespace

// The host side of one batch, rows in plan order (Plan): the ids of every pass at the pass's own width, back to back, the lengths, and the results
// (NULL: an output not asked for)
struct Stage {
  int32_t *ids = nullptr, *lens = nullptr, *idx = nullptr;
  float *logits = nullptr, *probs = nullptr, *best = nullptr, *embed = nullptr;
  uint32_t* over = nullptr;  // the guarded form: per row, the monitor items over MV_SINK_COLLISION (AttnArgs::seq_over)
};

// Which results a staging holds, and a view of one without the others
struct Want {
  bool logits = false, probs = false, best = false, idx = false, embed = false, over = false;
};
inline Want wanted(const Stage& o, bool embed) { return {o.logits != nullptr, o.probs != nullptr, o.best != nullptr, o.idx != nullptr, embed, false}; }
inline Stage only(Stage s, const Want& w) {
  if (!w.logits) s.logits = nullptr;
  if (!w.probs) s.probs = nullptr;
  if (!w.best) s.best = nullptr;
  if (!w.idx) s.idx = nullptr;
  if (!w.embed) s.embed = nullptr;
  if (!w.over) s.over = nullptr;
  return s;
}

// Pageable host staging of the synchronous entry points
struct HostStage {
  std::vector<int32_t> ids, lens, idx;
  std::vector<float> logits, probs, best, embed;
  std::vector<uint32_t> over;
  // sized for `rows` rows of `tokens` ids in all against G anchors (ids and lengths always, of the results those wanted): the view of it
  Stage view(size_t rows, size_t tokens, size_t G, size_t P, const Want& w) {
    ids.resize(tokens);
    lens.resize(rows);
    if (w.logits) logits.resize(rows * G * 2);
    if (w.probs) probs.resize(rows * G * 2);
    if (w.best) best.resize(rows * 2);
    if (w.idx) idx.resize(rows);
    if (w.embed) embed.resize(rows * P);
    if (w.over) over.resize(rows);
    return only(Stage{ids.data(), lens.data(), idx.data(), logits.data(), probs.data(), best.data(), embed.data(), over.data()}, w);
  }
};

// How a batch runs: its row order (plan row i = caller row order[i]; empty = the identity) and its passes, each rows [first, first + rows) of that order
// at `width` tokens per row, its ids at token `tok` of the staging
struct Pass {
  int first, rows, width, min_len;  // min_len: the shortest row of the pass (encode_dev)
  int64_t tok;
};
struct Plan {
  std::vector<int> order;
  std::vector<Pass> passes;
  int64_t tokens = 0;  // ids of every pass
};

// What run_passes does with a planned batch besides encoding it, and where the results go
struct Job {
  const int32_t *ids = nullptr, *lens = nullptr;  // host, plan order: the ids of every pass at its own width, back to back (Pass::tok); NULL: the resident corpus
  int64_t c_row = 0; bool keep_psame = false;    // ... whose row c_row is plan row 0: ids read in place at pitch Corpus::S, results (and P(same)) to its arrays
  Stage out;                                      // host results, plan order (NULL: not asked for; out.ids / out.lens unused)
  bool match = false;                             // + the matcher: the best anchor always, logits / probs where `out` asks for them
  float* u_dev = nullptr;                         // the encoder's output to the device here (mv_anchor_append: the bank; a keeping sweep: Corpus::embed) instead of wk.u
  int topk = 0;                                   // the resident corpus, mv_corpus_keep: the rows' k best anchors to Corpus::topk_p / topk_idx as well (0: none)
  int n_layers = -1; bool full = false;           // mv_debug_encode: the layers to run, and the full last layer (encode_dev)
  int G = 0;                                      // the anchors it is matched against: the bank's first G rows (job_form: the count when the job is made)
  bool safe = false;                              // the form of its passes (job_form: from the handle, when the job is made)
  bool guard = false;                             // the guarded form: default-form passes with the per-sequence monitor counts kept (out.over / Corpus::over)
  bool monitor = true;                            // false: a rescoring job (PassForm::monitor)
  const uint8_t* routed = nullptr;                // the guarded form, plan order: rows the sink-token list routed — they ran in no pass yet, rescore_rows encodes them
};

// Activation buffers of ONE in-flight batch and the stream its kernels run on, and what is in flight there
struct Work {
  hipStream_t stream = nullptr;
  int32_t *d_ids = nullptr, *d_lens = nullptr;  // host-path inputs
  uint32_t* seq_over = nullptr;                 // the guarded form: AttnArgs::seq_over of the passes of a host batch [max_batch]
  int32_t* d_idx = nullptr;                     // ... and the corpus rows of one rescoring pass of the resident sweep [max_batch] (corpus_gather_kernel)
  float* xres = nullptr;                        // residual stream fp32 [T][768]
  half_t *x16 = nullptr, *q = nullptr, *k = nullptr, *vt = nullptr, *ctx = nullptr, *h16 = nullptr;
  half_t *vt_lo = nullptr, *q_lo = nullptr, *k_lo = nullptr;  // MV_F16X8, passes of padded length <= 128 (the safe form: every pass): second fp16 planes of V^T, Q, K (attention_v2.h VLO)
  float *u = nullptr, *pooled = nullptr;
  float *logits = nullptr, *probs = nullptr, *psame = nullptr, *best = nullptr;
  int32_t* best_idx = nullptr;
  float* topk_p = nullptr;
  int32_t* topk_idx = nullptr;
  float *part_p = nullptr, *part_q = nullptr;   // per-chunk top-k candidates of the fused matcher (G > 256)
  int32_t* part_i = nullptr;
  float* u_in = nullptr;                        // host-provided embeddings for mv_match / mv_topk
  float *c32 = nullptr, *cq = nullptr;          // [CLS]-row buffers of the pruned last layer
  float* ch32 = nullptr;                        // MV_F16X8: the fp32 [CLS] tail's FFN intermediate [Bp][3072]
  half_t *c16 = nullptr, *cctx = nullptr, *ch16 = nullptr;
  float *lnstats = nullptr, *lnpart = nullptr;  // the two vstats buffers [T][3][2] of the virtual LayerNorm (layer input / mid-layer;
                                                // each residual GEMM reads one, writes the other)
  half_t* xlo = nullptr;                        // MV_F16: lo plane of the two-plane raw stream (PP_RESLN3), allocated by mv_finalize_weights.  MV_F16X8 has none: the stream's low part is the lo8 plane of x8 (+ st_lo)
  uint8_t *x8 = nullptr, *ctx8 = nullptr, *h8 = nullptr;  // MV_F16X8: [lo8 | hi8] planes of the raw stream [T][1536], the attention
                                                          // context [T][1536] and the GELU output [T][6144]
  half_t* cls_lo = nullptr;   // MV_F16X8, special rows (rows 0, 1 of every sequence: its [CLS] and [SEP] token): 2^11 x the low parts of those rows of the NEXT GEMM's A operand,
                              // compact [2 Bp][3072] fp16, written by the producing kernel's epilogue (GemmArgs::sp_lo_out / AttnArgs::sp_lo_out / embed_ln_kernel)
  half_t* st_lo = nullptr;    // ... 2^11 x the low parts of those rows of the RAW STREAM [2 Bp][768]: the A operand of the QKV / FFN-1 row terms, and — in the [CLS]-row form,
                              // with the stream of every other row being hi + the lo8 plane of its fp8 planes (gemm.h GemmArgs::out16b) — what the residual GEMMs read back
  float* cls_corr = nullptr;  // ... and 2^11 x their A-side correction term A_lo W_hi^T [2 Bp][3072] (GemmArgs::cls_corr)
  half_t* vlo_sp = nullptr;   // 2^11 x the low parts of V of the special rows [B 12][64][2] (GemmArgs::vlo_sp -> AttnArgs::vlo_sp)
  float *qkv32 = nullptr, *ctx32 = nullptr, *h32 = nullptr;  // MV_F32: Q | K | V [T][2304], attention context [T][768], GELU output [T][3072], allocated by mv_finalize_weights
  int32_t* tile_both = nullptr;  // cls_aside: per 256-row tile of the pass, non-zero = its sequence is shorter than cls_min_len (GemmArgs::tile_both)
  // in flight on this stream: batches of a resident sweep (check_ready waits for them) and / or a ticket of mv_forward_ragged_begin — its plan and the job it
  // was begun with (form, anchor count, and as ids / out the view of `pin` it is staged in: PINNED, allocated at the set's first ticket)
  bool sweep = false, ticket = false;
  Plan plan;
  Job job;
  std::vector<uint8_t> routed;  // the rows of the plan that the sink-token list of that moment routed (job.routed points here)
  Stage pin;
};

// The resident corpus (corpus.h), whole: mv_corpus_upload replaces it by Corpus{} after release_corpus has freed its device arrays.  A new field gets its default
// here and, if it is device memory, its line in release_corpus — nothing else resets it.
struct Corpus {
  int32_t *ids = nullptr, *lens = nullptr;
  std::vector<int32_t> lens_host;  // the lengths as uploaded (encode_dev's min_len of each pass)
  int64_t n = 0;
  int S = 0;
  float* best = nullptr;
  int32_t* idx = nullptr;
  float* psame = nullptr;  // [psame_rows][G], sized at the first run that keeps P(same) against G anchors (ensure_psame)
  int64_t psame_rows = 0;
  int G = 0;
  // what the corpus keeps of a sweep besides the best anchor (mv_corpus_keep: after an upload, before its first run; allocated at that run): the embeddings, so
  // that mv_corpus_rematch can match them again against a changed bank without the encoder, and the k best anchors of every row
  int keep_embed = 0, k = 0;
  bool ran = false;                   // a run since the upload: mv_corpus_keep comes too late
  float* embed = nullptr;             // [n][P]
  float* topk_p = nullptr;            // [n][k]
  int32_t* topk_idx = nullptr;
  std::vector<uint8_t> has;           // [n] a keeping run covered the row (empty while nothing is kept)
  // the guarded form on the resident corpus: the sweep records the per-row monitor counts and which rows it ran at which width; rescore_corpus (mv_corpus_results)
  // encodes the flagged ones again
  uint32_t* over = nullptr;           // [n] AttnArgs::seq_over of the row's last guarded run
  struct Pending {
    int16_t w = 0;                    // the width (s_eff) of the row's guarded run not yet rescored; 0 = none
    uint8_t keep = 0;                 // ... and whether that run kept P(same)
    uint8_t force = 0;                // ... and whether it left the row out: routed
  };
  std::vector<Pending> pend;          // [n]
  std::vector<uint8_t> forms;         // [n] mv_corpus_row_forms
  bool pending = false;
  // ... and the sink-token list there: the flags of every corpus row under the current list (route_flags_kernel), recomputed lazily after an upload or a list
  // change; a guarded sweep leaves the routed rows of its range out and marks them forced (rescore_corpus encodes them without looking at `over`)
  uint8_t* route_dev = nullptr;       // [n]
  std::vector<uint8_t> route;         // [n] on the host
  bool route_stale = true;
  std::vector<std::vector<int32_t>> idx_live;  // index lists of the split batches of sweeps in flight (alive until rescore_corpus has waited for them)
};

// The multi-GPU exchange (comm.h): librccl.so as opened at run time, the communicator, and the device staging of mv_comm_allgather
struct Comm {
  void* lib = nullptr;
  ncclComm_t comm = nullptr;
  int rank = 0, world = 1;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  decltype(&ncclGetVersion) GetVersion = nullptr;      // optional (mv_comm_info)
  decltype(&ncclCommCount) CommCount = nullptr;        // optional
  decltype(&ncclCommUserRank) CommUserRank = nullptr;  // optional
  void *send = nullptr, *recv = nullptr;  // grow to the largest call
  int64_t send_cap = 0, recv_cap = 0;
};

struct mv_handle {
  int device = 0;
  mv_config cfg{};
  std::string err;
  bool finalized = false;
  int compute_dtype = MV_F16;
  bool precise = false;    // MV_F16X8: every persistent GEMM adds the fp8 correction sweep (gemm_pp.h X8)
  bool f32 = false;        // MV_F32: the reference form — every pass through encode_f32_dev (ref_f32.h)
  std::map<std::string, HostTensor> staged;
  std::vector<void*> allocs;

  // weights
  float *wemb = nullptr, *pemb = nullptr, *temb = nullptr, *embg = nullptr, *embb = nullptr;
  std::vector<LayerW> L;
  float *WpT = nullptr, *bp = nullptr, *WhT = nullptr, *bh = nullptr, *Wm = nullptr;
  int P = MV_PROJ;  // width of the embedding the matcher runs on: 512 = header output (use_header, every reference config),
                    // 768 = the pooler output itself (use_header = False, model_memory.py:69-73): mv_config.proj_dim

  // workspaces: two sets, each with its own stream.  mv_corpus_run alternates the batches of a sweep between them,
  // so two batches are in flight on the GPU at once: the persistent kernels of one batch fill the CUs the other
  // batch's kernel tails, small kernels and memory phases leave idle (+5 % issue reports/s, scripts/dual_stream_probe.py).
  // mv_forward_ragged_begin puts its batch on a set without a ticket; every other entry point works on set 0.
  int64_t cap_tokens = 0;  // rows every activation buffer holds (multiple of 128, + slack)
  Work work[2];
  int n_streams = 2;       // sets in use by the resident sweep (mv_set_streams); env MEMVUL_STREAMS=1: only one is created
  int n_alloc = 2;         // sets created
  int rr = 0;              // workspace set of the next resident-sweep batch
  Plan plan;               // the synchronous entry points' plan and by-length staging (they run on set 0, behind whatever ticket is in flight there)
  HostStage stage, stage2;  // stage2 / plan2: the guarded form's rescoring batch (the flagged rows of the batch just run, in plan order)
  Plan plan2;
  // the sink-token list (mv_set_sink_tokens; route.h): acted on in the guarded form only — a sequence that carries a listed token at positions 1 .. len - 2 never
  // runs in the default form, it seeds the rescoring plan directly
  std::vector<int32_t> sink_tokens;     // as given (duplicates kept)
  std::vector<uint32_t> sink_bitmap;    // route_bitmap of it over mv_config.vocab_size
  std::vector<uint8_t> route_flags, routed;  // of the host batch being made: caller's row order / plan order (Job::routed)
  Plan plan1;                           // ... and its plan without the routed rows (split_plan)
  int64_t routed_seqs = 0;              // mv_route_stats
  std::vector<uint8_t> last_forms;             // mv_last_row_forms: the form that produced each row of the last host-buffer call, caller's row order
  int64_t guard_seqs = 0, guard_rescored = 0;  // mv_form_stats
  float* anchors = nullptr;
  int n_anchors = 0;
  unsigned long long* attn_conc = nullptr;  // MV_F16X8: [0] max collision mass of the [CLS] row on ordinary keys (float bits), [1] items above 0.25 (AttnArgs::conc)
  // the sink census (mv_sink_census_enable / mv_sink_census_read; sink_census.h): allocated at the first enable, sized by the loaded vocabulary
  bool census = false;                        // one host-side test per monitored layer of a pass while it is off
  uint32_t* census_items = nullptr;           // [vocab_size]
  unsigned long long* census_share = nullptr; // [vocab_size] sum of round(p* 2^20)
  uint32_t* census_heads = nullptr;           // [layers][12]
  unsigned long long* x8_sat = nullptr;  // MV_F16X8: device counter (64-bit: it cannot wrap within a run) of activation elements beyond the fp8 planes' range (mv_x8_saturation)

  std::vector<void*> pinned;  // the pinned staging of the tickets (Work::pin)
  Corpus corpus;              // the resident corpus (corpus.h)
  uint32_t* route_bm_dev = nullptr;  // the sink-token list's bitmap on the device [ceil(vocab / 32)], for the corpus' route flags: it stays with the list, an upload keeps it

  // last-layer pruning ([CLS] rows only after the last layer's K / V projection) and its compact buffers
  bool cls_prune = true;   // env MEMVUL_CLS_PRUNE=0 disables
  int pp_gn_max = 4;       // raster group width cap of the persistent GEMM (env MEMVUL_GN_MAX: the A/B of profiles/r04_*)
  int pp_raster = 0;       // env MEMVUL_RASTER=1: the A-stationary raster where it applies (FFN-1, QKV at full-size grids)
  bool short_vlo = true;   // MV_F16X8, env MEMVUL_SHORT_VLO=0 disables: passes of padded length <= 128 carry V and P as hi + lo fp16 planes through attention
                           // (attention_v2.h VLO): the fp16 storage of V and P is what is left of the precise mode's error and short sequences average it least
  bool cls_aside = true;   // MV_F16X8, the [CLS]-row form (default; env MEMVUL_CLS_ASIDE=0 = both correction terms in every row, the form of rounds 3-4): passes of
                           // padded length 256 / 512 sweep the weight-side term only in every GEMM (the Q block of the QKV projection keeps both) and add the A-side
                           // term for the [CLS] row of each sequence alone (a skinny fp16 GEMM over those B rows in front of each launch, GemmArgs::cls_corr): the
                           // pooler reads only that row, every other row's A-side rounding reaches it averaged over the keys.  +14 % at the same error (r05_j*, r05_k*)
  int cls_min_len = 128;   // ... for sequences of at least this many tokens (env MEMVUL_CLS_ASIDE_MIN_LEN): a short sequence averages over few keys (model: 1.2 -
                           // 1.6x the error at 16 - 128 tokens), so its row tiles run the both-terms form, bit for bit (GemmArgs::tile_both, cls_tile_flags_kernel)
  int qkv_aside_mask = 0;  // MV_F16X8: which of the Q / K / V blocks of the QKV projection sweep the A-side correction term for EVERY row (bit 0 / 1 / 2;
                           // gemm_pp.h x8_aside_mask).  Default (round 6, second half): none — the special rows get the term from their row term in every block, and an
                           // ordinary row's Q rounding, like its K and V rounding, reaches the pooler only through attention, averaged over the keys (model: q / none / qkv
                           // within 7 % of each other, scripts/r06_qkv_model.py; GPU, 60 draws: +3 % error for +2.7 % issue reports/s, profiles/r06_m_*).  Rounds 4 - 6a: Q ("q").
                           // env MEMVUL_QKV_ASIDE = a subset of "qkv", "" or "none" ("qkv" = round 3's form)

  bool pp_fixed = true;    // MV_F16X8, env MEMVUL_PP_FORM=fixed (default) | runtime: the persistent GEMMs of a long pass in the [CLS]-row form take the fixed-form
                           // kernels of libmemvul_pp_fixed.so (encoder_pass.h pp_fixed_form; gemm_pp_fixed.hip) — the same bits from kernels that spill less;
                           // runtime = every launch on the kernels of this library, as before
  int64_t pp_fixed_launches = 0;  // launches of this handle that took a fixed-form kernel (mvpp_fixed_launches)

  int form = MV_FORM_DEFAULT;  // MV_F16X8, mv_set_form / env MEMVUL_FORM: MV_FORM_SAFE = the form that holds 1e-3 with an attention sink on an ORDINARY token too — both
                           // first-order terms in every row of every GEMM (no [CLS]-row form, no row terms), the A-side term in all three QKV blocks, and Q, K, V, P as
                           // hi + lo fp16 planes through attention at EVERY padded length (attention_v2.h VLO, NCH > 1 above 128) and through the pruned last layer's
                           // single-query attention.  Read on the host when a pass is enqueued (encode_dev); cls_aside / cls_min_len / qkv_aside_mask / short_vlo do
                           // not reach it (it is their most conservative setting by construction).  MV_FORM_GUARDED = the default form, then the safe form again
                           // for the sequences whose own monitor items ask for it (Job::guard, rescore_rows / rescore_corpus)

  // profiling
  uint32_t prof_mask = 0xffffffffu;  // kernel classes that get HIP events while profiling is on
  bool prof = false;
  std::vector<ProfRec> recs;
  std::vector<hipEvent_t> free_events;

  // GEMM path (env MEMVUL_GEMM_TILE): 0 auto (persistent ping-pong kernels when the pass fills the chip, else the
  // one-tile-per-workgroup kernels on an fp32 stream), 128 forces the small path, 512 the persistent one.
  int gemm_tile = 0;
  int num_cu = 256;

  // debug
  int dbg_B = 0, dbg_Sp = 0;
  int dbg_stop = 0;  // development build only (read_switches): mv_debug_encode ends inside its last layer, after this many launch groups (encode_dev); 0 = off
#if defined(MEMVUL_DEV_SWITCHES)
  // development build only, MEMVUL_DEBUG_TAIL=1 (read_switches; encoder_pass.h tail_tap): every launch of the pruned last layer's [CLS] tail on workspace set 0
  // is followed by a device-to-device copy of its B output rows into this arena, for mv_debug_read 22 - 33 (the tail overwrites c32 and pooled in place)
  bool dbg_tail = false;
  uint8_t* tail_arena = nullptr;  // [TT_COUNT slots], slot s at TT_OFF[s] x max_batch bytes (allocated at the first tapped pass)
  int tail_passes = 0;            // pruned passes tapped so far: a batch that ran as ONE pass adds 1 (mv_debug_read 34)
#endif

  Comm comm;  // the multi-GPU exchange (comm.h)
};

// The host code, part by part, each included here once, in dependency order: no part refers to a name a later one defines.  The state structs above stay with
// mv_handle (a member held by value must be complete before it, and every part's functions need the handle complete).
#include "host_base.h"
#include "weights.h"
#include "workspace.h"
#include "encoder_pass.h"
#include "batch_flow.h"
#include "corpus.h"
#include "comm.h"
#include "records_format.h"
#include "tokenizer_object.h"

namespace {

// The environment switches of mv_create (include/memvul_hip.h lists them), read into the handle before anything is created from them.  Every one is parsed
// strictly: a value the library does not understand fails mv_create with a message (g_create_error) — a typo must never silently select other numerics (or
// another stream count) than the one asked for.  h->num_cu holds the device's own count already (MEMVUL_NUM_CU's upper bound).
int read_switches(mv_handle* h) {
  auto env_int = [&](const char* name, int lo, int hi, int* out) -> bool {  // false = present and malformed (g_create_error set)
    const char* e = getenv(name);
    if (!e) return true;
    char* end = nullptr;
    const long v = strtol(e, &end, 10);
    if (end == e || *end != '\0' || v < lo || v > hi) {
      g_create_error = std::string(name) + "=\"" + e + "\": expected an integer in " + std::to_string(lo) + " .. " + std::to_string(hi);
      return false;
    }
    *out = (int)v;
    return true;
  };
  auto env_flag = [&](const char* name, bool* out) -> bool {
    int v = *out ? 1 : 0;
    if (!env_int(name, 0, 1, &v)) return false;
    *out = v != 0;
    return true;
  };
  {
    int ns = h->n_streams;
    if (!env_int("MEMVUL_STREAMS", 1, 2, &ns)) return MV_ERR_INVALID;
    h->n_streams = h->n_alloc = ns;
  }
  if (!env_flag("MEMVUL_CLS_PRUNE", &h->cls_prune)) return MV_ERR_INVALID;
  if (const char* e = getenv("MEMVUL_QKV_ASIDE")) {
    h->qkv_aside_mask = 0;
    if (strcmp(e, "none")) {
      for (const char* c = e; *c; ++c) {
        const int bit = (*c == 'q' || *c == 'Q') ? 1 : (*c == 'k' || *c == 'K') ? 2 : (*c == 'v' || *c == 'V') ? 4 : 0;
        if (!bit) {
          g_create_error = std::string("MEMVUL_QKV_ASIDE=\"") + e + "\": expected a subset of \"qkv\", \"\" or \"none\"";
          return MV_ERR_INVALID;
        }
        h->qkv_aside_mask |= bit;
      }
    }
  }
  if (!env_flag("MEMVUL_CLS_ASIDE", &h->cls_aside)) return MV_ERR_INVALID;
  if (!env_int("MEMVUL_CLS_ASIDE_MIN_LEN", 1, 512, &h->cls_min_len)) return MV_ERR_INVALID;
  if (const char* e = getenv("MEMVUL_FORM")) {  // the form of MV_F16X8 the handle starts in (mv_set_form changes it later); MV_F16 has none: mv_finalize_weights
    if (!strcmp(e, "safe")) h->form = MV_FORM_SAFE;
    else if (!strcmp(e, "default")) h->form = MV_FORM_DEFAULT;
    else if (!strcmp(e, "guarded")) h->form = MV_FORM_GUARDED;
    else {
      g_create_error = std::string("MEMVUL_FORM=\"") + e + "\": expected \"default\", \"safe\" or \"guarded\"";
      return MV_ERR_INVALID;
    }
  }
  if (const char* e = getenv("MEMVUL_PP_FORM")) {  // which kernels the persistent GEMMs of a long pass take (mv_handle::pp_fixed): the bits do not depend on it
    if (!strcmp(e, "fixed")) h->pp_fixed = true;
    else if (!strcmp(e, "runtime")) h->pp_fixed = false;
    else {
      g_create_error = std::string("MEMVUL_PP_FORM=\"") + e + "\": expected \"fixed\" or \"runtime\"";
      return MV_ERR_INVALID;
    }
  }
#ifdef MEMVUL_DEV_SWITCHES
  // Development A/B knobs: compiled only into libmemvul_hip_dev.so (memvul_amd/build.py dev=True; the GPU tests that force a kernel path at test
  // sizes and the A/B scripts load that build) — the product library does not read them.
  //   MEMVUL_GEMM_TILE  0 by pass size / 128 the small-pass kernels / 512 the persistent kernels forced
  //   MEMVUL_SHORT_VLO  0: passes of padded length <= 128 carry Q, K, V, P as ONE fp16 plane through attention (the A/B of attention_v2.h VLO)
  //   MEMVUL_NUM_CU     size the persistent grids for a share of the chip;  MEMVUL_RASTER 1: the A-stationary raster;  MEMVUL_GN_MAX 1 .. 12: raster group width cap
  {
    int gt = h->gemm_tile;
    if (!env_int("MEMVUL_GEMM_TILE", 0, 512, &gt)) return MV_ERR_INVALID;
    if (gt != 0 && gt != 128 && gt != 512) { g_create_error = "MEMVUL_GEMM_TILE: expected 0, 128 or 512"; return MV_ERR_INVALID; }
    h->gemm_tile = gt;
    if (!env_flag("MEMVUL_SHORT_VLO", &h->short_vlo)) return MV_ERR_INVALID;
    if (!env_int("MEMVUL_GN_MAX", 1, 12, &h->pp_gn_max)) return MV_ERR_INVALID;
    if (!env_int("MEMVUL_RASTER", 0, 1, &h->pp_raster)) return MV_ERR_INVALID;
    if (!env_int("MEMVUL_NUM_CU", 1, h->num_cu, &h->num_cu)) return MV_ERR_INVALID;
    //   MEMVUL_DEBUG_STOP 1 .. 5: mv_debug_encode(ids, lens, n) runs n - 1 whole layers, then only the first k launch groups of layer n - 1 (1 the QKV projection with
    //                     its row term, 2 + attention, 3 + the output projection, 4 + FFN-1, 5 + FFN-2) and NO final LayerNorm (nor with n = 0): every workspace buffer
    //                     keeps what the last launch left in it, for mv_debug_read (persistent path, MV_F16 / MV_F16X8).  MV_F32: the same k on its one path
    //                     (encoder_pass.h encode_f32_dev: 3 ends before LayerNorm 1, 4 after LayerNorm 1 and FFN-1, 5 before LayerNorm 2; no pooler)
    if (!env_int("MEMVUL_DEBUG_STOP", 1, 5, &h->dbg_stop)) return MV_ERR_INVALID;
    //   MEMVUL_DEBUG_TAIL 1: a pruned pass on workspace set 0 (mv_encode, mv_forward, ...) copies what each launch of its [CLS] tail wrote — the B real rows — into a
    //                     tap arena, device to device on the pass's own stream, for mv_debug_read 22 - 34 (encoder_pass.h tail_tap).  Copies only: no launch, argument or
    //                     order changes, so the embedding is the product library's bit for bit
    if (!env_flag("MEMVUL_DEBUG_TAIL", &h->dbg_tail)) return MV_ERR_INVALID;
  }
#endif
  return MV_OK;
}

// The mv_test_gemm* hooks: one warm-up / correctness launch, `iters` launches between two events, a synchronise; *ms = the time per launch, the status = the
// first error (the events are destroyed on every path)
template <typename Run>
int timed_launches(mv_handle* h, hipStream_t s0, int iters, float* ms, const char* what, Run run) {
  if (iters < 1) iters = 1;
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  int rc = run();
  if (rc == MV_OK) {
    hipEventRecord(e0, s0);
    for (int i = 0; i < iters && rc == MV_OK; ++i) rc = run();
    hipEventRecord(e1, s0);
  }
  const hipError_t se = hipStreamSynchronize(s0);
  float t = 0.f;
  hipEventElapsedTime(&t, e0, e1);
  hipEventDestroy(e0); hipEventDestroy(e1);
  if (ms) *ms = t / (float)iters;
  if (rc == MV_OK && se != hipSuccess) rc = fail(h, MV_ERR_HIP, std::string(what) + ": " + hipGetErrorString(se));
  return rc;
}

}  // namespace

extern "C" {

const char* mv_last_error(mv_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

const char* mv_kernel_class_name(int cls) {
  return (cls >= 0 && cls < MV_NUM_KERNEL_CLASSES) ? kKernelClassNames[cls] : "";
}

int mv_create(int device, const mv_config* cfg, mv_handle** out) try {
  if (!cfg || !out) return fail(nullptr, MV_ERR_INVALID, "null argument");
  if (cfg->hidden != MV_HIDDEN || cfg->heads != MV_HEADS || cfg->intermediate != MV_INTER ||
      (cfg->proj_dim != MV_PROJ && cfg->proj_dim != MV_HIDDEN))
    return fail(nullptr, MV_ERR_INVALID, "kernels are specialised to hidden=768, heads=12, intermediate=3072, proj_dim=512 (header) "
                                         "or 768 (use_header = False: no header)");
  if (cfg->layers < 0 || cfg->vocab_size <= 0 || cfg->max_pos <= 0 || cfg->max_pos > 512 || cfg->max_tokens <= 0 ||
      cfg->max_batch <= 0 || cfg->max_anchors <= 0 || cfg->type_vocab <= 0 || (cfg->same_idx != 0 && cfg->same_idx != 1))
    return fail(nullptr, MV_ERR_INVALID, "bad mv_config field");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail(nullptr, MV_ERR_HIP, std::string("no HIP device: ") + hipGetErrorString(e));
  if (device < 0 || device >= ndev) return fail(nullptr, MV_ERR_INVALID, "device index out of range");
  e = hipSetDevice(device);
  if (e != hipSuccess) return fail(nullptr, MV_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
  mv_handle* h = new (std::nothrow) mv_handle();
  if (!h) return fail(nullptr, MV_ERR_NOMEM, "out of host memory");
  struct Guard {  // an exception below (caught by this function's handler) must not leak the half-built handle
    mv_handle* h;
    ~Guard() { if (h) mv_destroy(h); }
  } guard{h};
  h->device = device;
  h->cfg = *cfg;
  h->P = cfg->proj_dim;
  {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) h->num_cu = ncu;
  }
  if (int rc = read_switches(h)) return rc;  // (the guard destroys the handle)
  for (int wi = 0; wi < h->n_alloc; ++wi) {
    e = hipStreamCreateWithFlags(&h->work[wi].stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      g_create_error = std::string("hipStreamCreate: ") + hipGetErrorString(e);
      return MV_ERR_HIP;  // the guard destroys the handle
    }
  }
  // dynamic LDS above 64 KiB needs an explicit opt-in — per device, so here and not behind a process-wide flag: every kernel of the two lists the launchers read
  for (const GemmLdsOptIn& k : GEMM_LDS_OPT_INS) hipFuncSetAttribute((const void*)k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds);
  for (const AttnVariant& v : ATTN_VARIANTS) hipFuncSetAttribute((const void*)v.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, v.lds);
  (void)pp_fixed_lds_opt_in();  // the fixed-form persistent GEMMs: kernels of libmemvul_pp_fixed.so, which opts its own list in
  (void)hipGetLastError();

  h->cap_tokens = round_up(cfg->max_tokens, 256) + 256;
  int rc = MV_OK;
  auto A = [&](int r) { if (rc == MV_OK) rc = r; };
  for (int wi = 0; wi < h->n_alloc; ++wi) A(alloc_work(h, h->work[wi], WORK_COMMON));
  const hipStream_t s0 = h->work[0].stream;
  A(dev_alloc(h, s0, &h->anchors, (int64_t)cfg->max_anchors * h->P));
  A(dev_alloc(h, s0, &h->x8_sat, 1));  // (zeroed by dev_alloc)
  A(dev_alloc(h, s0, &h->attn_conc, 4));
  if (rc == MV_OK && hipStreamSynchronize(s0) != hipSuccess) rc = MV_ERR_HIP;
  if (rc != MV_OK) {
    g_create_error = h->err.empty() ? "workspace allocation failed" : h->err;
    return rc;  // the guard destroys the handle
  }
  guard.h = nullptr;
  *out = h;
  return MV_OK;
} catch (...) { return on_exception(nullptr); }

void mv_destroy(mv_handle* h) {
  if (!h) return;
  hipSetDevice(h->device);
  mv_comm_destroy(h);
  for (auto& wk : h->work)
    if (wk.stream) hipStreamSynchronize(wk.stream);
  for (auto& r : h->recs) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
  for (auto e : h->free_events) hipEventDestroy(e);
  for (void* p : h->allocs) hipFree(p);
  for (void* p : h->pinned) hipHostFree(p);
  for (auto& wk : h->work)
    if (wk.stream) hipStreamDestroy(wk.stream);
  delete h;
}

int mv_sync(mv_handle* h) try {
  if (!h) return MV_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  return sync_all(h);
} catch (...) { return on_exception(h); }

int mv_load_tensor(mv_handle* h, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim) try {
  if (!h || !name || !host_ptr || !shape || ndim < 1 || ndim > 4) return fail(h, MV_ERR_INVALID, "mv_load_tensor: bad argument");
  if (h->finalized) return fail(h, MV_ERR_STATE, "weights already finalized");
  int64_t n = 1;
  for (int i = 0; i < ndim; ++i) {
    if (shape[i] < 0) return fail(h, MV_ERR_INVALID, "negative dimension");
    n *= shape[i];
  }
  HostTensor t;
  t.shape.assign(shape, shape + ndim);
  t.data.resize((size_t)n);
  if (dtype == MV_F32) std::memcpy(t.data.data(), host_ptr, (size_t)n * 4);
  else if (dtype == MV_F16) { const uint16_t* s = (const uint16_t*)host_ptr; for (int64_t i = 0; i < n; ++i) t.data[(size_t)i] = f16_bits_to_f32(s[i]); }
  else if (dtype == MV_BF16) { const uint16_t* s = (const uint16_t*)host_ptr; for (int64_t i = 0; i < n; ++i) t.data[(size_t)i] = bf16_bits_to_f32(s[i]); }
  else if (dtype == MV_I64 || dtype == MV_I32) return MV_OK;  // e.g. embeddings.position_ids: accepted, unused
  else return fail(h, MV_ERR_INVALID, "mv_load_tensor: unsupported dtype");
  h->staged[name] = std::move(t);
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_finalize_weights(mv_handle* h, int compute_dtype) try {
  if (!h) return MV_ERR_INVALID;
  if (h->finalized) return fail(h, MV_ERR_STATE, "weights already finalized");
  if (compute_dtype != MV_F16 && compute_dtype != MV_F16X8 && compute_dtype != MV_F32)
    return fail(h, MV_ERR_INVALID, "compute_dtype must be MV_F16 (fp16 MFMA operands, fp32 accumulation), MV_F16X8 (+ fp8 correction "
                                   "sweeps) or MV_F32 (the reference form); bf16 is a storage dtype of mv_load_tensor only (include/memvul_hip.h)");
  const bool precise = compute_dtype == MV_F16X8;
  const bool f32 = compute_dtype == MV_F32;  // the 16-bit weights, the folded ones and the second stream plane are not built
  if (!precise && h->form != MV_FORM_DEFAULT)
    return fail(h, MV_ERR_STATE, "the safe and the guarded form (MEMVUL_FORM / mv_set_form) are forms of compute dtype MV_F16X8: they cannot be combined with MV_F16 or MV_F32");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = upload_weights(h, precise, f32)) return rc;
  if (precise && h->gemm_tile == 128) return fail(h, MV_ERR_STATE, "MV_F16X8 runs on the persistent GEMM path: MEMVUL_GEMM_TILE=128 excludes it");
  for (int wi = 0; wi < h->n_alloc; ++wi)
    if (int rc = alloc_work(h, h->work[wi], compute_dtype)) return rc;
  h->precise = precise;
  h->f32 = f32;
  h->staged.clear();
  h->compute_dtype = compute_dtype;
  h->finalized = true;
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_anchor_reset(mv_handle* h) try {
  if (!h) return MV_ERR_INVALID;
  if (h->corpus.pending) {
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = rescore_corpus(h)) return rc;
  }
  h->n_anchors = 0;
  return MV_OK;
} catch (...) { return on_exception(h); }
int mv_anchor_count(mv_handle* h) { return h ? h->n_anchors : MV_ERR_INVALID; }

int mv_anchor_append(mv_handle* h, const int32_t* ids, const int32_t* lens, int n, int S) try {
  if (int rc = check_ready(h)) return rc;
  if (!ids || !lens || n <= 0 || S <= 0 || S > h->cfg.max_pos) return fail(h, MV_ERR_INVALID, "mv_anchor_append: bad argument");
  if (h->n_anchors + n > h->cfg.max_anchors) return fail(h, MV_ERR_CAPACITY, "anchor bank capacity (mv_config.max_anchors) exceeded");
  if (int rc = check_ids(h, ids, (int64_t)n * S, "mv_anchor_append")) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  for (int wi = 1; wi < h->n_alloc; ++wi)  // a ticket in flight on another set still reads the bank this call writes
    if (h->work[wi].ticket) HIPCHK(h, hipStreamSynchronize(h->work[wi].stream));
  if (int rc = rescore_corpus(h)) return rc;  // (a guarded sweep not yet collected is rescored against the bank it ran on)
  Job j;
  j.ids = ids; j.lens = lens; j.u_dev = h->anchors + (size_t)h->n_anchors * h->P;
  job_form(h, j);
  if (int rc = run_in_order(h, lens, n, S, j)) return rc;
  h->n_anchors += n;
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_anchor_get(mv_handle* h, float* out) try {
  if (!h || !out) return MV_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = sync_all(h)) return rc;  // a sweep may still be appending / reading on the other stream
  Work& wk = h->work[0];
  HIPCHK(h, hipMemcpyAsync(out, h->anchors, (size_t)h->n_anchors * h->P * 4, hipMemcpyDeviceToHost, wk.stream));
  HIPCHK(h, hipStreamSynchronize(wk.stream));
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_anchor_set(mv_handle* h, const float* v, int G) try {
  if (!h || !v || G <= 0) return fail(h, MV_ERR_INVALID, "mv_anchor_set: bad argument");
  if (G > h->cfg.max_anchors) return fail(h, MV_ERR_CAPACITY, "anchor bank capacity (mv_config.max_anchors) exceeded");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = sync_all(h)) return rc;  // batches of a resident sweep in flight read the bank
  if (int rc = rescore_corpus(h)) return rc;
  Work& wk = h->work[0];
  HIPCHK(h, hipMemcpyAsync(h->anchors, v, (size_t)G * h->P * 4, hipMemcpyHostToDevice, wk.stream));
  HIPCHK(h, hipStreamSynchronize(wk.stream));
  h->n_anchors = G;
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_encode(mv_handle* h, const int32_t* ids, const int32_t* lens, int B, int S, float* embed) try {
  if (int rc = check_ready(h)) return rc;
  if (!ids || !lens || B <= 0 || S <= 0 || S > h->cfg.max_pos) return fail(h, MV_ERR_INVALID, "mv_encode: bad argument");
  if (int rc = check_ids(h, ids, (int64_t)B * S, "mv_encode")) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  Job j;
  j.ids = ids; j.lens = lens; j.out.embed = embed;
  job_form(h, j);
  return run_in_order(h, lens, B, S, j);
} catch (...) { return on_exception(h); }

int mv_forward(mv_handle* h, const int32_t* ids, const int32_t* lens, int B, int S, float* logits, float* probs, float* best,
               int32_t* best_idx, float* embed) try {
  if (int rc = check_ready(h)) return rc;
  if (!ids || !lens || B <= 0 || S <= 0 || S > h->cfg.max_pos) return fail(h, MV_ERR_INVALID, "mv_forward: bad argument");
  if (h->n_anchors <= 0) return fail(h, MV_ERR_STATE, "anchor bank is empty (call mv_anchor_append / mv_anchor_set first)");
  if (int rc = check_ids(h, ids, (int64_t)B * S, "mv_forward")) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  Job j;
  j.ids = ids; j.lens = lens; j.match = true;
  j.out.logits = logits; j.out.probs = probs; j.out.best = best; j.out.idx = best_idx; j.out.embed = embed;
  job_form(h, j);
  return run_in_order(h, lens, B, S, j);
} catch (...) { return on_exception(h); }

// ---- by length: mv_forward on a pad-to-longest batch of UNSORTED rows (binding.Engine.forward_by_length) ----------------------------------------------------------
// enqueue_batch plans the rows by length, stages them in that order (each pass at its own width) and runs the passes back to back on one stream; collect_batch
// waits, rescores and puts the results back in the caller's row order.
// The whole flow in ONE call on workspace set 0 with the pageable staging: one release of the caller's interpreter lock per batch (next to two other Python
// threads every release cost the scoring thread ~10 ms of waiting: profiles/r06_*_e2e_dropin.txt).
int mv_forward_ragged(mv_handle* h, const int32_t* ids, const int32_t* lens, int B, int S, int min_tokens, float* logits, float* probs, float* best,
                      int32_t* best_idx, float* embed) try {
  if (int rc = check_ready(h)) return rc;
  if (!ids || !lens || B <= 0 || S <= 0 || S > h->cfg.max_pos || !best || !best_idx) return fail(h, MV_ERR_INVALID, "mv_forward_ragged: bad argument");
  if (h->n_anchors <= 0) return fail(h, MV_ERR_STATE, "anchor bank is empty (call mv_anchor_append / mv_anchor_set first)");
  if (int rc = check_ids(h, ids, (int64_t)B * S, "mv_forward_ragged")) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  Work& wk = h->work[0];
  const Stage dst{nullptr, nullptr, best_idx, logits, probs, best, embed};
  Job j;
  j.match = true;
  job_form(h, j);
  if (int rc = enqueue_batch(h, wk, h->plan, h->routed, &h->stage, ids, lens, B, S, min_tokens, true, wanted(dst, embed != nullptr), j)) return rc;
  return collect_batch(h, wk, h->plan, j, B, dst);
} catch (...) { return on_exception(h); }

// mv_forward_ragged in two halves, so that the caller can hand over batch k + 1 BEFORE it collects batch k: `begin` is enqueue_batch on a workspace set without
// a ticket, into that set's pinned staging, and returns a ticket (the set) without waiting; `end` is collect_batch on that set with the job the ticket was begun
// with — its form, its routing and its anchor count.  At most one batch per workspace set (MEMVUL_STREAMS: 2) is in flight; tickets are collected in the order
// they were issued.  The GPU then never waits for the caller's Python between two batches (predict_memory.evaluate).
int mv_forward_ragged_begin(mv_handle* h, const int32_t* ids, const int32_t* lens, int B, int S, int min_tokens, int want_logits, int want_probs, int want_embed,
                            int* ticket) try {
  if (int rc = check_ready(h)) return rc;
  if (!ids || !lens || !ticket || B <= 0 || S <= 0 || S > h->cfg.max_pos) return fail(h, MV_ERR_INVALID, "mv_forward_ragged_begin: bad argument");
  if (h->n_anchors <= 0) return fail(h, MV_ERR_STATE, "anchor bank is empty (call mv_anchor_append / mv_anchor_set first)");
  if (B > h->cfg.max_batch) return fail(h, MV_ERR_CAPACITY, "mv_forward_ragged_begin: the batch exceeds mv_config.max_batch");
  int set = 0;
  while (set < h->n_alloc && h->work[set].ticket) ++set;
  if (set == h->n_alloc) return fail(h, MV_ERR_CAPACITY, "mv_forward_ragged_begin: every workspace set has a batch in flight (score this one with mv_forward_ragged)");
  Work& wk = h->work[set];
  if (int rc = check_ids(h, ids, (int64_t)B * S, "mv_forward_ragged_begin")) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  if (!wk.pin.best) {  // pinned staging of this set, once: [max_batch][max_pos], [max_batch] x 2, [max_batch][max_anchors][2] x 2, [max_batch][2], [max_batch][P]
    const size_t mb = (size_t)h->cfg.max_batch, bg2 = mb * (size_t)h->cfg.max_anchors * 2;
    Stage s;
    auto pin = [&](void** p, size_t bytes) -> int {
      if (hipHostMalloc(p, bytes, hipHostMallocDefault) != hipSuccess) return fail(h, MV_ERR_NOMEM, "hipHostMalloc failed (mv_forward_ragged_begin)");
      h->pinned.push_back(*p);
      return MV_OK;
    };
    int rc = pin((void**)&s.ids, mb * (size_t)h->cfg.max_pos * 4);
    if (!rc) rc = pin((void**)&s.lens, mb * 4);
    if (!rc) rc = pin((void**)&s.idx, mb * 4);
    if (!rc) rc = pin((void**)&s.logits, bg2 * 4);
    if (!rc) rc = pin((void**)&s.probs, bg2 * 4);
    if (!rc) rc = pin((void**)&s.best, mb * 2 * 4);
    if (!rc) rc = pin((void**)&s.embed, mb * (size_t)h->P * 4);
    if (!rc) rc = pin((void**)&s.over, mb * 4);
    if (rc) return rc;
    wk.pin = s;
  }
  wk.job = Job();
  wk.job.match = true;
  job_form(h, wk.job);  // (the form, the sink-token list and the bank in force HERE are the ticket's)
  if (int rc = enqueue_batch(h, wk, wk.plan, wk.routed, nullptr, ids, lens, B, S, min_tokens, true, Want{want_logits != 0, want_probs != 0, true, true, want_embed != 0},
                             wk.job)) return rc;
  wk.ticket = true;
  *ticket = set;
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_forward_ragged_end(mv_handle* h, int ticket, float* logits, float* probs, float* best, int32_t* best_idx, float* embed) try {
  if (!h || ticket < 0 || ticket > 1 || !h->work[ticket].ticket) return fail(h, MV_ERR_STATE, "mv_forward_ragged_end: no batch in flight under this ticket");
  Work& wk = h->work[ticket];
  HIPCHK(h, hipSetDevice(h->device));
  wk.ticket = false;
  const Stage& st = wk.job.out;  // (the batch's ids are still in the pinned staging; the bank rows it was matched against are the first wk.job.G of what the bank holds now)
  if (!best || !best_idx || (st.logits && !logits) || (st.probs && !probs) || (st.embed && !embed)) {
    hipStreamSynchronize(wk.stream);  // (the set is free again only once its batch has left the pinned staging alone)
    return fail(h, MV_ERR_INVALID, "mv_forward_ragged_end: an output the batch was started with is missing");
  }
  return collect_batch(h, wk, wk.plan, wk.job, (int)wk.plan.order.size(), Stage{nullptr, nullptr, best_idx, logits, probs, best, embed});
} catch (...) { return on_exception(h); }

int mv_match(mv_handle* h, const float* u, int B, float* logits, float* probs, float* best, int32_t* best_idx) try {
  if (int rc = check_ready(h)) return rc;
  if (!u || B <= 0) return fail(h, MV_ERR_INVALID, "mv_match: bad argument");
  if (B > h->cfg.max_batch) return fail(h, MV_ERR_CAPACITY, "B exceeds mv_config.max_batch");
  HIPCHK(h, hipSetDevice(h->device));
  Work& wk = h->work[0];
  const int G = h->n_anchors;
  HIPCHK(h, hipMemcpyAsync(wk.u_in, u, (size_t)B * h->P * 4, hipMemcpyHostToDevice, wk.stream));
  if (int rc = match_dev(h, wk, wk.u_in, B, G, logits ? wk.logits : nullptr, probs ? wk.probs : nullptr, nullptr, 1, wk.best,
                         wk.best_idx)) return rc;
  const size_t bg = (size_t)B * G;
  if (logits) HIPCHK(h, hipMemcpyAsync(logits, wk.logits, bg * 8, hipMemcpyDeviceToHost, wk.stream));
  if (probs) HIPCHK(h, hipMemcpyAsync(probs, wk.probs, bg * 8, hipMemcpyDeviceToHost, wk.stream));
  if (best) HIPCHK(h, hipMemcpyAsync(best, wk.best, (size_t)B * 8, hipMemcpyDeviceToHost, wk.stream));
  if (best_idx) HIPCHK(h, hipMemcpyAsync(best_idx, wk.best_idx, (size_t)B * 4, hipMemcpyDeviceToHost, wk.stream));
  HIPCHK(h, hipStreamSynchronize(wk.stream));
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_topk(mv_handle* h, const float* u, int B, int k, float* topk_p, int32_t* topk_idx) try {
  if (int rc = check_ready(h)) return rc;
  if (!u || B <= 0 || k <= 0 || k > 64 || !topk_p || !topk_idx) return fail(h, MV_ERR_INVALID, "mv_topk: bad argument (1 <= k <= 64)");
  if (B > h->cfg.max_batch) return fail(h, MV_ERR_CAPACITY, "B exceeds mv_config.max_batch");
  if (k > h->n_anchors) return fail(h, MV_ERR_INVALID, "k exceeds the number of anchors");
  HIPCHK(h, hipSetDevice(h->device));
  Work& wk = h->work[0];
  HIPCHK(h, hipMemcpyAsync(wk.u_in, u, (size_t)B * h->P * 4, hipMemcpyHostToDevice, wk.stream));
  // one fused pass: P(same) [B, G] never reaches HBM, only 8 B k bytes of results do
  if (int rc = match_dev(h, wk, wk.u_in, B, h->n_anchors, nullptr, nullptr, nullptr, k, nullptr, nullptr, wk.topk_p, wk.topk_idx)) return rc;
  HIPCHK(h, hipMemcpyAsync(topk_p, wk.topk_p, (size_t)B * k * 4, hipMemcpyDeviceToHost, wk.stream));
  HIPCHK(h, hipMemcpyAsync(topk_idx, wk.topk_idx, (size_t)B * k * 4, hipMemcpyDeviceToHost, wk.stream));
  HIPCHK(h, hipStreamSynchronize(wk.stream));
  return MV_OK;
} catch (...) { return on_exception(h); }

// GPUs visible to this process (hipGetDeviceCount): 0 on a box without one (a HIP error there is "none", not a failure).
int mv_device_count(void) try {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
} catch (...) { return on_exception(nullptr); }

// ---- measurement / debug -----------------------------------------------------------------------
int mv_profile_enable(mv_handle* h, int on) try {
  if (!h) return MV_ERR_INVALID;
  h->prof = on != 0;
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_set_streams(mv_handle* h, int n) try {
  if (!h || (n != 1 && n != 2)) return fail(h, MV_ERR_INVALID, "mv_set_streams: 1 or 2");
  if (n == 2 && !h->work[1].stream) return fail(h, MV_ERR_STATE, "mv_set_streams: the second workspace set was not created (MEMVUL_STREAMS=1)");
  if (int rc = sync_all(h)) return rc;
  h->n_streams = n;
  h->rr = 0;
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_set_form(mv_handle* h, int form) try {
  if (!h) return MV_ERR_INVALID;
  if (form != MV_FORM_DEFAULT && form != MV_FORM_SAFE && form != MV_FORM_GUARDED)
    return fail(h, MV_ERR_INVALID, "mv_set_form: MV_FORM_DEFAULT (0), MV_FORM_SAFE (1) or MV_FORM_GUARDED (2)");
  if (form != MV_FORM_DEFAULT && h->finalized && !h->precise)
    return fail(h, MV_ERR_STATE, "mv_set_form: MV_FORM_SAFE and MV_FORM_GUARDED are forms of compute dtype MV_F16X8; this handle was finalized as MV_F16 or MV_F32");
  h->form = form;  // (no synchronisation: passes already enqueued were built with the form of their time)
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_get_form(mv_handle* h) try {
  if (!h) return MV_ERR_INVALID;
  return h->form;
} catch (...) { return on_exception(h); }

int mv_form_stats(mv_handle* h, int64_t* sequences, int64_t* rescored, int reset) try {
  if (!h || !sequences || !rescored) return fail(h, MV_ERR_INVALID, "mv_form_stats: bad argument");
  *sequences = h->guard_seqs;
  *rescored = h->guard_rescored;
  if (reset) h->guard_seqs = h->guard_rescored = 0;
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_set_sink_tokens(mv_handle* h, const int32_t* ids, int n) try {
  if (!h) return MV_ERR_INVALID;
  if (!h->finalized) return fail(h, MV_ERR_STATE, "mv_set_sink_tokens: weights not finalized (mv_finalize_weights)");
  if (!h->precise) return fail(h, MV_ERR_STATE, "mv_set_sink_tokens: the list routes between forms of compute dtype MV_F16X8; this handle was finalized as MV_F16 or MV_F32");
  if (n < 0 || n > MV_MAX_SINK_TOKENS || (n > 0 && !ids)) return fail(h, MV_ERR_INVALID, "mv_set_sink_tokens: 0 .. 64 token ids");
  for (int i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= h->cfg.vocab_size) return fail(h, MV_ERR_INVALID, "mv_set_sink_tokens: token id outside [0, vocab_size)");
  std::vector<int32_t> list(ids, ids + n);
  std::vector<uint32_t> bm = route_bitmap(ids, n, h->cfg.vocab_size);
  h->sink_tokens.swap(list);  // (nothing below throws: the list is replaced whole or not at all)
  h->sink_bitmap.swap(bm);
  h->corpus.route_stale = true;
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_get_sink_tokens(mv_handle* h, int32_t* ids, int capacity) try {
  if (!h) return MV_ERR_INVALID;
  if (capacity < 0 || (capacity > 0 && !ids)) return fail(h, MV_ERR_INVALID, "mv_get_sink_tokens: bad argument");
  const int n = (int)h->sink_tokens.size();
  for (int i = 0; i < n && i < capacity; ++i) ids[i] = h->sink_tokens[(size_t)i];
  return n;
} catch (...) { return on_exception(h); }

int mv_route_stats(mv_handle* h, int64_t* routed, int reset) try {
  if (!h || !routed) return fail(h, MV_ERR_INVALID, "mv_route_stats: bad argument");
  *routed = h->routed_seqs;
  if (reset) h->routed_seqs = 0;
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_route_scan(const int32_t* ids, const int32_t* lens, int B, int S, const int32_t* tokens, int n, int vocab, uint8_t* flags) try {
  if (!ids || !lens || !flags || B < 0 || S <= 0 || vocab <= 0 || n < 0 || n > MV_MAX_SINK_TOKENS || (n > 0 && !tokens)) return MV_ERR_INVALID;
  for (int i = 0; i < n; ++i)
    if (tokens[i] < 0 || tokens[i] >= vocab) return MV_ERR_INVALID;
  const std::vector<uint32_t> bm = route_bitmap(tokens, n, vocab);
  route_scan(ids, lens, B, S, bm.data(), vocab, flags);
  return MV_OK;
} catch (...) { return on_exception(nullptr); }

int mv_last_row_forms(mv_handle* h, uint8_t* forms, int n) try {
  if (!h || !forms || n < 0 || (size_t)n != h->last_forms.size()) return fail(h, MV_ERR_INVALID, "mv_last_row_forms: n is not the row count of the last call");
  std::memcpy(forms, h->last_forms.data(), (size_t)n);
  return MV_OK;
} catch (...) { return on_exception(h); }

// launches of this handle that took a fixed-form persistent GEMM (encoder_pass.h launch_pp) since it was created or last reset; a host counter, no synchronisation.
// Outside the mv_ names: a figure for tests and A/B scripts, not an entry of the product ABI
int64_t mvpp_fixed_launches(mv_handle* h, int reset) {
  if (!h) return -1;
  const int64_t n = h->pp_fixed_launches;
  if (reset) h->pp_fixed_launches = 0;
  return n;
}

int mv_x8_saturation(mv_handle* h, int64_t* clamped, int reset) try {
  if (!h || !clamped) return fail(h, MV_ERR_INVALID, "mv_x8_saturation: bad argument");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = sync_all(h)) return rc;
  unsigned long long v = 0;
  HIPCHK(h, hipMemcpy(&v, h->x8_sat, sizeof(v), hipMemcpyDeviceToHost));
  if (reset) HIPCHK(h, hipMemset(h->x8_sat, 0, sizeof(v)));
  *clamped = v > (unsigned long long)INT64_MAX ? INT64_MAX : (int64_t)v;
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_attention_concentration(mv_handle* h, float* max_collision, int64_t* items_over, int64_t* items_total, int reset) try {
  if (!h || !max_collision || !items_over || !items_total) return fail(h, MV_ERR_INVALID, "mv_attention_concentration: bad argument");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = sync_all(h)) return rc;
  unsigned long long v[4] = {0, 0, 0, 0};
  HIPCHK(h, hipMemcpy(v, h->attn_conc, sizeof(v), hipMemcpyDeviceToHost));
  if (reset) HIPCHK(h, hipMemset(h->attn_conc, 0, sizeof(v)));
  const uint32_t bits = (uint32_t)v[0];
  std::memcpy(max_collision, &bits, 4);
  *items_over = v[1] > (unsigned long long)INT64_MAX ? INT64_MAX : (int64_t)v[1];
  *items_total = v[2] > (unsigned long long)INT64_MAX ? INT64_MAX : (int64_t)v[2];
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_sink_census_enable(mv_handle* h, int on) try {
  if (!h) return MV_ERR_INVALID;
  if (!h->finalized) return fail(h, MV_ERR_STATE, "mv_sink_census_enable: weights not finalized (mv_finalize_weights)");
  if (!h->precise) return fail(h, MV_ERR_STATE, "mv_sink_census_enable: the census reads the planes of compute dtype MV_F16X8; this handle was finalized as MV_F16 or MV_F32");
  if (on && !h->census_items) {
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s0 = h->work[0].stream;
    if (int rc = dev_alloc(h, s0, &h->census_items, (int64_t)h->cfg.vocab_size)) return rc;
    if (int rc = dev_alloc(h, s0, &h->census_share, (int64_t)h->cfg.vocab_size)) return rc;
    if (int rc = dev_alloc(h, s0, &h->census_heads, (int64_t)h->cfg.layers * MV_HEADS)) return rc;
    HIPCHK(h, hipStreamSynchronize(s0));  // (zeroed before a pass on another stream can add to them)
  }
  h->census = on != 0;  // (read on the host when a pass is enqueued: work in flight keeps what it was enqueued with)
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_sink_census_read(mv_handle* h, uint32_t* items, uint64_t* share_q20, int vocab, uint32_t* by_head, int layers_x_heads, int reset) try {
  if (!h) return MV_ERR_INVALID;
  if (!h->census_items) return fail(h, MV_ERR_STATE, "mv_sink_census_read: the census was never enabled (mv_sink_census_enable)");
  if (vocab != h->cfg.vocab_size || layers_x_heads != h->cfg.layers * MV_HEADS)
    return fail(h, MV_ERR_INVALID, "mv_sink_census_read: vocab must be mv_config.vocab_size and layers_x_heads mv_config.layers * 12");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = sync_all(h)) return rc;
  const size_t V = (size_t)vocab, LH = (size_t)layers_x_heads;
  if (items) HIPCHK(h, hipMemcpy(items, h->census_items, V * 4, hipMemcpyDeviceToHost));
  if (share_q20) HIPCHK(h, hipMemcpy(share_q20, h->census_share, V * 8, hipMemcpyDeviceToHost));
  if (by_head) HIPCHK(h, hipMemcpy(by_head, h->census_heads, LH * 4, hipMemcpyDeviceToHost));
  if (reset) {
    HIPCHK(h, hipMemset(h->census_items, 0, V * 4));
    HIPCHK(h, hipMemset(h->census_share, 0, V * 8));
    HIPCHK(h, hipMemset(h->census_heads, 0, LH * 4));
  }
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_profile_select(mv_handle* h, uint32_t class_mask) try {
  if (!h) return MV_ERR_INVALID;
  h->prof_mask = class_mask;
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_profile_read(mv_handle* h, double* ms, int64_t* launches, int n) try {
  if (!h || !ms || !launches || n < MV_NUM_KERNEL_CLASSES) return fail(h, MV_ERR_INVALID, "mv_profile_read: bad argument");
  if (int rc = sync_all(h)) return rc;
  for (int i = 0; i < n; ++i) { ms[i] = 0; launches[i] = 0; }
  for (auto& r : h->recs) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, r.e0, r.e1) == hipSuccess) { ms[r.cls] += t; launches[r.cls] += 1; }
    h->free_events.push_back(r.e0);
    h->free_events.push_back(r.e1);
  }
  h->recs.clear();
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_debug_encode(mv_handle* h, const int32_t* ids, const int32_t* lens, int B, int S, int n_layers) try {
  if (int rc = check_ready(h)) return rc;
  if (!ids || !lens || B <= 0 || S <= 0 || S > h->cfg.max_pos) return fail(h, MV_ERR_INVALID, "mv_debug_encode: bad argument");
  if (B > max_rows_for(h, S)) return fail(h, MV_ERR_CAPACITY, "mv_debug_encode: batch too large for one pass");
  if (int rc = check_ids(h, ids, (int64_t)B * S, "mv_debug_encode")) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  Job j;  // (on workspace set 0: what mv_debug_read reads)
  j.ids = ids; j.lens = lens; j.n_layers = n_layers < 0 ? h->cfg.layers : n_layers; j.full = true;
  j.safe = h->precise && h->form == MV_FORM_SAFE;  // (MV_FORM_GUARDED: the taps show the default form, nothing is rescored)
  return run_in_order(h, lens, B, S, j);
} catch (...) { return on_exception(h); }

int mv_debug_read(mv_handle* h, int buffer, void* dst, int64_t bytes) try {
  if (!h || !dst || bytes <= 0) return MV_ERR_INVALID;
  Work& wk = h->work[0];  // (mv_debug_encode's set)
  const int64_t T = (int64_t)h->dbg_B * h->dbg_Sp, Tp = round_up(T, 256);
  const void* src = nullptr;
  int64_t avail = 0;
  if (h->f32 && buffer >= 1 && buffer <= 9)
    return fail(h, MV_ERR_INVALID, "mv_debug_read: buffers 1 - 9 are the fp16 planes of MV_F16 / MV_F16X8; an MV_F32 handle has buffer 0 (hidden fp32), 10 (embedding) and its fp32 planes 35 - 37 (Q | K | V, context, GELU output)");
  switch (buffer) {
    case 0: src = wk.xres; avail = T * MV_HIDDEN * 4; break;
    case 1: src = wk.x16; avail = T * MV_HIDDEN * 2; break;
    case 2: src = wk.q; avail = T * MV_HIDDEN * 2; break;
    case 3: src = wk.k; avail = T * MV_HIDDEN * 2; break;
    case 4: src = wk.vt; avail = T * MV_HIDDEN * 2; break;
    case 5: src = wk.ctx; avail = T * MV_HIDDEN * 2; break;
    case 6: src = wk.h16; avail = T * MV_INTER * 2; break;
    case 7: src = wk.q_lo; avail = T * MV_HIDDEN * 2; break;
    case 8: src = wk.k_lo; avail = T * MV_HIDDEN * 2; break;
    case 9: src = wk.vt_lo; avail = T * MV_HIDDEN * 2; break;
    case 10: src = wk.u; avail = (int64_t)h->dbg_B * h->P * 4; break;
    // the raw planes of the persistent path (include/memvul_hip.h); the compact special-row buffers hold 2 rows per sequence; the per-token planes can be
    // read to the end of the pass' last 256-row tile (Tp rows: the persistent GEMMs compute the rows past B*Sp like any other)
    case 11: src = wk.x8; avail = Tp * 2 * MV_HIDDEN; break;
    case 12: src = wk.st_lo; avail = (int64_t)2 * h->dbg_B * MV_HIDDEN * 2; break;
    case 13: src = wk.lnstats; avail = Tp * 6 * 4; break;
    case 14: src = wk.lnpart; avail = Tp * 6 * 4; break;
    case 15: src = wk.ctx8; avail = Tp * 2 * MV_HIDDEN; break;
    case 16: src = wk.cls_lo; avail = (int64_t)2 * h->dbg_B * MV_INTER * 2; break;
    case 17: src = wk.h8; avail = Tp * 2 * MV_INTER; break;
    case 18: src = wk.vlo_sp; avail = (int64_t)h->dbg_B * MV_HEADS * MV_HEAD_DIM * 2 * 2; break;
    case 19: src = wk.xlo; avail = Tp * MV_HIDDEN * 2; break;
    case 20: src = wk.cls_corr; avail = (int64_t)2 * h->dbg_B * MV_INTER * 4; break;
    case 21: src = wk.tile_both; avail = (int64_t)((T + 255) / 256) * 4; break;
    // the fp32 planes of the reference form (MV_F32 only; allocated for no other compute dtype), token order
    case 35: src = wk.qkv32; avail = T * 3 * MV_HIDDEN * 4; break;
    case 36: src = wk.ctx32; avail = T * MV_HIDDEN * 4; break;
    case 37: src = wk.h32; avail = T * MV_INTER * 4; break;
#if defined(MEMVUL_DEV_SWITCHES)
    // the tail taps (include/memvul_hip.h 22 - 34; encoder_pass.h tail_tap): B rows each, of the last pruned pass on workspace set 0
    case 22: case 23: case 24: case 25: case 26: case 27: case 28: case 29: case 30: case 31: case 32: case 33: {
      const int s = buffer - 22;
      if (!h->dbg_tail) return fail(h, MV_ERR_STATE, "mv_debug_read: the tail taps 22 - 34 exist with MEMVUL_DEBUG_TAIL=1 only");
      if (h->f32 || !h->tail_arena) return fail(h, MV_ERR_STATE, "mv_debug_read: no pruned pass has filled the tail taps");
      int64_t row = TT_ROW[s];
      if (!h->precise && (s == TT_CTX || s == TT_FFN1)) row /= 2;  // MV_F16: cctx / ch16 are fp16
      if (s == TT_U) row = (int64_t)h->P * 4;
      src = h->tail_arena + tt_off(s) * h->cfg.max_batch; avail = (int64_t)h->dbg_B * row;
      break;
    }
    case 34: {  // int32 [3]: pruned passes tapped since mv_create, and the rows and the padded length of the last pass (host state: no copy from the device)
      if (bytes > 12) return fail(h, MV_ERR_INVALID, "mv_debug_read: more bytes requested than the buffer holds");
      const int32_t info[3] = {h->tail_passes, h->dbg_B, h->dbg_Sp};
      HIPCHK(h, hipStreamSynchronize(wk.stream));
      std::memcpy(dst, info, (size_t)bytes);
      return MV_OK;
    }
#endif
    default: return fail(h, MV_ERR_INVALID, "mv_debug_read: unknown buffer");
  }
  if (!src) return fail(h, MV_ERR_STATE, "mv_debug_read: this buffer does not exist in this compute dtype");
  if (bytes > avail) return fail(h, MV_ERR_INVALID, "mv_debug_read: more bytes requested than the buffer holds");
  HIPCHK(h, hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, wk.stream));
  HIPCHK(h, hipStreamSynchronize(wk.stream));
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_test_gemm(mv_handle* h, int variant, int M, int N, int K, const uint16_t* A, const uint16_t* W, const float* bias,
                 float* C, int iters, float* ms) try {
  if (!h || !A || !W || M <= 0 || N <= 0 || K <= 0) return fail(h, MV_ERR_INVALID, "mv_test_gemm: bad argument");
  if (variant != 0 && variant != 19) return fail(h, MV_ERR_INVALID, "mv_test_gemm: variant 0 (128^2 tile) or 19 (64^2 ring)");
  if (variant == 0 && (M % 128 || N % 128 || K % 64)) return fail(h, MV_ERR_INVALID, "mv_test_gemm: M,N % 128 and K % 64 required");
  HIPCHK(h, hipSetDevice(h->device));
  const hipStream_t s0 = h->work[0].stream;
  half_t *dA = nullptr, *dW = nullptr;
  float *dB = nullptr, *dC = nullptr;
  int rc;
  if ((rc = dev_alloc(h, s0, &dA, (int64_t)M * K, false))) return rc;
  if ((rc = dev_alloc(h, s0, &dW, (int64_t)N * K, false))) return rc;
  if ((rc = dev_alloc(h, s0, &dB, N))) return rc;
  if ((rc = dev_alloc(h, s0, &dC, (int64_t)M * N))) return rc;
  HIPCHK(h, hipMemcpyAsync(dA, A, (size_t)M * K * 2, hipMemcpyHostToDevice, s0));
  HIPCHK(h, hipMemcpyAsync(dW, W, (size_t)N * K * 2, hipMemcpyHostToDevice, s0));
  if (bias) HIPCHK(h, hipMemcpyAsync(dB, bias, (size_t)N * 4, hipMemcpyHostToDevice, s0));
  GemmArgs g{};
  g.A = dA; g.W = dW; g.bias = dB; g.M = M; g.Mreal = M; g.N = N; g.K = K; g.outf = dC; g.S = 64;
  rc = timed_launches(h, s0, iters, ms, "test gemm", [&]() -> int { return variant == 0 ? launch_gemm128<EPI_F32>(h, s0, KC_TEST_GEMM, g) : launch_ring64<EPI_F32>(h, s0, KC_TEST_GEMM, g); });
  if (rc == MV_OK && C) {
    hipError_t se = hipMemcpy(C, dC, (size_t)M * N * 4, hipMemcpyDeviceToHost);
    if (se != hipSuccess) rc = fail(h, MV_ERR_HIP, std::string("test gemm copy: ") + hipGetErrorString(se));
  }
  dev_free(h, dA); dev_free(h, dW); dev_free(h, dB); dev_free(h, dC);
  return rc;
} catch (...) { return on_exception(h); }

// The MV_F32 GEMM (ref_f32.h) on caller data: C = act(A W^T + bias) (+ res), everything fp32.  act 0 bias only, 1 GELU, 2 + res.
int mv_test_gemm_f32(mv_handle* h, int act, int M, int N, int K, const float* A, const float* W, const float* bias, const float* res, float* C, int iters,
                     float* ms) try {
  if (!h || !A || !W || M <= 0 || N <= 0 || K <= 0) return fail(h, MV_ERR_INVALID, "mv_test_gemm_f32: bad argument");
  if (act < RF_ACT_NONE || act > RF_ACT_RES || (act == RF_ACT_RES && !res)) return fail(h, MV_ERR_INVALID, "mv_test_gemm_f32: act 0 (bias), 1 (GELU) or 2 (+ res, res required)");
  if (M % 128 || N % 128 || K % 32) return fail(h, MV_ERR_INVALID, "mv_test_gemm_f32: M,N % 128 and K % 32 required");
  HIPCHK(h, hipSetDevice(h->device));
  const hipStream_t s0 = h->work[0].stream;
  float *dA = nullptr, *dW = nullptr, *dB = nullptr, *dR = nullptr, *dC = nullptr;
  int rc;
  if ((rc = dev_alloc(h, s0, &dA, (int64_t)M * K, false))) return rc;
  if ((rc = dev_alloc(h, s0, &dW, (int64_t)N * K, false))) return rc;
  if ((rc = dev_alloc(h, s0, &dB, N))) return rc;
  if ((rc = dev_alloc(h, s0, &dR, (int64_t)M * N))) return rc;
  if ((rc = dev_alloc(h, s0, &dC, (int64_t)M * N))) return rc;
  HIPCHK(h, hipMemcpyAsync(dA, A, (size_t)M * K * 4, hipMemcpyHostToDevice, s0));
  HIPCHK(h, hipMemcpyAsync(dW, W, (size_t)N * K * 4, hipMemcpyHostToDevice, s0));
  if (bias) HIPCHK(h, hipMemcpyAsync(dB, bias, (size_t)N * 4, hipMemcpyHostToDevice, s0));
  if (res) HIPCHK(h, hipMemcpyAsync(dR, res, (size_t)M * N * 4, hipMemcpyHostToDevice, s0));
  auto run = [&]() -> int {
    switch (act) {
      case RF_ACT_GELU: return launch_gemm_f32<RF_ACT_GELU>(h, s0, KC_TEST_GEMM, dA, dW, dB, nullptr, dC, M, N, K);
      case RF_ACT_RES: return launch_gemm_f32<RF_ACT_RES>(h, s0, KC_TEST_GEMM, dA, dW, dB, dR, dC, M, N, K);
      default: return launch_gemm_f32<RF_ACT_NONE>(h, s0, KC_TEST_GEMM, dA, dW, dB, nullptr, dC, M, N, K);
    }
  };
  rc = timed_launches(h, s0, iters, ms, "test gemm_f32", run);
  if (rc == MV_OK && C) {
    hipError_t se = hipMemcpy(C, dC, (size_t)M * N * 4, hipMemcpyDeviceToHost);
    if (se != hipSuccess) rc = fail(h, MV_ERR_HIP, std::string("test gemm_f32 copy: ") + hipGetErrorString(se));
  }
  dev_free(h, dA); dev_free(h, dW); dev_free(h, dB); dev_free(h, dR); dev_free(h, dC);
  return rc;
} catch (...) { return on_exception(h); }

// The FFN-1 kernel of the persistent path (gemm_pp_kernel<PP_GELU, RAW>) on caller-provided fp32 operands with unit row
// statistics: out16 = fp16(gelu(A W^T + bias)) [M][N]; x8 != 0: the MV_F16X8 build (fp16 sweep + fp8 correction sweep) and, with
// out8, the [lo8 | hi8] planes of the output [M][2 N].  A / W are split into their planes on the host exactly as
// mv_finalize_weights does for weights (W) and as the producing epilogues do for activations (A: shift MV_X8_ACT_SHIFT).
int mv_test_gemm_pp(mv_handle* h, int x8, int M, int N, int K, const float* A, const float* W, const float* bias, uint16_t* out16,
                    uint8_t* out8, int iters, float* ms) try {
  if (!h || !A || !W || !bias || !out16 || M <= 0 || N <= 0 || K <= 0) return fail(h, MV_ERR_INVALID, "mv_test_gemm_pp: bad argument");
  if (M % 256 || N % 256 || K % 128 || K < 256 || N > MV_INTER)
    return fail(h, MV_ERR_INVALID, "mv_test_gemm_pp: M,N % 256, K % 128, K >= 256, N <= 3072 required");
  if (x8 == 2 && K % 256) return fail(h, MV_ERR_INVALID, "mv_test_gemm_pp: the weight-side-only sweep walks K / 128 K-tiles in pairs: K % 256 required");
  HIPCHK(h, hipSetDevice(h->device));
  const hipStream_t s0 = h->work[0].stream;
  std::vector<uint16_t> a16((size_t)M * K), w16((size_t)N * K);
  for (size_t i = 0; i < a16.size(); ++i) a16[i] = f32_to_f16_bits(A[i]);
  for (size_t i = 0; i < w16.size(); ++i) w16[i] = f32_to_f16_bits(W[i]);
  std::vector<uint8_t> a8, w8;
  int scale_word = 0;
  if (x8) {
    make_x8_weight_planes(W, N, K, w8, &scale_word);
    a8.resize((size_t)M * 2 * K);
    const float sh = std::ldexp(1.0f, MV_X8_ACT_SHIFT), sl = std::ldexp(1.0f, 11 + MV_X8_ACT_SHIFT);
    for (int64_t m = 0; m < M; ++m)
      for (int64_t k = 0; k < K; ++k) {
        const float v = A[m * K + k], hi = f16_bits_to_f32(a16[(size_t)(m * K + k)]);
        a8[(size_t)(m * 2 * K + k)] = f32_to_e4m3_bits((v - hi) * sl);   // [lo8 | hi8]
        a8[(size_t)(m * 2 * K + K + k)] = f32_to_e4m3_bits(v * sh);
      }
  }
  std::vector<float> st((size_t)M * 6, 0.f);
  for (int64_t m = 0; m < M; ++m) st[(size_t)m * 6 + 1] = (float)MV_HIDDEN;  // (sum, sumsq) = (0, 768): mean 0, rstd 1
  half_t *dA = nullptr, *dW = nullptr, *dO = nullptr;
  uint8_t *dA8 = nullptr, *dW8 = nullptr, *dO8 = nullptr;
  float *dB = nullptr, *dS = nullptr;
  int rc;
  if ((rc = dev_alloc(h, s0, &dA, (int64_t)M * K, false))) return rc;
  if ((rc = dev_alloc(h, s0, &dW, (int64_t)N * K, false))) return rc;
  if ((rc = dev_alloc(h, s0, &dO, (int64_t)M * N))) return rc;
  if ((rc = dev_alloc(h, s0, &dB, N, false))) return rc;
  if ((rc = dev_alloc(h, s0, &dS, (int64_t)M * 6, false))) return rc;
  HIPCHK(h, hipMemcpyAsync(dA, a16.data(), a16.size() * 2, hipMemcpyHostToDevice, s0));
  HIPCHK(h, hipMemcpyAsync(dW, w16.data(), w16.size() * 2, hipMemcpyHostToDevice, s0));
  HIPCHK(h, hipMemcpyAsync(dB, bias, (size_t)N * 4, hipMemcpyHostToDevice, s0));
  HIPCHK(h, hipMemcpyAsync(dS, st.data(), st.size() * 4, hipMemcpyHostToDevice, s0));
  GemmArgs g{};
  g.A = dA; g.W = dW; g.bias = dB; g.M = M; g.Mreal = M; g.N = N; g.K = K; g.out16 = dO; g.S = 64; g.lnstats = dS; g.ln_eps = 0.f;
  if (x8) {
    if ((rc = dev_alloc(h, s0, &dA8, (int64_t)a8.size(), false))) return rc;
    if ((rc = dev_alloc(h, s0, &dW8, (int64_t)w8.size(), false))) return rc;
    if ((rc = dev_alloc(h, s0, &dO8, (int64_t)M * 2 * N))) return rc;
    HIPCHK(h, hipMemcpyAsync(dA8, a8.data(), a8.size(), hipMemcpyHostToDevice, s0));
    HIPCHK(h, hipMemcpyAsync(dW8, w8.data(), w8.size(), hipMemcpyHostToDevice, s0));
    g.A8 = dA8; g.W8 = dW8; g.out8 = dO8; g.x8_scale = scale_word;
    g.x8_terms = (x8 == 2) ? 1 : 2;  // x8 = 2: the weight-side term only (the QKV projection's form)
  }
  rc = timed_launches(h, s0, iters, ms, "test gemm_pp", [&]() -> int { return launch_pp<PP_GELU>(h, s0, KC_TEST_GEMM, g); });
  if (rc == MV_OK) {
    hipError_t se = hipMemcpy(out16, dO, (size_t)M * N * 2, hipMemcpyDeviceToHost);
    if (se == hipSuccess && x8 && out8) se = hipMemcpy(out8, dO8, (size_t)M * 2 * N, hipMemcpyDeviceToHost);
    if (se != hipSuccess) rc = fail(h, MV_ERR_HIP, std::string("test gemm_pp copy: ") + hipGetErrorString(se));
  }
  dev_free(h, dA); dev_free(h, dW); dev_free(h, dO); dev_free(h, dB); dev_free(h, dS);
  dev_free(h, dA8); dev_free(h, dW8); dev_free(h, dO8);
  return rc;
} catch (...) { return on_exception(h); }

// host-side e4m3 encoder of the MV_F16X8 weight planes (no GPU needed): tests pin it to the oracle's rounding model
int mv_test_e4m3(const float* in, uint8_t* out, int64_t n) try {
  if (!in || !out || n < 0) return MV_ERR_INVALID;
  for (int64_t i = 0; i < n; ++i) out[i] = f32_to_e4m3_bits(in[i]);
  return MV_OK;
} catch (...) { return on_exception(nullptr); }

}  // extern "C"
