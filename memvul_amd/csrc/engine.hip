// libmemvul_hip.so — C ABI (include/memvul_hip.h) over the gfx950 kernels in this directory.
// Host side: weight staging/packing, workspace ownership, launch sequencing on one HIP stream,
// HIP-event profiling per kernel class, error translation.  No torch, no exceptions across the ABI.
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

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// fp32 -> fp16 bits, round-to-nearest-even (same result as numpy astype(float16))
inline uint16_t f32_to_f16_bits(float f) {
  uint32_t x;
  std::memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u;
  x &= 0x7fffffffu;
  if (x >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | ((x > 0x7f800000u) ? 0x200u : 0));
  if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // rounds to >= 65520 -> inf
  if (x < 0x38800000u) {                                     // subnormal half or zero
    if (x < 0x33000000u) return (uint16_t)sign;              // < 2^-25 -> 0
    const int e = (int)(x >> 23);
    uint32_t m = (x & 0x7fffffu) | 0x800000u;
    const int shift = 126 - e;  // 14..24 -> bits to drop
    const uint32_t half_m = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1), halfway = 1u << (shift - 1);
    uint32_t r = half_m;
    if (rem > halfway || (rem == halfway && (half_m & 1))) r++;
    return (uint16_t)(sign | r);
  }
  const uint32_t e = (x >> 23) - 112, m = x & 0x7fffffu;
  uint32_t h = (e << 10) | (m >> 13);
  const uint32_t rem = m & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (h & 1))) h++;
  return (uint16_t)(sign | h);
}
inline float f16_bits_to_f32(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  uint32_t e = (h >> 10) & 0x1f, m = h & 0x3ffu, x;
  if (e == 0) {
    if (m == 0) x = sign;
    else {
      int sh = 0;
      while (!(m & 0x400u)) { m <<= 1; sh++; }
      m &= 0x3ffu;
      x = sign | ((uint32_t)(113 - sh) << 23) | (m << 13);
    }
  } else if (e == 31) x = sign | 0x7f800000u | (m << 13);
  else x = sign | ((e + 112) << 23) | (m << 13);
  float f;
  std::memcpy(&f, &x, 4);
  return f;
}
inline float bf16_bits_to_f32(uint16_t h) {
  uint32_t x = (uint32_t)h << 16;
  float f;
  std::memcpy(&f, &x, 4);
  return f;
}

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
  int64_t c_row = 0; bool keep_psame = false;    // ... whose row c_row is plan row 0: ids read in place at pitch c_S, results (and P(same)) to its arrays
  Stage out;                                      // host results, plan order (NULL: not asked for; out.ids / out.lens unused)
  bool match = false;                             // + the matcher: the best anchor always, logits / probs where `out` asks for them
  float* u_dev = nullptr;                         // the encoder's output to the device here (mv_anchor_append: the bank; a keeping sweep: c_embed) instead of wk.u
  int topk = 0;                                   // the resident corpus, mv_corpus_keep: the rows' k best anchors to c_topk_p / c_topk_idx as well (0: none)
  int n_layers = -1; bool full = false;           // mv_debug_encode: the layers to run, and the full last layer (encode_dev)
  int G = 0;                                      // the anchors it is matched against: the bank's first G rows (job_form: the count when the job is made)
  bool safe = false;                              // the form of its passes (job_form: from the handle, when the job is made)
  bool guard = false;                             // the guarded form: default-form passes with the per-sequence monitor counts kept (out.over / the corpus' c_over)
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

  // resident corpus
  int32_t *c_ids = nullptr, *c_lens = nullptr;
  std::vector<int32_t> c_lens_host;  // the lengths as uploaded (encode_dev's min_len of each pass)
  std::vector<void*> pinned;
  int64_t c_n = 0;
  int c_S = 0;
  float* c_best = nullptr;
  int32_t* c_idx = nullptr;
  float* c_psame = nullptr;
  int64_t c_psame_rows = 0;
  int c_G = 0;
  // what the corpus keeps of a sweep besides the best anchor (mv_corpus_keep: after an upload, before its first run; allocated at that run): the embeddings, so
  // that mv_corpus_rematch can match them again against a changed bank without the encoder, and the k best anchors of every row
  int c_keep_embed = 0, c_k = 0;
  bool c_ran = false;                   // a run since the upload: mv_corpus_keep comes too late
  float* c_embed = nullptr;             // [c_n][P]
  float* c_topk_p = nullptr;            // [c_n][c_k]
  int32_t* c_topk_idx = nullptr;
  std::vector<uint8_t> c_has;           // [c_n] a keeping run covered the row (empty while nothing is kept)
  // the guarded form on the resident corpus: the sweep records the per-row monitor counts and which rows it ran at which width; rescore_corpus (mv_corpus_results)
  // encodes the flagged ones again
  uint32_t* c_over = nullptr;           // [c_n] AttnArgs::seq_over of the row's last guarded run
  std::vector<int16_t> c_pend_w;        // [c_n] the width (s_eff) of the row's guarded run not yet rescored; 0 = none
  std::vector<uint8_t> c_pend_keep;     // ... and whether that run kept P(same)
  std::vector<uint8_t> c_forms;         // mv_corpus_row_forms
  bool c_pending = false;
  // ... and the sink-token list there: the flags of every corpus row under the current list (route_flags_kernel), recomputed lazily after an upload or a list
  // change; a guarded sweep leaves the routed rows of its range out and marks them forced (rescore_corpus encodes them without looking at c_over)
  uint32_t* route_bm_dev = nullptr;     // the bitmap on the device [ceil(vocab / 32)]
  uint8_t* c_route_dev = nullptr;       // [c_n]
  std::vector<uint8_t> c_route;         // [c_n] on the host
  bool c_route_stale = true;
  std::vector<uint8_t> c_pend_force;    // [c_n] the row's pending run (c_pend_w) left it out: routed
  std::vector<std::vector<int32_t>> c_idx_live;  // index lists of the split batches of sweeps in flight (alive until rescore_corpus has waited for them)

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

  // multi-GPU exchange (mv_comm_*): RCCL entry points resolved from librccl.so at run time
  void* rccl_lib = nullptr;
  ncclComm_t comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  decltype(&ncclGetUniqueId) p_ncclGetUniqueId = nullptr;
  decltype(&ncclCommInitRank) p_ncclCommInitRank = nullptr;
  decltype(&ncclAllGather) p_ncclAllGather = nullptr;
  decltype(&ncclCommDestroy) p_ncclCommDestroy = nullptr;
  decltype(&ncclGetErrorString) p_ncclGetErrorString = nullptr;
  decltype(&ncclGetVersion) p_ncclGetVersion = nullptr;      // optional (mv_comm_info)
  decltype(&ncclCommCount) p_ncclCommCount = nullptr;        // optional
  decltype(&ncclCommUserRank) p_ncclCommUserRank = nullptr;  // optional
  void *comm_send = nullptr, *comm_recv = nullptr;
  int64_t comm_send_cap = 0, comm_recv_cap = 0;
};

namespace {

int fail(mv_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg; else g_create_error = msg;
  return code;
}

// No C++ exception crosses the ABI (include/memvul_hip.h): every entry point is a function-try-block whose handler lands here
// (std::bad_alloc of the host-side staging vectors / maps -> MV_ERR_NOMEM, anything else -> MV_ERR_INTERNAL).
int on_exception(mv_handle* h) noexcept {
  int code = MV_ERR_INTERNAL;
  const char* what = "unknown C++ exception";
  try {
    throw;
  } catch (const std::bad_alloc&) {
    code = MV_ERR_NOMEM;
    what = "out of host memory";
  } catch (const std::exception& e) {
    what = e.what();
  } catch (...) {
  }
  try {
    fail(h, code, std::string("internal: ") + what);
  } catch (...) {  // not even the message could be stored
  }
  return code;
}

#define HIPCHK(h, expr)                                                                             \
  do {                                                                                              \
    hipError_t _e = (expr);                                                                         \
    if (_e != hipSuccess)                                                                           \
      return fail(h, MV_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));                \
  } while (0)

template <typename T>
int dev_alloc(mv_handle* h, hipStream_t stream, T** p, int64_t count, bool zero = true) {
  void* d = nullptr;
  const size_t bytes = (size_t)count * sizeof(T);
  hipError_t e = hipMalloc(&d, bytes ? bytes : 16);
  if (e != hipSuccess) return fail(h, MV_ERR_NOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e));
  if (zero) {
    e = hipMemsetAsync(d, 0, bytes ? bytes : 16, stream);
    if (e != hipSuccess) return fail(h, MV_ERR_HIP, std::string("hipMemset failed: ") + hipGetErrorString(e));
  }
  h->allocs.push_back(d);
  *p = (T*)d;
  return MV_OK;
}
void dev_free(mv_handle* h, void* p) {
  if (!p) return;
  for (auto it = h->allocs.begin(); it != h->allocs.end(); ++it)
    if (*it == p) { h->allocs.erase(it); break; }
  hipFree(p);
}

hipEvent_t get_event(mv_handle* h) {
  if (!h->free_events.empty()) {
    hipEvent_t e = h->free_events.back();
    h->free_events.pop_back();
    return e;
  }
  hipEvent_t e;
  hipEventCreate(&e);
  return e;
}

struct ProfScope {
  mv_handle* h;
  hipStream_t stream;
  ProfRec rec;
  bool on;
  ProfScope(mv_handle* h_, hipStream_t s, int cls) : h(h_), stream(s), on(h_->prof && ((h_->prof_mask >> cls) & 1u)) {
    if (on) {
      rec.cls = cls;
      rec.e0 = get_event(h);
      rec.e1 = get_event(h);
      hipEventRecord(rec.e0, stream);
    }
  }
  ~ProfScope() {
    if (on) {
      hipEventRecord(rec.e1, stream);
      h->recs.push_back(rec);
    }
  }
};

int launch_check(mv_handle* h, const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(h, MV_ERR_HIP, std::string("launch ") + what + ": " + hipGetErrorString(e));
  return MV_OK;
}

int choose_gn(int tn, int gn_max) {
  int g = 1;
  for (int d = 1; d <= gn_max && d <= tn; ++d)
    if (tn % d == 0) g = d;
  return g;
}

template <int EPI>
int launch_gemm128(mv_handle* h, hipStream_t stream, int cls, GemmArgs a) {
  if (a.M % 128 || a.N % 128 || a.K % 64) return fail(h, MV_ERR_INVALID, "gemm128: M,N % 128, K % 64 required");
  a.GN = choose_gn(a.N / 128, 8);
  const int grid = (a.M / 128) * (a.N / 128);
  ProfScope ps(h, stream, cls);
  hipLaunchKernelGGL((gemm128_kernel<EPI>), dim3(grid), dim3(256), G128_LDS_BYTES, stream, a);
  return launch_check(h, "gemm128");
}

// skinny problems (the [CLS] tail of the pruned last layer: M = batch rows): 64 x 64 tiles on a 4-stage LDS ring,
// 4x the workgroups of the 128^2 kernel and a K loop that is DMA-latency-bound per step rather than per tile
constexpr int RING64_LDS = 4 * (64 + 64) * 64 * 2;
template <int EPI>
constexpr auto ring64_kernel = gemm_ring_kernel<EPI, 1, 1, 2, 2, 64, 4, 2>;
template <int EPI>
int launch_ring64(mv_handle* h, hipStream_t stream, int cls, GemmArgs a) {
  if (a.M % 64 || a.N % 64 || a.K % 64) return fail(h, MV_ERR_INVALID, "gemm_ring: shape not a multiple of the 64 x 64 x 64 tile");
  a.GN = choose_gn(a.N / 64, 8);
  const int grid = (a.M / 64) * (a.N / 64);
  ProfScope ps(h, stream, cls);
  hipLaunchKernelGGL(ring64_kernel<EPI>, dim3(grid), dim3(256), RING64_LDS, stream, a);
  return launch_check(h, "gemm_ring");
}

// The persistent ping-pong GEMM (gemm_pp.h): one workgroup per CU walks the 256^2 output tiles.  a.A8 set = the
// MV_F16X8 build (a second, fp8 sweep over [A8 | W8]).
template <int PPEPI, int X8>
constexpr auto pp_kernel = gemm_pp_kernel<PPEPI, PPEPI != PP_RESLN3, X8>;  // (RAW: every kind but the residual one)
template <int PPEPI>
constexpr int pp_lds = PPEPI != PP_RESLN3 ? PP_LDS_BYTES_RAW : PP_LDS_BYTES;
template <int PPEPI>
int launch_pp(mv_handle* h, hipStream_t stream, int cls, GemmArgs a) {
  if (a.M % 256 || a.N % 256 || a.K % 128 || a.K < 256 || a.N > MV_INTER)
    return fail(h, MV_ERR_INVALID, "gemm_pp: M,N % 256, K % 128, K >= 256, N <= 3072 required");  // K >= 256: the RAW kernels stage the
                                                                                              // next tile's statistics at K-tile 2
  if (!a.bias || !a.lnstats) return fail(h, MV_ERR_STATE, "internal: gemm_pp without bias / row statistics");
  // a weight-side-only fp8 sweep walks K / 128 K-tiles IN PAIRS (gemm_pp.h two_ktiles): the staging and consume cursors only stay in
  // step when that count is even
  if (a.A8 && (a.x8_terms == 1 || a.x8_terms == 3) && a.K % 256)
    return fail(h, MV_ERR_INVALID, "gemm_pp: a weight-side-only fp8 correction sweep needs K % 256 == 0");
  a.GN = choose_gn(a.N / 256, h->pp_gn_max);  // widths 2 / 3 / 6 / 12 measured: 4 (or the largest divisor below it) is the fastest
  const int tiles = (a.M / 256) * (a.N / 256);
  const int grid = tiles < h->num_cu ? tiles : h->num_cu;
  // the A-stationary raster (gemm_pp.h raster_pp; MEMVUL_RASTER=1): only where its windows tile the sequence exactly
  a.raster_mode = (h->pp_raster == 1 && a.N / 256 > a.GN && ((a.M / 256) * a.GN) % grid == 0) ? 1 : 0;
  ProfScope ps(h, stream, cls);
  if (a.A8) {
    if (!a.W8 || (PPEPI != PP_QK && !a.out8)) return fail(h, MV_ERR_STATE, "internal: MV_F16X8 GEMM without its fp8 planes");
    hipLaunchKernelGGL((pp_kernel<PPEPI, 1>), dim3(grid), dim3(512), pp_lds<PPEPI>, stream, a);
  } else {
    hipLaunchKernelGGL((pp_kernel<PPEPI, 0>), dim3(grid), dim3(512), pp_lds<PPEPI>, stream, a);
  }
  return launch_check(h, "gemm_pp");
}

// The kernels above that ask for more than 64 KiB of dynamic LDS, with the bytes their launchers pass: mv_create opts every one of them in
struct GemmLdsOptIn { void (*kernel)(GemmArgs); int lds; };
constexpr GemmLdsOptIn GEMM_LDS_OPT_INS[] = {
    {ring64_kernel<EPI_F32>, RING64_LDS},       {ring64_kernel<EPI_QKV>, RING64_LDS},        {ring64_kernel<EPI_GELU>, RING64_LDS},
    {ring64_kernel<EPI_RES>, RING64_LDS},       {pp_kernel<PP_QK, 0>, pp_lds<PP_QK>},        {pp_kernel<PP_GELU, 0>, pp_lds<PP_GELU>},
    {pp_kernel<PP_RESLN3, 0>, pp_lds<PP_RESLN3>}, {pp_kernel<PP_QK, 1>, pp_lds<PP_QK>},      {pp_kernel<PP_GELU, 1>, pp_lds<PP_GELU>},
    {pp_kernel<PP_RESLN3, 1>, pp_lds<PP_RESLN3>},
};

// path choice: the persistent kernels need enough 256^2 tiles to fill the CUs (one workgroup each); both residual GEMMs
// have N = 768 and every K is a multiple of 128, so ONE predicate (on the padded token count) decides the path of a pass
bool pp_selected(const mv_handle* h, int64_t M) {
  if (M % 256) return false;
  if (h->gemm_tile == 128) return false;
  return h->gemm_tile == 512 || h->precise || (M / 256) * (MV_HIDDEN / 256) >= 256;
}

// the mid-size / skinny GEMMs of a pass that does not fill the chip (and of the [CLS] tail)
template <int EPI>
int launch_small(mv_handle* h, hipStream_t stream, int cls, const GemmArgs& a) {
  if (h->gemm_tile == 0 && a.M <= 512 && a.M % 64 == 0 && a.N % 64 == 0) return launch_ring64<EPI>(h, stream, cls, a);
  return launch_gemm128<EPI>(h, stream, cls, a);
}

// K7 + K8: pooler on the [CLS] rows (row_stride floats apart), then the header
int pool_head(mv_handle* h, Work& wk, const float* x, size_t row_stride, int B, float* u_out) {
  const unsigned gx = (unsigned)((B + 31) / 32);
  hipLaunchKernelGGL(dense768_kernel<0>, dim3(gx, MV_HIDDEN / 32), dim3(512), 0, wk.stream, x, row_stride, B, h->WpT, h->bp,
                     MV_HIDDEN, h->P == MV_HIDDEN ? u_out : wk.pooled);
  if (int rc = launch_check(h, "pooler")) return rc;
  if (h->P == MV_HIDDEN) return MV_OK;  // use_header = False: the pooler output is the embedding
  hipLaunchKernelGGL(dense768_kernel<1>, dim3(gx, MV_PROJ / 32), dim3(512), 0, wk.stream, wk.pooled, (size_t)MV_HIDDEN, B, h->WhT,
                     h->bh, MV_PROJ, u_out);
  return launch_check(h, "header");
}

// padded sequence length of a pass: attention_v2 runs 64-key blocks up to 256 and 128-key chunks above
inline int padded_len(int S_in) { return (int)round_up(S_in, S_in <= 256 ? 64 : 128); }

// the two-plane attention (attention_v2.h VLO) serves this pass: the QKV projection wrote the lo planes of Q, K, V^T (encode_dev: the same predicate)
inline bool two_plane_pass(const mv_handle* h, bool x8, bool safe, int Sp) { return x8 && (safe || (h->short_vlo && Sp <= 128)); }

// How a pass of MV_F16X8 runs: its form, and what the concentration monitor keeps of it
struct PassForm {
  bool safe = false;
  bool monitor = true;           // false: the monitor detached (a rescoring pass of the guarded form: a sequence is counted once)
  uint32_t* seq_over = nullptr;  // device [rows of the pass], zeroed by the caller: AttnArgs::seq_over
};

// The attention variants: one row per instantiation of attention_v2_kernel<NKB, NCH, X8, VLO> (padded length = 64 NKB NCH keys, workgroups of 2 NKB waves).
// launch_attention looks its row up by (padded length, x8, two planes); mv_create opts every row in for its dynamic LDS.
//   one plane: the whole key range up to 256 (8 waves and <= 128 KiB LDS per CU decide the resident workgroups); 384 / 512 as chunks of 128 keys per (row,
//     head, 128-query block) through the same ring: 64 score registers per lane, two workgroups of 4 waves per CU, consecutive units of a workgroup are
//     the query blocks of one head (K / V^T from L2);
//   two planes (MV_F16X8: padded length <= 128, the safe form at every length): a 64 / 128 KiB ring = two / one workgroup per CU; above 128 keys chunks
//     through that ring, 192 = 3 chunks of 64 keys (2 waves), 256 / 384 / 512 = 2 / 3 / 4 chunks of 128 (4 waves) — one wave per SIMD either way.
struct AttnVariant {
  int Sp; bool x8, two_plane;  // the key: padded length, MV_F16X8, Q / K / V / P as hi + lo planes
  void (*kernel)(AttnArgs, int);
  int block, lds;              // threads, dynamic LDS bytes
  int wg_per_cu, units;        // resident workgroups per CU (the grid: that many per CU, or one per unit if there are fewer); work units per (row, head)
};
#define MV_ATT_1P(SP, NKB, NCH, WG)                                                                          \
  {SP, false, false, attention_v2_kernel<NKB, NCH, 0>, NKB * 128, ATT2_LDS_BYTES(NKB), WG, NCH},             \
  {SP, true, false, attention_v2_kernel<NKB, NCH, 1>, NKB * 128, ATT2_LDS_BYTES(NKB), WG, NCH}
#define MV_ATT_2P(SP, NKB, NCH, WG) {SP, true, true, attention_v2_kernel<NKB, NCH, 1, 1>, NKB * 128, ATT2_LDS_BYTES_VLO(NKB), WG, NCH}
constexpr AttnVariant ATTN_VARIANTS[] = {
    MV_ATT_1P(64, 1, 1, 4),  MV_ATT_1P(128, 2, 1, 2), MV_ATT_1P(192, 3, 1, 1), MV_ATT_1P(256, 4, 1, 1), MV_ATT_1P(384, 2, 3, 2), MV_ATT_1P(512, 2, 4, 2),
    MV_ATT_2P(64, 1, 1, 2),  MV_ATT_2P(128, 2, 1, 1), MV_ATT_2P(192, 1, 3, 2), MV_ATT_2P(256, 2, 2, 1), MV_ATT_2P(384, 2, 3, 1), MV_ATT_2P(512, 2, 4, 1),
};
#undef MV_ATT_1P
#undef MV_ATT_2P

int launch_attention(mv_handle* h, Work& wk, const int32_t* d_lens, int B, int Sp, bool x8, bool sp_out = false, const PassForm& pf = PassForm()) {
  const bool vlo = two_plane_pass(h, x8, pf.safe, Sp);
  AttnArgs a{wk.q, wk.k, wk.vt, d_lens, wk.ctx, Sp, B, x8 ? wk.ctx8 : nullptr, h->x8_sat, vlo ? wk.vt_lo : nullptr,
             vlo ? wk.q_lo : nullptr, vlo ? wk.k_lo : nullptr,
             (x8 && !vlo) ? wk.vlo_sp : nullptr,     // special rows: V of keys 0, 1 as hi + lo (the two-plane short passes carry every key's lo plane)
             (x8 && pf.monitor) ? h->attn_conc : nullptr,  // concentration monitor (mv_attention_concentration)
             sp_out ? h->cls_min_len : 0,               // [CLS]-row form: no lo8 plane of the context for the sequences that take it
             sp_out ? wk.cls_lo : nullptr,
             (x8 && pf.monitor) ? pf.seq_over : nullptr};
  const AttnVariant* v = nullptr;
  for (const AttnVariant& r : ATTN_VARIANTS)
    if (r.Sp == Sp && r.x8 == x8 && r.two_plane == vlo) v = &r;
  if (!v) return fail(h, MV_ERR_INVALID, "internal: attention at a padded length other than 64 .. 256 / 384 / 512");
  const int units = B * MV_HEADS * v->units, slots = h->num_cu * v->wg_per_cu;
  ProfScope ps(h, wk.stream, KC_ATTENTION);
  hipLaunchKernelGGL(v->kernel, dim3(units < slots ? units : slots), dim3(v->block), v->lds, wk.stream, a, units);
  return launch_check(h, "attention");
}

// ---- MV_F32: the encoder in fp32 (ref_f32.h) ---------------------------------------------------------------------------------------------
template <int ACT>
int launch_gemm_f32(mv_handle* h, hipStream_t stream, int cls, const float* A, const float* W, const float* bias, const float* res, float* C, int M, int N, int K) {
  if (M <= 0 || M % 128 || N <= 0 || N % 128 || K <= 0 || K % 32) return fail(h, MV_ERR_INVALID, "gemm_f32: M,N % 128, K % 32 required");
  if (ACT == RF_ACT_RES && !res) return fail(h, MV_ERR_STATE, "internal: gemm_f32 residual epilogue without a residual");
  ProfScope ps(h, stream, cls);
  hipLaunchKernelGGL((gemm_f32_kernel<ACT>), dim3((unsigned)((M / 128) * (N / 128))), dim3(256), 0, stream, A, W, bias, res, C, M, N, K);
  return launch_check(h, "gemm_f32");
}

// One pass in the reference form: the small-pass structure (fp32 stream xres, explicit LayerNorm kernels, natural token order) with every GEMM and the
// attention in fp32.  No last-layer pruning in this dtype (1/12 of the time of a form that is not run for throughput; one code path): after the last layer
// xres holds the normalised stream of every token, which is also what the debug taps read.
int encode_f32_dev(mv_handle* h, Work& wk, const int32_t* d_ids, const int32_t* d_lens, int B, int S_in, int n_layers, float* u_out, int pitch) {
  const mv_config& c = h->cfg;
  const int Sp = padded_len(S_in);
  const int64_t M = (int64_t)B * Sp, Mpad = round_up(M, 256);
  if (S_in > c.max_pos) return fail(h, MV_ERR_INVALID, "sequence longer than max_pos");
  if (Mpad > h->cap_tokens) return fail(h, MV_ERR_CAPACITY, "B*S exceeds mv_config.max_tokens");
  if (n_layers < 0 || n_layers > c.layers) n_layers = c.layers;
  h->dbg_B = B;
  h->dbg_Sp = Sp;
  {
    ProfScope ps(h, wk.stream, KC_EMBED_LN);
    hipLaunchKernelGGL(embed_ln_kernel<false>, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, wk.stream, d_ids, pitch, S_in, Sp, (int)M, c.vocab_size,
                       h->wemb, h->pemb, h->temb, h->embg, h->embb, c.ln_eps, wk.xres, wk.x16, (float*)nullptr,
                       (half_t*)nullptr, (uint8_t*)nullptr, (unsigned long long*)nullptr);
    if (int rc = launch_check(h, "embed_ln")) return rc;
  }
  auto run_ln = [&](const float* g, const float* b) -> int {  // all Mpad rows: the rows past M take the residual GEMMs' output like any other and must stay bounded
    ProfScope ps(h, wk.stream, KC_LN);
    hipLaunchKernelGGL(ln_kernel<true>, dim3((unsigned)(Mpad / 4)), dim3(256), 0, wk.stream, wk.xres, wk.x16, (int)Mpad, g, b, c.ln_eps, (float*)nullptr);
    return launch_check(h, "layernorm");
  };
  const int Mp = (int)Mpad, H = MV_HIDDEN, I = MV_INTER;
  for (int l = 0; l < n_layers; ++l) {
    const LayerW& w = h->L[l];
    if (int rc = launch_gemm_f32<RF_ACT_NONE>(h, wk.stream, KC_GEMM_QKV, wk.xres, w.wqkv32, w.bqkv, nullptr, wk.qkv32, Mp, 3 * H, H)) return rc;
    {
      ProfScope ps(h, wk.stream, KC_ATTENTION);
      const int units = B * MV_HEADS * (Sp / 32);
      hipLaunchKernelGGL(attention_f32_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, wk.stream, (const float*)wk.qkv32, d_lens, wk.ctx32, Sp, units);
      if (int rc = launch_check(h, "attention_f32")) return rc;
    }
    if (int rc = launch_gemm_f32<RF_ACT_RES>(h, wk.stream, KC_GEMM_OUT, wk.ctx32, w.wo32, w.bo, wk.xres, wk.xres, Mp, H, H)) return rc;
    if (int rc = run_ln(w.ln1g, w.ln1b)) return rc;
    if (int rc = launch_gemm_f32<RF_ACT_GELU>(h, wk.stream, KC_GEMM_FFN1, wk.xres, w.w132, w.b1, nullptr, wk.h32, Mp, I, H)) return rc;
    if (int rc = launch_gemm_f32<RF_ACT_RES>(h, wk.stream, KC_GEMM_FFN2, wk.h32, w.w232, w.b2, wk.xres, wk.xres, Mp, H, I)) return rc;
    if (int rc = run_ln(w.ln2g, w.ln2b)) return rc;
  }
  if (u_out) {
    ProfScope ps(h, wk.stream, KC_POOL_HEAD);
    if (int rc = pool_head(h, wk, wk.xres, (size_t)Sp * MV_HIDDEN, B, u_out)) return rc;
  }
  return MV_OK;
}

// ---- encoder: ids (device) -> u (device, [B][512]); stops after n_layers (<0: all) ------------
// Two paths, chosen by the size of the pass (pp_selected):
//   * bench scale: the persistent GEMMs on the two-plane raw stream with the virtual LayerNorm (gemm_pp.h), five launches per
//     layer; compute dtype MV_F16X8 adds the fp8 correction sweep to each GEMM and the [lo8 | hi8] planes to each producer;
//   * small passes: one-tile-per-workgroup GEMMs (gemm.h) on an fp32 stream with explicit LayerNorm kernels.
// The last layer is pruned to the [CLS] rows when the pooler follows (cls_prune); `full` (debug taps) disables that and
// leaves the normalised fp32 stream of the last layer run in xres.
// One pass: its shape and every decision about it, taken once (encode_dev) and read by the launches below.
struct PassPlan {
  int B, S_in, Sp, pitch;  // pitch: ints between the rows of d_ids
  int64_t M, Mpad;
  bool big;    // persistent GEMMs, raw stream as hi + a low part (x16 = hi; MV_F16: xlo, MV_F16X8: the lo8 plane of x8 + st_lo), virtual LayerNorm
  bool x8;     // MV_F16X8: + fp8 correction sweeps (forces the persistent path, pp_selected)
  bool safe;   // (the form of the planned job, read from the handle when the job was made: work in flight keeps the form it was enqueued with)
  bool prune;  // the last layer on the [CLS] rows only
  // The [CLS]-row form (mv_handle::cls_aside): every persistent GEMM of this pass sweeps the weight-side correction term only (x8_terms = 1) and the
  // A-side term A_lo W_hi^T is formed for the B [CLS] rows alone: their low parts (2^11 x, fp16) gathered from the operand's lo plane (raw stream) or
  // lo8 plane (context, GELU output), one skinny fp16 GEMM [B x K] x [K x N], and the launch adds the result to those rows' accumulators
  // (gemm_pp.h GemmArgs::cls_corr).  Passes of padded length 256 / 512: a 256-row tile then belongs to ONE sequence, so the form of a sequence
  // depends on its own length alone (cls_tile_flags_kernel: sequences shorter than cls_min_len keep the both-terms form, tile by tile) and a row's
  // result stays independent of the batch it travels in.  Passes of padded length 192 / 384 (a tile there spans two sequences, a per-tile rule would mix the
  // forms inside a sequence): the form for the WHOLE pass when its shortest sequence has cls_min_len tokens — what a length-sorted sweep hands over by
  // construction (ModelMemory.sweep / Engine.bucketed_sweep: a pass at 192 holds 129 .. 192 tokens, at 384 257 .. 384) — else the both-terms form for the whole pass.
  bool cls_as, one_seq_tiles;
  // Special rows (round 6): rows 0 and 1 of every sequence hold its [CLS] and its [SEP] token (embed_ln_kernel swaps the last token into row 1) — the token the
  // pooler reads and the two tokens trained BERT heads use as attention sinks, i.e. the rows whose roundings can reach the pooler un-averaged.  For them every
  // GEMM whose sweep carried the weight-side term only gets the A-side term from a skinny GEMM over the 2 B compact rows the PRODUCER's epilogue left in cls_lo
  // (no gather launch), and attention adds p[:, 0..1] V_lo[0..1].  The K and V blocks of the QKV projection take it in every pass of this compute dtype (they
  // never sweep the A-side term for all rows by default), the other three GEMMs where the [CLS]-row form is in force.
  bool special;
  bool two_plane;  // Q, K, V^T as hi + lo planes (two_plane_pass: launch_attention asks the same predicate)
  int qkv_mask;    // GemmArgs::x8_aside_mask of the QKV projection
};

// what every GEMM of the layer stack is given, whatever its kind
GemmArgs pass_gemm(const mv_handle* h, const Work& wk, const PassPlan& p) {
  GemmArgs g{};
  g.M = (int)p.Mpad; g.Mreal = (int)p.M; g.S = p.Sp; g.ln_eps = h->cfg.ln_eps; g.x8_sat = h->x8_sat;
  g.tile_both = (p.cls_as && p.one_seq_tiles) ? wk.tile_both : nullptr;  // (the whole-pass form: no tile is short)
  return g;
}

// The row term of the launch `g` is being built for: cls_corr [2 B][N] = A [2 B][K] W^T (both 2^11 x), A = st_lo (stream) or cls_lo (context, GELU output)
int row_term(mv_handle* h, Work& wk, const PassPlan& p, const half_t* A, GemmArgs& g) {
  GemmArgs t{};
  t.M = (int)round_up(2 * p.B, 64); t.Mreal = 2 * p.B; t.S = 64; t.A = A; t.W = g.W; t.N = g.N; t.K = g.K; t.outf = wk.cls_corr;
  g.cls_corr = wk.cls_corr;
  return launch_ring64<EPI_F32>(h, wk.stream, KC_CLS_ROW_TERM, t);
}

// V of the special rows as hi + lo, for the attention that follows (a two-plane pass carries every key's lo plane instead)
inline half_t* special_v_lo(const Work& wk, const PassPlan& p) { return (p.special && !p.two_plane) ? wk.vlo_sp : nullptr; }

// K2: Q, K, V^T projection of the stream (persistent path: the raw stream, LayerNorm folded into W'' / b').  kv_only: the K and V blocks alone (the pruned last layer)
int launch_qkv(mv_handle* h, Work& wk, const PassPlan& p, const LayerW& w, bool kv_only) {
  const size_t col0 = kv_only ? MV_HIDDEN : 0;  // first packed-QKV column of the launch
  const int cls = kv_only ? KC_GEMM_KV_LAST : KC_GEMM_QKV;
  GemmArgs g = pass_gemm(h, wk, p);
  g.A = wk.x16; g.W = (p.big ? w.wqkv_f : w.wqkv) + col0 * MV_HIDDEN; g.bias = (p.big ? w.bqkv_f : w.bqkv) + col0;
  g.N = 3 * MV_HIDDEN - (int)col0; g.K = MV_HIDDEN; g.col0 = (int)col0;
  g.q = wk.q; g.k = wk.k; g.vt = wk.vt;
  if (!p.big) return launch_small<EPI_QKV>(h, wk.stream, cls, g);
  g.lnstats = wk.lnstats;
  if (p.x8) { g.A8 = wk.x8; g.W8 = w.wqkv_f8 + col0 * 2 * MV_HIDDEN; g.x8_scale = w.sc_qkv; g.x8_terms = 3; g.x8_aside_mask = p.qkv_mask; }
  // Q, K, V^T as hi + lo planes: wherever the two-plane attention follows; of the pruned layer only in the safe form, whose single-query attention reads K and
  // V as hi + lo (the [CLS] query itself is fp32: cls_tail_f32)
  if (kv_only ? p.safe : p.two_plane) { g.vt_lo = wk.vt_lo; g.q_lo = wk.q_lo; g.k_lo = wk.k_lo; }
  // x8_terms stays 3 — a block of x8_aside_mask (Q by default) keeps its A-side term for EVERY row; the other blocks take it for the special rows from
  // the row term (the launch skips it in blocks that swept both terms: gemm_pp.h).  With diffuse attention K and V of one token are one key among S for
  // every query and the term buys nothing (round 5: model, four draws); with an attention sink on that token they reach every row un-averaged.
  if (p.special) {
    const int blocks = kv_only ? 6 : 7;  // the Q / K / V blocks of this launch, as bits of x8_aside_mask
    if ((p.qkv_mask & blocks) != blocks) { if (int rc = row_term(h, wk, p, wk.st_lo, g)) return rc; }
    g.vlo_sp = special_v_lo(wk, p);
  }
  return launch_pp<PP_QK>(h, wk.stream, cls, g);
}

// The fields of the two residual GEMMs of the persistent path (K4, K6: N = 768, in place on the raw stream): + bias + LayerNorm(residual) with gamma / beta of
// the LayerNorm pending on the stream, whose statistics lie in `stats`; the vstats of the new rows go to `stats_out`
void residual_fields(const Work& wk, const PassPlan& p, GemmArgs& g, const float* stats, float* stats_out, const float* gamma, const float* beta) {
  g.lnstats = stats; g.lng = gamma; g.lnb = beta; g.lnpart = stats_out; g.out16 = wk.x16; g.out16b = wk.xlo;
  if (p.x8) { g.out8 = wk.x8; g.x8_terms = p.cls_as ? 1 : 2; }
  // [CLS]-row form: out8_hi_only stays 0 — the consumers sweep the weight-side term only (the next QKV projection's Q block apart), but the lo8 plane IS the
  // stream's low part: the next residual GEMM reads it back (gemm.h GemmArgs::out16b).  special: the stream rows' special low parts, read back and rewritten in
  // place — the operand of the row terms of FFN-1 and of the next QKV projection, in every pass of this compute dtype
  if (p.special) g.sp_lo_out = wk.st_lo;
}

// K4: attention output projection + bias + LayerNorm(residual), in place on the stream; persistent path: + vstats of the new rows (wk.lnpart)
int launch_out_proj(mv_handle* h, Work& wk, const PassPlan& p, const LayerW& w, const float* pend_g, const float* pend_b) {
  GemmArgs g = pass_gemm(h, wk, p);
  g.A = wk.ctx; g.W = w.wo; g.bias = w.bo; g.N = MV_HIDDEN; g.K = MV_HIDDEN;
  if (!p.big) { g.xres = wk.xres; return launch_small<EPI_RES>(h, wk.stream, KC_GEMM_OUT, g); }
  residual_fields(wk, p, g, wk.lnstats, wk.lnpart, pend_g, pend_b);
  if (p.x8) { g.A8 = wk.ctx8; g.W8 = w.wo8; g.x8_scale = w.sc_o; }
  if (p.cls_as) { if (int rc = row_term(h, wk, p, wk.cls_lo, g)) return rc; }  // (the context's special low parts: launch_attention)
  return launch_pp<PP_RESLN3>(h, wk.stream, KC_GEMM_OUT, g);
}

// K5: FFN-1 + exact-erf GELU
int launch_ffn1(mv_handle* h, Work& wk, const PassPlan& p, const LayerW& w) {
  GemmArgs g = pass_gemm(h, wk, p);
  g.A = wk.x16; g.N = MV_INTER; g.K = MV_HIDDEN; g.out16 = wk.h16;
  if (!p.big) { g.W = w.w1; g.bias = w.b1; return launch_small<EPI_GELU>(h, wk.stream, KC_GEMM_FFN1, g); }
  g.W = w.w1_f; g.bias = w.b1_f; g.lnstats = wk.lnpart;
  if (p.x8) { g.A8 = wk.x8; g.W8 = w.w1_f8; g.x8_scale = w.sc_1; g.out8 = wk.h8; g.x8_terms = p.cls_as ? 1 : 2; }
  if (p.cls_as) {
    if (int rc = row_term(h, wk, p, wk.st_lo, g)) return rc;
    g.out8_hi_only = 1;       // h8 is FFN-2's A8: hi8 alone
    g.sp_lo_out = wk.cls_lo;  // the GELU output's special low parts: FFN-2's row term
  }
  return launch_pp<PP_GELU>(h, wk.stream, KC_GEMM_FFN1, g);
}

// K6: FFN-2 + bias + LayerNorm(residual); persistent path: + vstats of the new rows (wk.lnstats: the next layer's input)
int launch_ffn2(mv_handle* h, Work& wk, const PassPlan& p, const LayerW& w) {
  GemmArgs g = pass_gemm(h, wk, p);
  g.A = wk.h16; g.W = w.w2; g.bias = w.b2; g.N = MV_HIDDEN; g.K = MV_INTER;
  if (!p.big) { g.xres = wk.xres; return launch_small<EPI_RES>(h, wk.stream, KC_GEMM_FFN2, g); }
  residual_fields(wk, p, g, wk.lnpart, wk.lnstats, w.ln1g, w.ln1b);
  if (p.x8) { g.A8 = wk.h8; g.W8 = w.w28; g.x8_scale = w.sc_2; }
  if (p.cls_as) { if (int rc = row_term(h, wk, p, wk.cls_lo, g)) return rc; }
  return launch_pp<PP_RESLN3>(h, wk.stream, KC_GEMM_FFN2, g);
}

int run_ln(mv_handle* h, Work& wk, float* x32, half_t* x16, int rows, const float* g, const float* b) {
  ProfScope ps(h, wk.stream, KC_LN);
  hipLaunchKernelGGL(ln_kernel<true>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, wk.stream, x32, x16, rows, g, b, h->cfg.ln_eps, (float*)nullptr);
  return launch_check(h, "layernorm");
}

// persistent path: two-plane raw stream -> normalised fp32 rows (pooler / debug taps)
int final_ln(mv_handle* h, Work& wk, const PassPlan& p, const float* g, const float* b) {
  const size_t n4 = (size_t)p.M * MV_HIDDEN / 4;
  hipLaunchKernelGGL(hilo_to_f32_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, wk.stream, wk.x16, wk.xlo, n4, wk.xres,
                     p.special ? (const half_t*)wk.st_lo : (const half_t*)nullptr, p.Sp, (const uint8_t*)wk.x8);
  if (int rc = launch_check(h, "hilo_to_f32")) return rc;
  return run_ln(h, wk, wk.xres, wk.x16, (int)p.M, g, b);
}

// A layer of the persistent path: five launches (+ the row terms; + the sink census).  pend_g / pend_b: gamma / beta of the LayerNorm whose statistics are
// pending in wk.lnstats (the embedding's, or the previous layer's second one) — the output projection applies it; wk.lnstats = vstats of the layer's input
// rows, wk.lnpart = of the rows after the output projection; no statistics kernel in between (gemm_pp.h)
int persistent_layer(mv_handle* h, Work& wk, const PassPlan& p, const PassForm& pf, int l, const int32_t* d_ids, const int32_t* d_lens, const float* pend_g, const float* pend_b) {
  const LayerW& w = h->L[l];
  if (int rc = launch_qkv(h, wk, p, w, false)) return rc;
  // the sink census: the layers whose attention launch feeds the concentration monitor, and only where it is attached (a rescoring pass counts nothing twice)
  if (h->census && p.x8 && pf.monitor) {
    ProfScope ps(h, wk.stream, KC_ATTENTION);
    hipLaunchKernelGGL(sink_census_kernel, dim3((unsigned)((p.B * MV_HEADS + 3) / 4)), dim3(256), 0, wk.stream, (const half_t*)wk.q, (const half_t*)wk.k, d_lens,
                       d_ids, p.pitch, p.S_in, p.Sp, p.B * MV_HEADS, h->cfg.vocab_size, h->census_items, h->census_share, h->census_heads + (size_t)l * MV_HEADS);
    if (int rc = launch_check(h, "sink_census")) return rc;
  }
  // K3: attention (cls_as: + the context's special rows' low parts for the output projection's row term)
  if (int rc = launch_attention(h, wk, d_lens, p.B, p.Sp, p.x8, p.cls_as, pf)) return rc;
  if (int rc = launch_out_proj(h, wk, p, w, pend_g, pend_b)) return rc;
  if (int rc = launch_ffn1(h, wk, p, w)) return rc;
  return launch_ffn2(h, wk, p, w);
}

// A layer of a small pass: fp32 stream, explicit LayerNorm kernels, one-plane MV_F16 attention
int small_layer(mv_handle* h, Work& wk, const PassPlan& p, const LayerW& w, const int32_t* d_lens) {
  if (int rc = launch_qkv(h, wk, p, w, false)) return rc;
  if (int rc = launch_attention(h, wk, d_lens, p.B, p.Sp, false)) return rc;
  if (int rc = launch_out_proj(h, wk, p, w, nullptr, nullptr)) return rc;
  if (int rc = run_ln(h, wk, wk.xres, wk.x16, (int)p.M, w.ln1g, w.ln1b)) return rc;
  if (int rc = launch_ffn1(h, wk, p, w)) return rc;
  if (int rc = launch_ffn2(h, wk, p, w)) return rc;
  return run_ln(h, wk, wk.xres, wk.x16, (int)p.M, w.ln2g, w.ln2b);
}

// MV_F16X8: the B [CLS] rows in full fp32 on the fp32-input matrix cores (their operand rounding would reach the pooler un-attenuated): Q projection,
// single-query attention (fp16 K / V^T of the main path, fp32 context), output projection + residual, LayerNorm, FFN, LayerNorm
int cls_tail_f32(mv_handle* h, Work& wk, const PassPlan& p, const LayerW& w, const int32_t* d_lens, float* u_out) {
  const int B = p.B;
  const unsigned gx = (unsigned)((B + 31) / 32);
  hipLaunchKernelGGL((dense768_kernel<2, MV_HIDDEN>), dim3(gx, MV_HIDDEN / 32), dim3(512), 0, wk.stream, (const float*)wk.c32,
                     (size_t)MV_HIDDEN, B, (const float*)w.wqT32, (const float*)w.bqkv, MV_HIDDEN, wk.cq, (const float*)nullptr);
  if (int rc = launch_check(h, "cls q")) return rc;
  const half_t* vlo_sp = special_v_lo(wk, p);
  if (p.safe)
    hipLaunchKernelGGL(attention_cls_kernel<true>, dim3((B * MV_HEADS + 3) / 4), dim3(256), 0, wk.stream, wk.cq, wk.k, wk.vt, d_lens, wk.cctx, p.Sp,
                       B * MV_HEADS, wk.pooled, vlo_sp, (const half_t*)wk.k_lo, (const half_t*)wk.vt_lo);
  else
    hipLaunchKernelGGL(attention_cls_kernel<false>, dim3((B * MV_HEADS + 3) / 4), dim3(256), 0, wk.stream, wk.cq, wk.k, wk.vt, d_lens, wk.cctx, p.Sp,
                       B * MV_HEADS, wk.pooled, vlo_sp, (const half_t*)nullptr, (const half_t*)nullptr);
  if (int rc = launch_check(h, "attention_cls")) return rc;
  hipLaunchKernelGGL((dense768_kernel<4, MV_HIDDEN>), dim3(gx, MV_HIDDEN / 32), dim3(512), 0, wk.stream, (const float*)wk.pooled,
                     (size_t)MV_HIDDEN, B, (const float*)w.woT32, (const float*)w.bo, MV_HIDDEN, wk.c32, (const float*)wk.c32);
  if (int rc = launch_check(h, "cls out")) return rc;
  if (int rc = run_ln(h, wk, wk.c32, wk.c16, B, w.ln1g, w.ln1b)) return rc;
  hipLaunchKernelGGL((dense768_kernel<3, MV_HIDDEN>), dim3(gx, MV_INTER / 32), dim3(512), 0, wk.stream, (const float*)wk.c32,
                     (size_t)MV_HIDDEN, B, (const float*)w.w1T32, (const float*)w.b1, MV_INTER, wk.ch32, (const float*)nullptr);
  if (int rc = launch_check(h, "cls ffn1")) return rc;
  hipLaunchKernelGGL((dense768_kernel<4, MV_INTER>), dim3(gx, MV_HIDDEN / 32), dim3(512), 0, wk.stream, (const float*)wk.ch32,
                     (size_t)MV_INTER, B, (const float*)w.w2T32, (const float*)w.b2, MV_HIDDEN, wk.c32, (const float*)wk.c32);
  if (int rc = launch_check(h, "cls ffn2")) return rc;
  if (int rc = run_ln(h, wk, wk.c32, wk.c16, B, w.ln2g, w.ln2b)) return rc;
  return pool_head(h, wk, wk.c32, MV_HIDDEN, B, u_out);
}

// MV_F16: the same tail as fp16 skinny GEMMs on an fp32 stream of B rows
int cls_tail_f16(mv_handle* h, Work& wk, const PassPlan& p, const LayerW& w, const int32_t* d_lens, float* u_out) {
  const int B = p.B;
  auto skinny = [&](const half_t* A, const half_t* W, const float* bias, int N, int K) {
    GemmArgs t{};
    t.M = (int)round_up(B, 128); t.Mreal = B; t.S = 64; t.A = A; t.W = W; t.bias = bias; t.N = N; t.K = K;
    return t;
  };
  GemmArgs q = skinny(wk.c16, w.wqkv, w.bqkv, MV_HIDDEN, MV_HIDDEN);
  q.outf = wk.cq;
  if (int rc = launch_small<EPI_F32>(h, wk.stream, KC_CLS_TAIL, q)) return rc;
  hipLaunchKernelGGL(attention_cls_kernel<false>, dim3((B * MV_HEADS + 3) / 4), dim3(256), 0, wk.stream, wk.cq, wk.k, wk.vt,
                     d_lens, wk.cctx, p.Sp, B * MV_HEADS, (float*)nullptr, (const half_t*)nullptr, (const half_t*)nullptr, (const half_t*)nullptr);
  if (int rc = launch_check(h, "attention_cls")) return rc;
  GemmArgs o = skinny(wk.cctx, w.wo, w.bo, MV_HIDDEN, MV_HIDDEN);
  o.xres = wk.c32;
  if (int rc = launch_small<EPI_RES>(h, wk.stream, KC_CLS_TAIL, o)) return rc;
  if (int rc = run_ln(h, wk, wk.c32, wk.c16, B, w.ln1g, w.ln1b)) return rc;
  GemmArgs f1 = skinny(wk.c16, w.w1, w.b1, MV_INTER, MV_HIDDEN);
  f1.out16 = wk.ch16;
  if (int rc = launch_small<EPI_GELU>(h, wk.stream, KC_CLS_TAIL, f1)) return rc;
  GemmArgs f2 = skinny(wk.ch16, w.w2, w.b2, MV_HIDDEN, MV_INTER);
  f2.xres = wk.c32;
  if (int rc = launch_small<EPI_RES>(h, wk.stream, KC_CLS_TAIL, f2)) return rc;
  if (int rc = run_ln(h, wk, wk.c32, wk.c16, B, w.ln2g, w.ln2b)) return rc;
  return pool_head(h, wk, wk.c32, MV_HIDDEN, B, u_out);
}

// The last layer on the [CLS] rows only: K and V of every token, everything else on B rows, down to the embedding
int pruned_last_layer(mv_handle* h, Work& wk, const PassPlan& p, const LayerW& w, const int32_t* d_lens, const float* pend_g, const float* pend_b, float* u_out) {
  if (int rc = launch_qkv(h, wk, p, w, true)) return rc;
  ProfScope tail(h, wk.stream, KC_CLS_TAIL);
  struct Restore { mv_handle* h; uint32_t mask; ~Restore() { h->prof_mask = mask; } } restore{h, h->prof_mask};  // (on every return)
  h->prof_mask = 0;  // the tail is one profiled span; its inner launches carry no events of their own
  hipLaunchKernelGGL(cls_gather_kernel, dim3((p.B + 3) / 4), dim3(256), 0, wk.stream, wk.xres, wk.x16, p.Sp, p.B,
                     p.big ? (const float*)wk.lnstats : (const float*)nullptr, pend_g, pend_b, wk.c32, wk.c16, p.big ? 1 : 0,
                     (p.big && !p.x8) ? wk.xlo : (const half_t*)nullptr, p.big ? 1 : 0, h->cfg.ln_eps,
                     p.special ? (const half_t*)wk.st_lo : (const half_t*)nullptr);
  if (int rc = launch_check(h, "cls_gather")) return rc;
  return p.x8 ? cls_tail_f32(h, wk, p, w, d_lens, u_out) : cls_tail_f16(h, wk, p, w, d_lens, u_out);
}

int encode_dev(mv_handle* h, Work& wk, const int32_t* d_ids, const int32_t* d_lens, int min_len, int B, int S_in, int n_layers, float* u_out,
               const PassForm& pf = PassForm(), bool full = false, int pitch = 0) {  // min_len: the shortest sequence of the pass as the HOST knows it (Pass::min_len; 0 = unknown)
  if (pitch <= 0) pitch = S_in;
  if (h->f32) return encode_f32_dev(h, wk, d_ids, d_lens, B, S_in, n_layers, u_out, pitch);  // MV_F32: no forms, no monitors, no pruning
  const mv_config& c = h->cfg;
  PassPlan p{};
  p.B = B; p.S_in = S_in; p.Sp = padded_len(S_in); p.pitch = pitch;
  p.M = (int64_t)B * p.Sp; p.Mpad = round_up(p.M, 256);
  if (S_in > c.max_pos) return fail(h, MV_ERR_INVALID, "sequence longer than max_pos");
  if (p.Mpad > h->cap_tokens) return fail(h, MV_ERR_CAPACITY, "B*S exceeds mv_config.max_tokens");
  if (n_layers < 0 || n_layers > c.layers) n_layers = c.layers;
  h->dbg_B = B;
  h->dbg_Sp = p.Sp;
  p.big = pp_selected(h, p.Mpad);
  p.x8 = h->precise;
  p.safe = p.x8 && pf.safe;
  p.prune = !full && h->cls_prune && u_out && n_layers == c.layers && n_layers > 0;
  p.one_seq_tiles = p.Sp == 256 || p.Sp == 512;
  const bool whole_pass = (p.Sp == 192 || p.Sp == 384) && min_len >= h->cls_min_len;
  p.cls_as = p.big && p.x8 && !p.safe && h->cls_aside && (p.one_seq_tiles || whole_pass);
  p.special = p.big && p.x8;
  p.two_plane = two_plane_pass(h, p.x8, p.safe, p.Sp);
  p.qkv_mask = p.safe ? 7 : h->qkv_aside_mask;
  const int M = (int)p.M, Sp = p.Sp, ntile = (int)(p.Mpad / 256);
  if (p.cls_as && p.one_seq_tiles) {
    hipLaunchKernelGGL(cls_tile_flags_kernel, dim3((unsigned)((ntile + 255) / 256)), dim3(256), 0, wk.stream, d_lens, B, Sp, h->cls_min_len, ntile,
                       wk.tile_both);
    if (int rc = launch_check(h, "cls_tile_flags")) return rc;
  }
  {
    ProfScope ps(h, wk.stream, KC_EMBED_LN);
    const unsigned ln_grid = (unsigned)((M + 3) / 4);
    if (p.big)
      hipLaunchKernelGGL(embed_ln_kernel<true>, dim3(ln_grid), dim3(256), 0, wk.stream, d_ids, pitch, S_in, Sp, M, c.vocab_size,
                         h->wemb, h->pemb, h->temb, h->embg, h->embb, c.ln_eps, wk.xres, wk.x16, wk.lnstats,
                         p.x8 ? (half_t*)nullptr : wk.xlo, p.x8 ? wk.x8 : (uint8_t*)nullptr, h->x8_sat, p.special ? d_lens : (const int32_t*)nullptr,
                         p.special ? wk.st_lo : (half_t*)nullptr);
    else
      hipLaunchKernelGGL(embed_ln_kernel<false>, dim3(ln_grid), dim3(256), 0, wk.stream, d_ids, pitch, S_in, Sp, M, c.vocab_size,
                         h->wemb, h->pemb, h->temb, h->embg, h->embb, c.ln_eps, wk.xres, wk.x16, (float*)nullptr,
                         (half_t*)nullptr, (uint8_t*)nullptr, (unsigned long long*)nullptr);
    if (int rc = launch_check(h, "embed_ln")) return rc;
  }
  // persistent path: the LayerNorm whose statistics are pending in the vstats buffers — gamma / beta the next residual GEMM applies
  const float *pend_g = h->embg, *pend_b = h->embb;
  if (p.big && n_layers == 0) { if (int rc = final_ln(h, wk, p, pend_g, pend_b)) return rc; }
  for (int l = 0; l < n_layers; ++l) {
    const LayerW& w = h->L[l];
    const bool last = (l == n_layers - 1);
    if (last && p.prune) return pruned_last_layer(h, wk, p, w, d_lens, pend_g, pend_b, u_out);
    if (int rc = p.big ? persistent_layer(h, wk, p, pf, l, d_ids, d_lens, pend_g, pend_b) : small_layer(h, wk, p, w, d_lens)) return rc;
    if (!p.big) continue;
    pend_g = w.ln2g; pend_b = w.ln2b;
    if (last) { if (int rc = final_ln(h, wk, p, pend_g, pend_b)) return rc; }  // the pooler reads a normalised stream
  }
  if (u_out) {
    ProfScope ps(h, wk.stream, KC_POOL_HEAD);
    if (int rc = pool_head(h, wk, wk.xres, (size_t)Sp * MV_HIDDEN, B, u_out)) return rc;
  }
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

// largest batch one encoder pass can take at padded length Sp
int max_rows_for(mv_handle* h, int S_in) {
  const int Sp = padded_len(S_in);
  int64_t r = (h->cap_tokens - 256) / Sp;
  if (r > h->cfg.max_batch) r = h->cfg.max_batch;
  return (int)r;
}

// K9 + K10 fused (match_topk.h): logits / probs / psame_out are optional full outputs; k >= 1 selects the best anchor
// (and, with topk_p / topk_idx, the k best).  g_first: against anchors [g_first, g_first + G) of the bank instead of its first G.  4 issue reports per workgroup when that already fills the chip, else 1
// (the same bits either way).
int match_dev(mv_handle* h, Work& wk, const float* u_dev, int B, int G, float* logits, float* probs, float* psame_out, int k, float* best_out,
              int32_t* idx_out, float* topk_p = nullptr, int32_t* topk_idx = nullptr, int g_first = 0) {
  const float* anchors = h->anchors + (size_t)g_first * h->P;  // mv_corpus_rematch, appended mode: the G anchors from g_first on (indices relative to it)
  if (G <= 0) return fail(h, MV_ERR_STATE, "anchor bank is empty (call mv_anchor_append / mv_anchor_set first)");
  MatchArgs a{};
  a.B = B; a.G = G; a.same_idx = h->cfg.same_idx; a.k = k;
  const bool small = G <= 128;                      // one 128-anchor chunk per workgroup (the pass is latency-bound at this size)
  const int GC = small ? 128 : 256;
  a.nchunk = (G + GC - 1) / GC;
  if ((int64_t)a.nchunk * k > 1024) return fail(h, MV_ERR_INVALID, "top-k: anchors / 256 * k must not exceed 1024");
  a.logits = logits; a.probs = probs; a.psame = psame_out;
  a.best = best_out; a.best_idx = idx_out; a.topk_p = topk_p; a.topk_idx = topk_idx;
  a.part_p = wk.part_p; a.part_q = wk.part_q; a.part_i = wk.part_i;
  {
    ProfScope ps(h, wk.stream, KC_MATCH);
    const dim3 grid(small ? 1 : a.nchunk, (B + 3) / 4);
#define MV_MATCH(PD)                                                                                                                          \
    if (small && a.logits) hipLaunchKernelGGL((match_topk_kernel<2, 128, 64, 1, 2, PD>), grid, dim3(256), 0, wk.stream, u_dev, anchors, h->Wm, a); \
    else if (small) hipLaunchKernelGGL((match_topk_kernel<2, 128, 64, 0, 2, PD>), grid, dim3(256), 0, wk.stream, u_dev, anchors, h->Wm, a);        \
    else if (a.logits) hipLaunchKernelGGL((match_topk_kernel<2, 256, 32, 1, 2, PD>), grid, dim3(512), 0, wk.stream, u_dev, anchors, h->Wm, a);     \
    else hipLaunchKernelGGL((match_topk_kernel<2, 256, 32, 0, 2, PD>), grid, dim3(512), 0, wk.stream, u_dev, anchors, h->Wm, a)
    if (h->P == MV_PROJ) { MV_MATCH(MV_PROJ); } else { MV_MATCH(MV_HIDDEN); }
#undef MV_MATCH
    if (int rc = launch_check(h, "match_topk")) return rc;
  }
  if (a.nchunk > 1 && k > 0) {
    ProfScope ps(h, wk.stream, KC_TOPK);
    launch_topk_merge(a, wk.stream);
    if (int rc = launch_check(h, "topk_merge")) return rc;
  }
  return MV_OK;
}

int sync_all(mv_handle* h) {  // (a ticket stays in flight until mv_forward_ragged_end collects it)
  for (int wi = 0; wi < h->n_alloc; ++wi) { HIPCHK(h, hipStreamSynchronize(h->work[wi].stream)); h->work[wi].sweep = false; }
  return MV_OK;
}

// Every entry point but the resident sweep works on set 0 (mv_forward_ragged_begin: on a set without a ticket), stream-ordered behind
// what is there; a sweep may have left the other set busy (it reads the anchor bank and the resident corpus): wait for it first.
int check_ready(mv_handle* h) {
  if (!h) return MV_ERR_INVALID;
  if (!h->finalized) return fail(h, MV_ERR_STATE, "weights not finalized (mv_finalize_weights)");
  for (int wi = 1; wi < h->n_alloc; ++wi)
    if (h->work[wi].sweep) {
      HIPCHK(h, hipStreamSynchronize(h->work[wi].stream));
      h->work[wi].sweep = false;
    }
  return MV_OK;
}

// HF's embedding lookup raises on an id outside the table; the embedding kernel would clamp silently (a tokenizer /
// checkpoint vocabulary mismatch would then score garbage without a sign): reject such input at the boundary.
int check_ids(mv_handle* h, const int32_t* ids, int64_t n, const char* who) {
  const int32_t V = h->cfg.vocab_size;
  uint32_t bad = 0;
  for (int64_t i = 0; i < n; ++i) bad |= (uint32_t)(ids[i] < 0) | (uint32_t)(ids[i] >= V);
  if (bad) return fail(h, MV_ERR_INVALID, std::string(who) + ": token id outside [0, vocab_size) — tokenizer and checkpoint vocabularies differ?");
  return MV_OK;
}

const HostTensor* find(mv_handle* h, const std::string& k) {
  auto it = h->staged.find(k);
  return it == h->staged.end() ? nullptr : &it->second;
}

int need(mv_handle* h, const std::string& k, std::initializer_list<int64_t> shape, const HostTensor** out) {
  const HostTensor* t = find(h, k);
  if (!t) return fail(h, MV_ERR_MISSING_WEIGHT, "missing weight: " + k);
  std::vector<int64_t> s(shape);
  if (t->shape != s) {
    std::string got;
    for (auto d : t->shape) got += std::to_string(d) + ",";
    return fail(h, MV_ERR_INVALID, "bad shape for " + k + ": got [" + got + "]");
  }
  *out = t;
  return MV_OK;
}

int upload_f32(mv_handle* h, hipStream_t stream, float** dst, const float* src, int64_t n) {
  if (int rc = dev_alloc(h, stream, dst, n, false)) return rc;
  HIPCHK(h, hipMemcpyAsync(*dst, src, (size_t)n * 4, hipMemcpyHostToDevice, stream));
  HIPCHK(h, hipStreamSynchronize(stream));
  return MV_OK;
}
// Virtual LayerNorm weights (gemm_pp.h): W''[n][k] = W[n][k] gamma[k] - mean_k(W[n][.] gamma[.]),  b'[n] = b[n] + sum_k W[n][k] beta[k]
void fold_layernorm(const float* W, const float* b, const float* gamma, const float* beta, int64_t N, int64_t K,
                    std::vector<float>& Wf, std::vector<float>& bf) {
  Wf.resize((size_t)(N * K));
  bf.resize((size_t)N);
  for (int64_t n = 0; n < N; ++n) {
    double sum = 0.0, wb = 0.0;
    for (int64_t k = 0; k < K; ++k) {
      const double v = (double)W[n * K + k] * (double)gamma[k];
      sum += v;
      wb += (double)W[n * K + k] * (double)beta[k];
    }
    const double mean = sum / (double)K;
    for (int64_t k = 0; k < K; ++k) Wf[(size_t)(n * K + k)] = (float)((double)W[n * K + k] * (double)gamma[k] - mean);
    bf[(size_t)n] = (float)((double)b[n] + wb);
  }
}

// fp32 -> OCP e4m3fn bits (bias 7, 3 mantissa bits, subnormal step 2^-9, max 448, no infinities), round-to-nearest-even,
// saturating: the host-side twin of v_cvt_pk_fp8_f32 behind a clamp (common.h pack_fp8x4)
inline uint8_t f32_to_e4m3_bits(float f) {
  uint32_t x;
  std::memcpy(&x, &f, 4);
  const uint8_t sign = (uint8_t)((x >> 24) & 0x80u);
  x &= 0x7fffffffu;
  if (x > 0x7f800000u) return (uint8_t)(sign | 0x7fu);  // NaN
  float a;
  std::memcpy(&a, &x, 4);
  if (a >= 448.f) return (uint8_t)(sign | 0x7eu);        // saturate (0x7e = 448)
  if (a < 0.0009765625f) return sign;                    // < 2^-10: rounds to zero (2^-10 itself ties to even = 0)
  int e;
  (void)std::frexp(a, &e);                               // a = m 2^e, m in [0.5, 1)  ->  binade 2^(e-1)
  int be = e - 1;                                        // unbiased exponent
  if (be < -6) be = -6;                                  // subnormal range shares the exponent of the smallest normal
  const float q = std::ldexp(1.0f, be - 3);              // spacing of representable values in this binade
  const float r = std::nearbyint(a / q);                 // default rounding mode: to nearest, ties to even
  int mant = (int)r;                                     // 0..16 (8..16 for normals)
  int exp_field = be + 7;
  if (be == -6 && mant < 8) return (uint8_t)(sign | (uint8_t)mant);  // subnormal (exp field 0)
  if (mant == 16) { mant = 8; exp_field += 1; }
  if (exp_field > 15 || (exp_field == 15 && mant > 14)) return (uint8_t)(sign | 0x7eu);
  return (uint8_t)(sign | (uint8_t)(exp_field << 3) | (uint8_t)(mant - 8));
}

// MV_F16X8 planes of a weight matrix W [N][K] (gemm_pp.h): rows [hi8 | lo8] of 2 K bytes with hi8 = e4m3(fp16(W) 2^sw),
// lo8 = e4m3((W - fp16(W)) 2^(11 + sw)); sw = the largest shift that keeps max |W| inside e4m3's 448.  *scale_word = the E8M0
// byte of 2^-(11 + MV_X8_ACT_SHIFT + sw), replicated (the MFMA's scale operand of this GEMM's correction sweep).
void make_x8_weight_planes(const float* W, int64_t N, int64_t K, std::vector<uint8_t>& out, int* scale_word) {
  float mx = 0.f;
  for (int64_t i = 0; i < N * K; ++i) mx = std::fmax(mx, std::fabs(W[i]));
  int sw = 0;
  if (mx > 0.f) {
    sw = (int)std::floor(std::log2(448.0 / (double)mx));
    if (sw > 24) sw = 24;
    if (sw < -24) sw = -24;
  }
  const float sh = std::ldexp(1.0f, sw), sl = std::ldexp(1.0f, 11 + sw);
  out.resize((size_t)(N * 2 * K));
  for (int64_t n = 0; n < N; ++n) {
    uint8_t* row = out.data() + (size_t)(n * 2 * K);
    for (int64_t k = 0; k < K; ++k) {
      const float w = W[n * K + k], hi = f16_bits_to_f32(f32_to_f16_bits(w));
      row[k] = f32_to_e4m3_bits(hi * sh);
      row[K + k] = f32_to_e4m3_bits((w - hi) * sl);
    }
  }
  const int e8 = 127 - (11 + MV_X8_ACT_SHIFT + sw);
  *scale_word = e8 * 0x01010101;
}

int upload_x8_weight(mv_handle* h, hipStream_t stream, uint8_t** dst, int* scale_word, const float* W, int64_t N, int64_t K) {
  std::vector<uint8_t> tmp;
  make_x8_weight_planes(W, N, K, tmp, scale_word);
  if (int rc = dev_alloc(h, stream, dst, (int64_t)tmp.size(), false)) return rc;
  HIPCHK(h, hipMemcpyAsync(*dst, tmp.data(), tmp.size(), hipMemcpyHostToDevice, stream));
  HIPCHK(h, hipStreamSynchronize(stream));
  return MV_OK;
}

int upload_f16(mv_handle* h, hipStream_t stream, half_t** dst, const float* src, int64_t n, float scale = 1.0f) {
  std::vector<uint16_t> tmp((size_t)n);
  for (int64_t i = 0; i < n; ++i) tmp[(size_t)i] = f32_to_f16_bits(src[i] * scale);
  if (int rc = dev_alloc(h, stream, dst, n, false)) return rc;
  HIPCHK(h, hipMemcpyAsync(*dst, tmp.data(), (size_t)n * 2, hipMemcpyHostToDevice, stream));
  HIPCHK(h, hipStreamSynchronize(stream));
  return MV_OK;
}

// ---- the one planner, the one pass cutter, the one pass loop, the one row scatter ---------------------------------------------------------------------------------
// cut_passes: appends to pl the passes of its rows [start, end) at `width` tokens per row: max_rows_for(width) rows each (cap > 0: at most cap), min_len over
// len_of(plan row).
template <typename LenOf>
int cut_passes(mv_handle* h, Plan& pl, int start, int end, int width, int cap, LenOf len_of) {
  int rows = max_rows_for(h, width);
  if (cap > 0 && cap < rows) rows = cap;
  if (rows <= 0) return fail(h, MV_ERR_CAPACITY, "mv_config.max_tokens too small for one row of this length");
  for (int first = start; first < end; first += rows) {
    const int n = end - first < rows ? end - first : rows;
    int m = INT32_MAX;
    for (int i = first; i < first + n; ++i) m = std::min(m, (int)len_of(i));
    pl.passes.push_back({first, n, width, m, pl.tokens});
    pl.tokens += (int64_t)n * width;
  }
  return MV_OK;
}

// plan_batch: rows [0, B) of lengths `lens` into pl.  by_length false: the identity order in passes of max_rows_for(S) rows at width S.  by_length true
// (mv_forward_ragged*: a pad-to-longest batch of UNSORTED rows): the rows ordered (stably) by the padded length of their own token count, a run of one padded
// length merged into the next longer one while it holds fewer than min_tokens padded tokens, each group then cut into passes of max_rows_for(its width) rows.
// max_rows > 0 caps the rows of a pass further (the resident sweep's batch).
int plan_batch(mv_handle* h, const int32_t* lens, int B, int S, int min_tokens, bool by_length, int max_rows, Plan& pl) {
  pl.order.clear(), pl.passes.clear(), pl.tokens = 0;
  auto len_of = [&](int i) { return lens[pl.order.empty() ? i : pl.order[i]]; };  // of plan row i
  if (!by_length) return cut_passes(h, pl, 0, B, S, max_rows, len_of);
  auto pad = [&](int r) { return padded_len(lens[r] < 1 ? 1 : lens[r]); };  // of caller row r
  pl.order.resize(B);
  for (int i = 0; i < B; ++i) {
    if (lens[i] > S) return fail(h, MV_ERR_INVALID, "a row is longer than S");
    pl.order[i] = i;
  }
  std::stable_sort(pl.order.begin(), pl.order.end(), [&](int a, int b) { return pad(a) < pad(b); });
  int start = 0;
  for (int end = 1; end <= B; ++end) {
    const int width = pad(pl.order[end - 1]);
    if (end < B && pad(pl.order[end]) == width) continue;                   // inside a run of one padded length
    if (end < B && (int64_t)(end - start) * width < min_tokens) continue;  // too small a pass: these rows travel with the next longer group
    if (int rc = cut_passes(h, pl, start, end, width < S ? width : S, max_rows, len_of)) return rc;
    start = end;
  }
  return MV_OK;
}

// The form and the anchor count in force when a job is made (MV_F16 has no forms)
void job_form(const mv_handle* h, Job& j) {
  j.G = h->n_anchors;
  j.safe = h->precise && h->form == MV_FORM_SAFE;
  j.guard = h->precise && h->form == MV_FORM_GUARDED;
}

// The one pass loop: the passes [p0, p1) of pl enqueued on workspace set wk without waiting; after a failure it waits for what was enqueued.  Host ids /
// lengths: one upload when they fit wk's buffers, else one per pass at its own width.  Host results: one download each when the rows fit wk's max_batch
// rows (every pass writes at its own rows there), else one per pass.
int run_passes(mv_handle* h, Work& wk, const Plan& pl, size_t p0, size_t p1, const Job& j) {
  const int G = j.G;
  const size_t P = (size_t)h->P;
  const Pass &a = pl.passes[p0], &z = pl.passes[p1 - 1];
  const int rows = z.first + z.rows - a.first;
  const int64_t tokens = z.tok + (int64_t)z.rows * z.width - a.tok;
  const bool one_down = rows <= h->cfg.max_batch, one_up = one_down && tokens <= h->cap_tokens;
  auto upload = [&](int first, int n, int64_t tok, int64_t n_tok) -> int {
    HIPCHK(h, hipMemcpyAsync(wk.d_ids, j.ids + tok, (size_t)n_tok * 4, hipMemcpyHostToDevice, wk.stream));
    HIPCHK(h, hipMemcpyAsync(wk.d_lens, j.lens + first, (size_t)n * 4, hipMemcpyHostToDevice, wk.stream));
    return MV_OK;
  };
  auto download = [&](int first, int n) -> int {  // plan rows [first, first + n) from rows [0, n) of wk's buffers
    const Stage& o = j.out;
    const size_t bg = (size_t)n * G;
    if (o.logits) HIPCHK(h, hipMemcpyAsync(o.logits + (size_t)first * G * 2, wk.logits, bg * 8, hipMemcpyDeviceToHost, wk.stream));
    if (o.probs) HIPCHK(h, hipMemcpyAsync(o.probs + (size_t)first * G * 2, wk.probs, bg * 8, hipMemcpyDeviceToHost, wk.stream));
    if (o.best) HIPCHK(h, hipMemcpyAsync(o.best + (size_t)first * 2, wk.best, (size_t)n * 8, hipMemcpyDeviceToHost, wk.stream));
    if (o.idx) HIPCHK(h, hipMemcpyAsync(o.idx + first, wk.best_idx, (size_t)n * 4, hipMemcpyDeviceToHost, wk.stream));
    if (o.embed) HIPCHK(h, hipMemcpyAsync(o.embed + (size_t)first * P, wk.u, (size_t)n * P * 4, hipMemcpyDeviceToHost, wk.stream));
    if (o.over) HIPCHK(h, hipMemcpyAsync(o.over + first, wk.seq_over, (size_t)n * 4, hipMemcpyDeviceToHost, wk.stream));
    return MV_OK;
  };
  auto run = [&]() -> int {
    if (j.ids && one_up)
      if (int rc = upload(a.first, rows, a.tok, tokens)) return rc;
    for (size_t i = p0; i < p1; ++i) {
      const Pass& p = pl.passes[i];
      const int32_t* ids = j.ids ? wk.d_ids + (one_up ? p.tok - a.tok : 0) : h->c_ids + (size_t)(j.c_row + p.first) * h->c_S;
      const int32_t* lens = j.ids ? wk.d_lens + (one_up ? p.first - a.first : 0) : h->c_lens + j.c_row + p.first;
      if (j.ids && !one_up)
        if (int rc = upload(p.first, p.rows, p.tok, (int64_t)p.rows * p.width)) return rc;
      const size_t r = one_down ? (size_t)(p.first - a.first) : 0;  // the pass's first row in wk's buffers
      float* u = j.u_dev ? j.u_dev + (size_t)p.first * P : wk.u + r * P;
      PassForm pf;
      pf.safe = j.safe; pf.monitor = j.monitor;
      if (j.guard) {
        pf.seq_over = j.ids ? wk.seq_over + r : h->c_over + j.c_row + p.first;
        HIPCHK(h, hipMemsetAsync(pf.seq_over, 0, (size_t)p.rows * 4, wk.stream));
      }
      if (int rc = encode_dev(h, wk, ids, lens, p.min_len, p.rows, p.width, j.n_layers, u, pf, j.full, j.ids ? p.width : h->c_S)) return rc;
      if (!j.ids) {
        const size_t c = (size_t)(j.c_row + p.first);
        if (int rc = match_dev(h, wk, u, p.rows, G, nullptr, nullptr, j.keep_psame ? h->c_psame + c * G : nullptr, j.topk ? j.topk : 1, h->c_best + c * 2, h->c_idx + c,
                               j.topk ? h->c_topk_p + c * j.topk : nullptr, j.topk ? h->c_topk_idx + c * j.topk : nullptr)) return rc;
      } else if (j.match) {  // only the outputs the caller asked for leave the kernel (the best anchor always does)
        if (int rc = match_dev(h, wk, u, p.rows, G, j.out.logits ? wk.logits + r * G * 2 : nullptr, j.out.probs ? wk.probs + r * G * 2 : nullptr, nullptr, 1,
                               wk.best + r * 2, wk.best_idx + r)) return rc;
      }
      if (!one_down)
        if (int rc = download(p.first, p.rows)) return rc;
    }
    return one_down ? download(a.first, rows) : MV_OK;
  };
  const int rc = run();
  if (rc != MV_OK) hipStreamSynchronize(wk.stream);
  return rc;
}

// The one row scatter: row i of src to row map[i] of dst (an empty map: to row i), n rows — the results both hold.
void scatter_rows(const Stage& src, const Stage& dst, const std::vector<int>& map, size_t n, size_t G, size_t P) {
  const size_t g2 = G * 2;
  for (size_t i = 0; i < n; ++i) {
    const size_t o = map.empty() ? i : (size_t)map[i];
    if (src.logits && dst.logits) std::memcpy(dst.logits + o * g2, src.logits + i * g2, g2 * 4);
    if (src.probs && dst.probs) std::memcpy(dst.probs + o * g2, src.probs + i * g2, g2 * 4);
    if (src.best && dst.best) { dst.best[o * 2] = src.best[i * 2]; dst.best[o * 2 + 1] = src.best[i * 2 + 1]; }
    if (src.idx && dst.idx) dst.idx[o] = src.idx[i];
    if (src.embed && dst.embed) std::memcpy(dst.embed + o * P, src.embed + i * P, P * 4);
  }
}

// ---- the guarded form -------------------------------------------------------------------------------------------------------------------------------------
// The rule, per sequence: rescored in the safe form when more than kGuardShare of the (head, layer) items the monitor looked at for it are over MV_SINK_COLLISION
// (attention.h) — the 2 % rule of binding.Engine._check_saturation applied to one sequence.  The monitor looks at every head of every layer whose attention runs
// through attention_v2_kernel (the pruned last layer's single-query attention feeds none), for sequences of at least 16 tokens.
constexpr double kGuardShare = 0.02;
bool guard_flagged(const mv_handle* h, uint32_t over, int len) {
  const int layers = h->cfg.layers - ((h->cls_prune && h->cfg.layers > 0) ? 1 : 0);
  const int items = len >= 16 ? MV_HEADS * layers : 0;
  return (double)over > kGuardShare * (double)items;
}

// After the default-form passes of a guarded job (j.out.over holds the counts, the stream is idle): a second plan over the flagged rows — each at the width of
// the pass it first ran in, the flagged rows of every pass of one width sharing passes — run in the safe form with the monitor detached, against the job's own
// anchor count; those rows' results in j.out (and in the bank, j.u_dev: one copy per row) are overwritten.  Records the form of each of the B rows in the
// caller's order (mv_last_row_forms).
int rescore_rows(mv_handle* h, Work& wk, const Plan& pl, const Job& j, int B) {
  h->last_forms.assign((size_t)B, (uint8_t)(j.safe ? MV_FORM_SAFE : MV_FORM_DEFAULT));
  if (!j.guard) return MV_OK;
  h->guard_seqs += B;
  Plan& p2 = h->plan2;
  HostStage& v = h->stage2;
  p2.order.clear(), p2.passes.clear(), p2.tokens = 0;
  v.ids.clear(), v.lens.clear();
  std::vector<int> widths;
  int64_t n_routed = 0;
  for (const Pass& p : pl.passes)
    if (std::find(widths.begin(), widths.end(), p.width) == widths.end()) widths.push_back(p.width);
  for (const int w : widths) {
    const int start = (int)p2.order.size();
    for (const Pass& p : pl.passes) {
      if (p.width != w) continue;
      for (int i = 0; i < p.rows; ++i) {
        const int r = p.first + i;
        const bool forced = j.routed && j.routed[r];  // (its count was never written)
        if (!forced && !guard_flagged(h, j.out.over[r], j.lens[r])) continue;
        n_routed += forced;
        p2.order.push_back(r);
        v.lens.push_back(j.lens[r]);
        const int32_t* src = j.ids + p.tok + (int64_t)i * w;
        v.ids.insert(v.ids.end(), src, src + w);
      }
    }
    if (int rc = cut_passes(h, p2, start, (int)p2.order.size(), w, 0, [&](int i) { return v.lens[(size_t)i]; })) return rc;
  }
  const size_t n2 = p2.order.size(), P = (size_t)h->P;
  if (!n2) return MV_OK;
  Job r;
  r.match = j.match; r.G = j.G; r.safe = true; r.monitor = false;
  r.out = v.view(n2, (size_t)p2.tokens, (size_t)j.G, P, wanted(j.out, j.out.embed || j.u_dev));  // (the ids and the lengths are in it already)
  r.ids = r.out.ids; r.lens = r.out.lens;
  if (int rc = run_passes(h, wk, p2, 0, p2.passes.size(), r)) return rc;
  HIPCHK(h, hipStreamSynchronize(wk.stream));
  scatter_rows(r.out, j.out, p2.order, n2, (size_t)j.G, P);
  for (size_t i = 0; i < n2; ++i) {
    const size_t o = (size_t)p2.order[i];
    if (j.u_dev) HIPCHK(h, hipMemcpyAsync(j.u_dev + o * P, r.out.embed + i * P, P * 4, hipMemcpyHostToDevice, wk.stream));
    h->last_forms[pl.order.empty() ? o : (size_t)pl.order[o]] = MV_FORM_SAFE;
  }
  if (j.u_dev) HIPCHK(h, hipStreamSynchronize(wk.stream));
  h->guard_rescored += (int64_t)n2 - n_routed;
  h->routed_seqs += n_routed;
  return MV_OK;
}

// The one indexed pass over the resident corpus: rows idx[0, n) gathered into wk's pass buffer at width w, encoded in the form pf (counts: with the per-row
// monitor counts kept), matched, and scattered back to their corpus slots — keep: their P(same) rows too, counts: the counts to c_over; on a keeping corpus
// (mv_corpus_keep) their embeddings and top-k lists as well: a flagged or routed row holds the safe form's, like its best anchor.  Asynchronous on wk:
// idx stays alive until that stream has been waited for; after a failure it waits for what it enqueued.
int run_corpus_rows(mv_handle* h, Work& wk, const int32_t* idx, int n, int w, int min_len, PassForm pf, bool keep, bool counts) {
  const int G = h->n_anchors;
  auto run = [&]() -> int {
    HIPCHK(h, hipMemcpyAsync(wk.d_idx, idx, (size_t)n * 4, hipMemcpyHostToDevice, wk.stream));
    const int64_t nt = (int64_t)n * w;
    hipLaunchKernelGGL(corpus_gather_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, wk.stream, (const int32_t*)h->c_ids, (const int32_t*)h->c_lens,
                       h->c_S, (const int32_t*)wk.d_idx, n, w, wk.d_ids, wk.d_lens);
    if (int rc = launch_check(h, "corpus_gather")) return rc;
    if (counts) {
      pf.seq_over = wk.seq_over;
      HIPCHK(h, hipMemsetAsync(pf.seq_over, 0, (size_t)n * 4, wk.stream));
    }
    if (int rc = encode_dev(h, wk, wk.d_ids, wk.d_lens, min_len, n, w, -1, wk.u, pf, false, w)) return rc;
    const int k = h->c_k;  // mv_corpus_keep: the rows' top-k lists (and their embeddings, wk.u) go back to their corpus slots too
    if (int rc = match_dev(h, wk, wk.u, n, G, nullptr, nullptr, keep ? wk.psame : nullptr, k ? k : 1, wk.best, wk.best_idx, k ? wk.topk_p : nullptr,
                           k ? wk.topk_idx : nullptr)) return rc;
    const int64_t ns = (int64_t)n * (keep ? G : 1);
    hipLaunchKernelGGL(corpus_scatter_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, wk.stream, (const float*)wk.best, (const int32_t*)wk.best_idx,
                       keep ? (const float*)wk.psame : (const float*)nullptr, (const int32_t*)wk.d_idx, n, G, h->c_best, h->c_idx, h->c_psame,
                       counts ? (const uint32_t*)wk.seq_over : (const uint32_t*)nullptr, counts ? h->c_over : (uint32_t*)nullptr);
    if (int rc = launch_check(h, "corpus_scatter")) return rc;
    if (!h->c_embed && !k) return MV_OK;
    const int64_t nk = (int64_t)n * ((h->c_embed ? h->P / 4 : 0) + 2 * ((k & 3) ? k : k / 4));  // one thread per 16 bytes (corpus_scatter_keep_kernel)
    hipLaunchKernelGGL(corpus_scatter_keep_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, wk.stream, h->c_embed ? (const float*)wk.u : (const float*)nullptr,
                       (const uint32_t*)wk.topk_p, (const uint32_t*)wk.topk_idx, (const int32_t*)wk.d_idx, n, h->P, k, h->c_embed, (uint32_t*)h->c_topk_p,
                       (uint32_t*)h->c_topk_idx);
    return launch_check(h, "corpus_scatter_keep");
  };
  const int rc = run();
  if (rc != MV_OK) hipStreamSynchronize(wk.stream);
  return rc;
}

// The resident corpus: every row a guarded sweep ran since the last rescoring (c_pend_w) whose count (c_over) flags it, and every row it left out as routed —
// grouped by the s_eff width of the run (and whether it kept P(same)), each group cut into full passes and run through run_corpus_rows in the safe form with the
// monitor detached.  On workspace set 0, after every batch of the sweep has finished; waits once, at the end.
int rescore_corpus(mv_handle* h) {
  if (!h->c_pending) return MV_OK;
  if (int rc = sync_all(h)) return rc;
  h->c_pending = false;
  h->c_idx_live.clear();
  Work& wk = h->work[0];
  std::vector<uint32_t> over((size_t)h->c_n);
  HIPCHK(h, hipMemcpyAsync(over.data(), h->c_over, (size_t)h->c_n * 4, hipMemcpyDeviceToHost, wk.stream));
  HIPCHK(h, hipStreamSynchronize(wk.stream));
  std::map<int, std::vector<int32_t>> groups;  // 2 width + keep -> corpus rows (alive until the last upload from them has been waited for)
  for (int64_t r = 0; r < h->c_n; ++r) {
    const int w = h->c_pend_w[(size_t)r];
    if (!w) continue;
    h->c_pend_w[(size_t)r] = 0;
    const int forced = h->c_pend_force[(size_t)r];  // routed by the sink-token list of its sweep: it has run in no pass yet
    if (forced || guard_flagged(h, over[(size_t)r], h->c_lens_host[(size_t)r])) groups[2 * w + h->c_pend_keep[(size_t)r]].push_back((int32_t)r);
  }
  PassForm pf;
  pf.safe = true; pf.monitor = false;
  for (auto& kv : groups) {
    const int w = kv.first >> 1;
    const bool keep = (kv.first & 1) && h->c_psame && h->c_G == h->n_anchors;
    const std::vector<int32_t>& idx = kv.second;
    Plan g;  // the group's rows in passes
    if (int rc = cut_passes(h, g, 0, (int)idx.size(), w, 0, [&](int i) { return h->c_lens_host[(size_t)idx[(size_t)i]]; })) return rc;
    for (const Pass& p : g.passes) {
      if (int rc = run_corpus_rows(h, wk, idx.data() + p.first, p.rows, w, p.min_len, pf, keep, false)) return rc;
      for (int i = p.first; i < p.first + p.rows; ++i) {
        h->c_forms[(size_t)idx[(size_t)i]] = MV_FORM_SAFE;
        (h->c_pend_force[(size_t)idx[(size_t)i]] ? h->routed_seqs : h->guard_rescored) += 1;
      }
    }
  }
  HIPCHK(h, hipStreamSynchronize(wk.stream));
  return MV_OK;
}

// ---- the sink-token list (mv_set_sink_tokens; route.h) ----------------------------------------------------------------------------------------------------------
// A host batch of a guarded job: the rows of [B][S] the list routes (h->route_flags, caller's row order); returns how many.  0 without a list.
int scan_routed(mv_handle* h, const Job& j, const int32_t* ids, const int32_t* lens, int B, int S) {
  if (!j.guard || j.full || h->sink_tokens.empty()) return 0;
  h->route_flags.resize((size_t)B);
  return route_scan(ids, lens, B, S, h->sink_bitmap.data(), h->cfg.vocab_size, h->route_flags.data());
}

// A planned batch with routed rows (flags: caller's row order): every pass of pl keeps its rows and its width, with its unrouted rows first — pl.order is made
// explicit for that — `routed` marks the others in plan order, and p1 gets one pass per pass of pl that has unrouted rows: those rows alone, min_len over them
// (the ids of a pass are staged in plan order, so they are the head of the pass's ids: same Pass::tok).
void split_plan(Plan& pl, int B, const int32_t* lens, const uint8_t* flags, std::vector<uint8_t>& routed, Plan& p1) {
  if (pl.order.empty()) {
    pl.order.resize((size_t)B);
    for (int i = 0; i < B; ++i) pl.order[(size_t)i] = i;
  }
  routed.assign((size_t)B, 0);
  p1.order.clear(), p1.passes.clear(), p1.tokens = pl.tokens;
  for (const Pass& p : pl.passes) {
    const auto b = pl.order.begin() + p.first, e = b + p.rows;
    const auto mid = std::stable_partition(b, e, [&](int r) { return !flags[r]; });
    const int nu = (int)(mid - b);
    for (int i = nu; i < p.rows; ++i) routed[(size_t)(p.first + i)] = 1;
    if (!nu) continue;
    int m = INT32_MAX;
    for (auto it = b; it != mid; ++it) m = std::min(m, lens[*it]);
    p1.passes.push_back({p.first, nu, p.width, m, p.tok});
  }
}

// The resident corpus: h->c_route = the flag of every row under the current list, recomputed when an upload or a list change made it stale — one kernel over
// the whole corpus, one copy back, one wait (workspace set 0's stream; nothing on the device reads what it writes).  An empty list flags nothing, without a launch.
int ensure_route_flags(mv_handle* h) {
  if (!h->c_route_stale) return MV_OK;
  h->c_route.assign((size_t)h->c_n, 0);
  if (!h->sink_tokens.empty() && h->c_n > 0) {
    const hipStream_t s0 = h->work[0].stream;
    if (!h->route_bm_dev)
      if (int rc = dev_alloc(h, s0, &h->route_bm_dev, (int64_t)h->sink_bitmap.size(), false)) return rc;
    if (!h->c_route_dev)
      if (int rc = dev_alloc(h, s0, &h->c_route_dev, h->c_n, false)) return rc;
    HIPCHK(h, hipMemcpyAsync(h->route_bm_dev, h->sink_bitmap.data(), h->sink_bitmap.size() * 4, hipMemcpyHostToDevice, s0));
    hipLaunchKernelGGL(route_flags_kernel, dim3((unsigned)((h->c_n + 3) / 4)), dim3(256), 0, s0, (const int32_t*)h->c_ids, (const int32_t*)h->c_lens, h->c_n, h->c_S,
                       (const uint32_t*)h->route_bm_dev, h->cfg.vocab_size, h->c_route_dev);
    if (int rc = launch_check(h, "route_flags")) return rc;
    HIPCHK(h, hipMemcpyAsync(h->c_route.data(), h->c_route_dev, (size_t)h->c_n, hipMemcpyDeviceToHost, s0));
    HIPCHK(h, hipStreamSynchronize(s0));
  }
  h->c_route_stale = false;
  return MV_OK;
}

// One batch of a guarded sweep that has routed rows (pass p of the sweep's plan, whose row 0 is corpus row j.c_row): its unrouted rows through run_corpus_rows
// at the sweep's width, in the default form with the per-row monitor counts kept.  Asynchronous, like the in-place batches next to it: the index list lives in
// c_idx_live until rescore_corpus has waited for the sweep.
int run_split_batch(mv_handle* h, Work& wk, const Pass& p, const Job& j) {
  std::vector<int32_t> idx;
  int m = INT32_MAX;
  for (int i = 0; i < p.rows; ++i) {
    const int64_t r = j.c_row + p.first + i;
    if (h->c_route[(size_t)r]) continue;
    idx.push_back((int32_t)r);
    m = std::min(m, h->c_lens_host[(size_t)r]);
  }
  if (idx.empty()) return MV_OK;  // every row routed: nothing runs in the default form
  h->c_idx_live.push_back(std::move(idx));
  const std::vector<int32_t>& ix = h->c_idx_live.back();
  return run_corpus_rows(h, wk, ix.data(), (int)ix.size(), p.width, m, PassForm(), j.keep_psame, true);
}

// ---- the one host batch flow --------------------------------------------------------------------------------------------------------------------------------------
// The rows of a batch gathered into plan order: each pass's ids at its own width (ids [B][S]).
void gather(const Plan& pl, const int32_t* ids, const int32_t* lens, int S, int32_t* ids_out, int32_t* lens_out) {
  for (const Pass& p : pl.passes)
    for (int i = 0; i < p.rows; ++i) {
      const size_t r = (size_t)pl.order[p.first + i];
      std::memcpy(ids_out + p.tok + (int64_t)i * p.width, ids + r * S, (size_t)p.width * 4);
      lens_out[p.first + i] = lens[r];
    }
}

// Make and enqueue: rows [0, B) of ids [B][S] planned into pl (plan_batch), the rows the sink-token list routes split off (scan_routed, split_plan: `routed`,
// which j then points into), the batch gathered in plan order into a view of the staging — hs, or wk's pinned one — that holds the results `want` names, and the
// passes of the unrouted rows enqueued on wk.  Does not wait.  j comes in made (match, form, anchor count) and leaves with the staging as its ids, lens and out.
// A batch in its own order with no routed row is not staged: its ids are read in place and j.out stays the caller's arrays (the plan's order is empty).
int enqueue_batch(mv_handle* h, Work& wk, Plan& pl, std::vector<uint8_t>& routed, HostStage* hs, const int32_t* ids, const int32_t* lens, int B, int S,
                  int min_tokens, bool by_length, Want want, Job& j) {
  if (int rc = plan_batch(h, lens, B, S, min_tokens, by_length, 0, pl)) return rc;
  const Plan* p1 = &pl;  // the passes of the first run: without the routed rows
  routed.clear();
  j.routed = nullptr;
  if (scan_routed(h, j, ids, lens, B, S)) {
    split_plan(pl, B, lens, h->route_flags.data(), routed, h->plan1);
    j.routed = routed.data();
    p1 = &h->plan1;
  }
  const bool in_place = pl.order.empty();
  if (in_place) want = Want();  // (only the monitor counts go through the staging)
  want.over = j.guard;
  const Stage st = hs ? hs->view((size_t)B, in_place ? 0 : (size_t)pl.tokens, (size_t)j.G, (size_t)h->P, want) : only(wk.pin, want);
  if (in_place) {
    j.ids = ids; j.lens = lens; j.out.over = st.over;
  } else {
    gather(pl, ids, lens, S, st.ids, st.lens);
    j.ids = st.ids; j.lens = st.lens; j.out = st; j.u_dev = nullptr;
  }
  return p1->passes.empty() ? MV_OK : run_passes(h, wk, *p1, 0, p1->passes.size(), j);
}

// Collect: wait for wk, rescore the flagged and the routed rows of a guarded job (rescore_rows), and bring a staged batch's results to the caller's rows (dst).
int collect_batch(mv_handle* h, Work& wk, const Plan& pl, const Job& j, int B, const Stage& dst) {
  HIPCHK(h, hipStreamSynchronize(wk.stream));
  if (!j.full)  // (mv_debug_encode: the taps show the passes as they ran)
    if (int rc = rescore_rows(h, wk, pl, j, B)) return rc;
  if (!pl.order.empty()) scatter_rows(j.out, dst, pl.order, (size_t)B, (size_t)j.G, (size_t)h->P);
  return MV_OK;
}

// mv_forward / mv_encode / mv_anchor_append / mv_debug_encode: the rows in their own order on workspace set 0, both halves back to back.  mv_anchor_append with
// routed rows (the batch was staged): the bank's rows in the caller's order, in one copy.
int run_in_order(mv_handle* h, const int32_t* lens, int B, int S, const Job& j) {
  Work& wk = h->work[0];
  const size_t P = (size_t)h->P;
  Job s = j;
  if (int rc = enqueue_batch(h, wk, h->plan, h->routed, &h->stage, j.ids, lens, B, S, 0, false, wanted(j.out, j.out.embed || j.u_dev), s)) return rc;
  if (int rc = collect_batch(h, wk, h->plan, s, B, j.out)) return rc;
  if (j.u_dev && !h->plan.order.empty()) {
    Want e;
    e.embed = true;
    const Stage bank = h->stage2.view((size_t)B, 0, 0, P, e);  // (rescore_rows is done with it)
    scatter_rows(s.out, bank, h->plan.order, (size_t)B, 0, P);
    HIPCHK(h, hipMemcpyAsync(j.u_dev, bank.embed, (size_t)B * P * 4, hipMemcpyHostToDevice, wk.stream));
    HIPCHK(h, hipStreamSynchronize(wk.stream));
  }
  return MV_OK;
}

}  // namespace

// =================================================================================================
// The device WordPiece tokenizer (include/memvul_hip.h mv_tok_*; memvul_amd/csrc/wordpiece.h): an object of its own — its table, its stream, its buffers —
// that shares no mutable state with any mv_handle, so the tokenising thread may be inside mv_tok_encode while another thread is inside a handle's sweep.
struct mv_tokenizer {
  int device = -1;  // < 0: the table only (mv_tok_encode_host)
  WpHost host;
  WpTable dev{};    // the same table with device pointers
  hipStream_t stream = nullptr;
  void *d_slots = nullptr, *d_pool = nullptr, *d_lit = nullptr, *d_lit_off = nullptr;
  void *d_text = nullptr, *d_off = nullptr, *d_ids = nullptr, *d_lens = nullptr, *d_status = nullptr;  // grow to the largest call
  size_t cap_text = 0, cap_off = 0, cap_ids = 0, cap_lens = 0, cap_status = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around each chunk's kernel
  float kernel_ms = 0.f;                    // the kernel's own time over the chunks of the last mv_tok_encode (mv_tok_kernel_ms)
  std::vector<int64_t> rel;  // a chunk's offsets, rebased to its first byte
  std::string err;
};

namespace {

int tok_fail(mv_tokenizer* t, int code, const std::string& msg) {
  if (t) t->err = msg; else g_create_error = msg;
  return code;
}

int on_exception(std::nullptr_t) noexcept { return on_exception((mv_handle*)nullptr); }  // (the entries without an object: not ambiguous between the two below)

int on_exception(mv_tokenizer* t) noexcept {
  const int code = on_exception((mv_handle*)nullptr);  // (classifies the exception in flight; the message lands in g_create_error)
  try {
    if (t) t->err = g_create_error;
  } catch (...) {
  }
  return code;
}

#define TOKHIP(t, expr)                                                                              \
  do {                                                                                              \
    hipError_t _e = (expr);                                                                         \
    if (_e != hipSuccess)                                                                           \
      return tok_fail(t, MV_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));            \
  } while (0)

constexpr int64_t kTokChunkBytes = 64ll << 20;  // text per launch
constexpr int kTokChunkRows = 1 << 16;          // rows per launch: bounds the id buffer at 128 MiB

// what mv_tok_encode and mv_tok_encode_host refuse, before they touch an output
int tok_check_args(mv_tokenizer* tok, const char* what, const char* text, const int64_t* off, int n, int max_length, const int32_t* ids, const int32_t* lens,
                   const uint8_t* status) {
  if (n < 0 || max_length < 2 || max_length > WP_MAX_LENGTH) return tok_fail(tok, MV_ERR_INVALID, std::string(what) + ": n < 0 or max_length outside 2 .. 512");
  if (n == 0) return MV_OK;
  if (!off || !ids || !lens || !status) return tok_fail(tok, MV_ERR_INVALID, std::string(what) + ": NULL offsets or output");
  if (off[0] < 0) return tok_fail(tok, MV_ERR_INVALID, std::string(what) + ": negative offset");
  for (int i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return tok_fail(tok, MV_ERR_INVALID, std::string(what) + ": offsets not ascending");
  if (off[n] > off[0] && !text) return tok_fail(tok, MV_ERR_INVALID, std::string(what) + ": NULL text");
  return MV_OK;
}

int tok_grow(mv_tokenizer* tok, void** p, size_t* cap, size_t need) {
  if (need <= *cap) return MV_OK;
  if (*p) TOKHIP(tok, hipFree(*p));
  *p = nullptr;
  *cap = 0;
  const size_t want = (need + need / 4 + 255) & ~(size_t)255;
  if (hipMalloc(p, want) != hipSuccess) {
    *p = nullptr;
    (void)hipGetLastError();
    return tok_fail(tok, MV_ERR_NOMEM, "mv_tok_encode: device allocation of " + std::to_string(want) + " bytes failed");
  }
  *cap = want;
  return MV_OK;
}

void tok_release(mv_tokenizer* t) {
  if (t->device >= 0 && hipSetDevice(t->device) == hipSuccess) {
    if (t->stream) hipStreamSynchronize(t->stream);
    for (void* p : {t->d_slots, t->d_pool, t->d_lit, t->d_lit_off, t->d_text, t->d_off, t->d_ids, t->d_lens, t->d_status})
      if (p) hipFree(p);
    if (t->ev0) hipEventDestroy(t->ev0);
    if (t->ev1) hipEventDestroy(t->ev1);
    if (t->stream) hipStreamDestroy(t->stream);
  }
  delete t;
}

// the chunks of one mv_tok_encode call, enqueued and collected one after the other on the object's stream
int tok_encode_chunks(mv_tokenizer* tok, const char* text, const int64_t* off, int n, int max_length, int add_special, int32_t* ids, int32_t* lens, uint8_t* status) {
  for (int r0 = 0; r0 < n;) {
    // a chunk ends before the row that would take it past 64 MiB of text (a single larger row is a chunk of its own) and after 65 536 rows
    int r1 = r0 + 1;
    while (r1 < n && r1 - r0 < kTokChunkRows && off[r1 + 1] - off[r0] <= kTokChunkBytes) ++r1;
    const int m = r1 - r0;
    const int64_t bytes = off[r1] - off[r0];
    if (int rc = tok_grow(tok, &tok->d_text, &tok->cap_text, (size_t)bytes + 1)) return rc;
    if (int rc = tok_grow(tok, &tok->d_off, &tok->cap_off, (size_t)(m + 1) * sizeof(int64_t))) return rc;
    if (int rc = tok_grow(tok, &tok->d_ids, &tok->cap_ids, (size_t)m * max_length * sizeof(int32_t))) return rc;
    if (int rc = tok_grow(tok, &tok->d_lens, &tok->cap_lens, (size_t)m * sizeof(int32_t))) return rc;
    if (int rc = tok_grow(tok, &tok->d_status, &tok->cap_status, (size_t)m)) return rc;
    tok->rel.resize((size_t)m + 1);
    for (int i = 0; i <= m; ++i) tok->rel[i] = off[r0 + i] - off[r0];
    if (bytes > 0) TOKHIP(tok, hipMemcpyAsync(tok->d_text, text + off[r0], (size_t)bytes, hipMemcpyHostToDevice, tok->stream));
    TOKHIP(tok, hipMemcpyAsync(tok->d_off, tok->rel.data(), (size_t)(m + 1) * sizeof(int64_t), hipMemcpyHostToDevice, tok->stream));
    TOKHIP(tok, hipEventRecord(tok->ev0, tok->stream));
    hipLaunchKernelGGL(wp_encode_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, tok->stream, tok->dev, (const uint8_t*)tok->d_text,
                       (const int64_t*)tok->d_off, m, max_length, add_special ? 1 : 0, (int32_t*)tok->d_ids, (int32_t*)tok->d_lens, (uint8_t*)tok->d_status);
    TOKHIP(tok, hipGetLastError());
    TOKHIP(tok, hipEventRecord(tok->ev1, tok->stream));
    TOKHIP(tok, hipMemcpyAsync(ids + (size_t)r0 * max_length, tok->d_ids, (size_t)m * max_length * sizeof(int32_t), hipMemcpyDeviceToHost, tok->stream));
    TOKHIP(tok, hipMemcpyAsync(lens + r0, tok->d_lens, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, tok->stream));
    TOKHIP(tok, hipMemcpyAsync(status + r0, tok->d_status, (size_t)m, hipMemcpyDeviceToHost, tok->stream));
    TOKHIP(tok, hipStreamSynchronize(tok->stream));
    float ms = 0.f;
    TOKHIP(tok, hipEventElapsedTime(&ms, tok->ev0, tok->ev1));
    tok->kernel_ms += ms;
    r0 = r1;
  }
  return MV_OK;
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
  // ---- environment switches (include/memvul_hip.h lists them).  Every one is parsed strictly: a value the library does not understand fails
  // mv_create with a message — a typo must never silently select other numerics (or another stream count) than the one asked for.
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
    if (!env_int("MEMVUL_STREAMS", 1, 2, &ns)) return MV_ERR_INVALID;  // (the guard destroys the handle)
    h->n_streams = h->n_alloc = ns;
  }
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
  (void)hipGetLastError();
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
  {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) h->num_cu = ncu;
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
  }
#endif

  h->cap_tokens = round_up(cfg->max_tokens, 256) + 256;
  const int64_t T = h->cap_tokens;
  int rc = MV_OK;
  auto A = [&](int r) { if (rc == MV_OK) rc = r; };
  const int64_t BG = (int64_t)cfg->max_batch * cfg->max_anchors;
  const int64_t Bp = round_up(cfg->max_batch, 256);  // [CLS]-row buffers of the pruned last layer
  for (int wi = 0; wi < h->n_alloc; ++wi) {
    Work& wk = h->work[wi];
    A(dev_alloc(h, wk.stream, &wk.d_ids, T));
    A(dev_alloc(h, wk.stream, &wk.d_lens, (int64_t)cfg->max_batch + 16));
    A(dev_alloc(h, wk.stream, &wk.seq_over, (int64_t)cfg->max_batch));
    A(dev_alloc(h, wk.stream, &wk.d_idx, (int64_t)cfg->max_batch));
    A(dev_alloc(h, wk.stream, &wk.xres, T * MV_HIDDEN));
    A(dev_alloc(h, wk.stream, &wk.x16, T * MV_HIDDEN));
    A(dev_alloc(h, wk.stream, &wk.q, T * MV_HIDDEN));
    A(dev_alloc(h, wk.stream, &wk.k, T * MV_HIDDEN));
    A(dev_alloc(h, wk.stream, &wk.vt, T * MV_HIDDEN));
    A(dev_alloc(h, wk.stream, &wk.ctx, T * MV_HIDDEN));
    A(dev_alloc(h, wk.stream, &wk.h16, T * MV_INTER));
    A(dev_alloc(h, wk.stream, &wk.lnstats, T * 6));
    A(dev_alloc(h, wk.stream, &wk.lnpart, T * 6));
    A(dev_alloc(h, wk.stream, &wk.c32, Bp * MV_HIDDEN));
    A(dev_alloc(h, wk.stream, &wk.cq, Bp * MV_HIDDEN));
    A(dev_alloc(h, wk.stream, &wk.c16, Bp * MV_HIDDEN));
    A(dev_alloc(h, wk.stream, &wk.cctx, Bp * MV_HIDDEN));
    A(dev_alloc(h, wk.stream, &wk.ch16, Bp * MV_INTER));
    A(dev_alloc(h, wk.stream, &wk.u, (int64_t)cfg->max_batch * h->P));
    A(dev_alloc(h, wk.stream, &wk.pooled, (int64_t)cfg->max_batch * MV_HIDDEN));
    A(dev_alloc(h, wk.stream, &wk.u_in, (int64_t)cfg->max_batch * h->P));
    A(dev_alloc(h, wk.stream, &wk.logits, BG * 2));
    A(dev_alloc(h, wk.stream, &wk.probs, BG * 2));
    A(dev_alloc(h, wk.stream, &wk.psame, BG));
    A(dev_alloc(h, wk.stream, &wk.best, (int64_t)cfg->max_batch * 2));
    A(dev_alloc(h, wk.stream, &wk.best_idx, cfg->max_batch));
    A(dev_alloc(h, wk.stream, &wk.topk_p, (int64_t)cfg->max_batch * 64));
    A(dev_alloc(h, wk.stream, &wk.topk_idx, (int64_t)cfg->max_batch * 64));
    {
      const int64_t nch = (cfg->max_anchors + 255) / 256;
      const int64_t per = nch > 1 ? (nch * MK_KMAX < 1024 ? nch * MK_KMAX : 1024) : 0;  // chunks x k <= 1024 (match_dev)
      A(dev_alloc(h, wk.stream, &wk.part_p, (int64_t)cfg->max_batch * per));
      A(dev_alloc(h, wk.stream, &wk.part_q, (int64_t)cfg->max_batch * per));
      A(dev_alloc(h, wk.stream, &wk.part_i, (int64_t)cfg->max_batch * per));
    }
    if (rc == MV_OK && hipStreamSynchronize(wk.stream) != hipSuccess) rc = MV_ERR_HIP;
  }
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
  const hipStream_t s0 = h->work[0].stream;  // (the uploads)
  const mv_config& c = h->cfg;
  const std::string P = "_text_field_embedder.token_embedder_tokens.transformer_model.";
  const int64_t H = MV_HIDDEN, I = MV_INTER;
  const HostTensor *t = nullptr, *t2 = nullptr, *t3 = nullptr;
  int rc;
#define NEED(key, ...) if ((rc = need(h, key, {__VA_ARGS__}, &t)) != MV_OK) return rc
  NEED(P + "embeddings.word_embeddings.weight", c.vocab_size, H);
  if ((rc = upload_f32(h, s0, &h->wemb, t->data.data(), (int64_t)c.vocab_size * H))) return rc;
  {
    const HostTensor* tp = find(h, P + "embeddings.position_embeddings.weight");
    if (!tp) return fail(h, MV_ERR_MISSING_WEIGHT, "missing weight: " + P + "embeddings.position_embeddings.weight");
    if (tp->shape.size() != 2 || tp->shape[1] != H || tp->shape[0] < c.max_pos)
      return fail(h, MV_ERR_INVALID, "bad shape for position_embeddings");
    if ((rc = upload_f32(h, s0, &h->pemb, tp->data.data(), (int64_t)c.max_pos * H))) return rc;
  }
  NEED(P + "embeddings.token_type_embeddings.weight", c.type_vocab, H);
  if ((rc = upload_f32(h, s0, &h->temb, t->data.data(), H))) return rc;  // row 0 only: type ids are all zero on this path
  NEED(P + "embeddings.LayerNorm.weight", H);
  if ((rc = upload_f32(h, s0, &h->embg, t->data.data(), H))) return rc;
  NEED(P + "embeddings.LayerNorm.bias", H);
  if ((rc = upload_f32(h, s0, &h->embb, t->data.data(), H))) return rc;
  h->L.resize(c.layers);
  for (int l = 0; l < c.layers; ++l) {
    const std::string q = P + "encoder.layer." + std::to_string(l) + ".";
    LayerW& w = h->L[l];
    std::vector<float> wqkv_host, bqkv_host;
    // packed QKV [2304][768]; 1/sqrt(64) folded into W_q, b_q (exact: power of two)
    if ((rc = need(h, q + "attention.self.query.weight", {H, H}, &t))) return rc;
    if ((rc = need(h, q + "attention.self.key.weight", {H, H}, &t2))) return rc;
    if ((rc = need(h, q + "attention.self.value.weight", {H, H}, &t3))) return rc;
    {
      std::vector<float> pack((size_t)(3 * H * H));
      for (int64_t i = 0; i < H * H; ++i) {
        pack[(size_t)i] = t->data[(size_t)i] * 0.125f;
        pack[(size_t)(H * H + i)] = t2->data[(size_t)i];
        pack[(size_t)(2 * H * H + i)] = t3->data[(size_t)i];
      }
      if (f32 && (rc = upload_f32(h, s0, &w.wqkv32, pack.data(), 3 * H * H))) return rc;
      if (!f32 && (rc = upload_f16(h, s0, &w.wqkv, pack.data(), 3 * H * H))) return rc;
      wqkv_host = pack;
    }
    if ((rc = need(h, q + "attention.self.query.bias", {H}, &t))) return rc;
    if ((rc = need(h, q + "attention.self.key.bias", {H}, &t2))) return rc;
    if ((rc = need(h, q + "attention.self.value.bias", {H}, &t3))) return rc;
    {
      std::vector<float> pack((size_t)(3 * H));
      for (int64_t i = 0; i < H; ++i) {
        pack[(size_t)i] = t->data[(size_t)i] * 0.125f;
        pack[(size_t)(H + i)] = t2->data[(size_t)i];
        pack[(size_t)(2 * H + i)] = t3->data[(size_t)i];
      }
      if ((rc = upload_f32(h, s0, &w.bqkv, pack.data(), 3 * H))) return rc;
      bqkv_host = pack;
    }
    if (!f32) {  // the LayerNorm in front of this layer's QKV projection: the embedding LayerNorm or the previous layer's output LayerNorm
      const std::string lnk = l == 0 ? P + "embeddings.LayerNorm." : P + "encoder.layer." + std::to_string(l - 1) + ".output.LayerNorm.";
      const HostTensor *tg = nullptr, *tb = nullptr;
      if ((rc = need(h, lnk + "weight", {H}, &tg))) return rc;
      if ((rc = need(h, lnk + "bias", {H}, &tb))) return rc;
      std::vector<float> Wf, bf;
      fold_layernorm(wqkv_host.data(), bqkv_host.data(), tg->data.data(), tb->data.data(), 3 * H, H, Wf, bf);
      if ((rc = upload_f16(h, s0, &w.wqkv_f, Wf.data(), 3 * H * H))) return rc;
      if (precise && (rc = upload_x8_weight(h, s0, &w.wqkv_f8, &w.sc_qkv, Wf.data(), 3 * H, H))) return rc;
      if ((rc = upload_f32(h, s0, &w.bqkv_f, bf.data(), 3 * H))) return rc;
    }
    NEED(q + "attention.output.dense.weight", H, H);
    if (f32 && (rc = upload_f32(h, s0, &w.wo32, t->data.data(), H * H))) return rc;
    if (!f32 && (rc = upload_f16(h, s0, &w.wo, t->data.data(), H * H))) return rc;
    if (precise && (rc = upload_x8_weight(h, s0, &w.wo8, &w.sc_o, t->data.data(), H, H))) return rc;
    NEED(q + "attention.output.dense.bias", H);
    if ((rc = upload_f32(h, s0, &w.bo, t->data.data(), H))) return rc;
    NEED(q + "attention.output.LayerNorm.weight", H);
    if ((rc = upload_f32(h, s0, &w.ln1g, t->data.data(), H))) return rc;
    NEED(q + "attention.output.LayerNorm.bias", H);
    if ((rc = upload_f32(h, s0, &w.ln1b, t->data.data(), H))) return rc;
    NEED(q + "intermediate.dense.weight", I, H);
    if (f32 && (rc = upload_f32(h, s0, &w.w132, t->data.data(), I * H))) return rc;
    if (!f32 && (rc = upload_f16(h, s0, &w.w1, t->data.data(), I * H))) return rc;
    NEED(q + "intermediate.dense.bias", I);
    if ((rc = upload_f32(h, s0, &w.b1, t->data.data(), I))) return rc;
    if (!f32) {  // FFN-1 with the attention-output LayerNorm folded in
      const HostTensor *tw = nullptr, *tg = nullptr, *tb = nullptr;
      if ((rc = need(h, q + "intermediate.dense.weight", {I, H}, &tw))) return rc;
      if ((rc = need(h, q + "attention.output.LayerNorm.weight", {H}, &tg))) return rc;
      if ((rc = need(h, q + "attention.output.LayerNorm.bias", {H}, &tb))) return rc;
      std::vector<float> Wf, bf;
      fold_layernorm(tw->data.data(), t->data.data(), tg->data.data(), tb->data.data(), I, H, Wf, bf);
      if ((rc = upload_f16(h, s0, &w.w1_f, Wf.data(), I * H))) return rc;
      if (precise && (rc = upload_x8_weight(h, s0, &w.w1_f8, &w.sc_1, Wf.data(), I, H))) return rc;
      if ((rc = upload_f32(h, s0, &w.b1_f, bf.data(), I))) return rc;
    }
    NEED(q + "output.dense.weight", H, I);
    if (f32 && (rc = upload_f32(h, s0, &w.w232, t->data.data(), H * I))) return rc;
    if (!f32 && (rc = upload_f16(h, s0, &w.w2, t->data.data(), H * I))) return rc;
    if (precise && (rc = upload_x8_weight(h, s0, &w.w28, &w.sc_2, t->data.data(), H, I))) return rc;
    NEED(q + "output.dense.bias", H);
    if ((rc = upload_f32(h, s0, &w.b2, t->data.data(), H))) return rc;
    NEED(q + "output.LayerNorm.weight", H);
    if ((rc = upload_f32(h, s0, &w.ln2g, t->data.data(), H))) return rc;
    NEED(q + "output.LayerNorm.bias", H);
    if ((rc = upload_f32(h, s0, &w.ln2b, t->data.data(), H))) return rc;
  }
  if (precise && c.layers > 0) {  // fp32 [CLS] tail of the last layer: weights transposed to [k][n]
    const std::string q = P + "encoder.layer." + std::to_string(c.layers - 1) + ".";
    LayerW& w = h->L[c.layers - 1];
    auto up_T = [&](const std::string& key, int64_t N, int64_t K, float scale, float** dst) -> int {
      const HostTensor* tt = nullptr;
      if (int r = need(h, key, {N, K}, &tt)) return r;
      std::vector<float> tr((size_t)(N * K));
      for (int64_t n = 0; n < N; ++n) for (int64_t k = 0; k < K; ++k) tr[(size_t)(k * N + n)] = tt->data[(size_t)(n * K + k)] * scale;
      return upload_f32(h, s0, dst, tr.data(), N * K);
    };
    if ((rc = up_T(q + "attention.self.query.weight", H, H, 0.125f, &w.wqT32))) return rc;  // 1/sqrt(64) folded like the packed QKV
    if ((rc = up_T(q + "attention.output.dense.weight", H, H, 1.0f, &w.woT32))) return rc;
    if ((rc = up_T(q + "intermediate.dense.weight", I, H, 1.0f, &w.w1T32))) return rc;
    if ((rc = up_T(q + "output.dense.weight", H, I, 1.0f, &w.w2T32))) return rc;
  }
  // pooler / header: transposed to [k][n] (fp32)
  NEED("_bert_pooler.pooler.dense.weight", H, H);
  {
    std::vector<float> tr((size_t)(H * H));
    for (int64_t n = 0; n < H; ++n) for (int64_t k = 0; k < H; ++k) tr[(size_t)(k * H + n)] = t->data[(size_t)(n * H + k)];
    if ((rc = upload_f32(h, s0, &h->WpT, tr.data(), H * H))) return rc;
  }
  NEED("_bert_pooler.pooler.dense.bias", H);
  if ((rc = upload_f32(h, s0, &h->bp, t->data.data(), H))) return rc;
  if (h->P == MV_PROJ) {  // use_header (model_memory.py:69-71); with proj_dim = 768 the model has no _projector_single
    NEED("_projector_single._linear_layers.0.weight", MV_PROJ, H);
    {
      std::vector<float> tr((size_t)(H * MV_PROJ));
      for (int64_t n = 0; n < MV_PROJ; ++n) for (int64_t k = 0; k < H; ++k) tr[(size_t)(k * MV_PROJ + n)] = t->data[(size_t)(n * H + k)];
      if ((rc = upload_f32(h, s0, &h->WhT, tr.data(), H * MV_PROJ))) return rc;
    }
    NEED("_projector_single._linear_layers.0.bias", MV_PROJ);
    if ((rc = upload_f32(h, s0, &h->bh, t->data.data(), MV_PROJ))) return rc;
  }
  NEED("_projector.weight", 2, 3 * (int64_t)h->P);
  if ((rc = upload_f32(h, s0, &h->Wm, t->data.data(), 2 * 3 * (int64_t)h->P))) return rc;
#undef NEED
  if (f32) {  // MV_F32: the fp32 planes of one pass, 6144 floats per token (1.6 GB per workspace set at 65 536 tokens)
    for (int wi = 0; wi < h->n_alloc; ++wi) {
      Work& wk = h->work[wi];
      rc = dev_alloc(h, wk.stream, &wk.qkv32, h->cap_tokens * 3 * MV_HIDDEN);
      if (rc == MV_OK) rc = dev_alloc(h, wk.stream, &wk.ctx32, h->cap_tokens * MV_HIDDEN);
      if (rc == MV_OK) rc = dev_alloc(h, wk.stream, &wk.h32, h->cap_tokens * MV_INTER);
      if (rc == MV_OK && hipStreamSynchronize(wk.stream) != hipSuccess) rc = MV_ERR_HIP;
      if (rc != MV_OK) return rc;
    }
  }
  if (!precise && !f32) {  // MV_F16: the lo fp16 plane of the two-plane raw stream (MV_F16X8 keeps the stream's low part in the lo8 plane of x8 + st_lo: gemm.h GemmArgs::out16b)
    for (int wi = 0; wi < h->n_alloc; ++wi) {
      Work& wk = h->work[wi];
      rc = dev_alloc(h, wk.stream, &wk.xlo, h->cap_tokens * MV_HIDDEN);
      if (rc == MV_OK && hipStreamSynchronize(wk.stream) != hipSuccess) rc = MV_ERR_HIP;
      if (rc != MV_OK) return rc;
    }
  }
  if (precise) {  // fp8 planes [lo8 | hi8] of the three activations that are GEMM A operands
    if (h->gemm_tile == 128) return fail(h, MV_ERR_STATE, "MV_F16X8 runs on the persistent GEMM path: MEMVUL_GEMM_TILE=128 excludes it");
    for (int wi = 0; wi < h->n_alloc; ++wi) {
      Work& wk = h->work[wi];
      rc = dev_alloc(h, wk.stream, &wk.x8, h->cap_tokens * 2 * MV_HIDDEN);
      if (rc == MV_OK) rc = dev_alloc(h, wk.stream, &wk.ctx8, h->cap_tokens * 2 * MV_HIDDEN);
      if (rc == MV_OK) rc = dev_alloc(h, wk.stream, &wk.h8, h->cap_tokens * 2 * MV_INTER);
      if (rc == MV_OK) rc = dev_alloc(h, wk.stream, &wk.ch32, (int64_t)round_up(h->cfg.max_batch, 256) * MV_INTER);
      if (rc == MV_OK) rc = dev_alloc(h, wk.stream, &wk.cls_lo, 2 * (int64_t)round_up(h->cfg.max_batch, 256) * MV_INTER);
      if (rc == MV_OK) rc = dev_alloc(h, wk.stream, &wk.cls_corr, 2 * (int64_t)round_up(h->cfg.max_batch, 256) * MV_INTER);
      if (rc == MV_OK) rc = dev_alloc(h, wk.stream, &wk.st_lo, 2 * (int64_t)round_up(h->cfg.max_batch, 256) * MV_HIDDEN);
      if (rc == MV_OK) rc = dev_alloc(h, wk.stream, &wk.vlo_sp, (int64_t)h->cfg.max_batch * MV_HEADS * MV_HEAD_DIM * 2);
      if (rc == MV_OK) rc = dev_alloc(h, wk.stream, &wk.tile_both, h->cap_tokens / 256 + 1);
      // second fp16 planes of V^T, Q, K: read by passes of padded length <= 128 in the default form, by every pass in the safe form (attention_v2.h VLO)
      if (rc == MV_OK) rc = dev_alloc(h, wk.stream, &wk.vt_lo, h->cap_tokens * MV_HIDDEN);
      if (rc == MV_OK) rc = dev_alloc(h, wk.stream, &wk.q_lo, h->cap_tokens * MV_HIDDEN);
      if (rc == MV_OK) rc = dev_alloc(h, wk.stream, &wk.k_lo, h->cap_tokens * MV_HIDDEN);
      if (rc == MV_OK && hipStreamSynchronize(wk.stream) != hipSuccess) rc = MV_ERR_HIP;
      if (rc != MV_OK) return rc;
    }
  }
  h->precise = precise;
  h->f32 = f32;
  h->staged.clear();
  h->compute_dtype = compute_dtype;
  h->finalized = true;
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_anchor_reset(mv_handle* h) try {
  if (!h) return MV_ERR_INVALID;
  if (h->c_pending) {
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

// ---- resident corpus ---------------------------------------------------------------------------
// mv_corpus_keep in force at a run against G anchors: k checked against the bank, and the arrays allocated at the first such run (like c_psame).  The zeroing
// runs on set 0's stream and the batches may start on the other one: it is waited for here, once.
static int keep_prepare(mv_handle* h, int G) {
  const int k = h->c_k;
  if (!h->c_keep_embed && !k) return MV_OK;
  if (k > G) return fail(h, MV_ERR_INVALID, "mv_corpus_run: the kept top-k (mv_corpus_keep) exceeds the number of anchors");
  if ((int64_t)(G <= 128 ? 1 : (G + 255) / 256) * k > 1024) return fail(h, MV_ERR_INVALID, "top-k: anchors / 256 * k must not exceed 1024");
  const hipStream_t s0 = h->work[0].stream;
  bool fresh = false;
  auto alloc = [&](auto** p, int64_t count, const char* what) -> int {
    if (*p) return MV_OK;
    fresh = true;
    const int rc = dev_alloc(h, s0, p, count);
    if (rc != MV_ERR_NOMEM) return rc;
    return fail(h, MV_ERR_NOMEM, "mv_corpus_run: cannot allocate " + std::to_string((long long)count * 4) + " bytes for the kept " + what + " (mv_corpus_keep): " + h->err);
  };
  if (h->c_keep_embed)
    if (int rc = alloc(&h->c_embed, h->c_n * h->P, "embeddings")) return rc;
  if (k) {
    if (int rc = alloc(&h->c_topk_p, h->c_n * k, "top-k probabilities")) return rc;
    if (int rc = alloc(&h->c_topk_idx, h->c_n * k, "top-k indices")) return rc;
  }
  if (fresh) HIPCHK(h, hipStreamSynchronize(s0));
  return MV_OK;
}

int mv_corpus_upload(mv_handle* h, const int32_t* ids, const int32_t* lens, int64_t n, int S) try {
  if (int rc = check_ready(h)) return rc;
  if (!ids || !lens || n <= 0 || S <= 0 || S > h->cfg.max_pos) return fail(h, MV_ERR_INVALID, "mv_corpus_upload: bad argument");
  if (int rc = check_ids(h, ids, n * S, "mv_corpus_upload")) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const hipStream_t s0 = h->work[0].stream;
  HIPCHK(h, hipStreamSynchronize(s0));
  dev_free(h, h->c_ids); dev_free(h, h->c_lens); dev_free(h, h->c_best); dev_free(h, h->c_idx); dev_free(h, h->c_psame); dev_free(h, h->c_over);
  h->c_ids = nullptr; h->c_lens = nullptr; h->c_best = nullptr; h->c_idx = nullptr; h->c_psame = nullptr; h->c_over = nullptr;
  dev_free(h, h->c_route_dev);
  h->c_route_dev = nullptr;
  h->c_route_stale = true;
  h->c_idx_live.clear();
  h->c_pending = false;
  h->c_psame_rows = 0;
  dev_free(h, h->c_embed); dev_free(h, h->c_topk_p); dev_free(h, h->c_topk_idx);  // mv_corpus_keep: back to (0, 0)
  h->c_embed = nullptr; h->c_topk_p = nullptr; h->c_topk_idx = nullptr;
  h->c_keep_embed = 0; h->c_k = 0; h->c_ran = false;
  h->c_has.clear();
  if (int rc = dev_alloc(h, s0, &h->c_ids, n * S, false)) return rc;
  if (int rc = dev_alloc(h, s0, &h->c_lens, n, false)) return rc;
  if (int rc = dev_alloc(h, s0, &h->c_best, n * 2)) return rc;
  if (int rc = dev_alloc(h, s0, &h->c_idx, n)) return rc;
  if (int rc = dev_alloc(h, s0, &h->c_over, n)) return rc;
  h->c_pend_w.assign((size_t)n, 0);
  h->c_pend_keep.assign((size_t)n, 0);
  h->c_pend_force.assign((size_t)n, 0);
  h->c_forms.assign((size_t)n, MV_FORM_DEFAULT);
  HIPCHK(h, hipMemcpyAsync(h->c_ids, ids, (size_t)n * S * 4, hipMemcpyHostToDevice, s0));
  HIPCHK(h, hipMemcpyAsync(h->c_lens, lens, (size_t)n * 4, hipMemcpyHostToDevice, s0));
  HIPCHK(h, hipStreamSynchronize(s0));
  h->c_lens_host.assign(lens, lens + n);
  h->c_n = n;
  h->c_S = S;
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_corpus_run(mv_handle* h, int64_t first, int64_t count, int batch, int keep_probs) try {
  return mv_corpus_run_len(h, first, count, batch, keep_probs, 0);
} catch (...) { return on_exception(h); }

int mv_corpus_run_len(mv_handle* h, int64_t first, int64_t count, int batch, int keep_probs, int s_eff) try {
  if (!h) return MV_ERR_INVALID;
  if (!h->finalized) return fail(h, MV_ERR_STATE, "weights not finalized (mv_finalize_weights)");
  if (!h->c_ids) return fail(h, MV_ERR_STATE, "no resident corpus (mv_corpus_upload)");
  if (first < 0 || count <= 0 || first + count > h->c_n || count > INT32_MAX || batch <= 0) return fail(h, MV_ERR_INVALID, "mv_corpus_run: bad range");
  if (h->n_anchors <= 0) return fail(h, MV_ERR_STATE, "anchor bank is empty");
  HIPCHK(h, hipSetDevice(h->device));
  if (s_eff < 0 || s_eff > h->c_S) return fail(h, MV_ERR_INVALID, "mv_corpus_run_len: s_eff must be in [0, S of the resident corpus]");
  // tokens per row actually processed (rows longer than this must not be in the range); a batch larger than one pass holds is walked in passes (as
  // mv_forward / mv_encode do): a row's result does not depend on the batch it travels in (bit-identical, tests/test_gpu_parity.py::test_full_batch_properties)
  const int S_use = s_eff > 0 ? s_eff : h->c_S;
  Plan& pl = h->plan;
  if (int rc = plan_batch(h, h->c_lens_host.data() + first, (int)count, S_use, 0, false, batch, pl)) return rc;
  const int G = h->n_anchors;
  if (keep_probs && (h->c_psame_rows != h->c_n || h->c_G != G)) {
    if (int rc = sync_all(h)) return rc;
    dev_free(h, h->c_psame);
    h->c_psame = nullptr;
    if (int rc = dev_alloc(h, h->work[0].stream, &h->c_psame, h->c_n * G)) return rc;
    h->c_psame_rows = h->c_n;
    h->c_G = G;
  }
  if (int rc = keep_prepare(h, G)) return rc;
  h->c_ran = true;
  // consecutive batches (also across calls) alternate between the two workspace sets / streams: two batches are in
  // flight at once; their results go to disjoint slices of the resident arrays
  Job j;
  j.c_row = first; j.keep_psame = keep_probs != 0;
  job_form(h, j);
  if (h->c_embed) j.u_dev = h->c_embed + (size_t)first * h->P;  // a keeping sweep: the encoder writes the rows' slots, the matcher reads them there
  j.topk = h->c_k;
  if (!h->c_has.empty()) std::fill(h->c_has.begin() + first, h->c_has.begin() + first + count, (uint8_t)1);
  // ... with a sink-token list: the rows it routes run in no batch here, they are marked pending and forced (rescore_corpus encodes them in the safe form)
  const bool route = j.guard && !h->sink_tokens.empty();
  if (route)
    if (int rc = ensure_route_flags(h)) return rc;
  // the guarded form: the sweep stays asynchronous and only records the per-row counts (c_over) and what it ran (c_pend_w): rescore_corpus, from mv_corpus_results
  for (int64_t r = first; r < first + count; ++r) {
    h->c_pend_force[(size_t)r] = (uint8_t)(route && h->c_route[(size_t)r]);
    h->c_pend_w[(size_t)r] = (int16_t)(j.guard ? S_use : 0);
    h->c_pend_keep[(size_t)r] = (uint8_t)(keep_probs != 0);
    h->c_forms[(size_t)r] = (uint8_t)(j.safe ? MV_FORM_SAFE : MV_FORM_DEFAULT);
  }
  if (j.guard) { h->c_pending = true; h->guard_seqs += count; }
  for (size_t i = 0; i < pl.passes.size(); ++i) {
    Work& wk = h->work[h->rr];
    wk.sweep = true;
    if (h->n_streams == 2) h->rr ^= 1;
    const Pass& p = pl.passes[i];
    const uint8_t* f = route ? h->c_route.data() + first + p.first : nullptr;
    if (f && std::find(f, f + p.rows, (uint8_t)1) != f + p.rows) {  // (a batch with no routed row takes the in-place path)
      if (int rc = run_split_batch(h, wk, p, j)) return rc;
      continue;
    }
    if (int rc = run_passes(h, wk, pl, i, i + 1, j)) return rc;
  }
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_corpus_results(mv_handle* h, int64_t first, int64_t count, float* best, int32_t* best_idx, float* p_same) try {
  if (!h) return MV_ERR_INVALID;
  if (!h->c_ids) return fail(h, MV_ERR_STATE, "no resident corpus (mv_corpus_upload)");
  if (first < 0 || count <= 0 || first + count > h->c_n) return fail(h, MV_ERR_INVALID, "mv_corpus_results: bad range");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = sync_all(h)) return rc;
  if (int rc = rescore_corpus(h)) return rc;
  const hipStream_t s0 = h->work[0].stream;
  if (best) HIPCHK(h, hipMemcpyAsync(best, h->c_best + (size_t)first * 2, (size_t)count * 8, hipMemcpyDeviceToHost, s0));
  if (best_idx) HIPCHK(h, hipMemcpyAsync(best_idx, h->c_idx + first, (size_t)count * 4, hipMemcpyDeviceToHost, s0));
  if (p_same) {
    if (!h->c_psame) return fail(h, MV_ERR_STATE, "P(same) was not kept (mv_corpus_run keep_probs=0)");
    HIPCHK(h, hipMemcpyAsync(p_same, h->c_psame + (size_t)first * h->c_G, (size_t)count * h->c_G * 4, hipMemcpyDeviceToHost, s0));
  }
  HIPCHK(h, hipStreamSynchronize(s0));
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_corpus_keep(mv_handle* h, int keep_embed, int topk) try {
  if (int rc = check_ready(h)) return rc;
  if (!h->c_ids) return fail(h, MV_ERR_STATE, "no resident corpus (mv_corpus_upload)");
  if ((keep_embed != 0 && keep_embed != 1) || topk < 0 || topk > MK_KMAX) return fail(h, MV_ERR_INVALID, "mv_corpus_keep: keep_embed must be 0 or 1, topk in [0, 64]");
  if (h->c_ran) return fail(h, MV_ERR_STATE, "mv_corpus_keep: the corpus has been swept already (call it after mv_corpus_upload, before the first mv_corpus_run)");
  h->c_keep_embed = keep_embed;
  h->c_k = topk;
  if (keep_embed || topk) h->c_has.assign((size_t)h->c_n, 0); else h->c_has.clear();
  return MV_OK;
} catch (...) { return on_exception(h); }

// The checks the three readers of the kept arrays share: a corpus, a range inside it, every row of it covered by a keeping run — then what mv_corpus_results
// collects first (the sweeps in flight, the guarded form's rescoring).
static int kept_rows_ready(mv_handle* h, const char* who, int64_t first, int64_t count, bool kept) {
  if (!h->c_ids) return fail(h, MV_ERR_STATE, "no resident corpus (mv_corpus_upload)");
  if (!kept) return fail(h, MV_ERR_STATE, std::string(who) + ": the corpus does not keep that (mv_corpus_keep)");
  if (first < 0 || count <= 0 || first + count > h->c_n || count > INT32_MAX) return fail(h, MV_ERR_INVALID, std::string(who) + ": bad range");
  for (int64_t r = first; r < first + count; ++r)
    if (!h->c_has[(size_t)r]) return fail(h, MV_ERR_STATE, std::string(who) + ": row " + std::to_string((long long)r) + " has not been swept by a keeping run");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = sync_all(h)) return rc;
  return rescore_corpus(h);
}

int mv_corpus_rematch(mv_handle* h, int64_t first, int64_t count, int g_first, int keep_probs) try {
  if (int rc = check_ready(h)) return rc;
  if (!h->c_ids) return fail(h, MV_ERR_STATE, "no resident corpus (mv_corpus_upload)");
  if (!h->c_embed) return fail(h, MV_ERR_STATE, "mv_corpus_rematch: no embeddings kept (mv_corpus_keep before the sweep)");
  const int G = h->n_anchors, k = h->c_k;
  if (G <= 0) return fail(h, MV_ERR_STATE, "anchor bank is empty");
  if (g_first < 0 || g_first > G) return fail(h, MV_ERR_INVALID, "mv_corpus_rematch: g_first must be in [0, number of anchors]");
  if (keep_probs != 0 && keep_probs != 1) return fail(h, MV_ERR_INVALID, "mv_corpus_rematch: keep_probs must be 0 or 1");
  if (keep_probs && g_first > 0) return fail(h, MV_ERR_INVALID, "mv_corpus_rematch: keep_probs needs g_first == 0 (the pitch of the P(same) rows changes with the bank)");
  if (k > G) return fail(h, MV_ERR_INVALID, "mv_corpus_rematch: the kept top-k exceeds the number of anchors");
  if (int rc = kept_rows_ready(h, "mv_corpus_rematch", first, count, true)) return rc;
  if (g_first == G) return MV_OK;  // nothing was appended
  Work& wk = h->work[0];
  const size_t P = (size_t)h->P;
  if (keep_probs && (h->c_psame_rows != h->c_n || h->c_G != G)) {  // as mv_corpus_run_len
    dev_free(h, h->c_psame);
    h->c_psame = nullptr;
    if (int rc = dev_alloc(h, wk.stream, &h->c_psame, h->c_n * G)) return rc;
    h->c_psame_rows = h->c_n;
    h->c_G = G;
  }
  auto run = [&]() -> int {
    for (int64_t r = first; r < first + count; r += h->cfg.max_batch) {
      const int nb = (int)std::min<int64_t>(h->cfg.max_batch, first + count - r);
      const float* u = h->c_embed + (size_t)r * P;  // read in place
      if (g_first == 0) {  // full: the stored results rewritten
        if (int rc = match_dev(h, wk, u, nb, G, nullptr, nullptr, keep_probs ? h->c_psame + (size_t)r * G : nullptr, k ? k : 1, h->c_best + r * 2, h->c_idx + r,
                               k ? h->c_topk_p + r * k : nullptr, k ? h->c_topk_idx + r * k : nullptr)) return rc;
        continue;
      }
      // appended: the new anchors alone into the workspace, then folded into the stored results
      const int ks = k ? std::min(k, G - g_first) : 0;
      if (int rc = match_dev(h, wk, u, nb, G - g_first, nullptr, nullptr, nullptr, ks ? ks : 1, wk.best, wk.best_idx, ks ? wk.topk_p : nullptr, ks ? wk.topk_idx : nullptr,
                             g_first)) return rc;
      RematchMergeArgs a{nb, k, ks, g_first, h->cfg.same_idx, wk.best, wk.best_idx, wk.topk_p, wk.topk_idx, h->c_best + r * 2, h->c_idx + r,
                         k ? h->c_topk_p + r * k : nullptr, k ? h->c_topk_idx + r * k : nullptr};
      ProfScope ps(h, wk.stream, KC_TOPK);
      hipLaunchKernelGGL(rematch_merge_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, wk.stream, a);
      if (int rc = launch_check(h, "rematch_merge")) return rc;
    }
    return MV_OK;
  };
  const int rc = run();
  const hipError_t e = hipStreamSynchronize(wk.stream);
  if (rc != MV_OK) return rc;
  HIPCHK(h, e);
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_corpus_embeddings(mv_handle* h, int64_t first, int64_t count, float* embed) try {
  if (int rc = check_ready(h)) return rc;
  if (int rc = kept_rows_ready(h, "mv_corpus_embeddings", first, count, h->c_keep_embed != 0)) return rc;
  if (!embed) return fail(h, MV_ERR_INVALID, "mv_corpus_embeddings: bad argument");
  const hipStream_t s0 = h->work[0].stream;
  HIPCHK(h, hipMemcpyAsync(embed, h->c_embed + (size_t)first * h->P, (size_t)count * h->P * 4, hipMemcpyDeviceToHost, s0));
  HIPCHK(h, hipStreamSynchronize(s0));
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_corpus_topk(mv_handle* h, int64_t first, int64_t count, float* topk_p, int32_t* topk_idx) try {
  if (int rc = check_ready(h)) return rc;
  if (int rc = kept_rows_ready(h, "mv_corpus_topk", first, count, h->c_k > 0)) return rc;
  if (!topk_p || !topk_idx) return fail(h, MV_ERR_INVALID, "mv_corpus_topk: bad argument");
  const hipStream_t s0 = h->work[0].stream;
  const size_t k = (size_t)h->c_k;
  HIPCHK(h, hipMemcpyAsync(topk_p, h->c_topk_p + (size_t)first * k, (size_t)count * k * 4, hipMemcpyDeviceToHost, s0));
  HIPCHK(h, hipMemcpyAsync(topk_idx, h->c_topk_idx + (size_t)first * k, (size_t)count * k * 4, hipMemcpyDeviceToHost, s0));
  HIPCHK(h, hipStreamSynchronize(s0));
  return MV_OK;
} catch (...) { return on_exception(h); }

// ---- multi-GPU exchange: RCCL bound directly ---------------------------------------------------
// librccl.so is opened at run time (never linked).  The unique id is drawn by rank 0 (mv_comm_unique_id) and handed to every
// rank's mv_comm_init as BYTES: how they travel is the host's business (memvul_amd/distributed.py broadcasts them over its
// rendezvous socket — no id file in a shared temp directory, no single-node assumption).
int mv_comm_prepare(mv_handle* h) try {
  if (!h) return MV_ERR_INVALID;
  if (h->rccl_lib) return MV_OK;
  for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
    h->rccl_lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
    if (h->rccl_lib) break;
  }
  if (!h->rccl_lib) return fail(h, MV_ERR_HIP, std::string("mv_comm_prepare: cannot open librccl.so: ") + dlerror());
#define RCCL_SYM(name)                                                                   \
  h->p_##name = (decltype(&name))dlsym(h->rccl_lib, #name);                            \
  if (!h->p_##name) { dlclose(h->rccl_lib); h->rccl_lib = nullptr; return fail(h, MV_ERR_HIP, "mv_comm_prepare: librccl.so lacks " #name); }
  RCCL_SYM(ncclGetUniqueId);
  RCCL_SYM(ncclCommInitRank);
  RCCL_SYM(ncclAllGather);
  RCCL_SYM(ncclCommDestroy);
  RCCL_SYM(ncclGetErrorString);
#undef RCCL_SYM
  h->p_ncclGetVersion = (decltype(&ncclGetVersion))dlsym(h->rccl_lib, "ncclGetVersion");
  h->p_ncclCommCount = (decltype(&ncclCommCount))dlsym(h->rccl_lib, "ncclCommCount");
  h->p_ncclCommUserRank = (decltype(&ncclCommUserRank))dlsym(h->rccl_lib, "ncclCommUserRank");
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_comm_unique_id(mv_handle* h, void* id_out, int capacity) try {
  if (!h || !id_out) return MV_ERR_INVALID;
  if (capacity < (int)sizeof(ncclUniqueId)) return fail(h, MV_ERR_INVALID, "mv_comm_unique_id: buffer smaller than ncclUniqueId (128 bytes)");
  if (int rc = mv_comm_prepare(h)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  ncclUniqueId id;
  ncclResult_t r = h->p_ncclGetUniqueId(&id);
  if (r != ncclSuccess) return fail(h, MV_ERR_HIP, std::string("ncclGetUniqueId: ") + h->p_ncclGetErrorString(r));
  std::memcpy(id_out, &id, sizeof(id));
  return (int)sizeof(id);
} catch (...) { return on_exception(h); }

int mv_comm_init(mv_handle* h, int rank, int world, const void* id, int id_bytes) try {
  if (!h || world < 1 || rank < 0 || rank >= world) return fail(h, MV_ERR_INVALID, "mv_comm_init: bad rank / world");
  if (h->comm) return fail(h, MV_ERR_STATE, "mv_comm_init: communicator already initialised");
  // rank / world are recorded only once the init has SUCCEEDED: a failed init leaves the handle in its one-rank state (the
  // gather is then a copy) instead of a world without a communicator
  if (world == 1 && !id) { h->comm_rank = 0; h->comm_world = 1; return MV_OK; }  // no transport needed (with an id: a real 1-rank communicator, the GPU-box test)
  if (!id || id_bytes != (int)sizeof(ncclUniqueId)) return fail(h, MV_ERR_INVALID, "mv_comm_init: the 128-byte unique id of rank 0 (mv_comm_unique_id) is required");
  if (int rc = mv_comm_prepare(h)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  ncclResult_t r = h->p_ncclCommInitRank(&h->comm, world, uid, rank);
  if (r != ncclSuccess) { h->comm = nullptr; return fail(h, MV_ERR_HIP, std::string("ncclCommInitRank: ") + h->p_ncclGetErrorString(r)); }
  h->comm_rank = rank;
  h->comm_world = world;
  return MV_OK;
} catch (...) { return on_exception(h); }

// What the transport IS, as RCCL itself reports it: info[0] = ranks of the live communicator by ncclCommCount (0: no
// communicator — one rank, or the run is on another transport), info[1] = this rank in it by ncclCommUserRank, info[2] = the
// RCCL version code of ncclGetVersion (0 while librccl.so is not open), info[3] = the world mv_comm_allgather will gather over.
int mv_comm_info(mv_handle* h, int* info, int n) try {
  if (!h || !info || n < 4) return fail(h, MV_ERR_INVALID, "mv_comm_info: int[4] required");
  info[0] = info[1] = info[2] = 0;
  info[3] = h->comm_world;
  if (h->rccl_lib && h->p_ncclGetVersion) { int v = 0; if (h->p_ncclGetVersion(&v) == ncclSuccess) info[2] = v; }
  if (h->comm) {
    int c = -1, r = -1;
    if (h->p_ncclCommCount && h->p_ncclCommCount(h->comm, &c) == ncclSuccess) info[0] = c;
    if (h->p_ncclCommUserRank && h->p_ncclCommUserRank(h->comm, &r) == ncclSuccess) info[1] = r;
  }
  return MV_OK;
} catch (...) { return on_exception(h); }

// GPUs visible to this process (hipGetDeviceCount): 0 on a box without one (a HIP error there is "none", not a failure).
int mv_device_count(void) try {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
} catch (...) { return on_exception(nullptr); }

int mv_comm_allgather(mv_handle* h, const void* send, void* recv, int64_t bytes_per_rank) try {
  if (!h || !send || !recv || bytes_per_rank <= 0) return fail(h, MV_ERR_INVALID, "mv_comm_allgather: bad argument");
  if (h->comm_world == 1 && !h->comm) { std::memcpy(recv, send, (size_t)bytes_per_rank); return MV_OK; }
  if (!h->comm) return fail(h, MV_ERR_STATE, "mv_comm_allgather: mv_comm_init first");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = sync_all(h)) return rc;
  hipStream_t st = h->work[0].stream;
  const int64_t total = bytes_per_rank * h->comm_world;
  if (h->comm_send_cap < bytes_per_rank) {
    if (h->comm_send) hipFree(h->comm_send);
    h->comm_send = nullptr; h->comm_send_cap = 0;
    HIPCHK(h, hipMalloc(&h->comm_send, (size_t)bytes_per_rank));
    h->comm_send_cap = bytes_per_rank;
  }
  if (h->comm_recv_cap < total) {
    if (h->comm_recv) hipFree(h->comm_recv);
    h->comm_recv = nullptr; h->comm_recv_cap = 0;
    HIPCHK(h, hipMalloc(&h->comm_recv, (size_t)total));
    h->comm_recv_cap = total;
  }
  HIPCHK(h, hipMemcpyAsync(h->comm_send, send, (size_t)bytes_per_rank, hipMemcpyHostToDevice, st));
  ncclResult_t r = h->p_ncclAllGather(h->comm_send, h->comm_recv, (size_t)bytes_per_rank, ncclChar, h->comm, st);
  if (r != ncclSuccess) return fail(h, MV_ERR_HIP, std::string("ncclAllGather: ") + h->p_ncclGetErrorString(r));
  HIPCHK(h, hipMemcpyAsync(recv, h->comm_recv, (size_t)total, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_comm_destroy(mv_handle* h) try {
  if (!h) return MV_ERR_INVALID;
  (void)hipSetDevice(h->device);
  if (h->comm) { h->p_ncclCommDestroy(h->comm); h->comm = nullptr; }
  if (h->comm_send) { hipFree(h->comm_send); h->comm_send = nullptr; h->comm_send_cap = 0; }
  if (h->comm_recv) { hipFree(h->comm_recv); h->comm_recv = nullptr; h->comm_recv_cap = 0; }
  h->comm_world = 1; h->comm_rank = 0;
  return MV_OK;
} catch (...) { return on_exception(h); }

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
  h->c_route_stale = true;
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

int mv_corpus_route_flags(mv_handle* h, int64_t first, int64_t count, uint8_t* flags) try {
  if (!h || !flags) return fail(h, MV_ERR_INVALID, "mv_corpus_route_flags: bad argument");
  if (!h->c_ids) return fail(h, MV_ERR_STATE, "no resident corpus (mv_corpus_upload)");
  if (first < 0 || count <= 0 || first + count > h->c_n) return fail(h, MV_ERR_INVALID, "mv_corpus_route_flags: bad range");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = ensure_route_flags(h)) return rc;
  std::memcpy(flags, h->c_route.data() + first, (size_t)count);
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_last_row_forms(mv_handle* h, uint8_t* forms, int n) try {
  if (!h || !forms || n < 0 || (size_t)n != h->last_forms.size()) return fail(h, MV_ERR_INVALID, "mv_last_row_forms: n is not the row count of the last call");
  std::memcpy(forms, h->last_forms.data(), (size_t)n);
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_corpus_row_forms(mv_handle* h, int64_t first, int64_t count, uint8_t* forms) try {
  if (!h || !forms) return fail(h, MV_ERR_INVALID, "mv_corpus_row_forms: bad argument");
  if (!h->c_ids) return fail(h, MV_ERR_STATE, "no resident corpus (mv_corpus_upload)");
  if (first < 0 || count <= 0 || first + count > h->c_n) return fail(h, MV_ERR_INVALID, "mv_corpus_row_forms: bad range");
  if (h->c_pending) return fail(h, MV_ERR_STATE, "mv_corpus_row_forms: a guarded sweep has not been collected yet (mv_corpus_results)");
  std::memcpy(forms, h->c_forms.data() + first, (size_t)count);
  return MV_OK;
} catch (...) { return on_exception(h); }

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
  const int64_t T = (int64_t)h->dbg_B * h->dbg_Sp;
  const void* src = nullptr;
  int64_t avail = 0;
  if (h->f32 && buffer >= 1 && buffer <= 9)
    return fail(h, MV_ERR_INVALID, "mv_debug_read: buffers 1 - 9 are the fp16 planes of MV_F16 / MV_F16X8; an MV_F32 handle has buffer 0 (hidden fp32) and 10 (embedding)");
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

// ---- JSON-lines records of one batch (host only) --------------------------------------------------------------------------------------
// Python's repr(float) — what json.dumps prints for every probability of make_output_human_readable's records (model_memory.py:169-191 ->
// predict_memory.py:111) — restated: the shortest digit string that round-trips the double (std::to_chars, scientific) laid out by CPython's rule
// (PyOS_double_to_string 'r': exponent form when the decimal exponent is < -4 or >= 16, at least two exponent digits, ".0" after a whole number).
// 0.65 us per double in CPython, ~40 ns here; pinned to repr() on millions of values by tests/test_host_logic.py.
static inline char* py_repr_double(char* o, double v) {
  if (v == 0.0) {
    if (std::signbit(v)) *o++ = '-';
    *o++ = '0'; *o++ = '.'; *o++ = '0';
    return o;
  }
  char b[40];
  const auto r = std::to_chars(b, b + sizeof b, v, std::chars_format::scientific);  // [-]d[.ddd]e[+-]XX
  const char* p = b;
  if (*p == '-') *o++ = *p++;
  char dig[24];
  int nd = 0;
  dig[nd++] = *p++;
  if (*p == '.') {
    ++p;
    while (*p != 'e') dig[nd++] = *p++;
  }
  ++p;  // 'e'
  const bool eneg = *p == '-';
  ++p;
  int e = 0;
  while (p < r.ptr) e = e * 10 + (*p++ - '0');
  if (eneg) e = -e;
  if (e < -4 || e >= 16) {
    *o++ = dig[0];
    if (nd > 1) {
      *o++ = '.';
      for (int i = 1; i < nd; ++i) *o++ = dig[i];
    }
    *o++ = 'e';
    *o++ = e < 0 ? '-' : '+';
    const int ae = e < 0 ? -e : e;
    if (ae >= 100) *o++ = (char)('0' + ae / 100);
    *o++ = (char)('0' + (ae / 10) % 10);
    *o++ = (char)('0' + ae % 10);
  } else if (e < 0) {
    *o++ = '0'; *o++ = '.';
    for (int i = 0; i < -e - 1; ++i) *o++ = '0';
    for (int i = 0; i < nd; ++i) *o++ = dig[i];
  } else {
    for (int i = 0; i <= e; ++i) *o++ = i < nd ? dig[i] : '0';
    *o++ = '.';
    if (nd > e + 1) for (int i = e + 1; i < nd; ++i) *o++ = dig[i];
    else *o++ = '0';
  }
  return o;
}

// out = "[" + ", ".join(prefix_i + piece_0 + repr(p[i][0]) + piece_1 + repr(p[i][1]) + ... + row_suffix) + "]"
int mv_format_records(const char* prefixes, const int64_t* prefix_off, int64_t rows, const char* pieces, const int64_t* piece_off, int64_t cols,
                      const char* row_suffix, const double* p, char* out, int64_t cap, int64_t* written) try {
  if (!prefixes || !prefix_off || !pieces || !piece_off || !row_suffix || !p || !out || !written || rows < 0 || cols < 0) return MV_ERR_INVALID;
  const int64_t nsuf = (int64_t)std::strlen(row_suffix);
  const int64_t piece_bytes = piece_off[cols] - piece_off[0];
  char* o = out;
  char* const end = out + cap;
  if (end - o < 2) return MV_ERR_CAPACITY;
  *o++ = '[';
  for (int64_t i = 0; i < rows; ++i) {
    const int64_t np_ = prefix_off[i + 1] - prefix_off[i];
    if (end - o < np_ + piece_bytes + cols * 26 + nsuf + 4) return MV_ERR_CAPACITY;  // (a repr is at most 24 characters)
    if (i) { *o++ = ','; *o++ = ' '; }
    std::memcpy(o, prefixes + prefix_off[i], (size_t)np_);
    o += np_;
    const double* row = p + i * cols;
    for (int64_t c = 0; c < cols; ++c) {
      const int64_t n = piece_off[c + 1] - piece_off[c];
      std::memcpy(o, pieces + piece_off[c], (size_t)n);
      o += n;
      if (!std::isfinite(row[c])) return MV_ERR_INVALID;  // json spells these NaN / Infinity: the caller's Python path does
      o = py_repr_double(o, row[c]);
    }
    std::memcpy(o, row_suffix, (size_t)nsuf);
    o += nsuf;
  }
  *o++ = ']';
  *written = o - out;
  return MV_OK;
} catch (...) { return on_exception(nullptr); }

// ---- the device WordPiece tokenizer ------------------------------------------------------------------------------------------------------------------------------
int mv_tok_create(int device, const char* vocab_bytes, const int64_t* vocab_off, int n_vocab, const char* literal_bytes, const int64_t* literal_off,
                  int n_literals, int unk_id, int cls_id, int sep_id, int max_chars_per_word, int lowercase, mv_tokenizer** out) try {
  if (!out) return tok_fail(nullptr, MV_ERR_INVALID, "mv_tok_create: out is NULL");
  *out = nullptr;
  mv_tokenizer* t = new mv_tokenizer();
  struct Guard {  // whatever leaves this function early, an exception included, releases the object
    mv_tokenizer* t;
    ~Guard() { if (t) tok_release(t); }
  } guard{t};
  std::string err;
  if (!wp_build(t->host, vocab_bytes, vocab_off, n_vocab, literal_bytes, literal_off, n_literals, unk_id, cls_id, sep_id, max_chars_per_word, lowercase, err))
    return tok_fail(nullptr, MV_ERR_INVALID, err);
  if (device >= 0) {
    t->device = device;
    const WpHost& H = t->host;
    auto up = [&](void** d, const void* src, size_t bytes) -> hipError_t {
      hipError_t e = hipMalloc(d, bytes);
      return e != hipSuccess ? e : hipMemcpy(*d, src, bytes, hipMemcpyHostToDevice);
    };
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&t->ev0);
    if (e == hipSuccess) e = hipEventCreate(&t->ev1);
    if (e == hipSuccess) e = up(&t->d_slots, H.slots.data(), H.slots.size() * sizeof(WpSlot));
    if (e == hipSuccess) e = up(&t->d_pool, H.pool.data(), H.pool.size());
    if (e == hipSuccess) e = up(&t->d_lit, H.lit.data(), H.lit.size());
    if (e == hipSuccess) e = up(&t->d_lit_off, H.lit_off.data(), H.lit_off.size() * sizeof(uint32_t));
    if (e != hipSuccess) {
      const std::string msg = std::string("mv_tok_create: ") + hipGetErrorString(e);
      (void)hipGetLastError();
      return tok_fail(nullptr, MV_ERR_HIP, msg);
    }
    t->dev = H.t;
    t->dev.slots = (const WpSlot*)t->d_slots;
    t->dev.pool = (const uint8_t*)t->d_pool;
    t->dev.lit = (const uint8_t*)t->d_lit;
    t->dev.lit_off = (const uint32_t*)t->d_lit_off;
  }
  guard.t = nullptr;
  *out = t;
  return MV_OK;
} catch (...) { return on_exception((mv_tokenizer*)nullptr); }

void mv_tok_destroy(mv_tokenizer* tok) {
  if (tok) tok_release(tok);
}

const char* mv_tok_last_error(mv_tokenizer* tok) { return tok ? tok->err.c_str() : g_create_error.c_str(); }

int mv_tok_encode_host(mv_tokenizer* tok, const char* text, const int64_t* off, int n, int max_length, int add_special, int32_t* ids, int32_t* lens,
                       uint8_t* status) try {
  if (!tok) return tok_fail(nullptr, MV_ERR_INVALID, "mv_tok_encode_host: tok is NULL");
  if (int rc = tok_check_args(tok, "mv_tok_encode_host", text, off, n, max_length, ids, lens, status)) return rc;
  for (int i = 0; i < n; ++i)
    wp_encode_text(tok->host.t, (const uint8_t*)text + off[i], off[i + 1] - off[i], max_length, add_special, ids + (size_t)i * max_length, lens + i, status + i);
  return MV_OK;
} catch (...) { return on_exception(tok); }

int mv_tok_encode(mv_tokenizer* tok, const char* text, const int64_t* off, int n, int max_length, int add_special, int32_t* ids, int32_t* lens,
                  uint8_t* status) try {
  if (!tok) return tok_fail(nullptr, MV_ERR_INVALID, "mv_tok_encode: tok is NULL");
  if (int rc = tok_check_args(tok, "mv_tok_encode", text, off, n, max_length, ids, lens, status)) return rc;
  if (n == 0) return MV_OK;
  if (tok->device < 0) return tok_fail(tok, MV_ERR_STATE, "mv_tok_encode: created without a device (mv_tok_create(device < 0) serves mv_tok_encode_host)");
  TOKHIP(tok, hipSetDevice(tok->device));
  tok->kernel_ms = 0.f;
  const int rc = tok_encode_chunks(tok, text, off, n, max_length, add_special, ids, lens, status);
  if (rc != MV_OK) (void)hipStreamSynchronize(tok->stream);  // nothing queued on the stream writes the caller's arrays after the call has failed
  return rc;
} catch (...) { return on_exception(tok); }

int mv_tok_kernel_ms(mv_tokenizer* tok, float* ms) try {
  if (!tok || !ms) return tok_fail(tok, MV_ERR_INVALID, "mv_tok_kernel_ms: NULL argument");
  *ms = tok->kernel_ms;
  return MV_OK;
} catch (...) { return on_exception(tok); }

}  // extern "C"
