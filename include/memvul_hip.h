/*
 * memvul_hip.h — C ABI of libmemvul_hip.so: the MI355X (gfx950) inference engine for MemVul's
 * predict_memory.py hot loop (BERT issue-encoder forward + CWE golden-anchor memory matching).
 *
 * The reference is pure Python and has no FFI of its own; this header is the boundary a
 * maintainer binds with ctypes from `MemVul/model_memory.py`.  Each entry
 * point names the reference code it replaces (paths relative to the MemVul repository).
 *
 * Conventions
 *   - every function returns MV_OK (0) or a negative mv_status; the message is available from
 *     mv_last_error(); no C++ exception crosses the ABI; HIP errors are captured and translated.
 *   - the caller owns every host buffer; the library owns all device memory (weights, anchor bank,
 *     workspaces, resident corpus).  No device pointer is ever returned.
 *   - one handle <-> one GPU <-> one HIP stream; a handle is not thread-safe; distinct handles are
 *     independent (one process per GPU in multi-GPU runs).
 *   - entry points that launch device work are asynchronous with respect to the host until
 *     mv_sync(), except where they copy results back to host memory (they synchronise first).
 *   - token ids are int32, sequences are 0-padded ([PAD]=0) to S columns, `lens[b]` is the number of
 *     real tokens of row b (the reference's boolean `mask` is `arange(S) < lens[b]`,
 *     custom_PTM_embedder.py:215-228).  S may be any value in [1, max_pos]; the engine pads
 *     internally to a multiple of 64 with masked keys.
 */
#ifndef MEMVUL_HIP_H
#define MEMVUL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mv_handle mv_handle;

typedef enum mv_status {
  MV_OK = 0,
  MV_ERR_INVALID = -1,        /* bad argument / shape */
  MV_ERR_HIP = -2,            /* a HIP runtime call or kernel launch failed */
  MV_ERR_STATE = -3,          /* call order violated (e.g. forward before finalize / no anchors) */
  MV_ERR_MISSING_WEIGHT = -4, /* mv_finalize_weights: a state-dict key was never loaded */
  MV_ERR_CAPACITY = -5,       /* B*S, B or G exceeds what mv_create reserved */
  MV_ERR_NOMEM = -6,          /* host or device allocation failed */
  MV_ERR_INTERNAL = -7        /* a C++ exception was caught at the ABI boundary (never propagated to the caller) */
} mv_status;

/* MV_F32 is a storage dtype of mv_load_tensor AND the third compute dtype of mv_finalize_weights — the reference form: the arithmetic the reference runs
 * (fp32 operands, fp32 accumulation, erf GELU, max-subtracted softmax), on the fp32-input MFMA (v_mfma_f32_32x32x2_f32); 1/16 of the 16-bit matrix rate; for
 * audits and envelope work (memvul_amd/audit.py measures the other compute dtypes against it on the model and the data a user has), not for throughput. */
typedef enum mv_dtype { MV_F32 = 0, MV_F16 = 1, MV_BF16 = 2, MV_I32 = 3, MV_I64 = 4,
                        /* compute dtype only ("precise"): the fp16 MFMA sweep of every encoder GEMM plus ONE correction sweep on the
                         * fp8 matrix path (OCP e4m3, v_mfma_scale_f32_16x16x128_f8f6f4) over the first-order terms of the split-operand
                         * product, A_lo8 W_hi8 + A_hi8 W_lo8 — ~15.5-bit operands at 2x the GEMM main loop: the mode that holds 1e-3 on
                         * the logits in the trained-like regime.  (5 was MV_F16X2, the three-sweep fp16 split
                         * of round 2 that this mode replaces; it is rejected now.) */
                        MV_F16X8 = 6 } mv_dtype;

/* Geometry + capacities.  The kernels are specialised to bert-base geometry (hidden 768, 12 heads
 * of 64, intermediate 3072, header 512); `layers`, `vocab_size`, `max_pos` are free.
 * (HF BertConfig defaults; model hyper-parameters MemVul/config_memory.json:31-49.) */
typedef struct mv_config {
  int32_t vocab_size;   /* 30522 */
  int32_t hidden;       /* 768  (must be 768) */
  int32_t layers;       /* 12 */
  int32_t heads;        /* 12   (must be 12) */
  int32_t intermediate; /* 3072 (must be 3072) */
  int32_t max_pos;      /* 512 */
  int32_t type_vocab;   /* 2 */
  int32_t proj_dim;     /* 512: the header output (FeedForward(768,1,[512],ReLU), model_memory.py:70; use_header = true, every reference
                         * config) — or 768: use_header = false (l.69-73): no `_projector_single`, the embedding is the pooler output
                         * and `_projector.weight` is [2, 3 * 768] */
  float ln_eps;         /* 1e-12 */
  int32_t max_tokens;   /* capacity of one forward in padded tokens, B * Sp (Sp = S rounded up to 64, above 256 to 128) */
  int32_t max_batch;    /* capacity of one forward in issue reports */
  int32_t max_anchors;  /* capacity of the anchor bank (G) */
  int32_t same_idx;     /* index of label "same" in the `labels` vocabulary (model_memory.py:61) */
} mv_config;

/* ---- lifetime ----------------------------------------------------------------------------- */

/* Replaces Model.from_params + model.to(cuda_device) (predict_memory.py:62-70): binds `device`,
 * creates the stream and reserves all workspaces. */
/* Environment switches read HERE — six, each with a tested default, each parsed strictly (a value the library does not understand fails mv_create with a
 * message; a typo never selects other numerics silently):
 *   MEMVUL_CLS_ASIDE          1 (default) | 0.  MV_F16X8: 1 = the [CLS]-row form (every GEMM sweeps the weight-side correction term, the A-side term is
 *                             restored for the [CLS] row of each sequence alone: only that row reaches the pooler, model_memory.py:99); 0 = both first-order
 *                             terms in every row (rounds 3-4: -13 % issue reports/s, same trained-like logit error on diffuse attention).
 *   MEMVUL_CLS_ASIDE_MIN_LEN  1 .. 512 (default 128): sequences shorter than this keep the both-terms form (few keys to average over) — decided per sequence in
 *                             passes of padded length 256 / 512, for the whole pass (by its shortest sequence) at 192 / 384; shorter passes always keep it.
 *   MEMVUL_QKV_ASIDE          a subset of "qkv", "" or "none" (default "none"): the blocks of the QKV projection that sweep the A-side term for EVERY row (the special
 *                             rows get it in every block either way; "q" = the default of rounds 4 - 6a: -2.7 % issue reports/s, 3 % less logit error).
 *   MEMVUL_CLS_PRUNE          1 (default) | 0: after the last layer's K / V projection only the [CLS] rows are processed.
 *   MEMVUL_STREAMS            2 (default) | 1: batches of the resident sweep in flight (mv_set_streams changes it later).
 *   MEMVUL_FORM               default | safe | guarded: the form of MV_F16X8 the handle starts in (mv_set_form changes it later).  "safe" and "guarded" with
 *                             mv_finalize_weights(MV_F16) fail.
 *                             In the safe form MEMVUL_CLS_ASIDE, MEMVUL_CLS_ASIDE_MIN_LEN and MEMVUL_QKV_ASIDE have no effect (it is their most conservative setting).
 * One more switch is read here that selects no numerics: MEMVUL_PP_FORM = fixed (default) | runtime.  MV_F16X8: the persistent GEMMs of a pass of padded length
 * 256 / 512 in the [CLS]-row form with no short sequence take kernels that hold the form of the launch as compile-time constants (libmemvul_pp_fixed.so) and
 * spill less; "runtime" keeps every launch on the kernels that read the form from their arguments.  The outputs are equal bit for bit.  Parsed strictly as well.
 * (The seventh switch of the product, MEMVUL_COMPUTE = precise | f16 | f32 (+ aliases), is read by the Python surface: memvul_amd/binding.py default_compute.)
 * (So are MEMVUL_ON_SINK = warn | safe and MEMVUL_SINK_CENSUS = 0 | 1 — binding.py on_sink_policy / sink_census_policy; the latter calls mv_sink_census_enable
 * after mv_finalize_weights — and MEMVUL_SINK_TOKENS = ID[,ID...] — binding.py sink_tokens_policy: mv_set_sink_tokens after mv_finalize_weights, guarded form only.)
 * Development A/B knobs (kernel path forced at test sizes, raster, grid share, one-plane short passes) exist only in the -DMEMVUL_DEV_SWITCHES build
 * (libmemvul_hip_dev.so: memvul_amd/build.py, loaded by the GPU tests and A/B scripts that need them); this library does not read them. */
int mv_create(int device, const mv_config* cfg, mv_handle** out);
void mv_destroy(mv_handle* h);
/* Last error message of this handle (or of a failed mv_create when h == NULL). */
const char* mv_last_error(mv_handle* h);
int mv_sync(mv_handle* h);

/* ---- weights (replaces model.load_state_dict(weights.th), AllenNLP archival) ---------------- */

/* `name` is a key of the reference model's state_dict:
 *   _text_field_embedder.token_embedder_tokens.transformer_model.<HF BertModel key>
 *   _bert_pooler.pooler.dense.{weight,bias}            (model_memory.py:64)
 *   _projector_single._linear_layers.0.{weight,bias}   (model_memory.py:70)
 *   _projector.weight                                  (model_memory.py:73)
 * Unknown keys (e.g. ...embeddings.position_ids, custom_PTM_embedder.py:64) are accepted and
 * ignored.  dtype MV_F32 / MV_F16 / MV_BF16; the data is copied, the caller may free it. */
int mv_load_tensor(mv_handle* h, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim);
/* Checks that every needed key is present and well-shaped, packs QKV, converts the GEMM weights to
 * `compute_dtype` and uploads.  Compute dtypes: MV_F16X8 (fp16 MFMA sweep + an fp8 correction sweep per GEMM, see mv_dtype:
 * what the Python surface passes by default and what bench.py's headline is measured in — it holds the 1e-3 logit tolerance of
 * model_memory.py:133-147 on trained-like weights) and MV_F16 (one fp16 sweep, fp32 accumulation: the explicit "fast" opt-in,
 * 3.0-5.6e-3 on such weights) and MV_F32 (the reference form, see mv_dtype: the four GEMM weights of every layer stay fp32 and un-folded, Q | K | V, the
 * attention context and the FFN intermediate are fp32 planes allocated here, 6144 floats per token of max_tokens and workspace set; no forms, no monitors — they
 * read 0 —, no last-layer pruning, natural token order; within 3e-5 of a float64 evaluation on the logits); anything else returns
 * MV_ERR_INVALID.  MV_BF16 is a STORAGE dtype of mv_load_tensor only (bf16 checkpoints load): as MFMA
 * operand format it was measured and rejected — 8 significand bits put the match logits 1.5e-2 off at |logit| ~ 3
 * and 2.5e-3 off even on random-init weights (oracle/precision_model.py), against a 1e-3 budget, at the
 * same MFMA rate as fp16.  Embeddings, LayerNorm, biases, pooler, header and matcher stay fp32. */
int mv_finalize_weights(mv_handle* h, int compute_dtype);

/* The three forms of compute dtype MV_F16X8: same weights, same planes, same handle; only the per-pass choices differ.
 *   MV_FORM_DEFAULT  what bench.py's headline is measured in: the [CLS]-row form, the special rows, two fp16 planes through attention up to 128 keys.  Holds 1e-3
 *                    on the logits for diffuse attention and for attention sinks on [CLS] / [SEP].
 *   MV_FORM_SAFE     the form for models whose heads park most of their mass on an ORDINARY token (mv_attention_concentration reports them), where the default reads
 *                    0.8 - 2.7e-3: both first-order correction terms in every row of every GEMM, the A-side term in all three blocks of the QKV projection, and
 *                    Q, K, V, P as hi + lo fp16 planes through attention at EVERY padded length (the sink token's V reaches every row un-averaged: its single-plane
 *                    fp16 storage is what is left otherwise) and through the single-query attention of the pruned last layer.  It costs the GEMMs their A-side sweep
 *                    in every row and attention three times the MFMAs, twice the K / V bytes and one wave per SIMD above 128 keys; rate and error envelope as
 *                    measured: DESIGN.md section 2, profiles/LEDGER.md.
 *   MV_FORM_GUARDED  the choice between the two made per SEQUENCE: every sequence the handle encodes — issue report or anchor — runs in the default form with the
 *                    concentration monitor also counting per sequence; a sequence with more than 2 % of its own monitored (head, layer) items above a collision mass of
 *                    0.25 (mv_attention_concentration; a sequence of fewer than 16 tokens has no items) is encoded AGAIN in the safe form, at the width of the pass it
 *                    first ran in, and only its results are replaced: it gets the bits a safe-form handle gives it through the same call, every other sequence the
 *                    bits of the default form.  mv_forward / mv_forward_ragged / mv_encode / mv_anchor_append rescore before they return, mv_forward_ragged_end
 *                    rescores the batch its ticket was started with (the form is the one in force at `begin`), the resident sweep records the counts while it runs
 *                    and rescores everything swept since, in full batches, before mv_corpus_results copies anything.  The rescoring passes leave the global
 *                    counters of mv_attention_concentration alone (a sequence is counted once).  Costs the default form's rate times (1 + 1.34 f) at a flagged
 *                    share f: above f ~ 0.25 the safe form is the cheaper one.  mv_debug_encode ignores it (taps show the default form).
 *                    With a sink-token list (mv_set_sink_tokens, below) a sequence that carries a listed token is not encoded twice: it skips the default form
 *                    and goes straight into the safe-form pass, next to the sequences the monitor flags.
 * mv_set_form: MV_FORM_SAFE / MV_FORM_GUARDED on a handle finalized as MV_F16 or MV_F32 -> MV_ERR_STATE, an unknown value -> MV_ERR_INVALID.  The form of a pass is read on the
 * host when the pass is enqueued: work already in flight keeps the form it was enqueued with.  mv_get_form returns the current form. */
#define MV_FORM_DEFAULT 0
#define MV_FORM_SAFE 1
#define MV_FORM_GUARDED 2
int mv_set_form(mv_handle* h, int form);
int mv_get_form(mv_handle* h);
/* MV_FORM_GUARDED: *sequences = the sequences encoded in the guarded form since the handle was created (or the last reset), *rescored = how many of them were
 * encoded again in the safe form (corpus rows count as rescored once mv_corpus_results has run their rescoring). */
int mv_form_stats(mv_handle* h, int64_t* sequences, int64_t* rescored, int reset);
/* The form (MV_FORM_DEFAULT / MV_FORM_SAFE) that produced each row of the last mv_forward / mv_forward_ragged / mv_forward_ragged_end / mv_encode /
 * mv_anchor_append, in the caller's row order; n = that call's row count (anything else -> MV_ERR_INVALID).  Outside the guarded form every row reads the
 * handle's form. */
int mv_last_row_forms(mv_handle* h, uint8_t* forms, int n);
/* The same for rows [first, first + count) of the resident corpus: valid after mv_corpus_results (rows never swept read MV_FORM_DEFAULT). */
int mv_corpus_row_forms(mv_handle* h, int64_t first, int64_t count, uint8_t* forms);

/* The sink-token list: ordinary-token sinks are driven by the token (mv_sink_census_read names it), so a sequence that is certain to be flagged
 * can be read off its ids.  THE RULE: a sequence is ROUTED iff one of its tokens at positions 1 .. len - 2 is in the list — positions 0 and len - 1 are [CLS] /
 * [SEP] (the special rows cover them; the census looks at the same positions), ids at positions >= len are padding and never looked at (a list that holds id 0
 * does not route by padding), there is no length gate, and a sequence of len <= 2 has no such position.
 * The list is kept in every form of MV_F16X8 and ACTED ON ONLY IN MV_FORM_GUARDED (the safe form is already safe, the default form stays the default form): there
 * a routed sequence never runs in the default form.  mv_forward / mv_forward_ragged / mv_forward_ragged_begin / mv_encode / mv_anchor_append plan the batch over
 * all its rows as without a list (every row keeps the width of its pass), run the unrouted rows of each pass in the default form with the per-sequence monitor
 * (the pass's shortest-sequence rule, MEMVUL_CLS_ASIDE_MIN_LEN, is taken over the rows that run in it), and encode the routed rows ONCE, in the safe form, in the
 * rescoring passes, together with the unrouted rows the monitor flagged.  A routed sequence gets the bits a safe-form handle gives it through the same call.  The
 * list is read where the form is: when the job is made — a ticket of mv_forward_ragged_begin keeps the routing it was begun with.  On the resident corpus the ids
 * live on the device: one kernel (memvul_amd/csrc/route.h) flags every corpus row under the current list, lazily, at the first mv_corpus_run* or
 * mv_corpus_route_flags after an upload or a list change (a kernel, one copy back, one wait — not per batch); a guarded sweep leaves the routed rows of its
 * range out of its batches and marks them, and the rescoring in front of mv_corpus_results encodes them with the flagged ones; rows swept before a list change keep
 * the routing of their sweep.  mv_debug_encode ignores the list, as it ignores the guarded form.
 * ROUTED SEQUENCES FEED NEITHER mv_attention_concentration NOR THE CENSUS: their only pass is a rescoring pass, which runs with the monitor detached (a sequence
 * is counted once — a routed one not at all: the list already says what the monitor would have).  A sink the list does not name is still caught by the monitor.
 * Empty (the default), the guarded form is what it is without this list, bit for bit, counters included.
 * mv_set_sink_tokens replaces the list: n == 0 clears it (ids may be NULL then), duplicates are allowed; n < 0, n > MV_MAX_SINK_TOKENS, ids == NULL with n > 0 or
 * an id outside [0, mv_config.vocab_size) -> MV_ERR_INVALID, the list unchanged; before mv_finalize_weights, or on a handle finalized as MV_F16 or MV_F32 ->
 * MV_ERR_STATE.  mv_get_sink_tokens returns the list's length (>= 0) and fills up to `capacity` ids.
 * mv_route_stats: *routed = the sequences sent directly to the safe form since the handle was created (or the last reset; corpus rows count once the rescoring
 * in front of mv_corpus_results has encoded them).  mv_form_stats keeps its meaning: *rescored counts only sequences encoded twice — the rows mv_last_row_forms /
 * mv_corpus_row_forms call MV_FORM_SAFE in the guarded form are routed + rescored.
 * mv_route_scan: the rule itself, host only, no handle, no GPU work, callable from any thread: flags[b] = 1 / 0 for the rows of ids [B][S] with lengths lens [B]
 * under the list tokens [n] over a vocabulary of `vocab` ids (a length outside [0, S] is read as clamped; an id outside the vocabulary matches nothing).  The
 * batch entry points run exactly this function.  A NULL array, B < 0, S <= 0, vocab <= 0, n outside 0 .. MV_MAX_SINK_TOKENS or a token outside [0, vocab) ->
 * MV_ERR_INVALID, flags untouched.
 * mv_corpus_route_flags: what the device kernel computed for rows [first, first + count) of the resident corpus under the current list (computed first if stale;
 * all 0 with an empty list); no corpus -> MV_ERR_STATE.  No reference counterpart (the reference computes in fp32). */
#define MV_MAX_SINK_TOKENS 64
int mv_set_sink_tokens(mv_handle* h, const int32_t* ids, int n);
int mv_get_sink_tokens(mv_handle* h, int32_t* ids, int capacity);
int mv_route_stats(mv_handle* h, int64_t* routed, int reset);
int mv_route_scan(const int32_t* ids, const int32_t* lens, int B, int S, const int32_t* tokens, int n, int vocab, uint8_t* flags);
int mv_corpus_route_flags(mv_handle* h, int64_t first, int64_t count, uint8_t* flags);

/* ---- anchor memory (replaces ModelMemory.forward_gold_instances, model_memory.py:105-115, as
 *      driven by predict_memory.py:81-83 and callbacks.py:48-53) ------------------------------ */

int mv_anchor_reset(mv_handle* h); /* _golden_instances_embeddings = None */
/* Encodes n anchors (ids [n,S], lens [n]) and appends their 512-d embeddings to the bank. */
int mv_anchor_append(mv_handle* h, const int32_t* ids, const int32_t* lens, int n, int S);
int mv_anchor_count(mv_handle* h);
/* Copies the bank to host: out fp32 [G,512]. */
int mv_anchor_get(mv_handle* h, float* out);
/* Installs a precomputed bank v fp32 [G,512] (BASELINE.json configs[4]: synthetic 1000-anchor bank). */
int mv_anchor_set(mv_handle* h, const float* v, int G);

/* ---- the hot loop (replaces ModelMemory.forward test/unlabel branch, model_memory.py:133-147,
 *      including _instance_forward l.90-103 and the embedder forward custom_PTM_embedder.py:172-242)
 * ids int32 [B,S] host, lens int32 [B] host.  Any output pointer may be NULL.
 *   logits fp32 [B,G,2]   W_m [u; v; |u-v|]                       (l.141)
 *   probs  fp32 [B,G,2]   softmax(logits, -1)                     (l.142; `output_dict['probs']`)
 *   best   fp32 [B,2]     probs[b, argmax_g probs[b,g,same_idx]]  (l.144-147)
 *   best_idx int32 [B]    that argmax (first maximal g)
 *   embed  fp32 [B,512]   u = header(pooler(BERT(ids)[:,0]))      (l.133)
 * (The matcher accumulates delta = logit_0 - logit_1 as one fp32 chain with the class-difference weights and derives probs from
 *  it — softmax_2 depends on nothing else — on every entry point; when `logits` is requested the class-0 chain runs too and
 *  logit_1 = logit_0 - delta.  Both agree with the reference's two separate sums to fp32 rounding: ~1e-6 on the logits.)
 * Returns after the results are in host memory. */
int mv_forward(mv_handle* h, const int32_t* ids, const int32_t* lens, int B, int S,
               float* logits, float* probs, float* best, int32_t* best_idx, float* embed);
/* mv_forward on a pad-to-longest batch of rows in ANY order (binding.Engine.forward_by_length: the reference's batch of UNSORTED issue reports,
 * predict_memory.py:97-101, scored without its padding): the rows are ordered by the padded length of their own token count (64 .. 256 in steps of 64, 384,
 * 512), groups of fewer than min_tokens padded tokens are merged into the next longer one, every group runs at its own length (in passes of as many rows as
 * one pass holds, like mv_forward's), the passes run back to back, one synchronisation, results in the caller's row order.  ids [B][S], outputs as
 * mv_forward's (best / best_idx required).  Takes every batch mv_forward takes: each pass's ids are uploaded at its own width, in one copy when they fit
 * max_tokens, and each output comes back in one copy when B <= max_batch. */
int mv_forward_ragged(mv_handle* h, const int32_t* ids, const int32_t* lens, int B, int S, int min_tokens, float* logits, float* probs, float* best,
                      int32_t* best_idx, float* embed);
/* mv_forward_ragged in two halves: `begin` enqueues the batch (upload, passes, download into pinned staging) on the stream of a workspace set without a ticket
 * and returns a ticket without waiting; `end` waits for it and fills the caller's arrays (those of the outputs `begin` was asked for; best / best_idx always).  One
 * batch per workspace set (MEMVUL_STREAMS, 2 by default) may be in flight: with no free workspace set, or B > max_batch, `begin` returns MV_ERR_CAPACITY before any
 * work, and the caller scores the batch synchronously (mv_forward_ragged: stream-ordered behind the batch in flight on workspace set 0).  mv_anchor_append waits
 * for a ticket in flight on another workspace set before it rewrites the bank (mv_anchor_set waits for everything): a ticket scores against the bank it began with.  Collect
 * tickets in the order they were issued; `end` consumes its ticket even when it fails.  predict_memory.evaluate hands over batch k + 1 before it collects batch k,
 * so the GPU does not wait for the host between batches (the reference's loop is serial: predict_memory.py:103-110).  The batches use the workspace sets of the
 * resident sweep (mv_corpus_run): collect every ticket before starting one, and the other way round; like the rest of a handle's entry points these two are not
 * thread-safe. */
int mv_forward_ragged_begin(mv_handle* h, const int32_t* ids, const int32_t* lens, int B, int S, int min_tokens, int want_logits, int want_probs, int want_embed,
                            int* ticket);
int mv_forward_ragged_end(mv_handle* h, int ticket, float* logits, float* probs, float* best, int32_t* best_idx, float* embed);
/* Encoder only (ModelMemory._instance_forward, model_memory.py:90-103): embed fp32 [B,512]. */
int mv_encode(mv_handle* h, const int32_t* ids, const int32_t* lens, int B, int S, float* embed);
/* Matcher only on host embeddings u fp32 [B,512] against the resident bank (model_memory.py:135-147). */
int mv_match(mv_handle* h, const float* u, int B, float* logits, float* probs, float* best, int32_t* best_idx);
/* Fused match + top-k over the resident bank (BASELINE.json configs[4]): for each u[b] the k anchors
 * with the largest P(same), ties to the lower anchor index; topk_p fp32 [B,k], topk_idx int32 [B,k]. */
int mv_topk(mv_handle* h, const float* u, int B, int k, float* topk_p, int32_t* topk_idx);

/* ---- HBM-resident corpus (the MI355X-native form of the AllenNLP `evaluate` loop,
 *      predict_memory.py:103-110): the whole tokenised shard (1.2 M x 256 x int32 = 1.25 GB) and all
 *      per-IR results live in HBM; the host launches batches back-to-back and downloads once. ---- */
int mv_corpus_upload(mv_handle* h, const int32_t* ids, const int32_t* lens, int64_t n, int S);
/* Runs IRs [first, first+count) in batches of `batch`; asynchronous. keep_probs != 0 also keeps
 * P(same) for every (IR, anchor) pair (what make_output_human_readable serialises, l.169-191). */
int mv_corpus_run(mv_handle* h, int64_t first, int64_t count, int batch, int keep_probs);
/* Same, processing only the first s_eff tokens of every row in the range (0 = all S): for a corpus uploaded sorted by
 * length, a batch runs at its own longest member's length (padded to 64) instead of the corpus-wide S — the engine
 * form of padding each batch to its longest instance (predict_memory.py:97-101). Rows longer than s_eff must not be
 * in the range (their tail would be cut). */
int mv_corpus_run_len(mv_handle* h, int64_t first, int64_t count, int batch, int keep_probs, int s_eff);
/* Batches of the resident sweep in flight at once: 2 (default; consecutive batches alternate between two workspace
 * sets on two HIP streams and overlap on the GPU) or 1.  Results are identical either way. */
int mv_set_streams(mv_handle* h, int n);
/* best fp32 [count,2], best_idx int32 [count], p_same fp32 [count,G] (NULL unless kept). Synchronises. */
int mv_corpus_results(mv_handle* h, int64_t first, int64_t count, float* best, int32_t* best_idx, float* p_same);
/* ---- the editable memory on a resident corpus.  The CWE anchor bank is the part of the reference model that changes without retraining
 *      (forward_gold_instances, model_memory.py:105-115, rebuilds it from the golden instances; the matcher of l.135-147 is all that reads it), and the
 *      encoder — all but tens of microseconds of a batch — does not depend on it.  A corpus that keeps its embeddings is matched again against a changed
 *      bank without the encoder; one that keeps top-k lists serves BASELINE.json configs[4] ("1000-anchor bank + top-k match") without the
 *      [N][G] P(same) array ever leaving the device.
 * mv_corpus_keep: what the sweeps of the CURRENT upload keep besides best / best_idx: keep_embed (0 | 1) the embedding of every row, fp32 [N][proj_dim] —
 * the encoder writes it there, no copy; topk (0 .. 64) the k anchors with the largest P(same) of every row, order and ties as mv_topk.  Call it after
 * mv_corpus_upload and before the first mv_corpus_run* of that upload (later: MV_ERR_STATE; no corpus: MV_ERR_STATE; a value out of range: MV_ERR_INVALID);
 * an upload resets it to (0, 0) and frees the arrays.  With (0, 0), the default, nothing is allocated and every other entry point is what it is without this
 * one: same results, same launches, same allocations.  The arrays are allocated at the first run (MV_ERR_NOMEM with the size in the message when that fails);
 * a run with topk larger than the bank, or anchors / 256 * topk > 1024, returns MV_ERR_INVALID.  In the guarded form a row that was encoded again in the
 * safe form, or routed there, keeps the safe form's embedding and top-k list, like its best anchor.  The library remembers which rows a keeping run covered.
 * mv_corpus_rematch: the matcher alone (model_memory.py:135-147) over the kept embeddings of rows [first, first + count) against the bank AS IT IS NOW: it
 * first collects what mv_corpus_results would (the sweeps in flight, the guarded form's rescoring), launches no encoder kernel, and waits before it returns.
 *   g_first == 0 (full): best, best_idx and the top-k lists of the rows are rewritten; with keep_probs also their P(same) rows (the array is reallocated at
 *     the present anchor count exactly as mv_corpus_run_len does, and only then does the pitch mv_corpus_results copies with change).  Byte-equal to
 *     running the same mv_corpus_run* calls again.
 *   0 < g_first < anchors (appended): THE CALLER STATES that the stored results of the rows were computed against a bank whose first g_first rows are the
 *     present ones (anchors were appended since, nothing else changed).  Only anchors [g_first, G) are matched and a merge kernel folds them into the stored
 *     best anchor and top-k lists, in the matcher's order — largest P(same) first, a tie to the lower anchor index, NaN above everything: byte-equal to the
 *     full mode.  keep_probs != 0 here: MV_ERR_INVALID.
 *   g_first == anchors: nothing was appended, MV_OK.  g_first outside [0, anchors]: MV_ERR_INVALID.
 * No embeddings kept, a row of the range that no keeping run covered, or an empty bank: MV_ERR_STATE; a kept top-k larger than the bank: MV_ERR_INVALID.
 * mv_corpus_embeddings: embed fp32 [count][proj_dim], what mv_encode returns for the rows at the width they were swept at (model_memory.py:90-103).
 * mv_corpus_topk: topk_p fp32 [count][k], topk_idx int32 [count][k] with the k of mv_corpus_keep (BASELINE.json configs[4]).  Both collect like
 * mv_corpus_results and return MV_ERR_STATE for a range with a row no keeping run covered, or when the corpus does not keep what they read. */
int mv_corpus_keep(mv_handle* h, int keep_embed, int topk);
int mv_corpus_rematch(mv_handle* h, int64_t first, int64_t count, int g_first, int keep_probs);
int mv_corpus_embeddings(mv_handle* h, int64_t first, int64_t count, float* embed);                 /* [count][proj_dim] fp32 */
int mv_corpus_topk(mv_handle* h, int64_t first, int64_t count, float* topk_p, int32_t* topk_idx);   /* [count][k] */
/* MV_F16X8 only (always 0 in MV_F16).  The fp8 planes of the activations (raw residual stream, attention context, GELU output) use ONE
 * static scale: |x| <= 112 is representable; an element beyond it keeps its fp16 accuracy but loses its correction term (the precision of
 * MV_F16 for that element) — the computation never fails over it.  *clamped = the number of such elements since the handle was created
 * (or since the last call with reset != 0; a 64-bit device counter: it does not wrap); synchronises.  A non-zero count on a real checkpoint means the 1e-3
 * logit contract of model_memory.py:141 is no longer backed by the measurements in DESIGN.md section 2 for that model: the Python
 * wrapper warns once (binding.Engine).  NaN activations are not counted (the range test is a floating-point maximum, which skips them): they
 * propagate to the outputs as NaN, where they are visible.  No reference counterpart (the reference computes in fp32). */
int mv_x8_saturation(mv_handle* h, int64_t* clamped, int reset);
/* How many kernel launches of this handle took a fixed-form persistent GEMM (MEMVUL_PP_FORM above) since it was created, or since the last call with reset != 0;
 * -1 for a null handle.  A host counter: no synchronisation.  For tests and A/B scripts (an equality test of the two forms proves nothing while this stays 0),
 * hence outside the mv_ names of the product ABI. */
int64_t mvpp_fixed_launches(mv_handle* h, int reset);

/* MV_F16X8 only (0 / 0 in MV_F16).  The concentration monitor: what the default form's 1e-3 is measured for is diffuse attention and attention sinks on the two
 * delimiter tokens — the [CLS] and the [SEP] token of a sequence sit in its rows 0 and 1 (the "special rows": A-side correction terms in every GEMM, V as hi + lo;
 * DESIGN.md section 2) — as trained BERT heads have them (custom_PTM_embedder.py:228 runs HF BertModel).  A head whose [CLS] row puts most of its mass on ONE
 * ORDINARY token is outside that envelope (measured 0.8 - 2.7e-3 with 50 - 80 % of the mass there, profiles/r06_n_sink_envelope.txt).  The attention kernel
 * therefore keeps, at no measurable cost, *max_collision = the maximum over every (sequence, head, layer) processed since the handle was created (or the last reset)
 * of sum_{j >= 2} p[CLS row][j]^2 (>= f^2 when one ordinary token holds the share f), *items_over = how many of them exceeded 0.25 (f > 0.5) and *items_total = how
 * many were looked at (sequences of at least 16 tokens); synchronises.  The Python wrapper warns once when more than 2 % of the items are over (binding.Engine).
 * The answer to a non-zero count is the safe form (mv_set_form(MV_FORM_SAFE) / MEMVUL_FORM=safe; the Python surface switches by itself under MEMVUL_ON_SINK=safe);
 * the safe form keeps counting, with the same meaning.  MV_FORM_GUARDED makes that choice per sequence from the same items (mv_set_form).
 * No reference counterpart (the reference computes in fp32). */
int mv_attention_concentration(mv_handle* h, float* max_collision, int64_t* items_over, int64_t* items_total, int reset);

/* MV_F16X8 only, in the default, safe and guarded forms (MV_ERR_STATE on a handle finalized as MV_F16 or MV_F32, and before mv_finalize_weights).  The sink
 * census: WHICH token the items counted by *items_over above sit on.  While it is on, every pass adds one small kernel per layer whose attention feeds the
 * concentration monitor (memvul_amd/csrc/sink_census.h: a reader of the Q / K planes the pass holds; the rescoring passes of the guarded form add nothing): for
 * every (sequence, head, layer) item whose collision mass of the [CLS] row on ordinary keys exceeds 0.25 it finds the ordinary token position with the largest
 * share p* of that row (ties: the lowest position) and adds, with integer atomics (the result depends on neither scheduling nor batching nor streams),
 * items[token id] += 1, share_q20[token id] += round(p* 2^20) and by_head[layer][head] += 1.  The buffers are allocated at the first enable, sized by
 * mv_config.vocab_size; `on` is read on the host when a pass is enqueued.  Off (the default) costs a pass one host-side test per layer.  The kernel recomputes
 * the row from the hi planes of Q and K: an item within rounding of the threshold may be counted here and not by the monitor, or the other way round.
 * mv_sink_census_read waits for the work in flight, then copies items uint32 [vocab], share_q20 uint64 [vocab] and by_head uint32 [layers][12] (any of them may
 * be NULL); vocab != mv_config.vocab_size or layers_x_heads != mv_config.layers * 12 -> MV_ERR_INVALID; before the first enable -> MV_ERR_STATE; reset != 0
 * zeroes all three.  No reference counterpart (the reference computes in fp32). */
int mv_sink_census_enable(mv_handle* h, int on);
int mv_sink_census_read(mv_handle* h, uint32_t* items, uint64_t* share_q20, int vocab, uint32_t* by_head, int layers_x_heads, int reset);

/* ---- multi-GPU exchange (the reference is single-process, predict_memory.py:103) --------------------
 * One process per GPU, contiguous corpus shards, no data-path collective; the ONE exchange is an all-gather of the
 * per-rank (score, label) statistics.  RCCL (librccl.so, opened at run time) is bound directly: the collective runs
 * on the engine's own stream and the process needs neither torch nor a launcher-specific runtime.
 * mv_comm_prepare: opens librccl.so and resolves its entry points (so that every rank can report "RCCL usable here" BEFORE
 * any rank enters the collective ncclCommInitRank).  mv_comm_unique_id: rank 0 draws the 128-byte ncclUniqueId (returns the
 * byte count).  mv_comm_init: ncclCommInitRank with those bytes — how they reach the other ranks is the host's business
 * (memvul_amd/distributed.py broadcasts them over its rendezvous socket; nothing is written to a shared temp directory and
 * nothing assumes one node).  mv_comm_allgather: `bytes_per_rank` bytes of host memory per rank -> world * bytes_per_rank
 * bytes on every rank, in rank order (staged through device buffers the library owns).  world == 1 needs no init: the
 * gather is then a copy (world == 1 WITH an id builds a real one-rank communicator: the single-GPU test of this path). */
int mv_comm_prepare(mv_handle* h);
int mv_comm_unique_id(mv_handle* h, void* id_out, int capacity);
int mv_comm_init(mv_handle* h, int rank, int world, const void* id, int id_bytes);
int mv_comm_allgather(mv_handle* h, const void* send, void* recv, int64_t bytes_per_rank);
int mv_comm_destroy(mv_handle* h);
/* What the transport is, as RCCL reports it: info[0] = ranks of the live communicator (ncclCommCount; 0 = no communicator),
 * info[1] = this rank in it (ncclCommUserRank), info[2] = RCCL version code (ncclGetVersion; 0 while librccl.so is not open),
 * info[3] = the world mv_comm_allgather gathers over.  bench.py --gpus N records it in its line. */
int mv_comm_info(mv_handle* h, int* info, int n);
/* GPUs visible to this process (hipGetDeviceCount; 0 without one; <= 0 means none): lets a test or a launcher decide whether a
 * two-rank RCCL run is possible here. */
int mv_device_count(void);

/* ---- measurement / test hooks ---------------------------------------------------------------- */

/* Per-kernel-class HIP-event timing on the engine's own stream. Classes: see mv_kernel_class_name. */
#define MV_NUM_KERNEL_CLASSES 14
int mv_profile_enable(mv_handle* h, int on);
/* Restrict the events to the classes whose bit is set (default: all).  bench.py times its K steps with events
 * on the dominant GEMM class only (the `roofline` figure) and takes the full breakdown in a separate pass, so
 * the timed region carries ~12 event pairs per step instead of ~90. */
int mv_profile_select(mv_handle* h, uint32_t class_mask);
/* Synchronises, adds up the recorded launches since the last read: ms[c], launches[c]; then clears. */
int mv_profile_read(mv_handle* h, double* ms, int64_t* launches, int n);
const char* mv_kernel_class_name(int cls);

/* Debug taps for per-kernel parity tests: run the encoder on (ids,lens) and stop after `n_layers`
 * encoder layers (0 = embeddings only, <0 = all), then copy an internal buffer to host.
 * buffer ids: 0 hidden fp32 [B*Sp,768]; 1 hidden fp16; 2 Q fp16 [B,12,Sp,64]; 3 K fp16 [B,12,Sp,64];
 * 4 V^T fp16 [B,12,64,Sp]; 5 attention context fp16 [B*Sp,768]; 6 FFN intermediate fp16 [B*Sp,3072];
 * 7, 8, 9 (MV_F16X8) the second fp16 planes of Q, K, V^T, fp16(x - fp16(x)), in the layouts of 2, 3, 4: valid after a pass that wrote them (padded length
 * <= 128 in the default form, every pass in the safe form); 10 the embedding fp32 [B, proj_dim] of a full run.
 * (Sp = S rounded up to a multiple of 64, above 256 to a multiple of 128; buffers hold the state of the LAST executed layer; Q carries
 * the folded 1/8.  The pass takes the path its size selects — persistent kernels or the small-pass kernels — with last-layer pruning
 * off and the final LayerNorm applied, so buffer 0 is the normalised output of layer n_layers.  MV_FORM_GUARDED is ignored here: the taps show the default
 * form, nothing is rescored.  An MV_F32 handle has buffers 0 and 10 and its own fp32 planes 35 - 37: its Q, K, V, context and intermediate are fp32 planes,
 * and mv_debug_read of the fp16 taps 1 - 9 returns MV_ERR_INVALID with a message that says so.)
 * The fp32 planes of the reference form, token order, product library and development build alike: 35 qkv32 fp32 [B*Sp][2304], Q (1/8 folded) | K | V, head h in
 * columns 64 h .. 64 h + 63 of each block; 36 ctx32 fp32 [B*Sp][768], the attention context; 37 h32 fp32 [B*Sp][3072], the GELU output.  Each is written once per
 * layer and holds the last executed layer's.  On a handle of another compute dtype they answer MV_ERR_STATE (the buffer does not exist in that dtype).
 * The raw planes of the persistent path, in the engine's own row order (rows 0 and 1 of a sequence hold its [CLS] and its LAST token; T = B*Sp tokens):
 * 11 x8, the stream's fp8 planes, bytes [T][2*768] = [lo8 | hi8] per row; 12 st_lo fp16 [2 B][768], 2^11 x the stream's low parts of the special rows, compact
 * [2 b + row]; 13 lnstats and 14 lnpart fp32 [T][3][2], per row and 256-column tile the (sum, sum of squares) of the stream at the layer's input / after the
 * output projection; 15 ctx8 bytes [T][2*768]; 16 cls_lo fp16, compact [2 b + row][N], 2^11 x the special rows' low parts of the context (N = 768) or of the GELU
 * output (N = 3072) — at most 2 B * 3072 elements; 17 h8 bytes [T][2*3072]; 18 vlo_sp fp16 [B*12][64][2], 2^11 x the low parts of V of the special rows; 19 xlo
 * fp16 [T][768], the stream's lo plane (MV_F16 only); 20 cls_corr fp32, compact [2 b + row][N] with the N of the last launch that took a row term, 2^11 x that
 * term; 21 tile_both int32 [ceil(T / 256)], the per-row-tile flags of the [CLS]-row form (written only by a pass of padded length 256 / 512 in that form).
 * The per-token planes 11, 13 - 15, 17 and 19 may be read up to the end of the pass' last 256-row tile (T rounded up to 256 rows: the persistent GEMMs compute
 * those rows like any other; no token lives there, the embedding kernel leaves them as the pass before left them, and a pass that MEMVUL_DEBUG_STOP ended
 * between a residual GEMM and the launch that writes the matching vstats leaves them with a stream and statistics that do not belong together).
 * After an ordinary mv_debug_encode they hold what the last layer and the final LayerNorm left (buffer 1 is then the NORMALISED stream); the development build's
 * MEMVUL_DEBUG_STOP=k ends the pass after the first k launch groups of its last layer, without the final LayerNorm, so that every plane is what that launch
 * wrote.  A buffer that does not exist in the handle's compute dtype (11, 12, 15 - 18, 20, 21: MV_F16X8; 19: MV_F16; 35 - 37: MV_F32) answers MV_ERR_STATE.
 * On an MV_F32 handle MEMVUL_DEBUG_STOP=k ends the pass inside its last layer after 1 the QKV GEMM, 2 attention, 3 the output-projection GEMM (buffer 0 = the raw
 * x + ctx Wo^T + bo, before LayerNorm 1), 4 LayerNorm 1 and FFN-1 (buffer 0 the normalised stream, 37 the GELU output), 5 FFN-2 (buffer 0 raw, before LayerNorm 2);
 * the pooler does not run, and with n_layers = 0 the embedding stays as it is.
 * The tail taps, development build with MEMVUL_DEBUG_TAIL=1 only (the product library answers "unknown buffer"): mv_debug_encode never prunes its last layer, so these
 * are filled by an ORDINARY pruned pass on workspace set 0 (mv_encode, mv_forward), which then copies the B real rows each launch of the pruned last layer's
 * [CLS] tail wrote into an arena of its own — the tail overwrites c32 and pooled in place.  22 c32 fp32 [B][768] and 23 c16 fp16 [B][768] as cls_gather_kernel
 * left them; 24 cq fp32 [B][768], the [CLS] query (1/8 folded); 25 the single-query attention's context [B][768], fp32 in MV_F16X8, fp16 in MV_F16; 26 c32 after the
 * output projection + residual; 27 c32 and 28 c16 after LayerNorm 1; 29 the FFN intermediate [B][3072], fp32 in MV_F16X8 (ch32), fp16 in MV_F16 (ch16); 30 c32 after
 * FFN-2 + residual; 31 c32 after LayerNorm 2; 32 the pooler output fp32 [B][768]; 33 the embedding u fp32 [B][proj_dim]; 34 int32 [3]: the pruned passes tapped since
 * mv_create, and B and Sp of the last pass (a batch that ran as one pass adds 1).  After such a call buffers 0, 1, 12, 13, 19 (the stream the tail gathers from) and
 * 3, 4, 8, 9, 18 (K, V^T, their lo planes, vlo_sp) still hold the tail's inputs: the pruned layer overwrites none of them. */
int mv_debug_encode(mv_handle* h, const int32_t* ids, const int32_t* lens, int B, int S, int n_layers);
int mv_debug_read(mv_handle* h, int buffer, void* dst, int64_t bytes);
/* Stand-alone GEMM check/bench on caller data: C[M,N] = A[M,K] (fp16 bits) x W[N,K]^T (fp16 bits)
 * + bias, fp32 out.  variant 0 = the 128^2-tile kernel of small passes (M,N multiples of 128), 19 = the 64^2-tile ring kernel of
 * the [CLS] tail (multiples of 64); K a multiple of 64.  iters > 1 repeats for timing; *ms = average milliseconds per launch. */
int mv_test_gemm(mv_handle* h, int variant, int M, int N, int K, const uint16_t* A, const uint16_t* W,
                 const float* bias, float* C, int iters, float* ms);
/* The persistent FFN-1 kernel (gemm_pp.h PP_GELU) on caller data with unit row statistics: out16 [M][N] = fp16 bits of
 * gelu(A W^T + bias) for fp32 A [M][K], W [N][K]; x8 != 0 runs the MV_F16X8 build (the operands are split into their fp16 / fp8
 * planes on the host) and, with out8, returns the [lo8 | hi8] e4m3 planes of the output [M][2 N].  M,N % 256, K % 128, K >= 256. */
int mv_test_gemm_pp(mv_handle* h, int x8, int M, int N, int K, const float* A, const float* W, const float* bias, uint16_t* out16,
                    uint8_t* out8, int iters, float* ms);
/* The MV_F32 GEMM (ref_f32.h) on caller data, all fp32: C [M][N] = act(A [M][K] W [N][K]^T + bias) (+ res [M][N]); act 0 = bias only, 1 = erf GELU,
 * 2 = + res (required then).  bias may be NULL (zeros).  M, N % 128, K % 32.  Works on a handle of any compute dtype.  iters / ms as mv_test_gemm. */
int mv_test_gemm_f32(mv_handle* h, int act, int M, int N, int K, const float* A, const float* W, const float* bias, const float* res, float* C, int iters,
                     float* ms);
/* The host-side e4m3 encoder used for the MV_F16X8 weight planes (needs no GPU, h may be NULL elsewhere): out[i] = OCP e4m3fn bits of in[i]. */
int mv_test_e4m3(const float* in, uint8_t* out, int64_t n);

/* Host only, no GPU work, callable from any thread: the JSON line of one batch's records — replaces json.dumps(make_output_human_readable(...))
 * (model_memory.py:169-191 -> predict_memory.py:111), whose cost is CPython's repr() of B x G doubles.
 *   out = "[" + ", ".join(prefix_i + piece_0 + repr(p[i][0]) + ... + piece_{cols-1} + repr(p[i][cols-1]) + row_suffix for i in rows) + "]"
 * prefixes / pieces: the strings back to back, *_off[k] .. *_off[k + 1] the bytes of string k (rows + 1 / cols + 1 offsets); p: double [rows][cols];
 * every double is printed exactly as Python's repr(float) prints it.  MV_ERR_CAPACITY: `cap` too small; MV_ERR_INVALID: a non-finite value (json.dumps
 * spells those NaN / Infinity: the caller formats such a batch itself). */
int mv_format_records(const char* prefixes, const int64_t* prefix_off, int64_t rows, const char* pieces, const int64_t* piece_off, int64_t cols,
                      const char* row_suffix, const double* p, char* out, int64_t cap, int64_t* written);

/* ---- the device WordPiece tokenizer (memvul_amd/csrc/wordpiece.h states the rule) ---------------------------------------------------------------------------
 * Replaces, for ASCII text, the tokenisation the reference's reader runs per issue report (PretrainedTransformerTokenizer over bert-base-uncased,
 * reader_memory.py:88, test_config_memory.json:5-16): BertNormalizer(clean_text) -> BertPreTokenizer -> WordPiece("##") -> [CLS] A [SEP] -> truncation on the
 * right, byte-equal to the Rust backend of BertTokenizerFast for every text whose bytes are all below 0x80.  A row that holds a byte >= 0x80, or one of the
 * tokenizer's added tokens as a literal, case-sensitive substring of its raw bytes, is NOT tokenised: status[i] = 1, lens[i] = 0, its id row zero — the
 * caller sends it through the tokenizer it has (memvul_amd/tokenizer.py does).
 * An object of its own, not part of mv_handle: it needs no weights, owns its stream and its device buffers and shares no mutable state with any handle, so
 * one thread may be inside mv_tok_encode while another is inside mv_corpus_run* / mv_forward_ragged_* on a handle of the same device.  The object itself is
 * not re-entrant: one call at a time.
 * mv_tok_create: the vocabulary as n_vocab strings back to back (string k = bytes vocab_off[k] .. vocab_off[k + 1] of vocab_bytes, its id is k; "##x" is
 * the continuation piece x; an empty string stands for an id the vocabulary does not use), the added-token literals likewise, the ids of [UNK] / [CLS] /
 * [SEP], WordPiece's max_input_chars_per_word (1 .. 190) and the normalizer's lowercase flag.  The hash table is built here, on the host (open addressing,
 * load <= 0.5, every hit confirmed on the bytes).  device >= 0 uploads it and creates the stream; device < 0 builds the table only: such an object serves
 * mv_tok_encode_host and needs no GPU.  A bad argument -> MV_ERR_INVALID, *out = NULL, the message from mv_tok_last_error(NULL).
 * mv_tok_encode: n texts (text i = bytes off[i] .. off[i + 1] of `text`, off int64 [n + 1] ascending) -> ids int32 [n][max_length] zero-padded, lens
 * int32 [n], status uint8 [n].  add_special != 0 writes [CLS] first and [SEP] last; truncation to max_length counts them.  The kernel (one wave per text),
 * synchronous: the results are in host memory on return.  Device buffers grow to the largest call; the text goes to the device in chunks of at most 64 MiB
 * (a chunk ends at a row boundary; a single larger row is a chunk of its own).  On an object created with device < 0 -> MV_ERR_STATE.
 * mv_tok_encode_host: the same arguments, the same rule, single-threaded on the CPU: the rule's reference and the tests' second opinion, not a product path.
 * Both: n < 0, max_length outside 2 .. 512, offsets not ascending or negative, or NULL where data is needed -> MV_ERR_INVALID with ids, lens and status
 * untouched; n == 0 -> MV_OK, nothing read or written (also on an object without a device).  A HIP failure in the middle of a call waits for whatever the
 * call had queued before it returns: the caller's arrays are not written after a failed call.
 * mv_tok_kernel_ms: *ms = the kernel's own time, from HIP events around each chunk's launch, summed over the chunks of the last mv_tok_encode (0 before the
 * first): what of a call is tokenising and what is copying.  It covers whichever kernel ran last (mv_tok_encode or mv_tok_encode_u8).
 *
 * UTF-8 text (opt-in; the rule: memvul_amd/csrc/wordpiece.h).  mv_tok_set_unicode attaches a code-point table to an existing object and uploads it when the
 * object has a device: n_entries (1 .. 131072) entries of 16 bytes, entry i for code point i (entries below 0x80 are never read; code points from n_entries
 * on count as uncovered): bytes 0 .. 11 the UTF-8 of the tokenizer's normalizer applied to that one code point, byte 12 their count (0 .. 12), byte 13 the
 * classes of the output code points, two bits each, the first in the low bits (1 whitespace, 2 punctuation, 3 word), byte 14 the covered flag (0 / 1), byte 15
 * the number of output code points (0 .. 3).  MV_ERR_INVALID, the object unchanged, on a malformed table — a byte count over 12, output bytes that are not
 * well-formed UTF-8, a class outside the three, a character count that is not the bytes' — and when a word of max_chars_per_word characters plus one
 * 64-byte step's largest output under this table does not fit the kernel's word buffer (640 bytes: max_chars_per_word 100 fits the tables BertNormalizer
 * gives).  memvul_amd/tokenizer.py builds the table from the tokenizer's own normalizer and pre-tokenizer and decides there which code points are covered.
 * mv_tok_encode_u8 / mv_tok_encode_u8_host: the arguments, checks, chunking and "outputs untouched on error" of mv_tok_encode / mv_tok_encode_host, for text
 * in UTF-8.  status[i] is 0 (tokenised, byte-equal to the Rust backend), 1 (an added-token literal in the raw bytes, as above, here also a literal with bytes >= 0x80; it wins over 2) or 2 (a
 * malformed UTF-8 sequence, a code point >= U+20000 or one the table marks uncovered); rows of status 1 and 2 have length 0 and a zero id row.  On an object
 * without a table -> MV_ERR_STATE.  mv_tok_encode and mv_tok_encode_host are unchanged on an object with a table: they hand back every byte >= 0x80. */
typedef struct mv_tokenizer mv_tokenizer;
int mv_tok_create(int device, const char* vocab_bytes, const int64_t* vocab_off, int n_vocab, const char* literal_bytes, const int64_t* literal_off,
                  int n_literals, int unk_id, int cls_id, int sep_id, int max_chars_per_word, int lowercase, mv_tokenizer** out);
int mv_tok_encode(mv_tokenizer* tok, const char* text, const int64_t* off, int n, int max_length, int add_special, int32_t* ids, int32_t* lens,
                  uint8_t* status);
int mv_tok_encode_host(mv_tokenizer* tok, const char* text, const int64_t* off, int n, int max_length, int add_special, int32_t* ids, int32_t* lens,
                       uint8_t* status);
int mv_tok_kernel_ms(mv_tokenizer* tok, float* ms);
int mv_tok_set_unicode(mv_tokenizer* tok, const void* entries, int n_entries);
int mv_tok_encode_u8(mv_tokenizer* tok, const char* text, const int64_t* off, int n, int max_length, int add_special, int32_t* ids, int32_t* lens,
                     uint8_t* status);
int mv_tok_encode_u8_host(mv_tokenizer* tok, const char* text, const int64_t* off, int n, int max_length, int add_special, int32_t* ids, int32_t* lens,
                          uint8_t* status);
void mv_tok_destroy(mv_tokenizer* tok);
/* Last error message of this object (or of a failed mv_tok_create when tok == NULL). */
const char* mv_tok_last_error(mv_tokenizer* tok);

#ifdef __cplusplus
}
#endif
#endif /* MEMVUL_HIP_H */
