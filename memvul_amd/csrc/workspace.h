// Part of engine.hip: the buffers of a workspace set (Work, engine.hip), allocated in one function — the common buffers at mv_create, the
// compute dtype's group at mv_finalize_weights.

namespace {

constexpr int WORK_COMMON = -1;  // alloc_work's group at mv_create; at mv_finalize_weights the group is the compute dtype

// One group of wk's buffers, zeroed on wk's own stream, with one wait for the set.  Known: an MV_F32 handle holds the 16-bit planes of the common group
// without reading most of them.
int alloc_work(mv_handle* h, Work& wk, int group) {
  const mv_config& c = h->cfg;
  const int64_t T = h->cap_tokens;           // rows of every activation buffer
  const int64_t B = c.max_batch;
  const int64_t Bp = round_up(B, 256);       // [CLS]-row buffers of the pruned last layer
  const int64_t BG = B * c.max_anchors;
  int rc = MV_OK;
  auto A = [&](auto** p, int64_t count) { if (rc == MV_OK) rc = dev_alloc(h, wk.stream, p, count); };
  if (group == WORK_COMMON) {
    A(&wk.d_ids, T);
    A(&wk.d_lens, B + 16);
    A(&wk.seq_over, B);
    A(&wk.d_idx, B);
    A(&wk.xres, T * MV_HIDDEN);
    A(&wk.x16, T * MV_HIDDEN);
    A(&wk.q, T * MV_HIDDEN);
    A(&wk.k, T * MV_HIDDEN);
    A(&wk.vt, T * MV_HIDDEN);
    A(&wk.ctx, T * MV_HIDDEN);
    A(&wk.h16, T * MV_INTER);
    A(&wk.lnstats, T * 6);
    A(&wk.lnpart, T * 6);
    A(&wk.c32, Bp * MV_HIDDEN);
    A(&wk.cq, Bp * MV_HIDDEN);
    A(&wk.c16, Bp * MV_HIDDEN);
    A(&wk.cctx, Bp * MV_HIDDEN);
    A(&wk.ch16, Bp * MV_INTER);
    A(&wk.u, B * h->P);
    A(&wk.pooled, B * MV_HIDDEN);
    A(&wk.u_in, B * h->P);
    A(&wk.logits, BG * 2);
    A(&wk.probs, BG * 2);
    A(&wk.psame, BG);
    A(&wk.best, B * 2);
    A(&wk.best_idx, B);
    A(&wk.topk_p, B * 64);
    A(&wk.topk_idx, B * 64);
    const int64_t nch = (c.max_anchors + 255) / 256;
    const int64_t per = nch > 1 ? (nch * MK_KMAX < 1024 ? nch * MK_KMAX : 1024) : 0;  // chunks x k <= 1024 (match_dev)
    A(&wk.part_p, B * per);
    A(&wk.part_q, B * per);
    A(&wk.part_i, B * per);
  } else if (group == MV_F32) {  // the fp32 planes of one pass, 6144 floats per token (1.6 GB per workspace set at 65 536 tokens)
    A(&wk.qkv32, T * 3 * MV_HIDDEN);
    A(&wk.ctx32, T * MV_HIDDEN);
    A(&wk.h32, T * MV_INTER);
  } else if (group == MV_F16) {  // the lo fp16 plane of the two-plane raw stream (MV_F16X8 keeps the stream's low part in the lo8 plane of x8 + st_lo: gemm.h GemmArgs::out16b)
    A(&wk.xlo, T * MV_HIDDEN);
  } else {  // MV_F16X8: fp8 planes [lo8 | hi8] of the three activations that are GEMM A operands
    A(&wk.x8, T * 2 * MV_HIDDEN);
    A(&wk.ctx8, T * 2 * MV_HIDDEN);
    A(&wk.h8, T * 2 * MV_INTER);
    A(&wk.ch32, Bp * MV_INTER);
    A(&wk.cls_lo, 2 * Bp * MV_INTER);
    A(&wk.cls_corr, 2 * Bp * MV_INTER);
    A(&wk.st_lo, 2 * Bp * MV_HIDDEN);
    A(&wk.vlo_sp, B * MV_HEADS * MV_HEAD_DIM * 2);
    A(&wk.tile_both, T / 256 + 1);
    // second fp16 planes of V^T, Q, K: read by passes of padded length <= 128 in the default form, by every pass in the safe form (attention_v2.h VLO)
    A(&wk.vt_lo, T * MV_HIDDEN);
    A(&wk.q_lo, T * MV_HIDDEN);
    A(&wk.k_lo, T * MV_HIDDEN);
  }
  if (rc == MV_OK && hipStreamSynchronize(wk.stream) != hipSuccess) rc = MV_ERR_HIP;
  return rc;
}

}  // namespace
