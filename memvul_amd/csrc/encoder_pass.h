// Part of engine.hip: one encoder pass — the launchers of every kernel class, the form and the plan of a pass (PassForm, PassPlan), the attention variants,
// the layer bodies, encode_dev / encode_f32_dev, and the matcher (match_dev).  Every launch of a pass is stated here, once.

namespace {

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
// fixed: the launch belongs to a pass of the fixed form (pp_fixed_form below) and goes to the kernels of libmemvul_pp_fixed.so (gemm_pp_fixed.hip), which take the
// form's fields as constants and do not read them from `a`; what the pass cannot know is checked here — the raster the launch gets and the N those kernels fix
template <int PPEPI>
int launch_pp(mv_handle* h, hipStream_t stream, int cls, GemmArgs a, bool fixed = false) {
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
    if (fixed && a.raster_mode == 0 && (PPEPI == PP_QK || a.N == (PPEPI == PP_GELU ? MV_INTER : MV_HIDDEN))) {
      const int e = pp_fixed_launch(PPEPI, &a, grid, pp_lds<PPEPI>, stream);
      if (e < 0) return fail(h, MV_ERR_STATE, "internal: no fixed-form gemm_pp kernel for this launch");
      if (e != (int)hipSuccess) return fail(h, MV_ERR_HIP, std::string("launch gemm_pp (fixed form): ") + hipGetErrorString((hipError_t)e));
      ++h->pp_fixed_launches;
      return MV_OK;
    }
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

// form choice: the persistent GEMMs of this pass take the fixed-form kernels (gemm_pp_fixed.hip) — every form field those kernels hold as a constant has, in this
// pass, the value they fix.  The [CLS]-row form on one-sequence tiles (padded length 256 / 512) with no sequence below cls_min_len as the HOST knows the
// lengths (min_len; 0 = unknown: no tile flag would be set, so no tile is short), one plane, not the safe form, and no QKV block that sweeps its A-side term.
// MEMVUL_PP_FORM=runtime (mv_handle::pp_fixed) keeps every launch on the run-time kernels: the two forms compute the same bits
struct PassPlan;
bool pp_fixed_form(const mv_handle* h, const PassPlan& p, int min_len);  // (defined below PassPlan)

// the mid-size / skinny GEMMs of a pass that does not fill the chip (and of the [CLS] tail)
template <int EPI>
int launch_small(mv_handle* h, hipStream_t stream, int cls, const GemmArgs& a) {
  if (h->gemm_tile == 0 && a.M <= 512 && a.M % 64 == 0 && a.N % 64 == 0) return launch_ring64<EPI>(h, stream, cls, a);
  return launch_gemm128<EPI>(h, stream, cls, a);
}

// The tail taps of the development build (MEMVUL_DEBUG_TAIL=1, engine.hip read_switches): after a launch of the pruned last layer's [CLS] tail, its B output
// rows copied into slot `stage` of the handle's tap arena — on the pass's stream, so the copy sees what that launch wrote and the next launch (which may
// overwrite it in place: c32 four times, pooled as the fp32 context and then as the pooler output) waits for it.  Workspace set 0 only (what mv_debug_read
// reads).  The product build compiles MV_TAIL_TAP to nothing.
#if defined(MEMVUL_DEV_SWITCHES)
enum TailTap { TT_GATHER32, TT_GATHER16, TT_Q, TT_CTX, TT_OUT, TT_LN1_32, TT_LN1_16, TT_FFN1, TT_FFN2, TT_LN2, TT_POOLED, TT_U, TT_COUNT };
// bytes per row of a slot (the widest form of the stage: fp32; MV_F16 stores fp16 in TT_CTX / TT_FFN1) and the slots' offsets in row units
constexpr int64_t TT_ROW[TT_COUNT] = {3072, 1536, 3072, 3072, 3072, 3072, 1536, 12288, 3072, 3072, 3072, 3072};
constexpr int64_t tt_off(int s) { return s == 0 ? 0 : tt_off(s - 1) + TT_ROW[s - 1]; }
int tail_tap(mv_handle* h, Work& wk, int stage, const void* src, size_t row_bytes, int B) {
  if (!h->dbg_tail || &wk != &h->work[0]) return MV_OK;
  if (!h->tail_arena)
    if (int rc = dev_alloc(h, wk.stream, &h->tail_arena, tt_off(TT_COUNT) * h->cfg.max_batch)) return rc;
  if (B > h->cfg.max_batch || (int64_t)row_bytes > TT_ROW[stage]) return fail(h, MV_ERR_STATE, "internal: tail tap larger than its slot");
  if (stage == TT_GATHER32) ++h->tail_passes;  // (the first tap of a pruned pass: a batch cut into several passes shows here, and only the last one's rows stay)
  HIPCHK(h, hipMemcpyAsync(h->tail_arena + tt_off(stage) * h->cfg.max_batch, src, row_bytes * (size_t)B, hipMemcpyDeviceToDevice, wk.stream));
  return MV_OK;
}
#define MV_TAIL_TAP(stage, src, row_bytes, B) \
  if (int rc_tap = tail_tap(h, wk, stage, src, row_bytes, B)) return rc_tap
#else
#define MV_TAIL_TAP(stage, src, row_bytes, B)
#endif

// K7 + K8: pooler on the [CLS] rows (row_stride floats apart), then the header
int pool_head(mv_handle* h, Work& wk, const float* x, size_t row_stride, int B, float* u_out) {
  const unsigned gx = (unsigned)((B + 31) / 32);
  hipLaunchKernelGGL(dense768_kernel<0>, dim3(gx, MV_HIDDEN / 32), dim3(512), 0, wk.stream, x, row_stride, B, h->WpT, h->bp,
                     MV_HIDDEN, h->P == MV_HIDDEN ? u_out : wk.pooled);
  if (int rc = launch_check(h, "pooler")) return rc;
  MV_TAIL_TAP(TT_POOLED, h->P == MV_HIDDEN ? u_out : wk.pooled, MV_HIDDEN * 4, B);
  if (h->P == MV_HIDDEN) {  // use_header = False: the pooler output is the embedding
    MV_TAIL_TAP(TT_U, u_out, MV_HIDDEN * 4, B);
    return MV_OK;
  }
  hipLaunchKernelGGL(dense768_kernel<1>, dim3(gx, MV_PROJ / 32), dim3(512), 0, wk.stream, wk.pooled, (size_t)MV_HIDDEN, B, h->WhT,
                     h->bh, MV_PROJ, u_out);
  if (int rc = launch_check(h, "header")) return rc;
  MV_TAIL_TAP(TT_U, u_out, MV_PROJ * 4, B);
  return MV_OK;
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
// stop (mv_debug_encode of the development build, mv_handle::dbg_stop; 0 = off): the pass ends inside its LAST layer — after 1 the QKV GEMM, 2 attention, 3 the
// output-projection GEMM (xres = the raw x + ctx Wo^T + bo, before LayerNorm 1), 4 LayerNorm 1 and FFN-1, 5 FFN-2 (xres raw, before LayerNorm 2) — and the pooler
// does not run.  qkv32, ctx32 and h32 are written once per layer, so stops 3, 4, 5 and the ordinary run expose every launch.  stop == 0 launches what it always did.
int encode_f32_dev(mv_handle* h, Work& wk, const int32_t* d_ids, const int32_t* d_lens, int B, int S_in, int n_layers, float* u_out, int pitch, int stop = 0) {
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
  if (stop && n_layers == 0) return MV_OK;  // the embedding as it is
  for (int l = 0; l < n_layers; ++l) {
    const LayerW& w = h->L[l];
    const int ls = l == n_layers - 1 ? stop : 0;  // the launch groups of this layer to run (0 = all)
    if (int rc = launch_gemm_f32<RF_ACT_NONE>(h, wk.stream, KC_GEMM_QKV, wk.xres, w.wqkv32, w.bqkv, nullptr, wk.qkv32, Mp, 3 * H, H)) return rc;
    if (ls == 1) return MV_OK;
    {
      ProfScope ps(h, wk.stream, KC_ATTENTION);
      const int units = B * MV_HEADS * (Sp / 32);
      hipLaunchKernelGGL(attention_f32_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, wk.stream, (const float*)wk.qkv32, d_lens, wk.ctx32, Sp, units);
      if (int rc = launch_check(h, "attention_f32")) return rc;
    }
    if (ls == 2) return MV_OK;
    if (int rc = launch_gemm_f32<RF_ACT_RES>(h, wk.stream, KC_GEMM_OUT, wk.ctx32, w.wo32, w.bo, wk.xres, wk.xres, Mp, H, H)) return rc;
    if (ls == 3) return MV_OK;
    if (int rc = run_ln(w.ln1g, w.ln1b)) return rc;
    if (int rc = launch_gemm_f32<RF_ACT_GELU>(h, wk.stream, KC_GEMM_FFN1, wk.xres, w.w132, w.b1, nullptr, wk.h32, Mp, I, H)) return rc;
    if (ls == 4) return MV_OK;
    if (int rc = launch_gemm_f32<RF_ACT_RES>(h, wk.stream, KC_GEMM_FFN2, wk.h32, w.w232, w.b2, wk.xres, wk.xres, Mp, H, I)) return rc;
    if (ls == 5) return MV_OK;
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
  bool fixed;      // the persistent GEMMs take the fixed-form kernels (pp_fixed_form)
};

bool pp_fixed_form(const mv_handle* h, const PassPlan& p, int min_len) {
  return h->pp_fixed && p.big && p.x8 && p.cls_as && p.one_seq_tiles && min_len >= h->cls_min_len && !p.two_plane && !p.safe && p.qkv_mask == 0;
}

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
  return launch_pp<PP_QK>(h, wk.stream, cls, g, p.fixed);
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
  return launch_pp<PP_RESLN3>(h, wk.stream, KC_GEMM_OUT, g, p.fixed);
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
  return launch_pp<PP_GELU>(h, wk.stream, KC_GEMM_FFN1, g, p.fixed);
}

// K6: FFN-2 + bias + LayerNorm(residual); persistent path: + vstats of the new rows (wk.lnstats: the next layer's input)
int launch_ffn2(mv_handle* h, Work& wk, const PassPlan& p, const LayerW& w) {
  GemmArgs g = pass_gemm(h, wk, p);
  g.A = wk.h16; g.W = w.w2; g.bias = w.b2; g.N = MV_HIDDEN; g.K = MV_INTER;
  if (!p.big) { g.xres = wk.xres; return launch_small<EPI_RES>(h, wk.stream, KC_GEMM_FFN2, g); }
  residual_fields(wk, p, g, wk.lnpart, wk.lnstats, w.ln1g, w.ln1b);
  if (p.x8) { g.A8 = wk.h8; g.W8 = w.w28; g.x8_scale = w.sc_2; }
  if (p.cls_as) { if (int rc = row_term(h, wk, p, wk.cls_lo, g)) return rc; }
  return launch_pp<PP_RESLN3>(h, wk.stream, KC_GEMM_FFN2, g, p.fixed);
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
// groups: the launch groups to run (5 = the layer; fewer only from mv_debug_encode of the development build, encode_dev: 1 the QKV projection, 2 + attention, 3 + the
// output projection, 4 + FFN-1)
int persistent_layer(mv_handle* h, Work& wk, const PassPlan& p, const PassForm& pf, int l, const int32_t* d_ids, const int32_t* d_lens, const float* pend_g, const float* pend_b,
                     int groups = 5) {
  const LayerW& w = h->L[l];
  if (int rc = launch_qkv(h, wk, p, w, false)) return rc;
  if (groups < 2) return MV_OK;
  // the sink census: the layers whose attention launch feeds the concentration monitor, and only where it is attached (a rescoring pass counts nothing twice)
  if (h->census && p.x8 && pf.monitor) {
    ProfScope ps(h, wk.stream, KC_ATTENTION);
    hipLaunchKernelGGL(sink_census_kernel, dim3((unsigned)((p.B * MV_HEADS + 3) / 4)), dim3(256), 0, wk.stream, (const half_t*)wk.q, (const half_t*)wk.k, d_lens,
                       d_ids, p.pitch, p.S_in, p.Sp, p.B * MV_HEADS, h->cfg.vocab_size, h->census_items, h->census_share, h->census_heads + (size_t)l * MV_HEADS);
    if (int rc = launch_check(h, "sink_census")) return rc;
  }
  // K3: attention (cls_as: + the context's special rows' low parts for the output projection's row term)
  if (int rc = launch_attention(h, wk, d_lens, p.B, p.Sp, p.x8, p.cls_as, pf)) return rc;
  if (groups < 3) return MV_OK;
  if (int rc = launch_out_proj(h, wk, p, w, pend_g, pend_b)) return rc;
  if (groups < 4) return MV_OK;
  if (int rc = launch_ffn1(h, wk, p, w)) return rc;
  if (groups < 5) return MV_OK;
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
  MV_TAIL_TAP(TT_Q, wk.cq, MV_HIDDEN * 4, B);
  const half_t* vlo_sp = special_v_lo(wk, p);
  if (p.safe)
    hipLaunchKernelGGL(attention_cls_kernel<true>, dim3((B * MV_HEADS + 3) / 4), dim3(256), 0, wk.stream, wk.cq, wk.k, wk.vt, d_lens, wk.cctx, p.Sp,
                       B * MV_HEADS, wk.pooled, vlo_sp, (const half_t*)wk.k_lo, (const half_t*)wk.vt_lo);
  else
    hipLaunchKernelGGL(attention_cls_kernel<false>, dim3((B * MV_HEADS + 3) / 4), dim3(256), 0, wk.stream, wk.cq, wk.k, wk.vt, d_lens, wk.cctx, p.Sp,
                       B * MV_HEADS, wk.pooled, vlo_sp, (const half_t*)nullptr, (const half_t*)nullptr);
  if (int rc = launch_check(h, "attention_cls")) return rc;
  MV_TAIL_TAP(TT_CTX, wk.pooled, MV_HIDDEN * 4, B);
  hipLaunchKernelGGL((dense768_kernel<4, MV_HIDDEN>), dim3(gx, MV_HIDDEN / 32), dim3(512), 0, wk.stream, (const float*)wk.pooled,
                     (size_t)MV_HIDDEN, B, (const float*)w.woT32, (const float*)w.bo, MV_HIDDEN, wk.c32, (const float*)wk.c32);
  if (int rc = launch_check(h, "cls out")) return rc;
  MV_TAIL_TAP(TT_OUT, wk.c32, MV_HIDDEN * 4, B);
  if (int rc = run_ln(h, wk, wk.c32, wk.c16, B, w.ln1g, w.ln1b)) return rc;
  MV_TAIL_TAP(TT_LN1_32, wk.c32, MV_HIDDEN * 4, B);
  MV_TAIL_TAP(TT_LN1_16, wk.c16, MV_HIDDEN * 2, B);
  hipLaunchKernelGGL((dense768_kernel<3, MV_HIDDEN>), dim3(gx, MV_INTER / 32), dim3(512), 0, wk.stream, (const float*)wk.c32,
                     (size_t)MV_HIDDEN, B, (const float*)w.w1T32, (const float*)w.b1, MV_INTER, wk.ch32, (const float*)nullptr);
  if (int rc = launch_check(h, "cls ffn1")) return rc;
  MV_TAIL_TAP(TT_FFN1, wk.ch32, MV_INTER * 4, B);
  hipLaunchKernelGGL((dense768_kernel<4, MV_INTER>), dim3(gx, MV_HIDDEN / 32), dim3(512), 0, wk.stream, (const float*)wk.ch32,
                     (size_t)MV_INTER, B, (const float*)w.w2T32, (const float*)w.b2, MV_HIDDEN, wk.c32, (const float*)wk.c32);
  if (int rc = launch_check(h, "cls ffn2")) return rc;
  MV_TAIL_TAP(TT_FFN2, wk.c32, MV_HIDDEN * 4, B);
  if (int rc = run_ln(h, wk, wk.c32, wk.c16, B, w.ln2g, w.ln2b)) return rc;
  MV_TAIL_TAP(TT_LN2, wk.c32, MV_HIDDEN * 4, B);
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
  MV_TAIL_TAP(TT_Q, wk.cq, MV_HIDDEN * 4, B);
  hipLaunchKernelGGL(attention_cls_kernel<false>, dim3((B * MV_HEADS + 3) / 4), dim3(256), 0, wk.stream, wk.cq, wk.k, wk.vt,
                     d_lens, wk.cctx, p.Sp, B * MV_HEADS, (float*)nullptr, (const half_t*)nullptr, (const half_t*)nullptr, (const half_t*)nullptr);
  if (int rc = launch_check(h, "attention_cls")) return rc;
  MV_TAIL_TAP(TT_CTX, wk.cctx, MV_HIDDEN * 2, B);
  GemmArgs o = skinny(wk.cctx, w.wo, w.bo, MV_HIDDEN, MV_HIDDEN);
  o.xres = wk.c32;
  if (int rc = launch_small<EPI_RES>(h, wk.stream, KC_CLS_TAIL, o)) return rc;
  MV_TAIL_TAP(TT_OUT, wk.c32, MV_HIDDEN * 4, B);
  if (int rc = run_ln(h, wk, wk.c32, wk.c16, B, w.ln1g, w.ln1b)) return rc;
  MV_TAIL_TAP(TT_LN1_32, wk.c32, MV_HIDDEN * 4, B);
  MV_TAIL_TAP(TT_LN1_16, wk.c16, MV_HIDDEN * 2, B);
  GemmArgs f1 = skinny(wk.c16, w.w1, w.b1, MV_INTER, MV_HIDDEN);
  f1.out16 = wk.ch16;
  if (int rc = launch_small<EPI_GELU>(h, wk.stream, KC_CLS_TAIL, f1)) return rc;
  MV_TAIL_TAP(TT_FFN1, wk.ch16, MV_INTER * 2, B);
  GemmArgs f2 = skinny(wk.ch16, w.w2, w.b2, MV_HIDDEN, MV_INTER);
  f2.xres = wk.c32;
  if (int rc = launch_small<EPI_RES>(h, wk.stream, KC_CLS_TAIL, f2)) return rc;
  MV_TAIL_TAP(TT_FFN2, wk.c32, MV_HIDDEN * 4, B);
  if (int rc = run_ln(h, wk, wk.c32, wk.c16, B, w.ln2g, w.ln2b)) return rc;
  MV_TAIL_TAP(TT_LN2, wk.c32, MV_HIDDEN * 4, B);
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
  MV_TAIL_TAP(TT_GATHER32, wk.c32, MV_HIDDEN * 4, p.B);
  MV_TAIL_TAP(TT_GATHER16, wk.c16, MV_HIDDEN * 2, p.B);
  return p.x8 ? cls_tail_f32(h, wk, p, w, d_lens, u_out) : cls_tail_f16(h, wk, p, w, d_lens, u_out);
}

int encode_dev(mv_handle* h, Work& wk, const int32_t* d_ids, const int32_t* d_lens, int min_len, int B, int S_in, int n_layers, float* u_out,
               const PassForm& pf = PassForm(), bool full = false, int pitch = 0) {  // min_len: the shortest sequence of the pass as the HOST knows it (Pass::min_len; 0 = unknown)
  if (pitch <= 0) pitch = S_in;
  // mv_debug_encode of the development build with its stop switch set (mv_handle::dbg_stop): the pass ends after that many launch groups of its last layer
  const int stop = full ? h->dbg_stop : 0;
  if (h->f32) return encode_f32_dev(h, wk, d_ids, d_lens, B, S_in, n_layers, u_out, pitch, stop);  // MV_F32: no forms, no monitors, no pruning; the stop ends its one path
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
  if (stop && !p.big) return fail(h, MV_ERR_STATE, "mv_debug_encode: the stop inside a layer exists on the persistent path only (this pass takes the small-pass kernels)");
  p.x8 = h->precise;
  p.safe = p.x8 && pf.safe;
  p.prune = !full && h->cls_prune && u_out && n_layers == c.layers && n_layers > 0;
  p.one_seq_tiles = p.Sp == 256 || p.Sp == 512;
  const bool whole_pass = (p.Sp == 192 || p.Sp == 384) && min_len >= h->cls_min_len;
  p.cls_as = p.big && p.x8 && !p.safe && h->cls_aside && (p.one_seq_tiles || whole_pass);
  p.special = p.big && p.x8;
  p.two_plane = two_plane_pass(h, p.x8, p.safe, p.Sp);
  p.qkv_mask = p.safe ? 7 : h->qkv_aside_mask;
  p.fixed = pp_fixed_form(h, p, min_len);
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
  if (stop && n_layers == 0) return MV_OK;  // the embedding kernel's planes as it left them
  if (p.big && n_layers == 0) { if (int rc = final_ln(h, wk, p, pend_g, pend_b)) return rc; }
  for (int l = 0; l < n_layers; ++l) {
    const LayerW& w = h->L[l];
    const bool last = (l == n_layers - 1);
    if (last && p.prune) return pruned_last_layer(h, wk, p, w, d_lens, pend_g, pend_b, u_out);
    if (last && stop) return persistent_layer(h, wk, p, pf, l, d_ids, d_lens, pend_g, pend_b, stop);  // no final LayerNorm, no pooler: the raw planes stay
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

}  // namespace
