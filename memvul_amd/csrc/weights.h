// Part of engine.hip: the weights — the staged host tensors looked up and checked (find / need), converted for the compute dtype (fp16, the folded
// LayerNorm, the fp8 planes of MV_F16X8, the fp32 forms) and uploaded; upload_weights is mv_finalize_weights' whole upload.

namespace {

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

// mv_finalize_weights' uploads, on workspace set 0's stream: every staged tensor the model needs checked, brought into the forms of the compute dtype and uploaded
int upload_weights(mv_handle* h, bool precise, bool f32) {
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
  return MV_OK;
}

}  // namespace
