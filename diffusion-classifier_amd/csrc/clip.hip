// clip.hip — the kernels a CLIP text transformer needs besides dc_igemm: causal self-attention with a row count per sample
// (dc_attention_causal), a LayerNorm with weight and bias that reads one type and writes another (dc_layernorm_rows), the token +
// position embedding (dc_embed_rows_pos) and the feed-forward's activation as a pass of its own (dc_act_pass: quick-GELU or erf-GELU).
//
// dc_attention_causal runs the two bodies of attn_strip.h (16-bit with d = 64 and 16-byte aligned rows: "mfma", attn_strip_run over key
// blocks of 32 with raw scores, exactly as cross-attention's; everything else: "fp32", attn_exact_run) with the causal structure:
//   * a wave whose queries start at q0 (a multiple of 32) walks the key blocks 0 .. q0 / 32 only: blocks above the diagonal are neither
//     fetched nor multiplied (the exact kernel's workgroup streams the keys up to its last query);
//   * only the diagonal block (keys q0 .. q0 + 31) applies the per-element mask k > q, BEFORE the running max, so a masked score never
//     enters it.  Every query keeps key 0 of block 0 and key q0 <= q of the diagonal block: no row of a block is ever fully masked, the
//     running max is finite after every block, and a masked position carries P = exp2(-inf - finite) = 0 exactly;
//   * the sample's length row_len[i] (clamped into [1, L]) bounds the queries; the causal mask already hides every key >= the length
//     from every query below it, so the length needs no key mask of its own.  Rows >= the length of q / k / v are never read (keys of
//     the diagonal block past the length are staged as zeros: a pad query of a live tile meets 0 x 0, never 0 x garbage), tiles of pad
//     queries store zeros and leave, pad rows inside a live tile are written as zeros.
// Fixed summation order, no atomics: the bits of a row depend on rows 0 .. q of its own sample only — they are those of cross-attention
// over the keys 0 .. q.
//
// dc_act_pass exists for the reason dc_relu does: dc_igemm, its dispatcher and the shared epilogue stay as they are.
#include <stdio.h>
#include "attn_strip.h"
#include "row_ops.h"

static constexpr int CA_KB = 32;    // keys per block = queries per wave: block q0 / 32 is the diagonal one

// key > query is masked: in the diagonal block alone on the matrix-core route, at every key on the exact one
struct CausalMode {
  static constexpr bool kZeroPad = true, kBiased = false;
  template <bool LAST> __device__ __forceinline__ bool masked(int key, int query) const { return LAST && key > query; }
};

template <typename T, int D>
__global__ __launch_bounds__(256) void attn_causal_kernel(const SeqAttnArgs a) {
  constexpr int KB = CA_KB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int wave, i, h, q0;
  if (!strip_item(a.n, a.heads, a.L, wave, i, h, q0)) return;
  StripView<T> w = seq_view<T>(a, i, h, D, q0);
  w.nplain = q0 / KB; w.nblk = w.nplain + 1;                  // nothing above the diagonal block, the only one with masked positions
  T *Kl, *Vl;
  strip_lds<T, D, KB>(smem, wave, Kl, Vl);
  CausalMode mode;
  attn_strip_run<T, D, KB>(w, mode, a.scale, Kl, Vl);
}

template <typename T>
__global__ __launch_bounds__(256) void attn_causal_f32_kernel(const SeqAttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float kv[];  // K[KB][d], V[KB][d]
  const int QT = 256 / (a.d / 16);
  int i, h, q0;
  exact_item(a.heads, a.L, QT, i, h, q0);
  StripView<T> w = seq_view<T>(a, i, h, a.d, q0);             // the length is uniform over the workgroup, as the barriers need
  w.nk = min(w.nk, q0 + QT);                                  // (uniform) the keys this workgroup's queries can see
  attn_exact_run<T, 16>(w, CausalMode{}, a.scale, a.d, a.KB, kv);
}

static int causal_validate(const dc_attention_causal_params* p) {
  return seq_attn_validate(p, "dc_attention_causal", DC_ATTENTION_CAUSAL_MAX_L, true, p ? (uintptr_t)p->row_len : 0, "row_len");
}

extern "C" const char* dc_attention_causal_variant(const dc_attention_causal_params* p) {
  if (causal_validate(p) != DC_OK) return "invalid";
  return seq_attn_mfma_ok(p) ? "mfma" : "fp32";
}

extern "C" int dc_attention_causal(const dc_attention_causal_params* p, dc_stream stream) {
  const int rc = causal_validate(p);
  if (rc != DC_OK) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SeqAttnArgs a{p->q, p->k, p->v, p->out, p->row_len, p->n, p->L, p->heads, p->d, p->ld_qkv, p->ld_out, p->scale, 0};
  return seq_attn_dispatch(p, a, "dc_attention_causal",
                           [&](auto t) {
                             using T = decltype(t);
                             return strip_launch(attn_causal_kernel<T, 64>, a, (long long)a.n * a.heads * ((a.L + CA_KB - 1) / CA_KB),
                                                 strip_lds_bytes<T, 64, CA_KB>(), s, "dc_attention_causal", "dc_attention_causal(mfma)");   // 36 KiB
                           },
                           [&](auto t, const ExactPlan& e) {
                             hipLaunchKernelGGL(attn_causal_f32_kernel<decltype(t)>, dim3(e.nb), dim3(256), e.lds, s, a);
                             return dc_check_launch("dc_attention_causal(fp32)");
                           });
}

// ------------------------------------------------------------------------------------------------
// LayerNorm with weight and bias, x read in one type and y written in another: one wave per row (4 rows per workgroup), fp32 statistics
// in a fixed order — the mean (per-lane strided partial sums, then the xor butterfly), then the centred second moment the same way.
// Rows at or past their sample's row_len are written as zeros and not read.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void layernorm_rows_kernel(const dc_layernorm_rows_params p) {
  const int lane = threadIdx.x & 63;
  const TI* x; TO* y;
  if (!norm_row(p, lane, x, y)) return;
  float sum = 0.f;
  for (int c = lane; c < p.C; c += 64) sum += Elem<TI>::to_f(x[c]);
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
  const float mean = sum / (float)p.C;
  float ss = 0.f;
  for (int c = lane; c < p.C; c += 64) { const float v = Elem<TI>::to_f(x[c]) - mean; ss = __builtin_fmaf(v, v, ss); }
  for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
  const float rs = 1.0f / sqrtf(ss / (float)p.C + p.eps);
  for (int c = lane; c < p.C; c += 64) y[c] = Elem<TO>::from_f((Elem<TI>::to_f(x[c]) - mean) * rs * p.gamma[c] + p.beta[c]);
}

extern "C" int dc_layernorm_rows(const dc_layernorm_rows_params* p, dc_stream stream) {
  DC_REQUIRE(p && p->x && p->y && p->gamma && p->beta, DC_ERR_ARG, "dc_layernorm_rows: null pointer");
  DC_REQUIRE((unsigned)p->dtype <= DC_F16 && (unsigned)p->out_dtype <= DC_F16, DC_ERR_DTYPE, "dc_layernorm_rows: dtype %d -> %d", p->dtype, p->out_dtype);
  DC_REQUIRE(p->rows > 0 && p->C > 0 && p->rows_per_sample > 0 && p->rows % p->rows_per_sample == 0, DC_ERR_SHAPE,
             "dc_layernorm_rows: rows=%d C=%d rows_per_sample=%d", p->rows, p->C, p->rows_per_sample);
  DC_REQUIRE(p->eps >= 0.f, DC_ERR_ARG, "dc_layernorm_rows: eps must not be negative (got %g)", (double)p->eps);
  DC_REQUIRE((((uintptr_t)p->x) & (dc_dtype_size(p->dtype) - 1)) == 0 && (((uintptr_t)p->y) & (dc_dtype_size(p->out_dtype) - 1)) == 0 &&
             ((((uintptr_t)p->gamma | (uintptr_t)p->beta | (uintptr_t)p->row_len)) & 3) == 0, DC_ERR_ALIGN, "dc_layernorm_rows: pointers must be element aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned nb = (unsigned)((p->rows + 3) / 4);
  return dc_by_dtype(p->dtype, "dc_layernorm_rows: dtype", [&](auto ti) {
    return dc_by_dtype(p->out_dtype, "dc_layernorm_rows: out_dtype", [&](auto to) {
      hipLaunchKernelGGL((layernorm_rows_kernel<decltype(ti), decltype(to)>), dim3(nb), dim3(256), 0, s, *p);
      return dc_check_launch("dc_layernorm_rows");
    });
  });
}

extern "C" int dc_embed_rows_pos(const dc_embed_rows_pos_params* p, dc_stream stream) {
  DC_REQUIRE(p, DC_ERR_ARG, "dc_embed_rows_pos: null pointer");
  return embed_rows_launch<true>(*p, stream, "dc_embed_rows_pos");
}

// ------------------------------------------------------------------------------------------------
// x = act(x) in place (inplace_pass_kernel), evaluated in fp32 and rounded once to the storage type; NaN stays NaN.
//   quick-GELU  x * sigmoid(1.702 x)              (OpenAI CLIP)
//   erf-GELU    x * Phi(x) = 0.5 x erfc(-x / sqrt 2)   (OpenCLIP): erfc keeps the relative accuracy of the negative tail, where
//               1 + erf(x / sqrt 2) cancels to zero in fp32
template <int KIND> struct ActPassOp {
  static __device__ __forceinline__ float f(float x) {
    if constexpr (KIND == DC_PASS_QUICK_GELU) return x * (1.0f / (1.0f + expf(-1.702f * x)));
    else return 0.5f * x * erfcf(-0.70710678118654752f * x);
  }
  template <typename T> static __device__ __forceinline__ T run(T v) { return Elem<T>::from_f(f(Elem<T>::to_f(v))); }
};

extern "C" int dc_act_pass(const dc_act_pass_params* p, dc_stream stream) {
  DC_REQUIRE(p && p->x, DC_ERR_ARG, "dc_act_pass: null pointer");
  DC_REQUIRE((unsigned)p->dtype <= DC_F16, DC_ERR_DTYPE, "dc_act_pass: dtype %d", p->dtype);
  DC_REQUIRE(p->kind == DC_PASS_QUICK_GELU || p->kind == DC_PASS_GELU_ERF, DC_ERR_ARG, "dc_act_pass: kind %d", p->kind);
  return inplace_pass_launch(p->x, (long long)p->n, p->dtype, stream, "dc_act_pass", [&](auto t, dim3 nb, hipStream_t s) {
    using T = decltype(t);
    if (p->kind == DC_PASS_QUICK_GELU) hipLaunchKernelGGL((inplace_pass_kernel<T, ActPassOp<DC_PASS_QUICK_GELU>>), nb, dim3(256), 0, s, reinterpret_cast<T*>(p->x), (long long)p->n);
    else hipLaunchKernelGGL((inplace_pass_kernel<T, ActPassOp<DC_PASS_GELU_ERF>>), nb, dim3(256), 0, s, reinterpret_cast<T*>(p->x), (long long)p->n);
  });
}
