// t5.hip — the kernels a T5 (v1.0) encoder stack needs besides dc_igemm: self-attention with an additive relative-position bias and a
// key count per sample (dc_attention_bias), RMS norm (dc_rmsnorm), the token-embedding gather (dc_embed_rows) and ReLU (dc_relu).
//
// dc_attention_bias runs the two bodies of attn_strip.h (16-bit with d = 64 and 16-byte aligned rows: "mfma", attn_strip_run over key
// blocks of 32; everything else: "fp32", attn_exact_run) in their biased form:
//   * the score is q k^T * scale + bias[h][k - q + L - 1] and the running max is taken over it (the bias can move the arg max).  On the
//     matrix-core route the 4 consecutive keys of a lane are 4 consecutive table entries: the wave keeps the slice of its head's table
//     that its 32 queries can reach (at most L + 31 entries), pre-multiplied by log2(e), in LDS next to its strips;
//   * the sample's length kv_len[i] (clamped into [1, L]) bounds BOTH the keys and the queries: rows >= the length of q / k / v are never
//     read (staged as zeros and masked), key blocks wholly past the length are skipped, output rows >= the length are written as zeros.
// Fixed summation order, no atomics: the bits of a sample depend on its own rows, its own length and the table only.
//
// dc_relu exists so that dc_igemm and its shared epilogue stay as they are: ReLU as a dc_igemm activation would save this pass over
// [rows, d_ff] and is the measured follow-up.
#include <stdio.h>
#include "attn_strip.h"
#include "row_ops.h"

struct BiasAttnArgs : SeqAttnArgs {
  const float* bias;
  int TBL;    // mfma kernel: floats of the per-wave table slice (L + 64: the last key block's masked lanes index up to L + 61)
};

static constexpr int BA_KB = 32;    // keys per block

// matrix-core mode.  Table slice of the wave, in log2 units: Tb[j] = bt[j + tb0] * log2(e) for key k and query q at j = k + (q0 + 31 - q),
// i.e. j = 0 .. len + 30; entries outside the head's table bt (queries that do not exist) are zero and never used.  A lookup is in range
// for every lane (j <= k0 + KB + 30 <= L + 61 < TBL); the entries of keys >= len are never written and never used (they are masked):
// their slots hold what LDS held, finite or not.
struct BiasStrip : KeyBound {
  static constexpr bool kZeroPad = true, kBiased = true;
  float* Tb; const float* bt; int L, q0;
  __device__ __forceinline__ void prologue(int lane) const {
    const int tb0 = L - 1 - (q0 + 31);
    for (int j = lane; j < len + 31; j += 64) {
      const int t = j + tb0;
      Tb[j] = (t >= 0 && t < 2 * L - 1) ? bt[t] * 1.4426950408889634f : 0.f;
    }
  }
  __device__ __forceinline__ float bias(int key, int query) const { return Tb[key + 31 - (query - q0)]; }
};

// exact mode: the head's table as it is
struct BiasExact : KeyBound {
  static constexpr bool kZeroPad = true, kBiased = true;
  const float* bt; int L;
  __device__ __forceinline__ float bias(int key, int query) const { return bt[key - query + L - 1]; }
};

template <typename T, int D>
__global__ __launch_bounds__(256) void attn_bias_kernel(const BiasAttnArgs a) {
  constexpr int KB = BA_KB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int wave, i, h, q0;
  if (!strip_item(a.n, a.heads, a.L, wave, i, h, q0)) return;
  StripView<T> w = seq_view<T>(a, i, h, D, q0);
  w.nblk = (w.nk + KB - 1) / KB; w.nplain = w.nk / KB;        // the last block is ragged when the length is no multiple of KB
  T *Kl, *Vl;
  strip_lds<T, D, KB>(smem, wave, Kl, Vl);
  float* const Tb = reinterpret_cast<float*>(smem + strip_lds_bytes<T, D, KB>()) + (size_t)wave * a.TBL;
  BiasStrip mode{{w.nk}, Tb, a.bias + (size_t)h * (2 * a.L - 1), a.L, q0};
  attn_strip_run<T, D, KB>(w, mode, a.scale, Kl, Vl);
}

template <typename T, int D>
static int launch_bias_mfma(const BiasAttnArgs& a, hipStream_t s) {
  constexpr size_t strips = strip_lds_bytes<T, D, BA_KB>();
  static bool done = false;
  if (!done) {      // the largest launch there is: L = DC_ATTENTION_BIAS_MAX_L
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_bias_kernel<T, D>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(strips + (size_t)4 * (DC_ATTENTION_BIAS_MAX_L + 64) * sizeof(float)));
    done = true;
  }
  return strip_launch(attn_bias_kernel<T, D>, a, (long long)a.n * a.heads * ((a.L + 31) / 32), strips + (size_t)4 * a.TBL * sizeof(float), s,
                      "dc_attention_bias", "dc_attention_bias(mfma)");
}

template <typename T>
__global__ __launch_bounds__(256) void attn_bias_f32_kernel(const BiasAttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float kv[];  // K[KB][d], V[KB][d]
  int i, h, q0;
  exact_item(a.heads, a.L, 256 / (a.d / 16), i, h, q0);
  const StripView<T> w = seq_view<T>(a, i, h, a.d, q0);       // the length is uniform over the workgroup, as the barriers need
  attn_exact_run<T, 16>(w, BiasExact{{w.nk}, a.bias + (size_t)h * (2 * a.L - 1), a.L}, a.scale, a.d, a.KB, kv);
}

static int bias_validate(const dc_attention_bias_params* p) {
  return seq_attn_validate(p, "dc_attention_bias", DC_ATTENTION_BIAS_MAX_L, p && p->bias, p ? (uintptr_t)p->bias | (uintptr_t)p->kv_len : 0, "bias / kv_len");
}

extern "C" const char* dc_attention_bias_variant(const dc_attention_bias_params* p) {
  if (bias_validate(p) != DC_OK) return "invalid";
  return seq_attn_mfma_ok(p) ? "mfma" : "fp32";
}

extern "C" int dc_attention_bias(const dc_attention_bias_params* p, dc_stream stream) {
  const int rc = bias_validate(p);
  if (rc != DC_OK) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  BiasAttnArgs a{{p->q, p->k, p->v, p->out, p->kv_len, p->n, p->L, p->heads, p->d, p->ld_qkv, p->ld_out, p->scale, 0}, p->bias, p->L + 64};
  return seq_attn_dispatch(p, a, "dc_attention_bias", [&](auto t) { return launch_bias_mfma<decltype(t), 64>(a, s); },
                           [&](auto t, const ExactPlan& e) {
                             hipLaunchKernelGGL(attn_bias_f32_kernel<decltype(t)>, dim3(e.nb), dim3(256), e.lds, s, a);
                             return dc_check_launch("dc_attention_bias(fp32)");
                           });
}

// ------------------------------------------------------------------------------------------------
// RMS norm: y = x * rsqrt(mean(x^2) + eps) * weight per row, one wave per row (4 rows per workgroup), fp32 statistics summed in a fixed
// order (per-lane strided partial sums, then the xor butterfly).  Rows at or past their sample's row_len are written as zeros and not read.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void rmsnorm_kernel(const dc_rmsnorm_params p) {
  const int lane = threadIdx.x & 63;
  const TI* x; TO* y;
  if (!norm_row(p, lane, x, y)) return;
  float ss = 0.f;
  for (int c = lane; c < p.C; c += 64) { const float v = Elem<TI>::to_f(x[c]); ss = __builtin_fmaf(v, v, ss); }
  for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
  const float rs = 1.0f / sqrtf(ss / (float)p.C + p.eps);
  for (int c = lane; c < p.C; c += 64) y[c] = Elem<TO>::from_f(Elem<TI>::to_f(x[c]) * rs * p.weight[c]);
}

static int rmsnorm_validate(const dc_rmsnorm_params* p) {
  DC_REQUIRE(p && p->x && p->y && p->weight, DC_ERR_ARG, "dc_rmsnorm: null pointer");
  DC_REQUIRE((unsigned)p->dtype <= DC_F16 && (unsigned)p->out_dtype <= DC_F16, DC_ERR_DTYPE, "dc_rmsnorm: dtype %d -> %d", p->dtype, p->out_dtype);
  DC_REQUIRE(p->rows > 0 && p->C > 0 && p->rows_per_sample > 0 && p->rows % p->rows_per_sample == 0, DC_ERR_SHAPE,
             "dc_rmsnorm: rows=%d C=%d rows_per_sample=%d", p->rows, p->C, p->rows_per_sample);
  DC_REQUIRE(p->eps >= 0.f, DC_ERR_ARG, "dc_rmsnorm: eps must not be negative (got %g)", (double)p->eps);
  DC_REQUIRE((((uintptr_t)p->x) & (dc_dtype_size(p->dtype) - 1)) == 0 && (((uintptr_t)p->y) & (dc_dtype_size(p->out_dtype) - 1)) == 0 &&
             ((((uintptr_t)p->weight | (uintptr_t)p->row_len)) & 3) == 0, DC_ERR_ALIGN, "dc_rmsnorm: pointers must be element aligned");
  return DC_OK;
}

extern "C" int dc_rmsnorm(const dc_rmsnorm_params* p, dc_stream stream) {
  const int rc = rmsnorm_validate(p);
  if (rc != DC_OK) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned nb = (unsigned)((p->rows + 3) / 4);
  return dc_by_dtype(p->dtype, "dc_rmsnorm: dtype", [&](auto ti) {
    return dc_by_dtype(p->out_dtype, "dc_rmsnorm: out_dtype", [&](auto to) {
      hipLaunchKernelGGL((rmsnorm_kernel<decltype(ti), decltype(to)>), dim3(nb), dim3(256), 0, s, *p);
      return dc_check_launch("dc_rmsnorm");
    });
  });
}

extern "C" int dc_embed_rows(const dc_embed_rows_params* p, dc_stream stream) {
  DC_REQUIRE(p, DC_ERR_ARG, "dc_embed_rows: null pointer");
  return embed_rows_launch<false>(dc_embed_rows_pos_params{p->table, nullptr, p->ids, p->out, p->out_dtype, p->rows, p->C, p->vocab, 0, 0}, stream, "dc_embed_rows");
}

// x = max(x, 0): a negative element becomes zero, every other one — NaN as torch.relu, -0, subnormals — is handed back as it is
struct ReluOp {
  template <typename T> static __device__ __forceinline__ T run(T v) { return Elem<T>::to_f(v) < 0.f ? Elem<T>::from_f(0.f) : v; }
};

extern "C" int dc_relu(const dc_relu_params* p, dc_stream stream) {
  DC_REQUIRE(p && p->x, DC_ERR_ARG, "dc_relu: null pointer");
  return inplace_pass_launch(p->x, (long long)p->n, p->dtype, stream, "dc_relu", [&](auto t, dim3 nb, hipStream_t s) {
    using T = decltype(t);
    hipLaunchKernelGGL((inplace_pass_kernel<T, ReluOp>), nb, dim3(256), 0, s, reinterpret_cast<T*>(p->x), (long long)p->n);
  });
}
