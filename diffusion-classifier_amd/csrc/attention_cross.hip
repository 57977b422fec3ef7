// attention_cross.hip — cross-attention: softmax(q k^T * scale) v where keys and values come from ANOTHER tensor (the prompt side
// path) with its own length S, picked per output sample through kv_map (ctx_of_unit), and queries are read through q_map
// (bj_of_unit: the class-shared trunk keeps q once per (image, trial) pair).
//
// Replaces F.scaled_dot_product_attention inside diffusers' Attention (attn2 of BasicTransformerBlock) for a context of several
// tokens; the one-token context needs no kernel (softmax over one key is 1: the class vector of the attn1.to_out epilogue).
//
// Both kernels are the bodies of attn_strip.h; this file adds the addressing (q_map / kv_map, separate ld_q / ld_kv) and the mode:
// 16-bit, d = 32 / 64 / 96 / 128 / 160: attn_strip_run with raw scores (the scale folded into the exponent's FMA), key blocks of 32
// (d >= 64) or 64 keys.  K / V of a launch are small (n_ctx * S rows) and stay in L2: the stream that costs is q in and out back, so the unit of
// work is a query tile.  The last block is ragged: keys >= S are staged as zeros and masked, never read (behind them lies the next
// context, or a gap).  A sample's bits depend on its own q rows and its own context only, not on n or on the position.
// LEN instantiations (dc_cross_attention_len): context c holds kv_len[c] <= S keys in its S rows; the length, uniform over the wave (over
// the workgroup in the fp32 kernel), replaces S in the block count, the prefetch condition, the staging bound and the ragged mask, so
// blocks wholly past it cost nothing and the surviving keys keep their blocks: the bits are those of a context of kv_len[c] rows.
// fp32 and d = 16: attn_exact_run (FMA chain over the keys in order).
// Self-attention is the same problem with q / k / v the three column offsets of a fused QKV tensor, Lq = S = L, ld_q = ld_kv and no
// maps: heads of 160 channels (Stable Diffusion 1.x: 1280 channels in 8 heads, L <= 256), which dc_attention does not serve, run here.
#include <stdio.h>
#include "attn_strip.h"

struct CrossArgs {
  const void* q; const void* k; const void* v; void* out;
  const int32_t* q_map; const int32_t* kv_map;
  int n, Lq, S, heads, d, ld_q, ld_kv, ld_out; float scale;
  int KB;     // fp32 kernel: keys per LDS block
  const int32_t* kv_len;   // LEN instantiations only: keys per context, clamped into [1, S] by the kernel
};

// keys per block: an LDS strip small enough for 2 - 4 workgroups per CU and 8 staging chunks per lane and operand at most — but
// for D = 160: 32 keys are 32 * 20 / 64 = 10 chunks per lane, and four waves' K and V strips 4 * 2 * 32 * 168 * 2 B = 86 KB, one
// workgroup per CU (at 64 keys they would take 172 KB, more than the CU's 160 KB)
static constexpr int cross_kb(int D) { return D <= 32 ? 64 : 32; }

// output sample i, head h (of width d): q rows through q_map, the context's k / v rows through kv_map, its S rows apart whatever its length
template <typename T, bool LEN>
__device__ __forceinline__ StripView<T> cross_view(const CrossArgs& a, int i, int h, int d, int q0, int KB) {
  const int qs = a.q_map ? a.q_map[i] : i, cs = a.kv_map ? a.kv_map[i] : i;
  const int len = LEN ? clamped_len(a.kv_len, cs, a.S) : a.S;
  const size_t kv0 = (size_t)cs * a.S * a.ld_kv + h * d;
  return {reinterpret_cast<const T*>(a.q) + (size_t)qs * a.Lq * a.ld_q + h * d, reinterpret_cast<const T*>(a.k) + kv0,
          reinterpret_cast<const T*>(a.v) + kv0, reinterpret_cast<T*>(a.out) + (size_t)i * a.Lq * a.ld_out + h * d,
          a.ld_q, a.ld_kv, a.ld_out, q0, a.Lq, a.Lq, len, (len + KB - 1) / KB, len / KB};
}

template <typename T, int D, bool LEN>
__global__ __launch_bounds__(256) void attn_cross_kernel(const CrossArgs a) {
  constexpr int KB = cross_kb(D);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int wave, i, h, q0;
  if (!strip_item(a.n, a.heads, a.Lq, wave, i, h, q0)) return;
  const StripView<T> w = cross_view<T, LEN>(a, i, h, D, q0, KB);
  PlainMode mode{{w.nk}};                                    // the keys stop at the context's length (S without LEN)
  T *Kl, *Vl;
  strip_lds<T, D, KB>(smem, wave, Kl, Vl);
  attn_strip_run<T, D, KB>(w, mode, a.scale, Kl, Vl);
}

template <typename T, int D, bool LEN>
static int launch_cross(const CrossArgs& a, hipStream_t s, const char* fn) {
  constexpr size_t lds = strip_lds_bytes<T, D, cross_kb(D)>();
  static bool done = false;
  if (!done) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_cross_kernel<T, D, LEN>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); done = true; }
  return strip_launch(attn_cross_kernel<T, D, LEN>, a, (long long)a.n * a.heads * ((a.Lq + 31) / 32), lds, s, fn,
                      LEN ? "dc_cross_attention_len(mfma)" : "dc_cross_attention(mfma)");
}

// Exact fp32 kernel (f32, d = 16, and operands the matrix-core kernel's 16-byte loads cannot take): SW = 16; 24 for d = 96 and 20 for
// d = 160 (eight lanes a query: the xor-shuffle reduction needs a power-of-two lane count).  The length
// is uniform over the workgroup, as the barriers need.
template <typename T, int SW, bool LEN>
__global__ __launch_bounds__(256) void attn_cross_f32_kernel(const CrossArgs a) {
  extern __shared__ __attribute__((aligned(16))) float kv[];  // K[KB][d], V[KB][d]
  int i, h, q0;
  exact_item(a.heads, a.Lq, 256 / (a.d / SW), i, h, q0);
  const StripView<T> w = cross_view<T, LEN>(a, i, h, a.d, q0, a.KB);
  attn_exact_run<T, SW>(w, PlainMode{{w.nk}}, a.scale, a.d, a.KB, kv);
}

// `fn`: the entry point's name in front of every message (dc_cross_attention / dc_cross_attention_len validate alike); kv_len: the
// length array of dc_cross_attention_len (null elsewhere)
static int cross_validate(const dc_cross_attention_params* p, const char* fn, const int32_t* kv_len = nullptr) {
  DC_REQUIRE(p && p->q && p->k && p->v && p->out, DC_ERR_ARG, "%s: null pointer", fn);
  DC_REQUIRE(p->dtype == DC_F32 || p->dtype == DC_BF16 || p->dtype == DC_F16, DC_ERR_DTYPE, "%s: dtype %d", fn, p->dtype);
  DC_REQUIRE(p->d == 16 || p->d == 32 || p->d == 64 || p->d == 96 || p->d == 128 || p->d == 160, DC_ERR_SHAPE, "%s: head dim %d (16/32/64/96/128/160)", fn, p->d);
  DC_REQUIRE(p->n > 0 && p->Lq > 0 && p->heads > 0, DC_ERR_SHAPE, "%s: n/Lq/heads", fn);
  DC_REQUIRE(p->S >= 1, DC_ERR_SHAPE, "%s: S=%d (at least one key)", fn, p->S);
  DC_REQUIRE(p->ld_q >= p->heads * p->d && p->ld_kv >= p->heads * p->d && p->ld_out >= p->heads * p->d, DC_ERR_SHAPE, "%s: ld", fn);
  // as seq_attn_validate: the kernels index q / k / v / out by element and the maps and lengths as int32
  DC_REQUIRE((((uintptr_t)p->q_map | (uintptr_t)p->kv_map | (uintptr_t)kv_len) & 3) == 0, DC_ERR_ALIGN, "%s: q_map / kv_map / kv_len must be 4-byte aligned", fn);
  const uintptr_t es = (uintptr_t)dc_dtype_size(p->dtype) - 1;
  DC_REQUIRE((((uintptr_t)p->q | (uintptr_t)p->k | (uintptr_t)p->v | (uintptr_t)p->out) & es) == 0, DC_ERR_ALIGN, "%s: q/k/v/out must be element aligned", fn);
  // the matrix-core kernel keeps the running max of the RAW scores and folds the scale into the exponent's FMA: valid for scale > 0 only
  DC_REQUIRE(p->scale > 0.f, DC_ERR_ARG, "%s: scale must be positive (got %g)", fn, (double)p->scale);
  return DC_OK;
}

// matrix cores: d = 32 / 64 / 96 / 128 / 160 on the strip route
static bool cross_mfma_ok(const dc_cross_attention_params* p) {
  return (p->d == 32 || p->d == 64 || p->d == 96 || p->d == 128 || p->d == 160) && strip_route_ok(p->dtype, p->q, p->k, p->v, p->out, p->ld_q, p->ld_kv, p->ld_out);
}

// validated parameters -> the launch; LEN: the instantiations that read a.kv_len
template <bool LEN>
static int cross_launch(const dc_cross_attention_params* p, const int32_t* kv_len, dc_stream stream, const char* fn) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  CrossArgs a{p->q, p->k, p->v, p->out, p->q_map, p->kv_map, p->n, p->Lq, p->S, p->heads, p->d, p->ld_q, p->ld_kv, p->ld_out, p->scale, 0, kv_len};
  char what[40];
  snprintf(what, sizeof(what), "%s: dtype", fn);
  if (cross_mfma_ok(p))
    return dc_by_dtype16(p->dtype, what, [&](auto t) {
      using T = decltype(t);
      if (p->d == 32) return launch_cross<T, 32, LEN>(a, s, fn);
      if (p->d == 64) return launch_cross<T, 64, LEN>(a, s, fn);
      if (p->d == 96) return launch_cross<T, 96, LEN>(a, s, fn);
      if (p->d == 128) return launch_cross<T, 128, LEN>(a, s, fn);
      return launch_cross<T, 160, LEN>(a, s, fn);
    });
  const int SW = p->d == 96 ? 24 : p->d == 160 ? 20 : 16;
  ExactPlan e;
  const int rc = exact_plan(p->n, p->heads, p->Lq, p->S, p->d, SW, fn, e);
  if (rc != DC_OK) return rc;
  a.KB = e.KB;
  return dc_by_dtype(p->dtype, what, [&](auto t) {
    using T = decltype(t);
    void (*kern)(const CrossArgs) = SW == 24 ? attn_cross_f32_kernel<T, 24, LEN> : SW == 20 ? attn_cross_f32_kernel<T, 20, LEN> : attn_cross_f32_kernel<T, 16, LEN>;
    hipLaunchKernelGGL(kern, dim3(e.nb), dim3(256), e.lds, s, a);
    return dc_check_launch(fn);
  });
}

extern "C" const char* dc_cross_attention_variant(const dc_cross_attention_params* p) {
  if (cross_validate(p, "dc_cross_attention") != DC_OK) return "invalid";
  return cross_mfma_ok(p) ? "mfma" : "fp32";
}

extern "C" int dc_cross_attention(const dc_cross_attention_params* p, dc_stream stream) {
  const int rc = cross_validate(p, "dc_cross_attention");
  if (rc != DC_OK) return rc;
  return cross_launch<false>(p, nullptr, stream, "dc_cross_attention");
}

// dc_cross_attention_len: the same problem with kv_len keys per context.  Everything but kv_len is validated and routed as above.
static dc_cross_attention_params cross_base(const dc_cross_attention_len_params* p) {
  return dc_cross_attention_params{p->q, p->k, p->v, p->out, p->q_map, p->kv_map, p->dtype, p->n, p->Lq, p->S, p->heads, p->d,
                                   p->ld_q, p->ld_kv, p->ld_out, p->scale};
}

extern "C" const char* dc_cross_attention_len_variant(const dc_cross_attention_len_params* p) {
  if (!p) return "invalid";
  const dc_cross_attention_params b = cross_base(p);
  if (cross_validate(&b, "dc_cross_attention_len", p->kv_len) != DC_OK) return "invalid";
  return cross_mfma_ok(&b) ? "mfma" : "fp32";
}

extern "C" int dc_cross_attention_len(const dc_cross_attention_len_params* p, dc_stream stream) {
  DC_REQUIRE(p, DC_ERR_ARG, "dc_cross_attention_len: null pointer");
  const dc_cross_attention_params b = cross_base(p);
  const int rc = cross_validate(&b, "dc_cross_attention_len", p->kv_len);
  if (rc != DC_OK) return rc;
  // no lengths: every context has S keys, which is dc_cross_attention's launch
  if (!p->kv_len) return cross_launch<false>(&b, nullptr, stream, "dc_cross_attention_len");
  return cross_launch<true>(&b, p->kv_len, stream, "dc_cross_attention_len");
}
