// t5.hip — the kernels a T5 (v1.0) encoder stack needs besides dc_igemm: self-attention with an additive relative-position bias and a
// key count per sample (dc_attention_bias), RMS norm (dc_rmsnorm), the token-embedding gather (dc_embed_rows) and ReLU (dc_relu).
//
// dc_attention_bias, 16-bit with d = 64 and 16-byte aligned rows ("mfma"): the transposed-score structure of attn_cross_kernel
// (attention_cross.hip) — one WAVE per (sample, head, 32 queries), wave-private K / V strips in LDS, nothing shared between waves and
// therefore no workgroup barrier; S^T = K Q^T on the 16x16x32 MFMA so that a lane holds 4 consecutive KEYS of ONE query, online fp32
// softmax in log2 units over key blocks of 32, O^T += V^T P^T with transposed LDS reads of the row-major V strip.  What differs:
//   * the score is q k^T * scale + bias[h][k - q + L - 1]: the 4 consecutive keys of a lane are 4 consecutive table entries.  The wave
//     keeps the slice of its head's table that its 32 queries can reach (at most L + 31 entries), pre-multiplied by log2(e), in LDS next
//     to its strips; the running max is taken over the biased scores (the bias can move the arg max);
//   * the sample's length kv_len[i] (clamped into [1, L]) bounds BOTH the keys and the queries: rows >= the length of q / k / v are never
//     read (staged as zeros and masked), key blocks wholly past the length are skipped, output rows >= the length are written as zeros.
// Fixed summation order, no atomics: the bits of a sample depend on its own rows, its own length and the table only.
// d = 32 / 128 would come from the same template but are not instantiated (nothing here needs them): they take the exact kernel.
//
// fp32, d = 16 / 32 / 128 and unaligned operands ("fp32"): the exact kernel of attention_cross.hip (K / V of one (sample, head) stream
// through LDS as f32, FMA chain over the keys in order, online softmax key by key), with the bias added to each score.
//
// dc_relu exists so that dc_igemm and its shared epilogue stay as they are: ReLU as a dc_igemm activation would save this pass over
// [rows, d_ff] and is the measured follow-up.
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>
#include "igemm_common.h"
#include "attn_lanes.h"

struct BiasAttnArgs {
  const void* q; const void* k; const void* v; void* out;
  const float* bias; const int32_t* kv_len;
  int n, L, heads, d, ld_qkv, ld_out; float scale;
  int KB;     // fp32 kernel: keys per LDS block
  int TBL;    // mfma kernel: floats of the per-wave table slice (L + 64: the last key block's masked lanes index up to L + 61)
};

// rows of sample i that exist: device data, clamped rather than trusted; uniform -> the scalar path
__device__ __forceinline__ int bias_len(const BiasAttnArgs& a, int i) {
  return a.kv_len ? __builtin_amdgcn_readfirstlane(min(max(a.kv_len[i], 1), a.L)) : a.L;
}

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

static constexpr int BA_KB = 32;    // keys per block

template <typename T, int D>
__global__ __launch_bounds__(256) void attn_bias_kernel(const BiasAttnArgs a) {
  constexpr int KB = BA_KB;
  constexpr int NKT = KB / 16, NQT = 2, NDT = D / 16, NKB = D / 32;
  constexpr int PITCH = D + 8, CPR = D / 8;                   // LDS row pitch in elements (+16 B); 16-byte chunks per row
  constexpr int NCH = KB * CPR / 64;                          // staging chunks per lane and operand
  static_assert(KB * CPR % 64 == 0 && NKT % 2 == 0 && D % 32 == 0, "whole staging chunks, key tiles in pairs, 32-wide k-chunks");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane & 15, lq = lane >> 4;
  const int L = a.L;
  const int qtiles = (L + 16 * NQT - 1) / (16 * NQT);
  long long item = (long long)blockIdx.x * 4 + wave;
  if (item >= (long long)a.n * a.heads * qtiles) return;      // whole waves leave: nothing below is shared between waves
  const int qt_i = (int)(item % qtiles); item /= qtiles;
  const int h = (int)(item % a.heads), i = (int)(item / a.heads);
  T* const Kl = reinterpret_cast<T*>(smem) + (size_t)wave * 2 * KB * PITCH;
  T* const Vl = Kl + KB * PITCH;
  float* const Tb = reinterpret_cast<float*>(smem + (size_t)4 * 2 * KB * PITCH * sizeof(T)) + (size_t)wave * a.TBL;
  const T* qg = reinterpret_cast<const T*>(a.q) + (size_t)i * L * a.ld_qkv + h * D;
  const T* kg = reinterpret_cast<const T*>(a.k) + (size_t)i * L * a.ld_qkv + h * D;
  const T* vg = reinterpret_cast<const T*>(a.v) + (size_t)i * L * a.ld_qkv + h * D;
  T* const og = reinterpret_cast<T*>(a.out) + (size_t)i * L * a.ld_out + h * D;
  const int len = bias_len(a, i);                             // rows of this sample (L without kv_len); the samples stay L rows apart
  const int q0 = qt_i * 16 * NQT;
  const int nqt = q0 < len ? min(NQT, (len - q0 + 15) >> 4) : 0;   // 16-query tiles of this wave that hold a query (wave-uniform)

  if (nqt == 0) {                                             // every query of this wave is padding: zero rows, nothing read
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
      const int qi = q0 + qt * 16 + lr;
      if (qi >= L) continue;
      typename Elem<T>::vec4 z;
#pragma unroll
      for (int r = 0; r < 4; ++r) z[r] = Elem<T>::from_f(0.f);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) *reinterpret_cast<typename Elem<T>::vec4*>(og + (size_t)qi * a.ld_out + dt * 16 + lq * 4) = z;
    }
    return;
  }

  // table slice of this wave, in log2 units: Tb[j] = bias[h][j + tb0] * log2(e) for key k and query q at j = k + (q0 + 31 - q), i.e.
  // j = 0 .. len + 30; entries outside the table (queries that do not exist) are zero and never used
  const int tb0 = L - 1 - (q0 + 31);
  {
    const float* bt = a.bias + (size_t)h * (2 * L - 1);
    const int nt = len + 31;
    for (int j = lane; j < nt; j += 64) {
      const int t = j + tb0;
      Tb[j] = (t >= 0 && t < 2 * L - 1) ? bt[t] * 1.4426950408889634f : 0.f;
    }
  }

  chunk16 qf[NQT][NKB];                                       // B operand of S^T: query lr, d = 32 kb + 8 lq .. +7
#pragma unroll
  for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      const int qi = q0 + qt * 16 + lr;
      qf[qt][kb] = *reinterpret_cast<const chunk16*>(qg + (size_t)(qi < len ? qi : len - 1) * a.ld_qkv + kb * 32 + lq * 8);
    }
  f32x4 O[NQT][NDT];                                          // O^T: rows d = 16 dt + 4 lq + r, column = query lr
  float m[NQT], l[NQT];
#pragma unroll
  for (int qt = 0; qt < NQT; ++qt) {
    m[qt] = -INFINITY; l[qt] = 0.f;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) O[qt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float sc2 = a.scale * 1.4426950408889634f;            // scores in log2 units

  chunk16 ks[NCH], vs[NCH];
  auto fetch = [&](int k0) {                                  // keys >= len: zeros, and no load (a masked key has P = 0, and 0 x garbage must not be a NaN)
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
      const int idx = u * 64 + lane, r = idx / CPR, c = idx - r * CPR;
      ks[u] = chunk16{0u, 0u, 0u, 0u}; vs[u] = ks[u];
      if (k0 + r < len) {
        ks[u] = *reinterpret_cast<const chunk16*>(kg + (size_t)(k0 + r) * a.ld_qkv + c * 8);
        vs[u] = *reinterpret_cast<const chunk16*>(vg + (size_t)(k0 + r) * a.ld_qkv + c * 8);
      }
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
      const int idx = u * 64 + lane, r = idx / CPR, c = idx - r * CPR;
      *reinterpret_cast<chunk16*>(Kl + r * PITCH + c * 8) = ks[u];
      *reinterpret_cast<chunk16*>(Vl + r * PITCH + c * 8) = vs[u];
    }
  };
  // the strips and the table slice are private to this wave and LDS executes a wave's operations in issue order: a wave-level barrier
  // between the writes of a block and its reads (and back) is all the synchronisation there is
  auto wave_sync = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  typedef __attribute__((address_space(3))) s16x4* lds_s16x4;
  const int nblk = (len + KB - 1) / KB;
  // one key block; RAGGED: it holds keys past len (only the last block of a sample whose length is not a multiple of KB)
  auto run_block = [&](int ib, auto raggedc) {
    constexpr bool ragged = decltype(raggedc)::value;
    const int k0 = ib * KB;
    if (ib + 1 < nblk) fetch(k0 + KB);                        // lands under this block's MFMAs
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
      if (qt >= nqt) break;
      f32x4 Sc[NKT];
      float mx = m[qt];                                       // running max of the biased scores, log2 units
      // table index of (key k0 + kt*16 + lq*4 + r, query q0 + qt*16 + lr): k + 31 - (q - q0); in range for every lane (j <= k0 + KB + 30
      // <= L + 61 < TBL), entries of keys >= len are never written and never used (ragged mask) — their slots hold what LDS held, finite or not
      const float* tp = Tb + k0 + lq * 4 + 31 - (qt * 16 + lr);
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
          const chunk16 kf = *reinterpret_cast<const chunk16*>(Kl + (kt * 16 + lr) * PITCH + kb * 32 + lq * 8);
          acc = Mma<T>::run(kf, qf[qt][kb], acc);             // rows = keys, column = query
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float s = __builtin_fmaf(acc[r], sc2, tp[kt * 16 + r]);
          if constexpr (ragged)
            if (k0 + kt * 16 + lq * 4 + r >= len) s = -INFINITY;   // keys past len never win the max nor add to the sum
          acc[r] = s;
          mx = fmaxf(mx, s);
        }
        Sc[kt] = acc;
      }
      mx = col4_max(mx);                                      // finite: key k0 exists in every block that runs
      const float corr = __builtin_amdgcn_exp2f(m[qt] - mx);  // exp2(-inf) = 0 on the first block
      m[qt] = mx;
      float ps = 0.f;
      s16x4 P[NKT];
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        float pv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { pv[r] = __builtin_amdgcn_exp2f(Sc[kt][r] - mx); ps += pv[r]; }
        typename Elem<T>::vec4 pk;
#pragma unroll
        for (int r = 0; r < 4; ++r) pk[r] = Elem<T>::from_f(pv[r]);
        P[kt] = __builtin_bit_cast(s16x4, pk);
      }
      l[qt] = l[qt] * corr + ps;                              // per-lane partial row sum: reduced once, behind the loop
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        f32x4 acc = O[qt][dt];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] *= corr;
#pragma unroll
        for (int kp = 0; kp < NKT / 2; ++kp) {
          // one 16x16x32 MFMA per PAIR of key tiles: lane group lq takes as its 8 k-slots the keys 4 lq .. +3 of tile 2 kp and of tile
          // 2 kp + 1 — the two packed P^T fragments it holds (B) against two transposed reads of the row-major V strip (A)
          s16x4 vf[2];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const T* vp = Vl + ((2 * kp + u) * 16 + lq * 4 + (lr >> 2)) * PITCH + dt * 16 + (lr & 3) * 4;
            vf[u] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(const_cast<T*>(vp)));
          }
          const s16x8 av = __builtin_shufflevector(vf[0], vf[1], 0, 1, 2, 3, 4, 5, 6, 7);
          const s16x8 bv = __builtin_shufflevector(P[2 * kp], P[2 * kp + 1], 0, 1, 2, 3, 4, 5, 6, 7);
          acc = Mma<T>::run(__builtin_bit_cast(chunk16, av), __builtin_bit_cast(chunk16, bv), acc);   // rows = d, column = query
        }
        O[qt][dt] = acc;
      }
    }
    if (ib + 1 < nblk) {
      wave_sync();                                            // this block's reads are issued before the strip is overwritten
      stash();
      wave_sync();
    }
  };
  fetch(0);
  stash();
  wave_sync();
  const int nfull = len / KB;
  for (int ib = 0; ib < nfull; ++ib) run_block(ib, std::false_type{});
  if (nfull < nblk) run_block(nfull, std::true_type{});
#pragma unroll
  for (int qt = 0; qt < NQT; ++qt) {
    const int qi = q0 + qt * 16 + lr;
    const float lsum = col4_sum(l[qt]);                       // (all lanes take part in the swaps: before the bounds test)
    if (qi >= L) continue;
    const bool real = qi < len;                               // a pad query (or a tile of pad queries, l = 0): a zero row
    const float inv = real ? 1.0f / lsum : 0.f;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      typename Elem<T>::vec4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = Elem<T>::from_f(real ? O[qt][dt][r] * inv : 0.f);
      *reinterpret_cast<typename Elem<T>::vec4*>(og + (size_t)qi * a.ld_out + dt * 16 + lq * 4) = o;
    }
  }
}

template <typename T, int D>
static int launch_bias_mfma(BiasAttnArgs a, hipStream_t s) {
  a.TBL = a.L + 64;
  const size_t lds = (size_t)4 * 2 * BA_KB * (D + 8) * sizeof(T) + (size_t)4 * a.TBL * sizeof(float);
  static bool done = false;
  if (!done) {      // the largest launch there is: L = DC_ATTENTION_BIAS_MAX_L
    const size_t lds_max = (size_t)4 * 2 * BA_KB * (D + 8) * sizeof(T) + (size_t)4 * (DC_ATTENTION_BIAS_MAX_L + 64) * sizeof(float);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_bias_kernel<T, D>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
    done = true;
  }
  const long long items = (long long)a.n * a.heads * ((a.L + 31) / 32);
  const long long nb = (items + 3) / 4;
  if (nb >= (1LL << 31)) { dc_set_error("dc_attention_bias: grid too large"); return DC_ERR_SHAPE; }
  hipLaunchKernelGGL((attn_bias_kernel<T, D>), dim3((unsigned)nb), dim3(256), lds, s, a);
  return dc_check_launch("dc_attention_bias(mfma)");
}

// ------------------------------------------------------------------------------------------------
// Exact fp32 kernel: K and V of one (sample, head) stream through LDS as f32 in blocks, each query is owned by d / 16 adjacent lanes
// holding a 16-wide slice of q and of the output, scores are reduced across those lanes with xor-shuffles, the softmax is online key
// by key — the order of operations does not depend on where a block ends.
template <typename T>
__global__ __launch_bounds__(256) void attn_bias_f32_kernel(const BiasAttnArgs a) {
  constexpr int SW = 16;
  extern __shared__ __attribute__((aligned(16))) float kv[];  // K[KB][d], V[KB][d]
  const int t = threadIdx.x;
  const int DS = a.d / SW;            // lanes per query (1,2,4,8): a power of two, the xor-shuffle ladder below needs one
  const int QT = 256 / DS;            // queries per workgroup
  const int qtiles = (a.L + QT - 1) / QT;
  int b = blockIdx.x;
  const int qt = b % qtiles; b /= qtiles;
  const int h = b % a.heads; const int i = b / a.heads;
  const int len = bias_len(a, i);                // uniform over the workgroup, as the barriers need
  float* Ks = kv; float* Vs = kv + a.KB * a.d;
  const T* kb = reinterpret_cast<const T*>(a.k) + (size_t)i * a.L * a.ld_qkv + h * a.d;
  const T* vb = reinterpret_cast<const T*>(a.v) + (size_t)i * a.L * a.ld_qkv + h * a.d;
  const int sl = t % DS;                         // my SW-wide slice of d
  const int qi = qt * QT + t / DS;               // my query
  const bool live = qi < len;                    // pad queries compute on row 0 (never stored) so that the shuffles stay whole
  float qv[SW], o[SW];
  const T* qp = reinterpret_cast<const T*>(a.q) + ((size_t)i * a.L + (live ? qi : 0)) * a.ld_qkv + h * a.d + sl * SW;
#pragma unroll
  for (int e = 0; e < SW; ++e) { qv[e] = Elem<T>::to_f(qp[e]) * a.scale; o[e] = 0.f; }
  const float* bt = a.bias + (size_t)h * (2 * a.L - 1) + (a.L - 1 - (live ? qi : 0));     // bt[k] = bias[h][k - q + L - 1]
  float m = -INFINITY, l = 0.f;
  if (qt * QT < len)                             // (uniform) a workgroup of pad queries reads nothing
    for (int j0 = 0; j0 < len; j0 += a.KB) {
      const int nk = min(a.KB, len - j0);
      if (j0) __syncthreads();                     // everyone is done with the previous block
      for (int e = t; e < nk * a.d; e += 256) {
        const int r = e / a.d, c = e - r * a.d;
        Ks[e] = Elem<T>::to_f(kb[(size_t)(j0 + r) * a.ld_qkv + c]);
        Vs[e] = Elem<T>::to_f(vb[(size_t)(j0 + r) * a.ld_qkv + c]);
      }
      __syncthreads();
      for (int j = 0; j < nk; ++j) {
        const float* kj = Ks + j * a.d + sl * SW;
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < SW; ++e) s += qv[e] * kj[e];
        for (int off = 1; off < DS; off <<= 1) s += __shfl_xor(s, off, 64);
        s += bt[j0 + j];
        const float mn = fmaxf(m, s);
        const float corr = expf(m - mn);
        const float p = expf(s - mn);
        l = l * corr + p;
        const float* vj = Vs + j * a.d + sl * SW;
#pragma unroll
        for (int e = 0; e < SW; ++e) o[e] = o[e] * corr + p * vj[e];
        m = mn;
      }
    }
  if (qi < a.L) {
    const float inv = live ? 1.0f / l : 0.f;
    T* op = reinterpret_cast<T*>(a.out) + ((size_t)i * a.L + qi) * a.ld_out + h * a.d + sl * SW;
#pragma unroll
    for (int e = 0; e < SW; ++e) op[e] = Elem<T>::from_f(live ? o[e] * inv : 0.f);
  }
}

static int bias_validate(const dc_attention_bias_params* p) {
  DC_REQUIRE(p && p->q && p->k && p->v && p->out && p->bias, DC_ERR_ARG, "dc_attention_bias: null pointer");
  DC_REQUIRE(p->dtype == DC_F32 || p->dtype == DC_BF16 || p->dtype == DC_F16, DC_ERR_DTYPE, "dc_attention_bias: dtype %d", p->dtype);
  DC_REQUIRE(p->d == 16 || p->d == 32 || p->d == 64 || p->d == 128, DC_ERR_SHAPE, "dc_attention_bias: head dim %d (16/32/64/128)", p->d);
  DC_REQUIRE(p->n > 0 && p->heads > 0, DC_ERR_SHAPE, "dc_attention_bias: n/heads");
  DC_REQUIRE(p->L >= 1 && p->L <= DC_ATTENTION_BIAS_MAX_L, DC_ERR_SHAPE, "dc_attention_bias: L=%d (1 .. %d)", p->L, DC_ATTENTION_BIAS_MAX_L);
  DC_REQUIRE(p->ld_qkv >= p->heads * p->d && p->ld_out >= p->heads * p->d, DC_ERR_SHAPE, "dc_attention_bias: ld");
  DC_REQUIRE((((uintptr_t)p->bias | (uintptr_t)p->kv_len) & 3) == 0, DC_ERR_ALIGN, "dc_attention_bias: bias / kv_len must be 4-byte aligned");
  const uintptr_t es = (uintptr_t)dc_dtype_size(p->dtype) - 1;
  DC_REQUIRE((((uintptr_t)p->q | (uintptr_t)p->k | (uintptr_t)p->v | (uintptr_t)p->out) & es) == 0, DC_ERR_ALIGN, "dc_attention_bias: q/k/v/out must be element aligned");
  // the matrix-core kernel folds the scale into an FMA in log2 units and the exact kernel into q; both are written for scale > 0
  DC_REQUIRE(p->scale > 0.f, DC_ERR_ARG, "dc_attention_bias: scale must be positive (got %g)", (double)p->scale);
  return DC_OK;
}

// matrix cores: 16-bit, d = 64, 16-byte aligned q / k / v rows and 8-byte aligned output rows
static bool bias_mfma_ok(const dc_attention_bias_params* p) {
  if (p->dtype == DC_F32 || p->d != 64) return false;
  if ((((uintptr_t)p->q | (uintptr_t)p->k | (uintptr_t)p->v) & 15) || (p->ld_qkv % 8)) return false;
  return p->ld_out % 4 == 0 && (((uintptr_t)p->out) & 7) == 0;
}

extern "C" const char* dc_attention_bias_variant(const dc_attention_bias_params* p) {
  if (bias_validate(p) != DC_OK) return "invalid";
  return bias_mfma_ok(p) ? "mfma" : "fp32";
}

extern "C" int dc_attention_bias(const dc_attention_bias_params* p, dc_stream stream) {
  const int rc = bias_validate(p);
  if (rc != DC_OK) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  BiasAttnArgs a{p->q, p->k, p->v, p->out, p->bias, p->kv_len, p->n, p->L, p->heads, p->d, p->ld_qkv, p->ld_out, p->scale, 0, 0};
  if (bias_mfma_ok(p))
    return dc_by_dtype16(p->dtype, "dc_attention_bias: dtype", [&](auto t) { return launch_bias_mfma<decltype(t), 64>(a, s); });
  a.KB = p->L < 4096 / p->d ? p->L : 4096 / p->d;                // at most 32 KiB of LDS
  const size_t lds = (size_t)2 * a.KB * p->d * sizeof(float);
  const int DS = p->d / 16, QT = 256 / DS, qtiles = (p->L + QT - 1) / QT;
  const long long nb = (long long)p->n * p->heads * qtiles;
  DC_REQUIRE(nb < (1LL << 31), DC_ERR_SHAPE, "dc_attention_bias: grid too large");
  return dc_by_dtype(p->dtype, "dc_attention_bias: dtype", [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(attn_bias_f32_kernel<T>, dim3((unsigned)nb), dim3(256), lds, s, a);
    return dc_check_launch("dc_attention_bias(fp32)");
  });
}

// ------------------------------------------------------------------------------------------------
// RMS norm: y = x * rsqrt(mean(x^2) + eps) * weight per row, one wave per row (4 rows per workgroup), fp32 statistics summed in a fixed
// order (per-lane strided partial sums, then the xor butterfly).  Rows at or past their sample's row_len are written as zeros and not read.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void rmsnorm_kernel(const dc_rmsnorm_params p) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.rows) return;
  const TI* x = reinterpret_cast<const TI*>(p.x) + (size_t)row * p.C;
  TO* y = reinterpret_cast<TO*>(p.y) + (size_t)row * p.C;
  if (p.row_len) {
    const int smp = (int)(row / p.rows_per_sample), r = (int)(row - (long long)smp * p.rows_per_sample);
    if (r >= p.row_len[smp]) {
      for (int c = lane; c < p.C; c += 64) y[c] = Elem<TO>::from_f(0.f);
      return;
    }
  }
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

// ------------------------------------------------------------------------------------------------
// out[r, :] = table[ids[r], :] in out_dtype; one workgroup per row.  An id outside [0, vocab) is clamped (the host validates ids where
// they enter; the kernel only makes sure that nothing outside the table is read).
template <typename TO>
__global__ __launch_bounds__(256) void embed_rows_kernel(const dc_embed_rows_params p) {
  const int r = blockIdx.x;
  long long id = p.ids[r];
  id = id < 0 ? 0 : (id >= p.vocab ? p.vocab - 1 : id);
  const float* src = p.table + (size_t)id * p.C;
  TO* dst = reinterpret_cast<TO*>(p.out) + (size_t)r * p.C;
  for (int c = threadIdx.x; c < p.C; c += 256) dst[c] = Elem<TO>::from_f(src[c]);
}

extern "C" int dc_embed_rows(const dc_embed_rows_params* p, dc_stream stream) {
  DC_REQUIRE(p && p->table && p->ids && p->out, DC_ERR_ARG, "dc_embed_rows: null pointer");
  DC_REQUIRE((unsigned)p->out_dtype <= DC_F16, DC_ERR_DTYPE, "dc_embed_rows: out_dtype %d", p->out_dtype);
  DC_REQUIRE(p->rows > 0 && p->C > 0 && p->vocab > 0, DC_ERR_SHAPE, "dc_embed_rows: rows=%d C=%d vocab=%d", p->rows, p->C, p->vocab);
  DC_REQUIRE((((uintptr_t)p->table) & 3) == 0 && (((uintptr_t)p->ids) & 7) == 0 && (((uintptr_t)p->out) & (dc_dtype_size(p->out_dtype) - 1)) == 0,
             DC_ERR_ALIGN, "dc_embed_rows: pointers must be element aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return dc_by_dtype(p->out_dtype, "dc_embed_rows: out_dtype", [&](auto to) {
    hipLaunchKernelGGL((embed_rows_kernel<decltype(to)>), dim3((unsigned)p->rows), dim3(256), 0, s, *p);
    return dc_check_launch("dc_embed_rows");
  });
}

// ------------------------------------------------------------------------------------------------
// x = max(x, 0) in place, a 16-byte chunk per thread and step; NaN stays NaN (as torch.relu).  The last n % (16 / size) elements go one by one.
template <typename T>
__global__ __launch_bounds__(256) void relu_kernel(T* x, long long n) {
  constexpr int EPC = Elem<T>::EPC;
  const long long nch = n / EPC;
  const long long stride = (long long)gridDim.x * 256;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < nch; c += stride) {
    typename Elem<T>::vec v = *reinterpret_cast<const typename Elem<T>::vec*>(x + c * EPC);
#pragma unroll
    for (int e = 0; e < EPC; ++e) { const float f = Elem<T>::to_f(v[e]); v[e] = f < 0.f ? Elem<T>::from_f(0.f) : v[e]; }
    *reinterpret_cast<typename Elem<T>::vec*>(x + c * EPC) = v;
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n - nch * EPC)) {
    T* t = x + nch * EPC + threadIdx.x;
    if (Elem<T>::to_f(*t) < 0.f) *t = Elem<T>::from_f(0.f);
  }
}

extern "C" int dc_relu(const dc_relu_params* p, dc_stream stream) {
  DC_REQUIRE(p && p->x, DC_ERR_ARG, "dc_relu: null pointer");
  DC_REQUIRE((unsigned)p->dtype <= DC_F16, DC_ERR_DTYPE, "dc_relu: dtype %d", p->dtype);
  DC_REQUIRE(p->n > 0, DC_ERR_SHAPE, "dc_relu: n=%lld", (long long)p->n);
  DC_REQUIRE((((uintptr_t)p->x) & 15) == 0, DC_ERR_ALIGN, "dc_relu: x must be 16-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long long nch = p->n / (16 / dc_dtype_size(p->dtype));
  long long nb = (nch + 255) / 256;
  nb = nb < 1 ? 1 : (nb > 4096 ? 4096 : nb);
  return dc_by_dtype(p->dtype, "dc_relu: dtype", [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(relu_kernel<T>, dim3((unsigned)nb), dim3(256), 0, s, reinterpret_cast<T*>(p->x), (long long)p->n);
    return dc_check_launch("dc_relu");
  });
}
