// attention_cross.hip — cross-attention: softmax(q k^T * scale) v where keys and values come from ANOTHER tensor (the prompt side
// path) with its own length S, picked per output sample through kv_map (ctx_of_unit), and queries are read through q_map
// (bj_of_unit: the class-shared trunk keeps q once per (image, trial) pair).
//
// Replaces F.scaled_dot_product_attention inside diffusers' Attention (attn2 of BasicTransformerBlock) for a context of several
// tokens; the one-token context needs no kernel (softmax over one key is 1: the class vector of the attn1.to_out epilogue).
//
// 16-bit, d = 32 / 64 / 96 / 128: the transposed-score structure of attn_flash_t_kernel (attention_mfma.hip), one WAVE per
// (output sample, head, 32 queries) with nothing shared between waves and therefore no workgroup barrier:
//   S^T = K Q^T     16x16x32 MFMA, A = K rows from a row-major wave-private LDS strip, B = Q fragments held in registers; a lane gets
//                   4 consecutive KEYS of ONE query
//   softmax         fp32 on the raw scores, the scale folded into the exponent's FMA, online over key blocks of 32 (d >= 64) or 64 keys
//   O^T += V^T P^T  the two packed P^T fragments a lane holds are its B operand, A is two ds_read_b64_tr_b16 of the row-major V strip
// K / V of a launch are small (n_ctx * S rows) and stay in L2: the stream that costs is q in and out back, so the unit of work is a
// query tile and the K / V block of the next step is fetched into registers under the MFMAs of the current one.  The last block is
// ragged: keys >= S are staged as zeros and masked, never read (behind them lies the next context, or a gap).
// A sample's bits depend on its own q rows and its own context only: no atomics, fixed order, no dependence on n or on the position.
// LEN instantiations (dc_cross_attention_len): context c holds kv_len[c] <= S keys in its S rows; the length, uniform over the wave (over
// the workgroup in the fp32 kernel), replaces S in the block count, the prefetch condition, the staging bound and the ragged mask, so
// blocks wholly past it cost nothing and the surviving keys keep their blocks: the bits are those of a context of kv_len[c] rows.
//
// fp32 and d = 16: the exact kernel (FMA chain over the keys in order), as attention.hip's.
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>
#include "igemm_common.h"
#include "attn_lanes.h"

struct CrossArgs {
  const void* q; const void* k; const void* v; void* out;
  const int32_t* q_map; const int32_t* kv_map;
  int n, Lq, S, heads, d, ld_q, ld_kv, ld_out; float scale;
  int KB;     // fp32 kernel: keys per LDS block
  const int32_t* kv_len;   // LEN instantiations only: keys per context, clamped into [1, S] by the kernel
};

// keys of context cs that are attended (LEN): device data, so a bad value is clamped rather than trusted; uniform -> the scalar path
template <bool LEN>
__device__ __forceinline__ int cross_len(const CrossArgs& a, int cs) {
  if constexpr (LEN) return __builtin_amdgcn_readfirstlane(min(max(a.kv_len[cs], 1), a.S));
  else return a.S;
}

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

// keys per block: 8 staging chunks per lane and operand at most, and an LDS strip small enough for 2 - 4 workgroups per CU
static constexpr int cross_kb(int D) { return D <= 32 ? 64 : 32; }

template <typename T, int D, bool LEN>
__global__ __launch_bounds__(256) void attn_cross_kernel(const CrossArgs a) {
  constexpr int KB = cross_kb(D);
  constexpr int NKT = KB / 16, NQT = 2, NDT = D / 16, NKB = D / 32;
  constexpr int PITCH = D + 8, CPR = D / 8;                   // LDS row pitch in elements (+16 B); 16-byte chunks per row
  constexpr int NCH = KB * CPR / 64;                          // staging chunks per lane and operand
  static_assert(KB * CPR % 64 == 0 && NKT % 2 == 0 && D % 32 == 0, "whole staging chunks, key tiles in pairs, 32-wide k-chunks");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane & 15, lq = lane >> 4;
  const int Lq = a.Lq, S = a.S;
  const int qtiles = (Lq + 16 * NQT - 1) / (16 * NQT);
  long long item = (long long)blockIdx.x * 4 + wave;
  if (item >= (long long)a.n * a.heads * qtiles) return;      // whole waves leave: nothing below is shared between waves
  const int qt_i = (int)(item % qtiles); item /= qtiles;
  const int h = (int)(item % a.heads), i = (int)(item / a.heads);
  const int qs = a.q_map ? a.q_map[i] : i, cs = a.kv_map ? a.kv_map[i] : i;
  T* const Kl = reinterpret_cast<T*>(smem) + (size_t)wave * 2 * KB * PITCH;
  T* const Vl = Kl + KB * PITCH;
  const T* qg = reinterpret_cast<const T*>(a.q) + (size_t)qs * Lq * a.ld_q + h * D;
  const T* kg = reinterpret_cast<const T*>(a.k) + (size_t)cs * S * a.ld_kv + h * D;
  const T* vg = reinterpret_cast<const T*>(a.v) + (size_t)cs * S * a.ld_kv + h * D;
  const int len = cross_len<LEN>(a, cs);                      // keys of this context (S without LEN); the rows stay S apart
  const int q0 = qt_i * 16 * NQT;
  const int nqt = min(NQT, (Lq - q0 + 15) >> 4);              // 16-query tiles of this wave that hold a query (wave-uniform)

  chunk16 qf[NQT][NKB];                                       // B operand of S^T: query lr, d = 32 kb + 8 lq .. +7
#pragma unroll
  for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      const int qi = q0 + qt * 16 + lr;
      qf[qt][kb] = *reinterpret_cast<const chunk16*>(qg + (size_t)(qi < Lq ? qi : Lq - 1) * a.ld_q + kb * 32 + lq * 8);
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
        ks[u] = *reinterpret_cast<const chunk16*>(kg + (size_t)(k0 + r) * a.ld_kv + c * 8);
        vs[u] = *reinterpret_cast<const chunk16*>(vg + (size_t)(k0 + r) * a.ld_kv + c * 8);
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
  // the strip is private to this wave and LDS executes a wave's operations in issue order: a wave-level barrier between the writes
  // of a block and its reads (and back) is all the synchronisation there is
  auto wave_sync = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  typedef __attribute__((address_space(3))) s16x4* lds_s16x4;
  const int nblk = (len + KB - 1) / KB;
  // one key block; RAGGED: it holds keys past len (only the last block of a context whose length is not a multiple of KB)
  auto run_block = [&](int ib, auto raggedc) {
    constexpr bool ragged = decltype(raggedc)::value;
    const int k0 = ib * KB;
    if (ib + 1 < nblk) fetch(k0 + KB);                        // lands under this block's MFMAs
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
      if (qt >= nqt) break;
      f32x4 Sc[NKT];
      float mx = m[qt];                                       // running max of the raw scores (the scale is positive: same arg max)
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
          const chunk16 kf = *reinterpret_cast<const chunk16*>(Kl + (kt * 16 + lr) * PITCH + kb * 32 + lq * 8);
          acc = Mma<T>::run(kf, qf[qt][kb], acc);             // rows = keys, column = query
        }
        if constexpr (ragged) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (k0 + kt * 16 + lq * 4 + r >= len) acc[r] = -INFINITY;   // keys past len never win the max nor add to the sum
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, acc[r]);
        Sc[kt] = acc;
      }
      mx = col4_max(mx);
      const float nms = -mx * sc2;
      const float corr = __builtin_amdgcn_exp2f(__builtin_fmaf(m[qt], sc2, nms));    // exp2(-inf) = 0 on the first block
      m[qt] = mx;
      float ps = 0.f;
      s16x4 P[NKT];
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        float pv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { pv[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(Sc[kt][r], sc2, nms)); ps += pv[r]; }
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
    if (qt >= nqt) break;
    const int qi = q0 + qt * 16 + lr;
    const float inv = 1.0f / col4_sum(l[qt]);                 // (all lanes take part in the swaps: before the bounds test)
    if (qi >= Lq) continue;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      typename Elem<T>::vec4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = Elem<T>::from_f(O[qt][dt][r] * inv);
      *reinterpret_cast<typename Elem<T>::vec4*>(reinterpret_cast<T*>(a.out) + ((size_t)i * Lq + qi) * a.ld_out + h * D + dt * 16 + lq * 4) = o;
    }
  }
}

template <typename T, int D, bool LEN>
static int launch_cross(const CrossArgs& a, hipStream_t s, const char* fn) {
  constexpr size_t lds = (size_t)4 * 2 * cross_kb(D) * (D + 8) * 2;
  static bool done = false;
  if (!done) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_cross_kernel<T, D, LEN>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); done = true; }
  const long long items = (long long)a.n * a.heads * ((a.Lq + 31) / 32);
  const long long nb = (items + 3) / 4;
  if (nb >= (1LL << 31)) { dc_set_error("%s: grid too large", fn); return DC_ERR_SHAPE; }
  hipLaunchKernelGGL((attn_cross_kernel<T, D, LEN>), dim3((unsigned)nb), dim3(256), lds, s, a);
  return dc_check_launch(LEN ? "dc_cross_attention_len(mfma)" : "dc_cross_attention(mfma)");
}

// ------------------------------------------------------------------------------------------------
// Exact fp32 kernel (f32, d = 16, and operands the matrix-core kernel's 16-byte loads cannot take): K and V of one (context, head) stream
// through LDS as f32 in blocks, each query is owned by d / SW adjacent lanes holding an SW-wide slice of q and of the output (SW = 16;
// 24 for d = 96), scores are reduced across those lanes with xor-shuffles, the softmax is online key by key — the order of operations
// does not depend on where a block ends.
template <typename T, int SW, bool LEN>
__global__ __launch_bounds__(256) void attn_cross_f32_kernel(const CrossArgs a) {
  extern __shared__ __attribute__((aligned(16))) float kv[];  // K[KB][d], V[KB][d]
  const int t = threadIdx.x;
  const int DS = a.d / SW;            // lanes per query (1,2,4,8): a power of two, the xor-shuffle ladder below needs one
  const int QT = 256 / DS;            // queries per workgroup
  const int qtiles = (a.Lq + QT - 1) / QT;
  int b = blockIdx.x;
  const int qt = b % qtiles; b /= qtiles;
  const int h = b % a.heads; const int i = b / a.heads;
  const int qs = a.q_map ? a.q_map[i] : i, cs = a.kv_map ? a.kv_map[i] : i;
  const int len = cross_len<LEN>(a, cs);         // keys of this context (S without LEN): uniform over the workgroup, as the barriers need
  float* Ks = kv; float* Vs = kv + a.KB * a.d;
  const T* kb = reinterpret_cast<const T*>(a.k) + (size_t)cs * a.S * a.ld_kv + h * a.d;
  const T* vb = reinterpret_cast<const T*>(a.v) + (size_t)cs * a.S * a.ld_kv + h * a.d;
  const int sl = t % DS;                         // my SW-wide slice of d
  const int qi = qt * QT + t / DS;               // my query
  const bool live = qi < a.Lq;
  float qv[SW], o[SW];
  const T* qp = reinterpret_cast<const T*>(a.q) + ((size_t)qs * a.Lq + (live ? qi : 0)) * a.ld_q + h * a.d + sl * SW;
#pragma unroll
  for (int e = 0; e < SW; ++e) { qv[e] = Elem<T>::to_f(qp[e]) * a.scale; o[e] = 0.f; }
  float m = -INFINITY, l = 0.f;
  for (int j0 = 0; j0 < len; j0 += a.KB) {
    const int nk = min(a.KB, len - j0);
    if (j0) __syncthreads();                     // everyone is done with the previous block
    for (int e = t; e < nk * a.d; e += 256) {
      const int r = e / a.d, c = e - r * a.d;
      Ks[e] = Elem<T>::to_f(kb[(size_t)(j0 + r) * a.ld_kv + c]);
      Vs[e] = Elem<T>::to_f(vb[(size_t)(j0 + r) * a.ld_kv + c]);
    }
    __syncthreads();
    for (int j = 0; j < nk; ++j) {
      const float* kj = Ks + j * a.d + sl * SW;
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < SW; ++e) s += qv[e] * kj[e];
      for (int off = 1; off < DS; off <<= 1) s += __shfl_xor(s, off, 64);
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
  if (live) {
    const float inv = 1.0f / l;
    T* op = reinterpret_cast<T*>(a.out) + ((size_t)i * a.Lq + qi) * a.ld_out + h * a.d + sl * SW;
#pragma unroll
    for (int e = 0; e < SW; ++e) op[e] = Elem<T>::from_f(o[e] * inv);
  }
}

// `fn`: the entry point's name in front of every message (dc_cross_attention / dc_cross_attention_len validate alike)
static int cross_validate(const dc_cross_attention_params* p, const char* fn) {
  DC_REQUIRE(p && p->q && p->k && p->v && p->out, DC_ERR_ARG, "%s: null pointer", fn);
  DC_REQUIRE(p->dtype == DC_F32 || p->dtype == DC_BF16 || p->dtype == DC_F16, DC_ERR_DTYPE, "%s: dtype %d", fn, p->dtype);
  DC_REQUIRE(p->d == 16 || p->d == 32 || p->d == 64 || p->d == 96 || p->d == 128, DC_ERR_SHAPE, "%s: head dim %d (16/32/64/96/128)", fn, p->d);
  DC_REQUIRE(p->n > 0 && p->Lq > 0 && p->heads > 0, DC_ERR_SHAPE, "%s: n/Lq/heads", fn);
  DC_REQUIRE(p->S >= 1, DC_ERR_SHAPE, "%s: S=%d (at least one key)", fn, p->S);
  DC_REQUIRE(p->ld_q >= p->heads * p->d && p->ld_kv >= p->heads * p->d && p->ld_out >= p->heads * p->d, DC_ERR_SHAPE, "%s: ld", fn);
  // the matrix-core kernel keeps the running max of the RAW scores and folds the scale into the exponent's FMA: valid for scale > 0 only
  DC_REQUIRE(p->scale > 0.f, DC_ERR_ARG, "%s: scale must be positive (got %g)", fn, (double)p->scale);
  return DC_OK;
}

// matrix cores: 16-bit, d = 32 / 64 / 96 / 128, 16-byte aligned q / k / v rows and 8-byte aligned output rows
static bool cross_mfma_ok(const dc_cross_attention_params* p) {
  if (p->dtype == DC_F32 || !(p->d == 32 || p->d == 64 || p->d == 96 || p->d == 128)) return false;
  if ((((uintptr_t)p->q | (uintptr_t)p->k | (uintptr_t)p->v) & 15) || (p->ld_q % 8) || (p->ld_kv % 8)) return false;
  return p->ld_out % 4 == 0 && (((uintptr_t)p->out) & 7) == 0;
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
      return launch_cross<T, 128, LEN>(a, s, fn);
    });
  a.KB = p->S < 4096 / p->d ? p->S : 4096 / p->d;                // at most 32 KiB of LDS
  const size_t lds = (size_t)2 * a.KB * p->d * sizeof(float);
  const int SW = p->d == 96 ? 24 : 16, DS = p->d / SW, QT = 256 / DS, qtiles = (p->Lq + QT - 1) / QT;
  const long long nb = (long long)p->n * p->heads * qtiles;
  DC_REQUIRE(nb < (1LL << 31), DC_ERR_SHAPE, "%s: grid too large", fn);
  return dc_by_dtype(p->dtype, what, [&](auto t) {
    using T = decltype(t);
    void (*kern)(const CrossArgs) = SW == 24 ? attn_cross_f32_kernel<T, 24, LEN> : attn_cross_f32_kernel<T, 16, LEN>;
    hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(256), lds, s, a);
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
  if (cross_validate(&b, "dc_cross_attention_len") != DC_OK) return "invalid";
  return cross_mfma_ok(&b) ? "mfma" : "fp32";
}

extern "C" int dc_cross_attention_len(const dc_cross_attention_len_params* p, dc_stream stream) {
  DC_REQUIRE(p, DC_ERR_ARG, "dc_cross_attention_len: null pointer");
  const dc_cross_attention_params b = cross_base(p);
  const int rc = cross_validate(&b, "dc_cross_attention_len");
  if (rc != DC_OK) return rc;
  // no lengths: every context has S keys, which is dc_cross_attention's launch
  if (!p->kv_len) return cross_launch<false>(&b, nullptr, stream, "dc_cross_attention_len");
  return cross_launch<true>(&b, p->kv_len, stream, "dc_cross_attention_len");
}
