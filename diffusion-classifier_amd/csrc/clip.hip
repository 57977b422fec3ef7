// clip.hip — the kernels a CLIP text transformer needs besides dc_igemm: causal self-attention with a row count per sample
// (dc_attention_causal), a LayerNorm with weight and bias that reads one type and writes another (dc_layernorm_rows), the token +
// position embedding (dc_embed_rows_pos) and the feed-forward's activation as a pass of its own (dc_act_pass: quick-GELU or erf-GELU).
//
// dc_attention_causal, 16-bit with d = 64 and 16-byte aligned rows ("mfma"): attn_bias_kernel<T,64> of t5.hip without the table and with
// the causal structure instead — one WAVE per (sample, head, 32 queries), four per workgroup, wave-private K / V strips in LDS, no
// workgroup barrier; S^T = K Q^T on the 16x16x32 MFMA so that a lane holds 4 consecutive KEYS of ONE query, online fp32 softmax in log2
// units with the scale folded into the exponent's FMA, the packed P^T fragments fed straight back as the MFMA operand, V read with
// ds_read_b64_tr_b16, the next key block fetched under the current block's MFMAs.  What is new:
//   * a wave whose queries start at q0 (a multiple of 32) walks the key blocks 0 .. q0 / 32 only: blocks above the diagonal are neither
//     fetched nor multiplied;
//   * only the diagonal block (keys q0 .. q0 + 31) applies the per-element mask k > q, BEFORE the running max, so a masked score never
//     enters it.  Every query keeps key 0 of block 0 and key q0 <= q of the diagonal block: no row of a block is ever fully masked, the
//     running max is finite after every block, and a masked position carries P = exp2(-inf - finite) = 0 exactly;
//   * the sample's length row_len[i] (clamped into [1, L]) bounds the queries; the causal mask already hides every key >= the length
//     from every query below it, so the length needs no key mask of its own.  Rows >= the length of q / k / v are never read (keys of
//     the diagonal block past the length are staged as zeros: a pad query of a live tile meets 0 x 0, never 0 x garbage), tiles of pad
//     queries store zeros and leave, pad rows inside a live tile are written as zeros.
// Fixed summation order, no atomics: the bits of a row depend on rows 0 .. q of its own sample only.
//
// fp32, d = 16 / 32 / 128 and unaligned operands ("fp32"): the exact kernel of t5.hip without the table (K / V of one (sample, head)
// stream through LDS as f32, FMA chain over the keys in order, online softmax key by key); a query stops at its own key.
//
// dc_act_pass exists for the reason dc_relu does: dc_igemm, its dispatcher and the shared epilogue stay as they are.
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>
#include "igemm_common.h"
#include "attn_lanes.h"

struct CausalAttnArgs {
  const void* q; const void* k; const void* v; void* out;
  const int32_t* row_len;
  int n, L, heads, d, ld_qkv, ld_out; float scale;
  int KB;     // fp32 kernel: keys per LDS block
};

// rows of sample i that exist: device data, clamped rather than trusted; uniform -> the scalar path
__device__ __forceinline__ int causal_len(const CausalAttnArgs& a, int i) {
  return a.row_len ? __builtin_amdgcn_readfirstlane(min(max(a.row_len[i], 1), a.L)) : a.L;
}

typedef __attribute__((ext_vector_type(4))) short cs16x4;
typedef __attribute__((ext_vector_type(8))) short cs16x8;

static constexpr int CA_KB = 32;    // keys per block = queries per wave: block q0 / 32 is the diagonal one

template <typename T, int D>
__global__ __launch_bounds__(256) void attn_causal_kernel(const CausalAttnArgs a) {
  constexpr int KB = CA_KB;
  constexpr int NKT = KB / 16, NQT = 2, NDT = D / 16, NKB = D / 32;
  constexpr int PITCH = D + 8, CPR = D / 8;                   // LDS row pitch in elements (+16 B); 16-byte chunks per row
  constexpr int NCH = KB * CPR / 64;                          // staging chunks per lane and operand
  static_assert(KB * CPR % 64 == 0 && NKT % 2 == 0 && D % 32 == 0 && KB == 16 * NQT, "whole staging chunks, key tiles in pairs, square diagonal block");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane & 15, lq = lane >> 4;
  const int L = a.L;
  const int qtiles = (L + KB - 1) / KB;
  long long item = (long long)blockIdx.x * 4 + wave;
  if (item >= (long long)a.n * a.heads * qtiles) return;      // whole waves leave: nothing below is shared between waves
  const int qt_i = (int)(item % qtiles); item /= qtiles;
  const int h = (int)(item % a.heads), i = (int)(item / a.heads);
  T* const Kl = reinterpret_cast<T*>(smem) + (size_t)wave * 2 * KB * PITCH;
  T* const Vl = Kl + KB * PITCH;
  const T* qg = reinterpret_cast<const T*>(a.q) + (size_t)i * L * a.ld_qkv + h * D;
  const T* kg = reinterpret_cast<const T*>(a.k) + (size_t)i * L * a.ld_qkv + h * D;
  const T* vg = reinterpret_cast<const T*>(a.v) + (size_t)i * L * a.ld_qkv + h * D;
  T* const og = reinterpret_cast<T*>(a.out) + (size_t)i * L * a.ld_out + h * D;
  const int len = causal_len(a, i);                           // rows of this sample (L without row_len); the samples stay L rows apart
  const int q0 = qt_i * KB;
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
  auto fetch = [&](int k0) {                                  // keys >= len (diagonal block only): zeros, and no load
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
  // the strips are private to this wave and LDS executes a wave's operations in issue order: a wave-level barrier between the writes
  // of a block and its reads (and back) is all the synchronisation there is
  auto wave_sync = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  typedef __attribute__((address_space(3))) cs16x4* lds_s16x4;
  const int nblk = qt_i + 1;                                  // blocks 0 .. q0 / 32: nothing above the diagonal
  // one key block; DIAG: the block of the wave's own queries, the only one with masked positions
  auto run_block = [&](int ib, auto diagc) {
    constexpr bool diag = decltype(diagc)::value;
    const int k0 = ib * KB;
    if (!diag) fetch(k0 + KB);                                // lands under this block's MFMAs
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
      if (qt >= nqt) break;
      f32x4 Sc[NKT];
      float mx = m[qt];                                       // running max of the visible RAW scores (scale > 0: the same arg max)
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
          float s = acc[r];
          if constexpr (diag)
            if (kt * 16 + lq * 4 + r > qt * 16 + lr) s = -INFINITY;   // key > query (both relative to q0): masked before the max
          acc[r] = s;
          mx = fmaxf(mx, s);
        }
        Sc[kt] = acc;
      }
      mx = col4_max(mx);                                      // finite: key k0 <= q is visible to every query of the wave in every block
      const float corr = __builtin_amdgcn_exp2f((m[qt] - mx) * sc2);   // exp2(-inf) = 0 on the first block
      m[qt] = mx;
      const float nm = -mx * sc2;
      float ps = 0.f;
      cs16x4 P[NKT];
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        float pv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { pv[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(Sc[kt][r], sc2, nm)); ps += pv[r]; }   // masked: exp2(-inf) = 0 exactly
        typename Elem<T>::vec4 pk;
#pragma unroll
        for (int r = 0; r < 4; ++r) pk[r] = Elem<T>::from_f(pv[r]);
        P[kt] = __builtin_bit_cast(cs16x4, pk);
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
          cs16x4 vf[2];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const T* vp = Vl + ((2 * kp + u) * 16 + lq * 4 + (lr >> 2)) * PITCH + dt * 16 + (lr & 3) * 4;
            vf[u] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(const_cast<T*>(vp)));
          }
          const cs16x8 av = __builtin_shufflevector(vf[0], vf[1], 0, 1, 2, 3, 4, 5, 6, 7);
          const cs16x8 bv = __builtin_shufflevector(P[2 * kp], P[2 * kp + 1], 0, 1, 2, 3, 4, 5, 6, 7);
          acc = Mma<T>::run(__builtin_bit_cast(chunk16, av), __builtin_bit_cast(chunk16, bv), acc);   // rows = d, column = query
        }
        O[qt][dt] = acc;
      }
    }
    if (!diag) {
      wave_sync();                                            // this block's reads are issued before the strip is overwritten
      stash();
      wave_sync();
    }
  };
  fetch(0);
  stash();
  wave_sync();
  for (int ib = 0; ib + 1 < nblk; ++ib) run_block(ib, std::false_type{});
  run_block(nblk - 1, std::true_type{});
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
static int launch_causal_mfma(CausalAttnArgs a, hipStream_t s) {
  const size_t lds = (size_t)4 * 2 * CA_KB * (D + 8) * sizeof(T);      // 36 KiB at d = 64
  const long long items = (long long)a.n * a.heads * ((a.L + CA_KB - 1) / CA_KB);
  const long long nb = (items + 3) / 4;
  if (nb >= (1LL << 31)) { dc_set_error("dc_attention_causal: grid too large"); return DC_ERR_SHAPE; }
  hipLaunchKernelGGL((attn_causal_kernel<T, D>), dim3((unsigned)nb), dim3(256), lds, s, a);
  return dc_check_launch("dc_attention_causal(mfma)");
}

// ------------------------------------------------------------------------------------------------
// Exact fp32 kernel: K and V of one (sample, head) stream through LDS as f32 in blocks, each query is owned by d / 16 adjacent lanes
// holding a 16-wide slice of q and of the output, scores are reduced across those lanes with xor-shuffles, the softmax is online key
// by key — the order of operations does not depend on where a block ends.  A query takes the keys 0 .. q; the workgroup streams the keys
// up to its last query.
template <typename T>
__global__ __launch_bounds__(256) void attn_causal_f32_kernel(const CausalAttnArgs a) {
  constexpr int SW = 16;
  extern __shared__ __attribute__((aligned(16))) float kv[];  // K[KB][d], V[KB][d]
  const int t = threadIdx.x;
  const int DS = a.d / SW;            // lanes per query (1,2,4,8): a power of two, the xor-shuffle ladder below needs one
  const int QT = 256 / DS;            // queries per workgroup
  const int qtiles = (a.L + QT - 1) / QT;
  int b = blockIdx.x;
  const int qt = b % qtiles; b /= qtiles;
  const int h = b % a.heads; const int i = b / a.heads;
  const int len = causal_len(a, i);              // uniform over the workgroup, as the barriers need
  float* Ks = kv; float* Vs = kv + a.KB * a.d;
  const T* kb = reinterpret_cast<const T*>(a.k) + (size_t)i * a.L * a.ld_qkv + h * a.d;
  const T* vb = reinterpret_cast<const T*>(a.v) + (size_t)i * a.L * a.ld_qkv + h * a.d;
  const int sl = t % DS;                         // my SW-wide slice of d
  const int qi = qt * QT + t / DS;               // my query
  const bool live = qi < len;                    // pad queries compute on row 0 (never stored) so that the shuffles stay whole
  const int qe = live ? qi : 0;                  // the last key my query sees
  float qv[SW], o[SW];
  const T* qp = reinterpret_cast<const T*>(a.q) + ((size_t)i * a.L + qe) * a.ld_qkv + h * a.d + sl * SW;
#pragma unroll
  for (int e = 0; e < SW; ++e) { qv[e] = Elem<T>::to_f(qp[e]) * a.scale; o[e] = 0.f; }
  float m = -INFINITY, l = 0.f;
  const int kend = min(len, qt * QT + QT);       // (uniform) keys this workgroup's queries can see; <= 0 rows for a workgroup of pad queries
  if (qt * QT < len)
    for (int j0 = 0; j0 < kend; j0 += a.KB) {
      const int nk = min(a.KB, kend - j0);
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
        for (int off = 1; off < DS; off <<= 1) s += __shfl_xor(s, off, 64);   // every lane takes part; the lanes of a query agree below
        if (j0 + j <= qe) {
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
    }
  if (qi < a.L) {
    const float inv = live ? 1.0f / l : 0.f;
    T* op = reinterpret_cast<T*>(a.out) + ((size_t)i * a.L + qi) * a.ld_out + h * a.d + sl * SW;
#pragma unroll
    for (int e = 0; e < SW; ++e) op[e] = Elem<T>::from_f(live ? o[e] * inv : 0.f);
  }
}

static int causal_validate(const dc_attention_causal_params* p) {
  DC_REQUIRE(p && p->q && p->k && p->v && p->out, DC_ERR_ARG, "dc_attention_causal: null pointer");
  DC_REQUIRE(p->dtype == DC_F32 || p->dtype == DC_BF16 || p->dtype == DC_F16, DC_ERR_DTYPE, "dc_attention_causal: dtype %d", p->dtype);
  DC_REQUIRE(p->d == 16 || p->d == 32 || p->d == 64 || p->d == 128, DC_ERR_SHAPE, "dc_attention_causal: head dim %d (16/32/64/128)", p->d);
  DC_REQUIRE(p->n > 0 && p->heads > 0, DC_ERR_SHAPE, "dc_attention_causal: n/heads");
  DC_REQUIRE(p->L >= 1 && p->L <= DC_ATTENTION_CAUSAL_MAX_L, DC_ERR_SHAPE, "dc_attention_causal: L=%d (1 .. %d)", p->L, DC_ATTENTION_CAUSAL_MAX_L);
  DC_REQUIRE(p->ld_qkv >= p->heads * p->d && p->ld_out >= p->heads * p->d, DC_ERR_SHAPE, "dc_attention_causal: ld");
  DC_REQUIRE((((uintptr_t)p->row_len) & 3) == 0, DC_ERR_ALIGN, "dc_attention_causal: row_len must be 4-byte aligned");
  const uintptr_t es = (uintptr_t)dc_dtype_size(p->dtype) - 1;
  DC_REQUIRE((((uintptr_t)p->q | (uintptr_t)p->k | (uintptr_t)p->v | (uintptr_t)p->out) & es) == 0, DC_ERR_ALIGN, "dc_attention_causal: q/k/v/out must be element aligned");
  // the matrix-core kernel folds the scale into the exponent in log2 units and the exact kernel into q; both are written for scale > 0
  DC_REQUIRE(p->scale > 0.f, DC_ERR_ARG, "dc_attention_causal: scale must be positive (got %g)", (double)p->scale);
  return DC_OK;
}

// matrix cores: 16-bit, d = 64, 16-byte aligned q / k / v rows and 8-byte aligned output rows
static bool causal_mfma_ok(const dc_attention_causal_params* p) {
  if (p->dtype == DC_F32 || p->d != 64) return false;
  if ((((uintptr_t)p->q | (uintptr_t)p->k | (uintptr_t)p->v) & 15) || (p->ld_qkv % 8)) return false;
  return p->ld_out % 4 == 0 && (((uintptr_t)p->out) & 7) == 0;
}

extern "C" const char* dc_attention_causal_variant(const dc_attention_causal_params* p) {
  if (causal_validate(p) != DC_OK) return "invalid";
  return causal_mfma_ok(p) ? "mfma" : "fp32";
}

extern "C" int dc_attention_causal(const dc_attention_causal_params* p, dc_stream stream) {
  const int rc = causal_validate(p);
  if (rc != DC_OK) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  CausalAttnArgs a{p->q, p->k, p->v, p->out, p->row_len, p->n, p->L, p->heads, p->d, p->ld_qkv, p->ld_out, p->scale, 0};
  if (causal_mfma_ok(p))
    return dc_by_dtype16(p->dtype, "dc_attention_causal: dtype", [&](auto t) { return launch_causal_mfma<decltype(t), 64>(a, s); });
  a.KB = p->L < 4096 / p->d ? p->L : 4096 / p->d;                // at most 32 KiB of LDS
  const size_t lds = (size_t)2 * a.KB * p->d * sizeof(float);
  const int DS = p->d / 16, QT = 256 / DS, qtiles = (p->L + QT - 1) / QT;
  const long long nb = (long long)p->n * p->heads * qtiles;
  DC_REQUIRE(nb < (1LL << 31), DC_ERR_SHAPE, "dc_attention_causal: grid too large");
  return dc_by_dtype(p->dtype, "dc_attention_causal: dtype", [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(attn_causal_f32_kernel<T>, dim3((unsigned)nb), dim3(256), lds, s, a);
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

// ------------------------------------------------------------------------------------------------
// out[r, :] = table[ids[r], :] + pos[r % L, :] in out_dtype (one fp32 add, one rounding); one workgroup per row.  An id outside
// [0, vocab) is clamped (the host validates ids where they enter; the kernel only makes sure that nothing outside the table is read).
template <typename TO>
__global__ __launch_bounds__(256) void embed_rows_pos_kernel(const dc_embed_rows_pos_params p) {
  const int r = blockIdx.x;
  long long id = p.ids[r];
  id = id < 0 ? 0 : (id >= p.vocab ? p.vocab - 1 : id);
  const float* src = p.table + (size_t)id * p.C;
  const float* ps = p.pos + (size_t)(r % p.L) * p.C;
  TO* dst = reinterpret_cast<TO*>(p.out) + (size_t)r * p.C;
  for (int c = threadIdx.x; c < p.C; c += 256) dst[c] = Elem<TO>::from_f(src[c] + ps[c]);
}

extern "C" int dc_embed_rows_pos(const dc_embed_rows_pos_params* p, dc_stream stream) {
  DC_REQUIRE(p && p->table && p->pos && p->ids && p->out, DC_ERR_ARG, "dc_embed_rows_pos: null pointer");
  DC_REQUIRE((unsigned)p->out_dtype <= DC_F16, DC_ERR_DTYPE, "dc_embed_rows_pos: out_dtype %d", p->out_dtype);
  DC_REQUIRE(p->rows > 0 && p->C > 0 && p->vocab > 0 && p->L > 0, DC_ERR_SHAPE, "dc_embed_rows_pos: rows=%d C=%d vocab=%d L=%d", p->rows, p->C, p->vocab, p->L);
  DC_REQUIRE((((uintptr_t)p->table | (uintptr_t)p->pos) & 3) == 0 && (((uintptr_t)p->ids) & 7) == 0 &&
             (((uintptr_t)p->out) & (dc_dtype_size(p->out_dtype) - 1)) == 0, DC_ERR_ALIGN, "dc_embed_rows_pos: pointers must be element aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return dc_by_dtype(p->out_dtype, "dc_embed_rows_pos: out_dtype", [&](auto to) {
    hipLaunchKernelGGL((embed_rows_pos_kernel<decltype(to)>), dim3((unsigned)p->rows), dim3(256), 0, s, *p);
    return dc_check_launch("dc_embed_rows_pos");
  });
}

// ------------------------------------------------------------------------------------------------
// x = act(x) in place, a 16-byte chunk per thread and step, evaluated in fp32 and rounded once to the storage type; NaN stays NaN.
//   quick-GELU  x * sigmoid(1.702 x)              (OpenAI CLIP)
//   erf-GELU    x * Phi(x) = 0.5 x erfc(-x / sqrt 2)   (OpenCLIP): erfc keeps the relative accuracy of the negative tail, where
//               1 + erf(x / sqrt 2) cancels to zero in fp32
// The last n % (16 / size) elements go one by one.
template <int KIND> __device__ __forceinline__ float act_pass_f(float x) {
  if constexpr (KIND == DC_PASS_QUICK_GELU) return x * (1.0f / (1.0f + expf(-1.702f * x)));
  else return 0.5f * x * erfcf(-0.70710678118654752f * x);
}

template <typename T, int KIND>
__global__ __launch_bounds__(256) void act_pass_kernel(T* x, long long n) {
  constexpr int EPC = Elem<T>::EPC;
  const long long nch = n / EPC;
  const long long stride = (long long)gridDim.x * 256;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < nch; c += stride) {
    typename Elem<T>::vec v = *reinterpret_cast<const typename Elem<T>::vec*>(x + c * EPC);
#pragma unroll
    for (int e = 0; e < EPC; ++e) v[e] = Elem<T>::from_f(act_pass_f<KIND>(Elem<T>::to_f(v[e])));
    *reinterpret_cast<typename Elem<T>::vec*>(x + c * EPC) = v;
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n - nch * EPC)) {
    T* t = x + nch * EPC + threadIdx.x;
    *t = Elem<T>::from_f(act_pass_f<KIND>(Elem<T>::to_f(*t)));
  }
}

extern "C" int dc_act_pass(const dc_act_pass_params* p, dc_stream stream) {
  DC_REQUIRE(p && p->x, DC_ERR_ARG, "dc_act_pass: null pointer");
  DC_REQUIRE((unsigned)p->dtype <= DC_F16, DC_ERR_DTYPE, "dc_act_pass: dtype %d", p->dtype);
  DC_REQUIRE(p->kind == DC_PASS_QUICK_GELU || p->kind == DC_PASS_GELU_ERF, DC_ERR_ARG, "dc_act_pass: kind %d", p->kind);
  DC_REQUIRE(p->n > 0, DC_ERR_SHAPE, "dc_act_pass: n=%lld", (long long)p->n);
  DC_REQUIRE((((uintptr_t)p->x) & 15) == 0, DC_ERR_ALIGN, "dc_act_pass: x must be 16-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long long nch = p->n / (16 / dc_dtype_size(p->dtype));
  long long nb = (nch + 255) / 256;
  nb = nb < 1 ? 1 : (nb > 4096 ? 4096 : nb);
  return dc_by_dtype(p->dtype, "dc_act_pass: dtype", [&](auto t) {
    using T = decltype(t);
    if (p->kind == DC_PASS_QUICK_GELU) hipLaunchKernelGGL((act_pass_kernel<T, DC_PASS_QUICK_GELU>), dim3((unsigned)nb), dim3(256), 0, s, reinterpret_cast<T*>(p->x), (long long)p->n);
    else hipLaunchKernelGGL((act_pass_kernel<T, DC_PASS_GELU_ERF>), dim3((unsigned)nb), dim3(256), 0, s, reinterpret_cast<T*>(p->x), (long long)p->n);
    return dc_check_launch("dc_act_pass");
  });
}
