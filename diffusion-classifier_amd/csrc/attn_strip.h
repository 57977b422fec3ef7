// attn_strip.h — the two attention bodies that attention_cross.hip (cross-attention), t5.hip (relative-position bias, a length per
// sample) and clip.hip (causal, a length per sample) share; attention.hip (self-attention) runs the exact body and builds its two
// transposed-score kernels from the same three pieces as attn_strip_run (attn_score_tile, attn_exp_pack, attn_pv_step);
// attention_wide.hip (heads of 256 / 512 channels) does the same with a query tile spread over four waves.  Each of
// those files keeps thin __global__ kernels that decode their item, fill a StripView and a Mode, and call a body; what differs between
// them lives in the Mode alone:
//   kZeroPad              queries at or past the length exist as rows: written as zeros, and a whole tile of them reads nothing
//   kBiased               the score is fma(q k^T, scale, bias(key, query)) and the max runs over it; otherwise the max runs over the raw
//                         q k^T and the scale is folded into the exponent's FMA (valid for scale > 0 only)
//   masked<LAST>(k, q)    whether the score of (key, query) is masked; LAST: the one block behind the plain ones (the last of the walk)
//   prologue(lane), bias(k, q)   kBiased only: fill the wave's table slice; look an entry up
//
// attn_strip_run, 16-bit ("mfma"): one WAVE per (sample, head, 32 queries), four per workgroup, nothing shared between waves and
// therefore no workgroup barrier:
//   S^T = K Q^T     16x16x32 MFMA, A = K rows from a row-major wave-private LDS strip, B = Q fragments held in registers; a lane gets
//                   4 consecutive KEYS of ONE query
//   softmax         fp32 in log2 units, online over key blocks of KB keys
//   O^T += V^T P^T  the two packed P^T fragments a lane holds are its B operand, A is two ds_read_b64_tr_b16 of the row-major V strip
// The K / V block of the next step is fetched into registers under the MFMAs of the current one.  Keys at or past the view's key bound
// are staged as zeros and never read (a masked key has P = 0, and 0 x garbage must not be a NaN).  Fixed order, no atomics.
//
// attn_exact_run, any type ("fp32"): K and V of one (sample, head) stream through LDS as f32 in blocks, each query is owned by d / SW
// adjacent lanes holding an SW-wide slice of q and of the output, scores are reduced across those lanes with xor-shuffles, the softmax
// is online key by key — the order of operations does not depend on where a block ends.
#pragma once
#include <stdio.h>
#include <type_traits>
#include "igemm_common.h"
#include "attn_lanes.h"

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4;

// ------------------------------------------------------------------------------------------------
// The three pieces of every transposed-score kernel (attn_strip_run below; attn_flash_t_kernel and attn_wave_kernel of attention.hip).
// lr = lane & 15, lq = lane >> 4; K / V images are row-major with a pitch of PITCH = D + 8 elements.

// one S^T tile: keys 16 kt .. +15 (rows) x the 16 queries of qf (column lr); qf: query lr, d = 32 kb + 8 lq .. +7
template <typename T, int NKB, int PITCH>
__device__ __forceinline__ f32x4 attn_score_tile(const T* Kb, int kt, const chunk16 (&qf)[NKB], int lr, int lq) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    const chunk16 kf = *reinterpret_cast<const chunk16*>(Kb + (kt * 16 + lr) * PITCH + kb * 32 + lq * 8);
    acc = Mma<T>::run(kf, qf[kb], acc);                       // rows = keys, column = query
  }
  return acc;
}

// p2 (the caller's score -> probability) of each score, four packed to the compute type per tile; returns the lane's partial row sum
// (of the unrounded p)
template <typename T, int NKT, typename F>
__device__ __forceinline__ float attn_exp_pack(const f32x4 (&S)[NKT], s16x4 (&P)[NKT], F&& p2) {
  float ps = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    float pv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { pv[r] = p2(S[kt][r]); ps += pv[r]; }
    typename Elem<T>::vec4 pk;
#pragma unroll
    for (int r = 0; r < 4; ++r) pk[r] = Elem<T>::from_f(pv[r]);
    P[kt] = __builtin_bit_cast(s16x4, pk);
  }
  return ps;
}

// acc += V^T P^T for d rows 16 dt .. +15 over all NKT key tiles of the V image
template <typename T, int NKT, int PITCH>
__device__ __forceinline__ f32x4 attn_pv_step(f32x4 acc, const T* Vb, int dt, const s16x4 (&P)[NKT], int lr, int lq) {
#pragma unroll
  for (int kp = 0; kp < NKT / 2; ++kp) {
    // one 16x16x32 MFMA per PAIR of key tiles: the sum over k is order-free as long as both operands agree, so lane group lq takes
    // as its 8 k-slots the keys 4 lq .. +3 of tile 2 kp and of tile 2 kp + 1 — exactly the two packed P^T D-fragments it already
    // holds (B operand), and two transposed reads of the row-major V image (A operand): for each, the 16-lane group takes keys
    // 16 kt + 4 lq .. +3 x d columns 16 dt .. +15; lane 4q+p supplies the address of key row q, columns 4p .. 4p+3 and receives
    // column lr of the four rows
    s16x4 vf[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const T* vp = Vb + ((2 * kp + u) * 16 + lq * 4 + (lr >> 2)) * PITCH + dt * 16 + (lr & 3) * 4;
      vf[u] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(const_cast<T*>(vp)));
    }
    const s16x8 av = __builtin_shufflevector(vf[0], vf[1], 0, 1, 2, 3, 4, 5, 6, 7);
    const s16x8 bv = __builtin_shufflevector(P[2 * kp], P[2 * kp + 1], 0, 1, 2, 3, 4, 5, 6, 7);
    acc = Mma<T>::run(__builtin_bit_cast(chunk16, av), __builtin_bit_cast(chunk16, bv), acc);   // rows = d, column = query
  }
  return acc;
}

// what a body sees of one (sample, head): row 0 of its q / k / v / out, and the bounds of its walk
template <typename T> struct StripView {
  const T* q; const T* k; const T* v; T* out;
  int ld_q, ld_kv, ld_out;
  int q0;        // first query of this wave (strip) / workgroup (exact)
  int q_rows;    // stored query rows: output rows below it are written
  int nq;        // real queries (= q_rows without kZeroPad)
  int nk;        // keys below it are staged, the others are zeros and never read
  int nblk;      // strip: key blocks walked ...
  int nplain;    // ... of which the first nplain hold no masked position (nplain = nblk, or nblk - 1)
};

// masks nothing but the keys at or past a length, which only the last block can hold
struct KeyBound {
  int len;
  template <bool LAST> __device__ __forceinline__ bool masked(int key, int) const { return LAST && key >= len; }
};

// every stored query is real and the scores are raw; the keys stop at a bound (cross-attention: the context's length, which only the
// ragged last block can cross; self-attention's exact kernel: L)
struct PlainMode : KeyBound { static constexpr bool kZeroPad = false, kBiased = false; };

// an entry of a device array of lengths: clamped rather than trusted; uniform -> the scalar path
__device__ __forceinline__ int clamped_len(const int32_t* len, int i, int rows) {
  return __builtin_amdgcn_readfirstlane(min(max(len[i], 1), rows));
}

// dynamic LDS of a workgroup: per wave a K and a V strip of KB rows of D + 8 elements (a mode's table slices come behind all of them)
template <typename T, int D, int KB> constexpr size_t strip_lds_bytes() { return (size_t)4 * 2 * KB * (D + 8) * sizeof(T); }
template <typename T, int D, int KB> __device__ __forceinline__ void strip_lds(char* smem, int wave, T*& Kl, T*& Vl) {
  Kl = reinterpret_cast<T*>(smem) + (size_t)wave * 2 * KB * (D + 8);
  Vl = Kl + KB * (D + 8);
}

// the wave's item: sample i, head h, first query q0 of its 32; false: past the last item (whole waves leave)
__device__ __forceinline__ bool strip_item(int n, int heads, int q_rows, int& wave, int& i, int& h, int& q0) {
  wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int qtiles = (q_rows + 31) / 32;
  long long item = (long long)blockIdx.x * 4 + wave;
  if (item >= (long long)n * heads * qtiles) return false;
  q0 = (int)(item % qtiles) * 32; item /= qtiles;
  h = (int)(item % heads); i = (int)(item / heads);
  return true;
}

// Kl / Vl: the wave's strips (strip_lds)
template <typename T, int D, int KB, typename Mode>
__device__ __forceinline__ void attn_strip_run(const StripView<T>& w, Mode& mode, float scale, T* Kl, T* Vl) {
  constexpr int NKT = KB / 16, NQT = 2, NDT = D / 16, NKB = D / 32;
  constexpr int PITCH = D + 8, CPR = D / 8;                   // LDS row pitch in elements (+16 B); 16-byte chunks per row
  constexpr int NCH = KB * CPR / 64;                          // staging chunks per lane and operand
  static_assert(KB * CPR % 64 == 0 && NKT % 2 == 0 && D % 32 == 0, "whole staging chunks, key tiles in pairs, 32-wide k-chunks");
  const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
  const int nqt = min(NQT, (w.nq - w.q0 + 15) >> 4);          // 16-query tiles of this wave that hold a query (wave-uniform)
  auto put = [&](int qi, int dt, f32x4 o4) {                  // 4 consecutive d of one output row
    typename Elem<T>::vec4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = Elem<T>::from_f(o4[r]);
    *reinterpret_cast<typename Elem<T>::vec4*>(w.out + (size_t)qi * w.ld_out + dt * 16 + lq * 4) = o;
  };
  if constexpr (Mode::kZeroPad)
    if (nqt <= 0) {                                           // every query of this wave is padding: zero rows, nothing read
#pragma unroll
      for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
          if (w.q0 + qt * 16 + lr < w.q_rows) put(w.q0 + qt * 16 + lr, dt, f32x4{0.f, 0.f, 0.f, 0.f});
      return;
    }
  if constexpr (Mode::kBiased) mode.prologue(lane);

  chunk16 qf[NQT][NKB];                                       // B operand of S^T: query lr, d = 32 kb + 8 lq .. +7
#pragma unroll
  for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      const int qi = w.q0 + qt * 16 + lr;
      qf[qt][kb] = *reinterpret_cast<const chunk16*>(w.q + (size_t)(qi < w.nq ? qi : w.nq - 1) * w.ld_q + kb * 32 + lq * 8);
    }
  f32x4 O[NQT][NDT];                                          // O^T: rows d = 16 dt + 4 lq + r, column = query lr
  float m[NQT], l[NQT];
#pragma unroll
  for (int qt = 0; qt < NQT; ++qt) {
    m[qt] = -INFINITY; l[qt] = 0.f;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) O[qt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float sc2 = scale * 1.4426950408889634f;              // scores in log2 units

  chunk16 ks[NCH], vs[NCH];
  auto fetch = [&](int k0) {                                  // keys >= nk: zeros, and no load
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
      const int idx = u * 64 + lane, r = idx / CPR, c = idx - r * CPR;
      ks[u] = chunk16{0u, 0u, 0u, 0u}; vs[u] = ks[u];
      if (k0 + r < w.nk) {
        ks[u] = *reinterpret_cast<const chunk16*>(w.k + (size_t)(k0 + r) * w.ld_kv + c * 8);
        vs[u] = *reinterpret_cast<const chunk16*>(w.v + (size_t)(k0 + r) * w.ld_kv + c * 8);
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
  // the strips (and a Mode's table slice) are private to this wave and LDS executes a wave's operations in issue order: a wave-level
  // barrier between the writes of a block and its reads (and back) is all the synchronisation there is
  auto wave_sync = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  auto run_block = [&](int ib, auto lastc) {
    constexpr bool LAST = decltype(lastc)::value;
    const int k0 = ib * KB;
    const bool more = !LAST && ib + 1 < w.nblk;
    if (more) fetch(k0 + KB);                                 // lands under this block's MFMAs
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
      if (qt >= nqt) break;
      f32x4 Sc[NKT];
      float mx = m[qt];                                       // running max: of the biased scores, or of the raw ones (scale > 0: same arg max)
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        f32x4 acc = attn_score_tile<T, NKB, PITCH>(Kl, kt, qf[qt], lr, lq);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = k0 + kt * 16 + lq * 4 + r, query = w.q0 + qt * 16 + lr;
          float s = acc[r];
          if constexpr (Mode::kBiased) s = __builtin_fmaf(s, sc2, mode.bias(key, query));
          if (mode.template masked<LAST>(key, query)) s = -INFINITY;    // before the max: a masked score never wins it nor adds to the sum
          acc[r] = s;
          mx = fmaxf(mx, s);
        }
        Sc[kt] = acc;
      }
      mx = col4_max(mx);                                      // finite: every block that runs shows every query of the wave a key
      const float nms = -mx * sc2;
      auto p2 = [&](float s) {                                // exp2 of a score below the new max, in log2 units; exp2(-inf) = 0 exactly
        if constexpr (Mode::kBiased) return __builtin_amdgcn_exp2f(s - mx);
        else return __builtin_amdgcn_exp2f(__builtin_fmaf(s, sc2, nms));
      };
      const float corr = p2(m[qt]);                           // 0 on the first block
      m[qt] = mx;
      s16x4 P[NKT];
      const float ps = attn_exp_pack<T>(Sc, P, p2);
      l[qt] = l[qt] * corr + ps;                              // per-lane partial row sum: reduced once, behind the loop
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        f32x4 acc = O[qt][dt];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] *= corr;
        O[qt][dt] = attn_pv_step<T, NKT, PITCH>(acc, Vl, dt, P, lr, lq);
      }
    }
    if (more) {
      wave_sync();                                            // this block's reads are issued before the strip is overwritten
      stash();
      wave_sync();
    }
  };
  fetch(0);
  stash();
  wave_sync();
  for (int ib = 0; ib < w.nplain; ++ib) run_block(ib, std::false_type{});
  if (w.nplain < w.nblk) run_block(w.nplain, std::true_type{});
#pragma unroll
  for (int qt = 0; qt < NQT; ++qt) {
    if (!Mode::kZeroPad && qt >= nqt) break;
    const int qi = w.q0 + qt * 16 + lr;
    const float lsum = col4_sum(l[qt]);                       // (all lanes take part in the swaps: before the bounds test)
    if (qi >= w.q_rows) continue;
    const bool real = !Mode::kZeroPad || qi < w.nq;           // a pad query: a zero row
    const float inv = real ? 1.0f / lsum : 0.f;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      f32x4 o4;
#pragma unroll
      for (int r = 0; r < 4; ++r) o4[r] = real ? O[qt][dt][r] * inv : 0.f;
      put(qi, dt, o4);
    }
  }
}

// items (one per wave) -> workgroups of 4 waves, and the launch
template <typename K, typename A>
static int strip_launch(K kern, const A& a, long long items, size_t lds, hipStream_t s, const char* fn, const char* what) {
  const long long nb = (items + 3) / 4;
  if (nb >= (1LL << 31)) { dc_set_error("%s: grid too large", fn); return DC_ERR_SHAPE; }
  hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(256), lds, s, a);
  return dc_check_launch(what);
}

// matrix-core route of every caller: 16-bit, 16-byte aligned q / k / v rows and 8-byte aligned output rows (the head dims are the caller's)
static inline bool strip_route_ok(int dtype, const void* q, const void* k, const void* v, const void* out, int ld_q, int ld_kv, int ld_out) {
  if (dtype == DC_F32) return false;
  if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) || (ld_q % 8) || (ld_kv % 8)) return false;
  return ld_out % 4 == 0 && (((uintptr_t)out) & 7) == 0;
}

// ------------------------------------------------------------------------------------------------
// the exact body: a workgroup of 256 lanes takes QT = 256 / (d / SW) queries of one (sample, head); Ks: 2 * KB * d floats of LDS
__device__ __forceinline__ void exact_item(int heads, int q_rows, int QT, int& i, int& h, int& q0) {
  const int qtiles = (q_rows + QT - 1) / QT;
  int b = blockIdx.x;
  q0 = b % qtiles * QT; b /= qtiles;
  h = b % heads; i = b / heads;
}

template <typename T, int SW, typename Mode>
__device__ __forceinline__ void attn_exact_run(const StripView<T>& w, const Mode& mode, float scale, int d, int KB, float* Ks) {
  const int t = threadIdx.x;
  const int DS = d / SW;              // lanes per query (1,2,4,8): a power of two, the xor-shuffle ladder below needs one
  float* Vs = Ks + KB * d;
  const int sl = t % DS;              // my SW-wide slice of d
  const int qi = w.q0 + t / DS;       // my query
  const bool live = qi < w.nq;        // the others compute on row 0 (never stored) so that the shuffles stay whole
  const int qe = live ? qi : 0;
  float qv[SW], o[SW];
  const T* qp = w.q + (size_t)qe * w.ld_q + sl * SW;
#pragma unroll
  for (int e = 0; e < SW; ++e) { qv[e] = Elem<T>::to_f(qp[e]) * scale; o[e] = 0.f; }
  float m = -INFINITY, l = 0.f;
  if (!Mode::kZeroPad || w.q0 < w.nq)            // (uniform) a workgroup of pad queries reads nothing
    for (int j0 = 0; j0 < w.nk; j0 += KB) {
      const int nk = min(KB, w.nk - j0);
      if (j0) __syncthreads();                   // everyone is done with the previous block
      for (int e = t; e < nk * d; e += 256) {
        const int r = e / d, c = e - r * d;
        Ks[e] = Elem<T>::to_f(w.k[(size_t)(j0 + r) * w.ld_kv + c]);
        Vs[e] = Elem<T>::to_f(w.v[(size_t)(j0 + r) * w.ld_kv + c]);
      }
      __syncthreads();
      for (int j = 0; j < nk; ++j) {
        const float* kj = Ks + j * d + sl * SW;
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < SW; ++e) s += qv[e] * kj[e];
        for (int off = 1; off < DS; off <<= 1) s += __shfl_xor(s, off, 64);   // every lane takes part; the lanes of a query agree below
        if constexpr (Mode::kBiased) s += mode.bias(j0 + j, qe);
        if (mode.template masked<true>(j0 + j, qe)) continue;
        const float mn = fmaxf(m, s);
        const float corr = expf(m - mn);
        const float p = expf(s - mn);
        l = l * corr + p;
        const float* vj = Vs + j * d + sl * SW;
#pragma unroll
        for (int e = 0; e < SW; ++e) o[e] = o[e] * corr + p * vj[e];
        m = mn;
      }
    }
  if (qi < w.q_rows) {
    const bool real = !Mode::kZeroPad || live;
    const float inv = real ? 1.0f / l : 0.f;
    T* op = w.out + (size_t)qi * w.ld_out + sl * SW;
#pragma unroll
    for (int e = 0; e < SW; ++e) op[e] = Elem<T>::from_f(real ? o[e] * inv : 0.f);
  }
}

// launch arithmetic of the exact kernels: keys per LDS block (at most 32 KiB), dynamic LDS, queries per workgroup, grid
struct ExactPlan { int KB; size_t lds; unsigned nb; };
static inline int exact_plan(int n, int heads, int q_rows, int keys, int d, int SW, const char* fn, ExactPlan& e) {
  e.KB = keys < 4096 / d ? keys : 4096 / d;
  e.lds = (size_t)2 * e.KB * d * sizeof(float);
  const int QT = 256 / (d / SW);
  const long long nb = (long long)n * heads * ((q_rows + QT - 1) / QT);
  DC_REQUIRE(nb < (1LL << 31), DC_ERR_SHAPE, "%s: grid too large", fn);
  e.nb = (unsigned)nb;
  return DC_OK;
}

// ------------------------------------------------------------------------------------------------
// Self-attention over q / k / v / out [n, L, heads, d] with one ld_qkv and a row count per sample (dc_attention_bias, dc_attention_causal)
struct SeqAttnArgs {
  const void* q; const void* k; const void* v; void* out;
  const int32_t* len;      // rows per sample (null: L everywhere), clamped into [1, L] by the kernel; the samples stay L rows apart
  int n, L, heads, d, ld_qkv, ld_out; float scale;
  int KB;     // fp32 kernel: keys per LDS block
};

// sample i, head h (of width d): rows at or past the length are pad queries and keys that are not read; nblk / nplain are left to the caller
template <typename T>
__device__ __forceinline__ StripView<T> seq_view(const SeqAttnArgs& a, int i, int h, int d, int q0) {
  const int len = a.len ? clamped_len(a.len, i, a.L) : a.L;
  const size_t in0 = (size_t)i * a.L * a.ld_qkv + h * d;
  return {reinterpret_cast<const T*>(a.q) + in0, reinterpret_cast<const T*>(a.k) + in0, reinterpret_cast<const T*>(a.v) + in0,
          reinterpret_cast<T*>(a.out) + (size_t)i * a.L * a.ld_out + h * d, a.ld_qkv, a.ld_qkv, a.ld_out, q0, a.L, len, len, 0, 0};
}

// `fn`: the entry point's name in front of every message; aux: the function's int32 / fp32 device arrays or-ed together, aux_name: what
// the message calls them; aux_ok: those of them that must not be null are not
template <typename P>
static int seq_attn_validate(const P* p, const char* fn, int max_L, bool aux_ok, uintptr_t aux, const char* aux_name) {
  DC_REQUIRE(p && p->q && p->k && p->v && p->out && aux_ok, DC_ERR_ARG, "%s: null pointer", fn);
  DC_REQUIRE(p->dtype == DC_F32 || p->dtype == DC_BF16 || p->dtype == DC_F16, DC_ERR_DTYPE, "%s: dtype %d", fn, p->dtype);
  DC_REQUIRE(p->d == 16 || p->d == 32 || p->d == 64 || p->d == 128, DC_ERR_SHAPE, "%s: head dim %d (16/32/64/128)", fn, p->d);
  DC_REQUIRE(p->n > 0 && p->heads > 0, DC_ERR_SHAPE, "%s: n/heads", fn);
  DC_REQUIRE(p->L >= 1 && p->L <= max_L, DC_ERR_SHAPE, "%s: L=%d (1 .. %d)", fn, p->L, max_L);
  DC_REQUIRE(p->ld_qkv >= p->heads * p->d && p->ld_out >= p->heads * p->d, DC_ERR_SHAPE, "%s: ld", fn);
  DC_REQUIRE((aux & 3) == 0, DC_ERR_ALIGN, "%s: %s must be 4-byte aligned", fn, aux_name);
  const uintptr_t es = (uintptr_t)dc_dtype_size(p->dtype) - 1;
  DC_REQUIRE((((uintptr_t)p->q | (uintptr_t)p->k | (uintptr_t)p->v | (uintptr_t)p->out) & es) == 0, DC_ERR_ALIGN, "%s: q/k/v/out must be element aligned", fn);
  // the matrix-core kernel folds the scale into an FMA in log2 units and the exact kernel into q; both are written for scale > 0
  DC_REQUIRE(p->scale > 0.f, DC_ERR_ARG, "%s: scale must be positive (got %g)", fn, (double)p->scale);
  return DC_OK;
}

// matrix cores: d = 64 on the strip route (d = 32 / 128 would come from the same template; nothing needs them, they take the exact kernel)
template <typename P> static bool seq_attn_mfma_ok(const P* p) {
  return p->d == 64 && strip_route_ok(p->dtype, p->q, p->k, p->v, p->out, p->ld_qkv, p->ld_qkv, p->ld_out);
}

// validated parameters -> a launch: mfma(t) on the strip route, else exact(t, plan) after a.KB is set; t: a value of the element type
template <typename P, typename FM, typename FE>
static int seq_attn_dispatch(const P* p, SeqAttnArgs& a, const char* fn, FM&& mfma, FE&& exact) {
  char what[48];
  snprintf(what, sizeof(what), "%s: dtype", fn);
  if (seq_attn_mfma_ok(p)) return dc_by_dtype16(p->dtype, what, mfma);
  ExactPlan e;
  const int rc = exact_plan(p->n, p->heads, p->L, p->L, p->d, 16, fn, e);
  if (rc != DC_OK) return rc;
  a.KB = e.KB;
  return dc_by_dtype(p->dtype, what, [&](auto t) { return exact(t, e); });
}
