// attention.hip — self-attention softmax(q k^T / sqrt(d)) v for the UNet and DiT token counts, gfx950.
//
// Replaces F.scaled_dot_product_attention in diffusers Attention (attn1 of BasicTransformerBlock) reached through reference
// nets/unet.py:186.  (Cross-attention over the single class token needs no kernel: softmax over one key is 1, see DESIGN.md.)
//
// Four kernels, chosen once per call by attn_plan (below, with the routing rules):
//   attn_wave_kernel     16-bit, L <= 64: one wave per (sample, head) pair, transposed scores
//   attn_mfma_kernel     16-bit, L <= 128: K and V^T of whole pairs in LDS, P through a per-wave LDS strip
//   attn_flash_t_kernel  16-bit, longer sequences: transposed scores, online softmax over double-buffered key blocks
//   attn_self_f32_kernel f32 (the parity path) and every shape the others do not take: attn_exact_run of attn_strip.h, exact in
//                        fp32 — K and V live in LDS as f32 (whole while they fit, else streamed in blocks), each query is owned by
//                        d / SW adjacent lanes (SW = 16; 24 for d = 96, so that the lane count stays a power of two: 4 lanes, not 6)
// The two transposed-score kernels are built from the pieces attn_strip_run is built from (attn_score_tile, attn_exp_pack,
// attn_pv_step); their work decompositions are their own.
#include <stdlib.h>
#include "attn_strip.h"

// ------------------------------------------------------------------------------------------------
// Whole sequence in LDS (L <= 128, L % 16 == 0, d % 32 == 0).  One 4-wave workgroup per group of G (sample, head) pairs: 1 pair when
// L >= 64, 2 when L == 32, 4 when L == 16, so every wave owns whole 16-query tiles.  K [L][d] and V^T [d][L] of a pair live in LDS (V is
// transposed while it is staged, so both MFMA operands are k-contiguous); Q fragments come straight from global memory.  Per 16-query tile:
//   S = Q K^T   (L/16 x d/32 MFMA 16x16x32, fp32 accumulate; lane holds 4 queries x 1 key per tile)
//   softmax over keys in fp32 registers (max/sum: across tiles, then xor-shuffles over the 16 lanes
//   that share a query), P -> 16-bit into a per-wave LDS strip in [query][key] order
//   O = P V     (d/16 x L/32 MFMA), scaled by 1/rowsum, stored as 16-bit, 2 bytes at a time.
struct AttnMArgs : SeqAttnArgs { int G, Lp; };                  // pairs per workgroup; L rounded up to a multiple of 32

template <typename T>
__global__ __launch_bounds__(256) void attn_mfma_kernel(const AttnMArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int lr = lane & 15, lq = lane >> 4;
  const int L = a.L, d = a.d, Lp = a.Lp, G = a.G;
  const int KS = d + 8, VS = Lp + 8, PS = Lp + 8;                // row strides in elements (+16 B pad)
  const int pair_bytes = (L * KS + d * VS) * 2;
  const int wpp = 4 / G;                                        // waves per pair
  const int g = wave / wpp, wl = wave - g * wpp;
  const long long pair = (long long)blockIdx.x * G + g;
  const long long npairs = (long long)a.n * a.heads;
  const bool pair_ok = pair < npairs;
  const int n = (int)((pair_ok ? pair : 0) / a.heads), h = (int)((pair_ok ? pair : 0) % a.heads);
  T* Ks = reinterpret_cast<T*>(smem + g * pair_bytes);
  T* Vt = Ks + L * KS;
  T* Pw = reinterpret_cast<T*>(smem + G * pair_bytes) + wave * 16 * PS;
  const T* qg = reinterpret_cast<const T*>(a.q) + (size_t)n * L * a.ld_qkv + h * d;
  const T* kg = reinterpret_cast<const T*>(a.k) + (size_t)n * L * a.ld_qkv + h * d;
  const T* vg = reinterpret_cast<const T*>(a.v) + (size_t)n * L * a.ld_qkv + h * d;

  // ---- stage K (row-major) and V^T into LDS, cooperatively by the waves of the pair ----
  const int tl = wl * 64 + lane, nth = wpp * 64;
  const int cpr = d / 8;                                        // 16-byte chunks per K/V row
  for (int idx = tl; idx < L * cpr; idx += nth) {
    const int r = idx / cpr, c = idx - r * cpr;
    const chunk16 kc = *reinterpret_cast<const chunk16*>(kg + (size_t)r * a.ld_qkv + c * 8);
    *reinterpret_cast<chunk16*>(Ks + r * KS + c * 8) = kc;
    const chunk16 vc = *reinterpret_cast<const chunk16*>(vg + (size_t)r * a.ld_qkv + c * 8);
    const typename Elem<T>::vec ve = __builtin_bit_cast(typename Elem<T>::vec, vc);
#pragma unroll
    for (int e = 0; e < 8; ++e) Vt[(c * 8 + e) * VS + r] = ve[e];
  }
  for (int idx = tl; idx < d * (Lp - L); idx += nth) {          // zero the padded keys (L == 16 -> Lp == 32)
    const int r = idx / (Lp - L), c = L + idx - r * (Lp - L);
    Vt[r * VS + c] = Elem<T>::from_f(0.f);
  }
  __syncthreads();
  if (!pair_ok) return;

  const int ktiles = L / 16, kblocks = d / 32;
  for (int qt = wl; qt < ktiles; qt += wpp) {
    const int q0 = qt * 16;
    chunk16 qf[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
      if (kb < kblocks) qf[kb] = *reinterpret_cast<const chunk16*>(qg + (size_t)(q0 + lr) * a.ld_qkv + kb * 32 + lq * 8);
    // S tiles: queries q0 + lq*4 + r, key kt*16 + lr
    f32x4 S[16];
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int kt = 0; kt < 16; ++kt) {
      if (kt < ktiles) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
          if (kb < kblocks) {
            const chunk16 kf = *reinterpret_cast<const chunk16*>(Ks + (kt * 16 + lr) * KS + kb * 32 + lq * 8);
            acc = Mma<T>::run(qf[kb], kf, acc);
          }
#pragma unroll
        for (int r = 0; r < 4; ++r) { acc[r] *= a.scale; m[r] = fmaxf(m[r], acc[r]); }
        S[kt] = acc;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) m[r] = fmaxf(m[r], __shfl_xor(m[r], o, 64));
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < 16; ++kt) {
      if (kt < ktiles) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = expf(S[kt][r] - m[r]);
          sum[r] += p;
          Pw[(lq * 4 + r) * PS + kt * 16 + lr] = Elem<T>::from_f(p);
        }
      }
    }
    if (Lp != L) {
#pragma unroll
      for (int r = 0; r < 4; ++r) Pw[(lq * 4 + r) * PS + L + lr] = Elem<T>::from_f(0.f);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) sum[r] += __shfl_xor(sum[r], o, 64);
    __builtin_amdgcn_wave_barrier();     // P strip is private to this wave: LDS executes its ops in issue order
    // O tiles: queries q0 + lq*4 + r, channel dt*16 + lr
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      if (dt * 16 < d) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int kb2 = 0; kb2 < Lp / 32; ++kb2) {
          const chunk16 pf = *reinterpret_cast<const chunk16*>(Pw + lr * PS + kb2 * 32 + lq * 8);
          const chunk16 vf = *reinterpret_cast<const chunk16*>(Vt + (dt * 16 + lr) * VS + kb2 * 32 + lq * 8);
          acc = Mma<T>::run(pf, vf, acc);
        }
        T* op = reinterpret_cast<T*>(a.out) + ((size_t)n * L + q0 + lq * 4) * a.ld_out + h * d + dt * 16 + lr;
#pragma unroll
        for (int r = 0; r < 4; ++r) op[(size_t)r * a.ld_out] = Elem<T>::from_f(acc[r] / sum[r]);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// (sample, head) pairs per workgroup.  L == 64 (8x8 tokens), d <= 64: four pairs, one wave each, instead of four waves on
// one pair — the four heads' 128-byte pieces of a qkv row are then fetched together (2.47 -> 2.67 TB/s on cfg2's blocks).
static int attn_pairs_per_wg(int L, int d) {
  if (L == 64 && d <= 64) return 4;
  return L >= 64 ? 1 : (L == 32 ? 2 : (L == 16 ? 4 : 0));
}

// ------------------------------------------------------------------------------------------------
// Long sequences (DiT: 1024 / 4096 tokens; 256 tokens of the CheXpert / IPMSA UNets).
// Flash forward, transposed-score form (head dims 32 / 64 / 96 / 128): no transposed V image, no LDS round trip for P.
//   S^T = K Q^T     16x16x32 MFMA, A = K rows straight from a row-major LDS image, B = Q fragments held in registers;
//                   the D fragment gives a lane 4 consecutive KEYS of ONE query (column lane&15)
//   softmax         per query = per lane column: running max / sum live in every lane of the column, the cross-lane part
//                   is two xor-shuffles (lanes 16 and 32 apart); exponentials as v_exp_f32 on log2-scaled scores
//   O^T += V^T P^T  16x16x32 MFMA over PAIRS of key tiles: the two packed P^T D-fragments a lane holds ARE its B operand
//                   (the k order inside an MFMA is free as long as A agrees), and the matching A operand (4 + 4
//                   consecutive keys of one d column) is two ds_read_b64_tr_b16 of the ROW-MAJOR V image
// K / V blocks of 128 / 64 / 64 / 32 keys (d = 32 / 64 / 96 / 128) are register-staged (global loads of block i+1 issued before the MFMAs of block i, written to
// the other LDS buffer after them), one barrier per block.  (The first version — transposed V staged with 2-byte LDS writes, P through
// LDS, no prefetch — ran DiT-B/4 attention at 0.2 PF and was removed in round 4.)

// (two workgroups per CU.  Three — launch bounds of 168 registers — were measured slower for D = 64: 10 spilled registers, 442 against
//  507 TFLOP/s on the DiT-B/4 shape, tools/bench_attention.py)
// Keys per block: sized so that scores + staged K/V fit the register file.  D = 96 takes 64, not 32 as D = 128 does: 32 rows of 12
// chunks are 1.5 staging chunks per thread; 64 rows are 3, and 2 x 2 buffers x 64 x 104 x 2 B = 52 KiB of LDS keep two workgroups per CU.
static constexpr int flash_kb(int D) { return D <= 32 ? 128 : (D <= 64 || D == 96 ? 64 : 32); }

template <typename T, int D>
__global__ __launch_bounds__(256, 2) void attn_flash_t_kernel(const SeqAttnArgs a) {
  constexpr int KB = flash_kb(D);
  constexpr int NKT = KB / 16, NQT = 2, NDT = D / 16, NKB = D / 32;
  constexpr int PITCH = D + 8;                                // LDS row pitch in elements (+16 B)
  constexpr int CPR = D / 8;                                  // 16-byte chunks per row
  constexpr int NST = KB * CPR / 256;                         // staging chunks per thread and operand
  static_assert(KB * CPR % 256 == 0 && NKT % 2 == 0 && D % 32 == 0, "whole staging chunks, key tiles in pairs, 32-wide k-chunks");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* const Kl = reinterpret_cast<T*>(smem);                   // [2][KB][PITCH]
  T* const Vl = Kl + 2 * KB * PITCH;                          // [2][KB][PITCH]
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int lr = lane & 15, lq = lane >> 4;
  const int L = a.L;
  const int qblocks = (L + 127) / 128;
  int b = blockIdx.x;
  const int qb = b % qblocks; b /= qblocks;
  const int h = b % a.heads, n = b / a.heads;
  const T* qg = reinterpret_cast<const T*>(a.q) + (size_t)n * L * a.ld_qkv + h * D;
  const T* kg = reinterpret_cast<const T*>(a.k) + (size_t)n * L * a.ld_qkv + h * D;
  const T* vg = reinterpret_cast<const T*>(a.v) + (size_t)n * L * a.ld_qkv + h * D;
  const int q0 = qb * 128 + wave * 32;

  chunk16 qf[NQT][NKB];                                       // B operand of S^T: query lr, d = 32 kb + 8 lq .. +7
#pragma unroll
  for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      const int qi = q0 + qt * 16 + lr;
      qf[qt][kb] = *reinterpret_cast<const chunk16*>(qg + (size_t)(qi < L ? qi : L - 1) * a.ld_qkv + kb * 32 + lq * 8);
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
  // The softmax keeps the running max of the RAW scores (the scale is positive: same arg max) and forms p = exp2(s * sc2 - m * sc2) as ONE
  // fused multiply-add per score in front of v_exp_f32; keys past L are masked only in a block that holds some (the DiT token counts have
  // none).  Per 64-key block and wave the kernel issues 34 v_exp_f32 (16 cycles each) and ~120 other VALU instructions against 512 cycles
  // of MFMA; the scale multiply, the subtraction and the per-score select were another ~90 (467 -> 507 TFLOP/s f16, 529 -> 578 bf16 on
  // 1024 tokens x 12 heads x 64; the serial MFMA -> max -> shuffle -> exp -> pack -> MFMA chain of a wave is what remains).

  chunk16 ks[NST], vs[NST];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int idx = i * 256 + t, r = idx / CPR, c = idx - r * CPR;
      const int key = k0 + r;
      ks[i] = chunk16{0u, 0u, 0u, 0u}; vs[i] = ks[i];
      if (key < L) {
        ks[i] = *reinterpret_cast<const chunk16*>(kg + (size_t)key * a.ld_qkv + c * 8);
        vs[i] = *reinterpret_cast<const chunk16*>(vg + (size_t)key * a.ld_qkv + c * 8);
      }
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int idx = i * 256 + t, r = idx / CPR, c = idx - r * CPR;
      *reinterpret_cast<chunk16*>(Kl + (buf * KB + r) * PITCH + c * 8) = ks[i];
      *reinterpret_cast<chunk16*>(Vl + (buf * KB + r) * PITCH + c * 8) = vs[i];
    }
  };
  fetch(0);
  stash(0);
  __syncthreads();
  const int nblk = (L + KB - 1) / KB;
  // one key block; RAGGED: it holds keys past L (only the last block of a sequence that is not a multiple of KB: its own copy of the
  // body behind the loop — as a condition inside one body hipcc turns the mask back into per-score selects)
  auto run_block = [&](int ib, auto raggedc) {
    constexpr bool ragged = decltype(raggedc)::value;
    const int k0 = ib * KB, buf = ib & 1;
    if (ib + 1 < nblk) fetch(k0 + KB);                        // lands under this block's MFMAs
    const T* Kb = Kl + buf * KB * PITCH;
    const T* Vb = Vl + buf * KB * PITCH;
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
      f32x4 S[NKT];
      float mx = m[qt];                                       // running max of the raw scores
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        f32x4 acc = attn_score_tile<T, NKB, PITCH>(Kb, kt, qf[qt], lr, lq);
        if constexpr (ragged) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (k0 + kt * 16 + lq * 4 + r >= L) acc[r] = -INFINITY;     // keys past L never win the max nor add to the sum
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, acc[r]);
        S[kt] = acc;
      }
      mx = col4_max(mx);
      const float nms = -mx * sc2;
      const float corr = __builtin_amdgcn_exp2f(__builtin_fmaf(m[qt], sc2, nms));    // exp2(-inf) = 0 on the first block
      m[qt] = mx;
      s16x4 P[NKT];
      const float ps = attn_exp_pack<T>(S, P, [&](float s) { return __builtin_amdgcn_exp2f(__builtin_fmaf(s, sc2, nms)); });
      l[qt] = l[qt] * corr + ps;                              // per-lane partial row sum (corr is the same in the column's four lanes): reduced once, behind the loop
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        f32x4 acc = O[qt][dt];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] *= corr;
        O[qt][dt] = attn_pv_step<T, NKT, PITCH>(acc, Vb, dt, P, lr, lq);
      }
    }
    if (ib + 1 < nblk) stash(buf ^ 1);
    __syncthreads();
  };
  const int nfull = L / KB;
  for (int ib = 0; ib < nfull; ++ib) run_block(ib, std::false_type{});
  if (nfull < nblk) run_block(nfull, std::true_type{});
#pragma unroll
  for (int qt = 0; qt < NQT; ++qt) {
    const int qi = q0 + qt * 16 + lr;
    const float inv = 1.0f / col4_sum(l[qt]);                 // (all lanes take part in the swaps: before the bounds test)
    if (qi >= L) continue;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      typename Elem<T>::vec4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = Elem<T>::from_f(O[qt][dt][r] * inv);
      *reinterpret_cast<typename Elem<T>::vec4*>(reinterpret_cast<T*>(a.out) + ((size_t)n * L + qi) * a.ld_out + h * D + dt * 16 + lq * 4) = o;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Token counts of the UNets' deep levels (L = 16 ... 64: 4x4 / 8x8 images): ONE WAVE per (sample, head) pair, four pairs per
// workgroup, nothing shared between waves and therefore no workgroup barrier.  Same arithmetic as attn_flash_t_kernel with a
// single key block: K and V of the pair are staged row-major (16-byte chunks) in a wave-private LDS strip; S^T = K Q^T
// (D-fragment = 4 consecutive keys of one query per lane), softmax in registers on log2-scaled scores (v_exp_f32, two
// xor-shuffles per query), the packed P^T D-fragments fed back as the B operand of O^T += V^T P^T with the A operand read by
// ds_read_b64_tr_b16, 8-byte output stores.  The first matrix-core kernel for these shapes (attn_mfma_kernel above: V transposed
// by 2-byte LDS writes, P through LDS, 2-byte strided output stores, one workgroup barrier) ran them at 2.5 - 2.9 TB/s of the
// q/k/v + output bytes they are bound by.
template <typename T, int D, int NKT>                          // NKT: 16-key tiles per pair (even; L <= 16 NKT, keys past L masked)
__global__ __launch_bounds__(256) void attn_wave_kernel(const SeqAttnArgs a) {
  constexpr int LP = NKT * 16, NDT = D / 16, NKB = D / 32;
  constexpr int PITCH = D + 8, CPR = D / 8;
  constexpr int NCH = LP * CPR / 64;                           // staging chunks per lane and operand
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane & 15, lq = lane >> 4;
  const int L = a.L;
  const long long pair = (long long)blockIdx.x * 4 + wave;
  if (pair >= (long long)a.n * a.heads) return;               // whole waves leave: nothing below is shared between waves
  const int n = (int)(pair / a.heads), h = (int)(pair % a.heads);
  T* const Kl = reinterpret_cast<T*>(smem) + (size_t)wave * 2 * LP * PITCH;
  T* const Vl = Kl + LP * PITCH;
  const T* qg = reinterpret_cast<const T*>(a.q) + (size_t)n * L * a.ld_qkv + h * D;
  const T* kg = reinterpret_cast<const T*>(a.k) + (size_t)n * L * a.ld_qkv + h * D;
  const T* vg = reinterpret_cast<const T*>(a.v) + (size_t)n * L * a.ld_qkv + h * D;
  // ---- every query fragment of the pair up front (B operand of S^T: query lr, d = 32 kb + 8 lq .. +7): their latency then sits
  // under the K / V staging instead of in front of each query tile ----
  chunk16 qfa[NKT][NKB];
#pragma unroll
  for (int qt = 0; qt < NKT; ++qt)
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      const int qi = qt * 16 + lr;
      qfa[qt][kb] = *reinterpret_cast<const chunk16*>(qg + (size_t)(qi < L ? qi : L - 1) * a.ld_qkv + kb * 32 + lq * 8);
    }
  // ---- stage K and V (rows past L as zeros: a masked key has P = 0, and 0 x garbage must not be a NaN) ----
#pragma unroll
  for (int i0 = 0; i0 < NCH; i0 += 8) {
    chunk16 kc[8], vc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (i0 + u < NCH) {
        const int idx = (i0 + u) * 64 + lane, r = idx / CPR, c = idx - r * CPR;
        kc[u] = chunk16{0u, 0u, 0u, 0u}; vc[u] = kc[u];
        if (r < L) {
          kc[u] = *reinterpret_cast<const chunk16*>(kg + (size_t)r * a.ld_qkv + c * 8);
          vc[u] = *reinterpret_cast<const chunk16*>(vg + (size_t)r * a.ld_qkv + c * 8);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (i0 + u < NCH) {
        const int idx = (i0 + u) * 64 + lane, r = idx / CPR, c = idx - r * CPR;
        *reinterpret_cast<chunk16*>(Kl + r * PITCH + c * 8) = kc[u];
        *reinterpret_cast<chunk16*>(Vl + r * PITCH + c * 8) = vc[u];
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const float sc2 = a.scale * 1.4426950408889634f;
  const int nqt = (L + 15) >> 4;
#pragma unroll
  for (int qt = 0; qt < NKT; ++qt) {                           // (unrolled: qfa is indexed statically; the bound is wave-uniform)
    if (qt >= nqt) break;
    const int qi = qt * 16 + lr;
    f32x4 S[NKT];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      f32x4 acc = attn_score_tile<T, NKB, PITCH>(Kl, kt, qfa[qt], lr, lq);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool kvalid = kt * 16 + lq * 4 + r < L;
        acc[r] = kvalid ? acc[r] : -INFINITY;                 // raw scores: the scale is positive, it enters with the max below
        mx = fmaxf(mx, acc[r]);
      }
      S[kt] = acc;
    }
    mx = col4_max(mx);
    const float nms = -mx * sc2;
    s16x4 P[NKT];
    float ps = attn_exp_pack<T>(S, P, [&](float s) { return __builtin_amdgcn_exp2f(__builtin_fmaf(s, sc2, nms)); });
    ps = col4_sum(ps);
    const float inv = __builtin_amdgcn_rcpf(ps);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      const f32x4 acc = attn_pv_step<T, NKT, PITCH>(f32x4{0.f, 0.f, 0.f, 0.f}, Vl, dt, P, lr, lq);
      if (qi < L) {
        typename Elem<T>::vec4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = Elem<T>::from_f(acc[r] * inv);
        *reinterpret_cast<typename Elem<T>::vec4*>(reinterpret_cast<T*>(a.out) + ((size_t)n * L + qi) * a.ld_out + h * D + dt * 16 + lq * 4) = o;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Exact fp32 kernel: attn_exact_run over the plain key bound L (no lengths: a.len is null).  (A mode of its own that masks nothing —
// the exact body never walks a key at or past the bound — was measured and is slower: DESIGN.md §6l.)
template <typename T, int SW>        // SW: slice width (16: d = 16/32/64/128; 24: d = 96)
__global__ __launch_bounds__(256) void attn_self_f32_kernel(const SeqAttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float kv[];  // K[KB][d], V[KB][d]
  int i, h, q0;
  exact_item(a.heads, a.L, 256 / (a.d / SW), i, h, q0);
  const StripView<T> w = seq_view<T>(a, i, h, a.d, q0);
  attn_exact_run<T, SW>(w, PlainMode{{w.nk}}, a.scale, a.d, a.KB, kv);
}

// ------------------------------------------------------------------------------------------------
static int attn_validate(const dc_attention_params* p) {
  DC_REQUIRE(p && p->q && p->k && p->v && p->out, DC_ERR_ARG, "dc_attention: null pointer");
  DC_REQUIRE(p->d == 16 || p->d == 32 || p->d == 64 || p->d == 96 || p->d == 128, DC_ERR_SHAPE, "dc_attention: head dim %d (16/32/64/96/128)", p->d);
  DC_REQUIRE(p->n > 0 && p->L > 0 && p->heads > 0, DC_ERR_SHAPE, "dc_attention: n/L/heads");
  DC_REQUIRE(p->ld_qkv >= p->heads * p->d && p->ld_out >= p->heads * p->d, DC_ERR_SHAPE, "dc_attention: ld");
  // the matrix-core kernels keep the running max of the RAW scores and fold the scale into the exponent's FMA: valid for scale > 0 only
  DC_REQUIRE(p->scale > 0.f, DC_ERR_ARG, "dc_attention: scale must be positive (got %g)", (double)p->scale);
  return DC_OK;
}

enum AttnRoute { ATTN_WAVE, ATTN_MFMA, ATTN_FLASH, ATTN_FP32 };

// Everything a valid problem decides, decided once: dc_attention launches from it, dc_attention_variant names its route.
struct AttnPlan {
  AttnRoute route;
  int D;             // wave, flash: the instance's head dim
  int NKT;           // wave: 16-key tiles per pair, 2 or 4 (an even count: the P.V MFMAs take key tiles in pairs)
  int G, Lp;         // mfma: pairs per workgroup; L rounded up to a multiple of 32
  int SW, KB;        // fp32: slice width; keys per LDS block
  size_t lds;        // dynamic LDS of a workgroup
  long long nb;      // workgroups
};

// L <= 64: one wave per pair (attn_wave_kernel); up to 128: the whole-sequence matrix-core kernel; beyond: the flash kernel, which
// also wins at 256 tokens (CheXpert 16x16 level, d = 64: 2.37 -> 0.71 ms per step; IPMSA: 13.2 -> 4.8 ms).  d = 96 (768 channels,
// 8 heads; 72 / 80 padded in the packed weights) has no wave instance: the whole-sequence kernel up to 128 tokens, the flash kernel beyond.
// fp32 (the parity path) and shapes the matrix-core kernels do not take: the exact fp32 kernel.
// The route is filled in even where the grid is refused (DC_ERR_SHAPE): dc_attention_variant names it regardless.
static int attn_plan(const dc_attention_params* p, AttnPlan& pl) {
  constexpr size_t lds_max = 160 * 1024;
  const int L = p->L, d = p->d;
  const long long pairs = (long long)p->n * p->heads;
  // 16-bit with q / k / v rows readable as 16-byte chunks: every matrix-core kernel needs it.  The wave and flash kernels store 8 bytes
  // at a time and need the output rows aligned as well; the whole-sequence kernel stores 2 bytes at a time and takes any output.
  const bool in_ok = strip_route_ok(p->dtype, p->q, p->k, p->v, nullptr, p->ld_qkv, p->ld_qkv, 0);
  const bool io_ok = strip_route_ok(p->dtype, p->q, p->k, p->v, p->out, p->ld_qkv, p->ld_qkv, p->ld_out);
  const size_t lds_all = (size_t)2 * L * d * sizeof(float);    // the fp32 image of the whole sequence
  // the whole-sequence kernel's form, if it has one: per pair K [L][d + 8] and V^T [d][Lp + 8], per wave a P strip [16][Lp + 8]
  const int G = (L <= 128 && L % 16 == 0 && d % 32 == 0) ? attn_pairs_per_wg(L, d) : 0, Lp = (L + 31) / 32 * 32;
  const size_t lds_mfma = (size_t)G * (L * (d + 8) + d * (Lp + 8)) * 2 + (size_t)4 * 16 * (Lp + 8) * 2;
  pl = AttnPlan{};
  if (io_ok && L <= 64 && (d == 32 || d == 64 || d == 128)) {
    pl.route = ATTN_WAVE; pl.D = d; pl.NKT = L <= 32 ? 2 : 4;
    pl.lds = (size_t)4 * 2 * pl.NKT * 16 * (d + 8) * 2;        // per wave a K and a V strip of 16 NKT rows
    pl.nb = (pairs + 3) / 4;
  } else if (in_ok && G && lds_mfma <= lds_max) {
    pl.route = ATTN_MFMA; pl.G = G; pl.Lp = Lp;
    pl.lds = lds_mfma;
    pl.nb = (pairs + G - 1) / G;
  } else if (io_ok && (L > 128 || lds_all > lds_max) && (d == 32 || d == 64 || d == 96 || d == 128)) {
    pl.route = ATTN_FLASH; pl.D = d;
    pl.lds = (size_t)4 * flash_kb(d) * (d + 8) * 2;            // K and V, two buffers each
    pl.nb = pairs * ((L + 127) / 128);
  } else {
    // K / V stay whole in LDS when they fit 160 KiB (one block: the order of operations of the UNet parity path is unchanged), else
    // stream in 64 KiB blocks
    pl.route = ATTN_FP32; pl.SW = d == 96 ? 24 : 16;
    pl.KB = lds_all <= lds_max ? L : 8192 / d;
    pl.lds = (size_t)2 * pl.KB * d * sizeof(float);
    const int QT = 256 / (d / pl.SW);
    pl.nb = pairs * ((L + QT - 1) / QT);
  }
  DC_REQUIRE(pl.nb < (1LL << 31), DC_ERR_SHAPE, "dc_attention: grid too large");
  return DC_OK;
}

extern "C" const char* dc_attention_variant(const dc_attention_params* p) {
  if (attn_validate(p) != DC_OK) return "invalid";
  static const char* const names[] = {"wave", "mfma", "flash", "fp32"};
  AttnPlan pl;
  (void)attn_plan(p, pl);
  return names[pl.route];
}

// the launch of one kernel instance; its first one lifts the instance's dynamic LDS limit to what any plan can ask for
template <auto KERN, typename A>
static int attn_launch(const A& a, const AttnPlan& pl, hipStream_t s, const char* what) {
  static bool done = false;
  if (!done) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); done = true; }
  hipLaunchKernelGGL(KERN, dim3((unsigned)pl.nb), dim3(256), pl.lds, s, a);
  return dc_check_launch(what);
}

extern "C" int dc_attention(const dc_attention_params* p, dc_stream stream) {
  int rc = attn_validate(p);
  if (rc != DC_OK) return rc;
  AttnPlan pl;
  if ((rc = attn_plan(p, pl)) != DC_OK) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const SeqAttnArgs a{p->q, p->k, p->v, p->out, nullptr, p->n, p->L, p->heads, p->d, p->ld_qkv, p->ld_out, p->scale, pl.KB};
  if (pl.route == ATTN_FP32)
    return dc_by_dtype(p->dtype, "dc_attention: dtype", [&](auto t) {
      using T = decltype(t);
      return pl.SW == 24 ? attn_launch<attn_self_f32_kernel<T, 24>>(a, pl, s, "dc_attention") : attn_launch<attn_self_f32_kernel<T, 16>>(a, pl, s, "dc_attention");
    });
  return dc_by_dtype16(p->dtype, "dc_attention: dtype", [&](auto t) {
    using T = decltype(t);
    const char* const fl = "dc_attention(flash_t)";
    const char* const wv = "dc_attention(wave)";
    switch (pl.route) {
      case ATTN_WAVE: {
        const bool two = pl.NKT == 2;
        if (pl.D == 32) return two ? attn_launch<attn_wave_kernel<T, 32, 2>>(a, pl, s, wv) : attn_launch<attn_wave_kernel<T, 32, 4>>(a, pl, s, wv);
        if (pl.D == 64) return two ? attn_launch<attn_wave_kernel<T, 64, 2>>(a, pl, s, wv) : attn_launch<attn_wave_kernel<T, 64, 4>>(a, pl, s, wv);
        return two ? attn_launch<attn_wave_kernel<T, 128, 2>>(a, pl, s, wv) : attn_launch<attn_wave_kernel<T, 128, 4>>(a, pl, s, wv);
      }
      case ATTN_MFMA: {
        AttnMArgs am{a, pl.G, pl.Lp};
        return attn_launch<attn_mfma_kernel<T>>(am, pl, s, "dc_attention(mfma)");
      }
      default:
        if (pl.D == 32) return attn_launch<attn_flash_t_kernel<T, 32>>(a, pl, s, fl);
        if (pl.D == 64) return attn_launch<attn_flash_t_kernel<T, 64>>(a, pl, s, fl);
        if (pl.D == 96) return attn_launch<attn_flash_t_kernel<T, 96>>(a, pl, s, fl);
        return attn_launch<attn_flash_t_kernel<T, 128>>(a, pl, s, fl);
    }
  });
}
