// attention_wide.hip — dc_attention_wide: softmax(q k^T * scale) v per (sample, head) for heads of 256 or 512 channels, gfx950.
//
// The mid block of an AutoencoderKL encoder is single-head attention whose head is the whole channel count (512 for the published SD
// VAEs); dc_attention stops at d = 128.  Two kernels, chosen once per call by wide_route:
//   attn_wide_kernel      16-bit, aligned operands ("wide"): one WORKGROUP of four waves per (sample, head, 32 queries).  The output
//                         strip of a query tile is d fp32 columns wide and does not fit one wave the way attn_strip_run holds it, so wave w
//                         owns slice w of the head dimension (DS = d / 4 channels) twice over: as the K-slice of the score product and as
//                         the column slice of the output.  Per block of 32 keys
//                           partial S^T   attn_score_tile over the wave's slice of q (registers) and of K (its own LDS strip)
//                           S^T           the four partials summed through LDS in fp32, always as ((w0 + w1) + w2) + w3: every wave then
//                                         holds the same full tile
//                           softmax       online, fp32, log2 units, in every wave (redundant and cheap: 8 exponentials per lane and block)
//                           O^T += V^T P^T  attn_pv_step for the wave's own DS columns only
//                         A wave stages only its own column slice of K and V (wave-private strips, as in attn_strip_run), so no operand
//                         byte is loaded twice within a workgroup; the exchange of the partials is the one thing shared, and its two
//                         workgroup barriers are the only ones of a key block.  Keys at or past L are staged as zeros and masked.
//   attn_wide_f32_kernel  f32, and 16-bit operands the first cannot read ("fp32"): attn_exact_run of attn_strip.h with 32-wide slices, a
//                         query on 8 (d = 256) or 16 (d = 512) adjacent lanes.
// Fixed summation order, no atomics: the bits of out[i] depend on sample i's own rows only.
#include "attn_strip.h"

static constexpr int WIDE_KB = 32;      // keys per block of attn_wide_kernel
static constexpr int WIDE_SW = 32;      // slice width of the exact kernel: d / 32 = 8 or 16 lanes per query, a power of two

// dynamic LDS of attn_wide_kernel: per wave a K and a V strip of KB rows of d / 4 + 8 elements, then per wave 4 score tiles of 64 x 16 bytes
static constexpr size_t wide_lds_bytes(int d) { return (size_t)4 * 2 * WIDE_KB * (d / 4 + 8) * 2 + (size_t)4 * 4 * 64 * sizeof(f32x4); }

template <typename T, int D>
__global__ __launch_bounds__(256) void attn_wide_kernel(const SeqAttnArgs a) {
  constexpr int DS = D / 4, KB = WIDE_KB;
  constexpr int NKT = KB / 16, NQT = 2, NDT = DS / 16, NKB = DS / 32;
  constexpr int PITCH = DS + 8, CPR = DS / 8;                 // LDS row pitch in elements (+16 B); 16-byte chunks per strip row
  constexpr int NCH = KB * CPR / 64;                          // staging chunks per lane and operand
  static_assert(KB * CPR % 64 == 0 && NKT == 2 && DS % 32 == 0, "whole staging chunks, one pair of key tiles, 32-wide k-chunks");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  T* const Kl = reinterpret_cast<T*>(smem) + (size_t)wave * 2 * KB * PITCH;
  T* const Vl = Kl + KB * PITCH;
  f32x4* const Xs = reinterpret_cast<f32x4*>(smem + (size_t)4 * 2 * KB * PITCH * sizeof(T));   // [wave][qt][kt][lane]
  const int L = a.L;
  const int qtiles = (L + 31) / 32;
  int b = blockIdx.x;
  const int q0 = b % qtiles * 32; b /= qtiles;
  const int h = b % a.heads, i = b / a.heads;
  const size_t in0 = (size_t)i * L * a.ld_qkv + h * D + wave * DS;     // this wave's column slice
  const T* qg = reinterpret_cast<const T*>(a.q) + in0;
  const T* kg = reinterpret_cast<const T*>(a.k) + in0;
  const T* vg = reinterpret_cast<const T*>(a.v) + in0;
  T* og = reinterpret_cast<T*>(a.out) + (size_t)i * L * a.ld_out + h * D + wave * DS;
  const int nqt = min(NQT, (L - q0 + 15) >> 4);               // 16-query tiles that hold a query: the same in all four waves

  chunk16 qf[NQT][NKB];                                       // B operand of S^T: query lr, d = 32 kb + 8 lq .. +7 of the slice
#pragma unroll
  for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      const int qi = q0 + qt * 16 + lr;
      qf[qt][kb] = *reinterpret_cast<const chunk16*>(qg + (size_t)(qi < L ? qi : L - 1) * a.ld_qkv + kb * 32 + lq * 8);
    }
  f32x4 O[NQT][NDT];                                          // O^T: rows d = 16 dt + 4 lq + r of the slice, column = query lr
  float m[NQT], l[NQT];
#pragma unroll
  for (int qt = 0; qt < NQT; ++qt) {
    m[qt] = -INFINITY; l[qt] = 0.f;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) O[qt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float sc2 = a.scale * 1.4426950408889634f;            // scores in log2 units

  chunk16 ks[NCH], vs[NCH];
  auto fetch = [&](int k0) {                                  // keys >= L: zeros, and no load
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
      const int idx = u * 64 + lane, r = idx / CPR, c = idx - r * CPR;
      ks[u] = chunk16{0u, 0u, 0u, 0u}; vs[u] = ks[u];
      if (k0 + r < L) {
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
  // the strips are private to a wave and LDS executes a wave's operations in issue order (attn_strip_run)
  auto wave_sync = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  const int nblk = (L + KB - 1) / KB;
  auto run_block = [&](int ib, auto lastc) {
    constexpr bool LAST = decltype(lastc)::value;             // the block that may hold keys at or past L
    const int k0 = ib * KB;
    const bool more = ib + 1 < nblk;
    if (more) fetch(k0 + KB);                                 // lands under this block's MFMAs
    // ---- the wave's partial of S^T over its DS channels, handed to the other three ----
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
      if (qt >= nqt) break;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
        Xs[((wave * NQT + qt) * NKT + kt) * 64 + lane] = attn_score_tile<T, NKB, PITCH>(Kl, kt, qf[qt], lr, lq);
    }
    __syncthreads();
    f32x4 Sc[NQT][NKT];
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
      if (qt >= nqt) break;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        f32x4 s = Xs[((0 * NQT + qt) * NKT + kt) * 64 + lane];
#pragma unroll
        for (int w = 1; w < 4; ++w) s += Xs[((w * NQT + qt) * NKT + kt) * 64 + lane];    // ((w0 + w1) + w2) + w3 in every wave
        Sc[qt][kt] = s;
      }
    }
    __syncthreads();                                          // the partials are read: the next block may overwrite them
    // ---- from here on as one wave of attn_strip_run, for DS of the D output columns ----
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
      if (qt >= nqt) break;
      float mx = m[qt];                                       // running max of the raw scores (scale > 0: same arg max)
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (LAST && k0 + kt * 16 + lq * 4 + r >= L) Sc[qt][kt][r] = -INFINITY;   // before the max: never wins it nor adds to the sum
          mx = fmaxf(mx, Sc[qt][kt][r]);
        }
      mx = col4_max(mx);                                      // finite: every block that runs holds key k0 < L
      const float nms = -mx * sc2;
      auto p2 = [&](float s) { return __builtin_amdgcn_exp2f(__builtin_fmaf(s, sc2, nms)); };   // exp2(-inf) = 0 exactly
      const float corr = p2(m[qt]);                           // 0 on the first block
      m[qt] = mx;
      s16x4 P[NKT];
      const float ps = attn_exp_pack<T>(Sc[qt], P, p2);
      l[qt] = l[qt] * corr + ps;                              // per-lane partial row sum of the unrounded p: reduced once, behind the loop
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        f32x4 acc = O[qt][dt];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] *= corr;
        O[qt][dt] = attn_pv_step<T, NKT, PITCH>(acc, Vl, dt, P, lr, lq);
      }
    }
    if (more) {
      wave_sync();                                            // this block's strip reads are issued before the strip is overwritten
      stash();
      wave_sync();
    }
  };
  fetch(0);
  stash();
  wave_sync();
  const int nfull = L / KB;
  for (int ib = 0; ib < nfull; ++ib) run_block(ib, std::false_type{});
  if (nfull < nblk) run_block(nfull, std::true_type{});
#pragma unroll
  for (int qt = 0; qt < NQT; ++qt) {
    if (qt >= nqt) break;
    const int qi = q0 + qt * 16 + lr;
    const float inv = 1.0f / col4_sum(l[qt]);                 // (all lanes take part in the swaps: before the bounds test)
    if (qi >= L) continue;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      typename Elem<T>::vec4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = Elem<T>::from_f(O[qt][dt][r] * inv);
      *reinterpret_cast<typename Elem<T>::vec4*>(og + (size_t)qi * a.ld_out + dt * 16 + lq * 4) = o;
    }
  }
}

// the exact kernel: attn_exact_run over the plain key bound L
template <typename T>
__global__ __launch_bounds__(256) void attn_wide_f32_kernel(const SeqAttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float kv[];  // K[KB][d], V[KB][d]
  int i, h, q0;
  exact_item(a.heads, a.L, 256 / (a.d / WIDE_SW), i, h, q0);
  const StripView<T> w = seq_view<T>(a, i, h, a.d, q0);
  attn_exact_run<T, WIDE_SW>(w, PlainMode{{w.nk}}, a.scale, a.d, a.KB, kv);
}

// ------------------------------------------------------------------------------------------------
static int wide_validate(const dc_attention_wide_params* p) {
  DC_REQUIRE(p && p->q && p->k && p->v && p->out, DC_ERR_ARG, "dc_attention_wide: null pointer");
  DC_REQUIRE(p->dtype == DC_F32 || p->dtype == DC_BF16 || p->dtype == DC_F16, DC_ERR_DTYPE, "dc_attention_wide: dtype %d", p->dtype);
  DC_REQUIRE(p->d == 256 || p->d == 512, DC_ERR_SHAPE, "dc_attention_wide: head dim %d (256/512)", p->d);
  DC_REQUIRE(p->n > 0 && p->L > 0 && p->heads > 0, DC_ERR_SHAPE, "dc_attention_wide: n/L/heads");
  DC_REQUIRE((long long)p->ld_qkv >= (long long)p->heads * p->d && (long long)p->ld_out >= (long long)p->heads * p->d, DC_ERR_SHAPE,
             "dc_attention_wide: ld");
  const uintptr_t es = (uintptr_t)dc_dtype_size(p->dtype) - 1;
  DC_REQUIRE((((uintptr_t)p->q | (uintptr_t)p->k | (uintptr_t)p->v | (uintptr_t)p->out) & es) == 0, DC_ERR_ALIGN,
             "dc_attention_wide: q/k/v/out must be element aligned");
  // the matrix-core kernel keeps the running max of the RAW scores and folds the scale into the exponent's FMA, the exact kernel folds
  // it into q: both are written for scale > 0
  DC_REQUIRE(p->scale > 0.f, DC_ERR_ARG, "dc_attention_wide: scale must be positive (got %g)", (double)p->scale);
  return DC_OK;
}

// the matrix-core route: 16-bit, q / k / v rows readable as 16-byte chunks (pointers 16-byte aligned, ld_qkv % 8 == 0) and output rows
// writable 8 bytes at a time (pointer 8-byte aligned, ld_out % 4 == 0); a head's and a wave's column offsets are multiples of 64
static bool wide_route(const dc_attention_wide_params* p) {
  return strip_route_ok(p->dtype, p->q, p->k, p->v, p->out, p->ld_qkv, p->ld_qkv, p->ld_out);
}

extern "C" const char* dc_attention_wide_variant(const dc_attention_wide_params* p) {
  if (wide_validate(p) != DC_OK) return "invalid";
  return wide_route(p) ? "wide" : "fp32";
}

template <auto KERN>
static int wide_launch(const SeqAttnArgs& a, long long nb, size_t lds, hipStream_t s, const char* what) {
  static bool done = false;
  if (!done) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); done = true; }
  DC_REQUIRE(nb < (1LL << 31), DC_ERR_SHAPE, "dc_attention_wide: grid too large");
  hipLaunchKernelGGL(KERN, dim3((unsigned)nb), dim3(256), lds, s, a);
  return dc_check_launch(what);
}

extern "C" int dc_attention_wide(const dc_attention_wide_params* p, dc_stream stream) {
  int rc = wide_validate(p);
  if (rc != DC_OK) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SeqAttnArgs a{p->q, p->k, p->v, p->out, nullptr, p->n, p->L, p->heads, p->d, p->ld_qkv, p->ld_out, p->scale, 0};
  if (wide_route(p)) {
    const long long nb = (long long)p->n * p->heads * ((p->L + 31) / 32);
    const size_t lds = wide_lds_bytes(p->d);
    return dc_by_dtype16(p->dtype, "dc_attention_wide: dtype", [&](auto t) {
      using T = decltype(t);
      return p->d == 256 ? wide_launch<attn_wide_kernel<T, 256>>(a, nb, lds, s, "dc_attention_wide(wide)")
                         : wide_launch<attn_wide_kernel<T, 512>>(a, nb, lds, s, "dc_attention_wide(wide)");
    });
  }
  ExactPlan e;
  if ((rc = exact_plan(p->n, p->heads, p->L, p->L, p->d, WIDE_SW, "dc_attention_wide", e)) != DC_OK) return rc;
  a.KB = e.KB;
  return dc_by_dtype(p->dtype, "dc_attention_wide: dtype", [&](auto t) {
    using T = decltype(t);
    return wide_launch<attn_wide_f32_kernel<T>>(a, e.nb, e.lds, s, "dc_attention_wide(fp32)");
  });
}
