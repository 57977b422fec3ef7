// elementwise.hip — the HBM-bound ends of the scoring step, gfx950:
//   q_sample (+ im2col of conv_in), Philox normal noise, sinusoidal log-SNR embedding,
//   eps-MSE reduction, the sampler steps and the noise map of the ancestral one, Haar DWT / inverse.
// Reference lines: diffusion/diffusion_classifier.py:100-117, :690-692 (q_sample),
// :706-711 (v->eps, squared L2 error); utils/wavelet.py:4-68 (Haar); diffusers Timesteps.
#include "common.h"

// ------------------------------------------------------------------ q_sample -------
struct QsArgs {
  const float* x; const float* eps; const float* alpha; const float* sigma; const int32_t* img_of_bj;
  void* out; int out_dtype, n_bj, C, H, W, ld, im2col, patch;
};

template <typename TO>
__global__ __launch_bounds__(256) void qsample_kernel(const QsArgs a) {
  constexpr int EPC = Elem<TO>::EPC;
  const int cpr = a.ld / EPC;                       // chunks per output row
  const int HW = a.H * a.W;
  const int pp = a.im2col == 2 ? a.patch : 1;
  const int gw = a.W / pp, rows_per = (a.H / pp) * gw;   // output rows per sample
  const long long total = (long long)a.n_bj * rows_per * cpr;
  for (long long idx = blockIdx.x * 256LL + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int ch = (int)(idx % cpr);
    const long long row = idx / cpr;
    const int p = (int)(row % rows_per);
    const int bj = (int)(row / rows_per);
    const int img = a.img_of_bj ? a.img_of_bj[bj] : bj;
    const float al = a.alpha[bj], sg = a.sigma[bj];
    const int y = p / gw, xw = p - y * gw;
    float f[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      const int k = ch * EPC + e;
      float v = 0.f;
      if (!a.im2col) {
        if (k < a.C) {
          const size_t o = (size_t)k * HW + p;
          v = al * a.x[(size_t)img * a.C * HW + o] + sg * a.eps[(size_t)bj * a.C * HW + o];
        }
      } else if (a.im2col == 2) {
        if (k < a.C * pp * pp) {
          const int c = k / (pp * pp), r = k - c * pp * pp;
          const size_t o = (size_t)c * HW + (size_t)(y * pp + r / pp) * a.W + (xw * pp + r % pp);
          v = al * a.x[(size_t)img * a.C * HW + o] + sg * a.eps[(size_t)bj * a.C * HW + o];
        }
      } else if (k < 9 * a.C) {
        const int tap = k / a.C, c = k - tap * a.C;
        const int iy = y + tap / 3 - 1, ix = xw + tap % 3 - 1;
        if ((unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W) {
          const size_t o = (size_t)c * HW + (size_t)iy * a.W + ix;
          v = al * a.x[(size_t)img * a.C * HW + o] + sg * a.eps[(size_t)bj * a.C * HW + o];
        }
      }
      f[e] = v;
    }
    reinterpret_cast<chunk16*>(a.out)[idx] = f_to_chunk<TO>(f);
  }
}

extern "C" int dc_qsample(const dc_qsample_params* p, dc_stream stream) {
  DC_REQUIRE(p && p->x && p->eps && p->alpha && p->sigma && p->out, DC_ERR_ARG, "dc_qsample: null pointer");
  const int epc = 16 / dc_dtype_size(p->out_dtype);
  DC_REQUIRE(p->n_bj > 0 && p->C > 0 && p->H > 0 && p->W > 0, DC_ERR_SHAPE, "dc_qsample: extents");
  DC_REQUIRE(p->im2col >= 0 && p->im2col <= 2, DC_ERR_ARG, "dc_qsample: im2col=%d", p->im2col);
  int need = p->C, pp = 1;
  if (p->im2col == 1) need = 9 * p->C;
  if (p->im2col == 2) {
    pp = p->patch;
    DC_REQUIRE(pp > 0 && p->H % pp == 0 && p->W % pp == 0, DC_ERR_SHAPE, "dc_qsample: patch=%d does not tile %dx%d", pp, p->H, p->W);
    need = p->C * pp * pp;
  }
  DC_REQUIRE(p->ld % epc == 0 && p->ld >= need, DC_ERR_SHAPE, "dc_qsample: ld=%d (need >= %d, multiple of %d)", p->ld, need, epc);
  QsArgs a{p->x, p->eps, p->alpha, p->sigma, p->img_of_bj, p->out, p->out_dtype, p->n_bj, p->C, p->H, p->W, p->ld, p->im2col, pp};
  const long long total = (long long)p->n_bj * (p->H / pp) * (p->W / pp) * (p->ld / epc);
  const unsigned grid = (unsigned)((total + 255) / 256 > 65536 ? 65536 : (total + 255) / 256);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return dc_by_dtype(p->out_dtype, "dc_qsample: out_dtype", [&](auto t) {
    hipLaunchKernelGGL((qsample_kernel<decltype(t)>), dim3(grid), dim3(256), 0, s, a);
    return dc_check_launch("dc_qsample");
  });
}

// ------------------------------------------------------------------ Philox normal --
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = n0; c[2] = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

__global__ __launch_bounds__(256) void philox_normal_kernel(float* out, long long rows, long long len4,
                                                            const int64_t* row_ids, uint64_t seed) {
  const long long n4 = rows * len4;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const long long r = i / len4, k = i - r * len4;
    const uint64_t ctr = (uint64_t)(row_ids ? row_ids[r] : r) * (uint64_t)len4 + (uint64_t)k;
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    float u[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) u[e] = ((float)(c[e] >> 8) + 0.5f) * (1.0f / 16777216.0f);  // (0,1)
    const float r0 = sqrtf(-2.0f * logf(u[0])), r1 = sqrtf(-2.0f * logf(u[2]));
    float s0, c0, s1, c1;
    sincosf(6.28318530717958647692f * u[1], &s0, &c0);
    sincosf(6.28318530717958647692f * u[3], &s1, &c1);
    reinterpret_cast<float4*>(out)[i] = make_float4(r0 * c0, r0 * s0, r1 * c1, r1 * s1);
  }
}

extern "C" int dc_philox_normal(float* out, int64_t rows, int64_t row_len, const int64_t* row_ids, uint64_t seed, dc_stream stream) {
  DC_REQUIRE(out && rows > 0 && row_len > 0 && row_len % 4 == 0, DC_ERR_ARG,
             "dc_philox_normal: rows=%lld row_len=%lld (row_len must be a positive multiple of 4)", (long long)rows, (long long)row_len);
  DC_REQUIRE(((uintptr_t)out & 15) == 0, DC_ERR_ALIGN, "dc_philox_normal: out must be 16-byte aligned");
  const long long n4 = rows * (row_len / 4);
  const unsigned grid = (unsigned)((n4 + 255) / 256 > 16384 ? 16384 : (n4 + 255) / 256);
  hipLaunchKernelGGL(philox_normal_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), out,
                     (long long)rows, (long long)(row_len / 4), row_ids, seed);
  return dc_check_launch("dc_philox_normal");
}

// ------------------------------------------------------------------ sinusoid -------
__global__ __launch_bounds__(256) void sinusoid_kernel(const float* lam, float* out, int n, int dim, int flip, float shift) {
  const int half = dim / 2;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n * half) return;
  const int r = i / half, k = i - r * half;
  const float ex = (-9.210340371976184f * (float)k) / ((float)half - shift);
  const float arg = lam[r] * expf(ex);
  const float sv = sinf(arg), cv = cosf(arg);
  float* o = out + (size_t)r * dim;
  if (flip) { o[k] = cv; o[half + k] = sv; } else { o[k] = sv; o[half + k] = cv; }
}

extern "C" int dc_sinusoid(const dc_sinusoid_params* p, dc_stream stream) {
  DC_REQUIRE(p && p->lam && p->out && p->n > 0 && p->dim > 0 && p->dim % 2 == 0, DC_ERR_ARG, "dc_sinusoid: bad args");
  const int total = p->n * (p->dim / 2);
  hipLaunchKernelGGL(sinusoid_kernel, dim3((total + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     p->lam, p->out, p->n, p->dim, p->flip_sin_to_cos, p->freq_shift);
  return dc_check_launch("dc_sinusoid");
}

// ------------------------------------------------------------------ eps-MSE --------
// One workgroup per unit; fixed-order accumulation (strided per lane -> xor tree per wave ->
// 4 wave partials added in order) so the result is bit-reproducible run to run.
struct MseArgs {
  const float* pred; const float* eps; const float* x; const float* alpha; const float* sigma;
  const int32_t* bj_of_unit; const int32_t* img_of_bj; const int32_t* out_index; float* out;
  int C, HW, ld, v_param, W, patch;
  float huber_delta;       // read by the DC_LOSS_HUBER instance only
};
struct MseWeightedArgs : MseArgs { LossWeights wt; };      // the weighted instances' argument: the unweighted ones keep theirs

// LOSS: the per-element term (common.h loss_term), a compile-time kind on all three read paths; the accumulation order is the same for
// every kind.  DC_LOSS_L2 ends in sqrt then square, the other two store the sum.
// WGT: the pixel / trial weights of the loss (dcamd.h dc_eps_mse_params), compile-time as well — the instances without them hold none
// of it.  m multiplies each term (loss_acc_weighted; the pixel-owner path loads it once per pixel), w the stored result.
template <int LOSS, bool WGT>
__global__ __launch_bounds__(256) void eps_mse_kernel(const std::conditional_t<WGT, MseWeightedArgs, MseArgs> a) {
  __shared__ float part[4];
  const int u = blockIdx.x, t = threadIdx.x;
  const int bj = a.bj_of_unit ? a.bj_of_unit[u] : u;
  const int img = a.img_of_bj ? a.img_of_bj[bj] : bj;
  const float al = a.alpha ? a.alpha[bj] : 1.f, sg = a.sigma ? a.sigma[bj] : 0.f;
  const size_t CHW = (size_t)a.C * a.HW;
  const float* pr = a.pred + (size_t)u * (a.patch > 1 ? a.HW / (a.patch * a.patch) : a.HW) * a.ld;
  const float* ep = a.eps + (size_t)bj * CHW;
  const float* xx = a.x ? a.x + (size_t)img * CHW : nullptr;
  const float* pw = nullptr;                       // WGT: the image's weight plane (NULL: ones)
  if constexpr (WGT) pw = a.wt.pixel_w ? a.wt.pixel_w + (size_t)img * a.HW : nullptr;
  float s = 0.f;
  if (a.patch <= 1 && a.C <= 16) {
    // image-shaped prediction with a few channels (UNets: C = 3..12): a lane owns whole pixels, so the C reads of an NHWC
    // row are back to back (cache hits after the first) and the C planes of eps / x are read coalesced across the wave.
    // (The element-indexed loop below walks plane by plane: every pass re-fetched the prediction, 4 bytes per row, and
    // paid a 64-bit division per element — 0.6 TB/s on the 256x256 workloads.)
    for (int p = t; p < a.HW; p += 256) {
      const float* row = pr + (size_t)p * a.ld;
      const float m = pw ? pw[p] : 1.f;
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if (c < a.C) {
          const size_t i = (size_t)c * a.HW + p;
          const float e = ep[i];
          float v = row[c];
          if (a.v_param) {
            const float z = al * xx[i] + sg * e;
            v = sg * z + al * v;
          }
          const float d = v - e;
          if constexpr (WGT) s = loss_acc_weighted<LOSS>(s, d, m, a.huber_delta);
          else s += loss_term<LOSS>(d, a.huber_delta);
        }
    }
  } else
  for (size_t i = t; i < CHW; i += 256) {
    const int c = (int)(i / a.HW), p = (int)(i - (size_t)c * a.HW);
    size_t pi;
    if (a.patch > 1) {
      const int y = p / a.W, xw = p - y * a.W, pp = a.patch;
      pi = ((size_t)(y / pp) * (a.W / pp) + xw / pp) * a.ld + (size_t)((y % pp) * pp + xw % pp) * a.C + c;
    } else {
      pi = (size_t)p * a.ld + c;
    }
    float pv = pr[pi];
    const float e = ep[i];
    if (a.v_param) {
      const float z = al * xx[i] + sg * e;
      pv = sg * z + al * pv;
    }
    const float d = pv - e;
    if constexpr (WGT) s = loss_acc_weighted<LOSS>(s, d, pw ? pw[p] : 1.f, a.huber_delta);
    else s += loss_term<LOSS>(d, a.huber_delta);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((t & 63) == 0) part[t >> 6] = s;
  __syncthreads();
  if (t == 0) {
    const float tot = ((part[0] + part[1]) + part[2]) + part[3];
    float r = tot;
    if constexpr (LOSS == DC_LOSS_L2) {
      r = sqrtf(tot);             // reference takes torch.norm(...)**2: sqrt, then square
      r = r * r;
    }
    if constexpr (WGT) r *= trial_weight(a.wt, a.out_index ? a.out_index[u] : u, img);
    a.out[a.out_index ? a.out_index[u] : u] = r;
  }
}

extern "C" int dc_eps_mse(const dc_eps_mse_params* p, dc_stream stream) {
  DC_REQUIRE(p && p->pred && p->eps && p->out, DC_ERR_ARG, "dc_eps_mse: null pointer");
  const int pp = p->patch > 1 ? p->patch : 1;
  DC_REQUIRE(p->n_units > 0 && p->C > 0 && p->H > 0 && p->W > 0 && p->ld >= p->C * pp * pp, DC_ERR_SHAPE, "dc_eps_mse: extents");
  DC_REQUIRE(p->H % pp == 0 && p->W % pp == 0, DC_ERR_SHAPE, "dc_eps_mse: patch=%d does not tile %dx%d", pp, p->H, p->W);
  if (p->v_param) DC_REQUIRE(p->x && p->alpha && p->sigma, DC_ERR_ARG, "dc_eps_mse: v-param needs x/alpha/sigma");
  MseArgs a{p->pred, p->eps, p->x, p->alpha, p->sigma, p->bj_of_unit, p->img_of_bj, p->out_index, p->out,
            p->C, p->H * p->W, p->ld, p->v_param, p->W, pp, p->huber_delta};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return dc_by_loss(p->loss, p->huber_delta, "dc_eps_mse", [&](auto kind) {
    return dc_by_weights(p, "dc_eps_mse", [&](auto weighted, const LossWeights& wt) {
      constexpr int LOSS = decltype(kind)::value;
      if constexpr (decltype(weighted)::value) {
        const MseWeightedArgs aw{a, wt};
        hipLaunchKernelGGL((eps_mse_kernel<LOSS, true>), dim3(p->n_units), dim3(256), 0, s, aw);
      } else {
        hipLaunchKernelGGL((eps_mse_kernel<LOSS, false>), dim3(p->n_units), dim3(256), 0, s, a);
      }
      return dc_check_launch("dc_eps_mse");
    });
  });
}

// ------------------------------------------------------------------ sampler step ---
// One ancestral DDPM step with classifier-free guidance (reference diffusion_classifier.py:175-208 ddpm_sampler_step and the
// update at :262-266), fused: the guidance mix, the x-prediction, the clip, the posterior mean and the noise add are one pass over
// the image instead of ~14 elementwise torch launches.  Same operation ORDER as the reference's torch expressions and no
// contraction, so every element equals the torch evaluation of the same fp32 scalars bit for bit — (1 + w) included: the caller
// passes one_plus_w = float(1.0 + w), the Python double rounded ONCE as torch does (1.f + (float)w can differ by an ulp).
// What the step kernels share: the latent, the prediction pair and its geometry, the guidance weights, the pass's alpha_t and sigma_t.
struct StepArgs {
  const float* z; const float* pred; float* out;
  int C, HW, W, ld, patch, v_param, n;
  int fs;                 // feature stride of a patch's pixels in pred: C (eps alone), or the learned-range step's fstride
  float w, one_plus_w, alpha_t, sigma_t;
};

// Element i = (b, r) of z -> its feature in image b's conditional rows of the prediction pair; the null rows' lies rows * ld behind
// it, the learned-range step's variance feature C behind it.
__device__ __forceinline__ const float* step_pair(const StepArgs& a, size_t i, size_t CHW, size_t rows, int& b, size_t& r) {
  b = (int)(i / CHW);
  r = i - (size_t)b * CHW;
  const int c = (int)(r / a.HW), p = (int)(r - (size_t)c * a.HW);
  size_t pi;
  if (a.patch > 1) {
    const int y = p / a.W, xw = p - y * a.W, pp = a.patch;
    pi = ((size_t)(y / pp) * (a.W / pp) + xw / pp) * a.ld + (size_t)((y % pp) * pp + xw % pp) * a.fs + c;
  } else {
    pi = (size_t)p * a.ld + c;
  }
  return a.pred + (size_t)(2 * b) * rows * a.ld + pi;                             // image b's conditional rows, then its null rows
}

// Element i = (b, r) of z: the indexing of the prediction pair, the guidance mix and the data prediction (clipped when `clip`) -> x;
// zt = z[i].  One body for every step kernel, so the mean a noise map is solved against is the mean the step adds it to and the
// solvers' x is the ancestral sampler's.  pair: the element's conditional feature, for a kernel that reads more behind it.
__device__ __forceinline__ float step_xpred(const StepArgs& a, size_t i, size_t CHW, size_t rows, bool clip, int& b, size_t& r, float& zt,
                                            const float** pair_out = nullptr) {
#pragma clang fp contract(off)
  const float* pair = step_pair(a, i, CHW, rows, b, r);
  if (pair_out) *pair_out = pair;
  const float pc = pair[0], pu = pair[rows * a.ld];
  zt = a.z[i];
  const float pr = a.one_plus_w * pc - a.w * pu;                                 // pred = (1 + w) * pred - w * u_pred
  float x = a.v_param ? a.alpha_t * zt - a.sigma_t * pr : (zt - a.sigma_t * pr) / a.alpha_t;
  if (clip) x = fminf(fmaxf(x, -1.f), 1.f);
  return x;
}

// Pointer, extent and patch checks, the kernels' common arguments and the grid size, for any of the four param structs.
template <typename P>
static int step_args(const char* who, const P* p, StepArgs& a, unsigned& grid) {
  DC_REQUIRE(p && p->z && p->pred && p->out, DC_ERR_ARG, "%s: null pointer", who);
  const int pp = p->patch > 1 ? p->patch : 1;
  DC_REQUIRE(p->n > 0 && p->C > 0 && p->H > 0 && p->W > 0 && p->ld >= p->C * pp * pp, DC_ERR_SHAPE, "%s: extents", who);
  DC_REQUIRE(p->H % pp == 0 && p->W % pp == 0, DC_ERR_SHAPE, "%s: patch=%d does not tile %dx%d", who, pp, p->H, p->W);
  a = StepArgs{p->z, p->pred, p->out, p->C, p->H * p->W, p->W, p->ld, pp, p->v_param, p->n, p->C, p->w, p->one_plus_w, p->alpha_t,
               p->sigma_t};
  const size_t total = (size_t)p->n * p->C * a.HW;
  grid = (unsigned)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
  return DC_OK;
}

struct DdpmArgs {
  StepArgs s;
  const float* noise;
  float alpha_s, c, sd;
  int noise_div;          // trajectory b adds noise row b / noise_div (dc_ddpm_step: 1, a row per trajectory)
  float k1, k2, log_hi, log_lo;      // DC_STEP_LEARNED_RANGE only (the fixed instance reads none of them)
};

// The learned-range deviation of one element from its variance feature vc (include/dcamd.h dc_ddpm_step_shared): the step and its
// noise map call this one function, so the map divides by the bits the step multiplies with.
__device__ __forceinline__ float learned_sde(float vc, float log_hi, float log_lo) {
#pragma clang fp contract(off)
  const float fr = 0.5f * vc + 0.5f;
  return expf(0.5f * (fr * log_hi + (1.f - fr) * log_lo));
}

// Mean and deviation of element i.  DC_STEP_FIXED: the posterior mean on the clipped data prediction, sde = sd.
// DC_STEP_LEARNED_RANGE: mu = k1 z + k2 x on the unclipped one (solver_step_kernel's first-order update), sde from the conditional
// row's variance feature, C behind its eps feature.
template <int MODE>
__device__ __forceinline__ float ddpm_mean(const DdpmArgs& a, size_t i, size_t CHW, size_t rows, int& b, size_t& r, float& sde) {
#pragma clang fp contract(off)
  float zt;
  if constexpr (MODE == DC_STEP_LEARNED_RANGE) {
    const float* pair;
    const float xp = step_xpred(a.s, i, CHW, rows, false, b, r, zt, &pair);
    sde = learned_sde(pair[a.s.C], a.log_hi, a.log_lo);
    return a.k1 * zt + a.k2 * xp;
  } else {
    const float xp = step_xpred(a.s, i, CHW, rows, true, b, r, zt);
    sde = a.sd;
    return a.alpha_s * (zt * (1.f - a.c) / a.s.alpha_t + a.c * xp);
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void ddpm_step_kernel(const DdpmArgs a) {
#pragma clang fp contract(off)
  const size_t CHW = (size_t)a.s.C * a.s.HW, total = CHW * a.s.n;
  const size_t rows = (size_t)a.s.HW / (a.s.patch * a.s.patch);
  for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    int b;
    size_t r;
    float sde;
    const float mu = ddpm_mean<MODE>(a, i, CHW, rows, b, r, sde);
    if (a.noise) {
      const size_t ni = a.noise_div == 1 ? i : (size_t)(b / a.noise_div) * CHW + r;
      a.s.out[i] = mu + a.noise[ni] * sde;
    } else if constexpr (MODE == DC_STEP_LEARNED_RANGE) {
      a.s.out[i] = mu;                                                           // last pass: the mean, nothing is clipped
    } else {
      a.s.out[i] = fminf(fmaxf(mu, -1.f), 1.f);                                  // last pass: the clipped mean
    }
  }
}

// The noise map of the same step (include/dcamd.h dc_ddpm_noise_map): out = (x_next - mu) / sd on ddpm_step_kernel's mean.  out may be
// x_next's buffer: a thread reads its element before it writes it, and no other thread touches that element.
template <int MODE>
__global__ __launch_bounds__(256) void ddpm_noise_map_kernel(const DdpmArgs a, const float* x_next) {
#pragma clang fp contract(off)
  const size_t CHW = (size_t)a.s.C * a.s.HW, total = CHW * a.s.n;
  const size_t rows = (size_t)a.s.HW / (a.s.patch * a.s.patch);
  for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    int b;
    size_t r;
    float sde;
    const float mu = ddpm_mean<MODE>(a, i, CHW, rows, b, r, sde);
    a.s.out[i] = (x_next[i] - mu) / sde;
  }
}

// The mode block a caller puts behind dc_ddpm_step_shared_params / dc_ddpm_noise_map_params when `v_param` carries DC_STEP_MODE_BLOCK
// (dcamd.h); without the flag nothing behind the struct is read.  dc_ddpm_step_params has no such flag: the fixed step, v_param as ever.
struct StepMode { int32_t mode, fstride; float k1, k2, log_hi, log_lo; };
static StepMode step_mode(const dc_ddpm_step_params*, bool& flagged) { flagged = false; return StepMode{DC_STEP_FIXED, 0, 0.f, 0.f, 0.f, 0.f}; }
template <typename P>
static StepMode step_mode(const P* p, bool& flagged) {
  static_assert(sizeof(P) % 8 == 0, "the mode block lies at sizeof of the struct");
  flagged = (p->v_param & DC_STEP_MODE_BLOCK) != 0;
  if (!flagged) return StepMode{DC_STEP_FIXED, 0, 0.f, 0.f, 0.f, 0.f};
  return *reinterpret_cast<const StepMode*>(reinterpret_cast<const char*>(p) + sizeof(P));
}

// The mode's checks (after step_args) and kernel arguments.  DC_STEP_FIXED reads nothing of the block but `mode`.
static int ddpm_mode_args(const char* who, const StepMode& m, bool flagged, DdpmArgs& a) {
  if (flagged) a.s.v_param &= ~DC_STEP_MODE_BLOCK;                                // the parametrisation next to the flag
  DC_REQUIRE(m.mode == DC_STEP_FIXED || m.mode == DC_STEP_LEARNED_RANGE, DC_ERR_ARG,
             "%s: mode=%d (DC_STEP_FIXED = 0, DC_STEP_LEARNED_RANGE = 1)", who, m.mode);
  a.k1 = a.k2 = a.log_hi = a.log_lo = 0.f;
  if (m.mode == DC_STEP_FIXED) return DC_OK;
  const long long pp = a.s.patch, C2 = 2ll * a.s.C, need = a.s.patch > 1 ? pp * pp * m.fstride : C2;
  DC_REQUIRE(m.fstride >= C2 && a.s.ld >= need, DC_ERR_SHAPE,
             "%s: the learned-range step needs fstride=%d >= 2C=%lld and ld=%d >= %lld (2C features per pixel)", who, m.fstride, C2, a.s.ld, need);
  const float inf = __builtin_huge_valf();
  DC_REQUIRE(m.log_lo > -inf && m.log_lo <= m.log_hi && m.log_hi <= 0.f, DC_ERR_ARG,      // NaN fails the comparisons
             "%s: log_lo=%g and log_hi=%g must be finite with log_lo <= log_hi <= 0", who, (double)m.log_lo, (double)m.log_hi);
  a.s.fs = m.fstride, a.k1 = m.k1, a.k2 = m.k2, a.log_hi = m.log_hi, a.log_lo = m.log_lo;
  return DC_OK;
}

template <typename P>
static int ddpm_step_entry(const char* who, const P* p, int noise_div, dc_stream stream) {
  DdpmArgs a;
  unsigned grid;
  if (const int rc = step_args(who, p, a.s, grid)) return rc;
  DC_REQUIRE(noise_div >= 1 && p->n % noise_div == 0, DC_ERR_ARG, "%s: noise_div=%d must be >= 1 and divide n=%d", who, noise_div, p->n);
  bool flagged;
  const StepMode m = step_mode(p, flagged);
  if (const int rc = ddpm_mode_args(who, m, flagged, a)) return rc;
  a.noise = p->noise, a.alpha_s = p->alpha_s, a.c = p->c, a.sd = p->sd, a.noise_div = noise_div;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (m.mode == DC_STEP_LEARNED_RANGE) hipLaunchKernelGGL(ddpm_step_kernel<DC_STEP_LEARNED_RANGE>, dim3(grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(ddpm_step_kernel<DC_STEP_FIXED>, dim3(grid), dim3(256), 0, s, a);
  return dc_check_launch(who);
}

extern "C" int dc_ddpm_step(const dc_ddpm_step_params* p, dc_stream stream) { return ddpm_step_entry("dc_ddpm_step", p, 1, stream); }

extern "C" int dc_ddpm_step_shared(const dc_ddpm_step_shared_params* p, dc_stream stream) {
  return ddpm_step_entry("dc_ddpm_step_shared", p, p ? p->noise_div : 1, stream);
}

extern "C" int dc_ddpm_noise_map(const dc_ddpm_noise_map_params* p, dc_stream stream) {
  DdpmArgs a;
  unsigned grid;
  if (const int rc = step_args("dc_ddpm_noise_map", p, a.s, grid)) return rc;
  DC_REQUIRE(p->x_next, DC_ERR_ARG, "dc_ddpm_noise_map: null pointer");
  bool flagged;
  const StepMode m = step_mode(p, flagged);
  if (const int rc = ddpm_mode_args("dc_ddpm_noise_map", m, flagged, a)) return rc;
  if (m.mode == DC_STEP_FIXED)
    DC_REQUIRE(p->sd > 0.f && p->sd < __builtin_huge_valf(), DC_ERR_ARG,    // NaN fails both comparisons
               "dc_ddpm_noise_map: sd=%g must be finite and > 0", (double)p->sd);
  a.noise = nullptr, a.alpha_s = p->alpha_s, a.c = p->c, a.sd = p->sd, a.noise_div = 1;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (m.mode == DC_STEP_LEARNED_RANGE)
    hipLaunchKernelGGL(ddpm_noise_map_kernel<DC_STEP_LEARNED_RANGE>, dim3(grid), dim3(256), 0, s, a, p->x_next);
  else
    hipLaunchKernelGGL(ddpm_noise_map_kernel<DC_STEP_FIXED>, dim3(grid), dim3(256), 0, s, a, p->x_next);
  return dc_check_launch("dc_ddpm_noise_map");
}

// ------------------------------------------------------------------ solver step ----
// One pass of a deterministic data-prediction solver on the same prediction pair (include/dcamd.h dc_solver_step): the guidance mix and
// the x-prediction are step_xpred's, then the update z_s = k1 z + k2 D with D = x (DDIM) or x + k3 (x - xprev) (DPM-Solver++ 2M).
// The operation order of the header's expressions, no contraction.  xhat may be xprev's buffer: a thread reads its element of xprev
// before it writes the same element of xhat, and no other thread touches that element.
struct SolverArgs {
  StepArgs s;
  const float* xprev; float* xhat;
  int clamp, final_pass;
  float k1, k2, k3;
};

__global__ __launch_bounds__(256) void solver_step_kernel(const SolverArgs a) {
#pragma clang fp contract(off)
  const size_t CHW = (size_t)a.s.C * a.s.HW, total = CHW * a.s.n;
  const size_t rows = (size_t)a.s.HW / (a.s.patch * a.s.patch);
  for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    int b;
    size_t r;
    float zt;
    const float x = step_xpred(a.s, i, CHW, rows, a.clamp, b, r, zt);
    float D = x;
    if (a.xprev) D = x + a.k3 * (x - a.xprev[i]);                                // read before the write below: xhat may be xprev
    if (a.xhat) a.xhat[i] = x;
    a.s.out[i] = a.final_pass ? fminf(fmaxf(D, -1.f), 1.f) : a.k1 * zt + a.k2 * D;
  }
}

extern "C" int dc_solver_step(const dc_solver_step_params* p, dc_stream stream) {
  SolverArgs a;
  unsigned grid;
  if (const int rc = step_args("dc_solver_step", p, a.s, grid)) return rc;
  DC_REQUIRE(p->out != p->z, DC_ERR_ARG, "dc_solver_step: out must not alias z");
  a.xprev = p->xprev, a.xhat = p->xhat, a.clamp = p->clamp, a.final_pass = p->final_pass, a.k1 = p->k1, a.k2 = p->k2, a.k3 = p->k3;
  hipLaunchKernelGGL(solver_step_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return dc_check_launch("dc_solver_step");
}

// ------------------------------------------------------------------ difference maps -
// One lane per output pixel: the C planes of a and of its reference row are read coalesced across the wave, summed in channel order.
__global__ __launch_bounds__(256) void abs_diff_map_kernel(const float* __restrict__ a, const float* __restrict__ r,
                                                           const int32_t* __restrict__ r_of_a, float* __restrict__ out,
                                                           long long total, int m, int C, int HW) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long u = i / HW;
    const int p = (int)(i - u * HW);
    const int ru = r_of_a[u];
    float s = __builtin_nanf("");
    if ((unsigned)ru < (unsigned)m) {
      const float* pa = a + (size_t)u * C * HW + p;
      const float* pr = r + (size_t)ru * C * HW + p;
      s = 0.f;
      for (int c = 0; c < C; ++c) s += fabsf(pa[(size_t)c * HW] - pr[(size_t)c * HW]);
    }
    out[i] = s;
  }
}

extern "C" int dc_abs_diff_map(const dc_abs_diff_map_params* p, dc_stream stream) {
  DC_REQUIRE(p && p->a && p->r && p->r_of_a && p->out, DC_ERR_ARG, "dc_abs_diff_map: null pointer");
  DC_REQUIRE(p->n > 0 && p->m > 0 && p->C > 0 && p->H > 0 && p->W > 0, DC_ERR_SHAPE, "dc_abs_diff_map: extents n=%d m=%d C=%d H=%d W=%d",
             p->n, p->m, p->C, p->H, p->W);
  const long long total = (long long)p->n * p->H * p->W;
  const unsigned grid = (unsigned)((total + 255) / 256 > 16384 ? 16384 : (total + 255) / 256);
  hipLaunchKernelGGL(abs_diff_map_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p->a, p->r, p->r_of_a,
                     p->out, total, p->m, p->C, p->H * p->W);
  return dc_check_launch("dc_abs_diff_map");
}

// ------------------------------------------------------------------ Haar -----------
// One lane per 2x2 input block: reads two float2 (rows 2y, 2y+1), writes the four sub-bands.
__global__ __launch_bounds__(256) void haar_dwt2_kernel(const float* in, float* out, long long total, int C, int H, int W, float scale) {
  const int h = H / 2, w = W / 2;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int xw = (int)(i % w); long long r = i / w;
    const int y = (int)(r % h); r /= h;
    const int c = (int)(r % C); const long long n = r / C;
    const float* src = in + ((n * C + c) * H + 2 * y) * (long long)W + 2 * xw;
    const float2 r0 = *reinterpret_cast<const float2*>(src), r1 = *reinterpret_cast<const float2*>(src + W);
    const float A = r0.x, B = r0.y, Cc = r1.x, D = r1.y;
    float* dst = out + ((n * 4 * C + 4 * c) * h + y) * (long long)w + xw;
    const long long hw = (long long)h * w;
    const float k = 0.5f * scale;
    dst[0] = (A + B + Cc + D) * k;
    dst[hw] = (A + B - Cc - D) * k;
    dst[2 * hw] = (A - B + Cc - D) * k;
    dst[3 * hw] = (A - B - Cc + D) * k;
  }
}
__global__ __launch_bounds__(256) void haar_idwt2_kernel(const float* in, float* out, long long total, int C, int h, int w, float scale) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int xw = (int)(i % w); long long r = i / w;
    const int y = (int)(r % h); r /= h;
    const int c = (int)(r % C); const long long n = r / C;
    const long long hw = (long long)h * w;
    const float* src = in + ((n * 4 * C + 4 * c) * h + y) * (long long)w + xw;
    const float cA = src[0], cH = src[hw], cV = src[2 * hw], cD = src[3 * hw];
    const float k = 0.5f * scale;
    float* dst = out + ((n * C + c) * 2 * h + 2 * y) * (long long)(2 * w) + 2 * xw;
    *reinterpret_cast<float2*>(dst) = make_float2((cA + cH + cV + cD) * k, (cA + cH - cV - cD) * k);
    *reinterpret_cast<float2*>(dst + 2 * w) = make_float2((cA - cH + cV - cD) * k, (cA - cH - cV + cD) * k);
  }
}

typedef float hv4 __attribute__((ext_vector_type(4)));     // native vector: what the nontemporal builtins take
__device__ __forceinline__ hv4 hv4_make(float a, float b, float c, float d) { hv4 v = {a, b, c, d}; return v; }
// Wide forms (W a multiple of 8, 16-byte aligned tensors): a lane owns 4 adjacent output pixels of one subband row — two
// 16-byte loads from each of the two source rows (a wave reads 2 x 2 KiB contiguous), one 16-byte store per subband
// (a wave writes 4 x 1 KiB contiguous).  Pure streaming: 8 bytes moved per input value, HBM-bound.
__global__ __launch_bounds__(256) void haar_dwt2_v4_kernel(const float* __restrict__ in, float* __restrict__ out, long long total4,
                                                           int C, int H, int W, float scale) {
  const int h = H / 2, w4 = W / 8;
  const long long hw = (long long)h * (W / 2);
  const float k = 0.5f * scale;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
    const int xq = (int)(i % w4); long long r = i / w4;
    const int y = (int)(r % h); r /= h;                         // r = n * C + c
    const float* src = in + (r * H + 2 * y) * (long long)W + 8 * xq;
    const hv4 a0 = __builtin_nontemporal_load(reinterpret_cast<const hv4*>(src));
    const hv4 a1 = __builtin_nontemporal_load(reinterpret_cast<const hv4*>(src) + 1);
    const hv4 b0 = __builtin_nontemporal_load(reinterpret_cast<const hv4*>(src + W));
    const hv4 b1 = __builtin_nontemporal_load(reinterpret_cast<const hv4*>(src + W) + 1);
    const float A[4] = {a0.x, a0.z, a1.x, a1.z}, B[4] = {a0.y, a0.w, a1.y, a1.w};
    const float Cc[4] = {b0.x, b0.z, b1.x, b1.z}, D[4] = {b0.y, b0.w, b1.y, b1.w};
    float o[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[0][j] = (A[j] + B[j] + Cc[j] + D[j]) * k;
      o[1][j] = (A[j] + B[j] - Cc[j] - D[j]) * k;
      o[2][j] = (A[j] - B[j] + Cc[j] - D[j]) * k;
      o[3][j] = (A[j] - B[j] - Cc[j] + D[j]) * k;
    }
    const long long c = r % C, n = r / C;
    float* dst = out + ((n * 4 * C + 4 * c) * h + y) * (long long)(W / 2) + 4 * xq;
#pragma unroll
    for (int sb = 0; sb < 4; ++sb)
      __builtin_nontemporal_store(hv4_make(o[sb][0], o[sb][1], o[sb][2], o[sb][3]), reinterpret_cast<hv4*>(dst + sb * hw));
  }
}
__global__ __launch_bounds__(256) void haar_idwt2_v4_kernel(const float* __restrict__ in, float* __restrict__ out, long long total4,
                                                            int C, int h, int w, float scale) {
  const int w4 = w / 4;
  const long long hw = (long long)h * w;
  const float k = 0.5f * scale;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
    const int xq = (int)(i % w4); long long r = i / w4;
    const int y = (int)(r % h); r /= h;
    const long long c = r % C, n = r / C;
    const float* src = in + ((n * 4 * C + 4 * c) * h + y) * (long long)w + 4 * xq;
    const hv4 cA = __builtin_nontemporal_load(reinterpret_cast<const hv4*>(src));
    const hv4 cH = __builtin_nontemporal_load(reinterpret_cast<const hv4*>(src + hw));
    const hv4 cV = __builtin_nontemporal_load(reinterpret_cast<const hv4*>(src + 2 * hw));
    const hv4 cD = __builtin_nontemporal_load(reinterpret_cast<const hv4*>(src + 3 * hw));
    const float a[4] = {cA.x, cA.y, cA.z, cA.w}, hh[4] = {cH.x, cH.y, cH.z, cH.w};
    const float v[4] = {cV.x, cV.y, cV.z, cV.w}, d[4] = {cD.x, cD.y, cD.z, cD.w};
    float t[8], b[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      t[2 * j] = (a[j] + hh[j] + v[j] + d[j]) * k;  t[2 * j + 1] = (a[j] + hh[j] - v[j] - d[j]) * k;
      b[2 * j] = (a[j] - hh[j] + v[j] - d[j]) * k;  b[2 * j + 1] = (a[j] - hh[j] - v[j] + d[j]) * k;
    }
    float* dst = out + (r * 2 * h + 2 * y) * (long long)(2 * w) + 8 * xq;
    __builtin_nontemporal_store(hv4_make(t[0], t[1], t[2], t[3]), reinterpret_cast<hv4*>(dst));
    __builtin_nontemporal_store(hv4_make(t[4], t[5], t[6], t[7]), reinterpret_cast<hv4*>(dst) + 1);
    __builtin_nontemporal_store(hv4_make(b[0], b[1], b[2], b[3]), reinterpret_cast<hv4*>(dst + 2 * w));
    __builtin_nontemporal_store(hv4_make(b[4], b[5], b[6], b[7]), reinterpret_cast<hv4*>(dst + 2 * w) + 1);
  }
}

static unsigned haar_grid(long long items) {
  const long long b = (items + 255) / 256;
  return (unsigned)(b > 65536 ? 65536 : b);
}

extern "C" int dc_haar_dwt2(const float* in, float* out, int32_t n, int32_t C, int32_t H, int32_t W, float scale, dc_stream stream) {
  DC_REQUIRE(in && out && n > 0 && C > 0 && H > 0 && W > 0, DC_ERR_ARG, "dc_haar_dwt2: bad args");
  DC_REQUIRE(H % 2 == 0 && W % 2 == 0, DC_ERR_SHAPE, "dc_haar_dwt2: H=%d W=%d must be even", H, W);
  DC_REQUIRE(((uintptr_t)in & 7) == 0, DC_ERR_ALIGN, "dc_haar_dwt2: input must be 8-byte aligned");
  const long long total = (long long)n * C * (H / 2) * (W / 2);
  if (W % 8 == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0) {
    hipLaunchKernelGGL(haar_dwt2_v4_kernel, dim3(haar_grid(total / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), in, out,
                       total / 4, C, H, W, scale);
    return dc_check_launch("dc_haar_dwt2");
  }
  const unsigned grid = (unsigned)((total + 255) / 256 > 16384 ? 16384 : (total + 255) / 256);
  hipLaunchKernelGGL(haar_dwt2_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), in, out, total, C, H, W, scale);
  return dc_check_launch("dc_haar_dwt2");
}
extern "C" int dc_haar_idwt2(const float* in, float* out, int32_t n, int32_t C, int32_t h, int32_t w, float scale, dc_stream stream) {
  DC_REQUIRE(in && out && n > 0 && C > 0 && h > 0 && w > 0, DC_ERR_ARG, "dc_haar_idwt2: bad args");
  DC_REQUIRE(((uintptr_t)out & 7) == 0, DC_ERR_ALIGN, "dc_haar_idwt2: output must be 8-byte aligned");
  const long long total = (long long)n * C * h * w;
  if (w % 4 == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0) {
    hipLaunchKernelGGL(haar_idwt2_v4_kernel, dim3(haar_grid(total / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), in, out,
                       total / 4, C, h, w, scale);
    return dc_check_launch("dc_haar_idwt2");
  }
  const unsigned grid = (unsigned)((total + 255) / 256 > 16384 ? 16384 : (total + 255) / 256);
  hipLaunchKernelGGL(haar_idwt2_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), in, out, total, C, h, w, scale);
  return dc_check_launch("dc_haar_idwt2");
}

// ------------------------------------------------------------------ im2col, stride 2 -
// out[i, oy, ox, (ky 3 + kx) C + c] = x[i, 2 oy + ky, 2 ox + kx, c], zero where 2 oy + ky >= H or 2 ox + kx >= W: the A operand of a
// stride-2 3x3 conv padded at the bottom and right only (AutoencoderKL's downsampler, F.pad(x, (0, 1, 0, 1)) in front of a stride-2 conv
// without padding) as a 1x1 GEMM over K = 9 C.  A pure move: one lane per unit U of the output (16 bytes where x, out, C and ld allow
// it, else one element), consecutive lanes on consecutive output units.  Cu / ldu: C and the row stride of x in units.
template <typename U>
__global__ __launch_bounds__(256) void im2col_s2_kernel(const U* __restrict__ x, U* __restrict__ out, long long total, int H, int W, int Cu, int ldu) {
  const int Ho = H / 2, Wo = W / 2;
  for (long long idx = blockIdx.x * 256LL + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int c = (int)(idx % Cu); long long r = idx / Cu;
    const int tap = (int)(r % 9); r /= 9;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const long long i = r / Ho;
    const int iy = 2 * oy + tap / 3, ix = 2 * ox + tap % 3;
    U v = {};
    if (iy < H && ix < W) v = x[((i * H + iy) * W + ix) * ldu + c];
    out[idx] = v;
  }
}

extern "C" int dc_im2col_s2(const dc_im2col_s2_params* p, dc_stream stream) {
  DC_REQUIRE(p && p->x && p->out, DC_ERR_ARG, "dc_im2col_s2: null pointer");
  DC_REQUIRE(p->dtype == DC_F32 || p->dtype == DC_BF16 || p->dtype == DC_F16, DC_ERR_DTYPE, "dc_im2col_s2: dtype %d", p->dtype);
  DC_REQUIRE(p->n > 0 && p->C > 0 && p->H > 0 && p->W > 0, DC_ERR_SHAPE, "dc_im2col_s2: extents n=%d C=%d H=%d W=%d", p->n, p->C, p->H, p->W);
  DC_REQUIRE(p->H % 2 == 0 && p->W % 2 == 0, DC_ERR_SHAPE, "dc_im2col_s2: H=%d W=%d must be even", p->H, p->W);
  DC_REQUIRE(p->ld >= p->C, DC_ERR_SHAPE, "dc_im2col_s2: ld=%d < C=%d", p->ld, p->C);
  const int es = dc_dtype_size(p->dtype), epc = 16 / es;
  DC_REQUIRE((((uintptr_t)p->x | (uintptr_t)p->out) & (uintptr_t)(es - 1)) == 0, DC_ERR_ALIGN, "dc_im2col_s2: x/out must be element aligned");
  const long long elems = (long long)p->n * (p->H / 2) * (p->W / 2) * 9 * p->C;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  auto grid = [](long long items) { const long long b = (items + 255) / 256; return (unsigned)(b > 65536 ? 65536 : b); };
  if (p->C % epc == 0 && p->ld % epc == 0 && (((uintptr_t)p->x | (uintptr_t)p->out) & 15) == 0) {
    hipLaunchKernelGGL(im2col_s2_kernel<chunk16>, dim3(grid(elems / epc)), dim3(256), 0, s, reinterpret_cast<const chunk16*>(p->x),
                       reinterpret_cast<chunk16*>(p->out), elems / epc, p->H, p->W, p->C / epc, p->ld / epc);
  } else if (es == 4) {
    hipLaunchKernelGGL(im2col_s2_kernel<uint32_t>, dim3(grid(elems)), dim3(256), 0, s, reinterpret_cast<const uint32_t*>(p->x),
                       reinterpret_cast<uint32_t*>(p->out), elems, p->H, p->W, p->C, p->ld);
  } else {
    hipLaunchKernelGGL(im2col_s2_kernel<uint16_t>, dim3(grid(elems)), dim3(256), 0, s, reinterpret_cast<const uint16_t*>(p->x),
                       reinterpret_cast<uint16_t*>(p->out), elems, p->H, p->W, p->C, p->ld);
  }
  return dc_check_launch("dc_im2col_s2");
}

// ------------------------------------------------------------------ latent im2col ----
// The head of the AutoencoderKL decoder (include/dcamd.h dc_latent_im2col): per pixel u = Q (z inv_scale + shift) + bias in fp32, channels
// ascending and no contraction, written as the 3x3 patches of u in dc_qsample's im2col column order (tap * Z + c), zero for taps outside
// the image and for the columns [9 Z, Kpad).  One lane per 16-byte chunk of the output, consecutive lanes on consecutive chunks; z is read
// inside the image only.  Kpad is a multiple of the K granule, so every row is whole chunks and every store is 16 bytes.
struct LatentArgs {
  const float* z; const float* Q; const float* bias; void* out;
  int n, Z, H, W, Kpad;
  float inv_scale, shift;
};

template <typename TO>
__global__ __launch_bounds__(256) void latent_im2col_kernel(const LatentArgs a) {
#pragma clang fp contract(off)
  constexpr int EPC = Elem<TO>::EPC;
  const int cpr = a.Kpad / EPC;
  const int HW = a.H * a.W;
  const long long total = (long long)a.n * HW * cpr;
  for (long long idx = blockIdx.x * 256LL + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int ch = (int)(idx % cpr);
    const long long row = idx / cpr;
    const int p = (int)(row % HW);
    const long long i = row / HW;
    const int y = p / a.W, xw = p - y * a.W;
    const float* zi = a.z + (size_t)i * a.Z * HW;
    float f[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      const int k = ch * EPC + e;
      float v = 0.f;
      if (k < 9 * a.Z) {
        const int tap = k / a.Z, c = k - tap * a.Z;
        const int iy = y + tap / 3 - 1, ix = xw + tap % 3 - 1;
        if ((unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W) {
          const float* zp = zi + (size_t)iy * a.W + ix;
          const float* q = a.Q + (size_t)c * a.Z;
          float s = 0.f;
          for (int j = 0; j < a.Z; ++j) s += q[j] * (zp[(size_t)j * HW] * a.inv_scale + a.shift);
          v = s + a.bias[c];
        }
      }
      f[e] = v;
    }
    reinterpret_cast<chunk16*>(a.out)[idx] = f_to_chunk<TO>(f);
  }
}

extern "C" int dc_latent_im2col(const dc_latent_im2col_params* p, dc_stream stream) {
  DC_REQUIRE(p && p->z && p->Q && p->bias && p->out, DC_ERR_ARG, "dc_latent_im2col: null pointer");
  DC_REQUIRE(p->out_dtype == DC_F32 || p->out_dtype == DC_BF16 || p->out_dtype == DC_F16, DC_ERR_DTYPE, "dc_latent_im2col: out_dtype %d", p->out_dtype);
  DC_REQUIRE(p->n > 0 && p->Z >= 1 && p->H > 0 && p->W > 0, DC_ERR_SHAPE, "dc_latent_im2col: extents n=%d Z=%d H=%d W=%d", p->n, p->Z, p->H, p->W);
  const int granule = 128 / dc_dtype_size(p->out_dtype);      // the K granule of dc_igemm: one 128-byte LDS row
  DC_REQUIRE(p->Z <= 0x7fffffff / 9 && p->Kpad >= 9 * p->Z && p->Kpad % granule == 0, DC_ERR_SHAPE,
             "dc_latent_im2col: Kpad=%d (need >= 9 Z = %lld, a multiple of %d)", p->Kpad, 9LL * p->Z, granule);
  DC_REQUIRE((((uintptr_t)p->z | (uintptr_t)p->Q | (uintptr_t)p->bias) & 3) == 0 && ((uintptr_t)p->out & 15) == 0, DC_ERR_ALIGN,
             "dc_latent_im2col: z / Q / bias must be 4-byte aligned, out 16-byte aligned");
  LatentArgs a{p->z, p->Q, p->bias, p->out, p->n, p->Z, p->H, p->W, p->Kpad, p->inv_scale, p->shift};
  const int epc = 16 / dc_dtype_size(p->out_dtype);
  const long long total = (long long)p->n * p->H * p->W * (p->Kpad / epc);
  const unsigned grid = (unsigned)((total + 255) / 256 > 65536 ? 65536 : (total + 255) / 256);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return dc_by_dtype(p->out_dtype, "dc_latent_im2col: out_dtype", [&](auto t) {
    hipLaunchKernelGGL((latent_im2col_kernel<decltype(t)>), dim3(grid), dim3(256), 0, s, a);
    return dc_check_launch("dc_latent_im2col");
  });
}

// ------------------------------------------------------------------------------------------------------------------
// Second launch of the tail fold (epi_pn.h): every tile of the last ResNet conv wrote the thin conv's sums of its OWN pixels (+ bias) into
// pred and its sums for the positions just around it into its ring slots (conv3_halo.h).  A pixel on a tile's border also gets what the
// (at most three) neighbouring tiles hold for it: added here in ascending tile index, one lane per (sample, tile, border pixel), so the
// result is the same bits at every launch.  Stream order is the only synchronisation between the two kernels.
#include "conv3_halo.h"
__global__ __launch_bounds__(256) void pn_tail_combine_kernel(float* pred, const float* ring, int total, int ltw, int lth, int tiles_x, int tiles_y,
                                                              int H, int W, int Co, int ld) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int tw = 1 << ltw, th = 1 << lth, tiles = tiles_x * tiles_y;
  const int nb = 2 * tw + 2 * (th - 2);                     // border pixels of a tile: its first and last row, then the two outer columns between
  const int b = idx % nb, rest = idx / nb, tile = rest % tiles, n = rest / tiles;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  int py, px;
  if (b < 2 * tw) { py = b < tw ? 0 : th - 1; px = b & (tw - 1); }
  else { const int c = b - 2 * tw; py = 1 + (c >> 1); px = (c & 1) ? tw - 1 : 0; }
  const int gy = ty * th + py, gx = tx * tw + px;
  float s[3] = {0.f, 0.f, 0.f};
  float* o = pred + ((size_t)n * H * W + (size_t)gy * W + gx) * ld;
  bool any = false;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      if (!dy && !dx) continue;
      const int ny = ty + dy, nx = tx + dx;
      if ((unsigned)ny >= (unsigned)tiles_y || (unsigned)nx >= (unsigned)tiles_x) continue;
      // the pixel in the neighbour's coordinates: inside its one-pixel surround?
      const int oy = gy - ny * th, ox = gx - nx * tw;
      if (oy < -1 || oy > th || ox < -1 || ox > tw) continue;
      const float* r = ring + (((size_t)n * tiles + ny * tiles_x + nx) * PN_TAIL_RING(tw, th) + pn_tail_ring_slot(oy, ox, tw, th)) * Co;
      if (!any) { for (int co = 0; co < 3; ++co) if (co < Co) s[co] = o[co]; any = true; }
      for (int co = 0; co < 3; ++co) if (co < Co) s[co] += r[co];
    }
  if (any)
    for (int co = 0; co < 3; ++co) if (co < Co) o[co] = s[co];
}

int dc_pn_tail_combine_launch(float* pred, const float* ring, int n_img, int ltw, int lth, int tiles_x, int tiles_y, int H, int W, int Co, int ld,
                              hipStream_t s) {
  if (tiles_x * tiles_y == 1) return DC_OK;                 // a sample that is one tile has no neighbour: pred is final
  const int tw = 1 << ltw, th = 1 << lth;
  const long long total = (long long)n_img * tiles_x * tiles_y * (2 * tw + 2 * (th - 2));
  if (total <= 0 || total > 0x7fffffffLL) { dc_set_error("dc_conv3_pn_tail: bad combine extent %lld", total); return DC_ERR_SHAPE; }
  hipLaunchKernelGGL(pn_tail_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, pred, ring, (int)total, ltw, lth, tiles_x, tiles_y,
                     H, W, Co, ld);
  return dc_check_launch("dc_conv3_pn_tail(combine)");
}
