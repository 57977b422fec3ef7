// evidence.hip — per-pixel class evidence from the scoring loop (include/dcamd.h "class evidence maps").
// dc_err_map: per (unit, pixel) the channel sum of the scoring loss's term ((eps_hat - eps)^2 for l2), quantised to fixed point and added to the cell's int64 plane.
// Integer adds are associative, so the result does not depend on arrival order, launch shape or how the grid was cut.
// dc_evidence_maps: the per-stage planes -> mean map, paired difference map to the winner, invalid counts.
#include <math.h>
#include "common.h"

// ------------------------------------------------------------------ error map ------
struct ErrMapArgs {
  const float* pred; const float* eps; const float* x; const float* alpha; const float* sigma;
  const int32_t* bj_of_unit; const int32_t* img_of_bj; const int32_t* out_index;
  unsigned long long* acc; int32_t* bad;
  int C, HW, ld, v_param, W, patch, T, cells, nblk;
  float huber_delta;       // read by the DC_LOSS_HUBER instance only
};
struct ErrMapWeightedArgs : ErrMapArgs { LossWeights wt; };      // the weighted instances' argument: the unweighted ones keep theirs

// One workgroup per (unit, 256 consecutive pixels); a lane owns one pixel and walks its channels in ascending order, so the C reads of
// an NHWC prediction row are back to back, the planes of eps / x are read coalesced across the wave, and a wave's 64 adds are one
// 512-byte run of the cell's plane.  LOSS: the per-element term (common.h loss_term), dc_eps_mse's, a compile-time kind.
// WGT: the loss weights (dcamd.h dc_err_map_params), compile-time too: v = ((channel sum) m[y, x]) w behind the unchanged channel loop.
template <int LOSS, bool WGT>
__global__ __launch_bounds__(256) void err_map_kernel(const std::conditional_t<WGT, ErrMapWeightedArgs, ErrMapArgs> a) {
  const int u = blockIdx.x / a.nblk;
  const int p = (blockIdx.x - u * a.nblk) * 256 + threadIdx.x;
  if (p >= a.HW) return;
  const int bj = a.bj_of_unit ? a.bj_of_unit[u] : u;
  const int img = a.img_of_bj ? a.img_of_bj[bj] : bj;
  const float al = a.alpha ? a.alpha[bj] : 1.f, sg = a.sigma ? a.sigma[bj] : 0.f;
  const long long oi = a.out_index ? a.out_index[u] : u;
  const long long cell = (oi >= 0 && oi < (long long)a.cells * a.T) ? oi / a.T : a.cells;      // anything else: the dump plane
  const size_t CHW = (size_t)a.C * a.HW;
  const float* pr = a.pred + (size_t)u * (a.patch > 1 ? a.HW / (a.patch * a.patch) : a.HW) * a.ld;
  const float* ep = a.eps + (size_t)bj * CHW;
  const float* xx = a.x ? a.x + (size_t)img * CHW : nullptr;
  size_t pi;                                       // channel 0 of this pixel in the prediction (dc_eps_mse's indexing)
  if (a.patch > 1) {
    const int y = p / a.W, xw = p - y * a.W, pp = a.patch;
    pi = ((size_t)(y / pp) * (a.W / pp) + xw / pp) * a.ld + (size_t)((y % pp) * pp + xw % pp) * a.C;
  } else {
    pi = (size_t)p * a.ld;
  }
  float v = 0.f;
  for (int c = 0; c < a.C; ++c) {
    const size_t i = (size_t)c * a.HW + p;
    const float e = ep[i];
    float pv = pr[pi + c];
    if (a.v_param) {
      const float z = al * xx[i] + sg * e;
      pv = sg * z + al * pv;
    }
    const float d = pv - e;
    v += loss_term<LOSS>(d, a.huber_delta);
  }
  if constexpr (WGT) {
    if (a.wt.pixel_w) v *= a.wt.pixel_w[(size_t)img * a.HW + p];
    v *= trial_weight(a.wt, oi, img);
  }
  if (v >= 0.f && v <= DC_EVIDENCE_VMAX) {         // false for NaN
    const long long q = (long long)rint((double)v * (double)(1ll << DC_EVIDENCE_FRAC_BITS));
    atomicAdd(a.acc + (size_t)cell * a.HW + p, (unsigned long long)q);
  } else {
    atomicAdd(a.bad + cell, 1);
  }
}

extern "C" int dc_err_map(const dc_err_map_params* p, dc_stream stream) {
  DC_REQUIRE(p && p->pred && p->eps && p->acc && p->bad, DC_ERR_ARG, "dc_err_map: null pointer");
  const int pp = p->patch > 1 ? p->patch : 1;
  DC_REQUIRE(p->n_units > 0 && p->C > 0 && p->H > 0 && p->W > 0 && p->ld >= p->C * pp * pp, DC_ERR_SHAPE, "dc_err_map: extents");
  DC_REQUIRE(p->H % pp == 0 && p->W % pp == 0, DC_ERR_SHAPE, "dc_err_map: patch=%d does not tile %dx%d", pp, p->H, p->W);
  DC_REQUIRE(p->T > 0 && p->cells > 0, DC_ERR_SHAPE, "dc_err_map: T=%d cells=%d", p->T, p->cells);
  DC_REQUIRE((long long)p->H * p->W <= (1ll << 24), DC_ERR_SHAPE, "dc_err_map: %dx%d pixels", p->H, p->W);
  if (p->v_param) DC_REQUIRE(p->x && p->alpha && p->sigma, DC_ERR_ARG, "dc_err_map: v-param needs x/alpha/sigma");
  const int HW = p->H * p->W, nblk = (HW + 255) / 256;
  DC_REQUIRE((long long)p->n_units * nblk < (1ll << 31), DC_ERR_SHAPE, "dc_err_map: %d units x %d pixel blocks", p->n_units, nblk);
  ErrMapArgs a{p->pred, p->eps, p->x, p->alpha, p->sigma, p->bj_of_unit, p->img_of_bj, p->out_index,
               reinterpret_cast<unsigned long long*>(p->acc), p->bad, p->C, HW, p->ld, p->v_param, p->W, pp, p->T, p->cells, nblk,
               p->huber_delta};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return dc_by_loss(p->loss, p->huber_delta, "dc_err_map", [&](auto kind) {
    return dc_by_weights(p, "dc_err_map", [&](auto weighted, const LossWeights& wt) {
      constexpr int LOSS = decltype(kind)::value;
      const dim3 grid((unsigned)(p->n_units * nblk));
      if constexpr (decltype(weighted)::value) {
        const ErrMapWeightedArgs aw{a, wt};
        hipLaunchKernelGGL((err_map_kernel<LOSS, true>), grid, dim3(256), 0, s, aw);
      } else {
        hipLaunchKernelGGL((err_map_kernel<LOSS, false>), grid, dim3(256), 0, s, a);
      }
      return dc_check_launch("dc_err_map");
    });
  });
}

// ------------------------------------------------------------------ evidence maps --
struct EvMapsArgs {
  const long long* acc; const int32_t* bad; const int32_t* stage_ends; const int32_t* n_eval; const int32_t* winner;
  float* mean_map; float* delta_map; int32_t* invalid;
  int n_stages, BS, C, HW, nblk;
};

// stages class (b, c) was scored on: n = 0 -> 0; n = stage_ends[s] -> s + 1; anything else -> -1
static __device__ inline int stages_of(const int32_t* ends, int n_stages, int n) {
  if (n == 0) return 0;
  for (int s = 0; s < n_stages; ++s)
    if (ends[s] == n) return s + 1;
  return -1;
}

__global__ __launch_bounds__(256) void evidence_maps_kernel(const EvMapsArgs a) {
  __shared__ int part[4];
  const int cell = blockIdx.x / a.nblk, blk = blockIdx.x - cell * a.nblk;
  const int b = cell / a.C, c = cell - b * a.C;
  const size_t plane = (size_t)a.HW, slab = (size_t)(a.BS * a.C + 1) * plane;
  const int nbad_stride = a.BS * a.C + 1;
  if (blk == 0 && c == 0) {            // invalid[b]: the bad counts of the image's scored cells (integer sum: any order)
    int s_ = 0;
    for (int cc = threadIdx.x; cc < a.C; cc += 256) {
      const int sc = stages_of(a.stage_ends, a.n_stages, a.n_eval[b * a.C + cc]);
      for (int s = 0; s < sc; ++s) s_ += a.bad[s * nbad_stride + b * a.C + cc];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s_ += __shfl_xor(s_, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s_;
    __syncthreads();
    if (threadIdx.x == 0) a.invalid[b] = part[0] + part[1] + part[2] + part[3];
  }
  const int p = blk * 256 + threadIdx.x;
  if (p >= a.HW) return;
  const int n = a.n_eval[cell];
  const int sc = stages_of(a.stage_ends, a.n_stages, n);
  const int w = a.winner[b];
  bool ok = sc > 0 && w >= 0 && w < a.C;
  for (int s = 0; ok && s < sc; ++s) ok = a.bad[s * nbad_stride + cell] == 0;
  float mean = __builtin_nanf(""), delta = __builtin_nanf("");
  if (ok) {
    long long sm = 0, sd = 0;
    for (int s = 0; s < sc; ++s) {
      const long long qc = a.acc[s * slab + (size_t)cell * plane + p];
      const long long qw = a.acc[s * slab + (size_t)(b * a.C + w) * plane + p];
      sm += qc;
      sd += qc - qw;
    }
    const double sc2 = 1.0 / (double)(1ll << DC_EVIDENCE_FRAC_BITS);
    mean = (float)(((double)sm * sc2) / (double)n);
    delta = (float)(((double)sd * sc2) / (double)n);
  }
  a.mean_map[(size_t)cell * plane + p] = mean;
  a.delta_map[(size_t)cell * plane + p] = delta;
}

extern "C" int dc_evidence_maps(const dc_evidence_maps_params* p, dc_stream stream) {
  DC_REQUIRE(p && p->acc && p->bad && p->stage_ends && p->n_eval && p->winner && p->mean_map && p->delta_map && p->invalid,
             DC_ERR_ARG, "dc_evidence_maps: null pointer");
  DC_REQUIRE(p->n_stages >= 1 && p->n_stages <= 64, DC_ERR_SHAPE, "dc_evidence_maps: n_stages=%d outside [1, 64]", p->n_stages);
  DC_REQUIRE(p->BS > 0 && p->C > 0 && p->HW > 0 && p->HW <= (1 << 24), DC_ERR_SHAPE, "dc_evidence_maps: extents");
  const int nblk = (p->HW + 255) / 256;
  DC_REQUIRE((long long)p->BS * p->C * nblk < (1ll << 31), DC_ERR_SHAPE, "dc_evidence_maps: %d cells x %d pixel blocks", p->BS * p->C, nblk);
  EvMapsArgs a{reinterpret_cast<const long long*>(p->acc), p->bad, p->stage_ends, p->n_eval, p->winner, p->mean_map, p->delta_map,
               p->invalid, p->n_stages, p->BS, p->C, p->HW, nblk};
  hipLaunchKernelGGL(evidence_maps_kernel, dim3((unsigned)(p->BS * p->C * nblk)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return dc_check_launch("dc_evidence_maps");
}
