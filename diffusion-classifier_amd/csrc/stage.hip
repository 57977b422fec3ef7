// stage.hip — the stage end of the scoring loop on the device (reference diffusion/diffusion_classifier.py:718-721 and the
// ragged class lists it produces, :671-677 / :695-698): mean over the trials evaluated so far, the k smallest classes per
// image, and the next stage's (pair, class) -> work-unit maps, so a multi-stage / fast classify has no device-to-host copy
// and no host index rebuild between stages (per-image early stopping, dc_stage_stop below, copies BS + 1 int32 per stage end).
// Tiny kernels (BS x classes x T floats): one wave per image, fixed order.
#include "common.h"

// One wave per image.  Lane l owns classes l, l+64, ...; the mean of a class is the fp32 sum over j = 0 .. t_end-1 in
// ascending order divided by t_end (inf for a class with an unevaluated cell, which is then never kept) — the order
// depends on nothing but (t_end), so every rank and every world size selects the same classes.  Selection: k rounds of a
// wave-wide arg-min on (order key of the mean, class id), ties to the lower class id; output ascending by mean like
// torch.topk(largest=False), which the host path this replaces used (reference :720): a NaN mean (an overflowed f16 forward:
// inf - inf) sorts AFTER +inf there, so it does here — the key maps every NaN to the largest value.  Taken classes are tracked
// in a per-lane bit mask, so each of the k <= C rounds yields a valid class id whatever the values are.
__device__ __forceinline__ uint32_t stage_order_key(float v) {
  if (v != v) return 0xFFFFFFFFu;                          // NaN: last
  const uint32_t u = __builtin_bit_cast(uint32_t, v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);       // monotone in v (the caller folds -0 into +0 first)
}

template <typename OutT>
__global__ __launch_bounds__(64) void stage_topk_kernel(const float* __restrict__ errors, int C, int T, int t_end, int k,
                                                        OutT* __restrict__ keep, float* __restrict__ means) {
  constexpr int MAXPL = 16;                     // classes per lane: C <= 1024
  const int b = blockIdx.x, lane = threadIdx.x;
  uint32_t m[MAXPL];
#pragma unroll
  for (int i = 0; i < MAXPL; ++i) {
    const int c = lane + 64 * i;
    float s = __builtin_inff();
    if (c < C) {
      const float* e = errors + ((size_t)b * C + c) * T;
      s = 0.f;
      for (int j = 0; j < t_end; ++j) s += e[j];
      s = s / (float)t_end;
      if (means) means[(size_t)b * C + c] = s;
    }
    s = s + 0.f;                                // -0 -> +0 (they compare equal in torch: one key)
    m[i] = stage_order_key(s);
  }
  uint32_t taken = 0;                           // bit i: class lane + 64 i was selected in an earlier round
  for (int r = 0; r < k; ++r) {
    uint32_t bv = 0xFFFFFFFFu;
    int bc = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < MAXPL; ++i) {
      const int c = lane + 64 * i;
      if (c < C && !((taken >> i) & 1u) && (m[i] < bv || (m[i] == bv && c < bc))) { bv = m[i]; bc = c; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const uint32_t ov = (uint32_t)__shfl_xor((int)bv, off, 64);
      const int oc = __shfl_xor(bc, off, 64);
      if (ov < bv || (ov == bv && oc < bc)) { bv = ov; bc = oc; }
    }
    // k <= C and every untaken class of a lane is a candidate (a NaN key equals the initial bv and wins on c < bc): bc is a class id
    if (lane == 0) keep[(size_t)b * k + r] = (OutT)bc;
    if ((bc & 63) == lane) taken |= 1u << (bc >> 6);
  }
}

extern "C" int dc_stage_topk(const float* errors, int32_t BS, int32_t C, int32_t T, int32_t t_end, int32_t k, int32_t* keep,
                             float* means, dc_stream s) {
  DC_REQUIRE(errors && keep, DC_ERR_ARG, "dc_stage_topk: null errors/keep");
  DC_REQUIRE(BS > 0 && C > 0 && C <= 1024 && T > 0 && t_end > 0 && t_end <= T && k > 0 && k <= C, DC_ERR_SHAPE,
             "dc_stage_topk: BS=%d C=%d (<= 1024) T=%d t_end=%d k=%d", BS, C, T, t_end, k);
  hipLaunchKernelGGL(stage_topk_kernel<int32_t>, dim3(BS), dim3(64), 0, reinterpret_cast<hipStream_t>(s), errors, C, T, t_end, k, keep, means);
  return dc_check_launch("dc_stage_topk");
}

// The last stage keeps one class: labels[b] = arg-min_c mean_j errors[b, c, 0 .. t_end)   (reference :718-725), int64 like the
// reference's LongTensor.
extern "C" int dc_reduce_argmin(const float* errors, int32_t BS, int32_t C, int32_t T, int32_t t_end, int64_t* labels, float* means,
                                dc_stream s) {
  DC_REQUIRE(errors && labels, DC_ERR_ARG, "dc_reduce_argmin: null errors/labels");
  DC_REQUIRE(BS > 0 && C > 0 && C <= 1024 && T > 0 && t_end > 0 && t_end <= T, DC_ERR_SHAPE,
             "dc_reduce_argmin: BS=%d C=%d (<= 1024) T=%d t_end=%d", BS, C, T, t_end);
  hipLaunchKernelGGL(stage_topk_kernel<int64_t>, dim3(BS), dim3(64), 0, reinterpret_cast<hipStream_t>(s), errors, C, T, t_end, 1, labels, means);
  return dc_check_launch("dc_reduce_argmin");
}

// Work-unit maps of the next stage's micro-batches, from the surviving classes keep[BS, k].  This rank's r-th pair of the
// stage is global pair g = rank + r * world: trial j = t0 + g / BS, image b = g % BS (dist.py's round-robin deal).  Micro-batch
// m holds local pairs [m * n_bj, (m+1) * n_bj); a slot past the last pair repeats the micro-batch's first pair and scores into
// the dump cell.  maps[m] = | ctx_of_unit[n_bj * k] | out_index[n_bj * k] |: class id of the unit, flat index of errors[b, class, j].
// rows (dc_stage_maps_rows): the stage runs over the images rows[0 .. n_rows) only — trial j = t0 + g / n_rows, image rows[g % n_rows];
// rows == nullptr is every image (n_rows = BS).
__global__ __launch_bounds__(256) void stage_maps_kernel(const int32_t* __restrict__ keep, const int32_t* __restrict__ rows, int n_rows,
                                                         int BS, int C, int T, int k, int t0, int n_pairs, int rank, int world, int n_bj,
                                                         int n_mb, int dump, int32_t* __restrict__ maps) {
  const int U = n_bj * k;
  const long long total = (long long)n_mb * U;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int m = (int)(i / U), u = (int)(i - (long long)m * U);
    const int slot = u / k, c = u - slot * k;
    int r = m * n_bj + slot;
    const bool pad = r >= n_pairs;
    if (pad) r = m * n_bj;
    const long long g = rank + (long long)r * world;
    const int j = t0 + (int)(g / n_rows);
    int b = (int)(g % n_rows);
    if (rows) {
      b = rows[b];
      b = b < 0 ? 0 : (b >= BS ? BS - 1 : b);           // rows[] comes from dc_stage_stop (always an image id); a foreign list must not index out of errors[]
    }
    int cls = keep[(size_t)b * k + c];
    cls = cls < 0 ? 0 : (cls >= C ? C - 1 : cls);       // keep[] comes from dc_stage_topk (always a class id); a foreign list must not index out of errors[]
    int32_t* row = maps + (size_t)m * 2 * U;
    row[u] = cls;
    row[U + u] = pad ? dump : (b * C + cls) * T + j;
  }
}

extern "C" int dc_stage_maps(const int32_t* keep, int32_t BS, int32_t C, int32_t T, int32_t k, int32_t t0, int32_t n_pairs,
                             int32_t rank, int32_t world, int32_t n_bj, int32_t n_mb, int32_t dump, int32_t* maps, dc_stream s) {
  DC_REQUIRE(keep && maps, DC_ERR_ARG, "dc_stage_maps: null keep/maps");
  DC_REQUIRE(BS > 0 && C > 0 && T > 0 && k > 0 && k <= C && t0 >= 0 && t0 < T && n_pairs > 0 && world > 0 && rank >= 0 && rank < world &&
             n_bj > 0 && n_mb > 0 && (long long)(n_mb - 1) * n_bj < n_pairs && (long long)n_mb * n_bj >= n_pairs, DC_ERR_SHAPE,
             "dc_stage_maps: inconsistent extents (BS=%d C=%d T=%d k=%d t0=%d pairs=%d rank=%d/%d n_bj=%d n_mb=%d)", BS, C, T, k, t0,
             n_pairs, rank, world, n_bj, n_mb);
  DC_REQUIRE((long long)BS * C * T < (1LL << 31), DC_ERR_SHAPE, "dc_stage_maps: errors tensor too large for int32 indices");
  const long long last_g = rank + (long long)(n_pairs - 1) * world;
  DC_REQUIRE(t0 + last_g / BS < T, DC_ERR_SHAPE, "dc_stage_maps: the stage's last pair lies beyond trial T-1");
  const long long total = (long long)n_mb * n_bj * k;
  const unsigned grid = (unsigned)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
  hipLaunchKernelGGL(stage_maps_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(s), keep, (const int32_t*)nullptr, BS, BS, C, T,
                     k, t0, n_pairs, rank, world, n_bj, n_mb, dump, maps);
  return dc_check_launch("dc_stage_maps");
}

// dc_stage_maps for a subset of the images (per-image early stopping: the images still undecided, ascending, from dc_stage_stop).
extern "C" int dc_stage_maps_rows(const int32_t* keep, const int32_t* rows, int32_t n_rows, int32_t BS, int32_t C, int32_t T, int32_t k,
                                  int32_t t0, int32_t n_pairs, int32_t rank, int32_t world, int32_t n_bj, int32_t n_mb, int32_t dump,
                                  int32_t* maps, dc_stream s) {
  DC_REQUIRE(keep && rows && maps, DC_ERR_ARG, "dc_stage_maps_rows: null keep/rows/maps");
  DC_REQUIRE(BS > 0 && n_rows > 0 && n_rows <= BS && C > 0 && T > 0 && k > 0 && k <= C && t0 >= 0 && t0 < T && n_pairs > 0 && world > 0 &&
             rank >= 0 && rank < world && n_bj > 0 && n_mb > 0 && (long long)(n_mb - 1) * n_bj < n_pairs && (long long)n_mb * n_bj >= n_pairs,
             DC_ERR_SHAPE, "dc_stage_maps_rows: inconsistent extents (BS=%d rows=%d C=%d T=%d k=%d t0=%d pairs=%d rank=%d/%d n_bj=%d n_mb=%d)", BS,
             n_rows, C, T, k, t0, n_pairs, rank, world, n_bj, n_mb);
  DC_REQUIRE((long long)BS * C * T < (1LL << 31), DC_ERR_SHAPE, "dc_stage_maps_rows: errors tensor too large for int32 indices");
  const long long last_g = rank + (long long)(n_pairs - 1) * world;
  DC_REQUIRE(t0 + last_g / n_rows < T, DC_ERR_SHAPE, "dc_stage_maps_rows: the stage's last pair lies beyond trial T-1");
  const long long total = (long long)n_mb * n_bj * k;
  const unsigned grid = (unsigned)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
  hipLaunchKernelGGL(stage_maps_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(s), keep, rows, n_rows, BS, C, T, k, t0, n_pairs,
                     rank, world, n_bj, n_mb, dump, maps);
  return dc_check_launch("dc_stage_maps_rows");
}

// The class posterior, its entropy and the paired confidence of the decision, from the errors the last stage end reduced to a label
// (include/dcamd.h has the definitions).  Same launch shape as stage_topk_kernel: one wave per image, lane l owns classes l, l+64, ...;
// every per-class sum is sequential over j ascending, every wave reduction a fixed xor butterfly (commutative at each step, so all 64
// lanes hold the same bits), no atomics.  The winner is picked with stage_order_key on (sum / t_end) + 0 — the value and the key
// dc_reduce_argmin uses — among the classes with all t_end cells evaluated, so it cannot disagree with the label.  Cells j >= t_end
// are never read.
__device__ __forceinline__ int posterior_argmin(const uint32_t (&key)[16], uint32_t cand, int lane) {
  uint32_t bv = 0xFFFFFFFFu;
  int bc = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = lane + 64 * i;
    if (((cand >> i) & 1u) && (key[i] < bv || (key[i] == bv && c < bc))) { bv = key[i]; bc = c; }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t ov = (uint32_t)__shfl_xor((int)bv, off, 64);
    const int oc = __shfl_xor(bc, off, 64);
    if (ov < bv || (ov == bv && oc < bc)) { bv = ov; bc = oc; }
  }
  return bc == 0x7fffffff ? -1 : bc;            // a candidate always beats the initial (all ones, int max) pair on c < bc
}

__device__ __forceinline__ float posterior_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// The decision of an image over its cells j < t_end, shared by class_posterior_kernel and stage_stop_kernel (one text: the z-score an
// image was stopped on is the z-score the posterior reports for it, bit for bit).  posterior_class_sums: the per-class sums of lane
// `lane`; paired_decide: winner, runner-up and the paired statistic from them (every lane ends with the same values).
struct paired_decision { int win, run; float mean_w, margin, margin_z; };

__device__ __forceinline__ void posterior_class_sums(const float* __restrict__ E, int C, int T, int t_end, int lane, float (&S)[16],
                                                     int (&n)[16], uint32_t (&key)[16], uint32_t& fin, int& bad_cells,
                                                     float* __restrict__ means, int32_t* __restrict__ n_eval) {
  const float inf = __builtin_inff();
  fin = 0;                                      // bit i: class lane + 64 i is a finalist
  bad_cells = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = lane + 64 * i;
    S[i] = 0.f; n[i] = 0; key[i] = 0xFFFFFFFFu;
    if (c < C) {
      const float* e = E + (size_t)c * T;
      float s = 0.f;
      int cnt = 0;
      for (int j = 0; j < t_end; ++j) {
        const float v = e[j];
        if (v != inf) { s += v; ++cnt; bad_cells += v != v; }
      }
      S[i] = s; n[i] = cnt;
      float mean = cnt > 0 ? s / (float)cnt : inf;          // a finalist: the sum over all j < t_end divided by t_end, as stage_topk_kernel
      if (means) means[c] = mean;
      if (n_eval) n_eval[c] = cnt;
      mean = mean + 0.f;                                    // -0 -> +0
      key[i] = stage_order_key(mean);
      if (cnt == t_end) fin |= 1u << i;
    }
  }
}

__device__ __forceinline__ paired_decision paired_decide(const float* __restrict__ E, int T, int t_end, const uint32_t (&key)[16], uint32_t fin,
                                                         int lane) {
  // every operation below is one IEEE fp32 operation, none fused (ss += d * d as a multiply and an add): posterior.py's torch statement
  // of margin_z then has the same bits, and a threshold that equals an image's z-score decides it the same way on both paths
#pragma clang fp contract(off)
  const float inf = __builtin_inff(), nan = __builtin_nanf("");
  const int win = posterior_argmin(key, fin, lane);
  uint32_t fin2 = fin;
  if (win >= 0 && (win & 63) == lane) fin2 &= ~(1u << (win >> 6));
  const int run = win >= 0 ? posterior_argmin(key, fin2, lane) : -1;

  // the winner's mean (every lane: the same loads in the same order as its owner's sum above) and the paired statistic
  float mean_w = nan, margin = nan, margin_z = nan;
  if (win >= 0) {
    const float* ew = E + (size_t)win * T;
    float sw = 0.f;
    for (int j = 0; j < t_end; ++j) sw += ew[j];
    mean_w = sw / (float)t_end;
    if (run >= 0) {
      const float* er = E + (size_t)run * T;
      float sd = 0.f;
      for (int j = 0; j < t_end; ++j) sd += er[j] - ew[j];
      margin = sd / (float)t_end;
      float ss = 0.f;
      for (int j = 0; j < t_end; ++j) { const float d = (er[j] - ew[j]) - margin; ss += d * d; }
      const float var = ss / (float)(t_end - 1);
      margin_z = margin / sqrtf(var / (float)t_end);
    } else {
      margin = inf; margin_z = inf;
    }
  }
  return {win, run, mean_w, margin, margin_z};
}

__global__ __launch_bounds__(64) void class_posterior_kernel(const dc_class_posterior_params p) {
  constexpr int MAXPL = 16;                     // classes per lane: C <= 1024
  const int b = blockIdx.x, lane = threadIdx.x;
  const int C = p.C, T = p.T, t_end = p.t_end;
  const float inf = __builtin_inff(), nan = __builtin_nanf("");
  const float* E = p.errors + (size_t)b * C * T;
  float S[MAXPL];
  int n[MAXPL];
  uint32_t key[MAXPL];
  uint32_t fin;
  int bad_cells;
  posterior_class_sums(E, C, T, t_end, lane, S, n, key, fin, bad_cells, p.means ? p.means + (size_t)b * C : nullptr,
                       p.n_eval ? p.n_eval + (size_t)b * C : nullptr);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) bad_cells += __shfl_xor(bad_cells, off, 64);

  const paired_decision dec = paired_decide(E, T, t_end, key, fin, lane);
  const int win = dec.win, run = dec.run;
  const float mean_w = dec.mean_w, margin = dec.margin, margin_z = dec.margin_z;
  const bool bad = win < 0 || mean_w != mean_w;

  // delta (kept in S) and the softmax over the classes that have one
  uint32_t valid = 0;
  float mx = -inf;
#pragma unroll
  for (int i = 0; i < MAXPL; ++i) {
    const int c = lane + 64 * i;
    if (c < C) {
      float d = nan;
      if (win >= 0) {
        const float* e = E + (size_t)c * T;
        const float* ew = E + (size_t)win * T;
        float sw = 0.f;
        for (int j = 0; j < t_end; ++j) if (e[j] != inf) sw += ew[j];
        d = (S[i] - sw) / (float)n[i];
      }
      if (p.delta) p.delta[(size_t)b * C + c] = d;
      if (n[i] > 0 && fabsf(d) < inf) {                     // finite: not NaN, not +-inf
        valid |= 1u << i;
        S[i] = -d / p.temperature;
        mx = fmaxf(mx, S[i]);
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  float part = 0.f;
#pragma unroll
  for (int i = 0; i < MAXPL; ++i) {
    S[i] = ((valid >> i) & 1u) ? expf(S[i] - mx) : 0.f;
    part += S[i];
  }
  const float sum = posterior_wave_sum(part);
  float h = 0.f;
#pragma unroll
  for (int i = 0; i < MAXPL; ++i) {
    const int c = lane + 64 * i;
    if (c < C) {
      const float pr = ((valid >> i) & 1u) ? S[i] / sum : 0.f;
      if (pr > 0.f) h += pr * logf(pr);
      p.probs[(size_t)b * C + c] = bad ? nan : pr;
    }
  }
  h = posterior_wave_sum(h);
  if (lane == 0) {
    p.entropy[b] = bad ? nan : 0.f - h;
    p.margin[b] = bad ? nan : margin;
    p.margin_z[b] = bad ? nan : margin_z;
    p.winner[b] = win;
    p.runner[b] = run;
    p.invalid[b] = bad_cells;
  }
}

extern "C" int dc_class_posterior(const dc_class_posterior_params* p, dc_stream s) {
  DC_REQUIRE(p, DC_ERR_ARG, "dc_class_posterior: null params");
  DC_REQUIRE(p->errors && p->probs, DC_ERR_ARG, "dc_class_posterior: null errors/probs");
  DC_REQUIRE(p->entropy && p->margin && p->margin_z && p->winner && p->runner && p->invalid, DC_ERR_ARG,
             "dc_class_posterior: null stats output (entropy, margin, margin_z, winner, runner and invalid are required)");
  DC_REQUIRE(p->temperature > 0.f && p->temperature < __builtin_inff(), DC_ERR_ARG, "dc_class_posterior: temperature %g must be positive and finite",
             (double)p->temperature);
  DC_REQUIRE(p->BS > 0 && p->C > 0 && p->C <= 1024 && p->T > 0 && p->t_end > 0 && p->t_end <= p->T, DC_ERR_SHAPE,
             "dc_class_posterior: BS=%d C=%d (<= 1024) T=%d t_end=%d", p->BS, p->C, p->T, p->t_end);
  hipLaunchKernelGGL(class_posterior_kernel, dim3(p->BS), dim3(64), 0, reinterpret_cast<hipStream_t>(s), *p);
  return dc_check_launch("dc_class_posterior");
}

// Per-image early stopping at a stage boundary (include/dcamd.h has the statement).  stage_stop_kernel: one wave per image still
// active (t_done[b] == 0), the decision by the posterior's own device code above; stage_compact_kernel: one workgroup lists the
// images still active in ascending order — per-wave ballots, a popcount prefix inside the wave and over the (4) waves, chunk after
// chunk in order: no atomics, the list does not depend on timing.
__global__ __launch_bounds__(64) void stage_stop_kernel(const float* __restrict__ errors, int C, int T, int t_end, float z_stop,
                                                        int32_t* __restrict__ t_done, int64_t* __restrict__ labels,
                                                        float* __restrict__ margin_z) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (t_done[b] != 0) return;                   // decided at an earlier boundary: nothing of this image is touched (uniform over the wave)
  const float* E = errors + (size_t)b * C * T;
  float S[16];
  int n[16];
  uint32_t key[16];
  uint32_t fin;
  int bad_cells;
  posterior_class_sums(E, C, T, t_end, lane, S, n, key, fin, bad_cells, nullptr, nullptr);
  const paired_decision dec = paired_decide(E, T, t_end, key, fin, lane);
  const bool bad = dec.win < 0 || dec.mean_w != dec.mean_w;
  if (lane == 0) {
    if (margin_z) margin_z[b] = bad ? __builtin_nanf("") : dec.margin_z;
    if (!bad && dec.margin_z >= z_stop) {       // a NaN z-score (t_end = 1, zero variance at zero margin) never stops; no runner-up (+inf) does
      labels[b] = dec.win;
      t_done[b] = t_end;
    }
  }
}

__global__ __launch_bounds__(256) void stage_compact_kernel(const int32_t* __restrict__ t_done, int BS, int32_t* __restrict__ active_ids,
                                                            int32_t* __restrict__ n_active) {
  __shared__ int wave_cnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;                                 // active images below this chunk (the same in every thread)
  for (int i0 = 0; i0 < BS; i0 += 256) {
    const int i = i0 + tid;
    const bool act = i < BS && t_done[i] == 0;
    const unsigned long long mask = __ballot(act);          // wave64: bit l = lane l of this wave
    if (lane == 0) wave_cnt[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int cnt = wave_cnt[w];
      before += w < wave ? cnt : 0;
      all += cnt;
    }
    if (act) active_ids[base + before + __popcll(mask & ((1ull << lane) - 1ull))] = i;
    base += all;
    __syncthreads();                            // wave_cnt is rewritten by the next chunk
  }
  for (int i = base + tid; i < BS; i += 256) active_ids[i] = -1;
  if (tid == 0) *n_active = base;
}

extern "C" int dc_stage_stop(const float* errors, int32_t BS, int32_t C, int32_t T, int32_t t_end, float z_stop, int32_t* t_done,
                             int64_t* labels, int32_t* active_ids, int32_t* n_active, float* margin_z, dc_stream s) {
  DC_REQUIRE(errors && t_done && labels && active_ids && n_active, DC_ERR_ARG, "dc_stage_stop: null errors/t_done/labels/active_ids/n_active");
  DC_REQUIRE(z_stop > 0.f, DC_ERR_ARG, "dc_stage_stop: z_stop %g must be positive (+inf: never stop)", (double)z_stop);
  DC_REQUIRE(BS > 0 && C > 0 && C <= 1024 && T > 0 && t_end > 0 && t_end <= T, DC_ERR_SHAPE,
             "dc_stage_stop: BS=%d C=%d (<= 1024) T=%d t_end=%d", BS, C, T, t_end);
  hipLaunchKernelGGL(stage_stop_kernel, dim3(BS), dim3(64), 0, reinterpret_cast<hipStream_t>(s), errors, C, T, t_end, z_stop, t_done, labels,
                     margin_z);
  hipLaunchKernelGGL(stage_compact_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(s), t_done, BS, active_ids, n_active);
  return dc_check_launch("dc_stage_stop");
}
