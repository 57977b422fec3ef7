// igemm.hip — implicit-GEMM convolution / GEMM on MFMA for gfx950.
//
// Replaces every Conv2d(3x3|1x1) and Linear of the diffusers backbone the reference calls
// through nets/unet.py:186-195 and nets/dit.py:49-51 (cuDNN/cuBLAS there).
//
// Data layout: activations NHWC (rows = sample*H*W pixels, channels contiguous); weights
// packed [Cout_pad][K], K contiguous, k = tap*(C0+C1) + c.  Both MFMA operands are therefore
// K-contiguous and every global / LDS transfer is a 16-byte chunk.
//
// Tile: BM pixels x BN output channels per 256-thread workgroup (4 waves), K-step = 128 bytes
// per row (64 bf16/f16 or 32 f32 elements), LDS double-buffered, register-staged prefetch of
// the next K-step while the current one is on the matrix cores.  LDS rows are 128 B with the
// 16-B chunk index XOR-swizzled by (row>>1)&7, which makes the ds_read_b128 fragment reads of
// a 16-row MFMA operand conflict-free (MI355X LDS: 64 banks x 4 B, b128 served per 16 lanes).
//
// MFMA orientation: A-operand = weight rows (cout), B-operand = pixel rows, so the f32
// accumulator of a lane is 4 CONSECUTIVE output channels of ONE pixel -> 8/16-byte NHWC stores.
//   bf16/f16: v_mfma_f32_16x16x32_{bf16,f16};  f32: v_mfma_f32_16x16x4_f32 (exact f32 fma chain).
//
// Block->tile map is XCD-aware: the 8 XCDs (private 4 MiB L2 each) receive contiguous ranges of
// the tile list, ordered M-fastest inside one N panel, so the workgroups sharing an L2 stream the
// same weight panel.
#include <stdio.h>
#include <stdlib.h>
#include "conv3_halo_plan.h"

template <typename T, int BM, int BN, int WGM, int WGN>
__global__ __launch_bounds__(256, 2) void igemm_kernel(const IgemmArgs a) {
  constexpr int EPC = Elem<T>::EPC;
  constexpr int BKE = 8 * EPC;            // elements per K-step
  constexpr int XL = BM / 32;             // 16-B X loads per thread per K-step
  constexpr int WL = (BN + 31) / 32;
  constexpr int WTM = BM / WGM, WTN = BN / WGN;
  constexpr int TM = WTM / 16, TN = WTN / 16;
  static_assert(WGM * WGN == 4, "4 waves");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int BUF = (BM + BN) * 128;

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wm = wave / WGN, wn = wave % WGN;
  const int lr = lane & 15, lq = lane >> 4;

  int tile_m, tile_n;
  tile_of_block(a, tile_m, tile_n);

  const int HWo = a.Hout * a.Wout;
  const int pad = (a.taps == 9) ? 1 : 0;
  const int Hs = a.upsample ? (a.Hin >> 1) : a.Hin;
  const int Ws = a.upsample ? (a.Win >> 1) : a.Win;
  const int chunk = t & 7, lrow = t >> 3;

  int ns0[XL], ns1[XL], iy0[XL], ix0[XL];
#pragma unroll
  for (int i = 0; i < XL; ++i) {
    const int m = tile_m * BM + lrow + 32 * i;
    const bool vm = m < a.M;
    const int mm = vm ? m : 0;
    const int n = mm / HWo;
    const int rem = mm - n * HWo;
    const int oy = rem / a.Wout, ox = rem - oy * a.Wout;
    ns0[i] = a.map0 ? a.map0[n] : n;
    ns1[i] = a.src1 ? (a.map1 ? a.map1[n] : n) : 0;
    iy0[i] = vm ? oy * a.stride - pad : -(1 << 20);
    ix0[i] = ox * a.stride - pad;
  }
  const T* wbase = reinterpret_cast<const T*>(a.W) + (size_t)(tile_n * BN + lrow) * a.Ktot + chunk * EPC;

  chunk16 xr[XL], wr[WL];
  const chunk16 zero = {0u, 0u, 0u, 0u};

  auto load_regs = [&](int ks, int tap, int cc) {
    int ky = 0, kx = 0;
    if (a.taps == 9) { ky = tap / 3; kx = tap - ky * 3; }
    const bool s1 = cc >= a.c0chunks;
    const T* src = reinterpret_cast<const T*>(s1 ? a.src1 : a.src0);
    const int ld = s1 ? a.ld1 : a.ld0;
    const int coff = (s1 ? cc - a.c0chunks : cc) * BKE + chunk * EPC;
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const int iy = iy0[i] + ky, ix = ix0[i] + kx;
      const bool ok = (unsigned)iy < (unsigned)a.Hin && (unsigned)ix < (unsigned)a.Win;
      const int sy = a.upsample ? (iy >> 1) : iy, sx = a.upsample ? (ix >> 1) : ix;
      const size_t pix = ((size_t)(s1 ? ns1[i] : ns0[i]) * Hs + sy) * Ws + sx;
      xr[i] = zero;
      if (ok) xr[i] = *reinterpret_cast<const chunk16*>(src + pix * ld + coff);
    }
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      if (BN >= 32 * (i + 1) || lrow + 32 * i < BN)
        wr[i] = *reinterpret_cast<const chunk16*>(wbase + (size_t)(32 * i) * a.Ktot + (size_t)ks * BKE);
    }
  };
  auto write_lds = [&](int buf) {
    char* Xs = smem + buf * BUF;
    char* Wsm = Xs + BM * 128;
#pragma unroll
    for (int i = 0; i < XL; ++i) *reinterpret_cast<chunk16*>(Xs + lds_off(lrow + 32 * i, chunk)) = xr[i];
#pragma unroll
    for (int i = 0; i < WL; ++i)
      if (BN >= 32 * (i + 1) || lrow + 32 * i < BN)
        *reinterpret_cast<chunk16*>(Wsm + lds_off(lrow + 32 * i, chunk)) = wr[i];
  };

  f32x4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  int tap = 0, cc = 0;
  load_regs(0, 0, 0);
  write_lds(0);
  __syncthreads();
  for (int ks = 0; ks < a.nk; ++ks) {
    const bool more = ks + 1 < a.nk;
    if (more) {
      if (++cc == a.cpt) { cc = 0; ++tap; }
      load_regs(ks + 1, tap, cc);
    }
    const char* Xs = smem + (ks & 1) * BUF;
    const char* Wsm = Xs + BM * 128;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int c = sub * 4 + lq;
      chunk16 xf[TM], wf[TN];
#pragma unroll
      for (int j = 0; j < TM; ++j) xf[j] = *reinterpret_cast<const chunk16*>(Xs + lds_off(wm * WTM + j * 16 + lr, c));
#pragma unroll
      for (int i = 0; i < TN; ++i) wf[i] = *reinterpret_cast<const chunk16*>(Wsm + lds_off(wn * WTN + i * 16 + lr, c));
#pragma unroll
      for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = Mma<T>::run(wf[i], xf[j], acc[i][j]);
    }
    if (more) write_lds((ks + 1) & 1);
    __syncthreads();
  }

  igemm_epilogue<TM, TN>(a, acc, tile_m * BM + wm * WTM, tile_n * BN + wn * WTN, lr, lq);
}

template <typename T, int BM, int BN, int WGM, int WGN>
static int launch(const IgemmArgs& a, hipStream_t s) {
  constexpr int lds = 2 * (BM + BN) * 128;
  static bool attr_done = false;
  auto kern = igemm_kernel<T, BM, BN, WGM, WGN>;
  if (!attr_done) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    attr_done = true;
  }
  const long long nblk = (long long)a.tiles_m * a.tiles_n;
  if (nblk <= 0 || nblk > 0x7fffffffLL) { dc_set_error("dc_igemm: bad grid %lld", nblk); return DC_ERR_SHAPE; }
  hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(256), lds, s, a);
  return dc_check_launch("dc_igemm");
}

extern "C" int32_t dc_igemm_cout_pad(int32_t cout, int32_t tile_n) {
  const int tn = tile_n == 32 ? 32 : 128;
  return (cout + tn - 1) / tn * tn;
}

// ---- dispatch ---------------------------------------------------------------------------------------------------------------------
// dc_igemm, dc_igemm_variant, dc_igemm_instance and the dc_igemm_*_ok probes all go the same way: igemm_validate_and_fill, then
// igemm_choose — the one place that picks a kernel or refuses — and then igemm_launch, igemm_name or a look at the choice.

static int igemm_validate_and_fill(const dc_igemm_params* p, IgemmArgs& a) {
  DC_REQUIRE(p, DC_ERR_ARG, "dc_igemm: null params");
  DC_REQUIRE(p->dtype == DC_F32 || p->dtype == DC_BF16 || p->dtype == DC_F16, DC_ERR_DTYPE, "dc_igemm: dtype %d", p->dtype);
  DC_REQUIRE(p->taps == 1 || p->taps == 9, DC_ERR_ARG, "dc_igemm: taps must be 1 or 9 (got %d)", p->taps);
  DC_REQUIRE(p->stride == 1 || p->stride == 2, DC_ERR_ARG, "dc_igemm: stride %d", p->stride);
  DC_REQUIRE(p->tile_n == 128 || p->tile_n == 32, DC_ERR_ARG, "dc_igemm: tile_n %d", p->tile_n);
  DC_REQUIRE(p->src0 && p->W && (p->out || p->pn_out), DC_ERR_ARG, "dc_igemm: null src0/W/out");
  const int bke = 128 / dc_dtype_size(p->dtype);
  DC_REQUIRE(p->C0 > 0 && p->C0 % bke == 0, DC_ERR_SHAPE, "dc_igemm: C0=%d not a multiple of %d", p->C0, bke);
  DC_REQUIRE(p->C1 >= 0 && p->C1 % bke == 0 && ((p->C1 > 0) == (p->src1 != nullptr)), DC_ERR_SHAPE,
             "dc_igemm: C1=%d / src1 mismatch or not a multiple of %d", p->C1, bke);
  DC_REQUIRE(p->n_img > 0 && p->Hout > 0 && p->Wout > 0 && p->Hin > 0 && p->Win > 0 && p->Cout > 0, DC_ERR_SHAPE,
             "dc_igemm: non-positive extent");
  if (p->taps == 9) {
    DC_REQUIRE(p->Hout == (p->Hin + 2 - 3) / p->stride + 1 && p->Wout == (p->Win + 2 - 3) / p->stride + 1, DC_ERR_SHAPE,
               "dc_igemm: 3x3 output %dx%d does not match input %dx%d stride %d", p->Hout, p->Wout, p->Hin, p->Win, p->stride);
  } else {
    DC_REQUIRE(p->stride == 1 && !p->upsample && p->Hout == p->Hin && p->Wout == p->Win, DC_ERR_SHAPE,
               "dc_igemm: taps=1 needs stride 1, no upsample, equal in/out extents");
  }
  if (p->upsample) DC_REQUIRE((p->Hin % 2 == 0) && (p->Win % 2 == 0), DC_ERR_SHAPE, "dc_igemm: upsample needs even Hin/Win");
  const long long M = (long long)p->n_img * p->Hout * p->Wout;
  DC_REQUIRE(M < (1LL << 31), DC_ERR_SHAPE, "dc_igemm: M=%lld too large", M);
  DC_REQUIRE(p->act >= 0 && p->act <= 3, DC_ERR_ARG, "dc_igemm: act %d", p->act);
  if (p->act == DC_ACT_GEGLU) DC_REQUIRE(p->Cout % 32 == 0 && p->tile_n == 128, DC_ERR_SHAPE, "dc_igemm: GEGLU needs Cout%%32==0, tile_n 128");
  // no GEGLU epilogue (igemm_common.h, igemm_epilogue.h) applies a per-sample row vector or gate: refuse them instead of dropping them
  if (p->act == DC_ACT_GEGLU) DC_REQUIRE(!p->rowvec, DC_ERR_ARG, "dc_igemm: rowvec cannot be combined with DC_ACT_GEGLU");
  if (p->act == DC_ACT_GEGLU) DC_REQUIRE(!p->gate, DC_ERR_ARG, "dc_igemm: gate cannot be combined with DC_ACT_GEGLU");
  DC_REQUIRE(((uintptr_t)p->src0 & 15) == 0 && ((uintptr_t)p->W & 15) == 0 && ((uintptr_t)p->src1 & 15) == 0, DC_ERR_ALIGN,
             "dc_igemm: src/W must be 16-byte aligned");
  const int epc = 16 / dc_dtype_size(p->dtype);
  DC_REQUIRE(p->ld0 % epc == 0 && p->ld1 % epc == 0 && (p->ld0 == 0 || p->ld0 >= p->C0) && (p->ld1 == 0 || p->ld1 >= p->C1),
             DC_ERR_SHAPE, "dc_igemm: ld0=%d ld1=%d", p->ld0, p->ld1);
  const int cout_out = p->act == DC_ACT_GEGLU ? p->Cout / 2 : p->Cout;
  DC_REQUIRE(p->out_ld >= cout_out, DC_ERR_SHAPE, "dc_igemm: out_ld %d < %d", p->out_ld, cout_out);
  if (p->residual) DC_REQUIRE(p->res_ld >= cout_out, DC_ERR_SHAPE, "dc_igemm: res_ld");
  if (p->rowvec) DC_REQUIRE(p->rowvec_ld >= cout_out, DC_ERR_SHAPE, "dc_igemm: rowvec_ld");
  if (p->gate) DC_REQUIRE(p->gate_ld >= cout_out, DC_ERR_SHAPE, "dc_igemm: gate_ld");

  a.src0 = p->src0; a.map0 = p->map0; a.src1 = p->src1; a.map1 = p->map1; a.W = p->W; a.bias = p->bias;
  a.rowvec = p->rowvec; a.rowvec_map = p->rowvec_map; a.gate = p->gate; a.gate_map = p->gate_map;
  a.residual = p->residual; a.res_map = p->res_map; a.out = p->out;
  a.gn_scale = p->gn_scale; a.gn_shift = p->gn_shift; a.gn_silu = p->gn_silu;
  a.src2 = p->src2; a.map2 = p->map2; a.W2 = p->W2; a.C2 = p->C2; a.ld2 = p->ld2 ? p->ld2 : p->C2;
  a.ln_eps = p->ln_eps; a.qstats = p->qstats;
  a.pn_out = p->pn_out; a.pn_gamma = p->pn_gamma; a.pn_beta = p->pn_beta; a.pn_cnt = reinterpret_cast<unsigned*>(p->pn_cnt);
  a.pn_ld = p->pn_ld ? p->pn_ld : p->Cout; a.pn_groups = p->pn_groups; a.pn_silu = p->pn_silu; a.pn_eps = p->pn_eps;
  DC_REQUIRE((p->gn_scale == nullptr) == (p->gn_shift == nullptr), DC_ERR_ARG, "dc_igemm: gn_scale/gn_shift must both be set or null");
  a.C0 = p->C0; a.C1 = p->C1; a.ld0 = p->ld0 ? p->ld0 : p->C0; a.ld1 = p->ld1 ? p->ld1 : p->C1;
  a.rowvec_ld = p->rowvec_ld; a.gate_ld = p->gate_ld; a.res_dtype = p->res_dtype;
  a.res_ld = p->res_ld; a.out_dtype = p->out_dtype; a.out_ld = p->out_ld; a.act = p->act;
  a.taps = p->taps; a.stride = p->stride; a.upsample = p->upsample; a.Hin = p->Hin; a.Win = p->Win;
  a.Hout = p->Hout; a.Wout = p->Wout; a.Cout = p->Cout;
  a.M = (int)M; a.Ktot = p->taps * (p->C0 + p->C1);
  a.c0chunks = p->C0 / bke; a.cpt = (p->C0 + p->C1) / bke; a.nk = p->taps * a.cpt;
  const int bn = p->tile_n;
  a.tiles_m = (a.M + 127) / 128;
  a.tiles_n = dc_igemm_cout_pad(p->Cout, bn) / bn;
  {
    // N fastest when the whole weight matrix can stay in an XCD's L2 next to the activation stream (<= 2 MiB), and for 1-tap GEMMs
    // up to gemm_cap (16 MiB, a compile-time constant): there the activation panel of an M tile (rows x K) is the big operand — with
    // M fastest it is re-fetched from HBM once per N panel (DiT-B/4 qkv: 9 x 786 MB per launch, the GEMM ran HBM-bound), with N
    // fastest the N tiles of an M tile run side by side on one XCD and share it in L2, while the weights come back from L2 / MALL
    constexpr long long gemm_cap = 16LL << 20;
    const long long wbytes = (long long)dc_igemm_cout_pad(p->Cout, bn) * a.Ktot * dc_dtype_size(p->dtype);
    a.n_fast = (a.tiles_n > 1 && (wbytes <= (2 << 20) || (p->taps == 1 && wbytes <= gemm_cap))) ? 1 : 0;
  }
  return DC_OK;
}

enum IgemmKernel { IG_THIN, IG_WS, IG_HALO, IG_UP4_HALO, IG_UP4_PIPE, IG_XREG, IG_PIPE, IG_REG128, IG_REG32 };

// What dc_igemm does with a valid problem: the kernel, or (status != DC_OK) the opted-in feature it cannot serve
struct IgemmChoice {
  IgemmKernel kernel = IG_REG32;
  int shape = 0;                   // IG_PIPE: dc_igemm_pipe_shape
  bool gn = false, pn = false;     // IG_WS: GroupNorm prologue; IG_HALO / IG_UP4_HALO: producer-side GroupNorm
  int status = DC_OK;
  const char* tag = nullptr;       // refusal: what dc_igemm_variant reports ...
  const char* message = nullptr;   // ... and what dc_last_error reports after dc_igemm
  HaloPlan halo;                   // IG_HALO / IG_UP4_HALO: the launch (a plan that failed is the launch's error, not a refusal)
};

// the caller opted in to a feature (src2, gn_scale, qstats, pn_out, up4, ln_eps), so a problem that cannot take it is an error
static IgemmChoice refuse(const char* tag, const char* message) { return IgemmChoice{IG_REG32, 0, false, false, DC_ERR_UNSUPPORTED, tag, message}; }

// p, a: after igemm_validate_and_fill.  No launch, no formatting (but the message of a halo plan that failed), no dc_set_error: dc_run_plan
// comes through here for every op of every step
static IgemmChoice igemm_choose(const dc_igemm_params* p, const IgemmArgs& a) {
  const int dt = p->dtype, bn = p->tile_n, epc = 16 / dc_dtype_size(dt);
  const int cout_out = p->act == DC_ACT_GEGLU ? p->Cout / 2 : p->Cout;
  // tile_n 128: the LDS-DMA kernels (igemm_pipe.hip, igemm_wide.hip, igemm_xreg.hip, conv3_*.hip).
  // the LDS-DMA kernels finish with the lane-resident epilogue (igemm_epilogue.h): whole 16-byte runs of 8 channels in
  // and out.  Anything else (channel counts / leading dimensions that are not multiples of 8, unaligned side
  // operands) takes the register-staged kernel, whose element-wise epilogue handles every case.
  const bool lane_epi_ok = cout_out % 8 == 0 && p->out_ld % 8 == 0 && ((uintptr_t)p->out & 15) == 0 &&      // (a null `out`: producer-side GroupNorm only)
                           (!p->residual || (p->res_ld % 8 == 0 && ((uintptr_t)p->residual & 15) == 0)) &&
                           (!p->bias || ((uintptr_t)p->bias & 15) == 0) &&
                           (!p->rowvec || (((uintptr_t)p->rowvec & 15) == 0 && p->rowvec_ld % 4 == 0)) &&
                           (!p->gate || (((uintptr_t)p->gate & 15) == 0 && p->gate_ld % 4 == 0 && p->act == DC_ACT_NONE)) &&
                           (!p->residual || p->res_dtype == dt) && (p->out_dtype == dt || p->out_dtype == DC_F32);
  const bool lds_dma = bn == 128 && lane_epi_ok;
  static const bool no_halo = getenv("DCAMD_NO_HALO") != nullptr;
  const bool halo_ok = lds_dma && !no_halo && dc_conv3_halo_applicable(a, dt);
  // quad statistics / producer-side GroupNorm: what the plain and the four-phase form both ask of the operands
  const bool qs_args_ok = p->out_dtype == dt && p->Cout % 8 == 0 && ((uintptr_t)a.qstats & 15) == 0;
  const bool pn_args_ok = a.pn_gamma && a.pn_beta && a.pn_cnt && p->out_dtype == dt && a.pn_ld % 8 == 0 && a.pn_ld >= p->Cout &&
                          (((uintptr_t)a.pn_out | (uintptr_t)a.qstats) & 15) == 0 && ((uintptr_t)a.pn_cnt & 3) == 0 && a.pn_eps > 0.f;
  const bool use_pn = a.pn_out != nullptr;

  if (p->up4) {      // four-phase upsample conv (W in the phase-summed form)
    const bool up4_halo = lds_dma && !no_halo && !a.src1 && dc_conv3_up4_applicable(a, dt) &&
                          (!a.qstats || (qs_args_ok && (a.Hin >> 1) >= 8 && (a.Win >> 1) >= 8));      // no quad statistics from mosaic (< 8x8) patches
    // sources smaller than 8x8 (4x4 -> 8x8): the same four phases on the tap-gather kernel (no quad statistics there)
    const bool up4_pipe = !up4_halo && lds_dma && !a.src1 && !a.qstats && p->taps == 9 && p->stride == 1 &&
                          p->upsample && p->act == DC_ACT_NONE && !p->gate && !p->residual && !a.gn_scale && !a.src2 &&
                          p->Hin >= 4 && p->Win >= 4 && p->Hin % 2 == 0 && p->Win % 2 == 0 && (p->Hin < 16 || p->Win < 16);
    const HaloPlan plan = up4_halo ? dc_conv3_halo_plan(dc_conv3_up4_walked(a), dt, p->n_img, true) : HaloPlan{};
    // producer-side GroupNorm on the four-phase form: the 4-wave one-image-per-patch kernel only (sources of 16x16 and more)
    if (use_pn && !(up4_halo && a.Hin > 16 && a.Win > 16 && dc_conv3_halo_pn_ok(a, plan, true) && a.qstats && pn_args_ok))
      return refuse("producer-groupnorm-unsupported", "dc_igemm: pn_out given but this upsample conv cannot normalise its own output (see dc_igemm_pn_ok)");
    if (!up4_halo && !up4_pipe)
      return refuse("up4-unsupported", "dc_igemm: up4 given but this problem cannot take the four-phase upsample conv (see dc_igemm_up4_ok)");
    if (up4_halo) return IgemmChoice{IG_UP4_HALO, 0, false, use_pn, DC_OK, nullptr, nullptr, plan};
    return IgemmChoice{IG_UP4_PIPE};
  }

  const bool thin_app = dc_conv3_thin_applicable(a, dt);
  const bool thin = thin_app && ((uintptr_t)p->out & 3) == 0;       // (with gn_scale: conv_out, normalised in the halo)
  // wave-specialised halo conv: takes the fused GroupNorm prologue (also together with the 1x1 side source / a residual); DCAMD_WS_PLAIN
  // routes the plain one-image-per-patch convs there too (A/B of the structure alone)
  static const bool ws_plain = getenv("DCAMD_WS_PLAIN") != nullptr;
  const bool ws_ok = halo_ok && dc_conv3_ws_ok(a, dt) && !thin_app;
  const bool use_ws = ws_ok && (a.gn_scale || ws_plain);
  // the route of the plain halo conv, unless a refusal below
  const HaloPlan plan = halo_ok && !thin && !use_ws ? dc_conv3_halo_plan(a, dt, p->n_img, false) : HaloPlan{};
  const int bke64 = 64 / dc_dtype_size(dt);
  if (a.src2 && !(halo_ok && (!a.gn_scale || ws_ok) && !a.upsample && a.W2 && a.C2 >= 2 * bke64 && a.C2 % bke64 == 0 && a.ld2 % epc == 0 &&
                  (((uintptr_t)a.src2 | (uintptr_t)a.W2) & 15) == 0))
    return refuse("side-source-unsupported", "dc_igemm: src2/W2 given but this problem cannot take the 1x1 side source (see dc_igemm_side_ok)");
  if (a.gn_scale && !thin && !ws_ok)
    return refuse("gn-not-fusable", "dc_igemm: gn_scale/gn_shift given but this problem cannot take the fused GroupNorm prologue (see dc_igemm_gn_fusable)");
  if (a.qstats && !(halo_ok && !thin_app && qs_args_ok && a.Hin >= 8 && a.Win >= 8))      // mosaic patches (images below 8x8) emit none: a wave's half holds four images
    return refuse("qstats-unsupported", "dc_igemm: qstats given but this problem cannot emit quad statistics (see dc_igemm_qstats_parts)");
  if (use_pn && !(halo_ok && !use_ws && !a.gn_scale && !thin_app && dc_conv3_halo_pn_ok(a, plan, false) &&
                  (a.qstats || (a.Hin == 4 && a.Win == 4)) && pn_args_ok))
    return refuse("producer-groupnorm-unsupported", "dc_igemm: pn_out given but this problem cannot normalise its own output (see dc_igemm_pn_ok)");
  const bool xreg_app = dc_igemm_xreg_applicable(a, dt);
  if (a.ln_eps > 0.f && !(lds_dma && !a.src1 && xreg_app))
    return refuse("row-layernorm-unsupported", "dc_igemm: ln_eps given but this problem cannot take the fused row LayerNorm (see dc_igemm_ln_ok)");

  if (thin) return IgemmChoice{IG_THIN};
  if (use_ws) return IgemmChoice{IG_WS, 0, a.gn_scale != nullptr};
  if (halo_ok) return IgemmChoice{IG_HALO, 0, false, use_pn, DC_OK, nullptr, nullptr, plan};
  if (!lds_dma) return IgemmChoice{bn == 128 ? IG_REG128 : IG_REG32};
  // short-K GEMMs: the activation-stationary kernel wins for GEGLU (448 vs 376 TFLOP/s at K = 256, 584 vs 544 at K = 512);
  // for plain epilogues the 256x256 tile is faster where it applies (q/k/v 505-709 vs 478-556), xreg elsewhere
  const int shape = dc_igemm_pipe_shape(a);
  if (xreg_app && (p->act == DC_ACT_GEGLU || a.ln_eps > 0.f || shape != 2)) return IgemmChoice{IG_XREG};
  return IgemmChoice{IG_PIPE, shape};
}

static const char* igemm_name(const IgemmChoice& c, int dtype) {
  // by dc_igemm_pipe_shape, as dc_igemm_launch_pipe switches
  static const char* const pipe_fmt[3] = {"igemm_pipe<%s,128x128,2st>", "igemm_pipe<%s,256x128,3st>", "igemm_wide8<%s,256x256>"};
  static thread_local char name[64];
  const char* dn = dtype == DC_BF16 ? "bf16" : (dtype == DC_F16 ? "f16" : "f32");
  switch (c.kernel) {
    case IG_THIN: snprintf(name, sizeof(name), "conv3_thin<%s>", dn); break;
    case IG_WS: snprintf(name, sizeof(name), c.gn ? "conv3_ws<%s,gn>" : "conv3_ws<%s>", dn); break;
    case IG_HALO: snprintf(name, sizeof(name), c.pn ? "conv3_halo<%s,%dw,pn>" : "conv3_halo<%s,%dw>", dn, c.halo.key.NW); break;
    case IG_UP4_HALO: snprintf(name, sizeof(name), c.pn ? "conv3_up4<%s,%dw,pn>" : "conv3_up4<%s,%dw>", dn, c.halo.key.NW); break;
    case IG_UP4_PIPE: snprintf(name, sizeof(name), "igemm_pipe_up4<%s,256x128,3st>", dn); break;
    case IG_XREG: snprintf(name, sizeof(name), "igemm_xreg<%s,96xN>", dn); break;
    case IG_PIPE: snprintf(name, sizeof(name), pipe_fmt[c.shape], dn); break;
    case IG_REG128: snprintf(name, sizeof(name), "igemm<%s,128x128>", dn); break;
    case IG_REG32: snprintf(name, sizeof(name), "igemm<%s,128x32>", dn); break;
  }
  return name;
}

static int igemm_launch(const IgemmChoice& c, const IgemmArgs& a, const dc_igemm_params* p, dc_stream stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  switch (c.kernel) {
    case IG_THIN: return dc_conv3_thin_launch(a, p->dtype, p->n_img, s);
    case IG_WS: return dc_conv3_ws_launch(a, p->dtype, p->n_img, s);
    case IG_HALO: return dc_conv3_halo_launch(c.halo, a, p->dtype, false, s);
    case IG_UP4_HALO: return dc_conv3_halo_launch(c.halo, a, p->dtype, true, s);
    case IG_UP4_PIPE: return dc_igemm_launch_pipe_up4(a, p->dtype, s);
    case IG_XREG: return dc_igemm_xreg_launch(a, p->dtype, s);
    case IG_PIPE: return dc_igemm_launch_pipe(a, p->dtype, c.shape, s);
    case IG_REG128: return dc_by_dtype(p->dtype, "dc_igemm: dtype", [&](auto t) { return launch<decltype(t), 128, 128, 2, 2>(a, s); });
    case IG_REG32: return dc_by_dtype(p->dtype, "dc_igemm: dtype", [&](auto t) { return launch<decltype(t), 128, 32, 4, 1>(a, s); });
  }
  return DC_ERR_ARG;
}

extern "C" int dc_igemm(const dc_igemm_params* p, dc_stream stream) {
  IgemmArgs a;
  const int rc = igemm_validate_and_fill(p, a);
  if (rc != DC_OK) return rc;
  const IgemmChoice c = igemm_choose(p, a);
  if (c.status != DC_OK) { dc_set_error("%s", c.message); return c.status; }
  return igemm_launch(c, a, p, stream);
}

extern "C" const char* dc_igemm_variant(const dc_igemm_params* p) {
  IgemmArgs a;
  if (igemm_validate_and_fill(p, a) != DC_OK) return "invalid";
  const IgemmChoice c = igemm_choose(p, a);
  return c.status == DC_OK ? igemm_name(c, p->dtype) : c.tag;
}

extern "C" const char* dc_igemm_instance(const dc_igemm_params* p, int32_t* geom) {
  IgemmArgs a;
  if (igemm_validate_and_fill(p, a) != DC_OK) return "invalid";
  const IgemmChoice c = igemm_choose(p, a);
  if (c.status != DC_OK) return c.tag;
  static thread_local char name[64];
  const char* dn = p->dtype == DC_BF16 ? "bf16" : (p->dtype == DC_F16 ? "f16" : "f32");
  HaloPlan pl;
  switch (c.kernel) {
    case IG_HALO: case IG_UP4_HALO: {
      pl = c.halo;
      const HaloKey& k = pl.key;
      snprintf(name, sizeof(name), "conv3_halo_kernel<%s,%d,%d,%d%s%s>", dn, k.NW, k.NTAP, k.MODE, k.STG ? ",stag" : "", k.PN ? ",pn" : "");
      break;
    }
    case IG_THIN: pl = dc_conv3_thin_plan(a, p->n_img); snprintf(name, sizeof(name), "conv3_thin_kernel<%s,%s>", dn, a.gn_scale ? "gn" : "plain"); break;
    case IG_WS: pl = dc_conv3_ws_plan(a, p->n_img); snprintf(name, sizeof(name), "conv3_ws_kernel<%s,%s>", dn, a.gn_scale ? "gn" : "plain"); break;
    default: return igemm_name(c, p->dtype);
  }
  if (geom) halo_plan_ints(pl, geom);
  return name;
}

// ---- probes: plant what the feature needs where the caller left it out, choose, test ---------------------------------------------
static int32_t igemm_accepts(const dc_igemm_params& q) {
  IgemmArgs a;
  return igemm_validate_and_fill(&q, a) == DC_OK && igemm_choose(&q, a).status == DC_OK ? 1 : 0;
}
alignas(16) static float g_probe_dummy[4] = {0.f, 0.f, 0.f, 0.f};

extern "C" int32_t dc_igemm_gn_fusable(const dc_igemm_params* p) {
  if (!p) return 0;
  dc_igemm_params q = *p;
  q.gn_scale = g_probe_dummy; q.gn_shift = g_probe_dummy;
  return igemm_accepts(q);
}

extern "C" int32_t dc_igemm_ln_ok(const dc_igemm_params* p) {
  if (!p) return 0;
  dc_igemm_params q = *p;
  if (!(q.ln_eps > 0.f)) q.ln_eps = 1e-5f;
  return igemm_accepts(q);
}

extern "C" int32_t dc_igemm_qstats_parts(const dc_igemm_params* p) {
  if (!p) return 0;
  dc_igemm_params q = *p;
  if (!q.qstats) q.qstats = g_probe_dummy;
  if (!igemm_accepts(q)) return 0;
  const int hw = p->Hout * p->Wout;
  if (p->up4) { const int lo = hw >> 2; return 4 * (lo >= 128 ? lo / 128 : 1); }     // per phase, on the low-resolution image
  return hw >= 128 ? hw / 128 : 1;          // one part per wave-sized run of 128 pixels (64-pixel images: one)
}

extern "C" int32_t dc_igemm_pn_ok(const dc_igemm_params* p) {
  if (!p || p->pn_groups <= 0) return 0;
  dc_igemm_params q = *p;
  if (!q.pn_out) q.pn_out = g_probe_dummy;
  if (!q.qstats && !(q.Hin == 4 && q.Win == 4)) q.qstats = g_probe_dummy;      // (4x4 mosaic patches form no quad records: their GroupNorm needs none)
  if (!q.pn_gamma) q.pn_gamma = g_probe_dummy;
  if (!q.pn_beta) q.pn_beta = g_probe_dummy;
  if (!q.pn_cnt) q.pn_cnt = reinterpret_cast<uint32_t*>(g_probe_dummy);
  if (!(q.pn_eps > 0.f)) q.pn_eps = 1e-5f;
  return igemm_accepts(q);
}

extern "C" int32_t dc_pn_timeouts(void) { return (int32_t)dc_conv3_halo_pn_timeouts(); }

// ---- tail fold: the last ResNet conv + conv_norm_out + SiLU + conv_out as one op (epi_pn.h) ----------------------------------------
// The conv goes the way of every dc_igemm call with pn_out — validate, choose — and must come out as the 4-wave exchange form of
// conv3_halo; what the tail adds is checked here.  Probes (no launch) may leave pointers out: dummies stand in, as in the probes above.
struct TailChoice { IgemmArgs a; IgemmChoice c; int status = DC_OK; const char* tag = nullptr; const char* message = nullptr; };

static TailChoice tail_choose(const dc_igemm_params* conv, const dc_pn_tail_params* tail, bool probe) {
  TailChoice t;
  auto fail = [&](int st, const char* tag, const char* msg) -> TailChoice& { t.status = st; t.tag = tag; t.message = msg; return t; };
  if (!conv || !tail) return fail(DC_ERR_ARG, "invalid", "dc_conv3_pn_tail: null params");
  if (conv->out || conv->pn_out) return fail(DC_ERR_UNSUPPORTED, "tail-raw-output", "dc_conv3_pn_tail: the conv's own output (out / pn_out) is never stored; leave both null");
  dc_igemm_params q = *conv;
  q.pn_out = g_probe_dummy;                                   // never written: the TAIL instance has no normalised store
  q.pn_gamma = tail->gamma; q.pn_beta = tail->beta; q.pn_cnt = tail->cnt;
  q.pn_ld = 0; q.pn_groups = tail->groups; q.pn_silu = tail->silu; q.pn_eps = tail->eps;
  if (probe) {
    if (!q.qstats) q.qstats = g_probe_dummy;
    if (!q.pn_gamma) q.pn_gamma = g_probe_dummy;
    if (!q.pn_beta) q.pn_beta = g_probe_dummy;
    if (!q.pn_cnt) q.pn_cnt = reinterpret_cast<uint32_t*>(g_probe_dummy);
    if (!(q.pn_eps > 0.f)) q.pn_eps = 1e-5f;
  } else if (!tail->Wt || !tail->pred || !tail->ring || ((uintptr_t)tail->Wt & 15) || (((uintptr_t)tail->pred | (uintptr_t)tail->ring | (uintptr_t)tail->bias) & 3)) {
    return fail(DC_ERR_ARG, "invalid", "dc_conv3_pn_tail: Wt (16-byte aligned), pred and ring must be given");
  }
  if (q.pn_groups <= 0) return fail(DC_ERR_ARG, "invalid", "dc_conv3_pn_tail: groups");
  if (igemm_validate_and_fill(&q, t.a) != DC_OK) return fail(DC_ERR_ARG, "invalid", nullptr);      // (the text is already in place)
  t.c = igemm_choose(&q, t.a);
  if (t.c.status != DC_OK) return fail(t.c.status, t.c.tag, t.c.message);
  if (t.c.kernel != IG_HALO || !t.c.pn || !dc_conv3_halo_tail_ok(t.a, t.c.halo, q.dtype, tail->Co) || tail->pred_ld < tail->Co)
    return fail(DC_ERR_UNSUPPORTED, "tail-unsupported",
                "dc_conv3_pn_tail: needs a 16-bit 3x3 conv with Cout = 128 on the 4-wave producer-GroupNorm form and 1 <= Co <= 3 (see dc_conv3_pn_tail_ok)");
  return t;
}

extern "C" int32_t dc_conv3_pn_tail_ok(const dc_igemm_params* conv, const dc_pn_tail_params* tail) {
  return tail_choose(conv, tail, true).status == DC_OK ? 1 : 0;
}

extern "C" const char* dc_conv3_pn_tail_variant(const dc_igemm_params* conv, const dc_pn_tail_params* tail) {
  const TailChoice t = tail_choose(conv, tail, true);
  if (t.status != DC_OK) return t.tag;
  return conv->dtype == DC_BF16 ? "conv3_halo<bf16,4w,pn,tail>" : "conv3_halo<f16,4w,pn,tail>";
}

extern "C" int64_t dc_conv3_pn_tail_ring_floats(const dc_igemm_params* conv, const dc_pn_tail_params* tail) {
  const TailChoice t = tail_choose(conv, tail, true);
  if (t.status != DC_OK) return 0;
  const HaloGeom& g = t.c.halo.g;
  return (long long)conv->n_img * g.tiles_x * g.tiles_y * PN_TAIL_RING(1 << g.ltw, 1 << g.lth) * tail->Co;
}

extern "C" int dc_conv3_pn_tail(const dc_igemm_params* conv, const dc_pn_tail_params* tail, dc_stream stream) {
  const TailChoice t = tail_choose(conv, tail, false);
  if (t.status != DC_OK) { if (t.message) dc_set_error("%s", t.message); return t.status; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const PnTail tl{tail->Wt, tail->bias, tail->pred, tail->ring, tail->Co, tail->pred_ld};
  const int rc = dc_conv3_halo_tail_launch(t.c.halo, t.a, conv->dtype, tl, s);
  if (rc != DC_OK) return rc;
  const HaloGeom& g = t.c.halo.g;
  return dc_pn_tail_combine_launch(tail->pred, tail->ring, conv->n_img, g.ltw, g.lth, g.tiles_x, g.tiles_y, g.H, g.W, tail->Co, tail->pred_ld, s);
}

extern "C" int32_t dc_igemm_up4_ok(const dc_igemm_params* p) {
  if (!p) return 0;
  dc_igemm_params q = *p;
  q.up4 = 1;
  return igemm_accepts(q);
}

extern "C" int32_t dc_igemm_side_ok(const dc_igemm_params* p) {
  if (!p) return 0;
  dc_igemm_params q = *p;
  if (!q.src2) { q.src2 = g_probe_dummy; q.W2 = g_probe_dummy; }
  return igemm_accepts(q);
}
