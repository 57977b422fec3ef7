// conv3_halo_plan.h — host side of the halo-tile 3x3 convolution kernels (conv3_halo.hip, conv3_ws.hip): the patch geometry, worked out
// in one function for all three kernels, and the plan of a launch — geometry, grid and template instance, decided once; the launchers,
// dc_conv3_halo_pn_ok, the dispatcher (igemm.hip) and dc_igemm_instance read it.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include "conv3_halo.h"

static inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// The patch of `pix` output pixels (a power of two) that a workgroup of `nt` threads owns on n_img images of H x W (the extents the kernel
// walks), and its halo: every field of g but xbuf and sws, which are the calling kernel's (0 here).  mosaic_ok: whole images below 8x8
// may share one halo (HaloGeom::mos; the 512-pixel patch only).  False: the halo needs more than nxl_cap loads per lane.
static inline bool halo_geom(HaloGeom& g, int H, int W, int n_img, int pix, int nt, int nxl_cap, bool mosaic_ok) {
  g.H = H; g.W = W; g.n_img = n_img;
  const int tw = W < 32 ? W : 32;
  int th = pix / tw; if (th > H) th = H;
  const int ni = pix / (tw * th);
  g.ltw = ilog2(tw); g.lth = ilog2(th); g.lni = ilog2(ni);
  g.tiles_x = W / tw; g.tiles_y = H / th;
  g.hw = tw + 2; g.hp = (th + 2) * g.hw; g.HR = ni * g.hp;
  g.mos = 0; g.lmc = 0; g.inv_ch = g.inv_cw = 0.f;
  if (mosaic_ok && (H < 8 || W < 8) && tw == W && th == H && ni >= 2) {      // whole small images: mosaic with shared zero borders
    g.mos = 1;
    g.lmc = (g.lni + 1) / 2;           // columns >= rows: 32 images -> 8 x 4
    const int cols = 1 << g.lmc, rows = ni >> g.lmc;
    g.hw = cols * (tw + 1) + 1;
    g.hp = 0;
    g.HR = (rows * (th + 1) + 1) * g.hw;
    g.inv_ch = 1.0f / (float)(th + 1); g.inv_cw = 1.0f / (float)(tw + 1);
  }
  g.inv_hp = g.hp ? 1.0f / (float)g.hp : 0.f; g.inv_hw = 1.0f / (float)g.hw;
  g.xbuf = 0; g.sws = 0;
  g.lpt = ilog2(g.tiles_x * g.tiles_y);
  g.nxl = (g.HR * 4 + nt - 1) / nt;
  return g.nxl <= nxl_cap;
}

// HaloGeom::xbuf beyond "one image per patch": every source image and the weight matrix stay below 2 GiB, the reach of a buffer
// descriptor's 32-bit offset.  a: the extents the kernel walks
static inline bool halo_xbuf_reach(const IgemmArgs& a, int dtype) {
  const long long es = dc_dtype_size(dtype);
  const long long hws = (long long)(a.upsample ? (a.Hin >> 1) * (a.Win >> 1) : a.Hin * a.Win);
  const long long ldmax = a.ld0 > a.ld1 ? (a.ld0 > a.ld2 ? a.ld0 : a.ld2) : (a.ld1 > a.ld2 ? a.ld1 : a.ld2);
  return hws * ldmax * es < (1LL << 31) && (long long)a.tiles_n * 128 * a.Ktot * es < (1LL << 31);
}

// conv3_halo_kernel<T, NW, NTAP, MODE, STG, PN>
struct HaloKey { int NW, NTAP, MODE; bool STG, PN; };

struct HaloPlan {
  HaloGeom g;
  int tiles_m = 0;          // patches x tiles per image (IgemmArgs::tiles_m of the launch)
  unsigned grid = 0;        // workgroups (producer-side GroupNorm across workgroups: padded to whole groups of 8, see the kernel)
  HaloKey key{};            // conv3_halo / conv3_up4 only
  int status = DC_OK;       // DC_OK, or what the launch returns ...
  char message[112] = "";   // ... and reports through dc_last_error
};

__attribute__((format(printf, 2, 3))) static inline HaloPlan& halo_plan_fail(HaloPlan& pl, const char* fmt, ...) {
  pl.status = DC_ERR_SHAPE;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(pl.message, sizeof(pl.message), fmt, ap);
  va_end(ap);
  return pl;
}

// the `geom` list of dc_igemm_instance (include/dcamd.h)
static inline void halo_plan_ints(const HaloPlan& pl, int32_t* out) {
  const HaloGeom& g = pl.g;
  const int32_t v[14] = {1 << g.ltw, 1 << g.lth, 1 << g.lni, g.tiles_x, g.tiles_y, g.hw, g.HR, g.nxl, g.mos, g.xbuf, g.sws, g.lpt, pl.tiles_m, (int32_t)pl.grid};
  for (int i = 0; i < 14; ++i) out[i] = v[i];
}

// conv3_halo.hip.  The plan takes the extents the kernel walks (four-phase upsample form: dc_conv3_up4_walked), the launch and
// dc_conv3_halo_pn_ok the problem as dc_igemm filled it
HaloPlan dc_conv3_halo_plan(const IgemmArgs& walked, int dtype, int n_img, bool up4);
int dc_conv3_halo_launch(const HaloPlan& pl, const IgemmArgs& a, int dtype, bool up4, hipStream_t s);
bool dc_conv3_halo_pn_ok(const IgemmArgs& a, const HaloPlan& pl, bool up4);   // producer-side GroupNorm possible (epi_pn.h)
HaloPlan dc_conv3_thin_plan(const IgemmArgs& a, int n_img);
// tail fold (epi_pn.h): the thin 3x3 conv of Co channels that is the only reader of a PN conv's normalised output, inside that conv.
// a: the conv as dc_igemm filled it (no raw output), pl: its plan
bool dc_conv3_halo_tail_ok(const IgemmArgs& a, const HaloPlan& pl, int dtype, int Co);
int dc_conv3_halo_tail_launch(const HaloPlan& pl, const IgemmArgs& a, int dtype, const PnTail& tl, hipStream_t s);
// elementwise.hip: the border sums of the tail fold (second, stream-ordered launch)
int dc_pn_tail_combine_launch(float* pred, const float* ring, int n_img, int ltw, int lth, int tiles_x, int tiles_y, int H, int W, int Co, int ld,
                              hipStream_t s);
// conv3_ws.hip
HaloPlan dc_conv3_ws_plan(const IgemmArgs& a, int n_img);
