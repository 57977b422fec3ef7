// api.hip — C-ABI glue of libdcamd: version / error reporting and the native plan runner.
// The plan runner replaces the reference's Python double loop body
// (diffusion/diffusion_classifier.py:695-714, one eager op per line) by ONE native call that
// enqueues the whole scoring step on a stream; it performs no allocation or synchronisation,
// so the caller may capture it into a hipGraph.
#include <stdarg.h>
#include <stdio.h>
#include "common.h"

static thread_local char g_err[512] = "";

void dc_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int dc_check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    dc_set_error("%s: HIP launch failed: %s", what, hipGetErrorString(e));
    return DC_ERR_LAUNCH;
  }
  return DC_OK;
}

extern "C" int dc_abi_version(void) { return DC_ABI_VERSION; }
extern "C" const char* dc_last_error(void) { return g_err; }
extern "C" const char* dc_arch(void) { return "gfx950"; }

static int run_one(const dc_op* ops, int i, dc_stream s);

extern "C" int dc_run_plan(const dc_op* ops, int32_t n, dc_stream s) {
  DC_REQUIRE(ops || n == 0, DC_ERR_ARG, "dc_run_plan: null ops");
  for (int i = 0; i < n; ++i) {
    const int rc = run_one(ops, i, s);
    if (rc != DC_OK) return rc;
  }
  return DC_OK;
}

extern "C" int dc_run_plan_timed(const dc_op* ops, int32_t n, dc_stream s, float* ms) {
  DC_REQUIRE((ops && ms) || n == 0, DC_ERR_ARG, "dc_run_plan_timed: null ops/ms");
  hipStream_t st = reinterpret_cast<hipStream_t>(s);
  hipEvent_t* ev = new hipEvent_t[n + 1];
  for (int i = 0; i <= n; ++i) (void)hipEventCreate(&ev[i]);
  int rc = DC_OK;
  (void)hipEventRecord(ev[0], st);
  int done = 0;
  for (; done < n; ++done) {
    rc = run_one(ops, done, s);
    if (rc != DC_OK) break;
    (void)hipEventRecord(ev[done + 1], st);
  }
  (void)hipStreamSynchronize(st);
  for (int i = 0; i < done; ++i) (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
  for (int i = 0; i <= n; ++i) (void)hipEventDestroy(ev[i]);
  delete[] ev;
  return rc;
}

static int run_one(const dc_op* ops, int i, dc_stream s) {
  {
    int rc;
    switch (ops[i].kind) {
      case DC_OP_QSAMPLE: rc = dc_qsample(static_cast<const dc_qsample_params*>(ops[i].params), s); break;
      case DC_OP_SINUSOID: rc = dc_sinusoid(static_cast<const dc_sinusoid_params*>(ops[i].params), s); break;
      case DC_OP_IGEMM: rc = dc_igemm(static_cast<const dc_igemm_params*>(ops[i].params), s); break;
      case DC_OP_GROUPNORM: rc = dc_groupnorm(static_cast<const dc_groupnorm_params*>(ops[i].params), s); break;
      case DC_OP_LAYERNORM: rc = dc_layernorm(static_cast<const dc_layernorm_params*>(ops[i].params), s); break;
      case DC_OP_ATTENTION: rc = dc_attention(static_cast<const dc_attention_params*>(ops[i].params), s); break;
      case DC_OP_CROSS_ATTENTION: rc = dc_cross_attention(static_cast<const dc_cross_attention_params*>(ops[i].params), s); break;
      case DC_OP_CROSS_ATTENTION_LEN: rc = dc_cross_attention_len(static_cast<const dc_cross_attention_len_params*>(ops[i].params), s); break;
      case DC_OP_ATTENTION_BIAS: rc = dc_attention_bias(static_cast<const dc_attention_bias_params*>(ops[i].params), s); break;
      case DC_OP_RMSNORM: rc = dc_rmsnorm(static_cast<const dc_rmsnorm_params*>(ops[i].params), s); break;
      case DC_OP_EMBED_ROWS: rc = dc_embed_rows(static_cast<const dc_embed_rows_params*>(ops[i].params), s); break;
      case DC_OP_RELU: rc = dc_relu(static_cast<const dc_relu_params*>(ops[i].params), s); break;
      case DC_OP_ATTENTION_CAUSAL: rc = dc_attention_causal(static_cast<const dc_attention_causal_params*>(ops[i].params), s); break;
      case DC_OP_LAYERNORM_ROWS: rc = dc_layernorm_rows(static_cast<const dc_layernorm_rows_params*>(ops[i].params), s); break;
      case DC_OP_EMBED_ROWS_POS: rc = dc_embed_rows_pos(static_cast<const dc_embed_rows_pos_params*>(ops[i].params), s); break;
      case DC_OP_ACT_PASS: rc = dc_act_pass(static_cast<const dc_act_pass_params*>(ops[i].params), s); break;
      case DC_OP_TBLOCK_FRONT: rc = dc_tblock_front(static_cast<const dc_tblock_front_params*>(ops[i].params), s); break;
      case DC_OP_EPS_MSE: rc = dc_eps_mse(static_cast<const dc_eps_mse_params*>(ops[i].params), s); break;
      case DC_OP_ERR_MAP: rc = dc_err_map(static_cast<const dc_err_map_params*>(ops[i].params), s); break;
      case DC_OP_ATTENTION_WIDE: rc = dc_attention_wide(static_cast<const dc_attention_wide_params*>(ops[i].params), s); break;
      case DC_OP_CONV3_PN_TAIL: {
        const dc_conv3_pn_tail_op* t = static_cast<const dc_conv3_pn_tail_op*>(ops[i].params);
        rc = dc_conv3_pn_tail(t->conv, t->tail, s);
        break;
      }
      case DC_OP_IM2COL_S2: rc = dc_im2col_s2(static_cast<const dc_im2col_s2_params*>(ops[i].params), s); break;
      case DC_OP_LATENT_IM2COL: rc = dc_latent_im2col(static_cast<const dc_latent_im2col_params*>(ops[i].params), s); break;
      default: dc_set_error("dc_run_plan: op %d has unknown kind %d", i, ops[i].kind); return DC_ERR_ARG;
    }
    if (rc != DC_OK) {
      char inner[400];
      snprintf(inner, sizeof(inner), "%s", g_err);
      dc_set_error("dc_run_plan: op %d (kind %d) failed: %s", i, ops[i].kind, inner);
      return rc;
    }
  }
  return DC_OK;
}
