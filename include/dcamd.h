/* dcamd.h — C-ABI of the MI355X (gfx950) diffusion-classifier scoring path.
 *
 * One shared library, libdcamd.so, plain C entry points, plain pointers and sizes, no
 * torch types.  Every entry point enqueues HIP kernels on the caller's stream and
 * returns; nothing allocates, frees or synchronises.  The caller owns every buffer.
 *
 * What each entry point replaces in the reference (faverogian/diffusion-classifier):
 *   dc_qsample          diffusion/diffusion_classifier.py:100-117 (diffuse) + :690-692
 *   dc_philox_normal    torch.randn_like at diffusion_classifier.py:113 (throughput mode)
 *   dc_sinusoid         diffusers Timesteps behind nets/unet.py:187 / nets/dit.py:50
 *   dc_igemm            every Conv2d 3x3/1x1 and Linear of the diffusers backbone behind
 *                       nets/unet.py:186-195 and nets/dit.py:49-51 (implicit GEMM on MFMA)
 *   dc_groupnorm        GroupNorm(+SiLU) sites of ResnetBlock2D / Transformer2DModel
 *   dc_layernorm        LayerNorm sites of BasicTransformerBlock; adaLN-Zero modulate (DiT)
 *   dc_attention        F.scaled_dot_product_attention self-attention (attn1)
 *   dc_cross_attention  F.scaled_dot_product_attention cross-attention (attn2) over a context of several tokens
 *                       (encode_text_prompt's [B, S, hid], diffusion_classifier.py:93-98; one token needs no kernel)
 *   dc_cross_attention_len  the same over prompts of different lengths padded to S tokens: a key count per context, which is
 *                       what diffusers' encoder_attention_mask expresses for a text encoder's padded output
 *   dc_attention_bias / dc_rmsnorm / dc_embed_rows / dc_relu
 *                       the T5 encoder behind encode_text_prompt (diffusion_classifier.py:59-74, :93-98: transformers' T5EncoderModel;
 *                       its Linear layers are dc_igemm): self-attention with the relative-position bias and the padding mask, T5LayerNorm,
 *                       the token embedding and the feed-forward's ReLU
 *   dc_attention_causal / dc_layernorm_rows / dc_embed_rows_pos / dc_act_pass
 *                       a CLIP text transformer (transformers' CLIPTextModel) as the text encoder behind encode_text_prompt: causal
 *                       self-attention with a row count per sample, LayerNorm from the fp32 stream into the compute type, token +
 *                       position embedding, quick-GELU / erf-GELU
 *   dc_attention_wide / dc_im2col_s2
 *                       nothing in the reference: the encoder half of diffusers' AutoencoderKL in front of a latent-space backbone
 *                       (config key vae_path) — its mid-block attention over one head of 256 / 512 channels, and the A operand of its
 *                       bottom/right-padded stride-2 downsampling conv; every other layer of the encoder is dc_igemm / dc_groupnorm
 *   dc_latent_im2col    nothing in the reference: the decoder half of the same AutoencoderKL (decode_latents, sample / counterfactual with
 *                       decode=True) — post_quant_conv and the un-scaling of the latents in fp32, written as the A operand of the
 *                       decoder's conv_in; every other layer of the decoder is dc_igemm / dc_groupnorm / dc_attention(_wide)
 *   dc_eps_mse          diffusion_classifier.py:706-711 (v->eps, torch.norm(...)**2); additive: DC_LOSS_L1 / DC_LOSS_HUBER sums
 *   dc_haar_dwt2/idwt2  utils/wavelet.py:4-35 / :37-68
 *   dc_ddpm_step        diffusion_classifier.py:175-208 (ddpm_sampler_step) + :262-266, one fused pass per sampling step
 *   dc_ddpm_step_shared / dc_abs_diff_map
 *                       experiments/ipmsa/explain.py: every class trajectory of an image from shared noise, and where they differ
 *   dc_solver_step      nothing in the reference: one pass of a deterministic sampler (DDIM, DPM-Solver++ 2M) or of DDIM inversion on
 *                       the prediction pair dc_ddpm_step reads, for sample / counterfactual with config.sampler set and for invert
 *   dc_ddpm_noise_map   nothing in the reference: the noise under which one ancestral step lands on a given next latent (edit-friendly
 *                       DDPM inversion), for invert_ddpm and counterfactual(start="ddpm_invert")
 *   dc_stage_topk / dc_reduce_argmin / dc_stage_maps
 *                       the stage end, diffusion_classifier.py:718-725 (mean over trials, k smallest classes) and the
 *                       per-image surviving-class lists of the next stage (:695-698, ragged after pruning / fast mode
 *                       :671-677) as device-side work-unit maps
 *   dc_stage_stop / dc_stage_maps_rows
 *                       nothing in the reference: per-image early stopping at a stage boundary (config key stop_margin_z) — the images
 *                       whose paired z-score reached the threshold keep their label and leave the grid; the next stage's maps over
 *                       the images still undecided
 *   dc_class_posterior  nothing in the reference: the class posterior (Li et al. 2023, eq. 5, on paired differences), its entropy and
 *                       the paired confidence of the decision, from the errors tensor :718-725 reduces to one label
 *   dc_err_map / dc_evidence_maps
 *                       nothing in the reference: per-pixel class evidence from the scoring loop — where in the image a class explains
 *                       the noise worse than the winner (the spatial form of dc_class_posterior's delta), from the same predictions
 *   dc_run_plan         the Python double loop body, diffusion_classifier.py:695-714, as
 *                       one native launch sequence (graph-capturable)
 *
 * Errors: 0 = ok; negative dc_status otherwise; text via dc_last_error() (thread-local).
 * No exception crosses the ABI.  HIP launch errors are returned as DC_ERR_LAUNCH.
 */
#ifndef DCAMD_H
#define DCAMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: qstats records are (mean, M2) sets (version 1: sum, sum of squares) and qparts must divide HW
 * 3: dc_ddpm_step_params.one_plus_w; dc_attention requires scale > 0; dc_igemm_params.pn_* (producer-side GroupNorm)
 * (dc_cross_attention, dc_cross_attention_variant and DC_OP_CROSS_ATTENTION are additive within 4: no existing struct or symbol changed)
 * (dc_cross_attention_len, dc_cross_attention_len_variant, dc_cross_attention_len_params and DC_OP_CROSS_ATTENTION_LEN likewise)
 * (the T5 encoder's entries — dc_attention_bias, dc_attention_bias_variant, dc_rmsnorm, dc_embed_rows, dc_relu, their structs and
 *  DC_OP_ATTENTION_BIAS / DC_OP_RMSNORM / DC_OP_EMBED_ROWS / DC_OP_RELU — likewise)
 * (dc_class_posterior and dc_class_posterior_params likewise; it is called directly, there is no DC_OP_* kind for it)
 * (the CLIP text encoder's entries — dc_attention_causal, dc_attention_causal_variant, dc_layernorm_rows, dc_embed_rows_pos,
 *  dc_act_pass, their structs, dc_pass_kind and DC_OP_ATTENTION_CAUSAL / DC_OP_LAYERNORM_ROWS / DC_OP_EMBED_ROWS_POS / DC_OP_ACT_PASS —
 *  likewise)
 * (dc_ddpm_step_shared, dc_abs_diff_map and their structs likewise; both are called directly)
 * (dc_stage_stop and dc_stage_maps_rows likewise; both are called directly)
 * (dc_err_map, dc_err_map_params and DC_OP_ERR_MAP, and dc_evidence_maps with dc_evidence_maps_params — called directly — are additive
 *  within 5: no existing struct or symbol changed)
 * (dc_solver_step and dc_solver_step_params — called directly — are additive within 5 likewise)
 * (dc_ddpm_noise_map and dc_ddpm_noise_map_params — called directly — likewise)
 * (the AutoencoderKL encoder's entries — dc_attention_wide, dc_attention_wide_variant, dc_im2col_s2, their structs and
 *  DC_OP_ATTENTION_WIDE / DC_OP_IM2COL_S2 — likewise)
 * (dc_conv3_pn_tail, dc_conv3_pn_tail_ok, dc_conv3_pn_tail_variant, dc_conv3_pn_tail_ring_floats, dc_pn_tail_params, dc_conv3_pn_tail_op
 *  and DC_OP_CONV3_PN_TAIL — likewise)
 * (the AutoencoderKL decoder's head — dc_latent_im2col, dc_latent_im2col_params and DC_OP_LATENT_IM2COL — likewise)
 * (the scoring loss — `loss` and `huber_delta`, the LAST two fields of dc_eps_mse_params and dc_err_map_params, with DC_LOSS_* — is
 *  additive within 5: no symbol, struct name or op kind changed, and a caller that zero-initialises the structs gets DC_LOSS_L2, the
 *  bits it got before)
 * (the loss weights — DC_LOSS_WEIGHTED, a flag bit of `loss`, announces a weights block BEHIND the struct in the caller's memory — are
 *  additive within 5 likewise: no struct, field, symbol or op kind changed, and without the bit nothing behind the struct is read)
 * (the learned-range step — DC_STEP_MODE_BLOCK, a flag bit of `v_param` in dc_ddpm_step_shared_params and dc_ddpm_noise_map_params,
 *  announces a mode block BEHIND the struct in the caller's memory, with DC_STEP_* — is additive within 5 likewise: no struct, field,
 *  symbol or op kind changed, and without the bit nothing behind the struct is read: the kernel instance and the bits as before) */
#define DC_ABI_VERSION 5

typedef void* dc_stream; /* hipStream_t */

typedef enum { DC_OK = 0, DC_ERR_ARG = -1, DC_ERR_SHAPE = -2, DC_ERR_DTYPE = -3,
               DC_ERR_ALIGN = -4, DC_ERR_LAUNCH = -5, DC_ERR_UNSUPPORTED = -6 } dc_status;

typedef enum { DC_F32 = 0, DC_BF16 = 1, DC_F16 = 2 } dc_dtype;

typedef enum { DC_ACT_NONE = 0, DC_ACT_SILU = 1, DC_ACT_GEGLU = 2, DC_ACT_GELU_TANH = 3 } dc_act;

int dc_abi_version(void);
const char* dc_last_error(void);
/* "gfx950" — the only code object in the library. */
const char* dc_arch(void);

/* ---------------------------------------------------------------- q_sample ------- */
/* z[bj] = alpha[bj]*x[img[bj]] + sigma[bj]*eps[bj]          (reference :115)
 * x   [n_img, C, H, W] f32 NCHW;  eps [n_bj, C, H, W] f32 NCHW.
 * out: im2col==0: z as NHWC [n_bj, H, W, ld] (channels >= C are written as zero)
 *      im2col==1: 3x3 zero-padded patches [n_bj, H, W, ld], k = tap*C + c for
 *                 tap = ky*3+kx, k in [9C, ld) zero — the A operand of conv_in as a GEMM.
 * out_dtype: DC_F32 / DC_BF16 / DC_F16. */
typedef struct {
  const float* x; const float* eps; const float* alpha; const float* sigma;
  const int32_t* img_of_bj; /* [n_bj] or NULL (identity) */
  void* out; int32_t out_dtype;
  int32_t n_bj, C, H, W, ld, im2col;
  int32_t patch;            /* im2col==2: non-overlapping patch x patch tokens [n_bj, H/p, W/p, ld],
                               k = c*p*p + py*p + px (the A operand of DiT's patch embedding) */
} dc_qsample_params;
int dc_qsample(const dc_qsample_params* p, dc_stream s);

/* out[r, i] ~ N(0,1) for r < rows, i < row_len (multiple of 4): Philox4x32-10 with key = seed and
 * counter = row_ids[r]*(row_len/4) + i/4 (row_ids NULL: r), Box-Muller.  The value of a row
 * depends only on (seed, row id), so sharding rows across GPUs never changes the noise. */
int dc_philox_normal(float* out, int64_t rows, int64_t row_len, const int64_t* row_ids, uint64_t seed, dc_stream s);

/* ---------------------------------------------------------------- sinusoid ------- */
/* emb[i, :] = [cos(lam_i*w_k), sin(lam_i*w_k)] (flip) or [sin, cos]; w_k = exp(-ln(1e4)*k/(half-shift)) */
typedef struct { const float* lam; float* out; int32_t n, dim, flip_sin_to_cos; float freq_shift; } dc_sinusoid_params;
int dc_sinusoid(const dc_sinusoid_params* p, dc_stream s);

/* ---------------------------------------------------------------- igemm ---------- */
/* Implicit GEMM on MFMA: conv 3x3 (pad 1, stride 1|2, optional nearest-2x upsample folded
 * into the gather, optional channel-concat of two sources) or a plain GEMM / 1x1 conv
 * (taps = 1).  Activations are NHWC: rows = n_img*Hout*Wout, K = taps*(C0+C1).
 *   out[row, co] = epilogue( sum_k A[row,k] * Wp[co,k] )
 * epilogue: (+bias[co]) (+rowvec[vmap[n]][co]) -> act -> (*gate[gmap[n]][co]) (+residual[row,co])
 * DC_ACT_GEGLU takes bias and residual only: with rowvec or gate set dc_igemm returns DC_ERR_ARG (the text names the field).
 * A/W dtype = dtype (f32 uses v_mfma_f32_16x16x4_f32; bf16/f16 use 16x16x32).
 * W is packed [Cout_pad][K] (K contiguous, k = tap*(C0+C1) + c), Cout_pad = multiple of the
 * kernel's N tile (dc_igemm_cout_pad), zero filled.  For DC_ACT_GEGLU the packed rows
 * interleave 16-row blocks of the value half and the gate half (see dc_igemm docs in
 * DESIGN.md) and the output has Cout/2 channels.
 * Constraints: C0, C1 multiples of 128/sizeof(dtype) elements (32 f32 / 64 bf16,f16). */
typedef struct {
  int32_t dtype, taps, stride, upsample;
  int32_t n_img, Hin, Win, Hout, Wout;      /* Hin/Win: conv input size AFTER upsample */
  const void* src0; const int32_t* map0; int32_t C0, ld0;  /* ld: pixel stride in elements (0: = C) */
  const void* src1; const int32_t* map1; int32_t C1, ld1;
  const void* W; int32_t Cout, tile_n;      /* tile_n: 128 or 32 (packing granularity) */
  const float* bias;
  const float* rowvec; const int32_t* rowvec_map; int32_t rowvec_ld, act;
  const float* gate; const int32_t* gate_map; int32_t gate_ld, pad2_;
  const void* residual; const int32_t* res_map; int32_t res_dtype, res_ld;
  void* out; int32_t out_dtype, out_ld;
  /* fused GroupNorm(+SiLU) prologue on the A operand: a[n,y,x,c] := act(a*gn_scale[n][c] + gn_shift[n][c]) for
   * real pixels (conv padding stays 0).  Only where dc_igemm_gn_fusable() says so (3x3 halo kernel, one sample
   * per workgroup, C0+C1 <= 512; or the thin-output 3x3 conv, Cout <= 16 on images >= 16x16: conv_norm_out + conv_out
   * as one launch, rounded exactly as the GroupNorm kernel rounds); NULL otherwise. */
  const float* gn_scale; const float* gn_shift; int32_t gn_silu, pad3_;
  /* optional 1x1 side source summed into the same output (a ResNet's conv_shortcut folded into its conv2):
   * out += sum_c A2[row, c] * W2p[co, c], A2 = src2 [*, Hout, Wout, C2] read through map2, W2p packed [Cout_pad][C2].
   * Only where dc_igemm_side_ok() says so (3x3 stride-1 halo kernel, no upsample); NULL / 0 otherwise. */
  const void* src2; const int32_t* map2; const void* W2; int32_t C2, ld2;
  /* ln_eps > 0: each A row is LayerNorm-ed on the fly, a := (a - mean(a)) * rsqrt(var(a) + ln_eps) over its K channels, no
   * affine (fold gamma into W's columns and beta into the bias when packing).  Only where dc_igemm_ln_ok() says so (the
   * activation-stationary GEMM: 1 tap, one source, K <= 512, 16-bit). */
  float ln_eps;
  /* up4 = 1 (only with upsample = 1, where dc_igemm_up4_ok() says so): W holds the four-phase form of the 3x3 weights,
   * [phase = 2a+b][Cout_pad][(dy*2+dx) * C + c], in which output pixel (2y+a, 2x+b) = sum over the 2x2 source pixels
   * (y+a-1+dy, x+b-1+dx) — the 3x3 taps that read the same source pixel of the nearest-2x upsampled image are summed
   * when packing (row taps: a=0 -> (k0 | k1+k2), a=1 -> (k0+k1 | k2); columns alike).  4/9 of the MACs, same result up
   * to the rounding of the summed weights. */
  int32_t up4;
  /* quad statistics of the OUTPUT for a following GroupNorm (dc_groupnorm_params.qstats): per output sample n, per part (a run
   * of HW / qparts pixels) and per quad q of 4 consecutive output channels the mean and the centred second moment
   * M2 = sum (v - mean)^2 of the quad's 4 * HW / qparts output values (fp32, before the rounding to out_dtype; shifted sums, no
   * cancellation for |mean| >> std): qstats[((n * qparts + part) * (Cout/4) + q) * 2 + (0 = mean | 1 = M2)],
   * qparts = dc_igemm_qstats_parts().  The GroupNorm then streams the tensor once instead of reading it twice.  NULL otherwise.
   * Which pixels a part holds: images of at most 32 columns — part i is the row-major run [128 i, 128 i + 128) (one part: the whole
   * image); wider images are cut into blocks of 8 rows x 32 columns, blocks in row-major order, and every block is two parts, its
   * upper 4 rows before its lower 4.  up4: parts [phase * qparts/4, (phase + 1) * qparts/4), phase = 2a + b, are those of the
   * low-resolution image by the same rule and hold the output pixels (2y+a, 2x+b).  (Every part has the same count, so a consumer
   * that merges all parts of a sample need not know this.) */
  float* qstats;
  /* producer-side GroupNorm (only where dc_igemm_pn_ok() says so: 3x3 stride-1 conv on power-of-two images of 16x16 ... 64x64, one
   * source, Cout a multiple of 128): besides — or, with out == NULL, instead of — the raw output v the conv stores
   *   pn_out[row, co] = act( (v - mean_g) * rstd_g * pn_gamma[co] + pn_beta[co] ),   act = SiLU if pn_silu else identity,
   * the GroupNorm over pn_groups groups of Cout / pn_groups consecutive channels and all Hout*Wout pixels of the sample (fp32
   * statistics from the fp32 accumulators, the same (mean, M2) quad records and the same fold dc_groupnorm uses; eps = pn_eps), in
   * the compute dtype with row stride pn_ld (0: = Cout).  The consumer of that GroupNorm then reads pn_out with a plain conv / GEMM
   * and the GroupNorm pass over the tensor never runs.  qstats must be given (dc_igemm_qstats_parts() parts per sample: the workgroups
   * of a sample exchange their records through it); pn_cnt: n_img * ceil(Cout / 128) uint32 arrival counters that belong to THIS
   * call site: zeroed once by the caller, then left alone — they only ever grow (every launch adds Hout*Wout/256 to each), which is
   * what makes a stale read of one harmless.  A wait that never completes cannot hang the device: it times out and is counted (dc_pn_timeouts). */
  void* pn_out; const float* pn_gamma; const float* pn_beta; uint32_t* pn_cnt;
  int32_t pn_ld, pn_groups, pn_silu; float pn_eps;
} dc_igemm_params;
int dc_igemm(const dc_igemm_params* p, dc_stream s);
int32_t dc_igemm_cout_pad(int32_t cout, int32_t tile_n);
/* Name of the kernel dc_igemm would launch for these parameters, e.g. "conv3_halo<bf16,4w>",
 * "igemm_pipe<bf16,256x128,3st>" (measurement / profiling only; static string). */
const char* dc_igemm_variant(const dc_igemm_params* p);
/* The template instance behind that name (measurement / tests only; static string).  The three halo-tile 3x3 kernels:
 * "conv3_halo_kernel<T,NW,NTAP,MODE[,stag][,pn]>" (NW waves; NTAP 9, or 4 for up4; MODE 0 per-lane addresses, 1 buffer-descriptor loaders,
 * 2 mosaic of images below 8x8; stag: the staggered tap loop; pn: producer-side GroupNorm), "conv3_thin_kernel<T,gn|plain>",
 * "conv3_ws_kernel<T,gn|plain>"; every other kernel, a refusal and invalid parameters: what dc_igemm_variant returns.  geom, where not
 * NULL and the kernel is one of those three, receives 14 ints, the patch geometry of the launch:
 *   tw, th, ni (tile width / height, images per patch), tiles_x, tiles_y (tiles per image), hw (halo width), HR (halo rows per patch),
 *   nxl (halo loads per lane), mos (mosaic), xbuf (buffer-descriptor loaders), sws (chunk swizzle shift), lpt (log2 of the tiles per
 *   image), tiles_m (patches x tiles per image), grid (workgroups). */
const char* dc_igemm_instance(const dc_igemm_params* p, int32_t* geom);
/* 1 when dc_igemm can take gn_scale/gn_shift for this problem (the other fields as for dc_igemm). */
int32_t dc_igemm_gn_fusable(const dc_igemm_params* p);
/* 1 when dc_igemm can take the 1x1 side source src2 / W2 for this problem. */
int32_t dc_igemm_side_ok(const dc_igemm_params* p);
/* 1 when dc_igemm can take ln_eps (row LayerNorm of the A operand) for this problem. */
int32_t dc_igemm_ln_ok(const dc_igemm_params* p);
/* > 0: dc_igemm can emit qstats for this problem, with that many parts per sample (3x3 halo kernel, output stored in the
 * compute type, Cout a multiple of 8); 0: it cannot. */
int32_t dc_igemm_qstats_parts(const dc_igemm_params* p);
/* 1 when dc_igemm can take pn_out / pn_groups (producer-side GroupNorm) for this problem. */
int32_t dc_igemm_pn_ok(const dc_igemm_params* p);
/* Number of waves whose wait inside a producer-side-GroupNorm launch timed out since the last call (0 = every launch was sound);
 * reads and clears a device-side counter: SYNCHRONISES with the device.  Non-zero means results of those launches are invalid. */
int32_t dc_pn_timeouts(void);
/* 1 when dc_igemm can take up4 = 1 (four-phase upsample conv) for this problem. */
int32_t dc_igemm_up4_ok(const dc_igemm_params* p);

/* Tail fold: a 3x3 conv with a producer-side GroupNorm whose normalised output has ONE reader, a bias-only 3x3 stride-1 conv of at most
 * 3 output channels (a UNet's last ResNet conv -> conv_norm_out -> SiLU -> conv_out), computes that reader itself:
 *   pred[row, co] = bias[co] + sum over the 9 taps and 128 channels of Wt[tap * Co + co][c] * y[row + tap offset, c],
 *   y = act(GroupNorm(v)) rounded to the compute type exactly as pn_out would have held it (zero outside the image),
 * and neither v nor y is ever stored.  `conv` describes the producing conv as for dc_igemm with out = pn_out = NULL and its pn_* fields
 * unused (qstats must be given: the workgroups of a sample exchange their records through it); the GroupNorm and the folded conv are
 * described here.  Wt: the folded conv's weights in the compute type, [32][128], row tap * Co + co (tap = 3 ky + kx) over the 128 input
 * channels, rows from 9 * Co on zero; packed once, it depends on the weights only.  pred: fp32, row stride pred_ld >= Co.  ring: fp32
 * scratch of as many floats as the ring_floats query below returns (each tile's sums for the pixels just outside it; a second,
 * stream-ordered launch inside the call adds them to the border pixels in ascending tile order, so results are bit-identical from
 * call to call).  cnt: as dc_igemm_params.pn_cnt (n_img counters, zeroed once, owned by this call site).  Neither ring nor cnt may
 * live in memory that other ops of the same stream reuse.  Served: 16-bit compute types, Cout = 128, 1 <= Co <= 3, whatever
 * dc_igemm_pn_ok accepts for the conv on images of 16x16 ... 64x64; everything else keeps the separate thin conv.  Additive within
 * version 5. */
typedef struct {
  const void* Wt; const float* bias; float* pred; float* ring;
  const float* gamma; const float* beta; uint32_t* cnt;
  int32_t Co, pred_ld, groups, silu; float eps; int32_t pad_;
} dc_pn_tail_params;
int dc_conv3_pn_tail(const dc_igemm_params* conv, const dc_pn_tail_params* tail, dc_stream s);
/* 1 when dc_conv3_pn_tail serves this pair (pointers may be NULL: nothing is touched). */
int32_t dc_conv3_pn_tail_ok(const dc_igemm_params* conv, const dc_pn_tail_params* tail);
/* "conv3_halo<bf16,4w,pn,tail>" / "conv3_halo<f16,4w,pn,tail>", or the reason of the refusal (static string). */
const char* dc_conv3_pn_tail_variant(const dc_igemm_params* conv, const dc_pn_tail_params* tail);
/* Floats of `ring` for this pair (0: not served): n_img x tiles per image x (2 (tw + 2) + 2 th) x Co for th x tw tiles. */
int64_t dc_conv3_pn_tail_ring_floats(const dc_igemm_params* conv, const dc_pn_tail_params* tail);
/* what DC_OP_CONV3_PN_TAIL points to */
typedef struct { const dc_igemm_params* conv; const dc_pn_tail_params* tail; } dc_conv3_pn_tail_op;

/* ---------------------------------------------------------------- weight packing - */
/* dc_igemm consumes weights as [Cout_pad][K] in the compute dtype, K contiguous, rows zero-padded to the N tile
 * (Cout_pad = dc_igemm_cout_pad(cout, tile_n)).  These entry points build that form on the device from the framework's fp32
 * parameter tensors (device pointers, row-major, diffusers layouts); run once per (weights, dtype).  All buffers caller-owned;
 * dc_packed_bytes gives the size of a packed [Cout_pad][K] buffer.
 *   matrix   Linear / Conv2d 1x1 weight [cout, K]: out[r][k] = w[row_perm ? row_perm[r] : r][k] * (col_scale ? col_scale[k] : 1),
 *            columns K..kpad-1 zero (kpad >= K: conv_in's K = 9*Cin is padded to the 128-byte K granule).  col_scale folds a
 *            LayerNorm gamma into the consumer GEMM (dc_igemm ln_eps); dc_fold_layernorm_bias gives the matching bias W beta + c.
 *   conv3x3  Conv2d weight [cout, cin, 3, 3], input-channel slice [c_lo, c_hi): out[r][tap*C + c], tap = ky*3 + kx, C = c_hi - c_lo
 *            (a slice: the two halves of a skip-connection conv, conv(cat(a, b)) = conv_a(a) + conv_b(b)).
 *   up4      the four-phase form of "nearest-2x upsample, then 3x3 conv" (dc_igemm_params.up4): out[2a+b][r][(dy*2+dx)*cin + c] =
 *            fp32 sum of the 3x3 taps that read source pixel (y+a-1+dy, x+b-1+dx) — rows a=0: {k0} | {k1,k2}, a=1: {k0,k1} | {k2},
 *            columns alike; buffer = 4 x dc_packed_bytes(cout, 4*cin).
 *   geglu    GEGLU projection [2*n_half, K] (+ bias [2*n_half]): packed row 32*blk + i = value row 16*blk + i (i < 16), gate row
 *            n_half + 16*blk + i - 16 otherwise, so value and gate of a channel meet in one lane of the epilogue; optional LayerNorm
 *            fold (gamma into the columns, out_bias = permuted (bias + W beta)); perm_ws: int32[2*n_half] scratch. */
int64_t dc_packed_bytes(int32_t cout, int32_t K, int32_t dtype, int32_t tile_n);
int dc_pack_weights_matrix(const float* w, int32_t cout, int32_t K, int32_t kpad, const int32_t* row_perm, const float* col_scale,
                           void* out, int32_t dtype, int32_t tile_n, dc_stream s);
int dc_pack_weights_conv3x3(const float* w, int32_t cout, int32_t cin, int32_t c_lo, int32_t c_hi, int32_t kpad, void* out,
                            int32_t dtype, int32_t tile_n, dc_stream s);
int dc_pack_weights_up4(const float* w, int32_t cout, int32_t cin, void* out, int32_t dtype, int32_t tile_n, dc_stream s);
int dc_pack_weights_geglu(const float* w, const float* bias, int32_t n_half, int32_t K, const float* ln_gamma, const float* ln_beta,
                          void* out_w, float* out_bias, int32_t* perm_ws, int32_t dtype, dc_stream s);
/* out_bias[r] = (bias ? bias[r] : 0) + sum_k w[r][k] * ln_beta[k]   (fp32, k ascending) */
int dc_fold_layernorm_bias(const float* w, const float* bias, const float* ln_beta, int32_t cout, int32_t K, float* out_bias, dc_stream s);

/* ---------------------------------------------------------------- norms ---------- */
/* GroupNorm over (C/groups)*HW per (sample, group), NHWC, optional SiLU.  fp32 statistics carried as (mean, M2) sets
 * merged with Chan's update in a fixed order (shifted per-thread sums): no sum / sum-of-squares cancellation.
 * ws: float workspace >= dc_groupnorm_ws_floats(n, groups, splits). */
typedef struct {
  const void* x; const int32_t* map0;   /* source 0: [*, HW, C] ; map: sample -> source sample or NULL */
  const void* x1; const int32_t* map1;  /* optional source 1 (channel concat after source 0), C1 channels */
  void* y; int32_t dtype, out_dtype;    /* y: [n, HW, C+C1] */
  int32_t n, HW, C, C1, groups, silu, splits; float eps;
  const float* gamma; const float* beta; float* ws;
  /* statistics-only mode (y == NULL): instead of normalising, write the per-(sample, channel) affine
   * out_scale[n][C+C1] = rstd*gamma and out_shift = beta - mean*rstd*gamma, which dc_igemm applies on the
   * fly (gn_scale / gn_shift) — the normalised tensor is then never written to HBM. */
  float* out_scale; float* out_shift;
  /* statistics already formed by the producer of x (dc_igemm_params.qstats; qparts parts per sample, qparts divides HW):
   * single source (C1 == 0), (C/groups) a multiple of 4.  The statistics sweep is skipped; in statistics-only mode the tensor
   * is not read at all (x is then only the sample count's witness).  NULL / 0 otherwise. */
  const float* qstats; int32_t qparts, pad_;
} dc_groupnorm_params;
int dc_groupnorm(const dc_groupnorm_params* p, dc_stream s);
/* Name of the launch sequence dc_groupnorm would run for these parameters: "qaffine", "stats", "wave", "span", "qfold+span", "image",
 * "stats+apply" or "qfold+apply"; "invalid" when dc_groupnorm would refuse them (measurement / tests only; static string; touches no
 * memory). */
const char* dc_groupnorm_variant(const dc_groupnorm_params* p);
int64_t dc_groupnorm_ws_floats(int32_t n, int32_t groups, int32_t splits);
int32_t dc_groupnorm_splits(int32_t n, int32_t HW, int32_t C);
/* Workspace bytes per op (only GroupNorm needs one; the others keep everything in registers / LDS and return 0). */
int64_t dc_workspace_bytes_groupnorm(const dc_groupnorm_params* p);
int64_t dc_workspace_bytes_igemm(const dc_igemm_params* p);

/* LayerNorm over C per row. gamma/beta may be NULL.  If scale/shift given (adaLN):
 * y = ln(x)*(1+scale[m[n]][c]) + shift[m[n]][c], n = row / rows_per_sample. */
typedef struct {
  const void* x; void* y; int32_t dtype, out_dtype;
  int32_t rows, C, rows_per_sample, mod_ld; float eps;
  const float* gamma; const float* beta;
  const float* scale; const float* shift; const int32_t* mod_map;
} dc_layernorm_params;
int dc_layernorm(const dc_layernorm_params* p, dc_stream s);
/* Name of the kernel dc_layernorm would launch for these parameters: "ln16x2", "ln16" or "ln"; "invalid" when dc_layernorm would
 * refuse them (measurement / tests only; static string; touches no memory). */
const char* dc_layernorm_variant(const dc_layernorm_params* p);
int64_t dc_workspace_bytes_layernorm(const dc_layernorm_params* p);

/* ---------------------------------------------------------------- attention ------ */
/* softmax(q k^T * scale) v per (sample, head).  q/k/v: [n, L, heads, d] with row stride
 * ld (elements) so a fused QKV GEMM output can be passed as three offset pointers.
 * scale must be > 0 (DC_ERR_ARG otherwise): the kernels take the running max on the raw scores.
 * Head dims d = 16, 32, 64, 96, 128 (DC_ERR_SHAPE otherwise); 96 is the UNets' 768-channel level with 8 heads.  Other widths
 * up to 128 run as the next of these with zero pad channels in q/k/v (the scale stays that of the true width): the pad adds
 * nothing to the scores and its output columns are zero.
 * Routes in 16-bit: L <= 64 one wave per (sample, head) (d = 32 / 64 / 128), L <= 128 the whole-sequence matrix-core kernel,
 * longer sequences the flash kernel (d = 32 / 64 / 96 / 128); fp32 and the shapes those do not take: the exact fp32 kernel.
 * Unaligned operands (16-bit q / k / v not 16-byte aligned, or ld_qkv % 8 != 0): the exact fp32 kernel. */
typedef struct {
  const void* q; const void* k; const void* v; void* out;
  int32_t dtype, n, L, heads, d, ld_qkv, ld_out; float scale;
} dc_attention_params;
int dc_attention(const dc_attention_params* p, dc_stream s);
/* Name of the kernel dc_attention would launch for these parameters: "wave", "mfma" (whole sequence), "flash" or "fp32";
 * "invalid" when dc_attention would refuse them (measurement / tests only; static string). */
const char* dc_attention_variant(const dc_attention_params* p);
int64_t dc_workspace_bytes_attention(const dc_attention_params* p);

/* The same arithmetic for heads of d = 256 or 512 channels (DC_ERR_SHAPE otherwise): the mid-block attention of an AutoencoderKL
 * encoder, one head as wide as the level.  Fields, layout, scale > 0 and the error codes as for dc_attention; L >= 1 of any size.
 * Routes: "wide", 16-bit with q / k / v 16-byte aligned, ld_qkv % 8 == 0, out 8-byte aligned and ld_out % 4 == 0 — one workgroup
 * of four waves per (sample, head, 32 queries), wave w on channels [w d/4, (w+1) d/4) of the score product and of the output, the four
 * partial score tiles summed through LDS in a fixed order, P rounded to the compute type for P.V only; "fp32", everything else — the
 * exact fp32 kernel.  No atomics: out[i] depends on sample i's rows only. */
typedef struct {
  const void* q; const void* k; const void* v; void* out;
  int32_t dtype, n, L, heads, d, ld_qkv, ld_out; float scale;
} dc_attention_wide_params;
int dc_attention_wide(const dc_attention_wide_params* p, dc_stream s);
/* "wide" or "fp32"; "invalid" when dc_attention_wide would refuse the parameters (measurement / tests only; static string). */
const char* dc_attention_wide_variant(const dc_attention_wide_params* p);

/* ---------------------------------------------------------------- im2col, stride 2  */
/* out[i, oy, ox, (ky*3 + kx)*C + c] = x[i, 2*oy + ky, 2*ox + kx, c], zero where 2*oy + ky >= H or 2*ox + kx >= W: the A operand of a
 * stride-2 3x3 conv padded at the bottom and right only (AutoencoderKL's downsampler), which then runs as a 1x1 dc_igemm over
 * K = 9 C with weights [Cout, (ky, kx, c)].  x [n, H, W, C] with row stride ld (elements); out [n, H/2, W/2, 9 C] dense; one dtype
 * (DC_F32 / DC_BF16 / DC_F16).  H and W must be even (DC_ERR_SHAPE).  16-byte moves where x and out are 16-byte aligned and C and ld
 * are multiples of 16 bytes, element moves otherwise. */
typedef struct { const void* x; void* out; int32_t dtype, n, H, W, C, ld; } dc_im2col_s2_params;
int dc_im2col_s2(const dc_im2col_s2_params* p, dc_stream s);

/* ---------------------------------------------------------------- latent im2col    */
/* The head of the AutoencoderKL decoder, one pass from the scaled latents to the A operand of decoder.conv_in as a GEMM.  Per pixel
 *   u[i, :, y, x] = Q (z[i, :, y, x] * inv_scale + shift) + bias        fp32, channels ascending, no contraction
 * (Q, bias: post_quant_conv; the identity and zeros for a VAE without one), then
 *   out[i, y, x, tap*Z + c] = u[i, c, y + tap/3 - 1, x + tap%3 - 1]     in out_dtype, tap = 0..8
 * with exact zeros for taps outside the image and for the columns [9 Z, Kpad): the column order of dc_qsample's im2col = 1, so
 * dc_pack_weights_conv3x3(..., kpad = Kpad) serves conv_in.  A 1x1 conv with a bias in front of a zero-padded 3x3 conv is not a 3x3
 * conv (the padded taps carry no bias), hence a kernel and no weight fold; the operand is rounded to out_dtype once.
 * z [n, Z, H, W] f32 NCHW, Q [Z, Z] f32 row-major, bias [Z] f32, out [n, H, W, Kpad] dense, 16-byte aligned.  Kpad >= 9 Z and a
 * multiple of dc_igemm's K granule (32 for DC_F32, 64 for the 16-bit types), else DC_ERR_SHAPE.  16-byte stores, no atomics; the rows
 * of sample i depend on sample i only. */
typedef struct {
  const float* z; const float* Q; const float* bias; void* out;
  int32_t out_dtype, n, Z, H, W, Kpad; float inv_scale, shift;
} dc_latent_im2col_params;
int dc_latent_im2col(const dc_latent_im2col_params* p, dc_stream s);

/* ---------------------------------------------------------------- cross-attention */
/* out[i] = softmax(q[q_map[i]] k[kv_map[i]]^T * scale) v[kv_map[i]] per head, for i < n: attention whose keys and values come from
 * another tensor with its own length (the prompt of a unit, picked through ctx_of_unit) and whose queries may be shared (the
 * class-shared trunk keeps them once per (image, trial) pair: bj_of_unit).  A map of NULL is the identity.
 * q [*, Lq, heads, d] with row stride ld_q, k / v [*, S, heads, d] with row stride ld_kv (a stacked K | V GEMM output is passed as two
 * offset pointers), out [n, Lq, heads, d] with row stride ld_out; all in `dtype`.  Every one of the S keys is attended (the reference
 * passes no mask, so padded prompt rows take part; dc_cross_attention_len below takes a key count per context).  Rows behind the S-th
 * of a context are never read.
 * scale must be > 0 and S >= 1 (DC_ERR_ARG / DC_ERR_SHAPE); head dims d = 16, 32, 64, 96, 128, 160 (DC_ERR_SHAPE otherwise), narrower
 * heads zero-padded by the caller exactly as for dc_attention (scale of the true width; the pad columns of the output are zero).
 * q / k / v / out must be aligned to their element and q_map / kv_map (and kv_len below) to 4 bytes (DC_ERR_ALIGN).
 * 160 is Stable Diffusion 1.x's 1280-channel level in 8 heads; its self-attention is this function too: q / k / v the three column
 * offsets of the fused QKV tensor, Lq = S = L, ld_q = ld_kv, both maps NULL (dc_attention serves no 160).
 * 16-bit with d = 32 / 64 / 96 / 128 / 160 and 16-byte aligned rows: the matrix-core kernel (one wave per 32 queries of a (sample, head),
 * online softmax over key blocks, fp32 statistics); f32, d = 16 and unaligned operands: the exact fp32 kernel.  Fixed summation
 * order, no atomics: the bits of out[i] depend on its own q rows and its own context only, not on n or on i. */
typedef struct {
  const void* q; const void* k; const void* v; void* out;
  const int32_t* q_map; const int32_t* kv_map;          /* NULL = identity */
  int32_t dtype, n, Lq, S, heads, d, ld_q, ld_kv, ld_out; float scale;
} dc_cross_attention_params;
int dc_cross_attention(const dc_cross_attention_params* p, dc_stream s);
/* Name of the kernel dc_cross_attention would launch for these parameters: "mfma" or "fp32"; "invalid" when it would refuse them
 * (measurement / tests only; static string; touches no memory). */
const char* dc_cross_attention_variant(const dc_cross_attention_params* p);

/* dc_cross_attention over prompts of different lengths.  k / v keep the padded layout (context c starts at row c * S); output sample
 * i, with context c = kv_map ? kv_map[i] : i, attends keys 0 .. kv_len[c] - 1 of it only: masking keys >= kv_len[c] out of the
 * softmax, which is attending the prompt truncated to kv_len[c] tokens.  Rows kv_len[c] .. S - 1 of a context are never read, key
 * blocks wholly past the length are skipped, and the surviving keys keep their blocks: the bits of out[i] are those dc_cross_attention
 * gives for a context of S = kv_len[c] rows.  kv_len [number of contexts] int32 on the device; NULL: every context has S keys (the
 * launch of dc_cross_attention).  A length is device data the host cannot see without a synchronisation: the kernels clamp it into
 * [1, S] (no read outside the context's own rows, no empty softmax); validate lengths where they are produced.  Every other argument
 * is validated and routed as for dc_cross_attention (same codes; messages under this function's name).  There is no mask with holes
 * and no per-query mask. */
typedef struct {
  const void* q; const void* k; const void* v; void* out;
  const int32_t* q_map; const int32_t* kv_map;          /* NULL = identity */
  const int32_t* kv_len;                                /* keys per context; NULL = S everywhere */
  int32_t dtype, n, Lq, S, heads, d, ld_q, ld_kv, ld_out; float scale;
} dc_cross_attention_len_params;
int dc_cross_attention_len(const dc_cross_attention_len_params* p, dc_stream s);
/* As dc_cross_attention_variant: "mfma", "fp32" or "invalid" (the routing does not depend on kv_len). */
const char* dc_cross_attention_len_variant(const dc_cross_attention_len_params* p);

/* ---------------------------------------------------------------- T5 encoder ----- */
/* Self-attention with an additive relative-position bias and a row count per sample (T5's attention under a right-padded mask):
 *   out[i] = softmax(q_i k_i^T * scale + bias[h][k - q + L - 1]) v_i   over keys k < kv_len[i], for queries q < kv_len[i].
 * q / k / v / out as for dc_attention: [n, L, heads, d] with row strides ld_qkv / ld_out (elements), one `dtype`.
 * bias [heads][2L - 1] fp32 on the device, indexed by the relative distance k - q + L - 1 (built on the host: a bucket boundary must not
 * depend on a device logarithm).  kv_len [n] int32 on the device, NULL meaning L everywhere; the kernels clamp it into [1, L].
 * Rows >= kv_len[i] of q / k / v are never read (staged as zeros and masked: 0 x garbage cannot make a NaN) and output rows >= kv_len[i]
 * are written as zeros.  scale must be > 0 (DC_ERR_ARG; T5 passes 1.0); 1 <= L <= DC_ATTENTION_BIAS_MAX_L and d in {16, 32, 64, 128}
 * (DC_ERR_SHAPE otherwise).
 * Routes: 16-bit with d = 64, 16-byte aligned q / k / v rows and 8-byte aligned output rows: the matrix-core kernel "mfma" (one wave per
 * 32 queries of a (sample, head), online fp32 softmax over key blocks of 32, the wave's slice of the table in LDS); fp32, d = 16 / 32 /
 * 128 and unaligned operands: the exact kernel "fp32".  (d = 32 / 128 would come from the matrix-core template too; they are not
 * instantiated, no T5 v1.0 shape has them.)  Fixed summation order, no atomics: the bits of out[i] depend on sample i's own rows, its
 * own length and the table only, not on n or on i. */
#define DC_ATTENTION_BIAS_MAX_L 512
typedef struct {
  const void* q; const void* k; const void* v; void* out;
  const float* bias;                                    /* [heads][2L - 1] */
  const int32_t* kv_len;                                /* rows per sample; NULL = L everywhere */
  int32_t dtype, n, L, heads, d, ld_qkv, ld_out; float scale;
} dc_attention_bias_params;
int dc_attention_bias(const dc_attention_bias_params* p, dc_stream s);
/* Name of the kernel dc_attention_bias would launch for these parameters: "mfma" or "fp32"; "invalid" when it would refuse them
 * (measurement / tests only; static string; touches no memory). */
const char* dc_attention_bias_variant(const dc_attention_bias_params* p);

/* RMS norm (T5LayerNorm: no mean subtraction, no bias): y[r, c] = x[r, c] * rsqrt(mean_c(x[r, :]^2) + eps) * weight[c].  fp32
 * statistics; x [rows, C] is read in `dtype`, y written in `out_dtype` (the encoder's residual stream is fp32, the GEMM that follows
 * reads the compute type).  row_len [rows / rows_per_sample] int32 on the device or NULL: rows whose index inside their sample is
 * >= row_len[sample] are written as zeros and not read. */
typedef struct {
  const void* x; void* y; const float* weight; const int32_t* row_len;
  int32_t dtype, out_dtype, rows, C, rows_per_sample; float eps;
} dc_rmsnorm_params;
int dc_rmsnorm(const dc_rmsnorm_params* p, dc_stream s);

/* out[r, :] = table[ids[r], :] for r < rows: fp32 table [vocab, C], int64 ids on the device, out [rows, C] in out_dtype.  Ids are
 * validated on the host where they enter; the kernel clamps them into [0, vocab) so that nothing outside the table is read. */
typedef struct {
  const float* table; const int64_t* ids; void* out;
  int32_t out_dtype, rows, C, vocab;
} dc_embed_rows_params;
int dc_embed_rows(const dc_embed_rows_params* p, dc_stream s);

/* x[i] = max(x[i], 0) in place for i < n (NaN stays NaN), 16-byte chunks; x 16-byte aligned.  One extra pass over the feed-forward's
 * [rows, d_ff]: it exists so that dc_igemm and its shared epilogue stay untouched; ReLU as a dc_igemm activation is the follow-up to
 * measure. */
typedef struct { void* x; int64_t n; int32_t dtype, pad_; } dc_relu_params;
int dc_relu(const dc_relu_params* p, dc_stream s);

/* ---------------------------------------------------------------- CLIP text encoder ----- */
/* Causal self-attention with a row count per sample (CLIP's text transformer under a right-padded mask):
 *   out[i] = softmax(q_i k_i^T * scale over keys k <= q) v_i   for queries q < row_len[i].
 * q / k / v / out as for dc_attention_bias: [n, L, heads, d] with row strides ld_qkv / ld_out (elements), one `dtype`.
 * row_len [n] int32 on the device, NULL meaning L everywhere; the kernels clamp it into [1, L].  Causality already hides every key at
 * or past the length from every query below it, so the length only decides which rows exist: rows >= row_len[i] of q / k / v are never
 * read and output rows >= row_len[i] are written as zeros.  scale must be > 0 (DC_ERR_ARG); 1 <= L <= DC_ATTENTION_CAUSAL_MAX_L and
 * d in {16, 32, 64, 128} (DC_ERR_SHAPE otherwise).
 * Routes: 16-bit with d = 64, 16-byte aligned q / k / v rows and 8-byte aligned output rows: the matrix-core kernel "mfma" (one wave per
 * 32 queries of a (sample, head); it walks the key blocks up to its own diagonal block only and masks inside that block alone); fp32,
 * d = 16 / 32 / 128 and unaligned operands: the exact kernel "fp32" (an FMA chain over the keys 0 .. q in order).  Fixed summation
 * order, no atomics: the bits of output row q of sample i depend on rows 0 .. q of sample i only.  (Masked positions carry P = 0
 * exactly; on the matrix-core route a NON-FINITE v row above q, below row_len[i] and inside q's own block of 32 rows still reaches row
 * q as 0 x NaN.  Rows at or past row_len[i] — what padding is — are never read on either route.) */
#define DC_ATTENTION_CAUSAL_MAX_L 512
typedef struct {
  const void* q; const void* k; const void* v; void* out;
  const int32_t* row_len;                               /* rows per sample; NULL = L everywhere */
  int32_t dtype, n, L, heads, d, ld_qkv, ld_out; float scale;
} dc_attention_causal_params;
int dc_attention_causal(const dc_attention_causal_params* p, dc_stream s);
/* Name of the kernel dc_attention_causal would launch for these parameters: "mfma" or "fp32"; "invalid" when it would refuse them
 * (measurement / tests only; static string; touches no memory). */
const char* dc_attention_causal_variant(const dc_attention_causal_params* p);

/* LayerNorm with weight and bias whose input and output types differ: y[r, c] = (x[r, c] - mean_r) * rsqrt(var_r + eps) * gamma[c] +
 * beta[c], fp32 statistics (the mean, then the centred second moment) in a fixed order.  x [rows, C] is read in `dtype` (the encoder's
 * residual stream is fp32), y written in `out_dtype` (the compute type for the GEMM that follows, or fp32).  row_len
 * [rows / rows_per_sample] int32 on the device or NULL: rows whose index inside their sample is >= row_len[sample] are written as
 * zeros and not read.  (dc_layernorm requires one type for both sides and has no row_len; it stays as it is.) */
typedef struct {
  const void* x; void* y; const float* gamma; const float* beta; const int32_t* row_len;
  int32_t dtype, out_dtype, rows, C, rows_per_sample; float eps;
} dc_layernorm_rows_params;
int dc_layernorm_rows(const dc_layernorm_rows_params* p, dc_stream s);

/* out[r, :] = table[ids[r], :] + pos[r % L, :] for r < rows: fp32 tables [vocab, C] and [>= L, C], int64 ids on the device, one fp32
 * add and one rounding to out_dtype.  Ids are validated on the host where they enter; the kernel clamps them into [0, vocab). */
typedef struct {
  const float* table; const float* pos; const int64_t* ids; void* out;
  int32_t out_dtype, rows, C, vocab, L, pad_;
} dc_embed_rows_pos_params;
int dc_embed_rows_pos(const dc_embed_rows_pos_params* p, dc_stream s);

/* x[i] = act(x[i]) in place for i < n, 16-byte chunks; x 16-byte aligned.  Evaluated in fp32 with one rounding to the storage type;
 * NaN stays NaN.  DC_PASS_QUICK_GELU: x * sigmoid(1.702 x) (OpenAI CLIP's hidden_act); DC_PASS_GELU_ERF: x * Phi(x) (OpenCLIP's).
 * A pass of its own over the feed-forward's [rows, intermediate] for the reason dc_relu is one: dc_igemm, its dispatcher and the
 * shared epilogue stay untouched (dc_act is not extended); the activation inside the GEMM is the follow-up to measure. */
typedef enum { DC_PASS_QUICK_GELU = 1, DC_PASS_GELU_ERF = 2 } dc_pass_kind;
typedef struct { void* x; int64_t n; int32_t dtype, kind; } dc_act_pass_params;
int dc_act_pass(const dc_act_pass_params* p, dc_stream s);

/* ---------------------------------------------------------------- transformer block, attention half --- */
/* One launch for the self-attention half of a UNet transformer block (the backbone behind /root/reference/nets/unet.py:186-195:
 * Transformer2DModel.proj_in -> BasicTransformerBlock.norm1 -> attn1 (to_q/k/v, softmax, to_out) -> + attn2's class vector -> residual):
 *   h = x Wp^T + bp;  hn = LayerNorm(h; eps) * ln_g + ln_b;  q | k | v = hn Wqkv^T (rows [0,C) q, [C,2C) k, [2C,3C) v; head i = channels
 *   [i d, (i+1) d), d = C / heads);  o = softmax(q k^T * scale) v per (sample, head);  out = ((o Wo^T + bo) + rowvec[rowvec_map[n]]) + h.
 * x [n, L, ldx], out [n, L, ld_out] in `dtype` (16-bit); Wp / Wo [C][C], Wqkv [3C][C] packed as dc_igemm takes them (dc_pack_weights_matrix,
 * tile_n 128); biases, LayerNorm affine and rowvec fp32.  h, hn, q, k, v, p, o are rounded to `dtype` where the separate launches
 * (dc_igemm, dc_layernorm, dc_attention) store them, so results agree with that chain to accumulation order.  The softmax row sum is
 * taken over the UNROUNDED fp32 p (p is rounded only as the operand of p v), and o = round((p v) * (1 / sum)); the epilogue adds in fp32 in
 * the order written above and rounds once.
 * Optional pointers: bo null: no to_out bias (+ 0).  rowvec null: no row vector (+ 0); rowvec_ld and rowvec_map are then ignored
 * (rowvec_ld = 0 is fine).  rowvec set, rowvec_map null: sample n takes row n of a table of n rows; rowvec_map set: row rowvec_map[n]
 * (int32 on the device, any order, rows may repeat; not range-checked).  rowvec rows are rowvec_ld >= C floats apart, rowvec_ld % 4 == 0.
 * ldx, ld_out >= C and multiples of 8 (rows are moved in 16-byte pieces); only columns [0, C) of a row are read or written.
 * Status: DC_ERR_SHAPE for L / C / heads / n / ldx / ld_out / rowvec_ld < C, DC_ERR_ALIGN for a pointer off 16 bytes or rowvec_ld % 4,
 * DC_ERR_ARG for a null required pointer or scale / ln_eps <= 0 — all before any launch, the output untouched.
 * Shapes: dc_tblock_front_ok() (L = 64, C = 256, heads = 4 or 8 today); anything else returns DC_ERR_SHAPE. */
typedef struct {
  const void* x; const void* Wp; const float* bp;
  const float* ln_g; const float* ln_b;
  const void* Wqkv; const void* Wo; const float* bo;
  const float* rowvec; const int32_t* rowvec_map;
  void* out;
  int32_t dtype, n, L, C, heads, ldx, ld_out, rowvec_ld;
  float ln_eps, scale;
} dc_tblock_front_params;
int dc_tblock_front(const dc_tblock_front_params* p, dc_stream s);
int32_t dc_tblock_front_ok(const dc_tblock_front_params* p);     /* 1: the shape / dtype is served (pointers are not looked at) */

/* ---------------------------------------------------------------- eps-MSE -------- */
/* err[u] = (|| eps_hat_u - eps_{bj(u)} ||_2)^2 over C*H*W   (reference :706-711)
 * pred [n_units, H, W, ld] f32 NHWC; eps [n_bj,C,H,W], x [n_img,C,H,W] f32 NCHW.
 * v_param: eps_hat = sigma*z + alpha*pred with z = alpha*x + sigma*eps (fp32), else pred.
 * out_index: err is stored at out[out_index[u]] (NULL: out[u]). Deterministic reduction.
 * loss: the per-element term summed over C*H*W, with d = eps_hat - eps in fp32 (Li et al. evaluate l1, l2 and Huber):
 *   DC_LOSS_L2     d^2, and the sum goes through sqrt then square as above (the zero value: what every caller got before the field)
 *   DC_LOSS_L1     |d|
 *   DC_LOSS_HUBER  |d| <= huber_delta ? 0.5 d^2 : huber_delta (|d| - 0.5 huber_delta)      torch's huber_loss, summed
 * l1 and Huber store the sum as it is.  Sums, not means.  huber_delta is read for DC_LOSS_HUBER only and must then be finite and > 0;
 * an unknown kind or such a delta is DC_ERR_ARG.  A NaN element makes its unit's error NaN for every kind.
 * Weights of the loss.  `loss` may carry the flag DC_LOSS_WEIGHTED next to the kind (loss = DC_LOSS_L1 | DC_LOSS_WEIGHTED); any other
 * bit is DC_ERR_ARG.  The caller then passes the struct as the head of a larger object: directly behind it (at sizeof of the struct,
 * which is a multiple of 8) stand, in this order,
 *     const float* pixel_w;  const float* trial_w;  int32_t w_T, w_cells;
 * — the same block behind a dc_err_map_params.  It is no struct of this header on purpose: the structs and their fields are frozen
 * within version 5, and a caller that never sets the bit never has anything read behind its struct.  Without the bit: the kernels above,
 * untouched.  With t the term above,
 *   s = sum over C*H*W of m[y, x] * t(d)      m = pixel_w[img, y, x], pixel_w f32 [n_img, H, W], img = img_of_bj[bj(u)] (NULL: bj(u));
 *                                             one fp32 multiply per element, the accumulation order of the unweighted kernel
 *                                             (DC_LOSS_L2: (m d) d, the second product fused into the sum as the unweighted d d is)
 *   r = sqrt(s), r = r * r for DC_LOSS_L2, r = s otherwise;   err[u] = r * w, one fp32 multiply
 *   w = trial_w[img * T + j], trial_w f32 [n_img, T], j = out_index[u] % T, with T = w_T and cells = w_cells (dc_err_map: its own T and
 *   cells fields, which w_T / w_cells must equal); w_T > 0 and w_cells > 0 are required whenever the flag is set, a guard against a
 *   stray bit; an out_index outside [0, cells * T) — the dump slot of padded units — takes w = 1.A NULL pointer of the two is a weight of 1.  All ones give the bits of the unweighted call.
 * trial_w needs out_index, img_of_bj, T > 0 and cells > 0: DC_ERR_ARG otherwise.  Weights are data: a NaN weight makes its units NaN. */
#define DC_LOSS_WEIGHTED 256
#define DC_LOSS_L2 0
#define DC_LOSS_L1 1
#define DC_LOSS_HUBER 2
typedef struct {
  const float* pred; const float* eps; const float* x; const float* alpha; const float* sigma;
  const int32_t* bj_of_unit; const int32_t* img_of_bj; const int32_t* out_index;
  float* out; int32_t n_units, C, H, W, ld, v_param;
  int32_t patch;            /* >1: pred is DiT's un-patchified projection [n_units, H/p, W/p, ld] with
                               k = (py*p+px)*C + c (nets/dit.py un-patchify folded into the read; the feature stride is C:
                               the caller projects the eps rows only) */
  int32_t loss; float huber_delta;
} dc_eps_mse_params;
int dc_eps_mse(const dc_eps_mse_params* p, dc_stream s);

/* ---------------------------------------------------------------- sampler step --- */
/* One ancestral DDPM step with classifier-free guidance (reference :175-208 ddpm_sampler_step + the update :262-266):
 *   pred = (1 + w) * pred_c - w * pred_u;  x = v_param ? alpha_t z - sigma_t pred : (z - sigma_t pred) / alpha_t;  x = clip(x, -1, 1)
 *   mu = alpha_s * (z * (1 - c) / alpha_t + c * x);   out = noise ? mu + noise * sd : clip(mu, -1, 1)      (sd = sqrt(sigma_s^2 c))
 * z / noise / out [n, C, H, W] f32 NCHW; pred [2n, H, W, ld] f32 NHWC, rows 2b (class token) and 2b+1 (null token) of image b —
 * the output of ONE batch-2 backbone plan (patch > 1: DiT's un-patchified projection as in dc_eps_mse, whose feature stride is C:
 * the caller projects the eps rows only, also of a backbone whose out_channels is 2C).  Same operation order as the reference's torch expressions, no contraction: equal to
 * them bit for bit for the same fp32 scalars (w, one_plus_w, alpha_*, sigma_t, c, sd — formed by the caller). */
typedef struct {
  const float* z; const float* pred; const float* noise; float* out;
  int32_t n, C, H, W, ld, patch, v_param;
  float w, alpha_t, sigma_t, alpha_s, c, sd;
  float one_plus_w;        /* (float)(1.0 + (double)w): the reference forms 1 + w as a Python double and torch rounds it once */
} dc_ddpm_step_params;
int dc_ddpm_step(const dc_ddpm_step_params* p, dc_stream s);

/* The same step on n = images x K trajectories that share their noise (counterfactual sampling: K class trajectories of one image see
 * one z_{from_t} and one noise draw per step).  z / out [n, C, H, W], pred [2n, ...] as above; trajectory u adds row u / noise_div of
 * noise [n / noise_div, C, H, W] (noise NULL: the clipped mean).  The arithmetic, its order and the kernel body are dc_ddpm_step's:
 * with noise_div = 1, or on noise repeated noise_div times, the two agree bit for bit.  noise_div < 1 or n % noise_div != 0:
 * DC_ERR_ARG.
 *
 * The step mode.  `v_param` may carry the flag DC_STEP_MODE_BLOCK next to the parametrisation (v_param = 1 | DC_STEP_MODE_BLOCK); it
 * announces a mode block in the caller's memory directly behind the struct, at sizeof(dc_ddpm_step_shared_params) (a multiple of 8):
 *     int32_t mode, fstride;  float k1, k2, log_hi, log_lo;
 * (the structs of this header are frozen: the layout is that of `struct { dc_ddpm_step_shared_params base; int32_t mode, fstride;
 * float k1, k2, log_hi, log_lo; }`).  Without the flag nothing behind the struct is read.  mode = DC_STEP_FIXED: all of the above, the
 * same kernel instance and bits, the other five block fields ignored; an unknown mode: DC_ERR_ARG.  DC_STEP_LEARNED_RANGE is the improved-DDPM step of a model that predicts its variance next to eps
 * (diffusers' variance_type = "learned_range"; a published DiT): pred holds, per pixel, 2C features — eps in 0 .. C-1 and the variance
 * interpolation v in C .. 2C-1 — at feature stride fstride: feature (py*p+px)*fstride + c for patch p > 1, p*ld + c for patch <= 1.
 * Per element, in this order, no contraction:
 *   pr  = one_plus_w * pc - w * pu                        (pc, pu: the eps features of rows 2b and 2b+1)
 *   x   = v_param ? alpha_t * z - sigma_t * pr : (z - sigma_t * pr) / alpha_t                          (never clipped)
 *   mu  = k1 * z + k2 * x                                 (dc_solver_step's first-order update: the same bits)
 *   fr  = 0.5f * vc + 0.5f                                (vc: the CONDITIONAL row's feature at the same index + C; guidance mixes
 *                                                          eps only, as diffusers' DiTPipeline steps the conditional half)
 *   sde = expf(0.5f * (fr * log_hi + (1.f - fr) * log_lo))
 *   out = noise ? mu + noise * sde : mu                   (no clip on the last pass; v is not clamped)
 * with k1 = sqrt(abar_t / abar_s) (1 - abar_s) / (1 - abar_t), k2 = sqrt(abar_s) beta / (1 - abar_t), log_hi = log beta and
 * log_lo = log of the posterior variance (1 - abar_s) / (1 - abar_t) beta, beta = 1 - abar_t / abar_s, formed by the caller.  alpha_s, c
 * and sd are ignored.  fstride >= 2C and ld >= p*p*fstride (patch <= 1: ld >= 2C) or DC_ERR_SHAPE; log_hi and log_lo finite with
 * log_lo <= log_hi <= 0 or DC_ERR_ARG.  dc_ddpm_step keeps its struct: the learned-range step of unshared noise is this entry with
 * noise_div = 1. */
#define DC_STEP_MODE_BLOCK 256
#define DC_STEP_FIXED 0
#define DC_STEP_LEARNED_RANGE 1
typedef struct {
  const float* z; const float* pred; const float* noise; float* out;
  int32_t n, C, H, W, ld, patch, v_param;
  int32_t noise_div;
  float w, alpha_t, sigma_t, alpha_s, c, sd;
  float one_plus_w;
  int32_t pad_;
} dc_ddpm_step_shared_params;
int dc_ddpm_step_shared(const dc_ddpm_step_shared_params* p, dc_stream s);

/* One pass of a deterministic data-prediction solver on the same prediction pair, in the layouts dc_ddpm_step reads (z / out / xprev /
 * xhat [n, C, H, W] f32 NCHW; pred [2n, H, W, ld] f32 NHWC, rows 2b and 2b+1; patch > 1: DiT's un-patchified projection, feature
 * stride C).  Per element, in this order, no contraction:
 *   pr  = one_plus_w * pc - w * pu
 *   x   = v_param ? alpha_t * z - sigma_t * pr : (z - sigma_t * pr) / alpha_t
 *   x   = clamp ? min(max(x, -1), 1) : x
 *   if (xhat) xhat[i] = x                                  (the history of the next pass)
 *   D   = xprev ? x + k3 * (x - xprev[i]) : x
 *   out = final_pass ? min(max(D, -1), 1) : k1 * z + k2 * D
 * With h = (lam_s - lam_t) / 2, k1 = sigma_s / sigma_t and k2 = -alpha_s * expm1(-h) the first-order pass (xprev NULL, k3 unused) is
 * DDIM, z_s = alpha_s x + sigma_s (z - alpha_t x) / sigma_t, in either direction (inversion: h < 0); with xprev and
 * k3 = 0.5 * h / h_prev it is DPM-Solver++(2M).  The caller forms the scalars.  The kernel equals the torch evaluation of the same
 * expressions bit for bit for the same fp32 scalars.  xhat may be the buffer of xprev (every thread reads its element before it writes
 * it); out must not alias z (DC_ERR_ARG). */
typedef struct {
  const float* z; const float* pred; const float* xprev; float* xhat; float* out;
  int32_t n, C, H, W, ld, patch, v_param, clamp, final_pass;
  float w, one_plus_w, alpha_t, sigma_t, k1, k2, k3;
} dc_solver_step_params;
int dc_solver_step(const dc_solver_step_params* p, dc_stream s);

/* The noise map of one ancestral step (edit-friendly DDPM inversion, Huberman-Spiegelglas et al. 2024): the noise under which
 * dc_ddpm_step takes z to x_next.  Layouts and indexing are dc_ddpm_step's (z / x_next / out [n, C, H, W] f32 NCHW; pred [2n, H, W, ld]
 * f32 NHWC, rows 2b and 2b+1; patch > 1: DiT's un-patchified projection, feature stride C).  Per element, in this order, no contraction:
 *   pr  = one_plus_w * pc - w * pu
 *   x   = v_param ? alpha_t * z - sigma_t * pr : (z - sigma_t * pr) / alpha_t;   x = min(max(x, -1), 1)
 *   mu  = alpha_s * (z * (1 - c) / alpha_t + c * x)                              (dc_ddpm_step's mean: the same device code)
 *   out = (x_next - mu) / sd
 * so that dc_ddpm_step on (z, pred) with noise = out gives mu + out * sd = x_next up to the rounding of the last two operations.  The
 * kernel equals the torch evaluation of the same expressions bit for bit for the same fp32 scalars.  out may be the buffer of x_next
 * (every thread reads its element before it writes it).  NULL pointers, or an sd that is not finite and > 0: DC_ERR_ARG.
 *
 * DC_STEP_MODE_BLOCK in `v_param`: dc_ddpm_step_shared's mode block (mode, fstride, k1, k2, log_hi, log_lo) behind THIS struct, at
 * sizeof(dc_ddpm_noise_map_params); without the bit nothing behind the struct is read.  mode = DC_STEP_FIXED: all of the above, the same
 * kernel instance and bits, the other five ignored; an unknown mode: DC_ERR_ARG.  DC_STEP_LEARNED_RANGE: the map of
 * dc_ddpm_step_shared's learned-range step, in its layout (2C features per pixel at feature stride fstride) — pr, x (unclipped), mu = k1 * z + k2 * x, fr and sde exactly as written there, by the same
 * device code, then
 *   out = (x_next - mu) / sde
 * so that the learned-range step on (z, pred) with noise = out lands on x_next up to the rounding of a division and a multiply-add on
 * the same sde bits.  alpha_s, c and sd are ignored (sd is not checked); the requirements on fstride, ld, log_hi and log_lo and their
 * codes are that entry's. */
typedef struct {
  const float* z; const float* pred; const float* x_next; float* out;
  int32_t n, C, H, W, ld, patch, v_param;
  float w, one_plus_w, alpha_t, sigma_t, alpha_s, c, sd;
} dc_ddpm_noise_map_params;
int dc_ddpm_noise_map(const dc_ddpm_noise_map_params* p, dc_stream s);

/* ---------------------------------------------------------------- difference maps - */
/* out[i, y, x] = sum_c |a[i, c, y, x] - r[r_of_a[i], c, y, x]|, fp32, c ascending (a fixed order).  a [n, C, H, W], r [m, C, H, W],
 * r_of_a [n] int32 (rows may repeat and be skipped), out [n, H, W].  An r_of_a[i] outside [0, m) reads nothing and writes NaN. */
typedef struct {
  const float* a; const float* r; const int32_t* r_of_a; float* out;
  int32_t n, m, C, H, W, pad_;
} dc_abs_diff_map_params;
int dc_abs_diff_map(const dc_abs_diff_map_params* p, dc_stream s);

/* ---------------------------------------------------------------- Haar ----------- */
/* in [n, C, H, W] f32 -> out [n, 4C, H/2, W/2], channel 4i+{0,1,2,3} = cA,cH,cV,cD; out*=scale */
int dc_haar_dwt2(const float* in, float* out, int32_t n, int32_t C, int32_t H, int32_t W, float scale, dc_stream s);
/* in [n, 4C, h, w] -> out [n, C, 2h, 2w] */
int dc_haar_idwt2(const float* in, float* out, int32_t n, int32_t C, int32_t h, int32_t w, float scale, dc_stream s);

/* ---------------------------------------------------------------- stage end ------ */
/* errors [BS, C, T] f32 (+inf = cell not evaluated).  mean[b, c] = (sum_{j < t_end} errors[b, c, j]) / t_end, fp32, j ascending
 * (a fixed order: identical on every rank and for every world size).  keep[b, 0..k) = the k classes of smallest mean, ascending,
 * ties to the lower class id (reference: torch.topk(mean, k, largest=False), :720-721).  means [BS, C] optional (NULL). C <= 1024. */
int dc_stage_topk(const float* errors, int32_t BS, int32_t C, int32_t T, int32_t t_end, int32_t k, int32_t* keep, float* means, dc_stream s);
/* The last stage (k = 1): labels[b] = arg-min class as int64 (the LongTensor classify returns, :725). */
int dc_reduce_argmin(const float* errors, int32_t BS, int32_t C, int32_t T, int32_t t_end, int64_t* labels, float* means, dc_stream s);
/* Next stage's work-unit maps from keep[BS, k]: this rank's r-th pair is global pair g = rank + r*world of the stage, trial
 * j = t0 + g / BS, image b = g % BS; micro-batch m = pairs [m*n_bj, (m+1)*n_bj) (n_mb = ceil(n_pairs / n_bj)); slots past n_pairs
 * repeat the micro-batch's first pair and score into cell `dump`.  maps[m] = | ctx_of_unit[n_bj*k] | out_index[n_bj*k] | (int32):
 * class id of each unit and the flat index of errors[b, class, j] it writes (dc_eps_mse out_index). */
int dc_stage_maps(const int32_t* keep, int32_t BS, int32_t C, int32_t T, int32_t k, int32_t t0, int32_t n_pairs, int32_t rank,
                  int32_t world, int32_t n_bj, int32_t n_mb, int32_t dump, int32_t* maps, dc_stream s);

/* dc_stage_maps over a subset of the images: rows [n_rows] int32 on the device (ascending image ids, dc_stage_stop's active_ids).
 * Global pair g = rank + r*world has trial j = t0 + g / n_rows and image b = rows[g % n_rows]; padding, the dump cell and the clamping
 * of foreign class ids are dc_stage_maps' (an id in rows outside [0, BS) is clamped the same way).  1 <= n_rows <= BS. */
int dc_stage_maps_rows(const int32_t* keep, const int32_t* rows, int32_t n_rows, int32_t BS, int32_t C, int32_t T, int32_t k, int32_t t0,
                       int32_t n_pairs, int32_t rank, int32_t world, int32_t n_bj, int32_t n_mb, int32_t dump, int32_t* maps, dc_stream s);
/* Per-image early stopping at a stage boundary.  t_done [BS] int32 in/out: 0 = the image is still active, otherwise the number of
 * trials it was decided on (such a row is not touched: neither t_done, labels nor margin_z).  For every active image winner, runner
 * and margin_z over the cells j < t_end are dc_class_posterior's, computed by the same device code (the same bits); the image stops
 * iff margin_z >= z_stop and it has a winner whose mean is not NaN — a NaN margin_z (t_end = 1) never stops, no runner-up (margin_z =
 * +inf) does.  A stopped image gets labels[b] = winner (int64) and t_done[b] = t_end.  Then active_ids [BS] int32 = the ids of the
 * images still active, ascending (entries from n_active on: -1), and n_active [1] int32 = their count: ballots and popcount prefix
 * sums in one workgroup, no atomics — the list is the same on every rank and from launch to launch.  margin_z [BS] f32 optional
 * (NULL): the z-score of each active image (NaN where dc_class_posterior reports NaN).  z_stop > 0, +inf allowed (DC_ERR_ARG
 * otherwise); C <= 1024.  Two launches on the stream. */
int dc_stage_stop(const float* errors, int32_t BS, int32_t C, int32_t T, int32_t t_end, float z_stop, int32_t* t_done, int64_t* labels,
                  int32_t* active_ids, int32_t* n_active, float* margin_z, dc_stream s);

/* ---------------------------------------------------------------- class posterior */
/* What a finished classify call knows beyond the label, from the same errors [BS, C, T] (cells j < t_end; +inf = not evaluated, NaN
 * counts as evaluated; cells j >= t_end are never read).  Per image, every sum fp32, sequential, j ascending (dc_stage_topk's order):
 *   n[c]      evaluated cells of class c;  S[c] their sum;  mean[c] = S[c] / n[c] (+inf for n[c] = 0)
 *   winner    arg-min of mean over the finalists (n[c] = t_end) by dc_reduce_argmin's key: NaN last, ties to the lower id; -1: none
 *   delta[c]  (S[c] - Sw[c]) / n[c], Sw[c] = the winner's errors summed over the cells class c has: the paired mean difference
 *             over the trials class c was scored on (all classes of a trial share (t, eps)); delta[winner] = 0
 *   probs     softmax_c(-delta[c] / temperature) over classes with n[c] > 0 and finite delta (max subtracted); exactly 0 elsewhere
 *   entropy   -sum p ln p in nats (p = 0 adds 0)
 *   runner    arg-min of mean over the finalists without the winner, same key; -1: none
 *   margin    mean_j d_j, d_j = errors[runner, j] - errors[winner, j];  margin_z = margin / sqrt(var / t_end), var = the two-pass sample
 *             variance of d_j (t_end - 1 in the denominator), plain IEEE: t_end = 1 -> NaN, var = 0 -> +inf or NaN; no runner: both +inf
 *   invalid   NaN cells among the evaluated ones
 * winner = -1 or a NaN mean[winner]: probs, entropy, margin and margin_z of that image are NaN.
 * For errors written by the scoring loop a pruned class lost to the winner on exactly its prefix, by these sums: every delta >= 0 and
 * argmax probs = winner = the label.  One wave per image, wave reductions in a fixed order, no atomics: the same bits on every rank.
 * probs / means / delta [BS, C] f32, n_eval [BS, C] int32, the rest [BS]; means, delta and n_eval optional (NULL).  C <= 1024;
 * temperature > 0 (DC_ERR_ARG otherwise). */
typedef struct {
  const float* errors;
  float* probs;
  float* entropy; float* margin; float* margin_z;
  int32_t* winner; int32_t* runner; int32_t* invalid;
  float* means; float* delta; int32_t* n_eval;          /* optional */
  int32_t BS, C, T, t_end; float temperature; int32_t pad_;
} dc_class_posterior_params;
int dc_class_posterior(const dc_class_posterior_params* p, dc_stream s);

/* ---------------------------------------------------------------- class evidence maps */
/* Where, not only which: the per-pixel form of the eps-error and of dc_class_posterior's paired delta.
 * For unit u = (image b, class c, trial j) and pixel (y, x) of the model's [H, W] grid
 *   v[u, y, x] = sum_ch (eps_hat_u[ch, y, x] - eps_bj[ch, y, x])^2          fp32, ch ascending,
 * eps_hat formed exactly as dc_eps_mse forms it (the v-param conversion, the patch > 1 un-patchified read).  Accumulation over trials is
 * FIXED-POINT, hence associative — the same bits for every micro-batch split, launch shape, arrival order and world size:
 *   q = (int64) rint((double) v * 2^DC_EVIDENCE_FRAC_BITS)    for a finite v with 0 <= v <= DC_EVIDENCE_VMAX;
 * any other v (NaN, inf, larger) adds 0 and increments the int32 counter bad[cell].  With at most 2^18 trials (the caller's limit)
 * 2^(14 + 30 + 18) < 2^63: the int64 sum cannot overflow.
 * dc_err_map takes dc_eps_mse's inputs and adds q to acc[cell, y, x], cell = out_index[u] / T (out_index NULL: u / T); an index outside
 * [0, cells * T) — the errors dump cell of padded slots — goes to the extra plane `cells`.  acc int64 [cells + 1, H * W], bad int32
 * [cells + 1]; both are accumulated into (the caller zeroes them).  A lane owns a pixel and loops over the channels; the adds are
 * 64-bit integer global atomics, one wave adding 512 contiguous bytes.  It runs right after DC_OP_EPS_MSE, which it leaves alone.
 * loss / huber_delta: as in dc_eps_mse_params — v is the channel sum of the same per-element term (DC_LOSS_L2, zero: the square
 * above), under the same fixed-point rule; the same values are refused.
 * DC_LOSS_WEIGHTED in `loss`: dc_eps_mse's weights block behind the struct; without the bit the kernel above, untouched — v =
 * ((channel sum) * m[y, x]) * w, two fp32
 * multiplies behind the channel loop, then the same fixed-point rule: a weighted v above DC_EVIDENCE_VMAX, or a NaN one, is counted in
 * bad like any other.  The dump plane's units take w = 1. */
#define DC_EVIDENCE_FRAC_BITS 30
#define DC_EVIDENCE_VMAX 16384.0f
typedef struct {
  const float* pred; const float* eps; const float* x; const float* alpha; const float* sigma;
  const int32_t* bj_of_unit; const int32_t* img_of_bj; const int32_t* out_index;
  int64_t* acc; int32_t* bad;
  int32_t n_units, C, H, W, ld, v_param, patch;
  int32_t T, cells, pad_;
  int32_t loss; float huber_delta;
} dc_err_map_params;
int dc_err_map(const dc_err_map_params* p, dc_stream s);

/* The maps of a finished call from per-stage accumulators: acc int64 [n_stages, BS * C + 1, HW] (slab s = the trials of stage s: the
 * cells of [stage_ends[s - 1], stage_ends[s])), bad int32 [n_stages, BS * C + 1], stage_ends int32 [n_stages] ascending (on the
 * device), n_eval int32 [BS, C] and winner int32 [BS] as dc_class_posterior reports them (the caller passes -1 for an image whose
 * winner's mean is NaN).  Pruning and early stopping act at stage ends only, so n = n_eval[b, c] is 0 or a stage end; s_c = the
 * number of stages class c was scored on (stage_ends[s_c - 1] = n), w = winner[b]:
 *   mean_map[b, c]  = (sum_{s < s_c} acc[s, b, c]) * 2^-F / n
 *   delta_map[b, c] = (sum_{s < s_c} (acc[s, b, c] - acc[s, b, w])) * 2^-F / n      the int64 difference is exact; it is converted
 *                     once (to double, times 2^-F, divided by n, rounded to f32): delta_map[b, w] is exactly 0 everywhere
 *   invalid[b]      = sum of bad[s, b, c] over the scored cells (n > 0, s < s_c) of the image
 * Both maps of a cell are NaN for n = 0, for an n that is no stage end, for a cell with bad > 0 on its stages, and for an image
 * with winner outside [0, C).  mean_map / delta_map [BS, C, HW] f32, invalid [BS] int32.  One pass over acc, no atomics.
 * 1 <= n_stages <= 64. */
typedef struct {
  const int64_t* acc; const int32_t* bad; const int32_t* stage_ends; const int32_t* n_eval; const int32_t* winner;
  float* mean_map; float* delta_map; int32_t* invalid;
  int32_t n_stages, BS, C, HW;
} dc_evidence_maps_params;
int dc_evidence_maps(const dc_evidence_maps_params* p, dc_stream s);

/* ---------------------------------------------------------------- plan ----------- */
typedef enum { DC_OP_QSAMPLE = 1, DC_OP_SINUSOID = 2, DC_OP_IGEMM = 3, DC_OP_GROUPNORM = 4,
               DC_OP_LAYERNORM = 5, DC_OP_ATTENTION = 6, DC_OP_EPS_MSE = 7, DC_OP_TBLOCK_FRONT = 8,
               DC_OP_CROSS_ATTENTION = 9, DC_OP_CROSS_ATTENTION_LEN = 10, DC_OP_ATTENTION_BIAS = 11, DC_OP_RMSNORM = 12,
               DC_OP_EMBED_ROWS = 13, DC_OP_RELU = 14, DC_OP_ATTENTION_CAUSAL = 15, DC_OP_LAYERNORM_ROWS = 16, DC_OP_EMBED_ROWS_POS = 17,
               DC_OP_ACT_PASS = 18, DC_OP_ERR_MAP = 19, DC_OP_ATTENTION_WIDE = 20, DC_OP_IM2COL_S2 = 21,
               DC_OP_CONV3_PN_TAIL = 22 /* params: dc_conv3_pn_tail_op */, DC_OP_LATENT_IM2COL = 23 } dc_op_kind;
typedef struct { int32_t kind; int32_t pad_; const void* params; } dc_op;
/* Launch ops[0..n) in order on the stream; stops at the first failure and returns its
 * status (failed index via dc_last_error text). */
int dc_run_plan(const dc_op* ops, int32_t n, dc_stream s);
/* Measurement variant (bench.py only): same launches bracketed by HIP events ON THE SAME STREAM;
 * synchronises the stream at the end and writes the elapsed milliseconds of op i to ms[i]. */
int dc_run_plan_timed(const dc_op* ops, int32_t n, dc_stream s, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* DCAMD_H */
