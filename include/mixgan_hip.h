/*
 * mixgan_hip.h -- C ABI of libmixgan_hip.so: the MI355X (gfx950) implementation of the
 * MixGAN-TTS diffusion hot path.
 *
 * The reference has no FFI for this path: its boundary is the Python nn.Module surface
 * (SURVEY.md section 8b).  Each entry point below names the reference function it stands in
 * for (file:line relative to the reference tree); the host-side mirror classes under
 * mixgan-tts_amd/ keep the reference's names, signatures and state_dict keys and call these
 * through ctypes.  INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - all tensors are dense fp32 (timesteps int64), caller-owned device memory;
 *   - the library never allocates device memory, never synchronises the host and enqueues
 *     only on `stream` (a hipStream_t passed as void*), so every call is hipGraph-capturable;
 *   - return 0 on success, <0 for argument/shape errors (MG_ERR_*), >0 = hipError_t;
 *   - sequence tensors are channel-major [B, C, L] (frames contiguous) unless stated.
 */
#ifndef MIXGAN_HIP_H
#define MIXGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MG_OK 0
#define MG_ERR_ARG (-1)       /* null pointer / bad enum */
#define MG_ERR_SHAPE (-2)     /* dimension the kernels do not support */
#define MG_ERR_WORKSPACE (-3) /* workspace too small */

#define MG_VERSION 100

int mg_version(void);
/* Human-readable text for a return code (negative: ours; positive: hipGetErrorString). */
const char *mg_error_string(int code);

/* ------------------------------------------------------------------ activations */
#define MG_ACT_NONE 0
#define MG_ACT_RELU 1
#define MG_ACT_LRELU02 2 /* F.leaky_relu(x, 0.2): model/mixgantts.py:273,282,286 */
#define MG_ACT_TANH 3
#define MG_ACT_LRELU 4 /* leaky ReLU with a caller-given slope (HiFi-GAN: hifigan/models.py:7,95,150,161) */

/* ------------------------------------------------------------------ Conv1d / Linear as MFMA GEMM
 * Stands in for every nn.Conv1d / nn.Linear on the path (ConvNorm model/blocks.py:364-371,
 * LinearNorm model/blocks.py:289-291, transformer/SubLayers.py:67-80, transformer/Layers.py:67-137).
 *
 * Weights are consumed in a packed, MFMA-fragment-ordered layout that is a *derived cache* of
 * the stored [Co, Ci, K] parameter (checkpoints keep the reference layout).
 */
#define MG_PACK_PLAIN 0  /* rows in natural order */
#define MG_PACK_GATE 1   /* rows interleaved so that channel c and c+Co/2 share a lane (GLU gate) */
#define MG_PACK_DGRAD 2  /* transposed + tap-flipped: the data-gradient convolution (stride 1) */
#define MG_PACK_TPOSE 3  /* internal to mg_conv_transpose_pack (polyphase ConvTranspose1d); rejected by mg_conv_pack */
#define MG_PACK_PLAIN16 4 /* as PLAIN, fragments of v_mfma_f32_16x16x4_f32 (16-row blocks, 16-channel k-groups); K <= 3 */
#define MG_PACK_GATE16 5  /* as GATE for the 16x16x4 form: per 32 channels two gate 16-row blocks, then two filter ones */

/* Number of floats of the packed form of a [Co, Ci, K] weight. */
size_t mg_conv_packed_floats(int Co, int Ci, int K, int mode);
/* w: [Co, Ci, K] fp32 -> packed. */
int mg_conv_pack(const float *w, float *packed, int Co, int Ci, int K, int mode, void *stream);

/* out[b, co, l] = act(alpha * sum_{ci,k} w[co,ci,k] * (in[b, ci, l*stride + k - pad] + in_vec[b,ci])
 *                     + bias[co]) (+ add[b,co,l]) (+ out_old if accumulate)
 * in: [B, Ci, Lin]; out/add: [B, Co, Lout]; bias may be NULL; in_vec ([B, Ci], added to in-range
 * input positions only, i.e. before zero padding) may be NULL.  K in {1,3,5,9}, stride in {1,2}. */
int mg_conv1d_fwd(const float *in, const float *in_vec, const float *packed, const float *bias,
                  const float *add, float *out, int B, int Ci, int Lin, int Co, int Lout, int K,
                  int stride, int pad, int act, float alpha, int accumulate, void *stream);

/* As mg_conv_pack, but writes k-groups [q0, q0+Q) of a packed buffer holding Qtot k-groups per
 * 32-row block: concatenates weights that share their rows along the reduction axis. */
int mg_conv_pack_at(const float *w, float *packed, int Co, int Ci, int K, int mode, int q0, int Qtot,
                    void *stream);

/* Weight gradient of the same convolution (autograd of nn.Conv1d / nn.Linear weights):
 *   dw[co,ci,k] (+)= alpha * sum_{b,l} dy[b,co,l] * (x[b,ci,l*stride+k-pad] + x_vec[b,ci])
 * dy [B,Co,Ldy], x [B,Ci,Lx], dw [Co,Ci,K]; scratch: mg_conv1d_wgrad_scratch_floats() floats
 * (per-split partial tiles, at most 512 x 128 x 128 floats = 33.5 MB; written then summed in a fixed order, so
 * the result is reproducible run to run; needs no initialisation). */
size_t mg_conv1d_wgrad_scratch_floats(int Co, int Ci, int K);
int mg_conv1d_wgrad(const float *dy, const float *x, const float *x_vec, float *dw, float *scratch,
                    int B, int Co, int Ci, int Ldy, int Lx, int K, int stride, int pad, float alpha,
                    int accumulate, void *stream);

/* Same with explicit batch strides (floats; 0 = dense) so dy / x may be channel slices of wider tensors. */
int mg_conv1d_wgrad_strided(const float *dy, long dy_bs, const float *x, long x_bs, const float *x_vec,
                            float *dw, float *scratch, int B, int Co, int Ci, int Ldy, int Lx, int K,
                            int stride, int pad, float alpha, int accumulate, void *stream);

/* G weight gradients of one shape in a single launch: group g uses dy + g*dy_gs, x + g*x_gs (a group stride of 0
 * shares that operand) and writes dw + g*dw_gs (0 = Co*Ci*K).  mg_denoiser_bwd computes the gradients of all
 * 20 residual layers' k=3 and output convolutions this way once their inputs are complete: with G*tiles >= 512
 * workgroups no frame split is needed and the combine pass degenerates to the layout transpose. */
size_t mg_conv1d_wgrad_grouped_scratch_floats(int Co, int Ci, int K, int G);
int mg_conv1d_wgrad_grouped(const float *dy, long dy_bs, long dy_gs, const float *x, long x_bs, long x_gs, float *dw,
                            long dw_gs, float *scratch, int G, int B, int Co, int Ci, int Ldy, int Lx, int K, int stride,
                            int pad, float alpha, int accumulate, void *stream);
/* ... and the bias gradients with it: db[g][co] (+)= alpha * sum_{b,l} dy_g[b,co,l] (group stride db_gs, 0 -> Co).
 * The streaming kernel (large stride-1 "same" shapes) sums the dY rows while it stages them; other shapes fall back
 * to one mg_rowsum launch per group.  Same scratch as mg_conv1d_wgrad_grouped. */
int mg_conv1d_wgrad_grouped_bias(const float *dy, long dy_bs, long dy_gs, const float *x, long x_bs, long x_gs, float *dw,
                                 long dw_gs, float *db, long db_gs, float *scratch, int G, int B, int Co, int Ci, int Ldy,
                                 int Lx, int K, int stride, int pad, float alpha, int accumulate, void *stream);

/* Row sums of in [B,R,L] (batch stride in_bs floats, 0 = dense): bias gradients and per-sample
 * channel sums.  out_r[r] (+)= alpha*sum_{b,l} (may be NULL); out_br[b,r] = alpha*sum_l (may be NULL). */
int mg_rowsum(const float *in, long in_bs, int B, int R, int L, float *out_r, float *out_br,
              float alpha, int accumulate, void *stream);

/* Extended form for the vocoder (hifigan/models.py): K additionally in {4,7,11,16},
 * dilation dil <= 5 (input sample l*stride + k*dil - pad), a leaky ReLU of slope in_slope applied to the
 * input samples while they are staged (1 = identity; pre-activation of ResBlock convs), and
 * act = MG_ACT_LRELU with slope act_slope. */
int mg_conv1d_fwd_ex(const float *in, const float *in_vec, const float *packed, const float *bias,
                     const float *add, float *out, int B, int Ci, int Lin, int Co, int Lout, int K,
                     int stride, int pad, int dil, float in_slope, int act, float act_slope, float alpha,
                     int accumulate, void *stream);
/* Same, with a split reduction for outputs of few tiles and deep reductions (the JCU discriminator's tail and its data
 * gradients, model/mixgantts.py:219-248: 512 channels x 5 taps into 128 channels at L/4 frames is 32 output tiles on 256
 * CUs): when `scratch` is given and the 128 x 128-tile grid would leave most CUs idle, the input-channel chunks of a tile
 * are dealt to up to 8 workgroups, which leave partial tiles in the scratch; a second, small launch adds them in split
 * order and applies bias / activation / add.  scratch: fp32, one per stream in flight; 12 Mi floats cover every shape of
 * the path.  Without scratch, or when a split does not pay, identical to mg_conv1d_fwd_ex. */
int mg_conv1d_fwd_split(const float *in, const float *in_vec, const float *packed, const float *bias,
                        const float *add, float *out, int B, int Ci, int Lin, int Co, int Lout, int K, int stride,
                        int pad, int dil, float in_slope, int act, float act_slope, float alpha, int accumulate,
                        float *scratch, size_t scratch_floats, void *stream);

/* Which instantiation of the convolution kernel a launch runs, and on what grid: the decision the launcher itself
 * switches on (conv_plan, csrc/conv_mfma.h).  rows: GEMM rows of the packed weight (Co; Co * u for the polyphase
 * transposed convolution, where Lout is the input length).  scratch_floats: the split-reduction scratch of
 * mg_conv1d_fwd_split, 0 = none.  epi: which set of instantiations the entry point has --
 * mg_conv1d_fwd / _ex / _split, mg_conv_transpose1d_fwd and mg_conv1x1_fwd_strided are MG_CONV_EPI_PLAIN.
 * MG_ERR_SHAPE where the launch would return it (no instantiation).  No GPU work. */
#define MG_CONV_EPI_PLAIN 0        /* K in {1,3,5,9} (K = 5 also at stride 2); K in {3,7,11} at dil <= 5, K in {4,16} */
#define MG_CONV_EPI_REFLECT 1      /* mg_conv1d_reflect_fwd: K = 3 at dil <= 9, K = 7 */
#define MG_CONV_EPI_PHASES_SLICE 2 /* mg_conv_transpose1d_fwd_slice: K = 3 */
#define MG_CONV_EPI_NEEDS_WM2 3    /* an epilogue that pairs 32-row blocks (the denoiser's gate): K in {1,3,5,9}, never
                                    * the one-block-per-wave forms */
#define MG_CONV_EPI_PERIOD 5       /* mg_period_conv_fwd / _dgrad: K = 5 at stride 3 and 1, K = 3, K = 2 (the two-tap
                                    * polyphase GEMM of the stride-3 data gradient).  (4 names nothing: MG_ERR_ARG.) */
typedef struct mg_conv_plan {
    int32_t kw, stride, ck, dilmax; /* the (K, stride, chunk channels, largest dilation) case */
    int32_t mw, wm, nnb;            /* waves along the rows, 32-row blocks and 32-frame blocks per wave:
                                     * a workgroup tile of 32 mw wm rows x 32 (4 / mw) nnb frames */
    int32_t ksplit;                 /* workgroups sharing a tile's reduction (1: unsplit) */
    int32_t grid;                   /* workgroups of the convolution launch: tiles x ksplit */
} mg_conv_plan;
int mg_conv1d_fwd_plan(int B, int Ci, int Lout, int rows, int K, int stride, int dil, size_t scratch_floats, int epi,
                       mg_conv_plan *out);

/* ------------------------------------------------------------------ diffusion algebra (HBM-bound)
 * Schedule tables are the fp32 buffers of GaussianDiffusion (model/diffusion.py:60-83). */

/* diffuse_fn + q_sample (model/diffusion.py:177-185, 147-153), fused with norm_spec (:228),
 * the [B,L,M] -> [B,1,M,L] transpose and the mask multiply of :206-207.
 *   mel [B, L, M]; t int64 [B] (t<0 rows return the clean normalised mel); noise [B, M, L];
 *   keep uint8 [B, L] (1 = valid frame) or NULL; out [B, M, L].
 * M <= mg_transpose_max_m() (below), MG_ERR_SHAPE beyond it.                                      */
int mg_diffuse_fwd(const float *mel, const int64_t *t, const float *noise, const uint8_t *keep,
                   const float *spec_min, const float *spec_max, const float *sqrt_ac,
                   const float *sqrt_1mac, float *out, int B, int L, int M, int T, void *stream);

/* q_posterior_sample (model/diffusion.py:104-119) with the clamp_ of :126-127 / :211-212 and the
 * mask multiply of :220 fused:  x0c = clamp(x0 (* keep), -1, 1) if clip;
 *   out = (coef1[t] x0c + coef2[t] x_t + [t != 0] exp(0.5 logvar[t]) noise) (* keep).
 * If x0_clamped_out != NULL the masked+clamped x0 is written there (training returns it).
 * Tensors [B, M, L]; keep uint8 [B, L] or NULL (p_sample applies no mask). */
int mg_posterior_sample_fwd(const float *x0, const float *x_t, const int64_t *t, const float *noise,
                            const uint8_t *keep, const float *coef1, const float *coef2,
                            const float *logvar, float *out, float *x0_clamped_out, int clip, int B,
                            int L, int M, int T, void *stream);

/* Gradient of mg_posterior_sample_fwd w.r.t. x0 (everything else on the path is data):
 *   g_x0 = keep * 1[-1 <= x0*keep <= 1 or !clip] * (g_x0c + coef1[t] * keep * g_xpp).
 * g_x0c or g_xpp may be NULL (not both). */
int mg_posterior_sample_bwd(const float *x0, const int64_t *t, const uint8_t *keep,
                            const float *coef1, const float *g_x0c, const float *g_xpp, float *g_x0,
                            int clip, int B, int L, int M, int T, void *stream);

/* norm_spec / denorm_spec (model/diffusion.py:228-232) on a flat [n/M, M] tensor:
 * mode 1 norm, 2 denorm, 3 gradient of norm (g * 2/(max-min)), 4 gradient of denorm. */
int mg_spec_affine(const float *in, float *out, const float *spec_min, const float *spec_max,
                   int mode, size_t n, int M, void *stream);

/* [B, M, L] <-> [B, L, M] transposes with optional norm/denorm_spec (model/diffusion.py:228-232):
 * mode 0 plain, 1 norm_spec on the way in (BLM->BML), 2 denorm_spec on the way out (BML->BLM). */
int mg_transpose_bml(const float *in, float *out, const float *spec_min, const float *spec_max,
                     const uint8_t *keep, int to_blm, int mode, int B, int L, int M, void *stream);
/* Same, with the [B,M,L] side being an M-channel slice of a wider tensor (batch stride bml_bs floats):
 * builds torch.cat([x_t_prevs, x_ts], -1).transpose(1,2) (model/mixgantts.py:262-264) without a copy. */
int mg_transpose_bml_strided(const float *in, float *out, const float *spec_min, const float *spec_max,
                             const uint8_t *keep, int to_blm, int mode, int B, int L, int M, long bml_bs,
                             void *stream);
/* Largest M of the two transposes and of mg_diffuse_fwd on the current device: they stage a [64][M + 1] float tile
 * in dynamic LDS, so M <= (dynamic LDS a workgroup of these kernels can get) / 256 - 1, and never above 1024.  639 on
 * an MI355X (163,840 bytes).  A wider M is refused with MG_ERR_SHAPE before anything is launched.  0 without a device. */
int mg_transpose_max_m(void);

/* ------------------------------------------------------------------ Denoiser (model/modules.py:382-446)
 * The pointer table of mg_denoiser_pack (weights) and mg_denoiser_bwd (gradients): MG_DEN_HEAD_PTRS head slots, then
 * MG_DEN_LAYER_PTRS slots per residual layer -- slot j of layer l is entry MG_DEN_HEAD_PTRS + MG_DEN_LAYER_PTRS * l + j.
 * Each slot is listed with the reference state_dict key it holds (under `diffusion.denoise_fn.`) and its shape. */
#define MG_DEN_HEAD_PTRS 8
#define MG_DEN_LAYER_PTRS 9
enum mg_den_head_slot {
    MG_DEN_IN_W = 0,   /* input_projection.0.conv.weight [C,M,1] */
    MG_DEN_IN_B = 1,   /* input_projection.0.conv.bias [C]       */
    MG_DEN_MLP0_W = 2, /* mlp.0.linear.weight [4C,C]             */
    MG_DEN_MLP2_W = 3, /* mlp.2.linear.weight [C,4C]             */
    MG_DEN_SKIP_W = 4, /* skip_projection.conv.weight [C,C,1]    */
    MG_DEN_SKIP_B = 5, /* skip_projection.conv.bias [C]          */
    MG_DEN_OUT_W = 6,  /* output_projection.conv.weight [M,C,1]  */
    MG_DEN_OUT_B = 7   /* output_projection.conv.bias [M]        */
};
enum mg_den_layer_slot { /* keys under residual_layers.<l>. */
    MG_DEN_L_CONV_W = 0,  /* conv_layer.conv.weight [2C,C,3]             */
    MG_DEN_L_CONV_B = 1,  /* conv_layer.conv.bias [2C]                   */
    MG_DEN_L_DIFF_W = 2,  /* diffusion_projection.linear.weight [C,C]    */
    MG_DEN_L_COND_W = 3,  /* conditioner_projection.conv.weight [C,H,1]  */
    MG_DEN_L_COND_B = 4,  /* conditioner_projection.conv.bias [C]        */
    MG_DEN_L_OUT_W = 5,   /* output_projection.conv.weight [2C,C,1]      */
    MG_DEN_L_OUT_B = 6,   /* output_projection.conv.bias [2C]            */
    MG_DEN_L_SPK_W = 7,   /* speaker_projection.linear.weight [C,H]; NULL unless multi_speaker */
    MG_DEN_L_RESERVED = 8 /* NULL */
};
typedef struct {
    int32_t n_layers;      /* model.denoiser.residual_layers (20) */
    int32_t channels;      /* C: residual_channels (256)          */
    int32_t cond_channels; /* H: transformer.encoder_hidden (256) */
    int32_t mel_bins;      /* M: n_mel_channels (80)              */
    int32_t multi_speaker; /* 0/1                                 */
} mg_denoiser_dims;

/* flags for mg_denoiser_packed_floats / mg_denoiser_pack */
#define MG_DEN_BACKWARD 1 /* also pack the transposed (data-gradient) forms mg_denoiser_bwd consumes */
#define MG_DEN_SPLIT 2    /* also pack hi/lo bf16 pairs for the split-precision forward */
#define MG_DEN_P16 4      /* also pack the 16x16x4-MFMA forms: the 16-frame tile width of the single-launch forward */
#define MG_DEN_JOBS_RESIDENT 8 /* mg_denoiser_pack only: the previous call had the same weight pointers, flags and `packed`
                                * buffer -- its job table is still in the buffer's tail, skip the host-to-device copy
                                * (the one host transfer of a training step: without it the step is hipGraph-capturable) */
/* flags for mg_denoiser_fwd's `mode` */
#define MG_FWD_SAVE 1     /* keep per-layer activations for mg_denoiser_bwd (fp32 path only) */
#define MG_FWD_SPLIT 2    /* residual-layer GEMMs as 3-term bf16-split MFMA products (fp32-grade, ~1e-5) */
#define MG_FWD_P16 4      /* `packed` was built with MG_DEN_P16: small launches may use the 16-frame tile width */
/* Accepted models: 1 <= n_layers <= 256, channels a multiple of 64, cond_channels a multiple of 32, mel_bins >= 1
 * (MG_ERR_SHAPE otherwise).  MG_DEN_SPLIT and MG_DEN_P16 exist for channels == cond_channels == 256 only: for any other
 * model mg_denoiser_packed_floats answers 0 and mg_denoiser_pack MG_ERR_SHAPE, before it queues or launches anything. */
size_t mg_denoiser_packed_floats(const mg_denoiser_dims *d, int flags);
/* freq: the C/2 step-embedding frequencies exp(-i ln(1e4)/(C/2-1)) (model/blocks.py:909-910),
 * computed by the host exactly as the reference does and cached in the packed blob.
 * The pack is a list of jobs (9 + 7 or 8 per layer, 3 + 3 per layer more with MG_DEN_BACKWARD, 3 + 5 per layer more with
 * MG_DEN_P16) executed from a 768-entry table in the blob's tail: one upload and one launch per 768 jobs, so every
 * accepted n_layers packs.  MG_DEN_JOBS_RESIDENT is honoured for a list of at most 768 jobs and ignored for a longer one. */
int mg_denoiser_pack(const mg_denoiser_dims *d, const float *const *weights, const float *freq,
                     float *packed, int flags, void *stream);
/* The host half of mg_denoiser_pack alone -- the same checks over the same arguments and the same job list, no device
 * call, no pointer dereferenced but the table itself: the code mg_denoiser_pack would return before its first upload,
 * and, when MG_OK, how many jobs it queues and in how many launches it runs them (either may be NULL). */
int mg_denoiser_pack_plan(const mg_denoiser_dims *d, const float *const *weights, const float *freq,
                          const float *packed, int flags, int *jobs, int *launches);
/* Workspace (floats) for a forward of batch B, L frames.  save_for_backward additionally keeps the
 * per-layer activations that mg_denoiser_bwd consumes. */
size_t mg_denoiser_workspace_floats(const mg_denoiser_dims *d, int B, int L, int save_for_backward);

/* Denoiser.forward: x_t [B, M, L] (the reference's [B,1,M,L]), t int64 [B], cond [B, H, L],
 * spk [B, H] or NULL -> out [B, M, L].  */
int mg_denoiser_fwd(const mg_denoiser_dims *d, const float *packed, const float *x_t,
                    const int64_t *t, const float *cond, const float *spk, float *out,
                    float *workspace, size_t workspace_floats, int B, int L, int mode, void *stream);

/* Which kernel mg_denoiser_fwd / mg_denoiser_psample run for (B, L, mode): the same decision they make, environment
 * pins (MG_DENOISER_PERSIST, MG_DENOISER_GENERIC, MG_PERSIST_NT / _SOLO / _TEAM) included.  cproj_mode: 0 none, 1 the
 * launch stores its conditioner projections (mg_sampling_loop.cproj_out), 2 it reads them (.cproj).  cus: compute
 * units to plan for, <= 0: the current device's.  No GPU work; the plan depends on no pointer. */
#define MG_PLAN_PER_LAYER 0 /* path: one launch per residual layer */
#define MG_PLAN_SINGLE 1    /* path: the whole forward as one launch */
#define MG_PLAN_PERSIST 0   /* family: denoiser_persist_kernel (32- or 64-frame tiles) */
#define MG_PLAN_PERSIST16 1 /* family: denoiser_persist16_kernel (16-frame tiles, one workgroup per tile) */
#define MG_PLAN_TEAM16 2    /* family: denoiser_team16_kernel (16-frame tiles, `team` workgroups per tile) */
typedef struct mg_fwd_plan {
    int32_t path;       /* MG_PLAN_PER_LAYER / MG_PLAN_SINGLE; the fields below describe the single launch (else 0) */
    int32_t family;     /* MG_PLAN_PERSIST / _PERSIST16 / _TEAM16 */
    int32_t nt;         /* tile width in frames */
    int32_t waves;      /* waves per workgroup */
    int32_t solo;       /* 1: the build for one workgroup per CU, 0: two per CU */
    int32_t team;       /* workgroups per tile (team16), else 0 */
    int32_t cproj_mode; /* conditioner-projection mode of the launch (0 when saving) */
    int32_t grid, block;
} mg_fwd_plan;
int mg_denoiser_fwd_plan(const mg_denoiser_dims *d, int B, int L, int mode, int cproj_mode, int cus, mg_fwd_plan *out);

/* The workspace's first use must find its 64-float counter block zeroed (allocate it zero-filled once; the kernels
 * re-arm the counters themselves, also under hipGraph replay).
 *
 * p_sample (model/diffusion.py:121-129) as one call: x_0 = Denoiser.forward(x_t, t, cond, spk); clamp to [-1, 1] when
 * clip; x_prev = coef1[t] x_0 + coef2[t] x_t + (t > 0) exp(0.5 logvar[t]) * noise  (q_posterior + q_posterior_sample,
 * :104-119).  coef1 / coef2 / logvar: the posterior_mean_coef1 / posterior_mean_coef2 / posterior_log_variance_clipped
 * buffers [n_steps].  noise [B, M, L], or NULL: N(0,1) from Philox4x32-10 (the reference draws torch.randn_like per
 * step, model/diffusion.py:32-35,118): key = `seed`, counter = (element index, noise_stream << 32 | launches completed
 * on this workspace).  The launch count lives in the workspace, so every call and every replay of a captured graph
 * draws fresh noise; `noise_stream` (its low 32 bits) must be unique per workspace instance within a process -- the
 * caller numbers its workspaces -- so that two workspaces (another shape, a re-allocated one, another captured graph)
 * never walk the same stream; ranks use different seeds.  x_prev [B, M, L] must not alias x_t; x0_out (optional)
 * receives the pre-clamp x_0.  On the fp32 inference path this is ONE kernel launch.
 *
 *
 * loop (optional): what the T steps of one sampling loop (model/diffusion.py:133-147) share -- see mg_sampling_loop.
 * Results are bit-identical to loop == NULL. */
typedef struct mg_sampling_loop {
    /* cproj / cproj_out (fp32 MG_FWD_P16 packs only, at most one of them): the conditioner projections of all layers,
     * [B, n_layers * channels, L].  The steps of a loop call the denoiser with the SAME cond, and
     * conditioner_projection(cond) (model/blocks.py:1160) depends on neither x_t nor t: the first step passes cproj_out
     * and leaves what it computed there, the steps behind it pass that buffer as cproj and skip the projections -- 11 %
     * of a step's multiply-adds.  The kernels form fl(P + fl(x + step)) either way, P = b_c with the products W_c cond
     * added onto it in channel order -- a function of cond alone.  (mg_denoiser_cond_project fills the same buffer without
     * a step; it adds b_c behind the sum, so its P may differ from a kernel's in the last bit.) */
    const float *cproj;
    float *cproj_out;
    /* step_vectors: mg_denoiser_step_vectors' output for all step_count steps of the loop (a loop knows its t values
     * in advance); this call is step step_index of them and reads its slice in place instead of launching the step
     * embedding, its MLP and the per-layer diffusion / speaker projections (model/modules.py:433-435,
     * model/blocks.py:1159-1163) itself.  `t` must still be this step's t (the posterior reads it). */
    const float *step_vectors;
    int step_index, step_count;
} mg_sampling_loop;
int mg_denoiser_psample(const mg_denoiser_dims *d, const float *packed, const float *x_t, const int64_t *t,
                        const float *cond, const float *spk, const float *coef1, const float *coef2,
                        const float *logvar, int n_steps, const float *noise, unsigned long long seed,
                        unsigned long long noise_stream, int clip, float *x_prev, float *x0_out,
                        const mg_sampling_loop *loop, float *workspace, size_t workspace_floats, int B, int L, int mode,
                        void *stream);
/* The step-dependent vectors of Denoiser.forward for n steps at once: t [n, B] (step-major), spk [B, H] (the same
 * utterances in every step; NULL unless multi_speaker).  For each step: diffusion_embedding(t) -> mlp
 * (model/modules.py:433-434), then per residual layer diffusion_projection(.) and, multi-speaker,
 * + speaker_projection(spk) (model/blocks.py:1159-1163).  `vectors`: mg_denoiser_step_vectors_floats(d, n, B) floats,
 * opaque; pass it to each step's mg_denoiser_psample through mg_sampling_loop.  Same values bit for bit as the vectors
 * a step computes for itself. */
size_t mg_denoiser_step_vectors_floats(const mg_denoiser_dims *d, int n, int B);
int mg_denoiser_step_vectors(const mg_denoiser_dims *d, const float *packed, const int64_t *t, const float *spk,
                             float *vectors, size_t vectors_floats, int n, int B, void *stream);
/* cproj[b, l * channels + c, :] = conditioner_projection_l(cond[b])[c, :] (model/blocks.py:1150,1160: Conv1d(H, C, 1) with
 * bias) for every residual layer l, as one [n_layers * channels, H] x [H, B * L] product.  `packed` must have been built
 * with MG_DEN_P16 (channels == cond_channels == 256). */
int mg_denoiser_cond_project(const mg_denoiser_dims *d, const float *packed, const float *cond, float *cproj, int B,
                             int L, void *stream);
/* Both generator forwards of a GAN training step (train.py:133 and :153 -- same weights, different t / noise) as ONE
 * launch of 64-frame tiles: problem A (x_tA, tA -> outA; nothing kept) is the D phase's no-grad forward, problem B
 * (x_tB, tB -> outB) the G phase's: its layer activations land in wsB exactly as mg_denoiser_fwd(MG_FWD_SAVE) leaves
 * them, so mg_denoiser_bwd runs on (x_tB, tB, wsB) unchanged.  Bh utterances per problem; problem A reads cond [Bh, H, L]
 * and spk, problem B condB / spkB (NULL = the same as A's: the reference runs its train-mode linguistic encoder once per
 * model call, so the two phases see different conditioners unless the encoder is deterministic).  wsA: mg_denoiser_workspace_floats(dims, 2 * Bh, L, 0) floats (zero before its first use, like every
 * forward workspace); wsB: mg_denoiser_workspace_floats(dims, Bh, L, 1).  packed: with the backward packs or without.
 * MG_ERR_SHAPE when the single-launch kernel does not take the shape -- run the two forwards separately then. */
int mg_denoiser_fwd_pair(const mg_denoiser_dims *dims, const float *packed, const float *x_tA, const int64_t *tA,
                         const float *x_tB, const int64_t *tB, const float *cond, const float *spk, const float *condB,
                         const float *spkB, float *outA, float *outB, float *wsA, size_t wsA_floats, float *wsB,
                         size_t wsB_floats, int Bh, int L, void *stream);
/* Failure reporting of the single-launch kernels (mg_denoiser_fwd / _psample / _fwd_pair / _bwd).  Their workgroups
 * hand halo columns to each other; every wait is bounded, and when one gives up (another tenant holding the GPU's
 * workgroup slots for seconds) the launch drains instead of hanging, and
 *   - the workspace's sticky error word is set: that launch, and every later one on the same workspace, writes NaN
 *     instead of its output (forward: out / x_prev; backward: d x_t and the input-projection gradients);
 *   - a process-wide word in pinned host memory receives the code (forward: 1 + layer, backward: 0x100 + layer).
 * mg_persist_error(clear) returns that word without synchronising anything (0 = no failure so far; after a stream
 * synchronisation it is exact for all work before it) and resets it when `clear`.  A caller that sees it non-zero must
 * discard the workspaces in use (their sticky words stay set).  Test hooks, read per call: MG_PERSIST_SPIN_LIMIT (polls
 * before giving up), MG_PERSIST_FLAGS bit 1 (a tile withholds one hand-off). */
unsigned mg_persist_error(int clear);
/* Order of the counter words that mg_denoiser_persist_status and mg_denoiser_bwd_status write to host_out4. */
enum mg_status_word {
    MG_STATUS_TICKET = 0,   /* tickets handed out by the running launch (0 between launches) */
    MG_STATUS_ERROR = 1,    /* sticky: code of a hand-off that timed out, or 0                */
    MG_STATUS_LAUNCHES = 2, /* single launches completed on the workspace                    */
    MG_STATUS_DONE = 3,     /* workgroups of the running launch that have exited             */
    MG_STATUS_WORDS = 4
};
/* Copies the single-launch forward's counter words (MG_STATUS_*: ticket, error, launches, workgroups done) of a (B, L, no-save)
 * workspace to host_out4 and synchronises the stream: error != 0 means a neighbour hand-off timed out (the launch
 * drained instead of hanging; its output is NaN). */
int mg_denoiser_persist_status(const mg_denoiser_dims *d, const float *workspace, int B, int L, unsigned *host_out4,
                               void *stream);

/* Backward of Denoiser.forward (what torch.autograd does for the reference).  `workspace` is the
 * forward's workspace of a save_for_backward call on the same inputs; `bwd_workspace` has
 * mg_denoiser_bwd_workspace_floats() floats.  g_out [B, M, L] is dL/d(out).
 * grads: pointer table in the order of mg_denoiser_pack's weight table; every non-NULL entry
 * receives dL/dW (overwritten, not accumulated).  Every per-layer entry (MG_DEN_L_CONV_W .. MG_DEN_L_SPK_W)
 * must be the layer's slice of one contiguous [n_layers, ...] buffer: the layer loop only
 * runs the two data-gradient GEMMs per layer and keeps their results (0.5 GB of the workspace at B=8, L=1000);
 * all weight and bias gradients are then produced by a few launches grouped over the layer axis.
 * d_x_t [B,M,L], d_cond [B,H,L], d_spk [B,H] may be NULL when not needed. */
size_t mg_denoiser_bwd_workspace_floats(const mg_denoiser_dims *d, int B, int L);
int mg_denoiser_bwd(const mg_denoiser_dims *d, const float *packed, const float *g_out,
                    const float *x_t, const float *cond, const float *spk, float *workspace,
                    float *bwd_workspace, size_t bwd_workspace_floats, float *const *grads,
                    float *d_x_t, float *d_cond, float *d_spk, int B, int L, void *stream);
/* Copies the single-launch data-gradient kernel's counter words (MG_STATUS_*: ticket, error, launches, workgroups done) of a (B, L)
 * backward workspace to host_out4 and synchronises the stream.  launches counts the single launches completed on this
 * workspace (the launch-per-layer path leaves it alone); error != 0: a hand-off timed out (sticky). */
int mg_denoiser_bwd_status(const mg_denoiser_dims *d, const float *bwd_workspace, int B, int L, unsigned *host_out4,
                           void *stream);
/* Same; conv3_grads_done (a hipEvent_t, or NULL) is recorded on `stream` right behind the launches that produce the
 * conv_layer weight and bias gradients of all layers (MG_DEN_L_CONV_W / _CONV_B: a third of the generator's gradient bytes), 0.6 ms
 * of GPU work before the last launch of the backward at B=8, L=1000 -- a data-parallel caller starts the all-reduce of
 * that slice behind the event while the remaining gradients are still being computed (train.py has no such exchange:
 * the reference is single-device). */
int mg_denoiser_bwd_staged(const mg_denoiser_dims *d, const float *packed, const float *g_out,
                           const float *x_t, const float *cond, const float *spk, float *workspace,
                           float *bwd_workspace, size_t bwd_workspace_floats, float *const *grads,
                           float *d_x_t, float *d_cond, float *d_spk, int B, int L, void *conv3_grads_done,
                           void *stream);

/* ------------------------------------------------------------------ pieces of autograd around the GEMMs
 * dpre = dy * act'(.) written through the saved OUTPUT y = act(pre) (ReLU / LeakyReLU(0.2) / tanh). */
int mg_act_bwd(const float *dy, const float *y, float *out, int act, size_t n, void *stream);
/* Zero insertion out[r, j] = in[r, j/stride] if stride | j else 0 (j < Lup): turns the data gradient
 * of a strided Conv1d (model/mixgantts.py:219-228, strides [1,2,2]) into a stride-1 convolution. */
int mg_upsample_zero(const float *in, float *out, int rows, int Lin, int stride, int Lup, void *stream);
/* Same with a leaky ReLU (slope) on the kept samples: lrelu + ConvTranspose1d of hifigan/models.py:150-151 as
 * zero insertion followed by a stride-1 convolution on the MG_PACK_DGRAD pack of the [Cin, Cout, K] weight. */
int mg_upsample_zero_act(const float *in, float *out, int rows, int Lin, int stride, int Lup, float slope,
                         void *stream);
/* ConvTranspose1d(Ci, Co, kernel 2u, stride u, padding u/2) of hifigan/models.py:121-127,151 without the zeros:
 * output phase r = n mod u is a 2-tap convolution of the input, so all u phases together are one 3-tap
 * implicit GEMM with Co*u rows (3/2 of the useful MACs instead of u times them with zero insertion) whose
 * epilogue interleaves the phases back into out [B, Co, u*Lin] with 16-byte stores.  u in {2,4,8}.
 * w is the PyTorch ConvTranspose1d weight [Ci, Co, 2u]; out = alpha * convT(lrelu(in, in_slope)) + bias. */
size_t mg_conv_transpose_packed_floats(int Ci, int Co, int u);
int mg_conv_transpose_pack(const float *w, float *packed, int Ci, int Co, int u, void *stream);
int mg_conv_transpose1d_fwd(const float *in, const float *packed, const float *bias, float *out, int B, int Ci,
                            int Lin, int Co, int u, float in_slope, float alpha, void *stream);

/* ------------------------------------------------------------------ MelGAN vocoder (melgan.py)
 * Generator(80, ngf=32, n_residual_layers=3) of descriptinc/melgan-neurips mel2wav/modules.py.  in_bs / out_bs are
 * batch strides in floats (0 = dense): they let x and t of a ResnetBlock share one [B, 2C, L] buffer. */
/* Same as mg_conv_transpose1d_fwd, writing channels [0, Co) of a buffer with batch stride out_bs (0 -> Co*u*Lin). */
int mg_conv_transpose1d_fwd_slice(const float *in, const float *packed, const float *bias, float *out, long out_bs,
                                  int B, int Ci, int Lin, int Co, int u, float in_slope, float alpha, void *stream);
/* ReflectionPad1d(pad) + Conv1d on the MG_PACK_PLAIN pack, pad = dil*(K-1)/2, Lout = L: out = act(alpha *
 * conv(reflect(lrelu(in, in_slope))) + bias).  Out-of-range input positions read in[-l] / in[2(L-1)-l].  K = 7 with
 * dil = 1 (first and last conv) or K = 3 with dil <= 9 (ResnetBlock); MG_ERR_SHAPE for L <= pad, as ReflectionPad1d. */
int mg_conv1d_reflect_fwd(const float *in, long in_bs, const float *packed, const float *bias, float *out, long out_bs,
                          int B, int Ci, int L, int Co, int K, int dil, float in_slope, int act, float act_slope,
                          float alpha, void *stream);
/* out = W in + bias, a K = 1 conv with batch strides.  A ResnetBlock's shortcut(x) + W2 t is this with Ci = 2C over
 * [x ; t] and the packs of Ws and W2 concatenated along the reduction (mg_conv_pack_at), bias = bs + b2. */
int mg_conv1x1_fwd_strided(const float *in, long in_bs, const float *packed, const float *bias, float *out, long out_bs,
                           int B, int Ci, int L, int Co, void *stream);
/* The three ResnetBlocks (dilations 1, 3, 9) of one stage in one launch, C in {32, 64}: out = block3(block2(block1(in))),
 * in != out, both [B, C, L] dense, L > 9.  Per block k: w1[k] = mg_conv_pack of W1 [C, C, 3]; b1[k] [C];
 * wmix[k] = [Ws | W2'] packed as K = 1 k-groups [0, C/8) and [C/8, C/4) of a C/4-group stream (mg_conv_pack_at), where
 * W2' = W2[:, perm], perm[8g + 2e + h] = 8g + 4h + e (the accumulator row order, melgan.hip); bmix[k] = bs + b2. */
int mg_melgan_stack_fwd(const float *in, float *out, const float *const *w1, const float *const *b1,
                        const float *const *wmix, const float *const *bmix, int B, int C, int L, void *stream);
/* Output samples per workgroup tile of mg_melgan_stack_fwd for C (0 if C is not taken). */
int mg_melgan_stack_tile(int C);

/* Audio front end (audio/stft.py, audio/audio_processing.py; csrc/audio.hip).  n_fft = MG_STFT_N, hop a power of two
 * <= MG_STFT_N; window [MG_STFT_N] fp32 (centre-padded), twiddle [MG_STFT_N] complex fp32 interleaved,
 * twiddle[k] = exp(-2 pi i k / MG_STFT_N).  x [B, L] with batch stride x_bs, L > MG_STFT_N / 2; lengths [B] int32
 * (null: all L) gives each item its own reflect end and frame count 1 + lengths[b] / hop; frames past it are 0.
 * T (<= 1 + L / hop) is the frame dimension of the outputs. */
#define MG_STFT_N 1024
#define MG_STFT_MAX_MELS 128
/* STFT.transform (stft.py:55-82): magnitude and phase [B, N/2+1, T] at element (b, k, t) = b s_bs + k s_ks + t s_ts.
 * mag null: phase only (the Griffin-Lim update). */
int mg_stft_fwd(const float *x, long x_bs, const int *lengths, int B, int L, int hop, const float *window,
                const float *twiddle, float *mag, float *phase, long s_bs, long s_ks, long s_ts, int T, void *stream);
/* TacotronSTFT.mel_spectrogram (stft.py:160-178): mel [B, n_mels, T] = log(max(mel_basis |STFT|, 1e-5)), energy [B, T]
 * = ||STFT||_2 over bins.  The basis is passed as per-row nonzero bands: band[m], band[n_mels + m],
 * band[2 n_mels + m] = first bin, bin count, offset into band_w. */
int mg_stft_mel(const float *x, long x_bs, const int *lengths, int B, int L, int hop, const float *window,
                const float *twiddle, const int *band, const float *band_w, int n_mels, float *mel, float *energy,
                int T, void *stream);
/* STFT.inverse (stft.py:84-121): out [B, (T-1) hop] from magnitude / phase (strides as mg_stft_fwd), T >= 2.
 * wsq [MG_STFT_N] float64 = the squared centre-padded window (window_sumsquare is evaluated in-kernel from it).
 * tile: output samples per workgroup, a multiple of 64 up to 1024 (a launch-shape choice; the result does not
 * depend on it). */
int mg_istft(const float *mag, const float *phase, long s_bs, long s_ks, long s_ts, int B, int T, int hop,
             const float *window, const double *wsq, const float *twiddle, float *out, int tile, void *stream);

/* ------------------------------------------------------------------ vocoder training (vocoder.py forward_train,
 * audio.py mel_spectrogram_diff; csrc/vocoder_train.hip).  Every result is reproducible run to run. */
/* dw[co,ci,k] (+)= alpha * sum_{b,l} dy[b,co,l] * lrelu(x[b,ci, l + k*dil - pad], in_slope), x out of range = 0:
 * the weight gradient of mg_conv1d_fwd_ex through the saved PRE-activation x (in_slope = 1: identity).
 * K in {3,7,11}, 1 <= dil <= 5, Ldy = Lx + 2 pad - dil (K-1); batch strides in floats (0 = dense); scratch of
 * mg_conv1d_wgrad_scratch_floats(Co, Ci, K) floats.  The bias gradient is mg_rowsum of dy. */
int mg_conv1d_wgrad_ex(const float *dy, long dy_bs, const float *x, long x_bs, float *dw, float *scratch, int B, int Co,
                       int Ci, int Ldy, int Lx, int K, int dil, int pad, float in_slope, float alpha, int accumulate,
                       void *stream);
/* out[i] = dy[i] * (x[i] > 0 ? 1 : slope) (+ add[i]): a leaky ReLU's backward through its saved input, with the
 * residual branch's gradient added (add may be NULL; out may be dy or add). */
int mg_lrelu_bwd(const float *dy, const float *x, const float *add, float *out, float slope, size_t n, void *stream);
/* Backward of mg_conv1d_reflect_fwd (csrc/melgan_train.hip): y = act(alpha * W (*)_dil reflect_p(lrelu(x, in_slope)) + b),
 * p = dil (K-1)/2, K = 3 at dil <= 9 or K = 7 at dil = 1, p < L (MG_ERR_SHAPE otherwise).  dy is the gradient in front of
 * act.  Batch strides in floats, 0 = dense, never smaller than a plane.  No atomics: the bits repeat run to run.
 *   wgrad: dw[co,ci,k] (+)= alpha * sum_{b,l} dy[b,co,l] lrelu(x)[b,ci, refl(l + k dil - p)], refl(j) = -j for j < 0 and
 *          2(L-1) - j for j >= L; scratch of mg_conv1d_wgrad_scratch_floats(Co, Ci, K) floats.
 *   dgrad: packed = mg_conv_pack(w, MG_PACK_DGRAD); dy [B, Co, L] dense -> the zero-padded correlation over the padded
 *          length L + 2p into the workspace, then mg_reflect_fold_bwd with x [B, Ci, L] the saved pre-activation and the
 *          optional residual gradient add; dx [B, Ci, L] dense (dx may be add when add is dense).
 *   fold:  P [B, C, L + 2p] -> out [B, C, L] dense, out[b,c,i] = (P[i+p] + [1 <= i <= p] P[p-i] + [L-1-p <= i <= L-2] P[2(L-1)-i+p])
 *          * (x > 0 ? 1 : slope) (+ add), x NULL = no mask, add NULL = none; out may be a dense add, and with
 *          p = 0 a dense P: a leaky ReLU's backward with batch strides. */
int mg_conv1d_reflect_wgrad(const float *dy, long dy_bs, const float *x, long x_bs, float *dw, float *scratch, int B,
                            int Co, int Ci, int L, int K, int dil, float in_slope, float alpha, int accumulate,
                            void *stream);
size_t mg_conv1d_reflect_dgrad_workspace_floats(int B, int Ci, int L, int K, int dil);
int mg_conv1d_reflect_dgrad(const float *dy, const float *packed, const float *x, long x_bs, const float *add, long add_bs,
                            float *dx, float *workspace, size_t workspace_floats, int B, int Co, int Ci, int L, int K,
                            int dil, float in_slope, float alpha, void *stream);
int mg_reflect_fold_bwd(const float *P, long p_bs, const float *x, long x_bs, const float *add, long add_bs, float *out,
                        int B, int C, int L, int p, float slope, void *stream);
/* Backward of y = alpha * convT(lrelu(x, in_slope), w, stride u, padding u/2) (mg_conv_transpose1d_fwd), w [Ci, Co, 2u],
 * x [B, Ci, L], dy [B, Co, u L], u in {2,4,8}; out-of-range dy is 0.
 *   dgrad: dx[b,ci,l] = (x > 0 ? 1 : in_slope) * alpha * sum_{co,k} w[ci,co,k] dy[b,co, u l + k - u/2], dy read as u
 *          phases of length L: a 3-tap implicit GEMM with Ci rows over Co*u channels.  w is the plain weight.
 *   wgrad: dw[ci,co,k] (+)= alpha * sum_{b,l} lrelu(x[b,ci,l], in_slope) dy[b,co, u l + k - u/2]. */
size_t mg_conv_transpose1d_dgrad_workspace_floats(int B, int Ci, int L, int Co, int u);
int mg_conv_transpose1d_dgrad(const float *dy, const float *w, const float *x, float *dx, float *workspace,
                              size_t workspace_floats, int B, int Ci, int L, int Co, int u, float in_slope, float alpha,
                              void *stream);
size_t mg_conv_transpose1d_wgrad_scratch_floats(int Ci, int Co, int u);
int mg_conv_transpose1d_wgrad(const float *dy, const float *x, float *dw, float *scratch, int B, int Ci, int L, int Co,
                              int u, float in_slope, float alpha, int accumulate, void *stream);
/* Gradient of mg_stft_mel's mel with respect to the signal: dx [B, L] (batch stride dx_bs) from dmel [B, n_mels, T].
 * lengths must be NULL (MG_ERR_SHAPE otherwise); energy is not differentiated.  Frames whose mel sum is under the 1e-5
 * clamp and bins with |X| = 0 contribute 0.  Two passes: windowed frame gradients into the workspace, then a gather
 * that overlap-adds them in ascending frame order and folds the reflect padding back. */
size_t mg_stft_mel_bwd_workspace_bytes(int B, int T);
int mg_stft_mel_bwd(const float *x, long x_bs, const int *lengths, int B, int L, int hop, const float *window,
                    const float *twiddle, const int *band, const float *band_w, int n_mels, const float *dmel, int T,
                    float *dx, long dx_bs, void *workspace, size_t workspace_bytes, void *stream);

/* Step-embedding MLP: out = W2 mish(W0 [sin|cos](t * freq)).  Denoiser: model/modules.py:398-403,434;
 * JCUDiscriminator: model/mixgantts.py:203-208,265.  emb [B,D0], pre/h [B,D1] are saved for backward.
 * Where D0 % 256 == 0, W0 and emb must be 16-byte aligned, and where D1 % 256 == 0, W2 and h (those reductions run on
 * 16-byte loads); MG_ERR_ARG otherwise. */
int mg_step_mlp_fwd(const int64_t *t, const float *freq, const float *W0, const float *W2, float *emb,
                    float *pre, float *h, float *out, int B, int D0, int D1, int D2, void *stream);
/* g_out [B,D2] -> dW0 [D1,D0], dW2 [D2,D1]; scratch 2*B*D1 floats. */
int mg_step_mlp_bwd(const float *g_out, const float *emb, const float *pre, const float *h,
                    const float *W2, float *dW0, float *dW2, float *scratch, int B, int D0, int D1, int D2,
                    void *stream);
/* Bias-free per-sample Linear (LinearNorm on [B,K] vectors: speaker projections, spk_mlp).  Where K % 256 == 0 the
 * forward reads x and W with 16-byte loads: both must be 16-byte aligned then, MG_ERR_ARG otherwise. */
int mg_linear_small_fwd(const float *x, const float *W, float *out, int B, int N, int K, void *stream);
int mg_linear_small_bwd(const float *g, const float *x, const float *W, float *dx, float *dW, int B,
                        int N, int K, void *stream);

/* Stand-alone ResidualBlock.forward (model/blocks.py:1157-1176) on one layer's packs (mg_conv_pack: conditioner 1x1
 * MG_PACK_PLAIN, k=3 conv MG_PACK_GATE, output 1x1 MG_PACK_PLAIN), the same fused kernel mg_denoiser_fwd launches per
 * layer.  hvec [B,C] = Wd s (+ Wp spk) enters h, dvec [B,C] = Wd s the residual.  x_out [B,C,L] (must differ from x)
 * and skip [B,C,L] are written.  h/g/sig/tnh_save [B,C,L]: all four (training) or all NULL.  C = H = 256. */
int mg_resblock_fwd(const float *x, const float *cond, const float *wc_packed, const float *w3_packed,
                    const float *wo_packed, const float *bc, const float *b3, const float *bo, const float *hvec,
                    const float *dvec, float *x_out, float *skip, float *h_save, float *g_save, float *sig_save,
                    float *tnh_save, int B, int C, int H, int L, void *stream);
/* Derivative of the GLU gate g = sigmoid(z[:C]) * tanh(z[C:]) (model/blocks.py:1170-1171) through the saved
 * sigmoid / tanh values: dg, sig, tnh [B,C,L] -> dz [B,2C,L]. */
int mg_gate_bwd(const float *dg, const float *sig, const float *tnh, float *dz, int B, int C, int L, void *stream);
/* Mish.forward (model/blocks.py:894-896): y = x tanh(softplus(x)), and its derivative gx = gy * mish'(x). */
int mg_mish_fwd(const float *x, float *y, size_t n, void *stream);
int mg_mish_bwd(const float *gy, const float *x, float *gx, size_t n, void *stream);
/* DiffusionEmbedding.forward (model/blocks.py:906-913): emb [B,D] = [sin(t f) | cos(t f)], f [D/2] host table. */
int mg_step_embed(const int64_t *t, const float *freq, float *emb, int B, int D, void *stream);

/* Gradient of diffuse_trace (model/diffusion.py:167-175) w.r.t. x_start [B,L,M]: g is the stack [T+1,B,L,M] of the
 * gradients of the T+1 trace entries (entry 0 = clamped normalised x_start, entry t+1 = q_sample at step t); keep
 * uint8 [B,L] (0 = padded frame) or NULL; sqrt_alphas_cumprod [T]. */
int mg_diffuse_trace_bwd(const float *g, const float *x_start, const float *spec_min, const float *spec_max,
                         const uint8_t *keep, const float *sqrt_alphas_cumprod, float *d_x, int T, int B, int L, int M,
                         void *stream);

/* ------------------------------------------------------------------ aux pre-training
 * Strided batched fp32 GEMM on the MFMA: C[z](m,n) (+)= alpha * sum_k A[z](m,k) B[z](k,n), z = b*heads + h,
 * operand z at base + b*x_bs + h*x_hs; A(m,k) at m*a_ms + k*a_ks, B(k,n) at k*b_ks + n*b_ns (one stride of each
 * operand must be 1), C row-major with row stride c_ms.  The six contractions of train-mode attention and its
 * backward (transformer/Modules.py:16-23) are calls of this on the channel-major q/k/v and the kept [B*H,L,L]
 * probabilities. */
int mg_bgemm(const float *A, const float *B, float *C, int M, int N, int K, int batch, int heads, long a_ms, long a_ks,
             long a_bs, long a_hs, long b_ks, long b_ns, long b_bs, long b_hs, long c_ms, long c_bs, long c_hs,
             float alpha, int accumulate, void *stream);
/* 64 or 128: the workgroup tile mg_bgemm launches for these sizes (64 x 64 while the 128 x 128 tiles would number
 * fewer than 512).  MG_BGEMM_TILE=64|128 pins it; read on every call, any other value is ignored. */
int mg_bgemm_tile(int M, int N, int batch, int heads);
/* In place: S [B*H, L, L] -> softmax over keys of scale*S with padded keys (key_pad [B, L] != 0) at -inf. */
int mg_softmax_rows_fwd(float *S, const uint8_t *key_pad, int B, int H, int L, float scale, void *stream);
/* In place on dP: dS = scale * P o (dP - rowsum(dP o P)). */
int mg_softmax_rows_bwd(const float *P, float *dP, int B, int H, int L, float scale, void *stream);
/* Train-mode post-LayerNorm (transformer/SubLayers.py:54-55,90-91): pre = a * keep * drop_scale + res (keep: uint8
 * [B,C,L] dropout keep-mask or NULL), out = pad ? 0 : LN_c(pre) * gamma + beta; `pre` is saved for the backward. */
int mg_layernorm_cm_train_fwd(const float *a, const uint8_t *keep, float drop_scale, const float *res,
                              const float *gamma, const float *beta, const uint8_t *pad, float *pre, float *out, int B,
                              int C, int L, float eps, void *stream);
/* d_pre (= d res), d_a = d_pre * keep * drop_scale (optional); dgamma / dbeta are [32][C] partial sums ACCUMULATED
 * by atomics (the caller zeroes them and sums the 32 rows). */
int mg_layernorm_cm_bwd(const float *pre, const float *dy, const float *gamma, const uint8_t *pad, const uint8_t *keep,
                        float drop_scale, float *d_pre, float *d_a, float *dgamma, float *dbeta, int B, int C, int L,
                        float eps, void *stream);
/* BatchNorm1d with batch statistics + tanh + dropout of PostNet (transformer/Layers.py:131-134) on [B,C,L]:
 * mg_bn_stats -> per-channel mean and biased variance over (B,L);  mg_bn_act_fwd: y = act((x-mean)*invstd*gamma+beta)
 * (act MG_ACT_NONE|MG_ACT_TANH; y saved when tanh), out = y * keep * drop_scale;  backward in two passes:
 * _reduce -> dbeta = sum dpre, dgamma = sum dpre*xhat (dpre = dout*keep*drop_scale*act'(y)), then _apply ->
 * dx = gamma*invstd*(dpre - dbeta*inv_count - xhat*dgamma*inv_count)  (all-reduce the two vectors between the
 * passes for cross-rank statistics). */
int mg_bn_stats(const float *x, float *mean, float *var, int B, int C, int L, void *stream);
int mg_bn_act_fwd(const float *x, const float *mean, const float *invstd, const float *gamma, const float *beta,
                  const uint8_t *keep, float drop_scale, int act, float *y, float *out, int B, int C, int L, void *stream);
int mg_bn_act_bwd_reduce(const float *dout, const uint8_t *keep, float drop_scale, const float *y, const float *x,
                         const float *mean, const float *invstd, int act, float *dgamma, float *dbeta, int B, int C, int L,
                         void *stream);
int mg_bn_act_bwd_apply(const float *dout, const uint8_t *keep, float drop_scale, const float *y, const float *x,
                        const float *mean, const float *invstd, const float *gamma, const float *dgamma,
                        const float *dbeta, float inv_count, int act, float *dx, int B, int C, int L, void *stream);

/* ------------------------------------------------------------------ optimizer step on flat buffers
 * The update of train.py:75-85 per optimizer -- nn.utils.clip_grad_norm_(params, clip) then Adam.step()
 * (utils/model.py:32-40 builds torch.optim.Adam(lr, betas)) -- with gradients, parameters and both moments each in
 * ONE flat fp32 buffer of n elements (16-byte aligned):
 * mg_grad_norm: out[0] = ||g||_2 (fixed summation order), out[1] = min(1, max_norm / (out[0] + 1e-6)), the factor
 *   clip_grad_norm_ multiplies into every gradient; scratch holds mg_grad_norm_scratch_floats() floats.
 * mg_adam_flat: one Adam step (torch.optim.Adam's rule: L2 weight decay, m lerp, bias corrections from `step` >= 1,
 *   denom = sqrt(v)/sqrt(1-beta2^step) + eps) on g * grad_scale[0] (device scalar, e.g. out + 1 above; NULL = 1).
 *   g is not modified. */
size_t mg_grad_norm_scratch_floats(void);
int mg_grad_norm(const float *g, size_t n, float max_norm, float *scratch, float *out, void *stream);
int mg_adam_flat(float *p, const float *g, float *m, float *v, size_t n, float lr, float beta1, float beta2, float eps,
                 float weight_decay, long step, const float *grad_scale, void *stream);
/* Same; hyper (device, 2 floats, or NULL) = {lr / (1 - beta1^step), 1 / sqrt(1 - beta2^step)} is read by the kernel
 * instead of the values derived from the lr / step arguments -- a captured hipGraph of a training step replays this launch
 * with the numbers the host wrote there before the replay (HotPathTrainer.capture). */
int mg_adam_flat_dev(float *p, const float *g, float *m, float *v, size_t n, float lr, float beta1, float beta2, float eps,
                     float weight_decay, long step, const float *grad_scale, const float *hyper, void *stream);

/* ------------------------------------------------------------------ losses on the path (model/loss.py)
 * mg_loss_sum: out[0] = sum (a-c)^2 (mode 0: F.mse_loss against a constant label, loss.py:14-19)
 *              or sum |a-b| (mode 1: F.l1_loss numerator, loss.py:221-227); the caller divides by n.
 * mg_loss_grad: da = g[0] * coef * {2(a-c) | sign(a-b)}; g is a device scalar (no host sync). */
int mg_loss_sum(const float *a, const float *b, float c, int mode, size_t n, float *out, void *stream);
int mg_loss_grad(const float *a, const float *b, float c, int mode, const float *g, float coef, size_t n,
                 float *da, void *stream);
/* A weighted sum of mean-reduced terms in one launch: total = sum_k weight_k * mean_k, mean_k = mean (a-c)^2
 * (mode 0) or mean |a-b| (mode 1) over n elements -- the LSGAN pair of model/loss.py:12-30 and the feature-matching
 * sum of model/loss.py:221-227 are such sums.  out[0] = total, out[1+q] = the weighted subtotal of the terms with
 * group == q (q < MG_LOSS_GROUPS; e.g. adversarial and feature-matching parts for logging),
 * out[1+MG_LOSS_GROUPS+k] = mean_k; fixed summation order.  scratch:
 * mg_multi_loss_scratch_floats() floats, ZERO before the first call (the kernel keeps a ticket in it and re-arms it),
 * private to one stream.  mg_multi_loss_bwd: da_k = g[0] * weight_k / n_k * {2(a-c) | sign(a-b)} for every term
 * whose da is not NULL.
 * Two more modes for MelGAN's hinge objective: mode 2 = mean max(0, 1 + c a) (c = -1 on real logits, +1 on generated
 * ones; da = c where 1 + c a > 0, else 0) and mode 3 = mean a (da = 1), each times g[0] weight / n.  Any other mode is
 * MG_ERR_SHAPE before any launch. */
#define MG_LOSSMODE_MSE 0
#define MG_LOSSMODE_L1 1
#define MG_LOSSMODE_HINGE 2
#define MG_LOSSMODE_MEAN 3
#define MG_LOSS_MAX_TERMS 16
#define MG_LOSS_GROUPS 4
typedef struct MgLossTerm {
    const float *a;
    const float *b;   /* mode 1 only */
    float *da;        /* backward only; NULL = no gradient wanted */
    size_t n;
    float c;          /* mode 0: the constant; mode 2: the sign */
    float weight;
    int32_t mode;
    int32_t group;
} MgLossTerm;
size_t mg_multi_loss_scratch_floats(void);
int mg_multi_loss_fwd(const MgLossTerm *terms, int nterms, float *scratch, float *out, void *stream);
int mg_multi_loss_bwd(const MgLossTerm *terms, int nterms, const float *g, void *stream);
/* The same two launches with den[k] (host array, one entry per term) in place of n_k as the divisor -- in the per-term
 * "means" of out and in da_k = g[0] * weight_k / den_k * {...}; n_k stays the number of elements the term reads.  A
 * rank of a sharded batch passes the denominators of the WHOLE batch, so the ranks' totals add up to the single-process
 * loss.  MG_ERR_ARG for a NULL den or den[k] <= 0.  den[k] == n_k returns the bits of mg_multi_loss_fwd / _bwd. */
int mg_multi_loss_fwd_den(const MgLossTerm *terms, int nterms, const double *den, float *scratch, float *out,
                          void *stream);
int mg_multi_loss_bwd_den(const MgLossTerm *terms, int nterms, const double *den, const float *g, void *stream);
/* Masked mel L1 (loss.py:229-242,255-259) over rows = B*L frames of M bins, pad uint8 [rows] (1 = pad):
 * out2 = {sum |p-t| over counted rows, M * #counted rows}; the loss is out2[0]/out2[1]. */
int mg_mel_l1_fwd(const float *pred, const float *targ, const uint8_t *pad, int rows, int M, float *out2,
                  void *stream);
int mg_mel_l1_bwd(const float *pred, const float *targ, const uint8_t *pad, int rows, int M,
                  const float *g, const float *den, float *dpred, void *stream);
/* out[0] (device int64) = the number of rows mg_mel_l1_fwd counts: unpadded and with a non-zero entry in targ.  An
 * integer, so a SUM all-reduce of it over ranks is exact.  MG_ERR_ARG for a NULL targ / out (pad may be NULL),
 * MG_ERR_SHAPE for rows <= 0 or M <= 0. */
int mg_mel_count_rows(const float *targ, const uint8_t *pad, int rows, int M, int64_t *out, void *stream);

/* ------------------------------------------------------------------ FFT blocks (shallow / aux coarse mel)
 * Multi-head self-attention of transformer/SubLayers.py:29-57 + Modules.py:16-23 without the
 * [n_head*B, L, L] score tensor (streaming softmax, fp32 MFMA).  qkv [B, 3*n_head*d_head, L]
 * channel-major, rows = [Q heads | K heads | V heads], head-major like the reference's .view();
 * key_pad uint8 [B, L] (1 = padded key, masked with -inf for every query) or NULL;
 * out [B, n_head*d_head, L]; scale = 1/temperature = 1/sqrt(d_k).  d_head must be 128. */
int mg_attention_fwd(const float *qkv, const uint8_t *key_pad, float *out, int B, int L, int n_head,
                     int d_head, float scale, void *stream);
/* The same function with fp16 MFMA operands (q*scale, k, v and the probabilities rounded to fp16; fp32
 * accumulation, softmax statistics and I/O): BASELINE configs[4]'s "fp16 MFMA attention path" for L = 4000. */
int mg_attention_fwd_f16(const float *qkv, const uint8_t *key_pad, float *out, int B, int L, int n_head,
                     int d_head, float scale, void *stream);
/* The form mg_attention_fwd (f16 == 0) or mg_attention_fwd_f16 (f16 != 0) launches for these sizes; both switch on it.
 * fp32: MG_ATTN_KSPLIT128 while the 128-query workgroups would number fewer than 512, else MG_ATTN_WIDE256 while the
 * 256-query workgroups number at least 512, else MG_ATTN_PLAIN128.  MG_ATTENTION_KSPLIT=0|1|2 pins the first choice
 * (0 never, 1 MG_ATTN_KSPLIT64, 2 MG_ATTN_KSPLIT128) and MG_ATTENTION_WIDE=0|1 the second; both are read on every call
 * and any other value is ignored.  fp16 operands: only MG_ATTN_PLAIN128 and MG_ATTN_WIDE256 exist and only
 * MG_ATTENTION_WIDE is read.  MG_ERR_SHAPE for a size that is not positive. */
#define MG_ATTN_PLAIN128 0  /* 128 queries per workgroup, 4 waves */
#define MG_ATTN_KSPLIT64 1  /* 64 queries, 4 waves: wave pairs split the keys of every tile */
#define MG_ATTN_KSPLIT128 2 /* 128 queries, 8 waves: four query groups x two key halves */
#define MG_ATTN_WIDE256 3   /* 256 queries, 8 waves */
int mg_attention_form(int B, int L, int n_head, int f16);
/* Post-LayerNorm on the channel-major layout (SubLayers.py:55,91 + Layers.py:25,28):
 * out[b,c,l] = pad[b,l] ? 0 : LN_c(a[b,:,l] + res[b,:,l]) * gamma[c] + beta[c];  C must be 256. */
int mg_layernorm_cm_fwd(const float *a, const float *res, const float *gamma, const float *beta,
                        const uint8_t *pad, float *out, int B, int C, int L, float eps, void *stream);

/* ------------------------------------------------------------------ linguistic-encoder index ops
 * Device versions of the four functions of the LinguisticEncoder that loop over the batch in
 * Python with one .item() per phoneme.  Durations / counts are int64 like the reference's LongTensors.
 * LengthRegulator (model/linguistic_encoder.py:383-416): x [B,Tw,H], dur [B,Tw] (negative = 0) ->
 * out [B,Lmax,H] (rows past the expanded length are zero, longer expansions are cropped), mel_len [B]. */
int mg_length_regulate_fwd(const float *x, const int64_t *dur, float *out, int64_t *mel_len, int B,
                           int Tw, int H, int Lmax, void *stream);
int mg_length_regulate_bwd(const float *dout, const int64_t *dur, float *dx, int B, int Tw, int H,
                           int Lmax, void *stream);
/* word_level_pooling (utils/tools.py:394-413): src [B,Tp,H], wb [B,Tw] phones per word,
 * src_w_len [B] -> out [B,Wout,H] (sum, or mean when mean != 0). */
int mg_word_pool_fwd(const float *src, const int64_t *wb, const int64_t *src_w_len, float *out, int B,
                     int Tp, int Tw, int H, int Wout, int mean, void *stream);
int mg_word_pool_bwd(const float *dout, const int64_t *wb, const int64_t *src_w_len, float *dsrc, int B,
                     int Tp, int Tw, int H, int Wout, int mean, void *stream);
/* get_mapping_mask (model/linguistic_encoder.py:185-199): out uint8 [B,Lq,Lkv], 1 inside the
 * (frames of word i) x (phonemes of word i) blocks. */
int mg_mapping_mask(const int64_t *dur_w, const int64_t *wb, const int64_t *src_w_len, uint8_t *out,
                    int B, int Tw, int Lq, int Lkv, void *stream);
/* get_rel_coef (model/linguistic_encoder.py:222-236): mask uint8 [B,Lout] (1 = valid) -> out [B,Lout]. */
int mg_rel_coef(const int64_t *dur, const int64_t *dur_len, const uint8_t *mask, float *out, int B, int T,
                int Lout, void *stream);

/* ------------------------------------------------------------------ linguistic encoder, inference (lingenc.hip)
 * Windowed relative-position self-attention (model/blocks.py:1016-1123, heads_share=True):
 * qkv [B, 3*H*D, L] channel-major (q, k, v stacked), valid uint8 [B,L] (1 = valid), emb_k / emb_v
 * [2*window+1, D] -> out [B, H*D, L] (before conv_o).  Scores masked with -1e4 where valid[i]*valid[j] == 0,
 * so padded queries come out finite (the reference's uniform rows).  D must be 128, window <= 8, L <= 2895. */
int mg_rel_attention_fwd(const float *qkv, const uint8_t *valid, const float *emb_k, const float *emb_v, float *out,
                         int B, int L, int n_head, int d_head, int window, void *stream);
/* Word-to-phoneme attention (model/blocks.py:695-768): q [B, H*D, Lq], kv [B, 2*H*D, Lk] (k then v) channel-major;
 * key_valid [B,Lk], query_valid [B,Lq], mapping [B,Lq,Lk] uint8; prior [B,Lk,Lq] or NULL (helper_type "ctc").
 * Writes out [B, H*D, Lq] and the head-major [H, B, Lq, Lk] tensors attn (= attn_raw * mapping), attn_raw
 * (= softmax * query mask) and logprob (the scores, -inf at padded keys).  D must be 128, Lk <= 2895. */
int mg_w2p_attention_fwd(const float *q, const float *kv, const uint8_t *key_valid, const uint8_t *query_valid,
                         const uint8_t *mapping, const float *prior, float *out, float *attn, float *attn_raw,
                         float *logprob, int B, int Lq, int Lk, int n_head, int d_head, void *stream);
/* Query rows per workgroup of the three attentions above (mg_rel_attention_fwd, mg_rel_attention_train_fwd,
 * mg_w2p_attention_fwd; their launcher switches on it) for Lk keys: 16 while 16 score rows fit the 64 KiB of dynamic
 * LDS (Lk <= 615), else 4 (Lk <= 2895), else 0: those entry points return MG_ERR_SHAPE.  0 for Lk <= 0. */
int mg_le_attention_rows(int Lk);
/* nn.Embedding into channel-major: out[b,c,l] = valid[b,l] ? table[ids[b,l], c] : 0 (table [n_rows, C]). */
int mg_embed_cm(const int64_t *ids, const float *table, const uint8_t *valid, float *out, int B, int L, int C,
                int n_rows, void *stream);
/* VariancePredictor head (model/linguistic_encoder.py:163-183,473-478) on h [B,C,L] channel-major:
 * pred[b,l] = (weight . h[b,:,l] + bias) * valid[b,l] (* control when target is NULL).  With emb [n_bounds+1, C]:
 * x[b,:,l] += emb[bucketize(target or pred, bins[n_bounds])] at every frame, pads included. */
int mg_variance_head(const float *h, const float *weight, const float *bias, const uint8_t *valid, float control,
                     const float *target, const float *bins, int n_bounds, const float *emb, float *pred, float *x,
                     int B, int C, int L, void *stream);
/* Word-level duration (model/linguistic_encoder.py:294-316): logw [B,W] = log(word sum of exp(logp [B,Tp]))
 * (-inf past src_w_len); dur [B,W] int64 = the word sum of target [B,Tp] (int64) when given, else
 * max(rint(exp(logw) - 1) * d_control, 0) truncated. */
int mg_duration_head(const float *logp, const int64_t *target, const int64_t *wb, const int64_t *src_w_len,
                     float d_control, float *logw, int64_t *dur, int B, int Tp, int Tw, int W, void *stream);
/* add_position_enc (model/linguistic_encoder.py:201-220): out [B,C,L] = x + coef[b,l] * table[l,c];
 * x is [B,L,C] when x_rowmajor, else [B,C,L]; table [>=L, C]. */
int mg_posenc_add(const float *x, int x_rowmajor, const float *coef, const float *table, float *out, int B, int C,
                  int L, void *stream);

/* ------------------------------------------------------------------ linguistic encoder, training (lingenc.hip,
 * lingenc_train.hip).  Every reduction has a fixed order: two runs give bit-identical gradients.
 * Train-mode relative self-attention: mg_rel_attention_fwd plus dropout on the probabilities (model/blocks.py:1059)
 * with keep [B,H,L,L] uint8 (NULL: none) and keep_scale = 1/(1-p); P [B,H,L,L] receives the softmax before dropout
 * (NULL: not saved). */
int mg_rel_attention_train_fwd(const float *qkv, const uint8_t *valid, const float *emb_k, const float *emb_v,
                               const uint8_t *keep, float keep_scale, float *out, float *P, int B, int L, int n_head,
                               int d_head, int window, void *stream);
/* Workspace (floats) of mg_rel_attention_bwd; 0 for unsupported sizes. */
size_t mg_rel_attention_bwd_ws_floats(int B, int L, int n_head, int window);
/* Backward of mg_rel_attention_train_fwd: dOut [B,H*D,L] -> dqkv [B,3*H*D,L], d_emb_k / d_emb_v [2*window+1, D]
 * (summed over batch, heads and queries: the heads share one table).  Masked scores pass no gradient. */
int mg_rel_attention_bwd(const float *qkv, const uint8_t *valid, const float *P, const uint8_t *keep, float keep_scale,
                         const float *dOut, const float *emb_k, const float *emb_v, float *dqkv, float *d_emb_k,
                         float *d_emb_v, float *ws, size_t ws_floats, int B, int L, int n_head, int d_head, int window,
                         void *stream);
/* Workspace (floats) of mg_w2p_attention_bwd. */
size_t mg_w2p_attention_bwd_ws_floats(int B, int Lq, int Lk, int n_head);
/* Backward of mg_w2p_attention_fwd from its inputs and its attn / attn_raw / logprob outputs.  Upstream gradients:
 * dOut [B,H*D,Lq], and d_attn / d_raw / d_logprob [H,B,Lq,Lk] each NULL when zero.  -> dq [B,H*D,Lq],
 * dkv [B,2*H*D,Lk].  Padded keys (-inf scores) get exactly zero. */
int mg_w2p_attention_bwd(const float *q, const float *kv, const uint8_t *key_valid, const uint8_t *query_valid,
                         const uint8_t *mapping, const float *prior, const float *attn, const float *attn_raw,
                         const float *logprob, const float *dOut, const float *d_attn, const float *d_raw,
                         const float *d_logprob, float *dq, float *dkv, float *ws, size_t ws_floats, int B, int Lq,
                         int Lk, int n_head, int d_head, void *stream);
/* nn.Embedding gradient: dtable [n_rows, C] (overwritten) = sum of dout[b,:,l] over the tokens with ids[b,l] == row
 * (and valid[b,l], when valid is not NULL); row skip_row (padding_idx, or -1) is zero. */
int mg_embed_cm_bwd(const int64_t *ids, const float *dout, const uint8_t *valid, float *dtable, int B, int L, int C,
                    int n_rows, int skip_row, void *stream);
/* Backward of mg_variance_head's prediction: g = dpred * valid * scale (scale = control without a target, else 1);
 * dh [B,C,L] = weight[c] g, dweight [C] = sum h g, dbias [1] = sum g. */
int mg_variance_head_bwd(const float *h, const float *weight, const uint8_t *valid, float scale, const float *dpred,
                         float *dh, float *dweight, float *dbias, int B, int C, int L, void *stream);
/* Backward of mg_duration_head's logw: dlogp [B,Tp] = dlogw[word] * exp(logp - logw[word]), 0 outside counted words. */
int mg_duration_head_bwd(const float *logp, const float *logw, const float *dlogw, const int64_t *wb,
                         const int64_t *src_w_len, float *dlogp, int B, int Tp, int Tw, int W, void *stream);
/* Backward of mg_posenc_add into the table: dtable [L,C] = sum_b coef[b,l] * dout[b,c,l] (dout channel-major). */
int mg_posenc_add_bwd(const float *dout, const float *coef, float *dtable, int B, int C, int L, void *stream);
/* Dropout with a given keep-mask: out[e] = keep[e] ? x[e] * scale : 0 (also its own backward). */
int mg_dropout_apply(const float *x, const uint8_t *keep, float scale, float *out, size_t n, void *stream);

/* DeepSpeaker ResCNN speaker embedder (reference deepspeaker package; csrc/deepspeaker.hip), fp32.
 * Filterbank front end: audio [B, x_bs] fp32; item b's trimmed signal is audio[b, start[b] : end[b]) (end > start);
 * out [B, frames, nfilt] = the normalised fbank of its frames offset[b] .. offset[b] + frames - 1 (frame_len samples
 * every frame_step, pre-emphasis 0.97, rectangular window, zero-padded 1024-point power spectrum / 1024, banded
 * filters as mg_stft_mel's band table, exact zeros -> DBL_EPSILON, per-frame (v - mean) / max(std, 1e-12)); rows at
 * or past the item's frame count are zeros.  frame_len <= MG_STFT_N, nfilt <= 64. */
int mg_ds_fbank(const float *audio, long x_bs, const int *start, const int *end, const int *offset, int B, int frames,
                int frame_len, int frame_step, const float *twiddle, const int *band, const float *band_w, int nfilt,
                float *out, void *stream);
/* 2-D convolution with TF 'same' padding (asymmetric: pad_total / 2 before), NHWC: x [Nb, H, W, Ci], w packed
 * [(kh ks + kw) Ci + ci][Co] (BN folded), y [Nb, ceil(H / stride), ceil(W / stride), Co] = clip(conv + bias, 0, 20),
 * then with res (same shape as y, or NULL) clip(y + res, 0, 20).  Co % 64 == 0; Ci % 32 == 0 runs the MFMA implicit
 * GEMM, other Ci a direct kernel. */
int mg_ds_conv2d(const float *x, const float *w, const float *bias, const float *res, float *y, int Nb, int H, int W,
                 int Ci, int Co, int ks, int stride, void *stream);
/* Head: out [B, O] = l2_normalize(mean over rows of x[b] ([rows, D]) . w [D, O] + bias).  O % 64 == 0, O <= 512. */
int mg_ds_head(const float *x, const float *w, const float *bias, float *out, int B, int rows, int D, int O,
               void *stream);

/* ------------------------------------------------------------------ corpus builder (preprocessor/preprocessor.py;
 * csrc/corpus.hip).
 * Beta-binomial alignment prior (:384-393 as called at :344-348), batched and padded: out [B, T, L], float32 or
 * (out_f64) float64.  src_lens, mel_lens: device int32 [B].  For phoneme row i < src_lens[b] and frame
 * k < mel_lens[b]: out[b, i, k] = betabinom(n = mel_len, a = s (i + 1), b = s (src_len - i)).pmf(k), evaluated in
 * float64; every other element is 0.  The caller passes T >= max(src_lens) and L >= max(mel_lens): a length beyond
 * them is not an error here (checking would need a host read) but is clamped, src_len to T and mel_len to L, and
 * the row is then the distribution of the clamped lengths, not a cut of the true one.  scaling points to the HOST
 * value s > 0, read before the launch. */
int mg_betabinom_prior(const int *src_lens, const int *mel_lens, const double *scaling, void *out, int B, int T, int L,
                       int out_f64, void *stream);
/* Frame level -> phoneme level (:311-341).  values [B, L], durations int32 [B, T], n_frames / n_phon int32 [B],
 * out [B, T]: out[b, i] = mean(values[b, pos_i : pos_i + d_i]) cut at n_frames[b], 0 where d_i == 0 or
 * i >= n_phon[b].  pitch == 0: float32 in and out (energy).  pitch == 1: float64 in and out, and zero frames are first
 * replaced by linear interpolation between their non-zero neighbours, the first / last non-zero value outside them; an
 * utterance needs at least one non-zero frame.  The reference averages in place, so segments with pos_i < i read
 * earlier results: reproduced.  T <= 2048, L <= 4096. */
int mg_phoneme_average(const void *values, const int *durations, const int *n_frames, const int *n_phon, void *out,
                       int B, int T, int L, int pitch, void *stream);

/* ------------------------------------------------------------------ prepare_align (prepare_align.py,
 * preprocessor/ljspeech.py, preprocessor/aishell3.py; csrc/resample.hip).
 * Rational-ratio polyphase resampler over a ragged batch: what librosa.load(path, sr) does to a wav of another rate.
 * x [B, N] with batch stride x_bs, lengths [B] device int32 (null: all N; clamped to [0, N]); y [B, M] with batch
 * stride y_bs.  up / down is the reduced ratio target rate / source rate.  With h the centred low-pass of odd length
 * 2 half + 1 and out_len[b] = ceil(lengths[b] up / down):
 *   y[b, n] = up sum_k h[n down - k up + half] x[b, k]   over 0 <= k < lengths[b] with the h index in [0, 2 half],
 * for n < min(out_len[b], M), and y[b, n] = 0 for out_len[b] <= n < M: zero extension at both ends, zero delay,
 * scipy.signal.resample_poly(x, up, down, window=h).  Nothing at or beyond lengths[b] is read.  n down is formed in
 * 64 bits.  up == down == 1 copies (h is not used; taps may be null).
 * taps: the phase-major table [up, Kp] with the factor up folded in, rows ascending in the input index.  With
 * Mh = half / up + 1 and n down = q up + r (0 <= r < up):
 *   taps[r, j] = up h[(Mh - 1 - j) up + r + half]  (0 where that index is outside [0, 2 half]; 0 for j >= 2 Mh),
 *   y[b, n]    = sum_{j < Kp} taps[r, j] x[b, q - Mh + 1 + j].
 * Kp >= 2 Mh, Kp % 4 == 0, taps 16-byte aligned.  MG_ERR_SHAPE beyond the limits below; the staged input span of one
 * tile, (MG_RESAMPLE_TILE - 1) down / up + Kp + 2 samples, must not exceed MG_RESAMPLE_MAX_SPAN. */
#define MG_RESAMPLE_MAX_UP 1024
#define MG_RESAMPLE_MAX_TAPS 1024 /* Kp, taps per output */
#define MG_RESAMPLE_TILE 1024     /* consecutive outputs of one workgroup */
#define MG_RESAMPLE_MAX_SPAN 16384
int mg_resample_poly(const float *x, long x_bs, const int *lengths, int B, int N, const float *taps, int up, int down,
                     int Kp, int half, float *y, long y_bs, int M, void *stream);
/* Peak normalisation to int16 (ljspeech.py:29-34, aishell3.py:32-37): x [B, N] ragged as above, out int16 [B, N] with
 * batch stride out_bs.  q = trunc((x / max_k |x[b, k]|) max_wav_value) in float32, in that order, saturated to
 * [-32768, 32767] (the reference's cast wraps +32768 to -32768); an all-zero row gives zeros (the reference divides
 * by zero); out[b, k] = 0 for k >= lengths[b]. */
int mg_peak_normalize_i16(const float *x, long x_bs, const int *lengths, int B, int N, float max_wav_value,
                          int16_t *out, long out_bs, void *stream);

/* ------------------------------------------------------------------ pitch extraction (csrc/pitch.hip; stands where
 * preprocessor.py:295-300 calls pyworld, with no claim of parity).  Both calls take ragged batches.
 * Stage 1, YIN candidates: x [B, L] with batch stride x_bs, lengths [B] device int32 (null: all L; clamped to
 * [0, L]); row b has lengths[b] / hop + 1 frames, frame k the MG_PITCH_N samples from k hop - MG_PITCH_N / 2 on, zero
 * outside the row (nothing at or past lengths[b] is read).  With W = MG_PITCH_W,
 *   d(tau) = sum_{j < W} (x_j - x_{j+tau})^2,  d'(tau) = d(tau) tau / sum_{1 <= j <= tau} d(j)  (1 at tau = 0 and where
 * the sum is 0), and the MG_PITCH_K deepest local minima of d' over [tau_min, tau_max] (strictly below the left
 * neighbour, not above the right one) leave in increasing lag: period [B, T, K] = lag + a three-point parabolic offset
 * clamped to +-0.5 (0 when the second difference is not positive), cost [B, T, K] = d' at the lag; an empty slot holds
 * period 0 and cost 1e30.  rms [B, T] is the frame's root mean square over its MG_PITCH_N samples.  Frames at or past
 * a row's count are zero in all three.  MG_ERR_SHAPE unless 2 <= tau_min <= tau_max, tau_max + 1 <= MG_PITCH_N -
 * MG_PITCH_W, hop >= 1 and 1 <= T <= L / hop + 1.  twiddle: the 1024 complex float32 roots exp(-2 pi i n / 1024). */
#define MG_PITCH_N 1024
#define MG_PITCH_W 512
#define MG_PITCH_K 4
int mg_yin_candidates(const float *x, long x_bs, const int *lengths, int B, int L, int hop, int tau_min, int tau_max,
                      const float *twiddle, float *period, float *cost, float *rms, int T, void *stream);
/* Stage 2, the track: a Viterbi pass per row over the K candidate slots and one unvoiced state, in float64, over the
 * first n_frames[b] (device int32, clamped to [0, T]) frames of stage 1's output.  params is a host array of
 * MG_PITCH_PARAMS doubles indexed by MG_PITCH_P_*: the sampling rate, tau_max, theta (cost of an unvoiced frame),
 * beta (a voiced slot costs cost + beta period / tau_max), lambda (voiced to voiced costs lambda |log2 p_a - log2 p_b|),
 * switch (voiced to unvoiced and back) and gate (frames whose rms is below gate times the row's largest have no voiced
 * state).  Ties go to the lowest state.  f0 [B, T] float64 = rate / period on voiced frames, 0 elsewhere and past
 * n_frames[b].  workspace: mg_pitch_track_workspace_bytes(B, T) bytes of device memory for the back-pointers;
 * MG_ERR_WORKSPACE when it is null or smaller. */
#define MG_PITCH_PARAMS 7
#define MG_PITCH_P_SR 0
#define MG_PITCH_P_TAU_MAX 1
#define MG_PITCH_P_THETA 2
#define MG_PITCH_P_BETA 3
#define MG_PITCH_P_LAMBDA 4
#define MG_PITCH_P_SWITCH 5
#define MG_PITCH_P_GATE 6
size_t mg_pitch_track_workspace_bytes(int B, int T);
int mg_pitch_track(const float *period, const float *cost, const float *rms, const int *n_frames, int B, int T,
                   const double *params, double *f0, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ forced alignment (aligner.py; csrc/align.hip;
 * stands where the corpus chain calls the Montreal Forced Aligner, with no claim of parity).  A monophone left-to-right
 * HMM with one diagonal Gaussian per state; all three calls take ragged batches, read nothing at or past a row's
 * length, use no atomics and give a row the same bits wherever it sits in the batch.
 * Emissions: x [B, T, D] features, n_frames [B] device int32, tables A, Bm [G, D] and c [G]
 * (A = -0.5 / var, Bm = mean / var, c = -0.5 sum_d (mean^2 / var + log(2 pi var))):
 *   ll[b, t, g] = sum_d (A[g, d] x[b, t, d]^2 + Bm[g, d] x[b, t, d]) + c[g]   for t < n_frames[b], 0 elsewhere,
 * accumulated in float32 over ascending d.  MG_ERR_SHAPE unless B, T >= 1, 1 <= D <= MG_ALIGN_MAX_D,
 * 1 <= G <= MG_ALIGN_MAX_G and B T <= 65535 * 64. */
#define MG_ALIGN_MAX_D 128
#define MG_ALIGN_MAX_G 1024
#define MG_ALIGN_MAX_S 2048
#define MG_ALIGN_MAX_T 4096
int mg_align_emissions(const float *x, const int *n_frames, int B, int T, int D, const float *A, const float *Bm,
                       const float *c, int G, float *ll, void *stream);
/* Viterbi: ll [B, T, G] as above, seq int32 [B, S] the Gaussian of each state (clamped to [0, G)), skip uint8 [B, S]
 * non-zero where a state may be passed over, n_frames / n_states int32 [B] (clamped to [0, T] / [0, S]), all on the
 * device.  With e_t(s) = ll[b, t, seq[b, s]], in float64:
 *   delta_0(s) = e_0(s) for s = 0, and for s = 1 if skip[0]; -inf otherwise,
 *   delta_t(s) = e_t(s) + max(delta_{t-1}(s), delta_{t-1}(s-1), skip[s-1] ? delta_{t-1}(s-2) : -inf),
 * ties to the smallest jump (stay, then advance, then skip); the path ends in state n_states - 1, or in n_states - 2
 * when skip[n_states - 1] and its delta is strictly larger.  A skippable state must have non-skippable neighbours:
 * skip lives on the device, so this call cannot check it, and the Python wrapper refuses two adjacent skippable states
 * (MG_ERR_SHAPE) before it uploads them.  durations int32 [B, S]: frames spent in each state, 0 for a state passed
 * over and for s >= n_states[b]; score [B] float64: delta at the end; ok int32 [B]: 0, with all-zero durations and
 * score -inf, when no path exists (fewer frames than non-skippable states, no frames, no states).
 * 1 <= S <= MG_ALIGN_MAX_S, 1 <= T <= MG_ALIGN_MAX_T, 1 <= G <= MG_ALIGN_MAX_G.  workspace:
 * mg_align_viterbi_workspace_bytes(B, T, S) bytes of device memory for the back-pointers, two bits each;
 * MG_ERR_WORKSPACE when it is null or smaller. */
size_t mg_align_viterbi_workspace_bytes(int B, int T, int S);
int mg_align_viterbi(const float *ll, const int *seq, const uint8_t *skip, const int *n_frames, const int *n_states,
                     int B, int T, int S, int G, int *durations, double *score, int *ok, void *workspace,
                     size_t workspace_bytes, void *stream);
/* Statistics of the hard-EM update: x [rows, D]; frame_index int32: the row numbers of the frames in use, stably
 * sorted by Gaussian; offsets int32 [G + 1]: Gaussian g owns frame_index[offsets[g] : offsets[g + 1]].  sum and
 * sumsq float64 [G, D]: the sums of x and x^2 over the Gaussian's rows, added in list order; zeros for an empty
 * segment.  The lists live on the device: their bounds are the caller's to keep (the Python wrapper checks them).
 * 1 <= D <= MG_ALIGN_MAX_D, 1 <= G <= MG_ALIGN_MAX_G. */
int mg_align_stats(const float *x, const int *frame_index, const int *offsets, int G, int D, double *sum,
                   double *sumsq, void *stream);

/* ------------------------------------------------------------------ objective synthesis metrics (metrics.py;
 * csrc/dtw.hip): mel-cepstral distortion along a dynamic-time-warping path.  All calls take ragged batches with device
 * int32 length arrays (clamped to the padded length), read nothing at or past a row's length, use no atomics and give
 * a pair the same bits wherever it sits in the batch and on every run.
 * Cepstra: mel [B, T, M] natural-log mel, n_frames [B]; out [B, T, n_coef] holds the coefficients 1 .. n_coef of the
 * orthonormal DCT-II over the M bins (c0, the energy term, is left out):
 *   out[b, t, k - 1] = sqrt(2 / M) sum_m mel[b, t, m] cos(pi / M (m + 1/2) k)   for t < n_frames[b], 0 elsewhere,
 * accumulated in float32 over ascending m.  MG_ERR_SHAPE unless 1 <= B <= 65535, T >= 1 and
 * 1 <= n_coef < M <= MG_CEPSTRA_MAX_M. */
#define MG_CEPSTRA_MAX_M 128
#define MG_DTW_MAX_T 4096
#define MG_DTW_MAX_D 64
int mg_mel_cepstra(const float *mel, const int *n_frames, int B, int T, int M, int n_coef, float *out, void *stream);
/* DTW: a [B, Ta, D], b [B, Tb, D], a_len / b_len [B].  With c(i, j) = sqrt(sum_d (a[i, d] - b[j, d])^2) in float32,
 *   Dacc(0, 0) = c(0, 0),  Dacc(i, j) = c(i, j) + min(Dacc(i-1, j-1), Dacc(i-1, j), Dacc(i, j-1))
 * over the predecessors that exist; ties go to the diagonal, then to (i-1, j), then to (i, j-1).  total [B] float32:
 * Dacc(a_len - 1, b_len - 1); path_len [B] int32: the cells on the back-traced path; path [B, Ta + Tb - 1, 2] int32,
 * may be null: the (i, j) cells in ascending order, -1 in the rows past path_len.  A pair with a_len or b_len 0 gives
 * total 0, path_len 0 and a path of -1.  MG_ERR_SHAPE unless B >= 1, 1 <= Ta, Tb <= MG_DTW_MAX_T and
 * 1 <= D <= MG_DTW_MAX_D.  workspace: mg_dtw_workspace_bytes(B, Ta, Tb) bytes of device memory,
 *   4 B (ceil(Tb / 16) Ta + MG_DTW_MAX_D (Ta + Tb)):
 * the back-pointers, two bits a cell, and a feature-major copy of both operands (sized for the largest D, so that
 * the query needs none); MG_ERR_WORKSPACE when it is null or smaller.  Every error returns before any launch. */
size_t mg_dtw_workspace_bytes(int B, int Ta, int Tb);
int mg_dtw(const float *a, const float *b, const int *a_len, const int *b_len, int B, int Ta, int Tb, int D,
           float *total, int *path_len, int *path, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ HiFi-GAN multi-scale discriminator (msd.hip)
 * Grouped strided Conv1d, channel-major [N, C, L], weight in torch's [Co, Ci/G, K] layout:
 *   out[n, g Cog + co, l] = act(sum_{ci<Cig, k<K} w[g Cog + co, ci, k] in[n, g Cig + ci, l s + k - pad] + bias),
 * in out of range = 0, Lout = (Lin + 2 pad - K) / s + 1 (MG_ERR_SHAPE otherwise), act MG_ACT_NONE or MG_ACT_LRELU with
 * the runtime `slope`.  Instantiated (Cig, Cog, K, s): (32,32,41,2) (8,16,41,2) (16,32,41,4) (32,64,41,4) (64,64,41,1),
 * the DiscriminatorS stack, for any G >= 1; every other form is MG_ERR_SHAPE (a packed size of 0) before any launch,
 * a null pointer MG_ERR_ARG.  `packed` is a derived cache in MFMA fragment order, per group:
 *   MG_GCONV_FWD   [G][Cog/32 up][K][Cig/2][64]: lane -> w[row lane&31, ci 2q + lane>>5, tap]
 *   MG_GCONV_DGRAD [G][Cig/32 up][K taps ordered by (k mod s, k div s)][Cog/2][64]: lane -> w[co 2q + lane>>5, row lane&31, tap]
 * rows past Cog (Cig) are zero.
 * MelGAN's discriminator (Kumar et al. 2019) has four input channels per group: (4,16,41,4) and (4,4,41,4) are
 * instantiated too, behind the same entry points and with the same semantics, on VALU kernels that put 16 (Cog = 4) or
 * 4 (Cog = 16) groups side by side in a workgroup and several in every wave (csrc/gconv_c4.h).  Their packs are plain
 * transposes, G Cog 4 K floats in either mode:
 *   MG_GCONV_FWD   [G][ci 4][K][Cog]: four consecutive output rows of one (ci, tap) are one 16-byte load
 *   MG_GCONV_DGRAD [G][Cog][K][ci 4]: the four input channels of one (co, tap) are one 16-byte load */
#define MG_GCONV_FWD 0
#define MG_GCONV_DGRAD 1
size_t mg_gconv_packed_floats(int Ci, int Co, int K, int stride, int groups, int mode);
int mg_gconv_pack(const float *w, float *packed, int Ci, int Co, int K, int stride, int groups, int mode, void *stream);
int mg_gconv1d_fwd(const float *in, const float *packed, const float *bias, float *out, int N, int Ci, int Lin, int Co,
                   int Lout, int K, int stride, int pad, int groups, int act, float slope, void *stream);
/* Data gradient of mg_gconv1d_fwd in polyphase form (per output phase (m + pad) mod s a stride-1 convolution over dy with
 * ceil(K / s) taps; no zero insertion):
 *   dx[n, g Cig + ci, m] = (sum_{co, k : (m + pad - k) = s l} w[g Cog + co, ci, k] dy[n, g Cog + co, l] + add) * mask,
 * mask = map > 0 ? 1 : slope from the layer below's stored activated map (NULL: no mask); add (NULL: none) is a
 * gradient that reaches the same map from elsewhere.  map, add and dx are [N, Ci, Lin]; positions no output read get
 * exactly add * mask.  packed: the MG_GCONV_DGRAD form. */
int mg_gconv1d_dgrad(const float *dy, const float *packed, const float *map, const float *add, float *dx, int N, int Ci,
                     int Lin, int Co, int Lout, int K, int stride, int pad, int groups, float slope, void *stream);
/* dw[g Cog + co, ci, k] = sum_{n,l} dy[n, g Cog + co, l] x[n, g Cig + ci, l s + k - pad].  A workgroup stages 64 frames
 * of dy and the matching x window once and takes every tap from it as an address offset; workgroups split (n, l) and
 * write partial tiles to `scratch`, a second kernel adds them in ascending order: two runs are bit-identical.  The bias
 * gradient is mg_rowsum of dy. */
size_t mg_gconv1d_wgrad_scratch_floats(int N, int Ci, int Co, int Lout, int K, int stride, int groups);
int mg_gconv1d_wgrad(const float *dy, const float *x, float *dw, float *scratch, size_t scratch_floats, int N, int Ci,
                     int Lin, int Co, int Lout, int K, int stride, int pad, int groups, void *stream);
/* The first layer, Conv1d(1, Co, K, stride 1): in [N, 1, L], w [Co, 1, K], Lout = L + 2 pad - K + 1 >= 1, K <= 16,
 * plain VALU kernels (one input channel leaves the matrix pipe nothing to reduce over).  fwd applies act as above;
 * dgrad: dx[n, m] = sum_{co,k} w[co,k] dy[n, co, m + pad - k]; wgrad writes dw [Co, K] and db [Co] (db may be NULL)
 * through partial sums in `scratch` added in a fixed order. */
int mg_conv1d_c1_fwd(const float *in, const float *w, const float *bias, float *out, int N, int L, int Co, int K, int pad,
                     int act, float slope, void *stream);
int mg_conv1d_c1_dgrad(const float *dy, const float *w, float *dx, int N, int L, int Co, int K, int pad, void *stream);
size_t mg_conv1d_c1_wgrad_scratch_floats(int N, int L, int Co, int K);
int mg_conv1d_c1_wgrad(const float *dy, const float *x, float *dw, float *db, float *scratch, size_t scratch_floats,
                       int N, int L, int Co, int K, int pad, void *stream);
/* AvgPool1d(4, 2, padding 2), padding counted (always / 4): in [rows, L] -> out [rows, L / 2 + 1], and its backward
 * dx[r, m] = (dy[r, (m + 2) / 2] + dy[r, (m + 2) / 2 - 1]) / 4 over the outputs that exist. */
int mg_avgpool4s2_fwd(const float *in, float *out, int rows, int L, void *stream);
int mg_avgpool4s2_bwd(const float *dy, float *dx, int rows, int L, void *stream);
/* MelGAN's pool, AvgPool1d(4, 2, padding 1, count_include_pad = False): in [rows, L] -> out [rows, (L - 2) / 2 + 1],
 * out[r, i] = mean of in[r, 2 i - 1 .. 2 i + 2] over the samples in range (the edge windows divide by 3, or by 2 where
 * L = 2), and its backward.  L < 2 is MG_ERR_SHAPE. */
int mg_avgpool4s2p1_fwd(const float *in, float *out, int rows, int L, void *stream);
int mg_avgpool4s2p1_bwd(const float *dy, float *dx, int rows, int L, void *stream);
/* ReflectionPad1d(p) on rows of T samples: out [rows, T + 2 p], out[r, i] = in[r, reflect(i - p)], reflect(j) = -j below
 * 0 and 2 (T - 1) - j past T - 1; and its backward dx [rows, T]: dx[r, m] = dy[r, m + p] plus the mirrored pad samples
 * that read m (m in [1, p] from the left pad, m in [T - 1 - p, T - 2] from the right), added in that fixed order.
 * p < 0 or T <= p is MG_ERR_SHAPE. */
int mg_reflect_pad1d_fwd(const float *in, float *out, int rows, int T, int p, void *stream);
int mg_reflect_pad1d_bwd(const float *dy, float *dx, int rows, int T, int p, void *stream);

/* ------------------------------------------------------------------ HiFi-GAN multi-period discriminator (mpd.hip)
 * DiscriminatorP(p) as six plain 1-D convolutions on a SLOTTED flat axis.  For T samples, reflect-padded on the right
 * to a multiple of p, mg_period_geometry writes the heights H[0..6] (H[0] = ceil(T / p), H[j+1] = (H[j] - 1) / 3 + 1
 * for the four stride-3 layers, H[5] = H[6] = H[4]) and the slot widths S[0..6] (S[4] = S[5] = S[6] = H[4] + 2,
 * S[j] = 3 S[j+1] below).  Map j is channel-major [C, R S[j]], R = N p: row r = n p + w owns columns [r S[j], r S[j] +
 * H[j]), element (n, c, h, w) of the published [N, C, H[j], p] map is column (n p + w) S[j] + h of channel c, and every
 * other column (the slack) holds exactly 0.  Because S[j] = stride S[j+1] and S[j] >= H[j] + 2, Conv2d((K,1), (stride,1),
 * ((K-1)/2, 0)) over all rows is ONE Conv1d(K, stride, (K-1)/2) along the flat axis: a row's zero padding is its
 * neighbour's slack, and Lout = R S[j+1] exactly.  No GPU work; MG_ERR_SHAPE for T < 1, p < 1, a reflect pad that does
 * not fit (T <= p - 1 - (T - 1) mod p) or widths past int; MG_ERR_ARG for a null array. */
int mg_period_geometry(int T, int p, int *H, int *S);
/* The fold: in0[(n p + w) S0 + h] = y[n, reflect(h p + w)] for h < H0, else 0 (y [N, T], in0 [N p S0]), and its backward
 * dy[n, t] = din0 at t's own column plus, where a pad sample mirrors t, that sample's column, added in that order.
 * H0, S0 are those of mg_period_geometry(T, p); N p S0 past 2^30 is MG_ERR_SHAPE. */
int mg_period_fold_fwd(const float *y, float *in0, int N, int T, int p, void *stream);
int mg_period_fold_bwd(const float *din0, float *dy, int N, int T, int p, void *stream);
/* One layer on the slotted axis: in [Ci, Lin], Lin = R S_in; out [Co, Lout], Lout = R S_out, S_in = stride S_out:
 *   out[co, l] = (l mod S_out < H_out) ? act(sum_{ci,k} w[co,ci,k] in[ci, l stride + k - (K-1)/2] + bias[co]) : 0,
 * act MG_ACT_NONE or MG_ACT_LRELU with `slope`; (K, stride) in {(5,3), (5,1), (3,1)}; packed = mg_conv_pack(w,
 * MG_PACK_PLAIN).  scratch (may be NULL): the split-reduction scratch of mg_conv1d_fwd_split, for the deep layers whose
 * output is a few tiles.  Lin != R S_in, Lout != R S_out, S_in != stride S_out, H_out > S_out - 2 or H_out < 1, another
 * (K, stride), or R S_in past 2^30 are MG_ERR_SHAPE before any launch; null in / packed / out MG_ERR_ARG. */
int mg_period_conv_fwd(const float *in, const float *packed, const float *bias, float *out, int R, int Ci, int Lin,
                       int S_in, int Co, int Lout, int S_out, int H_out, int K, int stride, int act, float slope,
                       float *scratch, size_t scratch_floats, void *stream);
/* Its data gradient, d [Co, Lout] -> dx [Ci, Lin]:
 *   dx[ci, m] = (m mod S_in < H_in) ? (sum_{co,k : m + (K-1)/2 - k = stride l} w[co,ci,k] d[co,l] + add[ci,m]) * mask : 0,
 * mask = map[ci,m] > 0 ? 1 : slope from the stored activated map of the layer below (NULL: 1), add (NULL: 0) a gradient
 * that reaches that map from outside; positions no output reads get exactly add * mask, the slack exactly 0.
 * Stride 1: packed = mg_conv_pack(w, MG_PACK_DGRAD).  Stride 3: packed = mg_period_dgrad3_pack(w), a polyphase two-tap
 * GEMM with 3 Ci rows over d -- with m = 3 q + f: f = 0 reads w[.,.,2] d[q]; f = 1 w[.,.,0] d[q+1] + w[.,.,3] d[q];
 * f = 2 w[.,.,1] d[q+1] + w[.,.,4] d[q] -- 6/5 of the forward's flops, no zero insertion; GEMM row ci 3 + f, column q
 * is written to dx[ci, 3 q + f].  Checks as mg_period_conv_fwd, with H_in against S_in. */
size_t mg_period_dgrad3_packed_floats(int Co, int Ci);
int mg_period_dgrad3_pack(const float *w, float *packed, int Co, int Ci, void *stream);
int mg_period_conv_dgrad(const float *d, const float *packed, const float *map, const float *add, float *dx, int R,
                         int Ci, int Lin, int S_in, int H_in, int Co, int Lout, int S_out, int K, int stride,
                         float slope, float *scratch, size_t scratch_floats, void *stream);

/* ------------------------------------------------------------------ measurement hooks (bench.py)
 * While a session is open, mg_denoiser_fwd brackets each launch of its dominant kernel (the k=3
 * gated convolution of a residual layer) with HIP events recorded on the launch stream.
 * mg_profile_end waits for them and returns the number of brackets written to ms_out. */
int mg_profile_begin(int max_brackets);
/* As above, bracketing only every `every`-th launch (keeps the events' own cost out of the timing). */
int mg_profile_begin_sampled(int max_brackets, int every);
int mg_profile_end(float *ms_out, int max_out);

#ifdef __cplusplus
}
#endif
#endif /* MIXGAN_HIP_H */
