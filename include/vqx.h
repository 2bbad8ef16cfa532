/*
 * vqx.h — C ABI of libvqx.so, the MI355X (gfx950) kernels behind the
 * vae_npvc VQ-VAE training step.
 *
 * The reference (Sinica-SLAM/vae_npvc) has no native layer: every op on its
 * hot path is a stock PyTorch call.  Each entry point below replaces one of
 * those calls (or a fused group of them); the reference site is cited per
 * function.  Paths are relative to the reference repository root.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch's caching
 *     allocator in the Python host layer); nothing here allocates or frees;
 *   - calls are stream-ordered on `stream` (a hipStream_t, NULL = legacy
 *     stream) and never synchronise the host, so they can be captured into a
 *     hipGraph;
 *   - activations are "frame-major": row n = b*T + t, channels contiguous
 *     (the reference's (B, C, T) tensors transposed to (B*T, C));
 *   - return 0 on success, <0 on an invalid argument (-1) or a HIP launch
 *     error (-2); vqx_last_error() then holds thread-local text.
 */
#ifndef VQX_H
#define VQX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vqx_stream_t; /* hipStream_t */

/* element types of activation / weight operands */
enum { VQX_F32 = 0, VQX_BF16 = 1 };

/* operand prologues, applied elementwise while a tile is staged into LDS */
enum {
  VQX_PRO_NONE = 0,
  VQX_PRO_LRELU = 1,      /* LeakyReLU(0.2)   layers.py:152, vqvae.py:171   */
  VQX_PRO_RELU = 2,       /* ReLU             vqvae.py:283,285              */
  VQX_PRO_SCALE_RELU = 3  /* ReLU(pro_scale*x) vqvae.py:316-317            */
};

/* epilogue flags of vqx_conv1d_fwd / vqx_conv1d_dgrad, applied in this order */
enum {
  VQX_EPI_BIAS = 1 << 0,    /* v += bias[c]                                    */
  VQX_EPI_ROWBIAS = 1 << 1, /* v += rowbias[(n/T)*cout + c]  (conv_cond term); with
                               rowbias_T = Tc > 1 (forward only, ABI 130) the term
                               varies in time: rowbias is [B*Tc][cout] and frame
                               t = n - b*T of utterance b = n/T reads row
                               b*Tc + min(t / (T/Tc), Tc - 1)                   */
  VQX_EPI_MASK = 1 << 2,    /* v *= (mask[n][c] > 0 ? 1 : mask_slope)*mask_scale */
  VQX_EPI_RES = 1 << 3,     /* v += res[n][c]                                  */
  VQX_EPI_GNADD = 1 << 4,   /* v += (gn_h[n][c]-mean[b])*rstd[b]*gamma[c]+beta[c] */
  VQX_EPI_SPLIT = 1 << 5,   /* cols >= split_col -> out2[n][c-split_col] (f32,
                               '+=' when out2_accumulate)                      */
  VQX_EPI_OUTF32 = 1 << 6,  /* y stored as f32 instead of `dtype`              */
  VQX_EPI_ACT = 1 << 7,     /* y = act(v), act = epi_act (VQX_PRO_LRELU/RELU)  */
  VQX_EPI_ACT2 = 1 << 8,    /* also y2[n][c] = act(v) (dtype): the producer writes
                               the pre-activated copy its consumers read, so no
                               GEMM applies an activation while staging        */
  VQX_EPI_COLSUM = 1 << 9,  /* colsum_part[tile][c] = sum over the 128-frame row
                               tile of the stored fp32 value (before rounding):
                               the bias gradient of the layer y feeds, reduced
                               later by a VQX_WN_COLREDUCE table entry          */
  VQX_EPI_GNSTATS = 1 << 10, /* y is a GroupNorm input: stat_part[g128][tn][4] =
                               (count, mean, M2, 0) of the stored fp32 values of
                               each 128-frame x 128-channel tile; combined by
                               vqx_gn_finalize_tiles.  Needs T % 128 == 0 and
                               cout/gn_groups % 128 == 0                        */
  VQX_EPI_GNBWD = 1 << 11   /* y is the gradient dy of a GroupNorm output (GLU-
                               gated when gn_glu): stat_part[g128][tn][4] = per
                               tile (sum g*dh, sum g*dh*xhat) for group a (and b)
                               with u = gn_h [N][ldgn], the forward mean/rstd,
                               gamma, beta; consumed by vqx_gn_bwd(nparts > 0)  */
};
#define VQX_CONV_TILE_ROWS 128   /* frames per GEMM row tile (COLSUM partial rows) */

/*
 * Stride-1 Conv1d / ConvTranspose1d as an implicit-im2col GEMM on MFMA.
 *   fwd  : y[n][co] = epi( sum_{j,ci} w[co][j*cin+ci] * pro(x[n+j*dil-pad][ci]) )
 *          rows n+j*dil-pad outside the utterance of n read as zero (padding).
 *   dgrad: the same args with x = dy [N][cin], w = the FORWARD layer's packed
 *          weight [cout][ntaps*cin_fwd]; computes
 *          dx[n][ci] = epi( sum_{j,c} w[c][(ntaps-1-j)*cout_total.. ] ... )
 *          i.e. the transposed, tap-flipped conv; here `cin` = channels of dy
 *          (the forward layer's cout) and `cout` = the forward layer's cin.
 * Reference: nn.Conv1d / nn.ConvTranspose1d forward and autograd backward,
 * vqvae.py:156,174,257-265,286; layers.py:157,164,196,208,213.
 */
typedef struct vqx_conv_args {
  const void* x;             /* [N][ldx]                                       */
  const void* w;             /* packed weight [cout_fwd][ntaps*cin_fwd]        */
  void* y;                   /* [N][ldy]                                       */
  const float* bias;         /* [cout]                                         */
  const float* rowbias;      /* [B][cout], or [B*rowbias_T][cout]              */
  const void* res;           /* [N][ldres]  dtype                              */
  const void* mask;          /* [N][ldmask] dtype                              */
  const void* gn_h;          /* [N][ldgn]   dtype                              */
  const float* gn_mean_rstd; /* [B][2]                                         */
  const float* gn_gamma;     /* [cout]                                         */
  const float* gn_beta;      /* [cout]                                         */
  float* out2;               /* [N][ldo2] f32                                  */
  int64_t n_rows;            /* N = B*T                                        */
  int32_t T;                 /* frames per utterance                           */
  int32_t cin, cout, ntaps, pad;
  int32_t ldx, ldy, ldres, ldmask, ldgn, ldo2;
  int32_t dtype;             /* VQX_F32 | VQX_BF16                             */
  int32_t prologue;          /* VQX_PRO_*  (applied to x)                      */
  int32_t epilogue;          /* VQX_EPI_* flags                                */
  int32_t split_col, out2_accumulate;
  float pro_scale, mask_slope, mask_scale;
  void* y2;                  /* ACT2 destination [N][ldy2]                     */
  int32_t ldy2, epi_act;
  float* colsum_part;        /* COLSUM destination [ceil(N/128)][cout]         */
  float* stat_part;          /* GNSTATS / GNBWD destination [N/128][ceil(cout/128)][4] */
  int32_t gn_groups, gn_glu;
  /* GNADD with gn_stat_tiles != NULL: the GroupNorm statistics (G = 1) are
   * merged from the producing GEMM's GNSTATS tiles inside this launch (as
   * vqx_gn_finalize_tiles computes them, eps gn_eps) and written to
   * gn_mean_rstd [B][2]; needs T % 128 == 0 and cout % 128 == 0. */
  const float* gn_stat_tiles;
  float gn_eps;
  int32_t dil;               /* tap spacing (dilation, vqvae.py:166,274); 0 or 1 = dense.
                                Taps sit at n + j*dil - pad; 1 <= ntaps <= 8 and
                                0 <= pad <= (ntaps-1)*dil.  DGRAD takes the forward
                                layer's ntaps/dil and pad' = (ntaps-1)*dil - pad    */
  int32_t kernel_policy;     /* VQX_POLICY_* (ABI 122): which bf16 GEMM kernels this call may
                                use; 0 = automatic.  Per call, no process-wide state.         */
  int32_t rowbias_T;         /* ABI 130: rows of rowbias per utterance (Tc); 0 or 1 = one row per
                                utterance.  Tc > 1: forward only, Tc <= T, T * (T / Tc) < 2^32
                                (dgrad and dgrad_wgrad return -1); the conv_cond term of a
                                conditioning stretched from Tc to T frames (vqvae2.py:105-114),
                                see VQX_EPI_ROWBIAS                                            */
} vqx_conv_args;

/* Kernel policy of a conv GEMM call (vqx_conv_args / vqx_wgrad_args
 * .kernel_policy; the data-gradient args decide for vqx_conv1d_dgrad_wgrad):
 * AUTO picks by shape (3-tap, pad-1 bf16 layers with T % 128 == 0 run the
 * tap-reuse kernels, the 512-frame tall kernel where it fills the GPU, 1x1
 * layers the implicit-im2col kernel, layer pairs the fused DGRAD + WGRAD
 * launches); IM2COL keeps every GEMM on the implicit-im2col kernel and turns
 * the fused launches off; TALL256 / TALL512 force the tall tap-reuse kernel's
 * 256 / 512-frame tiles where they apply; TR128 keeps 3-tap layers on the
 * 128-frame tap-reuse kernel.  All produce the same values (tests compare
 * them); the choice is speed only. */
#define VQX_POLICY_AUTO 0
#define VQX_POLICY_IM2COL 1
#define VQX_POLICY_TALL256 2
#define VQX_POLICY_TALL512 3
#define VQX_POLICY_TR128 4
#define VQX_POLICY_K1_2PCU 5  /* ABI 125: as AUTO, but the bf16 1x1 FWD and DGRAD+WGRAD on the
                                 two-workgroups-per-CU kernels (AUTO: three per CU, one round
                                 with spare slots, since round 5) */

int vqx_conv1d_fwd(const vqx_conv_args* a, vqx_stream_t stream);
int vqx_conv1d_dgrad(const vqx_conv_args* a, vqx_stream_t stream);

/*
 * Weight gradient of a stride-1 conv as split-K partial slabs:
 *   slabs[s][r][j*c_dim + c] = sum_{n in split s} p[n][r] * pro(q[n + sign*(j*dil-pad)][c])
 * Conv1d  (dW[co][ci][j]): p = dy, q = x,  sign = +1.
 * ConvT1d (dW[ci][co][k-1-j]): p = x, q = du, sign = -1.
 * vqx_weight_norm_bwd reduces the slabs.  Reference: autograd of the convs
 * above (convolution_backward, 49% of the reference CPU step).
 */
typedef struct vqx_wgrad_args {
  const void* p;
  const void* q;
  void* slabs;       /* [splits][r_dim][ntaps*c_dim] of slab_dtype */
  int64_t n_rows;
  int32_t T, r_dim, c_dim, ntaps, pad, shift_sign, ldp, ldq;
  int32_t dtype, q_prologue, splits;
  float pro_scale;
  int32_t dil;       /* taps at n + sign*(j*dil - pad); 0 or 1 = dense */
  int32_t slab_dtype; /* VQX_F32, or VQX_BF16 (bf16 operands only): each split's fp32 partial
                         rounded once to bf16, half the slab bytes written here and read by
                         vqx_weight_norm_bwd, which sums them in fp32 */
  int32_t kernel_policy; /* VQX_POLICY_* (ABI 122); IM2COL: no tap-reuse weight-gradient kernel */
  /* In-launch ordered split-K reduction (ABI 127, optional: NULL = off).  With
   * fixup_dw set, the split that finishes an output tile last (one agent-scope
   * counter per tile) sums every split's slab of that tile in split order
   * 0, 1, ... in fp32 -- the order vqx_weight_norm_bwd sums slabs -- and
   * stores the fp32 weight gradient fixup_dw [r_dim][ntaps*c_dim]; a
   * weight-norm backward table entry then reads it as one fp32 "slab"
   * (splits 1), bit for bit the gradient it would have formed from the
   * slabs.  The slabs are still written (write-through, for the last split to
   * read).  fixup_counters: vqx_wgrad_tiles(...) uint32 counters, zero before
   * the first call and left zero by every call.  Needs the 3-tap tap-reuse
   * weight-gradient kernel and bf16 slabs (vqx_wgrad_fixup_ok). */
  float* fixup_dw;
  uint32_t* fixup_counters;
} vqx_wgrad_args;

int vqx_conv1d_wgrad(const vqx_wgrad_args* a, vqx_stream_t stream);
/* *ok = 1 when a weight gradient of this shape takes the in-launch split-K
 * reduction (fixup_dw), else 0 (ABI 127). */
int vqx_wgrad_fixup_ok(int64_t n_rows, int32_t T, int32_t r_dim, int32_t c_dim, int32_t ntaps, int32_t pad, int32_t dil,
                       int32_t dtype, int32_t slab_dtype, int32_t q_prologue, int32_t policy, int32_t* ok);

/*
 * One layer's data gradient (d, as vqx_conv1d_dgrad) and weight gradient (w,
 * as vqx_conv1d_wgrad) from the same output gradient, in one launch whose
 * workgroups interleave the two GEMMs (each CU runs one of each, so the data
 * gradient's fused epilogue overlaps the weight gradient's main loop) where a
 * fused instance covers the pair: bf16, no prologue, the 3-tap tap-reuse
 * kernels, and 1x1 layers (their data gradient's workgroups first, then the
 * weight gradient's in the slots they free).  Otherwise the two are launched in sequence
 * (weight gradient first).  *fused (may be NULL) = 1 for one launch, 0 for
 * two.  Results equal the separate calls bit for bit.  Replaces the two
 * autograd calls of one conv in the reference backward.
 */
int vqx_conv1d_dgrad_wgrad(const vqx_conv_args* d, const vqx_wgrad_args* w, int32_t* fused, vqx_stream_t stream);

/*
 * Weight norm (torch.nn.utils.weight_norm, dim=0; applied at vqvae.py:203-208,
 * 329-334): w = g * v / ||v|| per row o of v[rows][cols] (Conv1d rows = cout,
 * ConvT rows = cin).  The forward packs w into the effective-conv layout the
 * GEMMs read: w_packed[co][j*cin + ci] in `dtype`.
 * kind 0: Conv1d v[cout][cin][k]; kind 1: ConvTranspose1d v[cin][cout][k]
 * (effective tap j' = k-1-j).  Descriptors are batched: one launch packs
 * every layer of the model.
 */
#define VQX_WN_COLREDUCE 2  /* table entry kind: dv[c] = sum_{r < cin} v[r*cout + c] (bias /
                               GroupNorm-affine gradients from per-tile or per-utterance
                               partials, reduced in the same backward launch)        */
/* Resampling convs of the multi-resolution models (vqvae.py:144-156 /
 * 243-263, vqvae2.py:197-226 / 297-319): kernel k = 2s, stride s, padding
 * p = s/2 + s%2 (ConvT output_padding s%2).  With frames folded s at a time
 * (x'[u] = x[s*u .. s*u+s-1], a reinterpretation of the frame-major [N][C]
 * layout as [N/s][s*C]) the strided conv is a stride-1, 3-tap, pad-1 conv:
 *   w_packed[r][m][q*C + c] = w[r][c][s*(m-1) + q + p]  (0 when outside [0,k))
 * for rows r (kind 3: cout of v[cout][cin][k], C = cin; kind 4: cin of the
 * ConvT's v[cin][cout][k], C = cout), m in 0..2, q in 0..s-1.  The strided
 * Conv1d runs as vqx_conv1d_fwd on the folded input; the ConvTranspose1d
 * (its adjoint) as vqx_conv1d_dgrad; both gradients follow the same way and
 * the backward folds the 3-tap wgrad slabs [splits][r][3*s*C] back to v. */
#define VQX_WN_RESAMPLE 3    /* strided Conv1d, v[cout][cin][k]          */
#define VQX_WN_RESAMPLE_T 4  /* strided ConvTranspose1d, v[cin][cout][k] */
typedef struct vqx_wn_layer {
  const float* v;       /* [rows][cols] */
  const float* g;       /* [rows]       */
  void* w_packed;       /* [cout][k*cin] dtype */
  float* norm;          /* [rows] ||v_o|| saved for the backward */
  float* dv;            /* bwd: [rows][cols] */
  float* dg;            /* bwd: [rows] */
  const void* slabs;    /* bwd: wgrad slabs (slab_dtype) */
  int32_t kind, cout, cin, k, splits, dtype;
  int32_t stride, pad;  /* kinds VQX_WN_RESAMPLE(_T) only */
  int32_t slab_dtype;   /* VQX_F32 | VQX_BF16 (vqx_wgrad_args.slab_dtype) */
} vqx_wn_layer;

/* `layers_host` sizes the launch; the kernels read the same table from the
 * device copy `layers_dev` (built once by the caller, so a captured graph
 * replays without host work). */
int vqx_weight_norm_fwd(const vqx_wn_layer* layers_host, const vqx_wn_layer* layers_dev,
                        int32_t n_layers, vqx_stream_t stream);
/* The same with flags (ABI 125): VQX_WNF_NORMS_READY skips the ConvTranspose
 * row norms (kind 1): vqx_adam_step_wn has written them for the current v. */
#define VQX_WNF_NORMS_READY 1
int vqx_weight_norm_fwd_flags(const vqx_wn_layer* layers_host, const vqx_wn_layer* layers_dev,
                              int32_t n_layers, int32_t flags, vqx_stream_t stream);
int vqx_weight_norm_bwd(const vqx_wn_layer* layers_host, const vqx_wn_layer* layers_dev,
                        int32_t n_layers, vqx_stream_t stream);
/* The same launch, also leaving the sum of squares of every gradient value it
 * writes (dv, dg, column reductions) as per-wave partials in
 * sq_partials[0 .. count) (ABI 125; count from vqx_weight_norm_bwd_partials):
 * the global gradient norm of clip_grad_norm_ (trainer/basic.py:63-67)
 * without re-reading the 125 MB gradient.  vqx_sq_norm_finish then sums the
 * partials and g^2 over the flat ranges [off, off+len) the weight-norm
 * backward does not write (ranges: int64 pairs, device memory), each in a
 * fixed order, into out[0] -- what vqx_grad_sq_norm computes, summed in
 * another order. */
int vqx_weight_norm_bwd_partials(const vqx_wn_layer* layers_host, int32_t n_layers, int64_t* count);
int vqx_weight_norm_bwd_sq(const vqx_wn_layer* layers_host, const vqx_wn_layer* layers_dev,
                           int32_t n_layers, float* sq_partials, int64_t sq_capacity, vqx_stream_t stream);
int vqx_sq_norm_finish(const float* partials, int64_t n_partials, const float* g, const int64_t* ranges,
                       int32_t n_ranges, float* scratch /* >= 256 floats */, float* out, vqx_stream_t stream);
/* vqx_sq_norm_finish followed by vqx_adam_hyper (same arguments, same
 * results) with the second folded into the finish's last launch (ABI 126). */
int vqx_sq_norm_finish_adam(const float* partials, int64_t n_partials, const float* g, const int64_t* ranges,
                            int32_t n_ranges, float* scratch, float* out, int64_t* step, double lr0, double gamma,
                            int32_t step_size, double beta1, double beta2, double eps, float* hyper,
                            vqx_stream_t stream);

/*
 * GroupNorm statistics (nn.GroupNorm, layers.py:154 (G=1), layers.py:201
 * (G=2); eps 1e-5): mean and 1/sqrt(var+eps) over (C/G, T) per utterance.
 * x [N][ldx] dtype, C channels; out mean_rstd[B][G][2] f32.  Two-pass
 * (mean, then centred sum of squares) per (b, g).
 */
int vqx_groupnorm_stats(const void* x, int32_t ldx, int32_t dtype, int64_t n_rows, int32_t T,
                        int32_t C, int32_t G, float eps, float* partials /* >= B*G*24 */,
                        float* mean_rstd, vqx_stream_t stream);

/*
 * Fused GroupNorm(G=2) + gated tanh/sigmoid unit, decoder ResSkip block
 * (layers.py:236-242):  g[n][c] = tanh(h(n,c)) * sigmoid(h(n,c+C/2)),
 * h = (u - mean)*rstd*gamma + beta.  u [N][ldu], g [N][ldg], C = 2*half.
 */
int vqx_gn_glu_fwd(const void* u, int32_t ldu, void* g, int32_t ldg, int32_t dtype, int64_t n_rows,
                   int32_t T, int32_t C, const float* mean_rstd, const float* gamma, const float* beta,
                   vqx_stream_t stream);

/* vqx_gn_glu_fwd with the GroupNorm statistics merged from the producing
 * GEMM's GNSTATS tiles (G = 2, as vqx_gn_finalize_tiles computes them) inside
 * the same launch; mean_rstd [B][2][2] is written for the backward.
 * Needs T % 128 == 0 and C % 256 == 0. */
int vqx_gn_glu_fwd_tiles(const void* u, int32_t ldu, void* g, int32_t ldg, int32_t dtype, int64_t n_rows,
                         int32_t T, int32_t C, const float* parts, float eps, float* mean_rstd,
                         const float* gamma, const float* beta, vqx_stream_t stream);

/* GroupNorm(G=1) + LeakyReLU(0.2): g = lrelu((h - mean)*rstd*gamma + beta),
 * the operand of each further conv of a residual stack with stack_layers > 1
 * (layers.py:156-161).  h, g [N][ld*] dtype; mean_rstd [B][2] from
 * vqx_groupnorm_stats / vqx_gn_finalize_tiles.  The backward needs no kernel
 * of its own: the next conv's DGRAD applies the LeakyReLU derivative with
 * VQX_EPI_MASK (mask = g, slope 0.2) and vqx_gn_bwd(glu = 0) the GroupNorm. */
int vqx_gn_lrelu_fwd(const void* h, int32_t ldh, void* g, int32_t ldg, int32_t dtype, int64_t n_rows, int32_t T,
                     int32_t C, const float* mean_rstd, const float* gamma, const float* beta, vqx_stream_t stream);

/*
 * Backward of GroupNorm(G) optionally preceded by the gated unit:
 *   glu=1: dy is dL/dg [N][C/2], u is the GN input [N][C]: computes dL/dh
 *          through tanh*sigmoid, then through GroupNorm, into du [N][C].
 *   glu=0: dy is dL/d(GN output) [N][C].
 * Also accumulates per-utterance column sums of du (for the conv bias and
 * conv_cond gradients) into colsum[B][C] and dgamma/dbeta partials
 * [B][C] (summed over B by the caller's reduction).
 * Reference: autograd of layers.py:236-242 and 170-176.
 */
int vqx_gn_bwd(const void* dy, int32_t lddy, const void* u, int32_t ldu, void* du, int32_t lddu,
               int32_t dtype, int64_t n_rows, int32_t T, int32_t C, int32_t G, int32_t glu,
               const float* mean_rstd, const float* gamma, const float* beta,
               float* partials /* nparts == 0: workspace >= B*64*G */,
               int32_t nparts /* 0: reduce here; > 0: partials hold the producing GEMM's
                                 VQX_EPI_GNBWD tiles, nparts per utterance */,
               float* colsum_b /* [B][C] */, float* dgamma_b /* [B][C] */, float* dbeta_b /* [B][C] */,
               vqx_stream_t stream);

/* GroupNorm statistics from a GEMM's VQX_EPI_GNSTATS tiles (see there):
 * mean_rstd[B][G][2], combined per (utterance, group) in double. */
int vqx_gn_finalize_tiles(const float* parts, int64_t n_rows, int32_t T, int32_t C, int32_t G, float eps,
                          float* mean_rstd, vqx_stream_t stream);

/*
 * Sum over rows: out[c] (+)= sum_n x[n][c] (f32 accumulation, deterministic
 * two-level tree).  Used for conv bias gradients and for reducing [B][C]
 * partials.  accumulate=1 adds into out.
 */
int vqx_colsum(const void* x, int32_t ldx, int32_t dtype, int64_t n_rows, int32_t C,
               float* partials /* >= 64*C */, float* out, int32_t accumulate, vqx_stream_t stream);

/*
 * The first level of vqx_colsum alone (ABI 126): partials[p][c] = the sum of
 * row part p of column c, p < vqx_colsum_parts(n_rows, C, dtype) <= 64.  The
 * caller reduces them later, e.g. as a VQX_WN_COLREDUCE entry of the batched
 * weight-norm backward (a conv bias gradient without a launch of its own).
 */
int vqx_colsum_parts(int64_t n_rows, int32_t C, int32_t dtype, int32_t* nparts);
int vqx_colsum_partials(const void* x, int32_t ldx, int32_t dtype, int64_t n_rows, int32_t C,
                        float* partials /* >= nparts * C */, vqx_stream_t stream);

/*
 * Frame-major copy of the (B, C, T) input batch, with dtype conversion
 * (the reference's z.transpose(1,2).contiguous(), layers_vq.py:274-276).
 */
int vqx_nct_to_ntc(const float* x_nct, int32_t B, int32_t C, int32_t T, void* y, int32_t ldy,
                   int32_t dtype, vqx_stream_t stream);
int vqx_ntc_to_nct(const void* y, int32_t ldy, int32_t dtype, int32_t B, int32_t C, int32_t T,
                   float* x_nct, vqx_stream_t stream);

/*
 * log_loss (layers.py:283-296, reduction 'frame_mean') fused with its
 * gradient: loss = sum 0.5*(log2pi + (x - xhat)^2) / (B*T);
 * dxhat = (xhat - x) * grad_scale (grad_scale = dL/dloss / (B*T)).
 * x is the reference (B, C, T) f32 batch; xhat is frame-major f32.
 * loss_out[0] receives the loss (deterministic reduction).
 */
int vqx_logloss_fwd_bwd(const float* x_nct, const float* xhat, int32_t ldxh, int32_t B, int32_t C,
                        int32_t T, float grad_scale, void* dxhat, int32_t lddx, int32_t dtype,
                        float* loss_out, float* partials, vqx_stream_t stream);
/* The same, and in its final sum launch also extra_out[0] = the sum of
 * extra_partials[0 .. n_extra) in the order vqx_vq_forward sums its
 * commitment partials (ABI 126: the VQ kernel then runs with sqerr_out NULL,
 * one launch fewer). */
int vqx_logloss_fwd_bwd_x(const float* x, const float* xhat, int32_t ldxh, int32_t B, int32_t C, int32_t T,
                          float grad_scale, void* dxhat, int32_t lddx, int32_t dtype, float* loss_out,
                          float* partials, const float* extra_partials, int32_t n_extra, float* extra_out,
                          vqx_stream_t stream);
/* The same without the final sum launch (ABI 128): the per-workgroup
 * partials only, their count in *n_parts (at most 1024); the total is
 * (1/(B*T)) * their sum in the order vqx_logloss_fwd_bwd adds them
 * (vqx_vq_ema_update_close sums them so). */
int vqx_logloss_parts(const float* x, const float* xhat, int32_t ldxh, int32_t B, int32_t C, int32_t T,
                      float grad_scale, void* dxhat, int32_t lddx, int32_t dtype, float* partials, int32_t* n_parts,
                      vqx_stream_t stream);

/*
 * EMA vector-quantizer forward (EMAVectorQuantizer.forward,
 * layers_vq.py:268-323, distances :285-289, argmin :291, gather :292,
 * commitment loss :301,308-309; update_emb statistics :207-211):
 *   dist[n][k] = (||z_n||^2 + ||e_k||^2) - 2 z_n.e_k   (fp32 MFMA)
 *   idx[n]     = first argmin_k dist[n][k]               (int64)
 *   zq[n]      = E[idx[n]]  (f32 [N][D]) and zq_c (dtype, decoder input)
 *   sqerr      : sum_n ||zq_n - z_n||^2  into sqerr_out[0] (deterministic)
 *   bsum[k][d] += sum_{n: idx=k} z[n][d], bcnt[k] += |{n: idx=k}|
 *                 (deterministic: 512-frame chunks sorted by code, segmented
 *                 sums, chunk tables reduced in order; pass NULL to skip, e.g.
 *                 eval / encode())
 * z [N][D] f32 (frame-major, D = z_dim in {64, 128, 256}), E [K][D] f32,
 * K % 16 == 0, K <= 2048.  `partials` is a caller workspace of
 * >= vqx_vq_workspace(N, K, D, bsum != NULL) floats.
 */
int vqx_vq_forward(const float* z, int64_t n_rows, int32_t D, const float* E, int32_t K,
                   int64_t* idx, float* zq, void* zq_c, int32_t zq_c_dtype, float* sqerr_out,
                   float* partials, float* bsum, float* bcnt, vqx_stream_t stream);
/* Workspace (floats) vqx_vq_forward needs for N frames and K codes of width
 * D, with or without the EMA statistics (ABI 123: D added). */
int vqx_vq_workspace(int64_t n_rows, int32_t K, int32_t D, int32_t with_stats, int64_t* floats);
/* The EMA statistics part of vqx_vq_forward on its own (bsum = one-hot^T z,
 * bcnt = counts of idx; update_emb's onehot matmul, layers_vq.py:207-211),
 * for callers that run it on another stream than the distance kernel.
 * `partials` is the same workspace (with stats); it does not touch the
 * commitment partials, so it may run beside vqx_vq_forward's sqerr sum. */
int vqx_vq_stats(const float* z, int64_t n_rows, int32_t D, const int64_t* idx, int32_t K, float* partials,
                 float* bsum, float* bcnt, vqx_stream_t stream);

/*
 * EMA codebook update (update_emb, layers_vq.py:203-233; init_emb :192-201):
 *   emb_sum  = mu*emb_sum  + (1-mu)*bsum;  emb_elem = mu*emb_elem + (1-mu)*bcnt
 *   usage    = emb_elem >= threshold
 *   E        = usage ? emb_sum/emb_elem : rand_rows
 *   diag[0..3] = {entropy (perplexity of bcnt), used_curr, usage, diff_emb}
 * rand_rows [K][D] are the rows z[perm[:K]] gathered by vqx_gather_rows.
 * partials: workspace of ceil(K*D/1024) + 1 words, the last a counter that
 * must be zero before the first call (each call leaves it zero; ABI 128: one
 * launch, its last workgroup runs the per-code pass).  Deterministic (fixed
 * summation order).
 */
int vqx_vq_ema_update(float* emb_sum, float* emb_elem, float* E, const float* bsum,
                      const float* bcnt, const float* rand_rows, int32_t K, int32_t D, float mu,
                      float threshold, float* diag, float* partials, vqx_stream_t stream);
/* The same, and bsum / bcnt are zero afterwards (ABI 126): the next step's
 * vqx_vq_forward accumulates into them without a zero-fill launch. */
int vqx_vq_ema_update_clear(float* emb_sum, float* emb_elem, float* E, float* bsum, float* bcnt,
                            const float* rand_rows, int32_t K, int32_t D, float mu, float threshold, float* diag,
                            float* partials, vqx_stream_t stream);
/* vqx_vq_ema_update_clear that also closes the training step's forward in
 * its last workgroup (ABI 128), the work of two one-workgroup launches:
 *   out[i][0] = scale[i] * (parts[i][0] + ... + parts[i][n[i]-1]), i < 2
 *     (parts[i] NULL: none), summed in the order of vqx_logloss_fwd_bwd_x's
 *     final launch (the log-loss total from vqx_logloss_parts' partials with
 *     scale 1/(B*T); the commitment sum from vqx_vq_forward's partials);
 *   then, with pub_box != NULL, pub_src[0 .. pub_n) published into mailbox
 *     slot pub_slot with number pub_seq as vqx_mailbox_publish does, after
 *     the sums and diag are stored (pub_src may hold them);
 *   with rows_src != NULL, the dead-code rows read straight from it: row k of
 *     rand_rows is rows_src[rows_host[k] * rows_ld ..] (a zero row for a
 *     negative index; rows_host: n_rows == K <= 512 host int32 indices, copied
 *     into the launch's arguments; rand_rows is then not read and may be
 *     NULL): vqx_gather_rows_host folded in.
 * The values equal those of the separate launches bit for bit. */
typedef struct {
  const float* parts[2];
  int32_t n[2];
  float scale[2];
  float* out[2];
  const float* pub_src;
  int32_t pub_n;
  float* pub_copy;     /* device copy of the published values, or NULL */
  void* pub_box;       /* vqx_mailbox_create's device pointer, or NULL */
  int32_t pub_slot, pub_slots, pub_floats;
  uint32_t pub_seq;
  const float* rows_src;   /* z, or NULL: rand_rows as given */
  int32_t rows_ld, n_rows;
  const int32_t* rows_host;
} vqx_step_close;
int vqx_vq_ema_update_close(float* emb_sum, float* emb_elem, float* E, float* bsum, float* bcnt,
                            const float* rand_rows, int32_t K, int32_t D, float mu, float threshold, float* diag,
                            float* partials, const vqx_step_close* close, vqx_stream_t stream);

/* out[i][:] = src[rows[i]][:] for i < n_out  (f32, row length D).  rows are
 * int64 indices; negative indices write zero rows (rows owned by another
 * rank in data-parallel training). */
int vqx_gather_rows(const float* src, int32_t ld_src, const int64_t* rows, int32_t n_out,
                    int32_t D, float* out, vqx_stream_t stream);

/* The same gather with the row indices in HOST memory (int32, read during
 * the call and passed to the kernels by value, 512 rows a launch): no
 * host-to-device copy on the stream.  Replaces the reference's
 * `_z[torch.randperm(N)][:K]` indexing with a CPU permutation
 * (layers_vq.py:197,213), whose index tensor torch copies to the device. */
int vqx_gather_rows_host(const float* src, int32_t ld_src, const int32_t* rows, int32_t n_out,
                         int32_t D, float* out, vqx_stream_t stream);

/* Commitment-loss gradient (layers_vq.py:301 backward):
 *   dz[n][d] = scale * (z[n][d] - zq[n][d])  written in dtype. */
int vqx_vq_commit_bwd(const float* z, const float* zq, int64_t count, float scale, void* dz,
                      int32_t dtype, vqx_stream_t stream);
/* The same over [n_rows][D] rows, plus the column sums of the dz it stores
 * (ABI 126): partials[p][d] = sum of dz[n][d] over the rows n of part p (rows
 * n_rows*p/P .. n_rows*(p+1)/P, P = VQX_COMMIT_PARTS; empty parts write 0),
 * the first level of the bias gradient of the conv producing z.  D % 4 == 0,
 * D <= 1024. */
#define VQX_COMMIT_PARTS 256
int vqx_vq_commit_bwd_cs(const float* z, const float* zq, int64_t n_rows, int32_t D, float scale, void* dz,
                         int32_t dtype, float* partials /* [VQX_COMMIT_PARTS][D] */, vqx_stream_t stream);

/* Jitter (layers_vq.py:353-379): y[b][t][:] = x[b][src_t[t]][:]. */
int vqx_time_gather(const void* x, void* y, int32_t B, int32_t T, int32_t C, const int32_t* src_t,
                    int32_t dtype, vqx_stream_t stream);

/* One training batch cut from a device-resident corpus (additive, ABI 130
 * unchanged): what dataset/utt2mel_spk.py's items and torch's default
 * collation give, without the per-item file reads and the batch copy.
 * corpus is device f32 [n_rows][mel], frame-major, the utterances back to
 * back; spk_table is device int64 [n_utts].  For item b < B:
 *   x[b][c][t] = corpus[row0[b] + t][c]   for t <  len[b]
 *   x[b][c][t] = 0                        for len[b] <= t < T
 *   y[b]       = spk_table[utt[b]]
 * x is f32 (B, mel, T) contiguous and y int64 [B]; every element of both is
 * written (no zero-fill by the caller).  row0 (int64), len and utt (int32)
 * are HOST arrays of B entries, read during the call and passed to the
 * kernel by value, 192 items a launch (as vqx_gather_rows_host passes its
 * rows): no host-to-device copy on the stream, no allocation, no
 * synchronisation.  Every item is validated before the first launch --
 * 0 <= len[b] <= T, row0[b] >= 0, row0[b] + len[b] <= n_rows,
 * 0 <= utt[b] < n_utts, and B, T, mel >= 1 (T, mel <= 2^20) -- and a failure
 * names the item in vqx_last_error() and launches nothing, so the kernel
 * reads no row outside the corpus. */
int vqx_crop_batch(const float* corpus, int64_t n_rows, int32_t mel, const int64_t* spk_table, int32_t n_utts,
                   const int64_t* row0, const int32_t* len, const int32_t* utt, int32_t B, int32_t T, float* x,
                   int64_t* y, vqx_stream_t stream);

/* Speaker embedding lookup (layers.py:42-54, nn.Embedding) and its
 * backward scatter-add (dense weight gradient). */
int vqx_embedding_fwd(const float* weight, const int64_t* ids, int32_t B, int32_t D, float* out,
                      vqx_stream_t stream);
int vqx_embedding_bwd(const float* dout, const int64_t* ids, int32_t B, int32_t D, float* dweight,
                      vqx_stream_t stream);
/* The dense weight gradient in one pass (ABI 126): every row r < n_rows of
 * dweight is written, dweight[r] (+)= sum over b with ids[b] == r of dout[b]
 * in batch order (0 for ids absent from the batch; accumulate = 1 adds).  No
 * zero-fill launch before it.  Any B (round 6): ids are staged 1024 at a
 * time, each chunk's sum added to the row in chunk order. */
int vqx_embedding_bwd_rows(const float* dout, const int64_t* ids, int32_t B, int32_t D, int32_t n_rows,
                           float* dweight, int32_t accumulate, vqx_stream_t stream);

/* Small dense GEMM for the time-constant conv_cond term (vqvae.py:309-312):
 * out[b][o] = sum_i W[o][i] * c[b][i] + bias[o]   (f32, W from weight norm
 * in f32).  And its backward:  dW[o][i] += sum_b dout[b][o] * c[b][i],
 * dc[b][i] += sum_o dout[b][o] * W[o][i]. */
/* All ResSkip blocks' speaker-conditioning linears in one launch (conv_cond on
 * the time-constant embedding, layers.py:218-236; table on the device).
 * fwd: out_l[b][o] = W_l[o][:] . c[b][:] + bias_l[o].
 * bwd: dW_l = dout_l^T c, dbias_l = colsum(dout_l) (both overwritten) and
 *      dc[b][i] = sum_l sum_o dout_l[b][o] W_l[o][i] (overwritten; NULL skips),
 *      reduced deterministically from split-K partials
 *      [n * ceil(O/64)][B][I] f32 (caller workspace). */
typedef struct vqx_linear_layer {
  const float* W;      /* [O][I] */
  const float* bias;   /* [O] or NULL */
  float* out;          /* fwd [B][O] */
  const float* dout;   /* bwd [B][O] */
  float* dW;           /* bwd [O][I] */
  float* dbias;        /* bwd [O] or NULL */
} vqx_linear_layer;
int vqx_linear_batched_fwd(const vqx_linear_layer* table_dev, int32_t n, const float* c, int32_t B,
                           int32_t I, int32_t O, vqx_stream_t stream);
int vqx_linear_batched_bwd(const vqx_linear_layer* table_dev, int32_t n, const float* c, int32_t B,
                           int32_t I, int32_t O, float* dc, float* partials, vqx_stream_t stream);
/* The same with c[b] = emb[ids[b]] (ABI 126): the embedding lookup
 * (vqx_embedding_fwd) folded into the operand loads, for I = 128, B <= 64,
 * O % 64 == 0 and a 16-B aligned table (anything else: an error). */
int vqx_linear_batched_fwd_ids(const vqx_linear_layer* table_dev, int32_t n, const float* emb,
                               const int64_t* ids, int32_t B, int32_t I, int32_t O, vqx_stream_t stream);
/* The training step's prologue as one launch (ABI 128): the three
 * independent jobs a step begins with --
 *   vqx_linear_batched_fwd_ids(cond_table_dev, n_cond, emb, ids, B, I, O)
 *     (the speaker conditioning, vqvae.py decoder inputs),
 *   vqx_nct_to_ntc(x_nct, xB, C, T, y, ldy, y_dtype) (the input's layout) and
 *   vqx_weight_norm_fwd_flags(wn_host, wn_dev, n_wn, VQX_WNF_NORMS_READY)
 *     (the ConvTranspose packs; their row norms must be current) --
 * with the three calls' results bit for bit, in one grid.  A job is skipped
 * with n_cond = 0, x_nct = NULL or n_wn = 0; n_wn <= 256; the conditioning
 * job has vqx_linear_batched_fwd_ids's limits (anything else: an error). */
int vqx_step_prologue(const vqx_wn_layer* wn_host, const vqx_wn_layer* wn_dev, int32_t n_wn,
                      const vqx_linear_layer* cond_table_dev, int32_t n_cond, const float* emb,
                      const int64_t* ids, int32_t B, int32_t I, int32_t O, const float* x_nct, int32_t xB,
                      int32_t C, int32_t T, void* y, int32_t ldy, int32_t y_dtype, vqx_stream_t stream);
int vqx_linear_batched_bwd_ids(const vqx_linear_layer* table_dev, int32_t n, const float* emb,
                               const int64_t* ids, int32_t B, int32_t I, int32_t O, float* dc, float* partials,
                               vqx_stream_t stream);

int vqx_linear_f32(const float* c, const float* W, const float* bias, int32_t B, int32_t I,
                   int32_t O, float* out, vqx_stream_t stream);
int vqx_linear_bwd_f32(const float* dout, const float* c, const float* W, int32_t B, int32_t I,
                       int32_t O, float* dW, float* dc, vqx_stream_t stream);

/*
 * Global gradient norm + fused Adam (trainer/basic.py:63-69:
 * clip_grad_norm_(max_norm) then torch.optim.Adam(betas, eps, wd=0)).
 * grad_sq_norm: out[0] = sum g^2 over the flat buffer (deterministic;
 *   partials >= 1024 floats).
 * adam_hyper: increments the device step counter t and writes
 *   hyper[8] = {lr_t, lr_t/(1-b1^t), sqrt(1-b2^t), t, 1-b1, b2, 1-b2, eps}
 *   with every scalar formed in double like torch's Python-float math, then
 *   rounded to f32; lr_t = lr0*gamma^floor((t-1)/step_size) (StepLR,
 *   basic.py:43-46, stepped once per iteration).  Graph-capturable.
 * adam_step: coef = min(1, max_norm/(sqrt(sumsq)+1e-6)) when max_norm > 0;
 *   g' = g*coef; m = lerp(m, g', 1-b1); v = v*b2 + ((1-b2)*g')*g';
 *   p += -(lr/bc1) * (m / (sqrt(v)/sqrt(bc2) + eps))   (torch single-tensor
 *   Adam operation order).
 */
int vqx_grad_sq_norm(const float* g, int64_t n, float* partials, float* out, vqx_stream_t stream);
int vqx_adam_hyper(int64_t* step, double lr0, double gamma, int32_t step_size, double beta1,
                   double beta2, double eps, float* hyper, vqx_stream_t stream);
int vqx_adam_step(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper,
                  const float* sumsq, float max_norm, vqx_stream_t stream);
/* adam_step with the next forward's weight-norm preparation fused in (ABI
 * 125; replaces the per-step torch weight_norm recomputation of
 * w = g*v/||v||, vqvae.py:203-208 / 329-334, that vqx_weight_norm_fwd does
 * otherwise).  rows: weight-normed convs (vqx_wn_layer with v, g pointing into
 * p; kind 0 needs w_packed) whose rows of v and gains g this launch updates,
 * writing norm[o] = ||v_o|| of the updated row and, for kind 0, the packed
 * weights -- bit for bit what vqx_weight_norm_fwd computes from the updated
 * parameters; kind 1 (ConvT) rows get their norms, to be packed by
 * vqx_weight_norm_fwd_flags(VQX_WNF_NORMS_READY).  segs: (offset, length)
 * int64 pairs covering every other element of p (host and device copies);
 * rows + segs must cover [0, n) exactly: the host rejects overlapping ranges
 * (round 6) and p, g, m, v that are not 16-B aligned.  The update of every
 * element is adam_step's, bit for bit.  At most 128 layers and 128 segments. */
int vqx_adam_step_wn(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper,
                     const float* sumsq, float max_norm, const vqx_wn_layer* rows_host,
                     const vqx_wn_layer* rows_dev, int32_t n_layers, const int64_t* segs_host,
                     const int64_t* segs_dev, int32_t n_segs, vqx_stream_t stream);

/* RAdam, optim_type: RAdam (replaces trainer/radam.py:5-78 RAdam.step, built
 * by trainer/basic.py:30-34 with betas (0.5, 0.999), weight_decay 0).
 * radam_hyper: increments t and writes hyper[9] = {lr_t, -ss*lr_t, rect, t,
 *   b1, 1-b1, b2, 1-b2, eps}: N_max = 2/(1-b2)-1, N = N_max - 2t b2^t/(1-b2^t);
 *   rect = N >= 5; ss = sqrt((1-b2^t)(N-4)/(N_max-4)(N-2)/N N_max/(N_max-2))
 *   / (1-b1^t) when rect, else 1/(1-b1^t) (radam.py:49-59), all in double
 *   like the Python floats, then rounded to f32; lr_t as adam_hyper (StepLR).
 * radam_step: g' = coef*g (clip as adam_step); v = v*b2 + ((1-b2)*g')*g';
 *   m = m*b1 + (1-b1)*g'; p += (-ss*lr) * (m / (sqrt(v) + eps)) when rect,
 *   else p += (-ss*lr) * m (radam.py:41-42, 64-71). */
int vqx_radam_hyper(int64_t* step, double lr0, double gamma, int32_t step_size, double beta1,
                    double beta2, double eps, float* hyper, vqx_stream_t stream);
int vqx_radam_step(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper,
                   const float* sumsq, float max_norm, vqx_stream_t stream);

/*
 * Multi-tensor clip + Adam / RAdam (ABI 130, additive): for a model whose
 * gradients are separate tensors with addresses that change every step (torch
 * autograd over vqvae2.Model), while p, m and v stay flat.  grads, numel and
 * offset are HOST arrays of n entries; the device pointers in grads may be
 * NULL (a parameter without a gradient) and must be 4-B aligned.  Any n is
 * accepted: the tensors go to the device in groups of at most
 * VQX_MULTI_MAX_TENSORS per launch, pointers and lengths by value in the
 * kernel arguments, so nothing is uploaded, allocated or synchronised.
 * multi_chunks: *out = sum ceil(numel[i] / VQX_MULTI_CHUNK) (host only).
 * multi_sq_norm: one partial sum of g^2 per VQX_MULTI_CHUNK-element chunk of
 *   every tensor, in tensor order, so the position of every partial follows
 *   from numel alone; a NULL gradient writes zeros for its chunks.  n_partials
 *   must equal multi_chunks.  Deterministic, and the same bits for a 16-B
 *   aligned gradient and one that is not.  Finish with vqx_sq_norm_finish_adam
 *   or vqx_sq_norm_finish (+ vqx_radam_hyper), no ranges.
 * multi_adam_step: tensor i updates p, m, v[offset[i], offset[i] + numel[i])
 *   from grads[i]; kind 0 is vqx_adam_step's element update, 1 vqx_radam_step's,
 *   bit for bit what those give on a gathered copy.  A NULL gradient leaves
 *   that tensor's p, m and v untouched (torch.optim.Adam skips a parameter
 *   without a gradient).  The ranges must be in increasing order, disjoint and
 *   inside [0, n_flat).  16-B accesses for a tensor whose p + offset,
 *   m + offset, v + offset and gradient are all 16-B aligned, single elements
 *   otherwise.
 * multi_pack (data parallel; additive, the ABI version does not change):
 *   flat[offset[i] + j] = grads[i][j] for every tensor, so that a collective
 *   sees one flat gradient; a NULL gradient has its range zero-filled (no rank
 *   sends uninitialised memory).  Same ranges rule as multi_adam_step, checked
 *   before any launch; flat and the gradients 4-B aligned.  16-B loads and
 *   stores for a tensor whose gradient and flat + offset are both 16-B
 *   aligned, single elements otherwise.  ceil(n / VQX_MULTI_MAX_TENSORS)
 *   launches.
 */
#define VQX_MULTI_MAX_TENSORS 128
#define VQX_MULTI_CHUNK 4096
int vqx_multi_chunks(const int64_t* numel, int32_t n, int64_t* out);
int vqx_multi_sq_norm(const float* const* grads, const int64_t* numel, int32_t n, float* partials,
                      int64_t n_partials, vqx_stream_t stream);
int vqx_multi_adam_step(float* p, float* m, float* v, int64_t n_flat, const int64_t* offset,
                        const int64_t* numel, const float* const* grads, int32_t n, const float* hyper,
                        const float* sumsq, float max_norm, int32_t kind, vqx_stream_t stream);
int vqx_multi_pack(float* flat, int64_t n_flat, const int64_t* offset, const int64_t* numel,
                   const float* const* grads, int32_t n, vqx_stream_t stream);

/*
 * Straight-through VectorQuantizer (use_ema: false; layers_vq.py:9-163,
 * reduction 'frame_mean', target_norm 1.0, z_dim 64, 128 or 256).
 * vqx_vq_normalize (embed_norm: true): the codebook parameter E [K][D] is
 *   renormalised in place (embed_norm(), :28-33) and emb_norm = E/||E||
 *   (:99), e_len = ||E|| after that step; z_norm = z/||z|| (:97), z_len =
 *   ||z||; normloss_out = sum (z_norm - z)^2 (:125-126; partials >= N/4+1).
 *   Then vqx_vq_forward(z_norm, emb_norm, ..., bsum, bcnt) gives idx, z_q,
 *   the commitment sum and the per-code sums/counts the backward uses.
 * vqx_vq_perplexity: exp(-sum p log(p + 1e-10)), p = counts/N (:112-114).
 * vqx_vq_plain_bwd: gradients of x_loss + z_qut + beta*z_enc (scale =
 *   2/(B*T)): dz [N][D] (dtype) from the decoder's straight-through gradient
 *   dzq (zeroed on frames the Jitter replaced: src_t[t] != t; NULL = no
 *   jitter) plus the commitment / normalisation terms through z/||z||, and
 *   the codebook-parameter gradient dE [K][D] f32 (overwritten) through
 *   E/||E|| (or directly when normalize = 0, emb = E).
 */
int vqx_vq_normalize(const float* z, int64_t n_rows, int32_t D, float* E, int32_t K, float* z_norm,
                     float* z_len, float* emb_norm, float* e_len, float* partials, float* normloss_out,
                     vqx_stream_t stream);
int vqx_vq_perplexity(const float* counts, int32_t K, int64_t n_rows, float* out, vqx_stream_t stream);
int vqx_vq_plain_bwd(const float* z, const float* z_norm, const float* z_len, const float* zq,
                     const void* dzq, const int32_t* src_t, int32_t T, int64_t n_rows, int32_t D,
                     int32_t normalize, float beta, float scale, void* dz, int32_t dtype, const float* bsum,
                     const float* bcnt, const float* emb, const float* e_len, int32_t K, float* dE,
                     vqx_stream_t stream);

/* vqx_vq_plain_bwd for a quantizer level inside autograd (no readback, no
 * jitter map): the weights of the two loss terms given apart, z_qut by s_qut
 * (vqx_vq_plain_bwd's scale) and z_enc by s_enc (its beta * scale), each
 * multiplied by an upstream gradient read from the device, g_qut[0] and
 * g_enc[0]; a NULL pointer stands for 1, and with both NULL the result has
 * vqx_vq_plain_bwd's bits.  Additive: the ABI version does not change. */
int vqx_vq_plain_bwd_g(const float* z, const float* z_norm, const float* z_len, const float* zq, const void* dzq,
                       int32_t T, int64_t n_rows, int32_t D, int32_t normalize, float s_qut, float s_enc,
                       const float* g_qut, const float* g_enc, void* dz, int32_t dtype, const float* bsum,
                       const float* bcnt, const float* emb, const float* e_len, int32_t K, float* dE,
                       vqx_stream_t stream);

/* dst[r][c] = act(scale * src[r][c]) with dtype conversion (act = VQX_PRO_*;
 * the decoder's ReLU(sqrt(1/11) * skip) operand, vqvae.py:316-317). */
int vqx_scale_act_2d(const void* src, int32_t ld_src, int32_t src_dtype, void* dst, int32_t ld_dst,
                     int32_t dst_dtype, int64_t rows, int32_t cols, float scale, int32_t act,
                     vqx_stream_t stream);

/* 2-D strided copy with dtype conversion: dst[r][c] = src[r][c] for r < rows,
 * c < cols; src == NULL fills zeros.  Used for the decoder's skip-sum cast
 * and the residual/skip gradient buffers of the backward. */
int vqx_convert_2d(const void* src, int32_t ld_src, int32_t src_dtype, void* dst, int32_t ld_dst,
                   int32_t dst_dtype, int64_t rows, int32_t cols, vqx_stream_t stream);
/* convert_2d(src, dst) and, in the same launch, zero_dst[r][c] = 0 for r <
 * zero_rows, c < zero_cols (dst's dtype; ABI 126: the decoder backward's
 * dL/dskip copy and the zero dL/dx at the decoder output in one launch). */
int vqx_convert_2d_zero2(const void* src, int32_t ld_src, int32_t src_dtype, void* dst, int32_t ld_dst,
                         int32_t dst_dtype, int64_t rows, int32_t cols, void* zero_dst, int32_t ld_zero,
                         int64_t zero_rows, int32_t zero_cols, vqx_stream_t stream);

/* Work units per split of the weight-gradient kernel that vqx_conv1d_wgrad
 * would launch for these arguments, one unit = one 4-wave group (two per CU
 * fill the GPU): 3-tap, pad-1 bf16 layers with T % 64 == 0 and
 * c_dim % 64 == 0 run the tap-reuse kernel (128 rows x 3 taps x 64 channels
 * per tile, two 4-wave K groups per tile), the rest one group per 128 x 128
 * tile.  Callers size `splits` (and the slab buffer) from it. */
int vqx_wgrad_tiles(int64_t n_rows, int32_t T, int32_t r_dim, int32_t c_dim, int32_t ntaps, int32_t pad,
                    int32_t dil, int32_t dtype, int32_t q_prologue, int32_t kernel_policy /* ABI 125 */,
                    int32_t* tiles);

/* Thread-local description of the last failure. */
const char* vqx_last_error(void);

/* Launch probe (measurement only; its log and switches are per host thread,
 * so calls on other threads are unaffected).  While on,
 * each conv GEMM launch records a start/stop event pair stamped on its own
 * dispatch (hipExtLaunchKernelGGL); after the stream is synchronised,
 * vqx_probe_read returns per launch {dtype, mode, prologue, gen, epilogue kind},
 * the algorithmic FLOPs and the kernel duration in ms.  enable(0/1) pauses /
 * resumes recording (an event-stamped dispatch costs a few us of queue time,
 * so callers sample); clear() empties the log. */
int vqx_probe_enable(int32_t on);
/* Record only the launches whose {dtype, mode, prologue, gen, epilogue kind}
 * equal info5 (one kernel symbol; the others launch without events); NULL =
 * every launch. */
int vqx_probe_select(const int32_t* info5);
int vqx_probe_clear(void);
int vqx_probe_count(int64_t* n);
int vqx_probe_read(int64_t i, int32_t* info5, double* flops, float* ms);

/* A stream on all but `reserve_cus` of the current device's CUs
 * (hipExtStreamCreateWithCUMask; mask bit i is CU i / 8 of XCD i % 8, so
 * the top `reserve_cus` bits are cleared: reserve_cus / 8 per XCD), for measuring what co-resident work such as RCCL's all-reduce
 * kernels costs the step (bench.py --reserve-cus).  *cus_used = the CUs the
 * stream may use.  No reference counterpart (measurement only). */
int vqx_stream_create_cu_mask(int32_t reserve_cus, vqx_stream_t* out, int32_t* cus_used);
int vqx_stream_destroy(vqx_stream_t stream);

/* Host mailbox for the step statistics (ABI 127; replaces the loss .item()
 * reads of vqvae.py:85-87 / layers_vq.py:229-232 with one stream-ordered
 * publish the host polls).  vqx_mailbox_create allocates `slots` slots of
 * `floats` (<= 64) f32 values in mapped, coherent pinned host memory: layout
 * [slots] uint32 sequence numbers, then [slots][floats] values, zeroed; *host
 * is the host view, *dev the device pointer of the same bytes.
 * vqx_mailbox_publish (one 64-thread workgroup on `stream`) copies src[0..n)
 * into slot `slot` (and into dev_copy, a device buffer, when non-NULL), then,
 * behind a system-scope release, stores `seq` as the slot's sequence number:
 * a host that reads the number equal to seq reads that step's values.  No
 * marker or copy enters the stream. */
int vqx_mailbox_create(int32_t slots, int32_t floats, void** host, void** dev);
int vqx_mailbox_destroy(void* host);
int vqx_mailbox_publish(const float* src, int32_t n, float* dev_copy, void* box_dev, int32_t slot, int32_t slots,
                        int32_t floats, uint32_t seq, vqx_stream_t stream);

/*
 * Style-token (GST) layer of the hierarchical model's top-level quantizer
 * (ABI 129; model/layers_gst.py:10-147, called as layer(z.mean(dim=-1)) at
 * vqvae2.py:97): a 1-query x N-token multi-head attention over
 * tanh(gst_embs) with q/k/v/out linears, fp32 throughout.
 *   ref[b]  = mean_t z[b*T + t][0..R)            (T = 1: forward(ref_embs))
 *   tok     = tanh(gst_embs) [N][E];  K = tok Wk^T + bk;  V = tok Wv^T + bv
 *   q[b]    = ref[b] Wq^T + bq;       per head h of width d_k = F / H:
 *   a[b][h] = softmax_n(q_h . K[n]_h / sqrt(d_k));  ctx_h = sum_n a[n] V[n]_h
 *   style[b] = ctx[b] Wo^T + bo                                    [B][F]
 * vqx_gst_fwd: 2 launches (K/V per token; pool + attention per batch row),
 * saving tok, K, V, ref, q, a, ctx in `ws`.  vqx_gst_bwd: 3 launches from
 * d_style and the `ws` the forward filled; every gradient is overwritten
 * (dz[b*T + t] = d_ref[b] / T on every frame; dbk is written as zeros: the
 * softmax is invariant to a per-head constant).  Every sum over B, T, N runs
 * in a fixed order without atomics: two runs give the same bits.
 * Weights are nn.Linear's [out][in]: wq [F][R], wk / wv [F][E], wo [F][F].
 * Limits (else -1): B, T >= 1; R % 4 == 0, R <= 512; 1 <= N <= 32; F % H == 0,
 * F <= 512, d_k <= 128; E >= 1; ldz, lddz >= R; the pointers each call reads
 * or writes non-NULL.  `ws` holds >= vqx_gst_workspace(...) floats.
 */
typedef struct {
  const float* z;        /* [B*T][ldz] frame-major, R columns used       */
  const float* gst_embs; /* [N][E]                                       */
  const float *wq, *bq, *wk, *bk, *wv, *bv, *wo, *bo;
  float* style;          /* fwd out [B][F]                               */
  float* ws;             /* workspace, fwd writes / bwd reads + scratch  */
  const float* d_style;  /* bwd in [B][F]                                */
  float* dz;             /* bwd out [B*T][lddz]                          */
  float* d_gst_embs;     /* bwd out, shapes of the parameters            */
  float *dwq, *dbq, *dwk, *dbk, *dwv, *dbv, *dwo, *dbo;
  int32_t B, T, R, N, E, F, H, ldz, lddz;
} vqx_gst_args;
/* Host-only size query (floats) of the workspace of one forward + backward. */
int vqx_gst_workspace(int32_t B, int32_t N, int32_t F, int32_t H, int32_t R, int32_t E, int64_t* floats);
int vqx_gst_fwd(const vqx_gst_args* a, vqx_stream_t stream);
int vqx_gst_bwd(const vqx_gst_args* a, vqx_stream_t stream);

/*
 * Level upsampling + concatenation of the hierarchical decoders (ABI 130;
 * Model.upsample + torch.cat, vqvae2.py:105-114, 130-143).  A level l is
 * frame-major fp32 z_l [B][T_l][ld] with C_l channels and 1 <= T_l <= T;
 * stretched to T frames, frame t reads src_l(t) = min(t / (T / T_l), T_l - 1)
 * (repetition by T / T_l, the tail replicate-padded; nothing is cropped).
 *   fwd: out[b*T + t][off_l + c] = z_l[b][src_l(t)][c], off_l the running sum
 *        of C_l; out [B*T][ldo] in VQX_F32 (a copy) or VQX_BF16 (rounded to
 *        nearest even); columns from sum C_l up are not written.
 *   bwd: z_l (overwritten) = dz_l[b][s][c] = sum_{t: src_l(t) = s}
 *        dout[b*T + t][off_l + c], dout fp32 or bf16, accumulated in fp32 in a
 *        fixed order without atomics (vqx_hier.hip states it): equal shapes
 *        give equal bits.  With one level of all the columns it is the
 *        per-segment column sum (the gradient of a segmented row bias).
 * Up to 8 levels, passed by value to the kernels (no device table).  Limits
 * (else -1): n_levels in 1..8; dtype F32 | BF16; B, T >= 1, B*T < 2^31;
 * every pointer non-NULL and 16-B aligned; C_l, ld_l, ldo multiples of 4,
 * ld_l >= C_l; sum C_l <= ldo.
 */
typedef struct vqx_hier_level {
  void* z;               /* fwd: source (read); bwd: dz (written)  [B][T_l][ld] f32 */
  int32_t T_l, C, ld;
} vqx_hier_level;
int vqx_upsample_cat_fwd(const vqx_hier_level* levels, int32_t n_levels, int32_t B, int32_t T, void* out,
                         int32_t ldo, int32_t out_dtype, vqx_stream_t stream);
int vqx_upsample_cat_bwd(const vqx_hier_level* levels, int32_t n_levels, int32_t B, int32_t T, const void* dout,
                         int32_t ldo, int32_t dout_dtype, vqx_stream_t stream);
/*
 * vqx_upsample_cat_bwd with the levels' storage type chosen: the same kernel,
 * the same fp32 sums in the same fixed order (no atomics; equal shapes give
 * equal bits), each level stored as level_dtype: VQX_F32 (bit-equal to
 * vqx_upsample_cat_bwd) or VQX_BF16, z_l then bf16 [B][T_l][ld] and every sum
 * rounded once to nearest even.  It hands a level decoder its output gradient
 * in the compute dtype without a convert launch (model/vqvae2b.py).
 * Limits (else -1): those of vqx_upsample_cat_bwd (ld_l counts elements of
 * level_dtype), and level_dtype F32 | BF16.  Additive: the ABI version does
 * not change.
 */
int vqx_upsample_cat_bwd_to(const vqx_hier_level* levels, int32_t n_levels, int32_t B, int32_t T, const void* dout,
                            int32_t ldo, int32_t dout_dtype, int32_t level_dtype, vqx_stream_t stream);

/*
 * The frame-major input of the hierarchical model's first decoder straight
 * from codes, in one launch (conversion: Model.synthesize; the reference's
 * VectorQuantizer.decode, layers_vq.py:61-76, + Model.upsample + torch.cat).
 * A level l is one of two kinds, told apart by `idx`:
 *   dense   (idx NULL)  z_l [B][T_l][ld] f32 with C channels, exactly a level
 *           of vqx_upsample_cat_fwd (the style vector, T_l = 1);
 *   indexed (idx set)   idx_l [B][T_l] int64 into the codebook E [K][ld] f32
 *           with C = D_l columns used:
 *             out[b*T + t][off_l + c] = E[idx_l[b][src_l(t)]][c]
 *           and with `normalize` != 0 that row divided by its own L2 norm
 *           sqrt(sum_c E[k][c]^2), recomputed per output row (the reference's
 *           target_norm * E / ||E|| with target_norm = 1).
 * src_l(t) = min(t / (T / T_l), T_l - 1) and off_l = the running sum of C_l, as
 * vqx_upsample_cat_fwd.  out [B*T][ldo] in VQX_F32 or VQX_BF16 (the f32 value
 * rounded once to nearest even); columns from sum C_l up are not written.  The
 * codebooks are only read; no atomics; equal arguments give equal bits.  The
 * indices are trusted: the caller checks 0 <= idx < K.
 * Up to 8 levels, passed by value to the kernel.  Limits (else -1): n_levels
 * in 1..8; dtype F32 | BF16; B, T >= 1, B*T < 2^31; out, z, idx and E
 * non-NULL where their kind reads them and 16-B aligned; C, ld, ldo multiples
 * of 4, ld >= C; 1 <= T_l <= T; sum C_l <= ldo; K >= 1 for an indexed level.
 * Additive: the ABI version does not change.
 */
typedef struct vqx_codes_level {
  const void* z;         /* dense: [B][T_l][ld] f32; indexed: the codebook E [K][ld] f32 */
  const int64_t* idx;    /* indexed: [B][T_l]; NULL makes the level dense               */
  int32_t T_l, C, ld;    /* C = C_l (dense) or D_l (indexed)                            */
  int32_t K, normalize;  /* indexed only                                                */
} vqx_codes_level;
int vqx_codes_upsample_cat(const vqx_codes_level* levels, int32_t n_levels, int32_t B, int32_t T, void* out,
                           int32_t ldo, int32_t out_dtype, vqx_stream_t stream);

/*
 * Masked layout change of the hierarchical encoder's backward (vqvae2.py:
 * 238-246, the encoder's second output `feat` = LeakyReLU_0.2(a)): the f32
 * (B, C, T) gradient into `feat`, through that LeakyReLU, frame-major:
 *   dst[b*T + t][c] = g_nct[b][c][t] * (a[b*T + t][c] > 0 ? 1 : slope)
 * One f32 product, rounded once to dst_dtype (VQX_F32 | VQX_BF16); `a` is the
 * stored activation [B*T][lda] in a_dtype (only its sign is read).  The result
 * is the `res` operand of the z_proj DGRAD whose epilogue applies MASK before
 * RES, so the sum is lrelu'(a) * (W^T dz + dfeat).  Any B, C, T >= 1
 * (B <= 65535); lda, lddst >= C; no alignment requirement.  Additive: the ABI
 * version does not change.
 */
int vqx_nct_to_ntc_lrelu_bwd(const float* g_nct, int32_t B, int32_t C, int32_t T, const void* a, int32_t lda,
                             int32_t a_dtype, float slope, void* dst, int32_t lddst, int32_t dst_dtype,
                             vqx_stream_t stream);

/* x_nct[b][c][t] = y[b*T + t][c] * g[0]: vqx_ntc_to_nct of an f32 frame-major
 * matrix with one device scalar folded in (the gradient of log_loss into xhat
 * times its upstream gradient, without a readback or a second pass).  Any
 * B, C, T >= 1 (B <= 65535), ldy >= C.  Additive: the ABI version stays. */
int vqx_ntc_to_nct_scale(const float* y, int32_t ldy, int32_t B, int32_t C, int32_t T, const float* g,
                         float* x_nct, vqx_stream_t stream);

/*
 * Layout changes of a quantizer level under autograd with the jitter
 * (layers_vq.py:353-379) folded in, and the EMA level's commitment gradient.
 * src_t is a device int32 [T] neighbour map (frame t shows frame src_t[t]);
 * NULL is the identity.  All three validate on the host before launching
 * (null required pointer, T < 1, C < 1, B < 1 or B > 65535, B*T*C >= 2^31 ->
 * -1 with vqx_last_error), are stream-ordered without host synchronisation
 * and go through the 32 x 32 LDS tile of vqx_nct_to_ntc / vqx_ntc_to_nct.
 * Additive: the ABI version does not change.
 *
 * vqx_ntc_to_nct_gather: x_nct[b][c][t] = y[b*T + src_t[t]][c], f32 (B, C, T)
 *   from rows in dtype (VQX_F32 | VQX_BF16), ldy >= C.  A map entry outside
 *   0..T-1 is clamped into it.
 * vqx_nct_to_ntc_keep: y[b*T + t][c] = src_t[t] == t ? g_nct[b][c][t] : 0,
 *   rounded once to dtype: the jitter's backward (a replaced frame is a
 *   detached copy and passes no gradient; a source frame keeps only its own).
 * vqx_vq_commit_bwd_g: dz = (s * g[0]) * (z - zq) from frame-major f32 z, zq
 *   [B*T][D]; dz is f32 (B, D, T) when nct != 0, else [B*T][D] rows.  g is a
 *   device scalar (NULL: 1).  The product s*g[0] is formed in fp32 first, then
 *   one subtraction and one multiplication per element.
 */
int vqx_ntc_to_nct_gather(const void* y, int32_t ldy, int32_t dtype, int32_t B, int32_t C, int32_t T,
                          const int32_t* src_t, float* x_nct, vqx_stream_t stream);
int vqx_nct_to_ntc_keep(const float* g_nct, int32_t B, int32_t C, int32_t T, const int32_t* src_t, void* y,
                        int32_t ldy, int32_t dtype, vqx_stream_t stream);
int vqx_vq_commit_bwd_g(const float* z, const float* zq, int32_t B, int32_t D, int32_t T, float s, const float* g,
                        int32_t nct, float* dz, vqx_stream_t stream);

/*
 * A batch of different lengths (the hierarchical model's batched conversion,
 * forward only): frame-major rows [B*T][ld] in which utterance b owns rows
 * t < len[b], 1 <= len[b] <= T.  `len` (and n_len / m_len) are HOST arrays:
 * they are checked item by item before the first launch (a failure names the
 * item in vqx_last_error() and launches nothing) and travel to the kernels by
 * value in the kernel arguments, 896 utterances a launch (96 for the
 * concatenation), so there is no device table, copy, allocation or
 * synchronisation.  n_rows = B*T < 2^31.  dtype VQX_F32 | VQX_BF16; pointers
 * 16-B aligned, channel counts and strides multiples of a 16-byte chunk (4 f32
 * / 8 bf16).  No atomics: equal arguments give equal bits.  Additive: the ABI
 * version does not change.
 *
 * vqx_groupnorm_stats_len: vqx_groupnorm_stats over rows t < len[b] only
 *   (G = 1 or 2; two passes per row part, the 8 parts merged in order in
 *   double); partials >= B*G*24 floats, mean_rstd [B][G][2] as the plain call.
 * vqx_gn_lrelu_fwd_len / vqx_gn_glu_fwd_len: vqx_gn_lrelu_fwd / vqx_gn_glu_fwd
 *   on rows t < len[b] (the same bits as the plain call on those rows); rows
 *   t >= len[b] of g are written as zeros and not read.
 * vqx_mask_tail: x[b*T + t][0..C) = 0 for len[b] <= t < T, in place; nothing
 *   else is read or written.
 * vqx_codes_upsample_cat_len: vqx_codes_upsample_cat with per-utterance
 *   lengths.  Level l is stored with its own padded T_l (levels[l].T_l);
 *   utterance b has target length n_len[b] <= T and level lengths
 *   m_len[b*n_levels + l], 1 <= m <= min(n_len[b], T_l):
 *     out[b*T + t][off_l + c] = level_l[b][min(t / (n_b / m), m - 1)][c], t < n_b
 *   and zeros over [0, sum C_l) for t >= n_b.  Index entries at t >= m are
 *   never read.
 * vqx_segment_mean: out[b][c] = (sum_{t < len[b]} z[b*T + t][c]) / len[b], f32
 *   z [B*T][ldz] -> out [B][ldo], summed in a fixed order.
 * vqx_nct_to_ntc_len / vqx_ntc_to_nct_len (the flat model's batched conversion):
 *   vqx_nct_to_ntc / vqx_ntc_to_nct with the tail mask in the same pass.
 *     y[b*T + t][c] = t < len[b] ? cvt(x_nct[b][c][t]) : 0          (x f32 (B, C, T))
 *     x_nct[b][c][t] = t < len[b] ? float(y[b*T + t][c]) : 0, t < T_out <= T
 *                                                          (x f32 (B, C, T_out))
 *   The zero is selected, not multiplied, and the source is not loaded at
 *   t >= len[b]: it may hold anything there, NaN included.  Any C >= 1,
 *   ldy >= C; pointers aligned to their element.
 * vqx_nct_to_ntc_pad_len (vqvae2a / vqvae2b's batched conversion): the source
 *   x f32 (B, C, T_in) is shorter than the T >= T_in rows every utterance gets
 *   in y [B*T][ldy]:
 *     y[b*T + t][c] = t < len[b] ? cvt(x_nct[b][c][t]) : 0, t < T, 1 <= len[b] <= T_in
 *   One pass in place of a zero-padded copy, vqx_nct_to_ntc and vqx_mask_tail.
 *   The zero is selected and x is not loaded at t >= len[b].  T < T_in -> -1.
 * vqx_index_mask_len: out[b][t] = t < len[b] ? idx[b*T + t] : 0 over
 *   t < T_out <= T, 1 <= len[b] <= T_out; idx int64 [B*T], out int64
 *   (B, T_out), both 8-B aligned: the codes of a padded batch with zeros at the
 *   padded positions.  idx is not loaded at t >= len[b].  T_out > T -> -1.
 */
int vqx_groupnorm_stats_len(const void* x, int32_t ldx, int32_t dtype, int64_t n_rows, int32_t T, int32_t C,
                            int32_t G, const int32_t* len, float eps, float* partials, float* mean_rstd,
                            vqx_stream_t stream);
int vqx_gn_lrelu_fwd_len(const void* h, int32_t ldh, void* g, int32_t ldg, int32_t dtype, int64_t n_rows, int32_t T,
                         int32_t C, const int32_t* len, const float* mean_rstd, const float* gamma, const float* beta,
                         vqx_stream_t stream);
int vqx_gn_glu_fwd_len(const void* u, int32_t ldu, void* g, int32_t ldg, int32_t dtype, int64_t n_rows, int32_t T,
                       int32_t C, const int32_t* len, const float* mean_rstd, const float* gamma, const float* beta,
                       vqx_stream_t stream);
int vqx_mask_tail(void* x, int32_t ldx, int32_t dtype, int64_t n_rows, int32_t T, int32_t C, const int32_t* len,
                  vqx_stream_t stream);
int vqx_codes_upsample_cat_len(const vqx_codes_level* levels, int32_t n_levels, int32_t B, int32_t T,
                               const int32_t* n_len, const int32_t* m_len, void* out, int32_t ldo, int32_t out_dtype,
                               vqx_stream_t stream);
int vqx_segment_mean(const float* z, int32_t ldz, int64_t n_rows, int32_t T, int32_t C, const int32_t* len,
                     float* out, int32_t ldo, vqx_stream_t stream);
int vqx_nct_to_ntc_len(const float* x_nct, int32_t B, int32_t C, int32_t T, const int32_t* len, void* y, int32_t ldy,
                       int32_t dtype, vqx_stream_t stream);
int vqx_ntc_to_nct_len(const void* y, int32_t ldy, int32_t dtype, int32_t B, int32_t C, int32_t T, const int32_t* len,
                       float* x_nct, int32_t T_out, vqx_stream_t stream);
int vqx_nct_to_ntc_pad_len(const float* x_nct, int32_t B, int32_t C, int32_t T_in, int32_t T, const int32_t* len,
                           void* y, int32_t ldy, int32_t dtype, vqx_stream_t stream);
int vqx_index_mask_len(const int64_t* idx, int32_t B, int32_t T, const int32_t* len, int64_t* out, int32_t T_out,
                       vqx_stream_t stream);

/*
 * Self-attention over latent frames (additive to ABI 130; the reference's
 * MultiHeadedAttention, model/layers_gst.py:63-147, called as
 * mha(x, x, x, key mask)): the part between the q/k/v GEMM and the output
 * GEMM, per utterance b and head h of width d_k = F / H:
 *   S   = q_h k_h^T / sqrt(d_k)  over the keys t2 < len[b]
 *   P   = softmax over those keys;   ctx_h = P v_h
 *   lse = log sum exp S per query row (all the forward saves beside qkv, ctx)
 * which equals the reference's masked branch (masked_fill(min), softmax,
 * masked_fill(0)) whenever len[b] >= 1.  `qkv` is the packed output of one
 * GEMM: frame-major rows [B*T][ldqkv] in the compute dtype, q in columns
 * [0, F), k in [F, 2F), v in [2F, 3F), head h in columns h*d_k .. (h+1)*d_k of
 * each part.  vqx_attn_fwd: 1 launch, keys streamed in tiles with an online
 * softmax (running maximum and sum per query row in f32), any T >= 1.
 * vqx_attn_bwd: 3 launches: delta = rowsum(d_ctx * ctx) into `ws`; dK and dV
 * of a 64-key tile held in accumulators over a sweep of the query tiles; dQ
 * of a 64-query tile over a sweep of the key tiles.  Both recompute P from
 * q, k and lse.  Each output is written by one workgroup: no atomics, no sum
 * whose order depends on scheduling; equal arguments give equal bits.
 * VQX_BF16 multiplies with mfma_f32_16x16x32_bf16 (f32 accumulation; scores,
 * maxima and sums f32; P and dS rounded to bf16 only as MFMA operands),
 * VQX_F32 with mfma_f32_16x16x4_f32 (P stays f32).  fp8 is not built.
 * Rows t >= len[b] of qkv and d_ctx are never loaded (they may hold NaN);
 * rows t >= len[b] of ctx and d_qkv are written as exact zeros (lse: 0).
 * `len` is a host array of B entries in [1, T], validated before the first
 * launch and passed by value (896 utterances a launch), or NULL (all T).
 * Limits (else -1): B, T >= 1, B*T < 2^31; F % H == 0, d_k in {32, 64};
 * ldqkv >= 3F, ldc >= F, both multiples of the 16-byte chunk; qkv, ctx, d_ctx,
 * d_qkv 16-byte aligned; `ws` holds >= vqx_attn_workspace(...) floats (bwd).
 */
typedef struct {
  const void* qkv;    /* [B*T][ldqkv], compute dtype                      */
  void* ctx;          /* [B*T][ldc], F columns: fwd out, bwd in           */
  float* lse;         /* [B][H][T]: fwd out, bwd in                       */
  const void* d_ctx;  /* bwd in, layout of ctx                            */
  void* d_qkv;        /* bwd out, layout of qkv                           */
  float* ws;          /* bwd scratch                                      */
  const int32_t* len; /* host, B entries, or NULL                         */
  int32_t B, T, F, H, ldqkv, ldc, dtype;
} vqx_attn_args;
/* Host-only size query (floats) of the backward's workspace. */
int vqx_attn_workspace(int32_t B, int32_t T, int32_t F, int32_t H, int32_t dtype, int64_t* floats);
int vqx_attn_fwd(const vqx_attn_args* a, vqx_stream_t stream);
int vqx_attn_bwd(const vqx_attn_args* a, vqx_stream_t stream);

/* ABI 130: vqx_conv_args.rowbias_T appended (segmented row bias of the forward
 * epilogue; 0 or 1 keeps every earlier call's bits) and vqx_upsample_cat_*. */
/* ABI version (major*100 + minor); VQX_ABI_VERSION is what this header describes. */
#define VQX_ABI_VERSION 130
int vqx_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VQX_H */
