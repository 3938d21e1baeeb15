/* dm3d.h — C ABI of libdm3d_hip.so: the MI355X (gfx950) kernels behind the 3D latent-diffusion denoising path.
 *
 * The reference (aayush9400/3D-Condtional-Stable-Diffusion) has no FFI / plugin boundary of its own: the path sits
 * behind Keras layer objects (networks/conditional_dm3d.py:324-415 build_model, :517-575 sample/generate).  This
 * header is therefore the build-defined replacement boundary: one entry point per stock
 * TensorFlow/Keras op family the reference's hot path executes.  Each entry cites the reference call it replaces.
 *
 * Conventions
 *   - plain C: raw device pointers, explicit sizes, a hipStream_t passed as void*; no torch types.
 *   - every function enqueues on the caller's stream and returns without synchronising (graph-capturable);
 *     nothing allocates, frees or retains pointers.  The caller owns every buffer.
 *   - return 0 on success, a negative DM3D_E* code otherwise; dm3d_last_error() gives the thread-local text.
 *   - all tensors float32, activations NDHWC (Keras channels_last), pointers 16-byte aligned.
 */
#ifndef DM3D_H
#define DM3D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DM3D_VERSION 111          /* major*100 + minor; the descriptor structs grew in 101 (w_layout), 102 (scratch), 103 (skip_*),
                                     104 (dm3d_attention), 105 (x1_fmt / out_fmt / post_*), 106 (ddpm seed_dev; conv/gemm range_flag; the
                                     training entries), 107 (conv wpk_f8: a float8 cross-term form, removed again in 109), 108 (conv wpk_wino: the Winograd-x form), 109 (wpk_f8 and
                                     dm3d_pack_weights_h3f8 are gone; the Winograd-x image pairs its taps differently; dm3d_mlp_fused; conv skip_wpk_frag, gn_stats; dm3d_groupnorm_finalize2), 110 (dm3d_attn_front), 111 (conv split_counters: the Cin split
                                     meets inside the launch; dm3d_conv_split_counter_words); dm3d_ddim_update / dm3d_ddim_desc, dm3d_edit_update / dm3d_edit_desc,
                                     dm3d_guide_update / dm3d_guide_desc, dm3d_dpm_update / dm3d_dpm_desc and dm3d_x0_threshold / dm3d_thresh_desc were added within 111 (no existing entry changed; dm3d_ddim_desc and dm3d_dpm_desc grew by one trailing optional pointer, x0_bound, which a zeroed descriptor leaves NULL; dm3d_thresh_desc then by one, frame, likewise, and dm3d_ddim_update_frame / dm3d_dpm_update_frame are new entries),
                                     and dm3d_pred_to_eps / dm3d_pred_desc, dm3d_objective_loss_grad / dm3d_loss_desc and dm3d_dpm_sde_update(_frame) / dm3d_dpm_sde_desc and dm3d_grad_scale / dm3d_gradscale_desc / dm3d_adam_scaled and dm3d_unipc_update / dm3d_unipc_desc likewise (new entries and structs only): a host built against an older header must be rebuilt */

#define DM3D_OK            0
#define DM3D_EINVAL       -1      /* bad argument (shape, alignment, null pointer) */
#define DM3D_EUNSUPPORTED -2      /* valid request the kernels do not implement */
#define DM3D_EHIP         -3      /* a HIP runtime call failed (text holds hipGetErrorString) */

#define DM3D_ACT_NONE 0
#define DM3D_ACT_RELU 1
#define DM3D_ACT_SILU 2

/* arithmetic of the contraction kernels.
 *   F32: v_mfma_f32_32x32x2_f32, exact float32 products and accumulation (157 TFLOP/s peak).
 *   H3 : every float32 operand x is split on the fly into two float16 terms x = hi + lo (|x - hi - lo| <= 2^-22 |x|),
 *        and a.b is evaluated as ah.bh + ah.bl + al.bh with three v_mfma_f32_32x32x16_f16 passes accumulating in
 *        float32 (dropped term al.bl <= 2^-22 |a.b|): float32-grade results at 1/3 of the 16-bit MFMA rate.  Weights
 *        are pre-scaled by 2^w_exp (undone exactly in the epilogue) so their lo terms stay normal float16 numbers;
 *        activations are clamped to +-65504 before the split. */
#define DM3D_PREC_F32 0
#define DM3D_PREC_H3  1

/* storage formats of a [rows][k] matrix (same 4 bytes per element, leading dimensions always counted in elements):
 *   F32: row-major float32.
 *   H2 : the float16 hi/lo split of DM3D_PREC_H3 made once by the producer instead of by every consumer: each run of 16
 *        consecutive k of a row is one 64-byte record [hi k0-7 | hi k8-15 | lo k0-7 | lo k8-15] — exactly the LDS record
 *        of the H3 kernels, so their staging degenerates to 16-byte copies.  ld % 16 == 0. */
#define DM3D_FMT_F32 0
#define DM3D_FMT_H2  1

/* padded extents of packed weights */
#define DM3D_COUT_PAD 64
#define DM3D_CIN_PAD  16

int         dm3d_version(void);
const char* dm3d_last_error(void);
/* 1 when a gfx950 device is visible to the calling process, 0 otherwise (never fails). */
int         dm3d_device_ok(void);

/* ---- weights ------------------------------------------------------------------------------------------------
 * Keras kernels are [kd,kh,kw,Cin,Cout] (Conv3D, conditional_dm3d.py:257-259) or [in,out] (Dense, :251; taps=1).
 * The kernels consume them as [taps][CoutPad][CinPad] (K contiguous per output channel, zero padded to
 * DM3D_COUT_PAD / DM3D_CIN_PAD) so that one (tap, Cin-chunk) slice is a dense LDS image.
 * in_scale (optional, [cin]) multiplies the rows — used to fold an inference BatchNormalization that directly
 * precedes a 1x1 conv into its weights (CrossAttentionBlock norm -> proj_in, :187-188). */
int64_t dm3d_packed_weight_elems(int32_t taps, int32_t cin, int32_t cout);
int     dm3d_pack_weights(const float* keras_kernel, int32_t taps, int32_t cin, int32_t cout,
                          const float* in_scale, float* packed, void* stream);

/* H3 image: [CoutPad/64][CinPad/16][taps][64][32 halfs] = per output channel one 64-byte LDS record (hi c0-7, hi c8-15,
 * lo c0-7, lo c8-15; the four 16-byte slots XOR-swizzled by the row), weights multiplied by 2^w_exp before the split.
 * dm3d_packed_weight_h3_bytes gives the buffer size. */
int64_t dm3d_packed_weight_h3_bytes(int32_t taps, int32_t cin, int32_t cout);
int     dm3d_pack_weights_h3(const float* keras_kernel, int32_t taps, int32_t cin, int32_t cout, int32_t w_exp,
                             const float* in_scale, void* packed, void* stream);

/* UpSample (UpSampling3D(2) + Conv3D k3, conditional_dm3d.py:288-296): a 3x3x3 conv on a nearest-2x upsampled tensor equals,
 * per output parity (a,b,c), a 2x2x2 conv on the low-resolution tensor whose taps are sums of the k3 taps that read the same
 * source voxel — 8 taps instead of 27.  These pack the [3,3,3,Cin,Cout] kernel into the 8 parity images that
 * dm3d_conv3d_ndhwc expects in wpk when upsample == 1 (for H3, choose w_exp from the summed taps: up to 8x the largest tap). */
int64_t dm3d_packed_weight_up_elems(int32_t cin, int32_t cout);
int     dm3d_pack_weights_up(const float* keras_kernel, int32_t cin, int32_t cout, float* packed, void* stream);
int64_t dm3d_packed_weight_up_h3_bytes(int32_t cin, int32_t cout);
int     dm3d_pack_weights_up_h3(const float* keras_kernel, int32_t cin, int32_t cout, int32_t w_exp, void* packed, void* stream);
/* (the _up_h3 and _convt_h3 packers write whichever layout dm3d_conv_weight_layout names for their conv, see below) */

/* Conv3DTranspose(k=4, strides=2, padding="same") kernels are [4,4,4,Cout,Cin] in Keras; packed as 8 parity images of a
 * taps=8 conv like the UpSample case (same buffer sizes: dm3d_packed_weight_up_elems / _up_h3_bytes with cin, cout). */
int     dm3d_pack_weights_convt(const float* keras_kernel, int32_t cin, int32_t cout, float* packed, void* stream);
int     dm3d_pack_weights_convt_h3(const float* keras_kernel, int32_t cin, int32_t cout, int32_t w_exp, void* packed, void* stream);

/* Second H3 weight layout, DM3D_WL_PAIR: the image read by the v_mfma_f32_16x16x32_f16 conv kernels (every k3/s1 conv — round 3: also cout <= 32, the narrow column forms —,
 * UpSample, Conv3DTranspose): taps padded to a multiple of 4 with zeros and consumed two at a time, rows permuted inside each
 * group of 16 output channels so that the operand reads are bank-conflict free.  mode 0: plain [taps,Cin,Cout] kernel;
 * mode 1: UpSample [3,3,3,Cin,Cout] -> 8 parity images of 8 taps; mode 2: Conv3DTranspose [4,4,4,Cout,Cin] -> 8 parity images.
 * dm3d_packed_weight_h3p_bytes is the size of ONE image (multiply by 8 for modes 1 and 2, where taps must be 8). */
#define DM3D_WL_TAP   0
#define DM3D_WL_PAIR  1
int64_t dm3d_packed_weight_h3p_bytes(int32_t taps, int32_t cin, int32_t cout);
int     dm3d_pack_weights_h3p(const float* keras_kernel, int32_t taps, int32_t cin, int32_t cout, int32_t w_exp,
                              const float* in_scale, void* packed, int32_t mode, void* stream);
/* image for dm3d_conv_desc.wpk_wino from a [3,3,3,Cin,Cout] kernel: the DM3D_WL_PAIR record format, per 16-channel chunk 20 steps
 * (5 pairs of (dz, dy) taps — (dz, 0) | (dz, 1) for dz = 0, 1, 2; (0, 2) | zero; (1, 2) | (2, 2) —) x 4 transform terms u0 = g0, u1 = (g0+g1+g2)/2, u2 = (g0-g1+g2)/2, u3 = g2 of the x taps */
int64_t dm3d_packed_weight_h3w_bytes(int32_t cin, int32_t cout);
int     dm3d_pack_weights_h3w(const float* keras_kernel, int32_t cin, int32_t cout, int32_t w_exp, const float* in_scale, void* packed,
                              void* stream);
/* the layout dm3d_conv3d_ndhwc wants in wpk for a DM3D_PREC_H3 conv of this geometry (what w_layout must say) */
int32_t dm3d_conv_weight_layout(int32_t ksize, int32_t stride, int32_t upsample, int32_t transpose, int32_t cout);
/* image of a 1x1 kernel [cin, cout] for dm3d_conv_desc.skip_wpk (two 16-channel chunks per MFMA k-step) */
int64_t dm3d_packed_weight_skip_h3p_bytes(int32_t cin, int32_t cout);
int     dm3d_pack_weights_skip_h3p(const float* keras_kernel, int32_t cin, int32_t cout, int32_t w_exp, void* packed, void* stream);
/* the same kernel as MFMA operand fragments (same byte size): [cout tile of 64][pair of 16-channel chunks][16-column tile][hi | lo][lane][16 B],
 * for dm3d_conv_desc.skip_wpk_frag — the Winograd-x form reads its skip weights with plain coalesced loads, without LDS */
int     dm3d_pack_weights_skip_h3f(const float* keras_kernel, int32_t cin, int32_t cout, int32_t w_exp, void* packed, void* stream);

/* ---- Conv3D(padding="same") as implicit GEMM on MFMA ---------------------------------------------------------
 * Replaces layers.Conv3D for k=3/s=1 (:257-259, :348-353, :412-414), k=3/s=2 (DownSample :274-285, TF SAME pad 0
 * before / 1 after on even sizes), k=1 (ResidualBlock skip :245-248) and UpSampling3D(2)+Conv3D (UpSample :288-296,
 * upsample=1 reads the low-resolution tensor at index>>1).  Fused around it:
 *   prologue  x -> silu(x*pro_scale[c] + pro_shift[c])   (inference BatchNormalization + swish, :255-256, 262-263,
 *             410-411), applied before zero padding;
 *   also      k=4/s=2 (VQ-VAE Encoder downsampling, vqvae3d_monai.py:266-273; SAME pad 1/1) and its transpose
 *             (Decoder, :373-377): Conv3DTranspose k4 s2 is evaluated per output parity as a 2x2x2 conv on the input
 *             (parity 0 reads sources {i-1,i} with taps w[3],w[1]; parity 1 reads {i,i+1} with w[2],w[0]);
 *   concat    channels of x1 then x2 (layers.Concatenate(axis=-1)([x, skip]), :396) without materialising it;
 *   epilogue  + bias[co] + vec[row(b)][co] (the time-embedding Dense broadcast-add, :250-253, 260) then optional
 *             ReLU, then + res (layers.Add with the residual, :268). */
typedef struct dm3d_conv_desc {
    const float* x1;            /* [batch, in_d, in_h, in_w, c1] */
    const float* x2;            /* optional second input, same spatial shape, c2 channels (NULL if c2 == 0) */
    int32_t c1, c2;             /* c1 % 4 == 0; with x2: c1 % 16 == 0 and c2 % 4 == 0 */
    int32_t batch;
    int32_t in_d, in_h, in_w;   /* physical extent of x1/x2 */
    int32_t upsample;           /* 1: convolve the nearest-2x upsampled tensor (stride must be 1) */
    int32_t ksize;              /* 1 or 3; 4 with stride 2 (and with transpose) */
    int32_t stride;             /* 1 or 2 */
    const float* wpk;           /* dm3d_pack_weights[_h3] output for (ksize^3, c1+c2, cout); upsample: dm3d_pack_weights_up[_h3] */
    const float* bias;          /* [cout] or NULL */
    const float* pro_scale;     /* [c1+c2] or NULL (both or neither) */
    const float* pro_shift;
    const float* vec;           /* [rows, vec_ld] or NULL */
    const int32_t* vec_idx;     /* [batch] row of vec per sample, or NULL for row = sample index */
    int32_t vec_ld;
    int32_t relu;               /* 1: ReLU after bias/vec, before res */
    const float* res;           /* [batch, out_d, out_h, out_w, cout] or NULL */
    float* out;                 /* [batch, out_d, out_h, out_w, cout], out = ceil(in*(upsample?2:1)/stride) */
    int32_t cout;
    int32_t precision;          /* DM3D_PREC_F32: wpk from dm3d_pack_weights; DM3D_PREC_H3: wpk from dm3d_pack_weights_h3 */
    int32_t w_exp;              /* H3 only: the power-of-two exponent the weights were packed with */
    /* autoencoder bracket (networks/vqvae3d_monai.py): */
    const float* prelu_alpha;   /* keras PReLU() with its default full-shape slope [out_d,out_h,out_w,cout] (shared by the batch),
                                   applied after bias/vec/relu and before res: v = v > 0 ? v : alpha*v; or NULL */
    int32_t relu_out;           /* 1: ReLU after the residual add (VQVAEResidualUnit: ReLU(x + PReLU(BN(conv)))) */
    int32_t transpose;          /* 1: Conv3DTranspose(k=4, strides=2, padding="same"): out = 2*in; wpk from
                                   dm3d_pack_weights_convt[_h3]; ksize must be 4, stride 2, no upsample */
    int64_t pro_batch_stride;   /* elements between consecutive samples' pro_scale / pro_shift vectors: 0 = one vector for
                                   the batch (folded BatchNormalization), c1+c2 = per-sample vectors (GroupNormalization,
                                   written by dm3d_groupnorm_finalize) */
    int32_t w_layout;           /* H3 only: DM3D_WL_TAP or DM3D_WL_PAIR, must equal dm3d_conv_weight_layout(...) */
    /* ResidualBlock skip path fused into this launch (DM3D_PREC_H3, DM3D_WL_PAIR, ksize 3, stride 1, no upsample only):
       out += Conv3D(cout, 1)(concat(skip_x1, skip_x2)) on the raw tensors (no prologue), i.e. layers.Add()([x, residual]) with
       residual = layers.Conv3D(width, kernel_size=1)(x) (conditional_dm3d.py:243-248, 268) without a launch, a tensor or a
       residual read of its own.  skip_wpk from dm3d_pack_weights_skip_h3p, packed with THIS conv's w_exp; add the skip bias into
       bias.  All NULL / 0 when unused. */
    const float* skip_x1; const float* skip_x2; int32_t skip_c1, skip_c2; const void* skip_wpk;
    /* A tensor with exactly one consumer (ResidualBlock: conv1 -> BatchNormalization -> swish -> conv2, :255-267) can skip the
       float32 round trip: the producer applies the consumer's folded norm + swish once per element and stores DM3D_FMT_H2
       (post_scale / post_shift per output channel, out_fmt = DM3D_FMT_H2), the consumer (x1_fmt = DM3D_FMT_H2, no x2, no
       prologue) stages plain copies.  k3 / stride 1 / DM3D_WL_PAIR convs only; an H2 output additionally needs extents that
       are whole 4x8x8 bricks and cout % 64 == 0.  Zero / NULL when unused. */
    int32_t x1_fmt, out_fmt;
    const float* post_scale; const float* post_shift;
    void* scratch;              /* optional workspace (16-byte aligned) of scratch_bytes bytes, or NULL: see split_counters below.
                                   dm3d_conv_scratch_bytes(d) says how much a descriptor can use (0: it never splits). */
    int64_t scratch_bytes;
    /* DM3D_PREC_H3 range guard.  An H3 consumer clamps float32 operands to the float16 range (+-65504) before the hi/lo split — a
       silent difference from the reference's float32 arithmetic if a value ever got there.  With range_flag set, this launch
       writes 1 to *range_flag when any |output value| exceeds range_limit (0 = 65504; hosts pass the smaller bound that also
       covers a consumer's folded norm: (65504 - max|shift|) / max|scale|).  The host reads the flag once per generate() / forward and raises instead of returning clamped results
       (rerun with DM3D_PREC_F32).  NULL: no check. */
    int32_t* range_flag; float range_limit;
    /* Optional weight image of the Winograd F(2,3)-along-x form of a DM3D_PREC_H3 k3 / stride-1 conv with cout > 32 (dm3d_pack_weights_h3w,
       packed with THIS conv's w_exp): two neighbouring outputs of a row from four transformed inputs — 36 instead of 54 MFMA k-steps per
       output pair, same split-float16 products and float32 accumulation (results differ from the direct form in the last bits only).
       The kernel uses it when the volume is whole 8x8x8 bricks, Cin >= 32, a fused skip conv is short and there are enough bricks (a launch of
       at most 128 of its work items with Cin >= 256 splits Cin two ways: split_counters below); one
       persistent workgroup per CU walks the list of (brick, column tile, Cin part) items
       (dm3d_conv_tile_form() == 10); otherwise wpk serves the launch as before.  The transformed inputs are up to 2 max|x|: producers of
       such a conv must keep |x| <= 32752 (pass range_limit <= 32752 to them).  NULL: never. */
    const void* wpk_wino;
    /* Optional second image of the fused skip conv's kernel (dm3d_pack_weights_skip_h3f, THIS conv's w_exp), beside skip_wpk: with it the
       Winograd-x form also serves launches that carry a skip conv — as a register-direct tail between an item's chunk loop and its
       epilogue (no LDS: such launches are persistent like the others); without it they stay on the direct kernel.  NULL: never. */
    const void* skip_wpk_frag;
    /* Optional: fused GroupNormalization statistics of the OUTPUT tensor: gn_stats[batch][slots][cout][2] float32 = partial (sum, sum of
       squares) per (sample, channel) over the voxels of a slot, slots = ceil(voxels / 64), dm3d_groupnorm_partials_bytes() bytes — the
       input dm3d_groupnorm_finalize2 needs to turn this tensor into a consumer's per-sample scale / shift, without a pass of its own over the
       tensor.  The 16x16x32 kernels' full-brick epilogue stores a wave's sums as the slot of its z-slice while it stores the output (no
       atomics; every slot is written); behind any other kernel or form the library runs dm3d_groupnorm_partials on the finished output
       itself.  Float32 output only (cout % 4 == 0, 16-byte aligned buffer).  NULL: none. */
    float* gn_stats;
    /* Cin split of small grids (DM3D_PREC_H3, DM3D_WL_PAIR).  A conv whose grid would leave most of the chip idle (small batches; the 8^3
       level at B = 32) runs up to 16 workgroups per tile (brick x 64 output channels), each contracting a share of the input channels.  The
       parts meet INSIDE the launch: each stores its raw accumulator tiles into `scratch`, draws a ticket from the tile's word of
       split_counters, and the part that draws the last one sums all parts in part order (results do not depend on timing) and applies the
       epilogue — every epilogue form, no zero fill, no atomic adds on the output, no second launch.  split_counters: at least
       dm3d_conv_split_counter_words(d) int32 words, ZERO before the first launch that uses them; every launch leaves them zero, so one
       buffer serves every conv of a stream.  Without split_counters (NULL / 0) no conv splits; with them a conv that wants to split
       requires scratch of dm3d_conv_scratch_bytes(d) bytes (DM3D_EINVAL otherwise). */
    int32_t* split_counters; int32_t split_counter_words;
} dm3d_conv_desc;

int     dm3d_conv3d_ndhwc(const dm3d_conv_desc* d, void* stream);
int64_t dm3d_conv_scratch_bytes(const dm3d_conv_desc* d);
int32_t dm3d_conv_split_counter_words(const dm3d_conv_desc* d);     /* words of split_counters a descriptor of this shape can use (0: it never splits) */
/* Which tile form of the 16x16x32 conv kernels serves this descriptor: 8 (8 z-slices per brick, 512 threads, one workgroup per CU — launches
 * with enough bricks to give every CU two such workgroups in turn), 4 (4 slices, 256 threads, two workgroups per CU: small grids, the parity
 * form, launches with a fused skip conv, and every k3 / stride-1 conv with Cout <= 32: the narrow column forms NCT 2 and 1), 10 (the Winograd-x
 * form: wpk_wino given and eligible; conv3d_igemm_h3w<MODE>), 0 (another kernel).  The launch and this query read the same resolved decision.  Profiling
 * harnesses use it to name the instantiation a launch runs (rocprofv3 lists conv3d_igemm_h3v3<KS, MODE, TD, NCT> and conv3d_igemm_h3w<MODE>). */
int32_t dm3d_conv_tile_form(const dm3d_conv_desc* d);

/* ---- Dense / einsum contractions: out[b][m][n] = act(alpha * sum_k A[b][m][k]*B[b][n][k] + bias) + res -------
 * Both operands K-contiguous ("TN").  Replaces layers.Dense on the last axis (:131-137, 164-169, 251, 301-304, 313),
 * the 1x1 Conv3D projections of CrossAttentionBlock (:129-130) and the two attention einsums "blc,bLc->blL" /
 * "blL,bLc->blc" (:177-180; U:51-61) as batched calls (stride_* in elements; 0 broadcasts an operand). */
typedef struct dm3d_gemm_desc {
    const float* a; int64_t lda; int64_t stride_a;
    const float* b; int64_t ldb; int64_t stride_b;
    float* out;     int64_t ldo; int64_t stride_o;
    int32_t m, n, k, batch;     /* k % 4 == 0, lda/ldb % 4 == 0 */
    float alpha;
    const float* bias;          /* [n] (or [m] when bias_along_m) or NULL */
    int32_t bias_along_m;
    int32_t act;                /* DM3D_ACT_* applied after bias */
    const float* res; int64_t ldr; int64_t stride_r;   /* added after act, or NULL */
    int32_t precision;          /* DM3D_PREC_F32 (all formats must be DM3D_FMT_F32) or DM3D_PREC_H3 */
    int32_t a_fmt, b_fmt;       /* H3: DM3D_FMT_F32 (split while staging) or DM3D_FMT_H2 (pre-split); k % 16 == 0 */
    int32_t out_fmt;            /* H3: DM3D_FMT_F32 or DM3D_FMT_H2 (n % 16 == 0, ldo % 16 == 0); res is always float32 */
    const float* res2;          /* optional second float32 residual, same ldr / stride_r as res (needs res) */
    int32_t* range_flag; float range_limit;     /* H3 only: as in dm3d_conv_desc */
} dm3d_gemm_desc;

int dm3d_gemm_tn(const dm3d_gemm_desc* d, void* stream);
/* Up to 4 independent DM3D_PREC_H3 contractions with identical operand formats in ONE launch (grid.z enumerates the problems'
 * batches).  The attention blocks' GEMMs are small (m = B*L rows, one workgroup per CU each); issuing the independent ones
 * together (q|k, v^T, q2 and the MLP hidden layer; the two score products; the two P.V products) fills the chip. */
int dm3d_gemm_tn_group(const dm3d_gemm_desc* descs, int32_t count, void* stream);

/* ---- the MLP of a CrossAttentionBlock in one launch (round 4): out = Dense_1(relu(Dense_0(x))) + res + res2
 * (conditional_dm3d.py:132-133 `keras.Sequential([Dense(units * 4, relu), Dense(units)])` applied at :194 with the residual adds of
 * :193-195).  DM3D_PREC_H3 arithmetic; x [m][units] in DM3D_FMT_H2 (ldx in 4-byte elements, a multiple of 16); w0 / w1 = the images
 * dm3d_pack_mlp_weights makes of the DM3D_FMT_H2 matrices [4 units][units] (which = 0) and [units][4 units] (which = 1), same byte size:
 * every (32-row tile, 16-k record, hi | lo) operand fragment contiguous in lane order, so that the kernel streams weights with plain
 * coalesced loads; biases and residuals float32 (16-byte aligned, ldr % 4 == 0); out float32 or DM3D_FMT_H2.  The 4 units-wide hidden
 * activation stays in LDS.  units == 256 only (DM3D_EINVAL otherwise: issue the two dm3d_gemm_tn calls instead). */
int dm3d_pack_mlp_weights(const void* w_h2, int32_t units, int32_t which, void* tiled, void* stream);
typedef struct dm3d_mlp_desc {
    const void* x; int64_t ldx;
    const void* w0; const float* b0;
    const void* w1; const float* b1;
    const float* res; const float* res2; int64_t ldr;      /* optional float32 residuals [m][units] (res2 needs res) */
    void* out; int64_t ldo; int32_t out_fmt;
    int32_t m, units;
    int32_t* range_flag; float range_limit;                /* as in dm3d_gemm_desc */
    /* optional tail (ABI 110): out = relu(W2 . a3 + b2) + res3 with a3 = the result above, which is then NOT stored (out is float32
     * [m][units]) — the block's proj_out and its residual add (conditional_dm3d.py:195).  w2: dm3d_pack_front_weights image of W2[units][units] */
    const void* w2; const float* b2;
    const float* res3; int64_t ldr3;
} dm3d_mlp_desc;
int dm3d_mlp_fused(const dm3d_mlp_desc* d, void* stream);

/* ---- front half of a CrossAttentionBlock in one launch (csrc/dm3d_attn_front_h3.hip; reference networks/conditional_dm3d.py:186-193,
 * 163-170):  y = relu(x . W_in^T + b_in)  (float32 out: the residual of the self-attention pass; an inference BatchNormalization in front
 * is folded into W_in / b_in by the caller),  n_i = LayerNormalization_i(y) for the block's three norms,  q|k = n1 . W_qk^T + b_qk,
 * v^T = (n1 . W_v^T + b_v)^T,  q2 = n2 . W_qk[0:units]^T + b_qk[0:units],  n3 as is — all but y in DM3D_FMT_H2; n1 and n2 never leave
 * the CU.  Replaces dm3d_gemm_tn (proj_in) + dm3d_layernorm3_h2 + a dm3d_gemm_tn_group of three.  units == 256, m % 64 == 0,
 * DM3D_PREC_H3 arithmetic.  Weights are operand-fragment images made once by dm3d_pack_front_weights from the DM3D_FMT_H2 rows
 * W[n][units] (dm3d_split_h2 of the [n][units] float32 weight; n = 256 for w_in / w_v, 512 for w_qk: query rows, then key rows);
 * same byte count as the source. */
typedef struct dm3d_attn_front_desc {
    const float* x; int64_t ldx;                           /* [m][units] float32 */
    const void* w_in; const float* b_in;
    const void* w_qk; const float* b_qk;                   /* b_qk: [2 units] */
    const void* w_v; const float* b_v;
    const float* g1; const float* be1;                     /* LayerNormalization (gamma, beta) of norm1 / norm2 / norm3, [units] each */
    const float* g2; const float* be2;
    const float* g3; const float* be3;
    float eps;
    float* y; int64_t ldy;                                 /* [m][units] float32 */
    void* qk; int64_t ldqk;                                /* DM3D_FMT_H2 [m][2 units] */
    void* vt; int64_t ldvt;                                /* DM3D_FMT_H2 [units][m] */
    void* q2; int64_t ldq2;                                /* DM3D_FMT_H2 [m][units] */
    void* n3; int64_t ldn3;                                /* DM3D_FMT_H2 [m][units] */
    int32_t m, units;
    int32_t* range_flag; float range_limit;                /* as in dm3d_gemm_desc */
} dm3d_attn_front_desc;
int dm3d_pack_front_weights(const void* w_h2, int32_t n, int32_t units, void* tiled, void* stream);
int dm3d_attn_front(const dm3d_attn_front_desc* d, void* stream);

/* dst(H2) = split(src * 2^exp2): one-time conversion of static operands (weights, context keys/values). k % 16 == 0 is
 * not required of src: columns k..round_up(k,16) of dst are zero filled; ld_dst % 16 == 0, ld_dst >= round_up(k,16). */
int dm3d_split_h2(const float* src, int64_t rows, int32_t k, int64_t ld_src, int32_t exp2, void* dst, int64_t ld_dst,
                  void* stream);

/* ---- LayerNormalization (eps passed; Keras default 1e-3) ------------------------------------------------------
 * CrossAttentionBlock normalises the same tensor three times (norm1/2/3, :191-193): one pass computes the row
 * statistics once and writes up to three affine outputs.  c % 4 == 0, c <= 1024. */
int dm3d_layernorm3(const float* x, int64_t rows, int32_t c, float eps,
                    const float* g1, const float* b1, float* o1,
                    const float* g2, const float* b2, float* o2,
                    const float* g3, const float* b3, float* o3, void* stream);
/* same with the outputs written in DM3D_FMT_H2 (c % 16 == 0): they only feed Dense layers */
int dm3d_layernorm3_h2(const float* x, int64_t rows, int32_t c, float eps,
                       const float* g1, const float* b1, void* o1,
                       const float* g2, const float* b2, void* o2,
                       const float* g3, const float* b3, void* o3, void* stream);

/* ---- GroupNormalization(groups, epsilon) statistics (the variant the reference keeps commented out, conditional_dm3d.py:77,
 * 254, 261, 409; keras default epsilon 1e-3).  Per-sample statistics cannot be folded at load time, so two small launches
 * turn a tensor into the per-(sample, channel) scale / shift that the conv prologue (pro_batch_stride = c) or
 * dm3d_affine_act_batched then applies, fused with swish:
 *   dm3d_groupnorm_stats:    acc[b][chan_off + c][0..1] += (sum, sum of squares) of x[b, :, c] in float64 (x [batch, voxels, c];
 *                            call once per concatenated input with its channel offset);  acc must be zero on entry.
 *   dm3d_groupnorm_finalize: group moments from acc (float64), scale[b][c] = gamma[c]*rstd, shift[b][c] = beta[c] - mean*scale;
 *                            acc is zeroed again for the next use. */
int dm3d_groupnorm_stats(const float* x, int32_t batch, int64_t voxels, int32_t c, double* acc, int32_t c_total,
                         int32_t chan_off, void* stream);
int dm3d_groupnorm_finalize(double* acc, int32_t batch, int64_t voxels, int32_t c_total, int32_t groups, float eps,
                            const float* gamma, const float* beta, float* scale, float* shift, void* stream);
/* the same from per-TENSOR partial statistics of up to two concatenated inputs: part [batch][slots][c][2] float32, slots = ceil(voxels / 64),
 * each slot the (sum, sum of squares) of its voxels per channel — what dm3d_conv_desc.gn_stats or dm3d_groupnorm_partials left there.
 * Float64 sums over the slots in a fixed order (no atomics anywhere on this path); nothing is cleared: a tensor with several consumers is
 * summed once.  The slots themselves are float32: the error of scale / shift grows with (|mean| / std)^2 of a group, along the measured curve
 * of DESIGN section 7 (dm3d_groupnorm_stats sums in float64 from the first addition on and has no such curve). */
int64_t dm3d_groupnorm_partials_bytes(int32_t batch, int64_t voxels, int32_t c);
int dm3d_groupnorm_partials(const float* x, int32_t batch, int64_t voxels, int32_t c, float* part, void* stream);
int dm3d_groupnorm_finalize2(const float* part1, int32_t c1, const float* part2, int32_t c2, int32_t batch, int64_t voxels, int32_t groups,
                             float eps, const float* gamma, const float* beta, float* scale, float* shift, void* stream);
/* y[b][r][c] = act(x[b][r][c]*scale[b][c] + shift[b][c]) : dm3d_affine_act with per-sample vectors. c % 4 == 0. */
int dm3d_affine_act_batched(const float* x, float* y, int32_t batch, int64_t rows_per_sample, int32_t c, const float* scale,
                            const float* shift, int32_t act, void* stream);

/* ---- tf.nn.softmax(scores, -1) in place, one wavefront per row (shuffle reductions) (:178; U:56) ------------ */
int dm3d_softmax_rows(float* s, int64_t rows, int32_t cols, int64_t ld, void* stream);
/* same, result left in place in DM3D_FMT_H2 (cols % 16 == 0, ld % 16 == 0; rows longer than 1024 take a three-pass streaming
 * form): it only feeds the P.V contraction */
int dm3d_softmax_rows_h2(float* s, int64_t rows, int32_t cols, int64_t ld, void* stream);

/* ---- single-head attention  out = softmax(q k^T * scale) v (+ res)  per sample (:163-184; U:47-61) in one call: the score
 * product, the row softmax and the P.V product that a host otherwise issues itself, on caller-provided scratch.  L = D*H*W
 * flattened tokens, single head (the reference never uses num_heads > 1).
 *   q   [batch, lq, c]       row stride ldq
 *   k   [batch | 1, lk, c]   row stride ldk; stride_k = 0 broadcasts one context's keys to the whole batch
 *   vt  [batch | 1, c, lk]   the value tensor TRANSPOSED (it is the K-contiguous operand of P.V); row stride ldv, stride_vt
 *   out [batch, lq, c]       row stride ldo; res: optional float32 tensor with out's layout, added to the result
 *   fmt DM3D_FMT_F32 (precision F32 or H3) or DM3D_FMT_H2 (precision H3): format of q, k and vt; out and res are float32.
 *   scratch: >= dm3d_attention_workspace_bytes(batch, lq, lk) bytes, 16-byte aligned (the [batch, lq, lk] probabilities). */
typedef struct dm3d_attention_desc {
    const float* q;  int64_t ldq;
    const float* k;  int64_t ldk; int64_t stride_k;
    const float* vt; int64_t ldv; int64_t stride_vt;
    float* out;      int64_t ldo;
    const float* res;
    int32_t batch, lq, lk, c;
    float scale;                /* units^-0.5 in the reference */
    int32_t precision, fmt;
} dm3d_attention_desc;
int64_t dm3d_attention_workspace_bytes(int32_t batch, int32_t lq, int32_t lk);
int     dm3d_attention(const dm3d_attention_desc* d, void* scratch, void* stream);
/* With DM3D_FMT_H2 operands, c == 256, lq % 128 == 0 and lk % 32 == 0 (the reference's 8^3 attention level: L = 512, units 256) the
 * call above is ONE fused launch: K / V^T stream through LDS in 32-key tiles, the scores and an online softmax (row maximum and sum kept
 * per query, accumulator rescaled when the maximum moves) live in registers, the [batch, lq, lk] probabilities never reach HBM and
 * scratch is not touched (it may be NULL).  Other shapes run as score product + row softmax + P.V on scratch.
 * dm3d_attention_group: up to 4 passes of identical (batch, lq, lk, scale) — the self- and the cross-attention pass of a
 * CrossAttentionBlock — in one grid (the three-launch form, when needed, runs them one after the other on the shared scratch). */
int     dm3d_attention_group(const dm3d_attention_desc* descs, int32_t count, void* scratch, void* stream);

/* ---- y = act(x*scale[c] + shift[c]) over the last axis (inference BatchNormalization of AttentionBlock, U:45;
 * swish of the time embedding, :250); scale/shift may be NULL (identity). */
int dm3d_affine_act(const float* x, float* y, int64_t rows, int32_t c, const float* scale, const float* shift,
                    int32_t act, void* stream);

/* *flag = 1 if any |x[i]| > limit (the H3 range guard for a tensor no dm3d kernel produced, e.g. the caller's x_t). n % 4 == 0. */
int dm3d_range_check(const float* x, int64_t n, float limit, int32_t* flag, void* stream);

/* ---- What "seeded" means: the N(0,1) stream of every entry that draws its own noise ----------------------------------
 * The draws are a function of the key, the element's position and two counter words, and of nothing else: not of the grid, the batch
 * split, the mode, a mask, or a graph replay.  oracle/ref_philox.py restates this block on the host from the Philox paper, and the GPU
 * tests hold every drawing entry to it element by element (tests/philox_cases.py: the bar), so a change to anything below changes every
 * seeded result and is a change of contract.
 *
 * Generator: Philox4x32-10 (Salmon et al., SC'11): multipliers 0xD2511F53 (word 0) and 0xCD9E8D57 (word 2), the key bumped by
 *   (0x9E3779B9, 0xBB67AE85) after each of the ten rounds.
 * Key: (k0, k1) = (seed & 0xffffffff, seed >> 32) of the 64-bit `seed`, or of *seed_dev where that pointer is set (the same 64 bits;
 *   a host that keeps the key in an int64 tensor writes seed - 2^64 for seed >= 2^63).
 * Counter: one block of four words per float4 of output, (i & 0xffffffff, i >> 32, word 2, word 3), where i is the flat float4 index
 *   into the tensor — element / 4 for dm3d_randn, b * (per_sample / 4) + (element of the sample) / 4 for the batched entries — and
 *
 *     entry                                     word 2                                      word 3 (stream constant)
 *     dm3d_randn                                stream_id                                   0x5eed
 *     dm3d_ddpm_update (mode 1, t > 0)          t[b], clamped to [0, timesteps)             0xd1f0
 *     dm3d_ddim_update[_frame]                  tau[r], r = clamp(pos[b])                   0xdd1a
 *     dm3d_dpm_sde_update[_frame]               tau[r], r = clamp(pos[b])                   0x5de2
 *     dm3d_edit_update                          (int32)levels[r][2], r = clamp(pos[b])      0xed17
 *
 *   An element a row or a mask leaves without noise (t == 0, sigma == 0, c_z == 0, a clean level, w == 0) draws nothing and shifts
 *   nobody else's counter.  The host's own dm3d_randn calls use stream_id 0x7fffffff (x_T of a chain) and 0x7ffffffe (training noise).
 * Uniforms, in float32, each operation rounded (the library is built without contraction), from the output words (c0, c1, c2, c3):
 *   u0 = ((float)c0 + 0.5f) * 2^-32, u1 = (float)c1 * 2^-32, u2 = ((float)c2 + 0.5f) * 2^-32, u3 = (float)c3 * 2^-32;
 *   u0 and u2 lie in (0, 1] (never 0; 1 after rounding gives r = 0), u1 and u3 in [0, 1].
 * Box-Muller: r0 = sqrtf(-2 logf(u0)), r1 = sqrtf(-2 logf(u2)), a1 = 6.283185307179586f * u1, a3 = 6.283185307179586f * u3; the four
 *   elements of the float4, in order, are (r0 cos a1, r0 sin a1, r1 cos a3, r1 sin a3).  logf, sqrtf, sinf and cosf are the device
 *   library's: they are not correctly rounded, so the float64 evaluation of these formulas is met to an absolute error on z, not
 *   bitwise (docs/EXPERIMENTS.md records the measured error and the bar). */

/* ---- DDPM posterior step: DiffusionModel.sample + the loop body of generate (:517-548, 571-573) --------------
 * Coefficients are gathered at t[b] and combined in float32 in the reference's order.
 *   mode 0 (sample):   mean_out = posterior mean, var_out[b] = posterior variance (no clip, no noise).
 *   mode 1 (generate): x <- clip(mean,-1,1) + sqrt(max(var,1e-20)) * z, z = noise (if given) or Philox N(0,1)
 *                      keyed by (seed, t[b], element); z = 0 where t[b] == 0. */
typedef struct dm3d_ddpm_desc {
    float* x;                   /* [batch, per_sample] x_t (updated in place in mode 1) */
    const float* eps;           /* predicted noise */
    const float* noise;         /* optional injected z, same shape */
    int32_t batch; int64_t per_sample;     /* per_sample % 4 == 0 */
    const int32_t* t;           /* [batch] device */
    int32_t timesteps;
    const float *beta, *sqrt_alpha, *alpha_bar, *alpha_bar_prev, *sqrt_alpha_bar, *sqrt_alpha_bar_prev,
                *sqrt_one_minus_alpha_bar;     /* [timesteps] device (Betas, :215-235) */
    uint64_t seed;
    int32_t mode;
    float* mean_out; float* var_out;
    const uint64_t* seed_dev;   /* optional: the Philox key is read from device memory instead of `seed`, so one captured step graph
                                   serves every seed (the host rewrites the scalar between chains).  t[b] is clamped to
                                   [0, timesteps) before any table is indexed. */
} dm3d_ddpm_desc;

int dm3d_ddpm_update(const dm3d_ddpm_desc* d, void* stream);

/* ---- DDIM step over a timestep schedule: the strided generalisation of generate's loop body (:517-548, 571-575) ---------
 * Row r = pos[b] of the coefficient table describes one step from timestep tau[r] (alpha_bar a) to a target a' (1 for the
 * last step of a chain):  x0 = (x - sqrt(1-a)*eps) / sqrt(a)          (ddpm_update's float32 order)
 *                         x0 = clip ? clamp(x0, -1, 1) : x0             (a NaN passes)
 *                         res = a_x0*x0 + a_eps*eps + sigma*z           (float32, in that order)
 * with a_x0 = sqrt(a'), a_eps = sqrt(max(1 - a' - sigma^2, 0)), sigma = eta*sqrt((1-a')/(1-a))*sqrt(1 - a/a'), computed by the host
 * in float64 once per chain and rounded once to float32.  One table serves sampling (eta = 0 deterministic, eta > 0 stochastic,
 * eta = 1 strided DDPM) and inversion (a' the next larger timestep's, sigma = 0, no clip).  z = noise (if given) or Philox N(0,1)
 * keyed by (seed, tau[r], element) under a stream constant of its own (never ddpm_update's draws); z = 0 where sigma == 0.
 *   mode 0 (DiffusionModel.ddim_step): out = res, x untouched.
 *   mode 1 (generate / invert):        x <- res.
 * Graph-capturable without host reads: the row comes from device memory (advanced with dm3d_add_i32 after each step), and with t_idx
 * set the kernel writes t_idx[b] = t_next[pos[b]] (the U-Net row of the next step; the kernel does not read t_idx).
 * dm3d_ddim_update_frame takes a frame table beside the descriptor (which stays as it is: x0_bound remains its last member).  With
 * `frame` non-NULL, `eps` holds the network's raw output p in its own frame (v or x0) and row r of the table, (k0x, k0p, kex, kep),
 * replaces the first line and supplies the model's eps:
 *                         x0  = k0x*x + k0p*p                           (float32: mul, mul, add, each rounded; no division)
 *                         eps = kex*x + kep*p                           (likewise)
 * then clip and res as above.  The host writes the rows in float64 from the float32 alpha_bar table, rounded once (schedules.py,
 * frame_table): with a = sqrt(alpha_bar), s = sqrt(1 - alpha_bar), v gives (a, -s, s, a) and x0 gives (0, 1, 1/s, -a/s), both finite
 * at alpha_bar = 0 (the zero-terminal-SNR schedule's last timestep, where the eps frame's 1/a is not).  Columns 0 and 1 of `coef` are
 * not read then.  frame: [rows][4] device, 16-byte aligned, indexed by the same clamped row as `coef`; NULL is dm3d_ddim_update itself
 * (the arithmetic and results of before). */
typedef struct dm3d_ddim_desc {
    float* x;                   /* [batch, per_sample] x at tau[pos[b]] (updated in place in mode 1) */
    const float* eps;           /* predicted noise */
    const float* noise;         /* optional injected z, same shape */
    float* out;                 /* mode 0: the result, same shape */
    int32_t batch; int64_t per_sample;     /* per_sample % 4 == 0 */
    const float* coef;          /* [rows][8] device: sqrt(a), sqrt(1-a), a_x0, a_eps, sigma, clip (nonzero: clamp x0), 0, 0 */
    const int32_t* tau;         /* [rows] device: the timestep each row steps from (the Philox counter) */
    const int32_t* t_next;      /* [rows] device, optional: the timestep the step after row r evaluates */
    int32_t rows;               /* pos[b] is clamped to [0, rows) before any table is indexed */
    const int32_t* pos;         /* [batch] device: the row of each sample */
    int32_t* t_idx;             /* [batch] device, optional: receives t_next[pos[b]] */
    uint64_t seed;
    const uint64_t* seed_dev;   /* optional: the Philox key is read from device memory instead of `seed` (as dm3d_ddpm_desc) */
    int32_t mode;
    const float* x0_bound;      /* optional [batch] device: the dynamic threshold s of dm3d_x0_threshold.  Where the row clips, x0 is
                                   clamp(x0, -s, s) / s (one correctly rounded division; a NaN passes) instead of clamp(x0, -1, 1);
                                   s == 1 is the static clamp bitwise.  NULL (a zeroed descriptor): the static clamp. */
} dm3d_ddim_desc;

int dm3d_ddim_update(const dm3d_ddim_desc* d, void* stream);
int dm3d_ddim_update_frame(const dm3d_ddim_desc* d, const float* frame, void* stream);

/* ---- DPM-Solver++(2M) step over a timestep schedule (Lu et al. 2022, "DPM-Solver++", Algorithm 2) -------------------------------
 * A second-order multistep solver of the sampling ODE in the data-prediction form: one U-Net evaluation per step, as DDIM, plus the
 * x0 estimate of the step before.  With alpha = sqrt(a), sigma = sqrt(1-a), lambda = log(alpha/sigma), a step from level s to level t
 * has h = lambda_t - lambda_s; for a second-order step p is the level the step before started from and r = (lambda_s - lambda_p) / h:
 *   x0  = (x - sigma_s*eps) / alpha_s                   (ddim_update's float32 order)
 *   x0  = clip ? clamp(x0, -1, 1) : x0                  (a NaN passes)
 *   first order:   res = (sigma_t/sigma_s)*x + alpha_t*(1 - exp(-h))*x0                          (DDIM's eta = 0 step where x0 is unclipped)
 *   second order:  res = (sigma_t/sigma_s)*x + alpha_t*(1 - exp(-h))*((1 + 1/(2r))*x0 - (1/(2r))*hist)
 *   to "clean" (a' = 1): res = x0, always first order (r would be 0)
 * The host folds this into one row (c_x, c_0, c_1) per step, in float64 from the float32 alpha_bar table, rounded once to float32:
 *   res = (c_x*x + c_0*x0) + c_1*hist                   (float32, in that order, each operation rounded)
 *   res = c_x*x + c_0*x0                                where c_1 == 0: hist is not read (a first step never sees a stale buffer)
 * and then hist <- x0 (the clipped estimate).  There is no noise term: no Philox stream, no seed.
 *   mode 0 (DiffusionModel.dpm_step): out = res and, with x0_out set, x0_out = x0; x and hist are left untouched (hist may be NULL:
 *                                     every row is then computed as a first-order row).
 *   mode 1 (generate / edit):         x <- res, hist <- x0.
 * Graph-capturable without host reads, as dm3d_ddim_desc: the row comes from device memory and, with t_idx set, the kernel writes
 * t_idx[b] = t_next[pos[b]] (the kernel does not read t_idx).
 * dm3d_dpm_update_frame takes a frame table beside the descriptor, as dm3d_ddim_update_frame (NULL: dm3d_dpm_update itself).  With it,
 * `eps` holds the network's raw output p (v or x0) and x0 = k0x*x + k0p*p (float32: mul, mul, add, each rounded) from
 * row r of the frame table replaces the first line; columns 0 and 1 of `coef` are not read, columns 2 and 3 of the
 * frame row neither (the solver needs no eps).  A row from a level with alpha_bar = 0 is (sigma_t, alpha_t, 0): lambda_s = -inf, h = +inf. */
typedef struct dm3d_dpm_desc {
    float* x;                   /* [batch, per_sample] x at the row's level (updated in place in mode 1) */
    const float* eps;           /* predicted noise */
    float* hist;                /* the x0 estimate of the step before, same shape (mode 1: required, replaced by this step's) */
    float* out;                 /* mode 0: the result, same shape */
    float* x0_out;              /* mode 0, optional: this step's x0 estimate, same shape */
    int32_t batch; int64_t per_sample;     /* batch <= 65535, per_sample % 4 == 0 */
    const float* coef;          /* [rows][8] device: sqrt(a), sqrt(1-a), c_x, c_0, c_1, clip (nonzero: clamp x0), 0, 0 */
    int32_t rows;               /* pos[b] is clamped to [0, rows) before any table is indexed */
    const int32_t* pos;         /* [batch] device: the row of each sample */
    const int32_t* t_next;      /* [rows] device, optional: the timestep the step after row r evaluates */
    int32_t* t_idx;             /* [batch] device, optional: receives t_next[pos[b]] */
    int32_t mode;
    const float* x0_bound;      /* optional [batch] device: the dynamic threshold s, as dm3d_ddim_desc.x0_bound; the thresholded
                                   estimate is what the update uses and what hist / x0_out receive.  NULL: the static clamp. */
} dm3d_dpm_desc;

int dm3d_dpm_update(const dm3d_dpm_desc* d, void* stream);
int dm3d_dpm_update_frame(const dm3d_dpm_desc* d, const float* frame, void* stream);

/* ---- Stochastic DPM-Solver++(2M) step: the SDE form (Lu et al. 2022, "DPM-Solver++", appendix; k-diffusion's dpmpp_2m_sde) -----------
 * dm3d_dpm_update's multistep update of the data-prediction form with one noise term per step.  With alpha, sigma, lambda and
 * h = lambda_t - lambda_s as there and eta >= 0 (1: the paper's solver, 0: the ODE solver dm3d_dpm_update):
 *   c_x = (sigma_t/sigma_s)*exp(-eta*h)      A = alpha_t*(1 - exp(-(1+eta)*h))      c_z = sigma_t*sqrt(1 - exp(-2*eta*h))
 *   first order:   res = c_x*x + A*x0 + c_z*z
 *   second order:  res = c_x*x + A*(1 + g)*x0 - A*g*hist + c_z*z,    g = 1/(2r) = h / (2*(lambda_s - lambda_p))   (the midpoint form)
 *   to "clean" (a' = 1): res = x0, no noise, always first order
 *   from a level with alpha_bar = 0 (h = +inf): res = sigma_t*x + alpha_t*x0 at eta = 0 and alpha_t*x0 + sigma_t*z at eta > 0
 * x0 and its clip are dm3d_dpm_update's.  The host folds a step into one row (c_x, c_0, c_1, c_z), in float64 from the float32
 * alpha_bar table, rounded once to float32 (schedules.py, dpm_sde_coefficients):
 *   res = ((c_x*x + c_0*x0) + c_1*hist) + c_z*z         (float32, in that order, each operation rounded)
 * where c_1 == 0 hist is not read and its add is skipped; where c_z == 0 nothing is drawn, `noise` is not read and the last add is
 * skipped: such a row is dm3d_dpm_update's result bitwise.  Then hist <- x0 (the clipped estimate).  z = noise (if given) or Philox
 * N(0,1) keyed by (seed, tau[r], element) as in dm3d_ddim_update, under a stream constant of this kernel's own (never ddim_update's
 * draws).  Modes, graph capture, t_idx / t_next and x0_bound: as dm3d_dpm_desc.  dm3d_dpm_sde_update_frame takes a frame table beside
 * the descriptor, as dm3d_dpm_update_frame (NULL: dm3d_dpm_sde_update itself). */
typedef struct dm3d_dpm_sde_desc {
    float* x;                   /* [batch, per_sample] x at the row's level (updated in place in mode 1) */
    const float* eps;           /* predicted noise */
    float* hist;                /* the x0 estimate of the step before, same shape (mode 1: required, replaced by this step's) */
    float* out;                 /* mode 0: the result, same shape */
    float* x0_out;              /* mode 0, optional: this step's x0 estimate, same shape */
    int32_t batch; int64_t per_sample;     /* batch <= 65535, per_sample % 4 == 0 */
    const float* coef;          /* [rows][8] device: sqrt(a), sqrt(1-a), c_x, c_0, c_1, clip (nonzero: clamp x0), c_z, 0 */
    int32_t rows;               /* pos[b] is clamped to [0, rows) before any table is indexed */
    const int32_t* pos;         /* [batch] device: the row of each sample */
    const int32_t* t_next;      /* [rows] device, optional: the timestep the step after row r evaluates */
    int32_t* t_idx;             /* [batch] device, optional: receives t_next[pos[b]] */
    int32_t mode;
    const float* x0_bound;      /* optional [batch] device: the dynamic threshold s, as dm3d_dpm_desc.x0_bound.  NULL: the static clamp. */
    const float* noise;         /* optional injected z, same shape as x (read only where the row's c_z != 0) */
    const int32_t* tau;         /* [rows] device, required: the timestep each row steps from (the Philox counter) */
    uint64_t seed;
    const uint64_t* seed_dev;   /* optional: the Philox key is read from device memory instead of `seed` (as dm3d_ddim_desc) */
} dm3d_dpm_sde_desc;

int dm3d_dpm_sde_update(const dm3d_dpm_sde_desc* d, void* stream);
int dm3d_dpm_sde_update_frame(const dm3d_dpm_sde_desc* d, const float* frame, void* stream);

/* ---- UniPC step over a timestep schedule (Zhao et al. 2023, "UniPC"): corrector and predictor in one launch ------------------------
 * The data-prediction, multistep form ("bh1" / "bh2").  After the U-Net has run on the predicted state x at the row's level s, one
 * launch forms the x0 estimate m there (dm3d_dpm_update's: the float32 order, the clamp, x0_bound), corrects the state at s with it
 * (the corrector reuses the evaluation the next step needs anyway) and predicts the state at the next level t from the corrected one.
 * Both updates are linear in their inputs; the host folds each into coefficients, in float64 from the float32 alpha_bar table, rounded
 * once to float32 (schedules.py, unipc_coefficients).  With h0, h1, h2 the x0 estimates of the one, two and three levels before s
 * and xc the corrected state of the level before:
 *   m    = clip ? bounded((x - sigma_s*eps) / alpha_s) : (x - sigma_s*eps) / alpha_s
 *   xc'  = (((k_x*xc + k_0*h0) + k_1*h1) + k_2*h2) + k_t*m       the corrector; k_t == 0: there is none and xc' = x bitwise
 *   res  = ((p_x*xc' + p_0*m) + p_1*h0) + p_2*h1                 the predictor; to "clean" (0, 1, 0, 0): res = m
 * in float32, in that order, each operation rounded.  A term whose coefficient is 0 is skipped and its buffer is not read: k_x for xc,
 * k_0 and p_1 for h0, k_1 and p_2 for h1, k_2 for h2 (dm3d_dpm_update's rule for c_1: stale history and a NaN in it never reach a
 * chain, whose first row has none of these).
 * The history is three slots hist[0..2]; column 7 of the row, rot in {0, 1, 2} (clamped), says which slot plays which role: h0 is
 * hist[(rot+2)%3], h1 hist[(rot+1)%3], h2 hist[rot], and m goes to hist[rot] (a lane reads its 16 bytes of every slot before it
 * stores).  A chain advances rot by one per row, so no host pointer swap happens between replays of a captured step.
 *   mode 0 (DiffusionModel.unipc_step): out = res and, where set, xc_out = xc', x0_out = m; x, xc and hist are left untouched.
 *   mode 1 (generate):                  x <- res, xc <- xc', hist[rot] <- m; xc and all three slots are required.
 * Graph-capturable without host reads, as dm3d_dpm_desc: the row comes from device memory and, with t_idx set, the kernel writes
 * t_idx[b] = t_next[pos[b]] (the kernel does not read t_idx).  There is no noise term and no frame form.
 * Checked before the launch (DM3D_EINVAL): x, eps, coef, corr, pos non-NULL; every tensor and both tables 16-byte aligned; per_sample
 * a positive multiple of 4; batch in [1, 65535]; rows > 0; the mode's required pointers; no two of x, eps, xc, the slots and the outputs
 * sharing a byte. */
typedef struct dm3d_unipc_desc {
    float* x;                   /* [batch, per_sample] the predicted state at the row's level (mode 1: becomes the next level's) */
    const float* eps;           /* predicted noise on x */
    float* xc;                  /* the corrected state of the level before, same shape (mode 1: required, replaced by this level's) */
    float* hist[3];             /* the x0 estimates of the three levels before, same shape each (mode 0: those a row reads; mode 1: all) */
    float* out;                 /* mode 0: the predicted state at the next level, same shape */
    float* xc_out;              /* mode 0, optional: the corrected state at this level */
    float* x0_out;              /* mode 0, optional: this level's x0 estimate */
    int32_t batch; int64_t per_sample;     /* batch <= 65535, per_sample % 4 == 0 */
    const float* coef;          /* [rows][8] device: sqrt(a), sqrt(1-a), p_x, p_0, p_1, clip (nonzero: clamp x0), p_2, rot */
    const float* corr;          /* [rows][8] device: k_x, k_0, k_1, k_2, k_t, 0, 0, 0 */
    int32_t rows;               /* pos[b] is clamped to [0, rows) before any table is indexed */
    const int32_t* pos;         /* [batch] device: the row of each sample */
    const int32_t* t_next;      /* [rows] device, optional: the timestep the step after row r evaluates */
    int32_t* t_idx;             /* [batch] device, optional: receives t_next[pos[b]] */
    int32_t mode;
    const float* x0_bound;      /* optional [batch] device: the dynamic threshold s, as dm3d_dpm_desc.x0_bound.  NULL: the static clamp. */
} dm3d_unipc_desc;

int dm3d_unipc_update(const dm3d_unipc_desc* d, void* stream);

/* ---- Dynamic thresholding of the x0 estimate (Saharia et al. 2022, "Imagen", section 2.3) ------------------------------------------
 * Between the U-Net (or the guidance) and dm3d_ddim_update / dm3d_dpm_update: the bound s the update clamps and divides the x0
 * estimate by, per sample b, from the exact p-quantile of its magnitudes.  With row r = clamp(pos[b], 0, rows-1) of either solver's
 * coefficient table (only columns 0, 1 and 5 are read) and N = per_sample:
 *   x0    = (x - sqrt(1-a)*eps) / sqrt(a)             float32, the update kernels' own device function (mul, sub, div, each rounded)
 *   v_0 <= v_1 <= ... <= v_{N-1}                      the sorted |x0_e|; a NaN sorts last (its bit pattern is above +inf's)
 *   i     = rank[b], f = frac[b]                      the host's q = p*(N-1) in float64, i = floor(q), f = float32(q - i); i is clamped
 *                                                     to [0, N-1], and at i = N-1 v_{i+1} stands for v_i (f is 0 there)
 *   s_raw = v_i + f*(v_{i+1} - v_i)                   float32: sub, mul, add, each rounded
 *   s     = s_raw is NaN ? s_raw : min(max(s_raw, 1), smax[b])
 *   bound[b] = s                                      rows with clip == 0 (column 5): bound[b] = 1, no selection work
 * The update then computes x0 = x0 is NaN ? x0 : clamp(x0, -s, s) / s through its x0_bound field.  Fewer than N-1-i NaNs in a sample
 * reach only their own elements; more make s NaN and with it every element of the sample.
 * v_i and v_{i+1} are exact: an MSB-first radix select over the 31 magnitude bits in three counting passes (12, 10 and 9 bits) that
 * carry both ranks.  The counts are integers summed with atomics, whose result does not depend on the order of arrival, and nothing
 * else is shared between blocks: runs repeat bitwise.  Graph-capturable without host reads: rank, frac and smax are device tables (one
 * captured graph serves every ratio and cap), and every launch clears its own counters (a kernel) before it counts.
 * scratch: dm3d_x0_threshold_scratch_bytes(batch, per_sample) bytes, 16-byte aligned; contents need not survive between launches.
 * With `frame` set (the update's own table), `eps` holds the raw prediction p and x0 = k0x*x + k0p*p with the update kernels' device
 * function (mul, mul, add, each rounded): the magnitudes ranked stay bitwise the values clamped.  Only column 5 of `coef` is read then. */
typedef struct dm3d_thresh_desc {
    const float* x;             /* [batch, per_sample] x at the row's level */
    const float* eps;           /* predicted noise (a guided chain: the guided one) */
    int32_t batch; int64_t per_sample;     /* batch <= 65535, per_sample % 4 == 0, per_sample < 2^31 */
    const float* coef;          /* [rows][8] device: either update descriptor's table: sqrt(a), sqrt(1-a), ..., clip in column 5 */
    int32_t rows;               /* pos[b] is clamped to [0, rows) before the table is indexed */
    const int32_t* pos;         /* [batch] device: the row of each sample */
    const int32_t* rank;        /* [batch] device: i */
    const float* frac;          /* [batch] device: f in [0, 1) */
    const float* smax;          /* [batch] device: the cap on s, >= 1 */
    float* bound;               /* [batch] device, out: s */
    void* scratch;              /* device: histograms, select states and the stashed magnitudes */
    const float* frame;         /* optional [rows][4] device, 16-byte aligned: the table of dm3d_ddim_update_frame.  NULL (a zeroed
                                   descriptor): `eps` is eps, the arithmetic and results of before. */
} dm3d_thresh_desc;

int64_t dm3d_x0_threshold_scratch_bytes(int32_t batch, int64_t per_sample);
int dm3d_x0_threshold(const dm3d_thresh_desc* d, void* stream);

/* ---- Known-latent step of inpainting / image-to-image editing (RePaint's replacement step, SDEdit's start) -------------
 * Row r = clamp(pos[b], 0, rows-1) of the level table gives a target level a' (alpha_bar of a timestep, 1 for "clean"):
 *   known_t = sqrt(a')*x0 + sqrt(1-a')*z            (float32, in that order: conditional_dm3d.py:484-491's q_sample)
 *   known_t = x0 (bitwise) where sqrt(1-a') == 0    (clean: z is not drawn)
 *   mode 0 (q_sample):  out = known_t; x and w are not read.
 *   mode 1 (blend):     x <- w*known_t + (1-w)*x    (float32, in that order) for 0 < w < 1, with w = w[b][e / channels] the keep
 *                        weight of element e's voxel; w == 0 leaves x bitwise untouched (x0, z are not read), w == 1 writes
 *                        known_t bitwise.
 * z = noise (if given) or Philox N(0,1) keyed by (seed, the row's level timestep, element) under a stream constant of its own
 * (never randn's, ddpm_update's or ddim_update's draws).  The host computes a' in float64 from the float32 alpha_bar table and
 * rounds sqrt(a') and sqrt(1-a') once to float32.  Graph-capturable without host reads, as dm3d_ddim_desc: in a DDPM chain the
 * blend runs after dm3d_ddpm_update and before the dm3d_add_i32 decrement with pos = t_idx (row t holds level t-1, row 0 clean);
 * in a DDIM chain after dm3d_ddim_update with pos = its row counter (row r holds that step's target, row 0 clean). */
typedef struct dm3d_edit_desc {
    float* x;                   /* mode 1: [batch, per_sample] the chain's state, updated in place */
    const float* x0;            /* [batch, per_sample] the known latent */
    const float* w;             /* mode 1: [batch, per_sample / channels] keep weight per voxel in [0, 1] */
    const float* noise;         /* optional injected z, x0's shape */
    float* out;                 /* mode 0: the result, x0's shape */
    int32_t batch; int64_t per_sample;     /* batch <= 65535, per_sample % 4 == 0 */
    int32_t channels;           /* innermost extent the weight is broadcast over; divides per_sample */
    const float* levels;        /* [rows][4] device: sqrt(a'), sqrt(1-a'), the level's timestep (the Philox counter, -1 clean), 0 */
    int32_t rows;
    const int32_t* pos;         /* [batch] device: the row of each sample */
    uint64_t seed;
    const uint64_t* seed_dev;   /* optional: the Philox key is read from device memory instead of `seed` (as dm3d_ddpm_desc) */
    int32_t mode;
} dm3d_edit_desc;

int dm3d_edit_update(const dm3d_edit_desc* d, void* stream);

/* ---- Classifier-free guidance (Ho and Salimans 2022) with the guidance rescale of Lin et al. 2023, section 3.4 ---------------
 * Between the U-Net and the update of a guided chain, whose plan holds batch "positive" rows followed by batch "negative" rows:
 *   eps_g   = eps_neg + w*(eps_pos - eps_neg)          float32, in that order: sub, mul, add, each rounded
 *   eps_g   = eps_pos bitwise where w == 1, eps_neg bitwise where w == 0 (the other operand is not read, unless the row's statistics
 *             below need eps_pos)
 *   f       = phi*std(eps_pos)/std(eps_g) + (1 - phi)  per sample; std is the population standard deviation (divide by per_sample; the
 *             ratio is the unbiased estimator's too) over all per_sample elements, from float64 sums of the values and of their
 *             squares; f is computed in float64 and rounded once to float32; std(eps_g) == 0 gives f = 1
 *   eps_out = f*eps_g                                   only where phi != 0; phi == 0 leaves eps_g bitwise
 * w = scale[b] and phi = rescale[b] are read from device memory, so one captured step graph serves every scale and rescale.
 *   mode 0 (combine): out = eps_g.  out may be eps_pos (in place: a row with w == 1 is then not touched at all), never eps_neg.
 *                     With partials set, each block of a row with phi != 0 also leaves its float64 partial sums (sum and sum of
 *                     squares of eps_pos and of eps_g) there; rows with phi == 0 leave theirs unwritten.
 *   mode 1 (rescale): out <- f*out for the rows with phi != 0, f from the partials mode 0 left (same batch and per_sample); rows with
 *                     phi == 0 are not touched.  A host that knows every phi to be 0 need not launch it.
 *   mode 2 (mirror):  x[batch + b] <- x[b] and, with t_idx set, t_idx[batch + b] <- t_idx[b] for b < batch: the second half of the
 *                     plan takes over the state the update left in the first.
 * The sums are reduced in a fixed order (lanes by shuffles, waves and blocks in index order, no atomics): runs repeat bitwise.
 * A NaN in eps_pos or eps_neg reaches that element of eps_g, and with phi != 0 every element of that sample. */
#define DM3D_GUIDE_PARTIAL_BLOCKS 256      /* partials holds [batch][DM3D_GUIDE_PARTIAL_BLOCKS][4] doubles */
typedef struct dm3d_guide_desc {
    const float* eps_pos;       /* mode 0: [batch, per_sample] prediction under the wanted context */
    const float* eps_neg;       /* mode 0: the same under the negative context */
    float* out;                 /* modes 0, 1: [batch, per_sample] */
    int32_t batch; int64_t per_sample;     /* batch <= 65535, per_sample % 4 == 0 */
    const float* scale;         /* mode 0: [batch] device, w */
    const float* rescale;       /* mode 0: optional (NULL: every phi is 0); mode 1: required.  [batch] device, phi in [0, 1] */
    double* partials;           /* mode 0: optional; mode 1: required.  [batch][256][4] device scratch */
    float* x;                   /* mode 2: [2*batch, per_sample] */
    int32_t* t_idx;             /* mode 2: optional [2*batch] device */
    int32_t mode;
} dm3d_guide_desc;

int dm3d_guide_update(const dm3d_guide_desc* d, void* stream);

/* ---- What the network predicts: eps, v (Salimans & Ho 2022) or x0; min-SNR-gamma loss weighting (Hang et al. 2023) ----------------
 * The solvers above read the network output as eps.  A model trained to predict v = sqrt(a)*z - sqrt(1-a)*x0 or x0 itself (a =
 * alpha_bar[t], x_t = sqrt(a)*x0 + sqrt(1-a)*z) is brought into that frame between the U-Net and the guidance of a step:
 *   eps = c_p*pred + c_x*x          float32, in that order: mul, mul, add, each rounded;  (c_p, c_x) = table[clamp(t_idx[b], 0, timesteps-1)]
 *   v:  (sqrt(a), sqrt(1-a))        x0: (-sqrt(a)/sqrt(1-a), 1/sqrt(1-a))        eps: (1, 0)   (the host computes the table in float64
 *                                   from the float32 alpha_bar and rounds once)
 * It writes over pred, or to out when out is given; out may be pred or x themselves (a lane reads its own 16 bytes of both before it
 * stores) or apart from both.  One HBM stream of 12 B per element, 16 B per lane.  Checked before the launch (DM3D_EINVAL): pred, x,
 * table, t_idx non-NULL; pred, x, out 16-byte aligned; per_sample a positive multiple of 4; batch in [1, 65535]; timesteps > 0; out
 * not overlapping pred or x partially (nor, in place, pred overlapping x partially).
 * Known price of converting rather than teaching the update kernels x0: at a = 4e-5 (t = T-1 of T = 1000) the round trip
 * v -> eps -> x0 loses about 6e-8*|x|/sqrt(a) = 1e-5 absolute in x0 (an estimate from the roundings, not a measurement). */
typedef struct dm3d_pred_desc {
    float* pred;                /* [batch, per_sample] the network's output; becomes eps when out is NULL */
    const float* x;             /* [batch, per_sample] x_t, the state the network was evaluated on */
    float* out;                 /* optional [batch, per_sample]: eps goes here and pred is left as it is */
    const float* table;         /* [timesteps][2] device, (c_p, c_x) per timestep */
    const int32_t* t_idx;       /* [batch] device, the evaluated timestep of each row */
    int32_t batch; int64_t per_sample;     /* batch <= 65535, per_sample % 4 == 0 */
    int32_t timesteps;
} dm3d_pred_desc;
int dm3d_pred_to_eps(const dm3d_pred_desc* d, void* stream);

/* The training loss of a prediction against its target, per sample b with coef[b] = (a_z, a_0, w, 0):
 *   target = a_z*noise + a_0*x0     float32: mul, mul, add       (eps: (1, 0); v: (sqrt(a), -sqrt(1-a)); x0: (0, 1))
 *   d      = pred - target          float32
 *   dpred  = d * (float)(2*inv_divisor*w)                         (NULL: not wanted)
 *   loss_rows[b] = w*inv_divisor*sum d^2  (float64),  loss[0] = sum_b loss_rows[b]     (both written, not accumulated into)
 * w is the loss weight of the sample (1, or min-SNR-gamma's: min(SNR, gamma)/SNR for eps, /(SNR+1) for v, min(SNR, gamma) for x0).
 * The grid is (min(ceil(per_sample/4/256), DM3D_LOSS_PARTIAL_BLOCKS), batch); every block leaves its float64 sum of d^2 in
 * partials[b][block], and a second launch of one block inside this entry adds each sample's partials, then the samples, in index order:
 * no atomics, so the loss repeats bitwise (dm3d_mse_loss_grad's does not).  With coef = (1, 0, 1) dpred is bitwise dm3d_mse_loss_grad's.
 * Checked before the launch (DM3D_EINVAL): every pointer but dpred non-NULL; pred, noise, x0, dpred, coef 16-byte aligned and the
 * float64 buffers 8-byte aligned; per_sample a positive multiple of 4; batch in [1, 65535]; inv_divisor finite; dpred apart from
 * pred, noise and x0. */
#define DM3D_LOSS_PARTIAL_BLOCKS 64        /* partials holds [batch][DM3D_LOSS_PARTIAL_BLOCKS] doubles */
typedef struct dm3d_loss_desc {
    const float* pred;          /* [batch, per_sample] */
    const float* noise;         /* [batch, per_sample] z of q_sample */
    const float* x0;            /* [batch, per_sample] the clean latents */
    const float* coef;          /* [batch][4] device */
    float* dpred;               /* optional [batch, per_sample] */
    double* partials;           /* [batch][64] device scratch */
    double* loss_rows;          /* [batch] device */
    double* loss;               /* [1] device */
    int32_t batch; int64_t per_sample;     /* batch <= 65535, per_sample % 4 == 0 */
    double inv_divisor;
} dm3d_loss_desc;
int dm3d_objective_loss_grad(const dm3d_loss_desc* d, void* stream);

/* ---- Autoencoder evaluation (VQVAE.test_step, vqvae3d_monai.py:504-544; VQGAN.test_step, vqgan.py:821-919): how well y reconstructs x.
 * x (the truth) and y (the reconstruction) are NDHWC float32 [batch, d, h, w, cx] and [batch, d, h, w, cy]; the nc channels x0c.. of x
 * are compared with the nc channels y0c.. of y, read in place (the image half of a 2-channel reconstruction needs no split copy).
 * Every depth slice (b, z) is one 2-D image of nc channels, as tf.image.ssim / tf.image.psnr see a volume [d, h, w, c].  Everything
 * stays on the device: no entry reads back or synchronises.  Sums are float64 in a fixed order (a block by the tree every fixed-order
 * reduction here shares, blocks through `partials` in block order by a second launch, no atomics): runs repeat bitwise.
 *
 * dm3d_pair_stats   one streaming pass, grid (P, d, batch) with P = min(ceil(h*w / 4096), DM3D_PAIR_PARTIAL_BLOCKS):
 *     sse[b*d + z]  = sum over h, w, nc of ((double)x - (double)y)^2          (a float32 difference is exact in float64)
 *     y_min[b], y_max[b] = min / max of the compared channels of y over the volume (exact, order-free: bitwise), and
 *     y_range[b] = y_max[b] - y_min[b] (float32; NULL: not wanted), the max_val the reference hands to both metrics.
 *   With d = h = 1 and w = the flattened extent the same entry gives the quantizer's sum (q - z)^2.  A NaN in y is skipped by min and
 *   max (fminf / fmaxf) and reaches sse.  partials: 3 * batch * d * P doubles.
 *
 * dm3d_ssim   tf.image.ssim with its defaults (11 x 11 Gaussian window of sigma 1.5, k1 0.01, k2 0.03), one value per slice:
 *     g[i] = exp(-(i - 5)^2 / 4.5) / sum, rounded to float32; the window is g (x) g, applied separably, VALID: (h - 10) x (w - 10) outputs
 *     L = max_val[b];  c1 = (0.01f L)^2;  c2 = (0.03f L)^2
 *     mx = F(x), my = F(y), sxy = F(x*y), sq = F(x*x + y*y)       float32; F: the row pass, then the column pass, each
 *                                                                  acc = fma(g[i], v[i], acc) from acc = 0 for i = 0..10
 *     n0 = (mx*my)*2;  d0 = mx*mx + my*my;  lum = (n0 + c1) / (d0 + c1);  cs = ((sxy*2 - n0) + c2) / ((sq - d0) + c2)
 *     out[b*d + z] = (float)(mean over channels of (sum over outputs of (double)(lum*cs)) / ((h - 10)(w - 10)))
 *   A workgroup owns a DM3D_SSIM_TILE^2 tile of outputs of one (b, z, channel): it stages the (TILE + 10)^2 halo of x and y in LDS once,
 *   runs the row pass into LDS, the column pass in registers, and leaves one float64 partial; a second launch adds each slice's
 *   partials in (channel, tile) order.  partials: batch * d * nc * ceil((h-10)/TILE) * ceil((w-10)/TILE) doubles.
 *   max_val[b] = 0 (a constant y under the reference's choice) yields what the formula yields, 0/0 = NaN, as TensorFlow does.
 *
 * dm3d_psnr_finalize   tf.image.psnr from dm3d_pair_stats' sse:  mse = (float)(sse / (h*w*nc));
 *     out[b*d + z] = (float)(20 log10 L) - (float)(10 log10 mse)   with L = max_val[b]: each term rounded to float32 once, one float32
 *   subtraction.  mse = 0 gives +inf.
 *
 * Checked before any launch (DM3D_EINVAL): the descriptor and every pointer the entry reads or writes non-NULL (y_range may be NULL);
 * batch, d in [1, 65535], h, w >= 1 (dm3d_ssim: >= 11); nc >= 1, x0c >= 0, y0c >= 0, x0c + nc <= cx, y0c + nc <= cy;
 * partials_elems at least what the entry needs; float64 buffers 8-byte aligned. */
#define DM3D_PAIR_PARTIAL_BLOCKS 64
#define DM3D_SSIM_TILE 32
typedef struct dm3d_metric_desc {
    const float* x;             /* [batch, d, h, w, cx] the truth */
    const float* y;             /* [batch, d, h, w, cy] the reconstruction */
    int32_t batch, d, h, w;
    int32_t cx, cy;             /* channel counts of the two tensors */
    int32_t x0c, y0c;           /* first channel read of each */
    int32_t nc;                 /* channels compared */
    double* partials;           /* device scratch, written before it is read by every call */
    int64_t partials_elems;     /* doubles it holds */
    float* y_min;               /* [batch]      pair_stats: out */
    float* y_max;               /* [batch]      pair_stats: out */
    float* y_range;             /* [batch]      pair_stats: out, optional */
    double* sse;                /* [batch * d]  pair_stats: out; psnr_finalize: in */
    const float* max_val;       /* [batch]      ssim, psnr_finalize: in */
    float* out;                 /* [batch * d]  ssim, psnr_finalize: out */
} dm3d_metric_desc;
int dm3d_pair_stats(const dm3d_metric_desc* d, void* stream);
int dm3d_ssim(const dm3d_metric_desc* d, void* stream);
int dm3d_psnr_finalize(const dm3d_metric_desc* d, void* stream);

/* ---- 3-D multi-scale SSIM (Wang, Simoncelli, Bovik 2003, with a 3-D window): a fidelity score of a reconstruction against its truth
 * and, over the pairs of a generated batch, a diversity score.  x is [nx, d, h, w, cx] and y [ny, d, h, w, cy], NDHWC float32; the nc
 * channels x0c.. of x are compared with the nc channels y0c.. of y, read in place.  Output row p compares volume x_index[p] of x with
 * volume y_index[p] of y (a NULL table is the identity p, and then pairs <= nx resp. ny); a table entry outside [0, nx) resp. [0, ny)
 * reads nothing and makes out[p] NaN.  max_val and out are indexed by p.  Nothing is read back; runs repeat bitwise.
 *
 *     g[i] = exp(-(i - (F-1)/2)^2 / (2 sigma^2)) / sum, i = 0..F-1, F = filter_size: float64, rounded to float32.  The window is
 *     g (x) g (x) g, applied separably along w, then h, then d, no padding: each pass acc = fma(g[i], v[i], acc) from acc = 0, i ascending.
 *     Scale j = 0..scales-1 has edges (d >> j, h >> j, w >> j) and a valid map of (edge - (F-1)) points per axis.
 *     L = max_val[p] at every scale;  c1 = (0.01f L)^2;  c2 = (0.03f L)^2
 *     mx = W(x), my = W(y), sxy = W(x*y), sq = W(x*x + y*y);  n0 = (mx*my)*2;  d0 = mx*mx + my*my          all float32
 *     lum = (n0 + c1) / (d0 + c1);  cs = ((sxy*2 - n0) + c2) / ((sq - d0) + c2)
 *     CS_j = (sum over the valid map of (double)cs) / points;  S_j = (sum of (double)(lum*cs)) / points        per channel
 *     between scales x and y become their 2 x 2 x 2 means, an odd edge dropping its last plane: the eight values added in float32 in
 *     (dz, dy, dx) index order, times 0.125f
 *     out[p] = (float)(mean over channels of  prod_{j < scales-1} max(CS_j, 0)^w_j  *  max(S_{scales-1}, 0)^w_{scales-1}),
 *     w = power_factors (float32 values), the product and pow() in float64, scales in ascending order.
 *
 * One launch per scale: a workgroup owns DM3D_MSSSIM_TD x TH x TW points of the valid map of one (p, channel), walks the input planes
 * along d (each staged in LDS once, w pass into LDS, h pass in registers, d pass as a register delay line) and leaves one float64 pair
 * (sum cs, sum lum*cs).  Between scales one pooling launch per tensor writes every volume's compared channels to `scratch`; a final
 * launch combines tiles, scales, powers and channels in index order.
 *     tiles_j          = ceil(od/TD) * ceil(oh/TH) * ceil(ow/TW)  with  (od, oh, ow) = ((d >> j) - (F-1), (h >> j) - (F-1), (w >> j) - (F-1))
 *     partials_elems  >= 2 * pairs * nc * sum_{j < scales} tiles_j                                   doubles, 8-byte aligned
 *     scratch_elems   >= (nx + ny) * nc * sum_{1 <= j < scales} (d >> j)(h >> j)(w >> j)            floats (scales = 1: none, may be NULL)
 *
 * Checked before any launch (DM3D_EINVAL, the message starts "ms_ssim:"): the descriptor, x, y, max_val, out, partials (and scratch
 * when scales > 1) non-NULL; pairs in [1, 65535] and, for a NULL table, at most the volumes of that tensor; nx, ny, d, h, w, nc >= 1;
 * filter_size odd in [3, 11]; filter_sigma > 0; scales in [1, 5]; power_factors[j] > 0 for j < scales; x0c, y0c >= 0,
 * x0c + nc <= cx, y0c + nc <= cy; min(d, h, w) >> (scales - 1) >= filter_size (the message names the largest number of scales that
 * fits); both buffer sizes; the alignment of partials.
 * Not offered: the 2-D tf.image.ssim_multiscale form, other pooling rules, uniform windows. */
#define DM3D_MSSSIM_TD 32
#define DM3D_MSSSIM_TH 16
#define DM3D_MSSSIM_TW 32
typedef struct dm3d_ms_ssim_desc {
    const float* x;             /* [nx, d, h, w, cx] */
    const float* y;             /* [ny, d, h, w, cy] */
    const int32_t* x_index;     /* [pairs] device, optional: the volume of x row p reads */
    const int32_t* y_index;     /* [pairs] device, optional: the volume of y row p reads */
    int32_t pairs;              /* P: rows of out */
    int32_t nx, ny;             /* volumes in x and in y */
    int32_t d, h, w;
    int32_t cx, cy;             /* channel counts of the two tensors */
    int32_t x0c, y0c;           /* first channel read of each */
    int32_t nc;                 /* channels compared */
    int32_t filter_size;        /* F: odd, 3..11 */
    float filter_sigma;
    int32_t scales;             /* M: 1..5 */
    float power_factors[5];     /* w_j, j < scales */
    const float* max_val;       /* [pairs] */
    float* out;                 /* [pairs] */
    double* partials;           /* device scratch, written before it is read by every call */
    int64_t partials_elems;     /* doubles it holds */
    float* scratch;             /* device scratch for the pooled volumes */
    int64_t scratch_elems;      /* floats it holds */
} dm3d_ms_ssim_desc;
int dm3d_ms_ssim(const dm3d_ms_ssim_desc* d, void* stream);

/* ---- Scores of the mask channels: overlap (Dice, IoU) and surface distances (Hausdorff, its percentile, ASSD) of binarised masks, by
 * MONAI's definitions, through an exact 3-D squared Euclidean distance transform.  x (the truth) is [batch, d, h, w, cx] and y
 * [batch, d, h, w, cy], NDHWC float32; the nc channels x0c.. of x are compared with the nc channels y0c.. of y, read in place.
 * Everything the entries write that has a voxel axis is channel-planar, [batch, nc, d, h, w], so that every column of the transform
 * is a strided run of one volume.  Distances are in voxels: anisotropic spacing is not offered, the caller scales.  Nothing is read
 * back.  Every quantity before the last kernel is an integer (integer atomics, min-plus over int32), the last kernel forms its float64
 * values in a fixed order: runs repeat bitwise.
 *
 *     mask        m = value > threshold (NaN is background), per volume and channel
 *     counts      counts[(b * nc + c) * 3 + {0, 1, 2}] = |X|, |Y|, |X and Y|                                               int64, exact
 *     surface     a mask voxel with one of its 6 face neighbours in the background or outside the volume                 uint8 0 / 1
 *     map         map[v] = min over feature voxels s of |v - s|^2 = dz^2 + dy^2 + dx^2; INT32_MAX everywhere without a feature   int32, exact
 *
 * dm3d_mask_overlap   one pass over both tensors: counts, and (surf_x and surf_y both non-NULL) the two surface masks.
 * dm3d_edt            map of x's surface (of = DM3D_EDT_SURFACE) or of its mask (DM3D_EDT_FOREGROUND; 0 inside it): y, cy, y0c are not
 *     read.  One pass writes the features to `masks`; then out[i] = min_j (i - j)^2 + g[j] along w (g = 0 at a feature, "none"
 *     elsewhere), along h and along d, in place in `map`: a workgroup stages DM3D_EDT_LANES neighbouring columns in LDS
 *     ([n][DM3D_EDT_LANES + 1] int32, twice: the columns and the results) and evaluates the form branch-free, O(n^2) per column.
 *     The staging is the line-pass tiler of csrc/dm3d_volume.h, shared with dm3d_spline_filter.
 *         masks_elems >= batch * nc * d * h * w                                   bytes
 * dm3d_surface_distance   the overlap pass (counts if non-NULL), the map of Y's surface, a histogram of its values at X's surface voxels,
 *     the same with X and Y exchanged, and one kernel that reads the two histograms of a (volume, channel):
 *         out[(b * nc + c) * 5 + {0..4}] = hd, hd_percentile, assd, |S_X|, |S_Y|                                           float64
 *         per direction: n voxels, max = sqrt(largest k), sum = sum_k count[k] sqrt(k) (256 runs of ascending k, added in ascending
 *         order), percentile = numpy's default (linear) rule on the sorted distances: r = (n - 1) * (percentile / 100), lo = floor(r),
 *         t = r - lo, a = sqrt(k at rank lo), b = sqrt(k at rank min(lo + 1, n - 1)), a + (b - a) t for t < 0.5, else b - (b - a)(1 - t)
 *         hd = the larger max, hd_percentile = the larger percentile, assd = (sum_0 + sum_1) / (n_0 + n_1); all three NaN when
 *         either surface is empty.
 *         bins         = (d-1)^2 + (h-1)^2 + (w-1)^2 + 1
 *         masks_elems >= 2 * batch * nc * d * h * w                               bytes
 *         work_elems  >= batch * nc * (d * h * w + 2 * (bins + 1))                int32, 4-byte aligned
 *
 * Checked before any launch (DM3D_EINVAL; the message starts "mask_overlap:", "edt:" or "surface_distance:"): the descriptor and every
 * pointer the entry reads or writes non-NULL (counts is optional for dm3d_surface_distance; surf_x and surf_y are given or omitted
 * together); batch, nc >= 1 and batch * nc <= 65535; d, h, w in [1, DM3D_EDT_MAX_EXTENT], a larger extent named as such; x0c >= 0,
 * x0c + nc <= cx (and y's window where y is read); threshold finite; of one of the two constants; percentile in (0, 100]; both scratch
 * sizes; int64 / float64 buffers 8-byte aligned, int32 buffers 4-byte aligned. */
#define DM3D_EDT_MAX_EXTENT 512
#define DM3D_EDT_LANES 32
#define DM3D_EDT_SURFACE 0
#define DM3D_EDT_FOREGROUND 1
typedef struct dm3d_mask_desc {
    const float* x;             /* [batch, d, h, w, cx] the truth */
    const float* y;             /* [batch, d, h, w, cy] the reconstruction (dm3d_edt: not read) */
    int32_t batch, d, h, w;
    int32_t cx, cy;             /* channel counts of the two tensors */
    int32_t x0c, y0c;           /* first channel read of each */
    int32_t nc;                 /* channels compared */
    float threshold;
    int32_t of;                 /* dm3d_edt: DM3D_EDT_SURFACE or DM3D_EDT_FOREGROUND */
    double percentile;          /* dm3d_surface_distance: in (0, 100] */
    int64_t* counts;            /* [batch, nc, 3]        mask_overlap: out; surface_distance: out, optional */
    uint8_t* surf_x;            /* [batch, nc, d, h, w]  mask_overlap: out, optional */
    uint8_t* surf_y;            /* [batch, nc, d, h, w]  mask_overlap: out, optional */
    int32_t* map;               /* [batch, nc, d, h, w]  edt: out */
    double* out;                /* [batch, nc, 5]        surface_distance: out */
    uint8_t* masks;             /* device scratch of edt and surface_distance */
    int64_t masks_elems;        /* bytes it holds */
    int32_t* work;              /* device scratch of surface_distance */
    int64_t work_elems;         /* int32 it holds */
} dm3d_mask_desc;
int dm3d_mask_overlap(const dm3d_mask_desc* d, void* stream);
int dm3d_edt(const dm3d_mask_desc* d, void* stream);
int dm3d_surface_distance(const dm3d_mask_desc* d, void* stream);

/* ---- Connected components of the mask channels: labels, count, largest, and the filters built on them (MONAI's
 * KeepLargestConnectedComponent, RemoveSmallObjects and FillHoles).  x is [batch, d, h, w, cx] NDHWC float32; the nc channels x0c.. are
 * read in place.  labels is channel-planar, [batch, nc, d, h, w]; out is NDHWC with nc channels.  Nothing is read back, every quantity
 * is an integer and the result does not depend on the order anything happened in: runs repeat bitwise.
 *
 *     mask          m = value > threshold (NaN is background), per volume and channel
 *     connectivity  6, 18 or 26: voxels are neighbours when they differ by at most 1 on every axis and on at most 1, 2 or 3 axes;
 *                   nothing connects across volumes, channels or round the border
 *     labels        0 at the background; a component's label is 1 + the rank of its smallest raster index (z * h + y) * w + x among the
 *                   components of its (volume, channel): scipy.ndimage.label's numbering                                     int32
 *     count         count[b * nc + c] components                                                                             int32
 *     largest       largest[(b * nc + c) * 2 + {0, 1}] = label, size of the component with the most voxels, the lowest label on a
 *                   tie, (0, 0) for an empty mask                                                                            int64
 *
 * dm3d_components        labels, count and largest.  A workgroup labels one 8 x 8 x 64 (d, h, w) brick by union-find in LDS; voxels on
 *     brick faces are united across the seams by device-scope atomic min on the larger root; one pass replaces every parent by its
 *     root and adds the brick pieces' sizes at the roots; the roots are counted per block of DM3D_CCL_BLOCK_VOXELS voxels, the block
 *     counts scanned by one workgroup per (volume, channel), and the roots' ranks written back through them.
 *         work_elems >= 2 * batch * nc * d * h * w + 1 + batch * nc * (3 * nblk + 2)      int32, 8-byte aligned
 * dm3d_component_filter  out = 1.0f at the voxels a mode keeps, 0.0f elsewhere:
 *     DM3D_CCL_LARGEST      the voxels of `largest`'s component; an empty mask stays empty
 *     DM3D_CCL_MIN_SIZE     the voxels of every component with at least min_size voxels
 *     DM3D_CCL_FILL_HOLES   the mask and every background voxel whose 6-connected background component touches no face of the volume
 *                           (scipy.ndimage.binary_fill_holes, default structure); `connectivity` is checked and not used
 *         work_elems >= 3 * batch * nc * d * h * w + 1 + batch * nc * (3 * nblk + 2)      int32, 8-byte aligned
 *         nblk        = ceil(d * h * w / DM3D_CCL_BLOCK_VOXELS)
 *
 * Checked before any launch (DM3D_EINVAL; the message starts "components:" or "component_filter:"): the descriptor and every pointer
 * the entry uses non-NULL; x, labels, count, out 4-byte and largest, work 8-byte aligned; batch, nc >= 1 and batch * nc <= 65535; d, h,
 * w in [1, DM3D_CCL_MAX_EXTENT], a larger extent named as such (at 512^3 an index still fits int32 beside the background sentinel and
 * the flag bits of a size word); x0c >= 0, x0c + nc <= cx; threshold finite; connectivity 6, 18 or 26; a known mode; min_size >= 1 for
 * DM3D_CCL_MIN_SIZE; the scratch size; labels and out share no byte with x. */
#define DM3D_CCL_MAX_EXTENT 512
#define DM3D_CCL_BLOCK_VOXELS 1024
#define DM3D_CCL_LARGEST 0
#define DM3D_CCL_MIN_SIZE 1
#define DM3D_CCL_FILL_HOLES 2
typedef struct dm3d_ccl_desc {
    const float* x;             /* [batch, d, h, w, cx] */
    int32_t batch, d, h, w;
    int32_t cx;                 /* channels of x */
    int32_t x0c;                /* first channel read */
    int32_t nc;                 /* channels read */
    float threshold;
    int32_t connectivity;       /* 6, 18 or 26 */
    int32_t mode;               /* dm3d_component_filter: DM3D_CCL_LARGEST, DM3D_CCL_MIN_SIZE or DM3D_CCL_FILL_HOLES */
    int32_t min_size;           /* DM3D_CCL_MIN_SIZE: at least 1 */
    int32_t* labels;            /* [batch, nc, d, h, w]  components: out */
    int32_t* count;             /* [batch, nc]           components: out */
    int64_t* largest;           /* [batch, nc, 2]        components: out */
    float* out;                 /* [batch, d, h, w, nc]  component_filter: out */
    int32_t* work;              /* device scratch */
    int64_t work_elems;         /* int32 it holds */
} dm3d_ccl_desc;
int dm3d_components(const dm3d_ccl_desc* d, void* stream);
int dm3d_component_filter(const dm3d_ccl_desc* d, void* stream);

/* ---- Distribution metrics on feature vectors: the all-pairs passes behind the Frechet distance, KID and precision / recall / density /
 * coverage.  x and y are float64 row-major feature matrices [nx, dim] and [ny, dim].  An entry reads n rows of x and m rows of y: row p
 * of the set is matrix row rows_x[p] (rows_y[p]), or row p where the table is NULL, so a subset or a resample is read in place.  A
 * table entry outside [0, nx) is clamped into it: the caller's fault, never a read outside the matrix.  Features are taken to be
 * finite.  Nothing is read back.
 *
 * Arithmetic, every entry: a pair's sum over the feature axis is float64, sequential in index order 0, 1, .., dim - 1, multiply and
 * add rounded separately (the library builds with -ffp-contract=off); sums over rows or pairs run in the one order given below; no
 * floating-point atomic.  Runs repeat bitwise and a restatement with the same operations in the same order agrees bit for bit.
 *
 *     d2(a, b)  = sum_f (a[f] - b[f]) * (a[f] - b[f])                           squared Euclidean distance, 0 between equal rows
 *     k(a, b)   = t * t * t,  t = (sum_f a[f] * b[f]) / dim + 1                 the cubic kernel of KID; (t * t) * t
 *
 * dm3d_feature_moments  mean[f] = (sum over p = 0 .. n-1 of x[p][f]) / n; cov[f][g] = (sum over p of (x[p][f] - mean[f]) *
 *     (x[p][g] - mean[g])) / (n - 1), both sums sequential in p.  The triangle f <= g is computed and mirrored.  n >= 2.
 * dm3d_knn_radius       radius[p] = the (k + 1)-th smallest of d2(x[p], x[q]) over q = 0 .. n-1, q = p included (the prdc package's
 *     rule: a duplicated row is a neighbour at distance 0).  Squared; no square root is taken.  1 <= k <= DM3D_DIST_MAX_K, k < n.
 * dm3d_prdc_counts      with x the real and y the generated set, radius_x [n] and radius_y [m] their dm3d_knn_radius:
 *     count_y[j] = the number of i with d2(x[i], y[j]) < radius_x[i]           (density; precision is count_y[j] > 0)      int32
 *     near_x[i]  = 1 if some j has d2(x[i], y[j]) < radius_y[j], else 0         (recall)                                    int32
 *     cover_x[i] = 1 if min over j of d2(x[i], y[j]) < radius_x[i], else 0      (coverage)                                  int32
 *     Strict <.  count_y is zeroed on the stream and summed with integer atomics.
 * dm3d_poly_mmd         for every subset s of `subsets`, with rows_x [subsets, n] and rows_y [subsets, m] (NULL: rows 0 .. n-1 and
 *     0 .. m-1 for every subset):  sums[s] = { sum_{i != j} k(x_i, x_j),  sum_{i != j} k(y_i, y_j),  sum_{i, j} k(x_i, y_j) }.
 *     i and j are positions in the subset.  A row sum runs over j in index order (j = i left out), the sum of row sums over i in
 *     index order.
 *         work_elems >= subsets * (2 * n + m)                                   float64
 *
 * A workgroup owns DM3D_DIST_TILE rows, walks the columns in tiles of DM3D_DIST_TILE and the feature axis in chunks of
 * DM3D_DIST_CHUNK, both tiles staged in LDS, 4 x 4 pairs per lane; what a row keeps across column tiles (its k + 1 smallest, its
 * minimum, its sum) stays in the workgroup, so no n x m intermediate reaches memory and no workgroup waits for another one.
 *
 * Checked before any launch (DM3D_EINVAL; the message starts "feature_moments:", "knn_radius:", "prdc_counts:" or "poly_mmd:"): the
 * descriptor and every pointer the entry uses non-NULL; float64 pointers 8-byte, int32 pointers 4-byte aligned; 1 <= dim <=
 * DM3D_DIST_MAX_DIM; n, m, nx, ny <= DM3D_DIST_MAX_ROWS, each limit named when exceeded; n <= nx and m <= ny without a table, nx,
 * ny >= 1; n >= 2 (and m >= 2 for poly_mmd, m >= 1 for prdc_counts); k as above; 1 <= subsets <= DM3D_DIST_MAX_SUBSETS; the scratch
 * size; no output shares a byte with x or y. */
#define DM3D_DIST_MAX_ROWS 65536
#define DM3D_DIST_MAX_DIM 4096
#define DM3D_DIST_MAX_K 16
#define DM3D_DIST_MAX_SUBSETS 16384
#define DM3D_DIST_TILE 64
#define DM3D_DIST_CHUNK 32
typedef struct dm3d_dist_desc {
    const double* x;            /* [nx, dim] */
    const double* y;            /* [ny, dim]             prdc_counts, poly_mmd */
    const int32_t* rows_x;      /* [n], poly_mmd [subsets, n]; NULL: rows 0 .. n-1 */
    const int32_t* rows_y;      /* [m], poly_mmd [subsets, m]; NULL: rows 0 .. m-1 */
    int32_t n;                  /* rows of x read */
    int32_t m;                  /* rows of y read */
    int32_t nx;                 /* rows x holds */
    int32_t ny;                 /* rows y holds */
    int32_t dim;
    int32_t k;                  /* knn_radius */
    int32_t subsets;            /* poly_mmd */
    const double* radius_x;     /* [n]                   prdc_counts: in */
    const double* radius_y;     /* [m]                   prdc_counts: in */
    double* mean;               /* [dim]                 feature_moments: out */
    double* cov;                /* [dim, dim]            feature_moments: out */
    double* radius;             /* [n]                   knn_radius: out */
    int32_t* count_y;           /* [m]                   prdc_counts: out */
    int32_t* near_x;            /* [n]                   prdc_counts: out */
    int32_t* cover_x;           /* [n]                   prdc_counts: out */
    double* sums;               /* [subsets, 3]          poly_mmd: out */
    double* work;               /* device scratch of poly_mmd */
    int64_t work_elems;         /* float64 it holds */
} dm3d_dist_desc;
int dm3d_feature_moments(const dm3d_dist_desc* d, void* stream);
int dm3d_knn_radius(const dm3d_dist_desc* d, void* stream);
int dm3d_prdc_counts(const dm3d_dist_desc* d, void* stream);
int dm3d_poly_mmd(const dm3d_dist_desc* d, void* stream);

/* ---- Volume preprocessing (the reference's dataset_utils.py: reslice, the affine recentring through scipy.ndimage.affine_transform,
 * the fold of negatives, min-max normalisation, flip / brightness / contrast): four entries, all on channel-planar volumes
 * [volumes, d, h, w] except dm3d_augment, which reads NDHWC batches.  Coordinates, weights, coefficients and sums are float64 in one
 * fixed order (the library builds with -ffp-contract=off), stores are float32; no kernel uses an atomic: runs repeat bitwise.
 *
 * dm3d_spline_filter   scipy.ndimage.spline_filter(order=3, mode="mirror"), the prefilter scipy runs in front of mode="constant"
 *     interpolation, per axis w, h, d:   z = sqrt(3) - 2;  c[i] *= (1 - z)(1 - 1/z);
 *         c[0] = (c[0] + z^(n-1) c[n-1] + sum_{i=1}^{n-2} z^i (c[i] + z^(n-1) c[n-1-i])) / (1 - z^(2n-2));   c[i] += z c[i-1]  (i = 1 .. n-1)
 *         c[n-1] = (z c[n-2] + c[n-1]) z / (z^2 - 1);   c[i] = z (c[i+1] - c[i])  (i = n-2 .. 0)
 *     in float64; an axis of length 1 is left unfiltered, as scipy leaves it.  A workgroup stages DM3D_SPLINE_LANES neighbouring lines
 *     in LDS ([n][DM3D_SPLINE_LANES + 1] float64; the line-pass tiler of csrc/dm3d_volume.h, shared with dm3d_edt) and one lane walks
 *     each line.  coeff holds volumes * d * h * w float64.
 * dm3d_affine_resample   out[v][o] = interp(src[v], M_v o + offset_v), scipy.ndimage.affine_transform(mode="constant") for a
 *     [3, 3] matrix; table[v] = {M row by row, offset} (12 float64); a diagonal matrix is the same entry with zeros off the diagonal.
 *         coordinate   c[h] = ((o0 M[h][0] + o1 M[h][1]) + o2 M[h][2]) + offset[h]      each product and sum rounded to float64
 *         outside      c[h] < 0 or c[h] > n[h] - 1 on any axis (or c[h] not a number): out = cval; exactly 0 and n - 1 are inside
 *         order 0      in[floor(c + 0.5)]
 *         order 1      taps floor(c), floor(c) + 1 with weights w0 = 1 - x, w1 = 1 - w0, x = c - floor(c)
 *         order 3      taps floor(c) - 1 .. floor(c) + 2 on the coefficients, y = 1 - x:  w1 = (x x (x - 2) 3 + 4) / 6,
 *                      w2 = (y y (y - 2) 3 + 4) / 6, w0 = y y y / 6, w3 = ((1 - w0) - w1) - w2
 *         a tap outside [0, n - 1] is mirrored (period 2n - 2, no repeated edge; n = 1: index 0)
 *         out = (float) sum over taps, axis 0 outermost, axis 2 innermost, of ((in * w0) * w1) * w2
 *     src is float32 (in_f64 = DM3D_RESAMPLE_F32) or float64 (DM3D_RESAMPLE_F64: dm3d_spline_filter's coefficients).  A workgroup owns
 *     a brick of 4 x 4 x 16 (d, h, w) outputs.  Nothing bounds the table's values: whatever they are, no read leaves the volume.
 * dm3d_volume_normalize   per volume of n elements: a = |x|; out = (a - min a) / (max a - min a), evaluated in float64 and rounded once.
 *     A first kernel leaves exact per-block minima and maxima in partials, a second folds them, writes minmax[v] = {min, max} and
 *     flag[v] = (max == min), and applies them; a constant volume is written as zeros.  No host read sits between the two.
 *         partials holds volumes * DM3D_NORM_PARTIAL_BLOCKS * 2 float32
 * dm3d_augment   per sample b of an NDHWC batch x [batch, d, h, w, c], with mask [batch, d, h, w, cm] (optional) flipped alike:
 *         t(v)   = clip((double)x[v] * brightness[b], 0, 1)
 *         mean   = (sum over the sample of t, float64: DM3D_AUG_PARTIAL_BLOCKS block sums by the fixed tree, added by the same tree) / (d h w c)
 *         out[v] = (float) clip((1 + contrast[b]) * (t(v') - mean) + mean, 0, 1),   v' = v with d - 1 - z for z where flip[b] != 0
 *     (the reference's flip_axis_0, adjust_brightness, adjust_contrast, with its literal (1 + factor)).  flip (int32), brightness and
 *     contrast (float32) are device tables [batch]; bit 1, 2, 4 of draw fills the respective table first, from the Philox4x32-10 block
 *     of counter (b, 0, 0, DM3D_STREAM_AUGMENT) under the key seed: u_k = (float)word_k * 2^-32,
 *         flip = !(u_0 < flip_chance),  brightness = lo + (hi - lo) * u_1,  contrast = lo + (hi - lo) * u_2        in float32
 *         partials holds batch * DM3D_AUG_PARTIAL_BLOCKS float64
 *
 * Checked before any launch (DM3D_EINVAL; the message starts "spline_filter:", "affine_resample:", "volume_normalize:" or "augment:"): the
 * descriptor and every pointer non-NULL (mask and mask_out are given or omitted together) and aligned to its element; volumes / batch
 * >= 1 (at most 65535 where it is a grid axis); every extent >= 1; spline_filter: d, h, w <= DM3D_SPLINE_MAX_EXTENT, a larger extent
 * named as such; affine_resample: order 0, 1 or 3, in_f64 one of the two constants, cval finite, an input volume below 2^31 voxels;
 * volume_normalize: n >= 1; augment: c >= 1, cm >= 1 with a mask, draw in [0, 7], neither out nor mask_out sharing a byte with x, mask or each other, and where draw != 0
 * flip_chance in [0, 1] and both ranges finite and ascending. */
#define DM3D_SPLINE_MAX_EXTENT 512
#define DM3D_SPLINE_LANES 32
#define DM3D_RESAMPLE_F32 0
#define DM3D_RESAMPLE_F64 1
#define DM3D_NORM_PARTIAL_BLOCKS 256
#define DM3D_AUG_PARTIAL_BLOCKS 256
#define DM3D_STREAM_AUGMENT 0xA063u
typedef struct dm3d_spline_desc {
    const float* x;             /* [volumes, d, h, w] */
    double* coeff;              /* [volumes, d, h, w] out */
    int32_t volumes, d, h, w;
} dm3d_spline_desc;
int dm3d_spline_filter(const dm3d_spline_desc* d, void* stream);
typedef struct dm3d_resample_desc {
    const void* src;            /* [volumes, id, ih, iw] float32 or float64 */
    const double* table;        /* [volumes, 12] */
    float* out;                 /* [volumes, od, oh, ow] */
    int32_t in_f64;             /* DM3D_RESAMPLE_F32 or DM3D_RESAMPLE_F64 */
    int32_t volumes, id, ih, iw, od, oh, ow;
    int32_t order;              /* 0, 1 or 3 */
    float cval;
} dm3d_resample_desc;
int dm3d_affine_resample(const dm3d_resample_desc* d, void* stream);
typedef struct dm3d_normalize_desc {
    const float* x;             /* [volumes, n] */
    float* out;                 /* [volumes, n]; may be x itself */
    int32_t volumes;
    int64_t n;
    float* partials;            /* device scratch, written before it is read by every call */
    float* minmax;              /* [volumes, 2] out */
    int32_t* flag;              /* [volumes] out: 1 where the volume is constant */
} dm3d_normalize_desc;
int dm3d_volume_normalize(const dm3d_normalize_desc* d, void* stream);
typedef struct dm3d_augment_desc {
    const float* x;             /* [batch, d, h, w, c] */
    float* out;                 /* [batch, d, h, w, c] */
    const float* mask;          /* [batch, d, h, w, cm] or NULL */
    float* mask_out;            /* [batch, d, h, w, cm] or NULL */
    int32_t batch, d, h, w, c, cm;
    int32_t* flip;              /* [batch] in, or out where bit 1 of draw is set */
    float* brightness;          /* [batch] in, or out where bit 2 of draw is set */
    float* contrast;            /* [batch] in, or out where bit 4 of draw is set */
    int32_t draw;
    uint64_t seed;
    float flip_chance, brightness_lo, brightness_hi, contrast_lo, contrast_hi;
    double* partials;           /* device scratch, written before it is read by every call */
} dm3d_augment_desc;
int dm3d_augment(const dm3d_augment_desc* d, void* stream);

/* ---- Spatial augmentation (random affine plus random elastic deformation, Simard et al. 2003): the Gaussian filter, the uniform draw of
 * a displacement field and the resample at per-voxel coordinates, on channel-planar volumes [volumes, d, h, w].  Sums and coordinates
 * are float64 in one fixed order (the library builds with -ffp-contract=off), stores are float32; no kernel uses an atomic: runs
 * repeat bitwise.
 *
 * dm3d_gaussian_filter   scipy.ndimage.gaussian_filter(order=0) per volume: one pass per axis in scipy's order d, h, w, each
 *         t = x[l] w[0];   t += (x[l - k] + x[l + k]) w[k]   for k = r .. 1          in float64, multiply and add rounded separately,
 *     stored as float32 after every axis (scipy's intermediate is its float32 output array).  weights is a HOST table
 *     [3][DM3D_GAUSS_MAX_RADIUS + 1] of float64, row a (d, h, w) holding w[0 .. r_a] as scipy forms them (r = int(truncate sigma + 0.5),
 *     exp(-0.5 / sigma^2 k^2) divided by the sum over -r .. r); it is read during the call.  A radius of -1 leaves that axis out (scipy's
 *     sigma = 0); an axis of length 1 is filtered like any other.  A tap outside the line maps into it: DM3D_GAUSS_REFLECT has period 2n
 *     with the edge repeated, _MIRROR period 2n - 2, _NEAREST clamps, _CONSTANT reads cval; no halo is staged, so r may exceed n.  A
 *     workgroup stages DM3D_SPLINE_LANES neighbouring lines in LDS ([n][DM3D_SPLINE_LANES + 1] float32, the line-pass tiler of
 *     csrc/dm3d_volume.h) and all its lanes form the outputs.  out may be x itself.  gains = 1 or 3 multiplies volume v by
 *     gain[v % gains] in float32 after the last pass (the alpha of an elastic field [fields, 3, d, h, w]); gains = 0 is scipy's result.
 * dm3d_uniform_field   out[e] = 2 v - 1 in float32, v = (float)word * 2^-32 (dm3d_augment's rule), word = word e & 3 of the
 *     Philox4x32-10 block of counter (lo32(e >> 2), hi32(e >> 2), draw, DM3D_STREAM_ELASTIC) under the key seed, for e < n.
 * dm3d_warp   out[v][o] = interp(src[v], c(o)),   c[h] = ((((o0 M[h][0] + o1 M[h][1]) + o2 M[h][2]) + offset[h]) + (double)u[h][o]
 *     with table[v] = {M row by row, offset} as in dm3d_affine_resample and u = field[v / vols_per_field] ([fields, 3, od, oh, ow],
 *     float32 or float64 by field_f64; NULL: no last term).  The inside test, the taps, the order of the tap sum, cval and the float32
 *     store are dm3d_affine_resample's, as is the brick of 4 x 4 x 16 outputs.  With a zero table and float64 coordinates as the field
 *     this is scipy.ndimage.map_coordinates(mode="constant").  Nothing bounds the field's values: no read leaves the volume.
 *
 * Checked before any launch (DM3D_EINVAL; the message starts "gaussian_filter:", "uniform_field:" or "warp:"): the descriptor and every
 * pointer but warp's field non-NULL and aligned to its element; volumes >= 1 (warp: at most 65535, a multiple of vols_per_field >= 1);
 * every extent >= 1; gaussian_filter: d, h, w <= DM3D_SPLINE_MAX_EXTENT, each radius in [-1, DM3D_GAUSS_MAX_RADIUS], mode one of the four
 * constants, cval, the weights in use and the gains finite, gains 0, 1 or 3, out either x or sharing no byte with it; uniform_field:
 * n >= 1, draw >= 0; warp: order 0, 1 or 3, in_f64 and field_f64 one of the two constants, cval finite, an input volume below 2^31
 * voxels, out sharing no byte with src. */
#define DM3D_GAUSS_MAX_RADIUS 64
#define DM3D_GAUSS_REFLECT 0
#define DM3D_GAUSS_MIRROR 1
#define DM3D_GAUSS_NEAREST 2
#define DM3D_GAUSS_CONSTANT 3
#define DM3D_STREAM_ELASTIC 0xE1A5u
typedef struct dm3d_gauss_desc {
    const float* x;             /* [volumes, d, h, w] */
    float* out;                 /* [volumes, d, h, w]; may be x itself */
    const double* weights;      /* host table [3, DM3D_GAUSS_MAX_RADIUS + 1]; may be NULL when every radius is -1 */
    int32_t volumes, d, h, w;
    int32_t rd, rh, rw;         /* radius per axis, -1: the axis is left out */
    int32_t mode;               /* DM3D_GAUSS_* */
    double cval;
    int32_t gains;              /* 0, 1 or 3 */
    float gain0, gain1, gain2;
} dm3d_gauss_desc;
int dm3d_gaussian_filter(const dm3d_gauss_desc* d, void* stream);
typedef struct dm3d_field_desc {
    float* out;                 /* [n] */
    int64_t n;
    uint64_t seed;
    int32_t draw;
} dm3d_field_desc;
int dm3d_uniform_field(const dm3d_field_desc* d, void* stream);
typedef struct dm3d_warp_desc {
    const void* src;            /* [volumes, id, ih, iw] float32 or float64 */
    const double* table;        /* [volumes, 12] */
    const void* field;          /* [volumes / vols_per_field, 3, od, oh, ow] float32 or float64, or NULL */
    float* out;                 /* [volumes, od, oh, ow] */
    int32_t in_f64, field_f64;  /* DM3D_RESAMPLE_F32 or DM3D_RESAMPLE_F64 */
    int32_t volumes, vols_per_field, id, ih, iw, od, oh, ow;
    int32_t order;              /* 0, 1 or 3 */
    float cval;
} dm3d_warp_desc;
int dm3d_warp(const dm3d_warp_desc* d, void* stream);

/* p[i] = max(p[i] + delta, 0) (the loop counter of generate kept on the device so a captured step replays unchanged; it
 * saturates at 0, so a step issued past the end of a chain never indexes row -1 of a table). */
int dm3d_add_i32(int32_t* p, int32_t n, int32_t delta, void* stream);
/* x ~ N(0,1) from Philox keyed by (seed, stream_id): the x_T draw of generate (:555). n % 4 == 0. */
int dm3d_randn(float* x, int64_t n, uint64_t seed, uint32_t stream_id, void* stream);
/* out[r][:] = table[idx[r]][:] (tf.gather / Embedding lookup, :358, 518-538). c % 4 == 0. */
int dm3d_gather_rows(const float* table, int32_t table_rows, const int32_t* idx, float* out, int32_t rows,
                     int32_t c, void* stream);

/* ---- VectorQuantizer.get_code_indices (vqvae3d_monai.py:164-177): idx[r] = argmin_k (|z_r|^2 + esq[k] - 2*sim[r][k]), float32 in
 * that order, lowest index on ties.  sim = z.E [rows, k] comes from dm3d_gemm_tn; esq[k] = |e_k|^2.  The quantised vectors are
 * then dm3d_gather_rows(E^T, idx). */
int dm3d_vq_assign(const float* z, int64_t rows, int32_t d, const float* sim, int32_t k, const float* esq, int32_t* idx,
                   void* stream);

/* ================= training (DiffusionModel.train_step, conditional_dm3d.py:471-510; compile() at main_conditional_dm.py:149-154) ==========
 * The forward pass of training reuses the entries above in DM3D_PREC_F32 (gradients span too many octaves for the float16 split);
 * data gradients of Conv3D / Dense are those same entries on flipped / transposed weights (dm3d_flip_transpose + dm3d_pack_weights).
 * What follows is what training needs in addition.  All tensors float32; "+=" outputs are accumulated into (the caller zeroes
 * gradient buffers once per step: a weight used twice, or a tensor with two consumers, collects both contributions). */

/* BatchNormalization(training=True) (network(..., training=True), :493): per-channel batch statistics over (B,D,H,W).
 * dm3d_groupnorm_stats (above) accumulates per-(sample, channel) sums into acc [batch][c][2] (float64, zero on entry; call it once per
 * concatenated input with its channel offset); this finishes them: mean, biased variance -> scale = gamma*rstd, shift = beta - mean*scale
 * (the vectors the conv prologue / dm3d_affine_act_cat apply), mean_out / rstd_out kept for the backward pass, and — when
 * moving_mean / moving_var are given — the Keras moving averages moving = moving*momentum + batch*(1 - momentum) (momentum 0.99;
 * unbiased_moving = 1 feeds the variance with Bessel's correction n/(n-1), as tf.nn.fused_batch_norm — what Keras runs for rank-5
 * inputs — does).  acc is zeroed again. */
int dm3d_batchnorm_finalize(double* acc, int32_t batch, int64_t voxels, int32_t c, float eps, const float* gamma, const float* beta,
                            float* scale, float* shift, float* mean_out, float* rstd_out, float* moving_mean, float* moving_var,
                            float momentum, int32_t unbiased_moving, void* stream);
/* y[row][:] = act(concat(x1[row], x2[row]) * scale + shift)  (x2 NULL / c2 0: one input; scale NULL: plain concatenation).
 * y is [rows][c1+c2]: the normalised, activated, concatenated tensor a training step keeps for the weight gradient. */
int dm3d_affine_act_cat(const float* x1, int32_t c1, const float* x2, int32_t c2, int64_t rows, const float* scale, const float* shift,
                        int32_t act, float* y, void* stream);
/* Backward of y = act(BatchNorm_train(concat(x1, x2))) given g = dL/dy [rows][c1+c2]: du = g*act'(x*scale+shift);
 * red[c][2] (float64, zero on entry) receives (sum du, sum du*xhat);  dx (+=) = scale*(du - mean(du) - xhat*mean(du*xhat)) written
 * to dx1 / dx2 (either NULL: no gradient wanted);  dgamma (+=) = sum du*xhat, dbeta (+=) = sum du (both or neither). */
int dm3d_bn_act_bwd(const float* g, const float* x1, int32_t c1, const float* x2, int32_t c2, int64_t rows, const float* scale,
                    const float* shift, const float* mean, const float* rstd, int32_t act, double* red, float* dx1, float* dx2,
                    float* dgamma, float* dbeta, void* stream);

/* Weight gradient of Conv3D(k in {1,3}, stride 1, "same") / Dense in the Keras layout:  dw[tap][ci][co] += sum over samples and voxels
 * of a[voxel + tap - 1][ci] * g[voxel][co]  (a: the layer's input [batch, in_d, in_h, in_w, cin]; g: dL/d output, same extent, cout
 * channels).  A contraction over voxels on v_mfma_f32_32x32x2_f32; partial sums meet through float atomics (dw must hold the running
 * gradient, zero at the start of a step).  ksize 1 covers Dense (rows = batch*in_d*in_h*in_w).  per_item_output = 1 (ksize 1): `batch`
 * independent products with their own output each (strides in elements) — the attention gradients dV = P^T dO, dK = dS^T Q per sample.
 * A stride-2 conv's gradient is this on the dilated output gradient (dm3d_dilate2); an UpSample conv's on the upsampled input. */
typedef struct dm3d_wgrad_desc {
    const float* a; const float* g; float* dw;
    int32_t batch, in_d, in_h, in_w, cin, cout, ksize;
    int32_t per_item_output; int64_t stride_a, stride_g, stride_dw;
} dm3d_wgrad_desc;
int dm3d_wgrad(const dm3d_wgrad_desc* d, void* stream);
/* out[group][:c] += column sums of x over the group's rows (x [groups*rows_per_group][c]): bias gradients (one group) and the gradient
 * of the per-sample time-embedding vector a conv epilogue adds (one group per sample, ld_out = row stride of the vector table). */
int dm3d_colsum(const float* x, int64_t groups, int64_t rows_per_group, int32_t c, float* out, int64_t ld_out, void* stream);
/* Keras kernel [taps][cin][cout] -> [taps][cout][cin] with the taps reversed: the kernel whose stride-1 "same" convolution of dL/dy is
 * dL/dx of the original layer (taps 1: the transpose). */
int dm3d_flip_transpose(const float* keras_kernel, int32_t taps, int32_t cin, int32_t cout, float* out, void* stream);

/* LayerNormalization backward (eps as in the forward): dx += rstd*(dy*gamma - mean(dy*gamma) - xhat*mean(dy*gamma*xhat)),
 * dgamma += sum dy*xhat, dbeta += sum dy.  c % 4 == 0, c <= 1024. */
int dm3d_layernorm_bwd(const float* x, int64_t rows, int32_t c, float eps, const float* gamma, const float* dy, float* dx, float* dgamma,
                       float* dbeta, void* stream);
/* softmax backward in place: dp <- scale * p * (dp - sum_j p_j dp_j) per row; scale = the factor the logits carried (units^-0.5). */
int dm3d_softmax_bwd(const float* p, float* dp, int64_t rows, int32_t cols, int64_t ld, float scale, void* stream);
/* dx = dy * act'(ref): ref = pre-activation (swish) or pre/post alike (ReLU).  dx may alias dy.  n % 4 == 0. */
int dm3d_act_bwd(const float* ref, const float* dy, float* dx, int64_t n, int32_t act, void* stream);
int dm3d_axpy(float* dst, const float* src, int64_t n, float alpha, void* stream);          /* dst += alpha*src */
int dm3d_fill(float* dst, int64_t n, float value, void* stream);
/* dst[b][j][i] = src[b][i][j]: the K-contiguous copies the TN contraction needs of K / V in the attention backward */
int dm3d_transpose(const float* src, int32_t rows, int32_t cols, int64_t ld_src, int64_t stride_src, float* dst, int64_t ld_dst,
                   int64_t stride_dst, int32_t batch, void* stream);
/* dst[r][dst_off + j] = (accumulate ? dst : 0) + src[r][src_off + j] for j < c: a column window of one row-major matrix into another
 * (Concatenate, and the split of its gradient).  c, offsets, leading dimensions % 4 == 0. */
int dm3d_copy_cols(const float* src, int64_t ld_src, int32_t src_off, float* dst, int64_t ld_dst, int32_t dst_off, int64_t rows, int32_t c,
                   int32_t accumulate, void* stream);
/* UpSampling3D(2) materialised (its conv then needs a weight gradient over the upsampled tensor), and its backward (8 children summed, +=) */
int dm3d_upsample2(const float* src, float* dst, int32_t batch, int32_t d, int32_t h, int32_t w, int32_t c, void* stream);
int dm3d_sumpool2_add(const float* src, float* dst, int32_t batch, int32_t d, int32_t h, int32_t w, int32_t c, void* stream);
/* dst [batch, id, ih, iw, c] = 0 except dst[2*o + off] = src[o]: the output gradient of a stride-2 conv spread over the input grid
 * (off = 1 - pad_front per axis), after which data and weight gradients are those of a stride-1 conv. */
int dm3d_dilate2(const float* src, float* dst, int32_t batch, int32_t od, int32_t oh, int32_t ow, int32_t id, int32_t ih, int32_t iw,
                 int32_t offz, int32_t offy, int32_t offx, int32_t c, void* stream);
/* table[idx[r]][:] += src[r][:]  (Embedding gradient, :358) */
int dm3d_scatter_add_rows(const float* src, const int32_t* idx, int32_t rows, int32_t c, float* table, int32_t table_rows, void* stream);
/* noisy = sqrt_alpha_bar[t[b]]*latents + sqrt_one_minus_alpha_bar[t[b]]*noise  (:484-490) */
int dm3d_q_sample(const float* latents, const float* noise, const int32_t* t, const float* sqrt_alpha_bar,
                  const float* sqrt_one_minus_alpha_bar, int32_t timesteps, float* out, int32_t batch, int64_t per_sample, void* stream);
/* *loss += sum((noise - pred)^2) * inv_divisor (float64);  dpred = 2*(pred - noise)*inv_divisor (or NULL).  With
 * inv_divisor = 1/(channels * global_bs * lc^4) this is keras MeanSquaredError(reduction=SUM) / loss_reduction_factor (:496-499). */
int dm3d_mse_loss_grad(const float* pred, const float* noise, int64_t n, double inv_divisor, double* loss, float* dpred, void* stream);
/* keras.optimizers.Adam step over a flat parameter buffer: m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; w -= lr_t*m/(sqrt(v)+eps),
 * lr_t = lr*sqrt(1-b2^t)/(1-b1^t) (the host supplies it; Keras defaults b1 0.9, b2 0.999, eps 1e-7). */
int dm3d_adam(float* w, const float* g, float* m, float* v, int64_t n, float lr_t, float beta1, float beta2, float eps, void* stream);
/* The same step and the exponential moving average of the weights in one launch and one pass over the five buffers: w, m and v
 * become bitwise what dm3d_adam makes of them (adam_kernel and adam_step_kernel call one element function), then
 *     ema += ema_rate * (w_new - ema)          (float32: one sub, one mul, one add)
 * so ema_rate = 0 leaves ema untouched; ema_rate = 1 stores w_new itself (the three operations could miss it by an ulp).  The host supplies ema_rate = 1 - decay (Trainer: with the
 * warm-up decay_t = min(decay, (1 + n) / (10 + n)) of n earlier updates).  HBM-bound at 36 B per element (Adam alone 28, Adam and a
 * separate averaging pass 40).  Checked before the launch (DM3D_EINVAL): every pointer non-NULL and 16-byte aligned, n > 0 and
 * n % 4 == 0 (float4 accesses), ema_rate finite in [0, 1], ema overlapping none of w, g, m, v. */
int dm3d_adam_ema(float* w, const float* g, float* m, float* v, float* ema, int64_t n, float lr_t, float beta1, float beta2, float eps,
                  float ema_rate, void* stream);

/* Global-norm gradient clipping and gradient accumulation, as two device scalars the optimizer's launch reads: no host read sits between
 * the norm and the step.  dm3d_grad_scale makes two launches on `stream`:
 *   grad_sqnorm_kernel          min(ceil(n/4/256), DM3D_GRADNORM_PARTIAL_BLOCKS) blocks (a function of n alone) stride over g as float4;
 *                               every block leaves the float64 sum of (double)g*g (exact products) of its share in partials[block] and
 *                               the slots past the grid are written as 0: nothing a previous launch left in partials is read
 *   grad_scale_finalize_kernel  one block adds the slots in one fixed tree (thread t its slots 4t..4t+3 in index order, then the
 *                               block sum every fixed-order reduction here shares, dm3d_block_sum_f64; no atomics: the result
 *                               repeats bitwise whatever order the blocks ran in)
 *                               and writes
 *     state[0] = (float)(pre_scale * sqrt(sum))                                  the norm of the gradient the step will apply
 *     state[1] = (float)(pre_scale * (norm > clip_norm ? clip_norm / norm : 1))  in float64, rounded once
 *     state[2] = 1 if sum is not finite (an inf or a NaN in g), else 0
 *     state[3] = 0
 * pre_scale is the 1/k of k accumulated micro-batches; clip_norm = +inf clips nothing.  With nothing to clip and pre_scale = 1 the
 * factor is exactly 1.0f, so the step is bitwise the unclipped one.  tf.clip_by_global_norm computes clip * min(1/norm, 1/clip)
 * instead, which is not exactly 1 under the threshold; the rule here differs from it by at most an ulp of the factor.
 * HBM-bound: 4 B per element read once.  Checked before any launch (DM3D_EINVAL): d and every pointer non-NULL, g and state 16-byte and
 * partials 8-byte aligned, n > 0 and n % 4 == 0, clip_norm > 0 (not NaN), pre_scale finite and > 0. */
#define DM3D_GRADNORM_PARTIAL_BLOCKS 1024  /* partials holds [DM3D_GRADNORM_PARTIAL_BLOCKS] doubles */
typedef struct dm3d_gradscale_desc {
    const float* g;             /* [n] the gradient buffer (read only) */
    int64_t n;                  /* > 0, n % 4 == 0 */
    double* partials;           /* [DM3D_GRADNORM_PARTIAL_BLOCKS] device scratch, written in full by every call */
    float* state;               /* [4] device, 16-byte aligned */
    float clip_norm;            /* > 0; +inf: no clipping */
    float pre_scale;            /* finite, > 0 */
} dm3d_gradscale_desc;
int dm3d_grad_scale(const dm3d_gradscale_desc* d, void* stream);
/* dm3d_adam_ema (ema NULL: dm3d_adam) on the gradient state[1] * g[i], one float32 multiply per element; g itself is not modified.
 * Every thread reads state[1] and state[2] (dm3d_grad_scale's) from device memory.  state[2] != 0 skips the step: nothing is stored, and
 * w, m, v and ema stay bitwise as they were.  This entry and dm3d_adam_ema launch forms of one kernel (adam_step_kernel), whose element
 * update is the function dm3d_adam runs, so with state[1] = 1 the results are bitwise theirs, and with state[1] = s bitwise theirs on the buffer float32(s) * g.  Checked before
 * the launch (DM3D_EINVAL): w, g, m, v, state non-NULL; every pointer 16-byte aligned; n > 0 and n % 4 == 0; ema_rate in [0, 1]; ema,
 * when given, overlapping none of w, g, m, v; state overlapping none of the buffers the step writes (w, m, v, ema). */
int dm3d_adam_scaled(float* w, const float* g, float* m, float* v, float* ema /* NULL: none */, int64_t n, float lr_t, float beta1,
                     float beta2, float eps, float ema_rate, const float* state, void* stream);

/* ---- Fitting the VQ codebook on the device: per-code statistics, usage, the exponential-moving-average update of the reference's
 * VectorQuantizerEMA (networks/emavqvae.py:213-222) and the dead-code replacement of NSVQ.replace_unused_codebooks
 * (networks/nsvqvae.py:193-230).  The codebook is [k, dim] float32, rows = codes: the layout dm3d_vq_assign and dm3d_gather_rows read.
 * No entry reads anything back, no kernel uses a floating-point atomic, no workgroup waits for another one, and every sum runs in the
 * one order stated here (the library builds with -ffp-contract=off): runs repeat bitwise and a restatement with the same operations
 * in the same order agrees bit for bit.
 *
 * dm3d_code_stats       z [rows, dim] float32, idx [rows] int32 ->
 *     counts[c]  = the number of rows r with idx[r] == c                                                            int32
 *     sums[c][f] = (double)z[r0][f] + (double)z[r1][f] + ..  over the rows r0 < r1 < .. with idx[r] == c, one add at a time,
 *                  starting from 0.0; a code without a member gets 0 and 0.0                                        float64
 *     invalid[0] = the number of rows with idx[r] outside [0, k); such a row counts nowhere and adds nowhere          int32
 *     A wave owns one code and DM3D_CODEBOOK_SLICE neighbouring features: it streams idx 64 rows at a time, ballots the members,
 *     queues their row numbers in ascending order, loads up to DM3D_CODEBOOK_BATCH queued rows at once and adds them in queue
 *     order, so a code that owns every row pays one load latency per batch, not per row.  No atomic of any kind.
 * dm3d_code_usage       counts [k], rows ->
 *     perplexity[0] = dexp(-(t[0] + t[1] + .. + t[k-1])),  t[c] = p * dlog(p + eps),  p = (double)counts[c] / (double)rows  float64
 *     active[0]     = the number of codes with counts[c] > 0                                                        int32
 *     used_accum[c] += counts[c] when used_accum is non-NULL (NSVQ's codebooks_used.assign_add, :186)               int32
 *     The sum runs over ascending c from 0.0.  dlog and dexp are the library's own, built from +, -, *, / alone so that their bits
 *     are stated, not a math library's:
 *         dlog(x), x > 0:  x = m * 2^e with m in [0.5, 1) (frexp); if m < 0.70710678118654757 then m = m * 2, e = e - 1;
 *             s = (m - 1) / (m + 1);  w = s * s;  P = 1/25;  for j = 23, 21, .., 3: P = P * w + 1/j;  P = P * w + 1;
 *             dlog = e * 0.69314718055994529 + (2 * s) * P       (1/j is the double nearest to it: the constant 1.0 / j)
 *         dexp(y):  n = rint(y * 1.4426950408889634);  r = (y - n * 0.693147180369123816490) - n * 1.90821492927058770002e-10;
 *             Q = 1/14!;  for j = 13, 12, .., 1: Q = Q * r + 1/j!;  Q = Q * r + 1;  dexp = ldexp(Q, n)   (1/j! = 1.0 / (double)j!)
 *     Both agree with a correctly rounded log and exp within 1e-15 relative on what this entry feeds them (tests/test_codebook_host.py).
 * dm3d_codebook_ema     counts [k], sums [k, dim] -> cluster_size [k], ema_w [k, dim], codebook [k, dim], esq [k], all in place, float32:
 *     om = 1.0f - decay;  N'[c] = N[c] * decay + om * (float)counts[c];  W'[c][f] = W[c][f] * decay + om * (float)sums[c][f]
 *     (every multiply and add rounded on its own, the float64 sum rounded to float32 once);
 *     n = N'[0] + N'[1] + .. in float64 over ascending c from 0.0;  g = (float)(n / (n + (double)epsilon));
 *     codebook[c][f] = (W'[c][f] / N'[c]) * g;  esq[c] = codebook[c][0]^2 + codebook[c][1]^2 + ..  in float32, sequential in f from
 *     0.0f, multiply and add rounded separately (numpy's (emb ** 2).sum(axis=0, dtype=float32) on [dim, k]).
 *     One departure from the reference: a code whose N' is exactly 0 (it has never had a member) keeps its codebook row and its esq;
 *     the literal rule divides by zero there.  One launch of one workgroup, since n needs every N' before any row is written.
 * dm3d_codebook_replace  used [k] int32 (NSVQ's codebooks_used), num_batches, threshold -> codebook, esq (and cluster_size, ema_w when
 *     given) in place, used zeroed, used_count[0] and unused_count[0] int32:
 *     code c is unused where (double)used[c] / (double)num_batches < threshold.  U = the used codes, V = the unused codes, both ascending.
 *       |U| == 0:          every row c becomes codebook[c] + noise; cluster_size and ema_w stay.
 *       |U| >= |V|:        V[j] takes the row of U[j].
 *       0 < |U| < |V|:     the list L[i] = U[i % |U|], i < |U| * (|V| / |U| + 1) (integer division; at most k entries), is sorted
 *                          ascending by (key[i], i), key[i] = word 0 of Philox4x32-10 on the counter (i, 0, draw,
 *                          DM3D_STREAM_CODEBOOK_SHUFFLE) under the key seed; V[j] takes the row of the j-th entry.
 *     A row c that takes the row of source s becomes codebook[s][f] + noise_scale * z[c][f] (float32, multiply and add rounded
 *     separately), z the N(0,1) stream of "What seeded means": float4 c * (dim / 4) + f / 4 has the counter (that index, draw,
 *     DM3D_STREAM_CODEBOOK) under the key seed; it also copies cluster_size[s] and ema_w[s] when those are given, so that an EMA step
 *     afterwards does not pull it straight back.  esq of every rewritten row is recomputed by dm3d_codebook_ema's rule.  Sources are
 *     used codes and are never written, so every source row is read as it was.  Two launches on the stream: one workgroup builds
 *     map[c] (the source of c, c itself where only noise is added, -1 where the row stays), then a workgroup per code applies it.
 *
 * Checked before any launch (DM3D_EINVAL; the message starts "code_stats:", "code_usage:", "codebook_ema:" or "codebook_replace:"):
 * the descriptor and every pointer the entry uses non-NULL (used_accum, and cluster_size with ema_w for codebook_replace, are
 * optional); float64 pointers 8-byte, all others 4-byte aligned, codebook and ema_w 16-byte; 1 <= k <= DM3D_CODEBOOK_MAX_K;
 * 4 <= dim <= DM3D_CODEBOOK_MAX_DIM and dim % 4 == 0; 1 <= rows <= DM3D_CODEBOOK_MAX_ROWS, each limit named when exceeded; eps >= 0;
 * 0 <= decay <= 1, epsilon >= 0; num_batches >= 1, noise_scale finite; no buffer an entry writes shares a byte with another buffer
 * it uses. */
#define DM3D_CODEBOOK_MAX_K 4096
#define DM3D_CODEBOOK_MAX_DIM 1024
#define DM3D_CODEBOOK_MAX_ROWS 1073741824
#define DM3D_CODEBOOK_SLICE 64
#define DM3D_CODEBOOK_BATCH 16
#define DM3D_STREAM_CODEBOOK 0xC0DE
#define DM3D_STREAM_CODEBOOK_SHUFFLE 0xC0D5
typedef struct dm3d_codebook_desc {
    const float* z;             /* [rows, dim]           code_stats: in */
    const int32_t* idx;         /* [rows]                code_stats: in */
    int32_t rows;               /* code_stats, code_usage */
    int32_t dim;
    int32_t k;
    int32_t* counts;            /* [k]                   code_stats: out; code_usage, codebook_ema: in */
    double* sums;               /* [k, dim]              code_stats: out; codebook_ema: in */
    int32_t* invalid;           /* [1]                   code_stats: out */
    double eps;                 /* code_usage */
    double* perplexity;         /* [1]                   code_usage: out */
    int32_t* active;            /* [1]                   code_usage: out */
    int32_t* used_accum;        /* [k]                   code_usage: in place, optional */
    float* cluster_size;        /* [k]                   codebook_ema: in place; codebook_replace: in place, optional */
    float* ema_w;               /* [k, dim]              codebook_ema: in place; codebook_replace: in place, optional */
    float* codebook;            /* [k, dim]              codebook_ema, codebook_replace: in place */
    float* esq;                 /* [k]                   codebook_ema, codebook_replace: in place */
    float decay;                /* codebook_ema */
    float epsilon;              /* codebook_ema */
    int32_t* used;              /* [k]                   codebook_replace: in, zeroed */
    int32_t num_batches;        /* codebook_replace */
    int32_t draw;               /* codebook_replace: word of both Philox counters; a caller counts its replacements here */
    double threshold;           /* codebook_replace */
    float noise_scale;          /* codebook_replace */
    uint64_t seed;              /* codebook_replace */
    int32_t* used_count;        /* [1]                   codebook_replace: out */
    int32_t* unused_count;      /* [1]                   codebook_replace: out */
    int32_t* map;               /* [k]                   codebook_replace: device scratch */
} dm3d_codebook_desc;
int dm3d_code_stats(const dm3d_codebook_desc* d, void* stream);
int dm3d_code_usage(const dm3d_codebook_desc* d, void* stream);
int dm3d_codebook_ema(const dm3d_codebook_desc* d, void* stream);
int dm3d_codebook_replace(const dm3d_codebook_desc* d, void* stream);

/* ---- HIP graph capture of one denoising step (replaces the eager per-op Python loop of generate, :559-573) -- */
int dm3d_graph_begin(void* stream);
int dm3d_graph_end(void* stream, void** graph_exec_out);
int dm3d_graph_launch(void* graph_exec, void* stream);
int dm3d_graph_destroy(void* graph_exec);

#ifdef __cplusplus
}
#endif
#endif /* DM3D_H */
