// dm3d_conv_args.h — what the Conv3d host code and kernels share.  ConvArgs: the launch arguments every conv kernel (fp32 and split-fp16
// "H3") takes by value.  ConvLaunch: the host's resolved description of one launch — the arguments the descriptor determines plus the
// decision which kernel, brick depth, column form and Cin split serve it and what workspace that needs.  dm3d_conv_resolve
// (dm3d_conv.hip) is the one place that fills it; dm3d_conv3d_ndhwc and the three queries (dm3d_conv_tile_form, dm3d_conv_scratch_bytes,
// dm3d_conv_split_counter_words) consume it, and the launchers dispatch on it without deriving anything again.
#pragma once
#include "dm3d_common.h"

struct ConvArgs {
    const float* x1; const float* x2; int c1, c2;
    int ind, inh, inw;        // physical input extent
    int lgd, lgh, lgw;        // logical extent seen by the conv (2x when upsampling)
    int od, oh, ow;
    int padz, pady, padx;     // zero voxels in front of index 0 per axis (TF SAME; parity mode: 1 - parity bit)
    int os;                   // output stride in the full output tensor (2 in parity mode, else 1)
    int ooz, ooy, oox;        // output offset in the full output tensor (the parity bits)
    int fd, fh, fw;           // extent of the full output tensor (od*os ...)
    int parity;               // 1: blockIdx.z enumerates the 8 output parities of a nearest-2x upsample + k3 conv, each a
                              //    2x2x2 conv on the low-resolution input with pre-summed weights
    long w_parity_stride;     // elements (fp32) / halfs (h3) between the packed weight images of two parities
    const void* wpk; int cinpad, coutpad;
    const float* bias; const float* pscale; const float* pshift; long pro_bstride;
    const float* vec; const int* vec_idx; int vec_ld;
    int relu; const float* res; float* out; int cout;
    const float* prelu; int relu_out;      // PReLU slope [od*os, oh*os, ow*os, cout] before res; ReLU after res
    int bd, bh, bw;           // bricks per volume along d, h, w
    int nchunks;
    int batch;
    float out_scale;          // H3: 2^-w_exp, applied to the accumulator
    int ksplit;               // h3v2: workgroups per brick along Cin (each contracts nchunks / ksplit chunks); > 1: the hand-over form
                              // (dm3d_conv_h3v2_parts.h, split_*): every part stores its raw accumulator tiles into scratch, the part that
                              // draws the last ticket of its tile sums them in part order and runs the epilogue
    int* split_counters;      // one ticket word per tile (brick x column tile x parity): zero before the launch, zero again behind it
    int split_counter_words;
    long split_tile_floats;   // floats of one part's image of one tile in scratch ([tile][part][piece][thread] x 4)
    void* scratch; long scratch_bytes;
    const float* post_scale; const float* post_shift;   // h3v2: out = silu(out*post_scale[c] + post_shift[c]) after everything else
    int out_h2;               // h3v2: store the output in DM3D_FMT_H2 (full bricks, cout % 64 == 0 only)
    int x_h2;                 // h3v2: x1 arrives in DM3D_FMT_H2 (c1 % 16 == 0, no x2, no prologue)
    // h3v2 only: a 1x1 conv over a second (raw, un-normalised) input accumulated into the same tile (ResidualBlock skip path)
    const float* sx1; const float* sx2; int sc1, sc2; const void* swpk; int s_npairs;
    const void* swpk_f;                      // optional: the skip weights as operand fragments (dm3d_pack_weights_skip_h3f): the Winograd-x form's tail   // s_npairs = round_up(sc1+sc2, 32) / 32
    const void* wpk_wino;                    // optional weight image of the Winograd-x form (dm3d_conv_h3w.hip)
    int* range_flag; float range_limit;      // H3 range guard (include/dm3d.h): *range_flag = 1 if any |output| > range_limit
    float* gn_stats;                         // fused GroupNormalization statistics of the OUTPUT (include/dm3d.h): [batch][slots][cout][2] partial (sum, sum of squares)
    int epi_vec4;                            // h3v2: every epilogue operand is 16-byte aligned (cout, vec_ld % 4 == 0): 16-byte epilogue accesses
};

// which tile configuration a (ksize, stride) pair uses
enum { DM3D_CONV_K3S1 = 0, DM3D_CONV_K3S2 = 1, DM3D_CONV_K1 = 2, DM3D_CONV_UP = 3, DM3D_CONV_K4S2 = 4 };

// Kernel family that serves a launch
enum { DM3D_CONV_FAM_F32 = 0,      // conv3d_igemm_f32 (dm3d_conv.hip)
       DM3D_CONV_FAM_TAP = 1,      // H3, DM3D_WL_TAP weights: conv3d_igemm_h3 (dm3d_conv_h3.hip)
       DM3D_CONV_FAM_V3 = 2,       // H3, DM3D_WL_PAIR weights: the free-running direct form conv3d_igemm_h3v3 (dm3d_conv_h3v3.hip)
       DM3D_CONV_FAM_WINO = 3 };   // H3, DM3D_WL_PAIR weights + wpk_wino: the Winograd-x form conv3d_igemm_h3w (dm3d_conv_h3w.hip)

// Host only: one conv launch, resolved from its descriptor by dm3d_conv_resolve.  `a` holds everything the descriptor determines (the
// launchers add what belongs to their kernel: bricks per volume, epi_vec4, the split fields); the rest is the decision.
struct ConvLaunch {
    ConvArgs a;
    int which;                  // DM3D_CONV_K3S1 ...
    int family;                 // DM3D_CONV_FAM_*
    // the two 16x16x32 kernels (FAM_V3, FAM_WINO) only; 0 elsewhere
    int td;                     // z-slices per brick: 4 or 8 (the Winograd-x form: 8)
    int nct;                    // 16-column tiles per workgroup: 4, or the narrow forms 2 (cout <= 32) and 1 (cout <= 16) of the k3 direct kernel
    int ksplit;                 // workgroups per tile along Cin (1: no split)
    long tiles, tile_floats;    // tiles of the launch (bricks x 64-column tiles x parities); floats of one part's image of one tile in scratch
    int64_t need_bytes; long need_words;        // scratch bytes and ticket words this launch needs (0 unless ksplit > 1)
    // what dm3d_conv_scratch_bytes / dm3d_conv_split_counter_words answer: the most a descriptor of this geometry can use
    int64_t can_bytes; long can_words;
};
ConvLaunch dm3d_conv_resolve(const dm3d_conv_desc* d);     // validates nothing (the queries ask about descriptors a launch refuses)

int dm3d_conv_launch_f32(ConvArgs& a, int which, hipStream_t st);
int dm3d_conv_launch_h3(ConvArgs& a, int which, hipStream_t st);
int dm3d_conv_launch_h3v3(const ConvLaunch& r, hipStream_t st);      // which in {K3S1, UP}
int dm3d_conv_launch_h3w(const ConvLaunch& r, hipStream_t st);
struct H3v2Launch { ConvArgs k; bool stats_after; };       // what pre_launch made of a ConvLaunch: the kernel's own arguments; the stand-alone statistics pass behind it
int dm3d_h3v2_pre_launch(const ConvLaunch& r, H3v2Launch& L);
int dm3d_h3v2_post_launch(const ConvArgs& a, const H3v2Launch& L, hipStream_t st);
