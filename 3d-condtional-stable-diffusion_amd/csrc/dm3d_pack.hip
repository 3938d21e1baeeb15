// dm3d_pack.hip — every Conv3d weight packer of the C ABI and its size query.  A packer runs once per weight set, never on the step.
//   * one source rule (src_value): the float32 a (parity, tap, ci, co) position of an image takes from the Keras kernel — plain, the
//     UpSample parity sums, Conv3DTranspose, or a Winograd F(2,3) term — times in_scale[ci], times 2^w_exp;
//   * one record writer (write_record): the float16 hi / lo split and the store into the XOR-swizzled 64-byte record (dm3d_h3.h);
//   * two image kernels: pack_f32_kernel ([parity][tap][CoutPad][CinPad] float32, conv3d_igemm_f32) and pack_h3_kernel (the
//     [parity][ntile][chunk][tap][64 positions][REC] family: DM3D_WL_TAP for conv3d_igemm_h3, DM3D_WL_PAIR for the two 16x16x32 kernels,
//     their Winograd-x image and the fused skip conv's image), plus pack_skip_h3f_kernel, whose operand-fragment order is its own.
// A grid-stride loop writes every element of an image exactly once from its own index, so the grid moves no byte: launch_pack gives
// every packer the same clamp.
// reference ops: Conv3D / UpSampling3D + Conv3D / Conv3DTranspose weights in Keras layouts (networks/conditional_dm3d.py:238-296,
// networks/vqvae3d_monai.py:373-377).
#include "dm3d_conv_h3v2_parts.h"

using h3v2::REC;
using h3v2::pi_col;

namespace {

// ---- the source rule ------------------------------------------------------------------------------------------------------------
enum { SRC_PLAIN = 0, SRC_UP = 1, SRC_CONVT = 2, SRC_WINO = 3 };       // (0-2 are dm3d_pack_weights_h3p's `mode`)

struct Src {
    const float* w; const float* in_scale;     // Keras kernel; optional per-input-channel factor
    int cin, cout, mode;
    float scale;                               // 2^w_exp (1 for the float32 images)
};

// Weight of tap2 = (td,th,tw) in {0,1}^3 of the 2x2x2 conv that reproduces, for output parity par = (a,b,c), a 3x3x3 conv on
// the nearest-2x upsampled tensor (reference UpSample, conditional_dm3d.py:288-296): along each axis the three taps of the
// k3 kernel read source voxels {i-1, i, i} (parity 0) or {i, i, i+1} (parity 1), so the taps sharing a source are summed.
__device__ __forceinline__ float up_weight(const float* __restrict__ w, int cin, int cout, int par, int tap2, int ci, int co) {
    float acc = 0.f;
    const int pa[3] = {par >> 2, (par >> 1) & 1, par & 1};
    const int tt[3] = {tap2 >> 2, (tap2 >> 1) & 1, tap2 & 1};
    int lo[3], hi[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        if (pa[ax] == 0) { lo[ax] = tt[ax] == 0 ? 0 : 1; hi[ax] = tt[ax] == 0 ? 0 : 2; }
        else             { lo[ax] = tt[ax] == 0 ? 0 : 2; hi[ax] = tt[ax] == 0 ? 1 : 2; }
    }
    for (int kd = lo[0]; kd <= hi[0]; ++kd)
        for (int kh = lo[1]; kh <= hi[1]; ++kh)
            for (int kw = lo[2]; kw <= hi[2]; ++kw)
                acc += w[((long)((kd * 3 + kh) * 3 + kw) * cin + ci) * cout + co];
    return acc;
}

// Weight of tap2 of the 2x2x2 conv that reproduces, for output parity par, Conv3DTranspose(k=4, strides=2, padding="same")
// (reference vqvae3d_monai.py:373-377).  Forward conv y[i] = sum_k x[2i+k-1] w[k]; its transpose out[j] = sum_{2i+k-1=j} y[i] w[k]:
// j = 2m reads y[m-1] w[3] + y[m] w[1]; j = 2m+1 reads y[m] w[2] + y[m+1] w[0].  Keras layout [kd,kh,kw,Cout,Cin].
__device__ __forceinline__ float convt_weight(const float* __restrict__ w, int cin, int cout, int par, int tap2, int ci, int co) {
    const int pa[3] = {par >> 2, (par >> 1) & 1, par & 1};
    const int tt[3] = {tap2 >> 2, (tap2 >> 1) & 1, tap2 & 1};
    int k[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) k[ax] = pa[ax] == 0 ? (tt[ax] == 0 ? 3 : 1) : (tt[ax] == 0 ? 2 : 0);
    return w[((long)((k[0] * 4 + k[1]) * 4 + k[2]) * cout + co) * cin + ci];
}

// Winograd F(2,3) along x (dm3d_conv_h3w.hip): virtual tap = 2 * step + h, step = 5 * t + tap pair; the pair's two (dz, dy) taps, lane
// half h picking one: (dz, 0) | (dz, 1) for pairs 0-2, (0, 2) | pad, (1, 2) | (2, 2) — two per-lane operand bases serve all five (the
// kernel's a_pair); transform term t of the tap's three x taps.  The pad half repeats (0, 2) (wino_pad_half).
__device__ __forceinline__ float wino_weight(const float* __restrict__ w, int cin, int cout, int tap, int ci, int co) {
    const int step = tap >> 1, t = step / 5;
    const int tq = (step % 5) < 3 ? (step % 5) * 3 + (tap & 1) : ((step % 5) == 3 ? 2 : ((tap & 1) ? 8 : 5));
    const float g0 = w[((long)(tq * 3 + 0) * cin + ci) * cout + co], g1 = w[((long)(tq * 3 + 1) * cin + ci) * cout + co],
                g2 = w[((long)(tq * 3 + 2) * cin + ci) * cout + co];
    return t == 0 ? g0 : (t == 1 ? 0.5f * ((g0 + g2) + g1) : (t == 2 ? 0.5f * ((g0 + g2) - g1) : g2));
}
// The Winograd image's pad half holds the hi pieces of (0, 2) over zero lo pieces: the kernel's lane half 1 holds the LO piece of
// (0, 2)'s voxels at that step, so one MFMA makes ah.bh + al.bh and the lo pass (bl | 0) ah.bl alone.
__device__ __forceinline__ bool wino_pad_half(int tap) { return ((tap >> 1) % 5) == 3 && (tap & 1); }

// The one rule: the value of input channel ci < cin, output channel co < cout at `tap` of parity image `par` (0 unless UP / CONVT).
__device__ __forceinline__ float src_value(const Src& s, int par, int tap, int ci, int co) {
    float v = s.mode == SRC_WINO ? wino_weight(s.w, s.cin, s.cout, tap, ci, co)
            : s.mode == SRC_UP ? up_weight(s.w, s.cin, s.cout, par, tap, ci, co)
            : s.mode == SRC_CONVT ? convt_weight(s.w, s.cin, s.cout, par, tap, ci, co) : s.w[((long)tap * s.cin + ci) * s.cout + co];
    if (s.in_scale) v *= s.in_scale[ci];
    return v * s.scale;
}
__host__ __device__ constexpr int src_parities(int mode) { return (mode == SRC_UP || mode == SRC_CONVT) ? 8 : 1; }

// ---- the H3 record ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void split_h3(float v, _Float16& hi, _Float16& lo) {
    hi = (_Float16)v;
    lo = (_Float16)(v - (float)hi);
}

// channel k of a chunk into the record of LDS position `pos`: slots (hi c0-7, hi c8-15, lo c0-7, lo c8-15), slot s at physical slot s ^ swz(pos)
__device__ __forceinline__ void write_record(_Float16* __restrict__ r, int pos, int k, float v, bool zero_lo) {
    _Float16 hi, lo;
    split_h3(v, hi, lo);
    const int sw = swz(pos);
    r[(((k >> 3) ^ sw) << 3) + (k & 7)] = hi;
    r[(((2 + (k >> 3)) ^ sw) << 3) + (k & 7)] = zero_lo ? (_Float16)0.0f : lo;
}

// [ntile][chunk][tap][64 positions] records of one parity image; taps and chunks already padded to what the reading kernel steps by
struct H3Geom {
    int tapsp, nchunks, ntiles;
    __host__ __device__ long records() const { return (long)ntiles * nchunks * tapsp * 64; }
    int64_t bytes() const { return (int64_t)records() * REC * (int64_t)sizeof(_Float16); }
};
H3Geom h3_geom(int taps, int tap_group, int cin, int cin_group, int cout) {
    return {(taps + tap_group - 1) / tap_group * tap_group, (int)(dm3d_round_up(cin, cin_group) / 16), (int)(dm3d_round_up(cout, 64) / 64)};
}
struct H3Index { int pos, tap, chunk, ntile; };
__device__ __forceinline__ H3Index h3_index(long rec, const H3Geom& g) {
    return {(int)(rec % 64), (int)((rec / 64) % g.tapsp), (int)((rec / (64L * g.tapsp)) % g.nchunks), (int)(rec / (64L * g.tapsp * g.nchunks))};
}

// Keras kernel -> src_parities(mode) images [ntile][chunk][tap][64][REC] halfs, scaled by 2^w_exp; taps >= taps, channels >= cin and
// columns >= cout are zero.  Which output channel of its 64-column tile a position holds:
//   DM3D_WL_TAP                  position n holds channel n (conv3d_igemm_h3 reads rows in channel order)
//   DM3D_WL_PAIR                 position 16 t16 + pi_pos(c) holds channel 16 t16 + c: the row MFMA column c of 16-column tile t16 reads
//   DM3D_WL_PAIR, SRC_WINO       ... holds channel 4 c + t16: a lane's four column tiles are four consecutive channels (epilogue_cq,
//                                dm3d_conv_h3v2_parts.h)
// The fused skip conv's image is the PAIR image of a one-tap kernel whose chunks come in pairs (h3_geom's cin_group = 32).
__global__ __launch_bounds__(256) void pack_h3_kernel(Src s, int taps, H3Geom g, int layout, _Float16* __restrict__ out) {
    const long nrec = g.records();
    for (long i0 = (long)blockIdx.x * 256 + threadIdx.x; i0 < nrec * 16 * src_parities(s.mode); i0 += (long)gridDim.x * 256) {
        const int par = (int)(i0 / (nrec * 16));
        const long i = i0 % (nrec * 16);
        const int k = (int)(i & 15);
        const long rec = i >> 4;
        const H3Index x = h3_index(rec, g);
        const int c = pi_col(x.pos & 15), t16 = x.pos >> 4;
        const int col = layout == DM3D_WL_TAP ? x.pos : (s.mode == SRC_WINO ? 4 * c + t16 : 16 * t16 + c);
        const int ci = x.chunk * 16 + k, co = x.ntile * 64 + col;
        const float v = (ci < s.cin && co < s.cout && x.tap < taps) ? src_value(s, par, x.tap, ci, co) : 0.f;
        write_record(out + ((long)par * nrec + rec) * REC, x.pos, k, v, s.mode == SRC_WINO && wino_pad_half(x.tap));
    }
}

// the 1x1 skip kernel as MFMA operand fragments: [coutpad/64][npairs][4 column tiles][hi | lo][64 lanes][8 halfs]; lane (column c = lane & 15,
// k group = lane >> 4: chunk 2 pair + (k group >> 1), channels 8 (k group & 1) .. + 7 of it) holds its 8 consecutive k of output channel
// 64 ntile + 4 c + tile (the Winograd kernel's column mapping) — what the v_mfma_f32_16x16x32_f16 B operand of that lane is.  One element
// per thread is one half of a split, not a record: the order is not the family's above, so this stays a kernel of its own.
__global__ __launch_bounds__(256) void pack_skip_h3f_kernel(Src s, int npairs, int ntiles, _Float16* __restrict__ out) {
    const long npieces = (long)ntiles * npairs * 4 * 2 * 64;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < npieces * 8; i += (long)gridDim.x * 256) {
        const int j = (int)(i & 7);
        long q = i >> 3;
        const int lane = (int)(q & 63); q >>= 6;
        const int hilo = (int)(q & 1); q >>= 1;
        const int ni = (int)(q & 3); q >>= 2;
        const int pair = (int)(q % npairs);
        const int nt = (int)(q / npairs);
        const int kg = lane >> 4;
        const int ci = (pair * 2 + (kg >> 1)) * 16 + (kg & 1) * 8 + j, co = nt * 64 + 4 * (lane & 15) + ni;
        _Float16 hi, lo;
        split_h3((ci < s.cin && co < s.cout) ? src_value(s, 0, 0, ci, co) : 0.0f, hi, lo);
        out[i] = hilo ? lo : hi;
    }
}

// Keras kernel -> src_parities(mode) images [taps][coutpad][cinpad] float32 (K contiguous per output channel), zero padded
__global__ __launch_bounds__(256) void pack_f32_kernel(Src s, int taps, int cinpad, int coutpad, float* __restrict__ out) {
    const long per = (long)taps * coutpad * cinpad;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per * src_parities(s.mode); i += (long)gridDim.x * 256) {
        const int par = (int)(i / per);
        const long j = i % per;
        const int ci = (int)(j % cinpad);
        const int co = (int)((j / cinpad) % coutpad);
        const int tap = (int)(j / ((long)cinpad * coutpad));
        out[i] = (ci < s.cin && co < s.cout) ? src_value(s, par, tap, ci, co) : 0.f;
    }
}

// ---- host: one argument check, one launcher -----------------------------------------------------------------------------------------
int pack_check(const char* entry, const void* kernel, const void* packed, int taps, int cin, int cout, int w_exp, bool h3) {
    DM3D_REQUIRE(kernel && packed && taps > 0 && cin > 0 && cout > 0, "%s: null pointer or non-positive size (taps %d, cin %d, cout %d)", entry,
                 taps, cin, cout);
    DM3D_REQUIRE(w_exp >= -100 && w_exp <= 100, "%s: w_exp %d out of range", entry, w_exp);
    DM3D_REQUIRE(!h3 || dm3d_aligned16(packed), "%s: packed must be 16-byte aligned", entry);
    return DM3D_OK;
}

// n elements, one per thread of a grid-stride loop: at most 4096 blocks of 256
template <class... P, class... A>
int launch_pack(const char* entry, void (*kernel)(P...), long n, void* stream, A... args) {
    const long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), args...);
    return dm3d_launch_check(entry);
}

int pack_h3(const char* entry, const float* w, int mode, int layout, int taps, const H3Geom& g, int cin, int cout, int w_exp,
            const float* in_scale, void* packed, void* stream) {
    if (int rc = pack_check(entry, w, packed, taps, cin, cout, w_exp, true)) return rc;
    const Src s{w, in_scale, cin, cout, mode, ldexpf(1.0f, w_exp)};
    return launch_pack(entry, pack_h3_kernel, g.records() * 16 * src_parities(mode), stream, s, taps, g, layout, static_cast<_Float16*>(packed));
}

int pack_f32(const char* entry, const float* w, int mode, int taps, int cin, int cout, const float* in_scale, float* packed, void* stream) {
    if (int rc = pack_check(entry, w, packed, taps, cin, cout, 0, false)) return rc;
    const int cinpad = (int)dm3d_round_up(cin, DM3D_CIN_PAD), coutpad = (int)dm3d_round_up(cout, DM3D_COUT_PAD);
    const Src s{w, in_scale, cin, cout, mode, 1.0f};
    return launch_pack(entry, pack_f32_kernel, (long)taps * cinpad * coutpad * src_parities(mode), stream, s, taps, cinpad, coutpad, packed);
}

bool positive(int a, int b, int c = 1) { return a > 0 && b > 0 && c > 0; }
H3Geom tap_geom(int taps, int cin, int cout) { return h3_geom(taps, 1, cin, 16, cout); }       // DM3D_WL_TAP
H3Geom pair_geom(int taps, int cin, int cout) { return h3_geom(taps, 4, cin, 16, cout); }      // DM3D_WL_PAIR: the kernels step by groups of 4 taps
H3Geom skip_geom(int cin, int cout) { return h3_geom(1, 1, cin, 32, cout); }                   // one tap, chunks in pairs

// the eight parity images of an UpSample / Conv3DTranspose conv, in the layout its geometry reads
int pack_parity_h3(const char* entry, const float* w, int mode, int layout, int cin, int cout, int w_exp, void* packed, void* stream) {
    return pack_h3(entry, w, mode, layout, 8, layout == DM3D_WL_PAIR ? pair_geom(8, cin, cout) : tap_geom(8, cin, cout), cin, cout, w_exp,
                   nullptr, packed, stream);
}

}  // namespace

// ---- float32 images ------------------------------------------------------------------------------------------------------------------
extern "C" int64_t dm3d_packed_weight_elems(int32_t taps, int32_t cin, int32_t cout) {
    return positive(taps, cin, cout) ? (int64_t)taps * dm3d_round_up(cout, DM3D_COUT_PAD) * dm3d_round_up(cin, DM3D_CIN_PAD) : 0;
}

extern "C" int dm3d_pack_weights(const float* keras_kernel, int32_t taps, int32_t cin, int32_t cout, const float* in_scale,
                                 float* packed, void* stream) {
    return pack_f32("pack_weights", keras_kernel, SRC_PLAIN, taps, cin, cout, in_scale, packed, stream);
}

extern "C" int64_t dm3d_packed_weight_up_elems(int32_t cin, int32_t cout) { return 8 * dm3d_packed_weight_elems(8, cin, cout); }

extern "C" int dm3d_pack_weights_up(const float* keras_kernel, int32_t cin, int32_t cout, float* packed, void* stream) {
    return pack_f32("pack_weights_up", keras_kernel, SRC_UP, 8, cin, cout, nullptr, packed, stream);
}

extern "C" int dm3d_pack_weights_convt(const float* keras_kernel, int32_t cin, int32_t cout, float* packed, void* stream) {
    return pack_f32("pack_weights_convt", keras_kernel, SRC_CONVT, 8, cin, cout, nullptr, packed, stream);
}

// ---- DM3D_WL_TAP images, and the parity images in the layout dm3d_conv_weight_layout names -------------------------------------------
extern "C" int64_t dm3d_packed_weight_h3_bytes(int32_t taps, int32_t cin, int32_t cout) {
    return positive(taps, cin, cout) ? tap_geom(taps, cin, cout).bytes() : 0;
}

extern "C" int dm3d_pack_weights_h3(const float* keras_kernel, int32_t taps, int32_t cin, int32_t cout, int32_t w_exp,
                                    const float* in_scale, void* packed, void* stream) {
    return pack_h3("pack_weights_h3", keras_kernel, SRC_PLAIN, DM3D_WL_TAP, taps, tap_geom(taps, cin, cout), cin, cout, w_exp, in_scale, packed,
                   stream);
}

extern "C" int64_t dm3d_packed_weight_up_h3_bytes(int32_t cin, int32_t cout) { return 8 * dm3d_packed_weight_h3_bytes(8, cin, cout); }

extern "C" int dm3d_pack_weights_up_h3(const float* keras_kernel, int32_t cin, int32_t cout, int32_t w_exp, void* packed,
                                       void* stream) {
    return pack_parity_h3("pack_weights_up_h3", keras_kernel, SRC_UP, dm3d_conv_weight_layout(3, 1, 1, 0, cout), cin, cout, w_exp, packed, stream);
}

extern "C" int dm3d_pack_weights_convt_h3(const float* keras_kernel, int32_t cin, int32_t cout, int32_t w_exp, void* packed,
                                          void* stream) {
    return pack_parity_h3("pack_weights_convt_h3", keras_kernel, SRC_CONVT, dm3d_conv_weight_layout(4, 2, 0, 1, cout), cin, cout, w_exp, packed,
                          stream);
}

// ---- DM3D_WL_PAIR images ---------------------------------------------------------------------------------------------------------------
extern "C" int64_t dm3d_packed_weight_h3p_bytes(int32_t taps, int32_t cin, int32_t cout) {
    return positive(taps, cin, cout) ? pair_geom(taps, cin, cout).bytes() : 0;
}

extern "C" int dm3d_pack_weights_h3p(const float* keras_kernel, int32_t taps, int32_t cin, int32_t cout, int32_t w_exp,
                                     const float* in_scale, void* packed, int32_t mode, void* stream) {
    DM3D_REQUIRE(mode >= 0 && mode <= 2 && (mode == 0 || taps == 8), "pack_weights_h3p: mode %d with taps %d", mode, taps);
    return pack_h3("pack_weights_h3p", keras_kernel, mode, DM3D_WL_PAIR, taps, pair_geom(taps, cin, cout), cin, cout, w_exp, in_scale, packed,
                   stream);
}

extern "C" int64_t dm3d_packed_weight_h3w_bytes(int32_t cin, int32_t cout) {
    return positive(cin, cout) ? pair_geom(40, cin, cout).bytes() : 0;          // 5 tap pairs x 4 transform terms x 2 taps
}

extern "C" int dm3d_pack_weights_h3w(const float* keras_kernel, int32_t cin, int32_t cout, int32_t w_exp, const float* in_scale, void* packed,
                                     void* stream) {
    return pack_h3("pack_weights_h3w", keras_kernel, SRC_WINO, DM3D_WL_PAIR, 40, pair_geom(40, cin, cout), cin, cout, w_exp, in_scale, packed,
                   stream);
}

extern "C" int64_t dm3d_packed_weight_skip_h3p_bytes(int32_t cin, int32_t cout) {
    return positive(cin, cout) ? skip_geom(cin, cout).bytes() : 0;
}

extern "C" int dm3d_pack_weights_skip_h3p(const float* keras_kernel, int32_t cin, int32_t cout, int32_t w_exp, void* packed, void* stream) {
    return pack_h3("pack_weights_skip_h3p", keras_kernel, SRC_PLAIN, DM3D_WL_PAIR, 1, skip_geom(cin, cout), cin, cout, w_exp, nullptr, packed,
                   stream);
}

extern "C" int dm3d_pack_weights_skip_h3f(const float* keras_kernel, int32_t cin, int32_t cout, int32_t w_exp, void* packed, void* stream) {
    if (int rc = pack_check("pack_weights_skip_h3f", keras_kernel, packed, 1, cin, cout, w_exp, true)) return rc;
    const H3Geom g = skip_geom(cin, cout);
    const Src s{keras_kernel, nullptr, cin, cout, SRC_PLAIN, ldexpf(1.0f, w_exp)};
    return launch_pack("pack_weights_skip_h3f", pack_skip_h3f_kernel, g.records() * REC, stream, s, g.nchunks / 2, g.ntiles,
                       static_cast<_Float16*>(packed));
}
