// dm3d_frag.h — the parts of the transposed fragment-stream product shared by dm3d_attn_front_h3.hip and dm3d_mlp_h3.hip.
//
// The scheme.  A workgroup (4 waves, one per SIMD) owns 32 or 64 rows; every product is computed TRANSPOSED, out^T = W . in^T: the weights
// are the MFMA's A operand and arrive as PRE-TILED operand fragments, 1 KB per (32-row tile, 16-k record, hi | lo), lane-ordered
// (dm3d_tile_weights), by plain coalesced 16-byte loads straight into registers a group of 8 fragments ahead of their MFMAs — no wave needs
// another wave's weights, so they never touch LDS; the input rows are the B operand, read from an LDS image of DM3D_FMT_H2 records.
// Wave w owns output columns 64 w .. 64 w + 63 as 2 column tiles of 32; a lane (l32, half) then holds, in registers 4 gq .. 4 gq + 3 of tile
// (mr, nr), columns col0 .. col0 + 3 of row 32 mr + l32: 16-byte float32 / 8 + 8-byte H2 accesses, no transposes.
//
// The record layout (dm3d_h3.h) as these kernels address it.  A DM3D_FMT_H2 row in memory is a sequence of 64-byte records; an LDS image is
// [record][row][64 B] with `rs` bytes between records (TM * 64, or + 32 so that row-major stores spread over the banks) and logical slot s
// of row r at physical slot s ^ swz(r).  Columns n0 .. n0 + 3: record n0 >> 4, slot (n0 >> 3) & 1 (lo: + 2), bytes 2 (n0 & 7) .. + 7.
// What issues the MFMA stays with each kernel (the builtin in one, asm with its pads in the other: their comments): dm3d_kstep takes it as
// a callable.
#pragma once
#include "dm3d_h3.h"
#include <type_traits>

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <int N, int I = 0, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, I + 1>(f);
    }
}

// raw barrier behind this wave's own LDS traffic (never drains the vector-memory counter: weight loads and DMA fills stay in flight across it)
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// hi = f16(x) (RNE), lo = f16(x - hi) of two values (dm3d_h3.h split8's instruction sequence)
__device__ __forceinline__ void dm3d_split2(float x0, float x1, unsigned int& hi, unsigned int& lo) {
    float r0, r1;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(hi) : "v"(x0), "v"(x1));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(hi), "v"(x0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(hi), "v"(x1));
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(lo) : "v"(r0), "v"(r1));
}
__device__ __forceinline__ float dm3d_clamp16(float v) { return __builtin_amdgcn_fmed3f(v, -65504.0f, 65504.0f); }

// ---- lane mapping: first of the four (col0) / eight (col8) consecutive columns behind registers 4 gq .. 4 gq + 3 of column tile nr
__device__ __forceinline__ int dm3d_col0(int wave, int nr, int gq, int half) { return wave * 64 + nr * 32 + 8 * gq + 4 * half; }
__device__ __forceinline__ int dm3d_col8(int wave, int nr, int gq) { return wave * 64 + nr * 32 + 8 * gq; }

// ---- record layout: B-operand fragment of a lane's row in one record of an LDS image: logical slot `half` (hi; lo: ^ 32), swizzled by the row
__device__ __forceinline__ unsigned dm3d_frag_off(int row, int half) { return (unsigned)(row * 64 + ((swz(row) ^ half) << 4)); }
// ---- weight stream: one group = 8 consecutive 1 KB fragments of this lane's stream (src: the group's first fragment + 16 lane)
__device__ __forceinline__ void dm3d_load_group(h8 (&w)[8], const char* src) {
#pragma unroll
    for (int t = 0; t < 8; ++t) w[t] = *reinterpret_cast<const h8*>(src + t * 1024);
}

// ---- the K step: one 16-k record into the 2 x MR tiles, acc[mr][nr] += W[nr] . in[mr]^T as W_hi . in_lo, W_lo . in_hi, W_hi . in_hi.
// w: the record's fragments [nr][hi | lo]; ih / il: the input's B fragments per row tile.  Pass-major over the tiles (a 32x32x16 that depends
// on the one issued just before it waits out its latency).  SWAP: the MFMA operands exchanged (the two fragment layouts are identical), which
// leaves acc^T: lane = column, registers = rows.  mfma(acc, a, b): the caller's instruction.
template <int MR, bool SWAP, class M>
__device__ __forceinline__ void dm3d_kstep(f32x16 (&acc)[MR][2], const h8* w, const h8 (&ih)[MR], const h8 (&il)[MR], M&& mfma) {
    auto mm = [&](f32x16& c, const h8& wf, const h8& in) __attribute__((always_inline)) {
        if constexpr (SWAP) mfma(c, in, wf); else mfma(c, wf, in);
    };
#pragma unroll
    for (int t = 0; t < 2 * MR; ++t) mm(acc[t >> 1][t & 1], w[2 * (t & 1)], il[t >> 1]);
#pragma unroll
    for (int t = 0; t < 2 * MR; ++t) mm(acc[t >> 1][t & 1], w[2 * (t & 1) + 1], ih[t >> 1]);
#pragma unroll
    for (int t = 0; t < 2 * MR; ++t) mm(acc[t >> 1][t & 1], w[2 * (t & 1)], ih[t >> 1]);
}

// ---- host: DM3D_FMT_H2 weight rows (`pitch` bytes each) -> operand fragments [block][wave][record][column tile nr][hi | lo][lane][16 B].
// Wave w of block b takes rows b * row_step + 32 nr_tiles w .. and records b * rec_step .. + recs - 1 of them: the blocks split the rows
// (rec_step = 0) or k (row_step = 0).  total: 16-byte pieces of the image.  (dm3d_attn_front_h3.hip)
int dm3d_tile_weights(const void* w_h2, void* tiled, long total, int pitch, int nr_tiles, int recs, int row_step, int rec_step, void* stream);
