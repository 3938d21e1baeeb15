// dm3d_conv_h3_host.hip — what the two 16x16x32 split-float16 Conv3d kernels (dm3d_conv_h3v3.hip: the free-running direct kernel;
// dm3d_conv_h3w.hip: its Winograd-x form) share on the host side around the launch itself.
//   * pre_launch / post_launch turn a resolved ConvLaunch (dm3d_conv_args.h; the decision — brick depth, Cin split, tile sizes, workspace
//     needs — is made in dm3d_conv_resolve, dm3d_conv.hip, not here) into the kernel's own arguments: bricks per volume, the split fields
//     of the hand-over form (raw partial tiles into caller scratch, the last part of a tile to arrive sums them and runs the epilogue —
//     one launch, no zero fill, no atomics on the output, no reduce launch), 16-byte epilogue eligibility, and where the
//     GroupNormalization statistics come from.
// (The weight images these kernels read are made in dm3d_pack.hip.)
#include "dm3d_conv_h3v2_parts.h"

using namespace h3v2;

int dm3d_h3v2_pre_launch(const ConvLaunch& r, H3v2Launch& L) {
    ConvArgs& k = L.k;
    k = r.a;
    k.bd = (k.od + r.td - 1) / r.td; k.bh = (k.oh + 7) / 8; k.bw = (k.ow + 7) / 8;
    k.ksplit = r.ksplit;
    auto al16 = [](const void* q) { return (reinterpret_cast<size_t>(q) & 15) == 0; };
    k.epi_vec4 = k.cout % 4 == 0 && al16(k.out) && al16(k.bias) && al16(k.res) && al16(k.prelu) && al16(k.post_scale) && al16(k.post_shift)
                 && al16(k.vec) && (k.vec == nullptr || k.vec_ld % 4 == 0);
    k.split_tile_floats = 0;
    if (r.ksplit > 1) {                 // the hand-over form (split_* in dm3d_conv_h3v2_parts.h): the parts meet inside the launch
        k.split_tile_floats = r.tile_floats;
        DM3D_REQUIRE(k.split_counters && k.split_counter_words >= r.need_words, "conv: a Cin-split launch of %ld tiles needs split_counters of as many zeroed words (have %d)",
                     r.tiles, k.split_counter_words);
        DM3D_REQUIRE(k.scratch && (size_t)k.scratch_bytes >= (size_t)r.need_bytes,
                     "conv: scratch of %ld bytes is too small for %d parts x %ld tiles (dm3d_conv_scratch_bytes)", k.scratch_bytes, r.ksplit, r.tiles);
        DM3D_REQUIRE((size_t)r.ksplit * r.tile_floats * sizeof(float) < (1ull << 31), "conv: %d parts overflow a tile's buffer descriptor", r.ksplit);
    }
    // Fused GroupNormalization statistics: the kernel's 16-byte full-brick epilogue accumulates them (whole bricks, cout % 64 == 0, plain
    // float32 output without PReLU; a split launch's last part runs that epilogue like any other); every other form leaves them to the
    // stand-alone kernel behind the launch (post_launch).
    L.stats_after = false;
    if (k.gn_stats) {
#ifdef DM3D_EPILOGUE_SCALAR
        const bool fused = false;            // (that A/B build compiles the 16-byte epilogue — the only form that accumulates — out)
#else
        const bool fused = k.od % r.td == 0 && k.oh % 8 == 0 && k.ow % 8 == 0 && k.cout % 64 == 0 && k.epi_vec4 && !k.prelu
                           && !k.out_h2 && !k.post_scale;
#endif
        if (!fused) { k.gn_stats = nullptr; L.stats_after = true; }
    }
    return DM3D_OK;
}

int dm3d_h3v2_post_launch(const ConvArgs& a, const H3v2Launch& L, hipStream_t st) {
    if (L.stats_after) return dm3d_groupnorm_partials(a.out, a.batch, (int64_t)a.fd * a.fh * a.fw, a.cout, a.gn_stats, st);
    return DM3D_OK;
}
