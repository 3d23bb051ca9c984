// kernel_shapes.h -- which instantiations of the width-templated kernels exist: one X-macro list per kernel family, and nothing else.
// Everything that enumerates a family is generated from its list -- the explicit instantiations (inst_scan_valu.hip,
// inst_scan_mfma.hip), the launch switches, the "has this width a kernel" predicates, the tile geometry and the dynamic-LDS
// attributes (host_launch.h, host_query.h, host_build.h, inst_small_filt.hip) -- so a width, an NT or a CPL is added, dropped or
// changed HERE and nowhere else.  W = dim / 64 throughout.  The lists need the RQ_NT_* constants of kernels_scan_decl.h where they
// are expanded, and nothing besides: the header is included by the host unit and by the inst_*.hip units alike.
#pragma once

// VALU scan, scan_kernel<W, CPL, ARENA, FILT>: (W, CPL = candidates per lane; the tile is 256 * CPL candidates)
#define RQ_SCAN_VALU_SHAPES(X) X(1, 2) X(2, 2) X(3, 2) X(4, 2) X(6, 2) X(8, 2) X(12, 1) X(16, 1)
// matrix-core scan, scan_mfma_kernel<W, NT, ARENA, false, FILT>: (W, NT = 32-candidate sub-tiles per wave)
#define RQ_SCAN_MFMA_SHAPES(X) X(1, 4) X(2, RQ_NT_W2) X(3, 4) X(4, 2) X(6, 2) X(8, 2) X(12, RQ_NT_W12) X(16, 2)
// ... with the additive gate, scan_mfma_kernel<W, NT, false, true> (dim 64 / 128, uniform survivor buffers)
#define RQ_SCAN_MFMA_ADD_SHAPES(X) X(1, 4) X(2, RQ_ADD_NT2)
// the bf16 tile kernels assign_approx_kernel<W, NT> and coarse_approx_kernel<W, NT>: (W, NT = 32-row tiles per wave)
#define RQ_BF16_TILE_SHAPES(X) X(1, 2) X(2, 2) X(3, 1) X(4, 1) X(6, 1) X(8, 1) X(12, 1)
// coarse_candidates_kernel<W, NT>: two query tiles per wave where their tile keys fit in LDS, else one (the launcher's rule picks
// between the two shapes of a width; widths 3 and 4 have the one)
#define RQ_COARSE_CAND_SHAPES(X) X(1, 2) X(2, 2) X(1, 1) X(2, 1) X(3, 1) X(4, 1)
// sb_query_kernel<W, mode, FILT>: the widths with a small-batch path
#define RQ_SMALL_BATCH_WIDTHS(X) X(1) X(2) X(4) X(8) X(12) X(16)
// accurate_ring8_kernel<RQ_RING_V, NPC>: NPC = dim / 16, the 16-byte pieces of an 8-bit shadow row
#define RQ_RING8_NPC(X) X(4) X(8) X(12) X(16)

// `switch (w) { RQ_..._SHAPES(RQ_SHAPE_CASE) return true; default: return false; }`: membership in a list by its first column
#define RQ_SHAPE_CASE(W, ...) case W:
