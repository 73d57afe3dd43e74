// What the host and the kernels of the column-strip chain generation (chain_t.hpp) have to agree on: the instantiated shapes
// and the LDS footprint of each kernel.  Included by chain_t.hpp (static_asserts, LDS arrays) and chain_t.hip (host predicates).
#pragma once

namespace gc {

// (gh, L) pairs the templates are instantiated for: the reference's model (64, 2), cfg 2's width (128, 2), cfg 3 (192, 4),
// and the neighbours a user is most likely to configure.  Four translation units (chain_t_u0 .. u3.hip) share them so that
// the build runs them side by side; X(gh, L, unit)
#define GC_CHAIN_T_SHAPES(X) \
  X(32, 2, 0) X(32, 4, 0) X(64, 1, 0) X(64, 2, 0) X(64, 3, 0) X(64, 4, 0) \
  X(128, 1, 1) X(128, 2, 1) X(128, 3, 1) X(128, 4, 1) \
  X(192, 2, 2) X(192, 4, 2) \
  X(256, 1, 3) X(256, 2, 3)

constexpr bool t_instantiated(int gh, int L) {
  bool yes = false;
#define X(gh_, l_, u_) yes = yes || (gh == gh_ && L == l_);
  GC_CHAIN_T_SHAPES(X)
#undef X
  return yes;
}

constexpr int T_LA = 68;  // row pitch of the 64 x 64 adjacency image (16-byte rows, conflict-free 16-byte reads)

// forward: adjacency image | Y image + two weight stages per later sub-layer (the attention core's scratch lies over them) | rinv
constexpr int t_fwd_room(int GH, int L) { return 64 * (GH + 4) + 2 * (L - 1) * 16 * (GH + 4); }
constexpr int t_fwd_lds(int GH, int L) { return 64 * T_LA + t_fwd_room(GH, L) + 64; }
constexpr int t_bwd_lds(int GH) { return 64 * T_LA + 2 * 64 * (GH + 4) + (GH / 16) * 64 + 128; }
// FUSE (the output projection's input gradient computed by the backward kernel itself): the dout image [64][D + 4] and two
// 16-deep stages of Wlin's slice lie over the dM / Pn images (used only afterwards); behind the row-sum areas the K slices of
// the residual gradient meet
constexpr int t_max(int a, int b) { return a > b ? a : b; }
constexpr int t_bwd_region(int GH, int L) { return t_max(2 * 64 * (GH + 4), 96 * (L * GH + 4)); }
constexpr int t_bwd_fuse_lds(int GH, int L) { return 64 * T_LA + t_bwd_region(GH, L) + (GH / 16) * 64 + 128 + (GH / 16) * 1024; }
// wider blocks: the images do not fit (and the product is a launch's worth); L = 3: the image pieces do not divide over the threads
constexpr bool t_fuse_shape(int GH, int L) { return L * GH <= 256 && GH <= 128 && 16 % L == 0; }

}  // namespace gc
