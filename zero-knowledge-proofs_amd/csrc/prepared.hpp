// prepared.hpp -- a verification key prepared once and kept on the device
// (zk_vk_dev, include/zkp.h "prepared verification keys"):
// the per-key words the batch verification calls otherwise make per call
// (pairing.hip's pairing_tables) and a window table of ic_g1[1..num_public],
// from which the public-input sums IC = ic[0] + sum x_k ic[k + 1] are a few
// mixed additions per input (prepared.hip) instead of a double-and-add walk.
//
// The table: for window width b and W = ceil(bits / b) windows (bits = 255 for
// a sound key, 64 in reference mode), entry ((k W + w) E + j - 1), E = 2^b - 1,
// holds [j 2^(b w)] ic[k + 1] for j = 1 .. E as a device affine point.  b
// divides 64, so a digit never straddles two words of an input.
#pragma once
#include <algorithm>

#include "ctx.hpp"

namespace zk {

// The most bytes a key's window table may take.  b = 8 gives the fewest
// additions per input (32 in sound mode) at 783 360 B per input; under this
// bound that serves 685 inputs, b = 4 (64 additions, 92 160 B) 5 825, b = 2
// 14 563 and b = 1 21 931 -- half a GiB keeps every table a small part of
// the device's memory while no circuit in ordinary use leaves b = 8.
constexpr uint64_t PREP_TABLE_MAX = 512ull << 20;
// Lanes that fill the GPU with one wave per SIMD: ZK_OPT_VERIFY_CHUNK's default
constexpr uint64_t PREP_FILL = 65536;
// XYZZ entries (192 B, plus 48 B of the normalisation's prefix products) one
// pass of the table build holds before they are normalised into the table
constexpr uint64_t PREP_BUILD_MAX = 256ull << 20;

inline int prep_windows(bool sound, int b) { return ((sound ? 255 : 64) + b - 1) / b; }
inline uint64_t prep_table_bytes(bool sound, uint64_t num_public, int b) {
  return num_public * (uint64_t)prep_windows(sound, b) * ((1ull << b) - 1) * 96;
}
// The window width of a key: the widest of 8, 4, 2, 1 whose table stays within
// PREP_TABLE_MAX; 0 when none does.
inline int prep_width(bool sound, uint64_t num_public) {
  if (num_public > (1ull << 24)) return 0;
  for (int b = 8; b >= 1; b >>= 1)
    if (prep_table_bytes(sound, num_public, b) <= PREP_TABLE_MAX) return b;
  return 0;
}
// Table additions one lane of the sums' first level makes in sequence, for a
// chunk of m proofs whose sums have T = num_public W terms each.  Small m: the
// square root of T, so that a lane of either level adds about as many points
// in sequence; as m grows the runs lengthen so that the first level stays near
// PREP_FILL lanes; from PREP_FILL proofs on a lane takes its whole proof and
// there is no second level.  Never below 1, never above max(T, 1).
inline uint64_t prep_run_len(uint64_t m, uint64_t num_public, int windows) {
  const uint64_t T = num_public * (uint64_t)windows;
  if (T <= 1) return 1;
  if (m >= PREP_FILL) return T;
  uint64_t s = 1;
  while (s * s < T) s++;
  const uint64_t fill = (T * m + PREP_FILL - 1) / PREP_FILL;
  return std::min(T, std::max(s, fill));
}
// words of the key's fixed part (pairing.hpp's VK_* layout) for num_public inputs
uint64_t prep_words(uint64_t num_public);

// The buffers of one chunk of sums: per proof the sum as a device affine point
// ((0, 0) the identity) and whether every input was in range.
struct PrepWork {
  DevBuf part, sum, pre, ic, ok;
};
// IC of m rows of inputs in device memory -> w.ic (m G1A) and w.ok (m bytes), on st
void prepared_sums_launch(zk_ctx* ctx, hipStream_t st, const zk_vk_dev* pvk, const uint64_t* d_in, size_t m,
                          PrepWork& w);

}  // namespace zk

struct zk_vk_dev {
  int device = 0;
  bool sound = false;
  uint64_t num_public = 0;
  int width = 0, windows = 0;     // b and W of the table
  uint64_t bytes = 0;             // device bytes the key holds
  zk::DevBuf words;               // pairing.hpp's VK_* words, ic_g1[0 .. num_public] included
  zk::DevBuf table;               // the window table of ic_g1[1 ..]
};
