// digest.hpp -- the leaf hashes of the V2 tree digests (include/zkp.h, "tree
// digests"), one lane per leaf of 256 points.  digest.hip
// holds the kernels, the host twin and the C ABI.
//
//   leaf(g, P[0..m)) = SHA-256( B0 | enc(P[0]) | ... | enc(P[m-1]) ),  1 <= m <= 256
//   B0 = "ZKAMD-LEAF-V2" | byte(g) | be16(m) | 48 zero bytes           (one block)
//
// Shape of a lane's work.  enc (zk_g1_compress / zk_g2_compress) never exists
// as bytes: the big-endian words of an Fq are the halves of its limbs from the
// top down, which for a point read as 32-bit words u[0..] is u[EW - 1 - j] for
// encoding word j (G2: x.c1 lies above x.c0 in the struct and comes first in
// the encoding, so the one rule covers both groups).  The flags go into the
// top byte of word 0.  B0 puts the points on a block boundary, so four G1
// encodings (4 x 12 words) or two G2 encodings (2 x 24 words) are exactly
// three blocks: the main loop is that unit, written out, and a tail takes the
// m mod 4 / m mod 2 points left with the padding.  Every array below is indexed
// by constants after unrolling, so the words stay in VGPRs as sha256.hpp's do
// (0 bytes of scratch; the build's resource remarks are in DESIGN.md 2.22).
//
// Loads.  A lane's leaf is 256 consecutive structs (26 KB / 50 KB from the
// next lane's), and a unit of it -- 416 B for G1, 400 B for G2 -- starts on a
// 16-byte boundary because 256 structs do: the unit is 26 / 25 16-byte loads.
// The tail's points are 8-byte aligned only and load as 8-byte pairs.
#pragma once
#include "../../include/zkp.h"
#include "constants.hpp"
#include "sha256.hpp"

namespace zk {

constexpr size_t DIGEST_LEAF = 256;       // points per leaf
constexpr int DG_BLOCK = 64;              // lanes (leaves) per block: one wave, so a chunk's leaves spread over the CUs
constexpr size_t DG_TAG_LEN = 13;
static constexpr uint8_t DG_TAG[DG_TAG_LEN + 1] = "ZKAMD-LEAF-V2";

#if defined(__HIPCC__)
template <int K>   // 1: G1, 2: G2
struct DgShape {
  static constexpr int W = 24 * K + 2;      // 32-bit words of an ABI struct (104 / 200 bytes)
  static constexpr int EW = 12 * K;         // words of an encoding
  static constexpr int PER = 4 / K;         // points of a three-block unit
  static constexpr int UW = PER * W;        // words of a unit: 104 / 100
  static constexpr int TB = K == 1 ? 3 : 2; // blocks the tail can need
  static_assert(PER * EW == 48 && UW % 4 == 0, "a unit is three blocks and whole 16-byte loads");
};

// the sort flag on a canonical value: c > (p - 1) / 2, by one borrow chain
__device__ __forceinline__ bool dg_largest(const uint32_t* c) {
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) (void)__builtin_subc(FQ_PM1_DIV2_32[i], c[i], br, &br);
  return br != 0;
}
__device__ __forceinline__ bool dg_is_zero(const uint32_t* c) {
  uint32_t x = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) x |= c[i];
  return x == 0;
}

// enc of the point whose struct words are u[0..W) -> e[0..EW).  What the host
// encoder does and no more: any non-zero infinity byte is the identity
// (0xc0, zeros) whatever the coordinates hold, and nothing is validated.
template <int K>
__device__ __forceinline__ void dg_encode(const uint32_t* u, uint32_t* e) {
  using S = DgShape<K>;
  const bool inf = (u[S::W - 2] & 0xffu) != 0;
  const uint32_t* y = u + S::EW;   // y (G2: y.c0, then y.c1)
  bool big;
  if (K == 1) big = dg_largest(y);
  else big = dg_is_zero(y + 12) ? dg_largest(y) : dg_largest(y + 12);
#pragma unroll
  for (int j = 0; j < S::EW; j++) e[j] = inf ? 0u : u[S::EW - 1 - j];
  e[0] = inf ? 0xc0000000u : (e[0] | 0x80000000u | (big ? 0x20000000u : 0u));
}

__device__ __forceinline__ Sha256Block dg_block(const uint32_t* w) {
  return {w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], w[10], w[11], w[12], w[13], w[14], w[15]};
}

// st <- st over the three blocks of one unit, u its UW struct words
template <int K>
__device__ __forceinline__ void dg_unit(uint32_t st[8], const uint32_t* u) {
  using S = DgShape<K>;
  uint32_t e[48];
#pragma unroll
  for (int k = 0; k < S::PER; k++) dg_encode<K>(u + S::W * k, e + S::EW * k);
  sha256_compress(st, dg_block(e));
  sha256_compress(st, dg_block(e + 16));
  sha256_compress(st, dg_block(e + 32));
}

// The tail of a leaf of m points: the r = m mod PER points at q, 0x80, zeros
// and the bit length in the last two words of block nb - 1.  Every position is
// a constant under a comparison with r.
template <int K>
__device__ __forceinline__ void dg_tail(uint32_t st[8], const uint2* __restrict__ q, uint32_t m) {
  using S = DgShape<K>;
  const uint32_t r = m % S::PER;
  const uint32_t nb = (r * S::EW + 3 + 15) / 16;
  uint32_t e[16 * S::TB];
#pragma unroll
  for (int j = 0; j < 16 * S::TB; j++) e[j] = 0;
#pragma unroll
  for (int k = 0; k < S::PER - 1; k++) {
    if ((uint32_t)k < r) {
      uint32_t u[S::W];
#pragma unroll
      for (int i = 0; i < S::W / 2; i++) {
        const uint2 v = q[(S::W / 2) * k + i];
        u[2 * i] = v.x; u[2 * i + 1] = v.y;
      }
      dg_encode<K>(u, e + S::EW * k);
    }
  }
#pragma unroll
  for (int k = 0; k < S::PER; k++)
    if (r == (uint32_t)k) e[S::EW * k] = 0x80000000u;
#pragma unroll
  for (int b = 1; b <= S::TB; b++)
    if (nb == (uint32_t)b) e[16 * b - 1] = 8u * (64u + 4u * S::EW * m);
#pragma unroll 1
  for (uint32_t b = 0; b < nb; b++) {
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      w[j] = e[j];
      if (b == 1) w[j] = e[16 + j];
      if (S::TB > 2 && b == 2) w[j] = e[16 * (S::TB - 1) + j];
    }
    sha256_compress(st, dg_block(w));
  }
}

__device__ __forceinline__ void dg_store(const uint32_t st[8], uint8_t* __restrict__ out) {
  uint4* o = reinterpret_cast<uint4*>(out);
  o[0] = make_uint4(__builtin_bswap32(st[0]), __builtin_bswap32(st[1]), __builtin_bswap32(st[2]),
                    __builtin_bswap32(st[3]));
  o[1] = make_uint4(__builtin_bswap32(st[4]), __builtin_bswap32(st[5]), __builtin_bswap32(st[6]),
                    __builtin_bswap32(st[7]));
}

// the state after B0: "ZKAM" "D-LE" "AF-V" '2' byte(g) be16(m), 48 zero bytes
template <int K>
__device__ __forceinline__ void dg_begin(uint32_t st[8], uint32_t m) {
  sha256_init(st);
  sha256_compress(st, {0x5a4b414du, 0x442d4c45u, 0x41462d56u, 0x32000000u | ((uint32_t)K << 16) | m, 0, 0, 0, 0, 0,
                       0, 0, 0, 0, 0, 0, 0});
}

// Leaf `leaf` (256 leaf < n) of the n points at pts (16-byte aligned) -> 32
// bytes at out + 32 leaf.
template <int K>
__device__ __forceinline__ void dg_leaf_lane(const uint64_t* __restrict__ pts, size_t n, size_t leaf,
                                             uint8_t* __restrict__ out) {
  using S = DgShape<K>;
  const size_t lo = DIGEST_LEAF * leaf;
  const uint32_t m = (uint32_t)(n - lo < DIGEST_LEAF ? n - lo : DIGEST_LEAF);
  uint32_t st[8];
  dg_begin<K>(st, m);
  const uint32_t units = m / S::PER;
  const uint4* p = reinterpret_cast<const uint4*>(pts + (size_t)(S::W / 2) * lo);
  for (uint32_t it = 0; it < units; it++, p += S::UW / 4) {
    uint32_t u[S::UW];
#pragma unroll
    for (int i = 0; i < S::UW / 4; i++) {
      const uint4 v = p[i];
      u[4 * i] = v.x; u[4 * i + 1] = v.y; u[4 * i + 2] = v.z; u[4 * i + 3] = v.w;
    }
    dg_unit<K>(st, u);
  }
  dg_tail<K>(st, reinterpret_cast<const uint2*>(p), m);
  dg_store(st, out + 32 * leaf);
}
#endif   // __HIPCC__

}  // namespace zk

struct zk_ctx;
namespace zk {
// 32 ceil(n / 256) bytes of leaf digests: through the GPU in chunks of whole
// leaves (digest.hip), or by the host twin
int leaf_digests_run(zk_ctx* ctx, bool g2, const void* pts, size_t n, uint8_t* out);
void leaf_digests_host(bool g2, const void* pts, size_t n, uint8_t* out);
}  // namespace zk
