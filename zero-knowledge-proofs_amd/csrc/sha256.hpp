// sha256.hpp -- SHA-256 (FIPS 180-4) for the hash to G2 (hash.hpp) and the
// transcript digests (hash.hip): one compression function for host and device
// and an incremental host context.
//
// Shape of the compression.  The 64 rounds are written out (no loop), the
// 16-word message schedule is sixteen named values w0 .. w15 updated in place,
// and the eight working variables rotate by renaming instead of by moves.
// Nothing is indexed at run time, so on the device everything stays in VGPRs
// (a runtime-indexed array would live in scratch memory).  A rotate is
// __builtin_rotateright32, which the gfx950 back end selects as one
// v_alignbit_b32 with both sources the same register.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZK_SHA_HD __host__ __device__ __forceinline__
#else
#define ZK_SHA_HD inline
#endif

namespace zk {

ZK_SHA_HD uint32_t sha_rotr(uint32_t x, int n) { return __builtin_rotateright32(x, (uint32_t)n); }
ZK_SHA_HD uint32_t sha_bsig0(uint32_t x) { return sha_rotr(x, 2) ^ sha_rotr(x, 13) ^ sha_rotr(x, 22); }
ZK_SHA_HD uint32_t sha_bsig1(uint32_t x) { return sha_rotr(x, 6) ^ sha_rotr(x, 11) ^ sha_rotr(x, 25); }
ZK_SHA_HD uint32_t sha_ssig0(uint32_t x) { return sha_rotr(x, 7) ^ sha_rotr(x, 18) ^ (x >> 3); }
ZK_SHA_HD uint32_t sha_ssig1(uint32_t x) { return sha_rotr(x, 17) ^ sha_rotr(x, 19) ^ (x >> 10); }

// the sixteen big-endian words of one 64-byte block
struct Sha256Block {
  uint32_t w0, w1, w2, w3, w4, w5, w6, w7, w8, w9, w10, w11, w12, w13, w14, w15;
};

ZK_SHA_HD void sha256_init(uint32_t st[8]) {
  st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au;
  st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
}

// one round: h and d change, the caller renames the variables
#define ZK_SHA_RND(a, b, c, d, e, f, g, h, k, w)                           \
  {                                                                        \
    const uint32_t t1_ = h + sha_bsig1(e) + ((e & f) ^ (~e & g)) + k + w;  \
    const uint32_t t2_ = sha_bsig0(a) + ((a & b) ^ (a & c) ^ (b & c));     \
    d += t1_;                                                              \
    h = t1_ + t2_;                                                         \
  }
// the schedule word sixteen places on: w[t] = ssig1(w[t-2]) + w[t-7] + ssig0(w[t-15]) + w[t-16]
#define ZK_SHA_EXP(wt, wm2, wm7, wm15) wt += sha_ssig1(wm2) + wm7 + sha_ssig0(wm15)
// eight rounds on eight consecutive schedule words
#define ZK_SHA_RND8(k0, k1, k2, k3, k4, k5, k6, k7, x0, x1, x2, x3, x4, x5, x6, x7) \
  ZK_SHA_RND(a, b, c, d, e, f, g, h, k0, x0)                                       \
  ZK_SHA_RND(h, a, b, c, d, e, f, g, k1, x1)                                       \
  ZK_SHA_RND(g, h, a, b, c, d, e, f, k2, x2)                                       \
  ZK_SHA_RND(f, g, h, a, b, c, d, e, k3, x3)                                       \
  ZK_SHA_RND(e, f, g, h, a, b, c, d, k4, x4)                                       \
  ZK_SHA_RND(d, e, f, g, h, a, b, c, k5, x5)                                       \
  ZK_SHA_RND(c, d, e, f, g, h, a, b, k6, x6)                                       \
  ZK_SHA_RND(b, c, d, e, f, g, h, a, k7, x7)
// the next sixteen schedule words, in place
#define ZK_SHA_EXP16()                                                                       \
  ZK_SHA_EXP(m.w0, m.w14, m.w9, m.w1);   ZK_SHA_EXP(m.w1, m.w15, m.w10, m.w2);                \
  ZK_SHA_EXP(m.w2, m.w0, m.w11, m.w3);   ZK_SHA_EXP(m.w3, m.w1, m.w12, m.w4);                 \
  ZK_SHA_EXP(m.w4, m.w2, m.w13, m.w5);   ZK_SHA_EXP(m.w5, m.w3, m.w14, m.w6);                 \
  ZK_SHA_EXP(m.w6, m.w4, m.w15, m.w7);   ZK_SHA_EXP(m.w7, m.w5, m.w0, m.w8);                  \
  ZK_SHA_EXP(m.w8, m.w6, m.w1, m.w9);    ZK_SHA_EXP(m.w9, m.w7, m.w2, m.w10);                 \
  ZK_SHA_EXP(m.w10, m.w8, m.w3, m.w11);  ZK_SHA_EXP(m.w11, m.w9, m.w4, m.w12);                \
  ZK_SHA_EXP(m.w12, m.w10, m.w5, m.w13); ZK_SHA_EXP(m.w13, m.w11, m.w6, m.w14);               \
  ZK_SHA_EXP(m.w14, m.w12, m.w7, m.w15); ZK_SHA_EXP(m.w15, m.w13, m.w8, m.w0);
#define ZK_SHA_RND16(k0, k1, k2, k3, k4, k5, k6, k7, k8, k9, k10, k11, k12, k13, k14, k15)             \
  ZK_SHA_RND8(k0, k1, k2, k3, k4, k5, k6, k7, m.w0, m.w1, m.w2, m.w3, m.w4, m.w5, m.w6, m.w7)          \
  ZK_SHA_RND8(k8, k9, k10, k11, k12, k13, k14, k15, m.w8, m.w9, m.w10, m.w11, m.w12, m.w13, m.w14, m.w15)

// st <- compress(st, block); m is the caller's copy and is used up
ZK_SHA_HD void sha256_compress(uint32_t st[8], Sha256Block m) {
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
  ZK_SHA_RND16(0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
               0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u)
  ZK_SHA_EXP16()
  ZK_SHA_RND16(0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
               0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u)
  ZK_SHA_EXP16()
  ZK_SHA_RND16(0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
               0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u)
  ZK_SHA_EXP16()
  ZK_SHA_RND16(0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
               0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u)
  st[0] += a; st[1] += b; st[2] += c; st[3] += d;
  st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}
#undef ZK_SHA_RND
#undef ZK_SHA_EXP
#undef ZK_SHA_RND8
#undef ZK_SHA_EXP16
#undef ZK_SHA_RND16

// Block `blk` of a message of `total` bytes with its padding (0x80, zeros, the
// bit length in the last eight bytes of the last block), the message given as
// a byte getter: src(pos) for pos < total.  The word loop unrolls, so the
// sixteen words are registers.
template <class Src>
ZK_SHA_HD Sha256Block sha256_block_of(const Src& src, size_t total, size_t blk) {
  uint32_t w[16];
  const size_t nblocks = (total + 9 + 63) / 64;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const size_t pos = 64 * blk + 4 * j + k;
      const uint32_t byte = pos < total ? (uint32_t)src(pos) : pos == total ? 0x80u : 0u;
      v = (v << 8) | byte;
    }
    w[j] = v;
  }
  if (blk + 1 == nblocks) {
    const uint64_t bits = (uint64_t)total * 8;
    w[14] = (uint32_t)(bits >> 32);
    w[15] = (uint32_t)bits;
  }
  return {w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], w[10], w[11], w[12], w[13], w[14], w[15]};
}
// the whole hash of such a message: digest words (big-endian values) in st
template <class Src>
ZK_SHA_HD void sha256_of(const Src& src, size_t total, uint32_t st[8]) {
  sha256_init(st);
  const size_t nblocks = (total + 9 + 63) / 64;
  for (size_t blk = 0; blk < nblocks; blk++) sha256_compress(st, sha256_block_of(src, total, blk));
}

// ---- incremental context (host) ------------------------------------------------
struct Sha256 {
  uint32_t st[8];
  uint8_t buf[64];
  size_t fill = 0;
  uint64_t total = 0;
  Sha256() { sha256_init(st); }
  void block(const uint8_t* p) {
    uint32_t w[16];
    for (int j = 0; j < 16; j++)
      w[j] = ((uint32_t)p[4 * j] << 24) | ((uint32_t)p[4 * j + 1] << 16) | ((uint32_t)p[4 * j + 2] << 8) | p[4 * j + 3];
    sha256_compress(st, {w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], w[10], w[11], w[12], w[13],
                         w[14], w[15]});
  }
  void update(const void* data, size_t len) {
    const uint8_t* p = static_cast<const uint8_t*>(data);
    total += len;
    if (fill) {
      const size_t take = len < 64 - fill ? len : 64 - fill;
      memcpy(buf + fill, p, take);
      fill += take; p += take; len -= take;
      if (fill < 64) return;
      block(buf);
      fill = 0;
    }
    for (; len >= 64; p += 64, len -= 64) block(p);
    if (len) memcpy(buf, p, len);
    fill = len;
  }
  void update_u64be(uint64_t v) {
    uint8_t b[8];
    for (int i = 0; i < 8; i++) b[i] = (uint8_t)(v >> (56 - 8 * i));
    update(b, 8);
  }
  void final(uint8_t out[32]) {
    const uint64_t bits = total * 8;
    buf[fill++] = 0x80;
    if (fill > 56) {
      memset(buf + fill, 0, 64 - fill);
      block(buf);
      fill = 0;
    }
    memset(buf + fill, 0, 56 - fill);
    for (int i = 0; i < 8; i++) buf[56 + i] = (uint8_t)(bits >> (56 - 8 * i));
    block(buf);
    for (int i = 0; i < 8; i++) {
      out[4 * i] = (uint8_t)(st[i] >> 24); out[4 * i + 1] = (uint8_t)(st[i] >> 16);
      out[4 * i + 2] = (uint8_t)(st[i] >> 8); out[4 * i + 3] = (uint8_t)st[i];
    }
  }
};

}  // namespace zk
