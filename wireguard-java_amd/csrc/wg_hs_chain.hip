// wg_hs_chain.hip — the machine that k_hs_open, k_hs_resp_chain, k_hs_init_chain, k_hs_fin_chain and
// k_hs_stamp_chain run their Noise chains on (included by wg_capi.hip before wg_hs_open.hip). The chains themselves are data: wg_hs_chain.h.
//
// A chain is a row of dependent BLAKE2s compressions per lane, nearly all of them parts of HMAC-BLAKE2s: an
// HMAC is four compressions (the two key blocks K ^ 0x36.., K ^ 0x5c.. as words, never bytes; the message
// behind the first; the inner digest behind the second), KDFn's expands of one extract share the key-block
// states, and T_{n-1} is the message of T_n. Each kernel runs its program in ONE loop around ONE b2s_compress:
//   the step's word {op, arg, imm, dst}  (step is wave-uniform: one scalar load from constant memory, fetch()ed
//                                   a step ahead, before the compression)
//   switch (s.arg)                  the 32 bytes the step takes: the kernel's own sources, else source()
//   switch (s.op)                   m, st, t, last for the compression: the kernel's own operations, else prepare()
//   b2s_compress
//   switch (s.dst)                  where the state goes: WG_HSC_PUT
// Inlined, the compressions would be some 200 KB (open) and 350 KB (respond) of straight-line code that every
// wave streams through the instruction cache once; the loop stays there. Every switch is over a byte of a
// wave-uniform word, so it is a scalar branch, and the registers are named by the cases, never indexed
// dynamically.
//
// Constant time: the programs are public and indexed by a public counter; nothing here branches on, or
// addresses by, a value of the state.
#pragma once
#include "wg_hs_chain.h"

namespace wghc {

// The registers of a chain: the Noise hash and chain key, the PRK of the current extract (and whatever an
// expand leaves for the next step: tau, k, send_key), the states after the current key's two key blocks, and
// one compression's state, message, byte count and final flag.
struct Chain {
  uint32_t hh[8], ck[8], x[8], ist[8], ost[8], st[8], m[16];
  uint32_t t;
  bool last;
};

__device__ __forceinline__ void set8(uint32_t d[8], const uint32_t s[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) d[j] = s[j];
}
// m = the 32 bytes w, zeros behind them
__device__ __forceinline__ void msg32(uint32_t m[16], const uint32_t w[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    m[j] = w[j];
    m[8 + j] = 0u;
  }
}
// m = the HMAC key block of a 32-byte key: key ^ pad, then pad (pad = 0x36363636 / 0x5c5c5c5c)
__device__ __forceinline__ void pad_block(uint32_t m[16], const uint32_t key[8], uint32_t pad) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    m[j] = key[j] ^ pad;
    m[8 + j] = pad;
  }
}
__device__ __forceinline__ void put8(uint32_t w[8], const uint4 a, const uint4 b) {
  w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}

// The word of step k (of the last step, for a k behind the end). A kernel fetches the next step's word before the
// compression of the current one: a wave that has its SIMD to itself would otherwise wait for the scalar load
// once per step.
template <uint32_t N>
__device__ __forceinline__ Step fetch(const Step (&prog)[N], uint32_t k) {
  return prog[k < N ? k : N - 1u];
}

__device__ __forceinline__ void clear(Chain& c) {
#pragma unroll
  for (int j = 0; j < 8; ++j) c.hh[j] = c.ck[j] = c.x[j] = c.ist[j] = c.ost[j] = c.st[j] = 0u;
  c.t = 0u;
  c.last = true;
}

// the sources that live in the chain; any other is 32 zero bytes
__device__ __forceinline__ void source(const Chain& c, uint32_t arg, uint32_t src[8]) {
  switch (arg) {
    case SRC_CK: set8(src, c.ck); break;
    case SRC_X: set8(src, c.x); break;
    default:
#pragma unroll
      for (int j = 0; j < 8; ++j) src[j] = 0u;
      break;
  }
}

// the generic operations: m, st, t and last for the compression of step s over src
__device__ __forceinline__ void prepare(Chain& c, const Step s, const uint32_t src[8]) {
  switch (s.op) {
    case OP_PAD:
      pad_block(c.m, src, (s.imm & PAD_OPAD) ? 0x5C5C5C5Cu : 0x36363636u);
      wghs::b2s_init(c.st, 32u, 0u);
      c.t = 64u; c.last = (s.imm & PAD_LAST) != 0;
      break;
    case OP_IN32:
      msg32(c.m, src);
      set8(c.st, c.ist);
      c.t = 96u; c.last = true;
      break;
    case OP_OUT:
      msg32(c.m, c.st);
      set8(c.st, c.ost);
      c.t = 96u; c.last = true;
      break;
    case OP_T1:
#pragma unroll
      for (int j = 0; j < 16; ++j) c.m[j] = j == 0 ? 1u : 0u;
      set8(c.st, c.ist);
      c.t = 65u; c.last = true;
      break;
    case OP_TN:
      msg32(c.m, src);
      c.m[8] = s.imm;
      set8(c.st, c.ist);
      c.t = 97u; c.last = true;
      break;
    default:  // OP_H2
      set8(c.m, c.hh);
      set8(c.m + 8, src);
      wghs::b2s_init(c.st, 32u, 0u);
      c.t = 64u; c.last = true;
      break;
  }
}

// The destinations every chain has: a kernel's switch on s.dst ends in `default: WG_HSC_PUT(c, s.dst)`. A macro,
// not a function like prepare(): the compiler optimises a function on its own before it inlines it, and there
// the five copies, which differ in nothing but the member they go to, become one copy to an address computed
// from dst. Inlined, that address keeps the whole chain in scratch memory (144 bytes per lane in both kernels).
// Expanded in the kernel the arms store to registers that are already named.
#define WG_HSC_PUT(c, dst)                                  \
  switch (dst) {                                            \
    case wghc::DST_H: wghc::set8((c).hh, (c).st); break;    \
    case wghc::DST_X: wghc::set8((c).x, (c).st); break;     \
    case wghc::DST_CK: wghc::set8((c).ck, (c).st); break;   \
    case wghc::DST_IST: wghc::set8((c).ist, (c).st); break; \
    case wghc::DST_OST: wghc::set8((c).ost, (c).st); break; \
    default: break;                                         \
  }

// tag = Poly1305(aad (32) || ct (16 CT) || LE64(32) || LE64(16 CT)) under the one-time key ks[0 .. 8), the
// counter-0 ChaCha20 block of the AEAD's key: the tag of RFC 8439 2.8 for 32 bytes of aad and CT whole blocks
// of ciphertext, as 3 + CT Horner steps.
template <int CT>
__device__ __forceinline__ void poly_tag(const uint32_t ks[16], const uint32_t aad[8], const uint32_t* ct, uint32_t tag[4]) {
  uint32_t r[5], s5[5], h[5] = {0u, 0u, 0u, 0u, 0u}, c[5];
  wgd::poly_r_limbs(ks[0], ks[1], ks[2], ks[3], r);
  wgd::poly_scale5(r, s5);
#pragma unroll
  for (int b = 0; b < 3 + CT; ++b) {
    if (b < 2) wgd::poly_block_limbs(aad[4 * b], aad[4 * b + 1], aad[4 * b + 2], aad[4 * b + 3], 1u << 24, c);
    else if (b < 2 + CT) wgd::poly_block_limbs(ct[4 * b - 8], ct[4 * b - 7], ct[4 * b - 6], ct[4 * b - 5], 1u << 24, c);
    else wgd::poly_block_limbs(32u, 0u, 16u * CT, 0u, 1u << 24, c);
#pragma unroll
    for (int j = 0; j < 5; ++j) h[j] += c[j];
    wgd::poly_mul<false>(h, r, s5);
  }
  wgd::poly_finish(h, ks[4], ks[5], ks[6], ks[7], tag);
}

// ... for a ciphertext of ct_bytes bytes, 16 (CT - 1) < ct_bytes <= 16 CT: ct holds CT blocks, the last one padded
// with zeros by the caller (RFC 8439 2.8: pad16), and the length block carries the true byte count. A sibling, so
// that poly_tag's instantiations stay as they are.
template <int CT>
__device__ __forceinline__ void poly_tag_bytes(const uint32_t ks[16], const uint32_t aad[8], const uint32_t* ct, uint32_t ct_bytes,
                                               uint32_t tag[4]) {
  uint32_t r[5], s5[5], h[5] = {0u, 0u, 0u, 0u, 0u}, c[5];
  wgd::poly_r_limbs(ks[0], ks[1], ks[2], ks[3], r);
  wgd::poly_scale5(r, s5);
#pragma unroll
  for (int b = 0; b < 3 + CT; ++b) {
    if (b < 2) wgd::poly_block_limbs(aad[4 * b], aad[4 * b + 1], aad[4 * b + 2], aad[4 * b + 3], 1u << 24, c);
    else if (b < 2 + CT) wgd::poly_block_limbs(ct[4 * b - 8], ct[4 * b - 7], ct[4 * b - 6], ct[4 * b - 5], 1u << 24, c);
    else wgd::poly_block_limbs(32u, 0u, ct_bytes, 0u, 1u << 24, c);
#pragma unroll
    for (int j = 0; j < 5; ++j) h[j] += c[j];
    wgd::poly_mul<false>(h, r, s5);
  }
  wgd::poly_finish(h, ks[4], ks[5], ks[6], ks[7], tag);
}

}  // namespace wghc
