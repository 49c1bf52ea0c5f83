// wg_transport.hip — the transport-data seal/open kernel for gfx950 (product path).
//
// Replaces the per-packet SymmetricKeypair.cipher / decipher
// (ax.xz.wireguard.noise/src/main/java/ax/xz/wireguard/noise/handshake/SymmetricKeypair.java:63-83)
// over a batch of independent packets: ChaCha20 keystream from counter 1, Poly1305 key from
// block 0, MAC over ct || pad16 || le64(0) || le64(len) (ChaCha20Poly1305.java:31-93), with the
// reference's nonce LE64(counter) || 0^4 (SymmetricKeypair.java:52-61).
//
// Layout (k_transport<MODE>): a wave is 8 SLOTS of 8 lanes; a slot owns one packet at a
// time and streams it in ROUNDS of 8 ChaCha20 counter blocks (512 bytes):
//   * lane j of the slot computes block b = 8 round + j in registers (block 0 = the
//     Poly1305 one-time key), XORs its 64 payload bytes, stores them, and leaves the
//     round's MAC input (the ciphertext) in a 4 KB per-wave LDS image;
//   * the same 8 lanes advance an 8-strided Horner evaluation of the MAC polynomial
//     over the image (lane j owns positions = j mod 8, multiplier r^8, front padding
//     so the length block lands on lane 7); on the last round lane j scales its partial
//     by r^(8-j), the slot sums the 8 partials and lane 0 finishes the tag.
// ChaCha20: the first column round of columns 1..3 depends only on the key and the nonce, so
// lanes 1..3 of a slot compute it once per packet and every block takes it by ds_swizzle
// broadcast (chacha20_block_hoisted: -3% VALU instructions on C1). Poly1305: the length block
// is written into the image by the lane whose counter block holds it, so the Horner steps
// read it like ciphertext; each step's product chains every limb's carry into the next limb's
// v_mad_u64_u32 accumulator (poly_mul: 5 fewer instructions per step than five independent
// chains with the carries added afterwards; C1 +1.2%, C2 +0.2% in round 3, where round 2's
// kernel had measured the independent chains +3% on C2). The
// r-power scan and the slot sum exchange limbs through DPP (row_shr / quad_perm), which stays
// in the VALU instead of an LDS round trip in the middle of a dependent chain.
// Slots are persistent: slot g of S processes batch positions g, 2S-1-g, 2S+g, ... (a
// snake over the grid). Mixed-length batches are first ordered longest-first on the
// device (k_lpt_*), so the snake deals every slot one long and one short packet
// (LPT); uniform batches take positions in order. The next packet's descriptor is
// prefetched one packet ahead (one dword per lane), so a slot never waits on a
// dependent descriptor load when it starts a packet.
//
// IO: a lane's 64 payload bytes are fetched before the ARX rounds with LDS-DMA
// (global_load_lds, 16 B per lane per instruction) into the wave's chunk-major LDS image,
// so no registers are held across the rounds; chunks holding a valid byte are read whole
// (an aligned 16-B read never leaves the granule of its first byte) and masked. Unaligned
// inputs stage aligned dwords through registers (v_alignbyte). Stores are dwordx4 for
// 16-B aligned outputs, dword + bytes for 4-B aligned ones, bytes otherwise.
// Per-slot state (offsets, counter, length, flags, R = r^8, 5R, s, key) lives in a 128-B
// LDS record. A wave whose 8 slots share one key slot fetches the key through the scalar
// cache. Open writes the plaintext in the same pass and zero-fills it again if the tag does
// not verify (the host per-packet wrappers copy back only verified plaintext, as
// ChaCha20Poly1305.java:40-56 leaves dst untouched).
// Uniform waves: in the WG_F_UNIFORM plan's 8-lane kernels (k_transport_uni, k_step_uni) a wave whose slots all
// hold valid packets of one length, 16-B aligned, under one key runs a smaller body with its uniform state in
// SGPRs (transport_body_uni, below the general body); every other wave runs transport_body.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wg_device.h"
#include "wg_kernels.h"

namespace wgt {

using namespace wgd;

#ifndef WG_TW
#define WG_TW 4
#endif
constexpr uint32_t TW = WG_TW;      // waves per workgroup
constexpr uint32_t LPT_BINS = 130;  // round counts 0..129 (65535-B payload = 1025 blocks = 129 rounds)

// AllowedIPs tables of the receive side (wg_rx.hip) as the open kernel reads them when
// wg_open_batch is called with WG_F_RX_FILTER: one struct in device memory, rebuilt whenever a
// filter or the slot -> filter map changes.
constexpr uint32_t kNoFilter = 0xFFFFFFFFu;
struct RxTables {
  const uint32_t* slot_filter;  // per key slot: filter id or kNoFilter (NULL: no map set)
  const uint32_t* hdr;          // per filter: root4, root6 (global node indices)
  const uint32_t* entries;      // nodes x 256 entries: next node | bit 31 "a prefix ended in this byte"
  uint32_t nfilters;
  uint32_t key_slots;
};

// TransportManager.processDecryptedTransport for one opened packet whose tag verified
// (TransportManager.java:98-119): a keepalive (len 0, :103-105), an address family that is not
// IPv4/IPv6 or a packet too short for the destination (destinationIPOf, :124-130, throws), or a
// destination outside the key slot's AllowedIPs (IPFilter.search, util/IPFilter.java:49-61).
// p: the plaintext (global memory, this launch's output). Shared by k_rx_filter and the fused
// open (WG_F_RX_FILTER).
__device__ inline uint32_t rx_verdict(const RxTables& T, const uint8_t* p, uint32_t len, uint32_t key_slot) {
  if (len == 0) return WG_PKT_KEEPALIVE;
  const uint32_t ver = p[0] >> 4;
  uint32_t nbytes, at;
  if (ver == 4) {
    nbytes = 4;
    at = 16;
  } else if (ver == 6) {
    nbytes = 16;
    at = 24;
  } else {
    return WG_PKT_BADIP;
  }
  if (len < at + nbytes) return WG_PKT_BADIP;
  if (!T.slot_filter || key_slot >= T.key_slots) return WG_PKT_OK;
  const uint32_t f = T.slot_filter[key_slot];
  if (f == kNoFilter) return WG_PKT_OK;
  uint32_t node = f < T.nfilters ? T.hdr[2 * f + (ver == 6 ? 1 : 0)] : 0u;  // never set: empty filter
  bool found = false;
  for (uint32_t L = 0; L < nbytes && node; ++L) {
    const uint32_t e = T.entries[(size_t)node * 256 + p[at + L]];
    found |= (e >> 31) != 0;
    node = e & 0x7FFFFFFFu;
  }
  return found ? WG_PKT_OK : WG_PKT_FILTERED;
}

struct TransportParams {
  const wg_pkt* desc;
  const uint32_t* order;  // batch position -> packet index (longest first); nullptr = identity
  uint32_t n;
  uint32_t slots;         // S = (64 / G) x waves in the grid
  uint32_t max_len;
  uint32_t key_slots;
  const uint8_t* in;
  uint64_t in_size;
  uint8_t* out;
  uint64_t out_size;
  const uint32_t* keys;   // device key table, 8 words per slot
  uint32_t* status;       // open: per-packet WG_PKT_*
  uint32_t prio_step;     // rounds per issue-priority level (0: no priority changes)
  const RxTables* rx;     // open with WG_F_RX_FILTER: receive-side verdict in the status (else NULL)
  const uint32_t* n_long; // k_*_mixed: device count of the packets at the front of the order that take
                          // 16-lane slots (written by k_lpt_scatter); NULL otherwise. With bin_cnt (one-launch
                          // planning, k_lpt_one) it only marks the launch as mixed.
  // one-launch planning (k_lpt_one, batches of max_len <= 2048): the longest-first order is SPARSE, key k's
  // packets at order[k * bin_cap ...], bin_cnt[k] of them; the kernel reads the counts into bc (mixed_part)
  // and maps a batch position to its packet through them (pkt_at). pos_base: the position of this part's
  // first packet in the whole order (the short part starts after the long one). split: keys > split are long.
  const uint32_t* bin_cnt;
  uint32_t bin_cap;
  uint32_t pos_base;
  uint32_t split;
  uint32_t split2;  // k_step_mixed with GT = 2: keys <= split2 (> 0) take 2-lane slots, after the GS-lane part
  // Five fields no code reads or writes (always zero). They were the dynamic-claim variant's (removed,
  // docs/EXPERIMENTS.md) and keep the kernel arguments' layout: without them every kernel has the same
  // registers, spills and occupancy, but k_step_mixed<4, 2> (IMIX) comes out of the register allocator and
  // the scheduler as different code, and this layout's code is the one every measurement was taken on.
  // Dropping them is a change to measure, not to make in passing.
  uint32_t* unused_ptr0;
  uint32_t unused_u0, unused_u1;
  uint2* unused_ptr1;
  const uint2* unused_ptr2;
  // 4-lane slots, one packet per slot (plan_transport): waves in one workgroup generation (workgroups
  // per CU x CUs x waves per workgroup); every odd generation takes its longest-first positions in
  // reverse, so the waves that share a SIMD get long and short packets in turn (0: no reversal)
  uint32_t wave_gen;
#ifdef WG_DIAG
  uint64_t* stamps;       // diagnostic build only: 10 x u64 per wave (cycles per phase, start/end times)
#endif
};

// Per-wave phase accounting, compiled only into the diagnostic library (make diag):
// cycles spent in each phase of the round loop, summed over the wave's rounds.
#ifdef WG_DIAG
#define WG_PH_DECL uint64_t ph_[7] = {0, 0, 0, 0, 0, 0, 0}; uint64_t ph_t = __builtin_amdgcn_s_memtime(); \
  const uint64_t ph_r0 = __builtin_amdgcn_s_memrealtime(); (void)ph_r0;
#define WG_PH(k) do { const uint64_t n_ = __builtin_amdgcn_s_memtime(); ph_[k] += n_ - ph_t; ph_t = n_; } while (0)
#define WG_PH_STORE(idx)                                                                       \
  do {                                                                                         \
    if (P.stamps && (threadIdx.x & 63u) == 0) {                                                \
      uint64_t* o_ = P.stamps + (size_t)(idx) * 10;                                            \
      for (int k_ = 0; k_ < 7; ++k_) o_[k_] = ph_[k_];                                         \
      o_[8] = ph_r0;                                                                           \
      o_[9] = __builtin_amdgcn_s_memrealtime();                                                \
    }                                                                                          \
  } while (0)
#elif defined(WG_MARKS)  // asm comments at the phase boundaries (tools/isa_phases.py)
#define WG_PH_DECL
#define WG_PH(k) asm volatile(";; WGMARK " #k)
#define WG_PH_STORE(idx) do {} while (0)
#else
#define WG_PH_DECL
#define WG_PH(k) do {} while (0)
#define WG_PH_STORE(idx) do {} while (0)
#endif

// ---- lane exchange inside a slot of G lanes (G = 4, 8 or 16) ------------------------
// ds_swizzle bitmask mode inside each 32-lane half: src = ((lane & and) | or) ^ xor.
template <int G, int K>
__device__ __forceinline__ uint32_t bcastg(uint32_t v) {  // every lane of the slot reads lane K of it
  static_assert(G == 2 || G == 4 || G == 8 || G == 16, "slots of 2, 4, 8 or 16 lanes");
  return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (0x20 - G) | (K << 5));
}
template <int K>
__device__ __forceinline__ uint32_t bcast8(uint32_t v) { return bcastg<8, K>(v); }
template <int X>
__device__ __forceinline__ uint32_t xorg(uint32_t v) {  // lane reads lane ^ X (X < 16)
  return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x1f | (X << 10));
}

// A slot's copy of one 32-B descriptor (wg_pkt = 8 dwords): with 8 or 16 lanes, lane j holds dword j & 7
// (w.x); with 4 lanes, lane j holds dwords 2j and 2j + 1 (w.x, w.y: one 8-B load, desc_load4); with 2 lanes,
// dwords 4j .. 4j + 3 (one 16-B load, desc_load2). desc_word<G, K> gives every lane of the slot dword K.
__device__ __forceinline__ uint2 desc_load4(const wg_pkt* d, uint32_t i, uint32_t j) {
  return i != ~0u ? ((const uint2*)(d + i))[j & 3u] : make_uint2(0u, 0u);
}
__device__ __forceinline__ uint4 desc_load2(const wg_pkt* d, uint32_t i, uint32_t j) {
  return i != ~0u ? ((const uint4*)(d + i))[j & 1u] : make_uint4(0u, 0u, 0u, 0u);
}
template <int G, int K>
__device__ __forceinline__ uint32_t desc_word(const uint4& w) {
  if constexpr (G == 2) return bcastg<2, K / 4>((K & 3) == 0 ? w.x : (K & 3) == 1 ? w.y : (K & 3) == 2 ? w.z : w.w);
  else if constexpr (G == 4) return bcastg<4, K / 2>((K & 1) ? w.y : w.x);
  else return bcastg<G, K>(w.x);
}

// The same exchanges through DPP (VALU, no LDS round trip) for the dependent chains of the
// r-power scan and the slot sum: row_shr:K (lane j reads j - K inside its 16-lane row; lanes j < K
// of a slot get garbage and must not use it), lane ^ 1, lane ^ 2 (quad_perm), lane ^ 4 (two half
// moves) and lane ^ 8 (row_ror:8, 16-lane slots).
template <int K>
__device__ __forceinline__ uint32_t shr_dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 | K, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t xor1_dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);  // quad_perm [1,0,3,2]
}
__device__ __forceinline__ uint32_t xor2_dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);  // quad_perm [2,3,0,1]
}
__device__ __forceinline__ uint32_t xor4_dpp(uint32_t v) {
  // lanes 4-7 of a slot (banks 1, 3) read j - 4 (row_shr:4), lanes 0-3 (banks 0, 2) read j + 4 (row_shl:4)
  const int t = __builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xa, false);
  return (uint32_t)__builtin_amdgcn_update_dpp(t, (int)v, 0x104, 0xf, 0x5, false);
}
__device__ __forceinline__ uint32_t xor8_dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);  // row_ror:8
}

// slot-record flags beyond valid / alignment (SlotRec.meta.w): an open whose plaintext range
// overlaps its ciphertext || tag range verifies first (no stores) and decrypts in a second pass
constexpr uint32_t kVerifyFirst = 16u, kDecryptPass = 32u;

// ---- validity of one transport descriptor (shared by seal, open and the framing) ----
template <int MODE>
__device__ __forceinline__ bool transport_valid(uint64_t in_off, uint64_t out_off, uint32_t len, uint32_t ks,
                                                uint32_t max_len, uint32_t key_slots, uint64_t in_size,
                                                uint64_t out_size) {
  const uint64_t in_need = (uint64_t)len + (MODE == WG_MODE_OPEN ? 16u : 0u);
  const uint64_t out_need = (uint64_t)len + (MODE == WG_MODE_SEAL ? 16u : 0u);
  return len <= max_len && ks < key_slots && in_off <= in_size && in_need <= in_size - in_off &&
         out_off <= out_size && out_need <= out_size - out_off;
}

// 16 bytes at p (any alignment), `avail` (1..16) of them inside the packet: the aligned dwords
// covering them (none leaves the granule of a valid byte), realigned with v_alignbyte
__device__ __forceinline__ uint4 chunk_any(const uint8_t* p, uint32_t avail) {
  const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
  const uint32_t* q = (const uint32_t*)(p - sh);
  const uint32_t nw = (sh + avail + 3u) >> 2;
  uint32_t W[5];
#pragma unroll
  for (uint32_t k = 0; k < 5; ++k) W[k] = k < nw ? q[k] : 0u;
  return make_uint4(__builtin_amdgcn_alignbyte(W[1], W[0], sh), __builtin_amdgcn_alignbyte(W[2], W[1], sh),
                    __builtin_amdgcn_alignbyte(W[3], W[2], sh), __builtin_amdgcn_alignbyte(W[4], W[3], sh));
}

// bytes >= cb (1..15) of a 16-B chunk zeroed: dword k keeps clamp(8 cb - 32 k, 0, 32) low bits
__device__ __forceinline__ uint4 mask_chunk(uint4 v, uint32_t cb) {
  int c8 = (int)(8u * cb);
  asm volatile("" : "+v"(c8));  // keep the mask arithmetic in the (rare) partial-chunk path
  uint32_t t[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) t[k] &= ~(uint32_t)(~0ull << min(max(c8 - 32 * k, 0), 32));
  return make_uint4(t[0], t[1], t[2], t[3]);
}

// cb (1..16) bytes of a chunk to p: oal bit 2 = p 16-B aligned, bit 3 = p 4-B aligned
__device__ __forceinline__ void store_chunk(uint8_t* p, uint32_t cb, uint4 o, uint32_t oal) {
  if (cb == 16u && (oal & 4u)) {
    *(uint4*)p = o;
    return;
  }
  const uint32_t t[4] = {o.x, o.y, o.z, o.w};
  if (oal & 8u) {
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      const int r = (int)cb - 4 * (int)k;
      if (r >= 4) {
        ((uint32_t*)p)[k] = t[k];
      } else if (r > 0) {
        uint8_t* q = p + 4u * k;
        q[0] = (uint8_t)t[k];
        if (r > 1) q[1] = (uint8_t)(t[k] >> 8);
        if (r > 2) q[2] = (uint8_t)(t[k] >> 16);
      }
    }
  } else {
#pragma unroll
    for (uint32_t i = 0; i < 16u; ++i)
      if (i < cb) p[i] = (uint8_t)(t[i >> 2] >> (8u * (i & 3u)));
  }
}

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void gbl_cvoid;

__device__ __forceinline__ uint32_t load_u32_any(const uint8_t* p) {
  if ((((uintptr_t)p) & 3u) == 0) return *(const uint32_t*)p;
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ __forceinline__ void store_u32_any(uint8_t* p, uint32_t v) {
  if ((((uintptr_t)p) & 3u) == 0) {
    *(uint32_t*)p = v;
    return;
  }
  p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

// orders this wave's LDS writes before its other lanes' reads
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

__device__ __forceinline__ uint32_t batch_pos(uint32_t g, uint32_t k, uint32_t S) {
  return k * S + ((k & 1u) ? S - 1u - g : g);
}

#define WG_CONST __attribute__((address_space(4)))  // constant address space: scalar loads

// batch position -> packet index: the identity, the dense longest-first order, or the sparse one of k_lpt_one
// (keys descending, key k's packets at order[k * bin_cap + i])
constexpr uint32_t kFastBins = 6;  // keys 0..5: every packet of at most 2,048 B (33 blocks, 5 rounds of 8)
// k_lpt_one's per-key counters, kCntStride words apart (every planner workgroup adds to each once). 16 (a
// 64-B line each) measured the same as 1: the planner's 5.1 us is not atomic contention
// (profiles/r06_cnt_stride_ab.jsonl)
#ifndef WG_CNT_STRIDE
#define WG_CNT_STRIDE 1
#endif
constexpr uint32_t kCntStride = WG_CNT_STRIDE;
template <int MX>  // MX: bins of the sparse order (kFastBins, the short-packet plan), 0: dense
__device__ __forceinline__ uint32_t pkt_at(const TransportParams& P, uint32_t pos) {
  if (MX && P.bin_cap) {
    // the counts through the scalar cache (constant for the launch), not held in SGPRs across the body
    // (branch-free: the position's key region and its offset in it, one select per key)
    const WG_CONST uint32_t* bc = (const WG_CONST uint32_t*)P.bin_cnt;
    const uint32_t p = P.pos_base + pos;
    uint32_t start = 0, at = 0;
#pragma unroll
    for (int k = MX - 1; k >= 0; --k) {
      const uint32_t c = bc[k * kCntStride];
      at = (p >= start) ? (uint32_t)k * P.bin_cap + (p - start) : at;
      start += c;
    }
    return P.order[at];
  }
  return P.order ? P.order[pos] : pos;
}

// ---- the kernel ------------------------------------------------------------------------
// Register budget: <= 64 VGPRs, so 8 waves share a SIMD (the payload stream and the ARX
// rounds of other waves hide each other's latency). What is constant for a packet lives
// in a 128-B LDS record per slot and is re-read where it is used; lane-derived values are
// recomputed from an opaque copy of the lane id instead of being held across the rounds.
struct SlotRec {  // per slot, in LDS
  uint4 addr;     // {in_off lo, in_off hi, out_off lo, out_off hi} (pointers are rebuilt from the kernel
                  // arguments, so the compiler keeps global, not flat, memory instructions)
  uint4 meta;     // {ctr lo, ctr hi, len, flags}: bit 0 valid, bit 1 input / bit 2 output 16-B aligned,
                  // bit 3 output 4-B aligned
  uint4 R0;       // R = r^8 limbs 0..3
  uint4 R1;       // {R4, 5 R1, 5 R2, 5 R3}
  uint4 R2;       // {5 R4, -, -, -}
  uint4 s;        // Poly1305 s
  uint4 key[2];   // ChaCha20 key
};
static_assert(sizeof(SlotRec) == 128, "slot record is 128 B");


__device__ __forceinline__ uint32_t opaque_lane() {
  uint32_t x = threadIdx.x & 63u;
  asm volatile("" : "+v"(x));
  return x;
}

// The per-wave body of k_transport (and of each half of k_duplex / k_step): workgroup `blk` of the
// direction's grid; img / rec are this wave's 4-KB image and slot records in LDS. G = lanes per
// slot: 8 (8 slots per wave, rounds of 8 blocks) or 16 (4 slots, rounds of 16 blocks = 1 KB:
// long packets take half as many rounds, so a mixed-length batch can pair them longest-first at
// 8 waves per SIMD).
// iter: rounds this wave has run so far in the launch (the issue-priority schedule spans both
// halves of a k_step launch).
// A slot's packets are the snake over the grid (batch_pos).
// MX: the launch is a k_*_mixed part (its positions may map through k_lpt_one's sparse order)
template <int MODE, int G = 8, bool VF = false, int MX = 0>
__device__ __forceinline__ void transport_body(const TransportParams& P, uint32_t blk, uint32_t wv, uint4* const img,
                                               SlotRec* const rec, uint32_t& iter) {
  static_assert(MODE == WG_MODE_SEAL || MODE == WG_MODE_OPEN, "transport modes only");
  static_assert(G == 2 || G == 4 || G == 8 || G == 16, "slots of 2, 4, 8 or 16 lanes");
  static_assert(G != 2 || (MX && !VF), "2-lane slots: the short-packet split plan's tiny packets only");
#ifdef WG_HORNER2
  static_assert(G != 2, "the two-chunk Horner assumes G >= 4");
#endif
  static_assert(!VF || MODE == WG_MODE_OPEN, "verify-first is an open variant");
  constexpr uint32_t SH = G == 2 ? 1u : G == 4 ? 2u : G == 8 ? 3u : 4u;  // log2 G
  constexpr uint32_t JM = G - 1u;
  // a slot's record (SlotRec); 2-lane slots keep an 80-B one, so 32 of them per wave leave the launch at 6
  // workgroups per CU: no key (read from the key table each round, the slot's key index in meta.w >> 8), no
  // 5 R limbs (formed where used), s = {R1.y, R1.z, R1.w, R2.x} beside R4 = R1.x
  constexpr uint32_t kRecStride = G == 2 ? 80u : (uint32_t)sizeof(SlotRec);
  auto RS = [rec](uint32_t si) -> SlotRec& { return *(SlotRec*)((char*)rec + si * kRecStride); };
  if (P.prio_step && iter == 0) __builtin_amdgcn_s_setprio(3);  // first instruction: a fresh wave is never starved
  const uint32_t S = P.slots;
  uint32_t wg = blk * TW + wv;  // this wave's index in the grid
  if constexpr (G == 4) {
    if (P.wave_gen) {  // odd generations reversed (a bijection: the last, partial one over its own size)
      const uint32_t k = wg / P.wave_gen, i = wg - k * P.wave_gen;
      const uint32_t size = min(P.wave_gen, gridDim.x * TW - k * P.wave_gen);
      if (k & 1u) wg = k * P.wave_gen + (size - 1u - i);
    }
  }
  const uint32_t g = wg * (64u / G) + (opaque_lane() >> SH);

  // descriptor prefetch: the next packet's wg_pkt spread over the slot's lanes (desc_load)
  uint32_t gen = 0;
  uint32_t nxt;
  {
    const uint32_t pos = batch_pos(g, 0, S);
    nxt = pos < P.n ? pkt_at<MX>(P, pos) : ~0u;
  }
  uint4 dn = make_uint4(0u, 0u, 0u, 0u);  // this lane's part of the next descriptor (desc_word)
  if constexpr (G == 2) {
    dn = desc_load2(P.desc, nxt, opaque_lane());
  } else if constexpr (G == 4) {
    const uint2 w = desc_load4(P.desc, nxt, opaque_lane());
    dn.x = w.x;
    dn.y = w.y;
  } else {
    dn.x = nxt != ~0u ? ((const uint32_t*)(P.desc + nxt))[opaque_lane() & 7u] : 0u;
  }

  bool have = false;
  uint32_t pkt = 0, round = 0;
  uint32_t acc[5], W[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) acc[i] = W[i] = 0;

  // lane j of a slot holds the packet's first-round column (j & 3) (a, b, c, d); lanes 1..3
  // feed the other lanes' blocks through ds_swizzle broadcasts
  uint32_t hc[4] = {0u, 0u, 0u, 0u};
  // Progress-based issue priority (mixed-length batches; prio_step = 0 for uniform ones): a SIMD
  // arbitrates VALU issue by priority, then age, so with equal priorities the oldest of its 8
  // waves runs ahead and the waves finish one after another. A wave drops one priority level
  // every prio_step rounds instead, so the waves that have done the least work issue first
  // (C2 +2%, C1 -2%: DESIGN.md §4.2).
  WG_PH_DECL
  while (true) {
    if (P.prio_step) {
      const uint32_t lvl = iter / P.prio_step;
      if (iter % P.prio_step == 0 && lvl <= 3u && lvl > 0u) {
        if (lvl == 1) __builtin_amdgcn_s_setprio(2);
        else if (lvl == 2) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
      }
      ++iter;
    }
    // ---- slots without a packet take their next one ------------------------------------
    if (!have && nxt != ~0u) {
      const uint32_t lane = opaque_lane(), s = lane >> SH, j = lane & JM;
      pkt = nxt;
#ifdef WG_DIAG
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(dn.x), "+v"(dn.y), "+v"(dn.z), "+v"(dn.w));
      WG_PH(6);
#endif
      const uint32_t d0 = desc_word<G, 0>(dn), d1 = desc_word<G, 1>(dn), d2 = desc_word<G, 2>(dn),
                     d3 = desc_word<G, 3>(dn);
      const uint32_t len = desc_word<G, 6>(dn), ks = desc_word<G, 7>(dn);
      const uint64_t in_off = (uint64_t)d0 | ((uint64_t)d1 << 32);
      const uint64_t out_off = (uint64_t)d2 | ((uint64_t)d3 << 32);
      const bool valid =
          transport_valid<MODE>(in_off, out_off, len, ks, P.max_len, P.key_slots, P.in_size, P.out_size);
      const uintptr_t ia = (uintptr_t)(P.in + in_off), oa = (uintptr_t)(P.out + out_off);
      uint32_t al = ((ia & 15u) == 0 ? 2u : 0u) | ((oa & 15u) == 0 ? 4u : 0u) | ((oa & 3u) == 0 ? 8u : 0u);
      // open with the plaintext range overlapping the ciphertext || tag range (in place): verify the
      // tag first and decrypt in a second pass, so a forged packet's bytes stay as they were
      // (ChaCha20Poly1305.java:40-56 verifies before it decrypts)
      if (VF && valid && len && ia < oa + len && oa < ia + len + 16u) al |= kVerifyFirst;
      // The session key. Vector loads come back in order through the CU's L1, so at a launch's
      // start a key load would queue behind the payload DMA of every wave already running on
      // the CU; when every slot of the wave uses one key (one session per wave: C1, C3) it comes
      // through the scalar cache instead, which no payload traffic passes.
      const uint32_t ks0 = __builtin_amdgcn_readfirstlane(ks);
      if (!__any(valid && ks != ks0) && ks0 < P.key_slots) {
        const WG_CONST uint32_t* kp = (const WG_CONST uint32_t*)P.keys + 8u * ks0;
        uint32_t k[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          k[i] = kp[i];  // s_load_dwordx8
#ifndef WG_NO_SKEY
          asm volatile("" : "+s"(k[i]));  // keep it scalar (no per-lane reload)
#endif
        }
        uint32_t v = k[0];
#pragma unroll
        for (uint32_t i = 1; i < 8u; ++i) v = j == i ? k[i] : v;
        if constexpr (G == 2) {  // 2 lanes: no key in the record
        } else if constexpr (G == 4) {  // 4 lanes: key words j and j + 4
          uint32_t v2 = k[4];
#pragma unroll
          for (uint32_t i = 1; i < 4u; ++i) v2 = j == i ? k[4u + i] : v2;
          if (valid) {
            ((uint32_t*)RS(s).key)[j] = v;
            ((uint32_t*)RS(s).key)[j + 4u] = v2;
          }
        } else if (valid && j < 8u) {
          ((uint32_t*)RS(s).key)[j] = v;
        }
      } else if (G == 2) {
      } else if (valid && G == 4) {
        ((uint32_t*)RS(s).key)[j] = P.keys[8u * ks + j];
        ((uint32_t*)RS(s).key)[j + 4u] = P.keys[8u * ks + j + 4u];
      } else if (valid && j < 8u) {
        ((uint32_t*)RS(s).key)[j] = P.keys[8u * ks + j];
      }
      // all lanes active: swizzles read live lanes
      const uint32_t c0 = desc_word<G, 4>(dn), c1 = desc_word<G, 5>(dn);
      if (j == 0) {
        RS(s).addr = make_uint4(d0, d1, d2, d3);
        RS(s).meta = make_uint4(c0, c1, len, (valid ? 1u : 0u) | al | (G == 2 && valid ? ks << 8 : 0u));
      }
      round = 0;
      have = true;
      // prefetch the descriptor of the slot's following packet
      ++gen;
      {
        const uint32_t pos = batch_pos(g, gen, S);
        nxt = pos < P.n ? pkt_at<MX>(P, pos) : ~0u;
      }
      if constexpr (G == 2) {
        dn = desc_load2(P.desc, nxt, j);
      } else if constexpr (G == 4) {
        const uint2 w = desc_load4(P.desc, nxt, j);
        dn.x = w.x;
        dn.y = w.y;
      } else {
        dn.x = nxt != ~0u ? ((const uint32_t*)(P.desc + nxt))[j & 7u] : 0u;
      }
    }
    if (!__any(have)) break;
    wave_lds_sync();  // the slot records before the lanes read them
    WG_PH(0);

    // this round's packet parameters, read once (meta = {ctr lo, ctr hi, len, flags})
    const uint4 meta = RS(opaque_lane() >> SH).meta;
    const uint32_t len = meta.z;
    const uint32_t nb = (meta.w & 1u) ? ((len + 63u) >> 6) + 1u : 0u;
    uint32_t x[16];
    {
      // ---- payload prefetch: LDS-DMA straight into this lane's slice of the image ---------
      // (no registers held across the ARX rounds)
      const uint32_t lane = opaque_lane(), s = lane >> SH, j = lane & JM;
      const uint32_t b = G * round + j;
      // (a lambda called once: written inline, the same statements allocate registers differently in every
      // transport kernel, and this file's measurements are of the code as it is)
      auto payload_dma = [&]() {
      if (have && b < nb && b > 0u) {
        const uint32_t off = 64u * (b - 1u);
        const uint32_t nbytes = min(64u, len - off);
        const uint4 ad = RS(s).addr;
        const uint8_t* src = P.in + (((uint64_t)ad.x | ((uint64_t)ad.y << 32)) + off);
        if (meta.w & 2u) {
          // chunks holding a valid byte, each read whole (an aligned 16-B read stays in the granule
          // of its first byte); lane i's chunk q lands at img[q * 64 + i]
          __builtin_amdgcn_global_load_lds((gbl_cvoid*)src, (lds_void*)&img[0], 16, 0, 0);
          if (nbytes > 16u) __builtin_amdgcn_global_load_lds((gbl_cvoid*)(src + 16), (lds_void*)&img[64], 16, 0, 0);
          if (nbytes > 32u) __builtin_amdgcn_global_load_lds((gbl_cvoid*)(src + 32), (lds_void*)&img[128], 16, 0, 0);
          if (nbytes > 48u) __builtin_amdgcn_global_load_lds((gbl_cvoid*)(src + 48), (lds_void*)&img[192], 16, 0, 0);
        } else {  // unaligned input: the same image, staged through registers one chunk at a time
#pragma unroll
          for (uint32_t q = 0; q < 4u; ++q)
            if (16u * q < nbytes) img[64u * q + lane] = chunk_any(src + 16u * q, min(16u, nbytes - 16u * q));
        }
      }
      };
      payload_dma();
      // ---- ChaCha20: block b = 8 round + j ----------------------------------------------
      if (G > 2 && __any(have && round == 0)) {  // a new packet: its columns 1..3 of the first round, once
        const uint32_t c = j & 3u;
        const uint4* kl = RS(s).key;
        const uint4 ka = kl[0], kb = kl[1];
        uint32_t a = c == 1u ? 0x3320646eu : c == 2u ? 0x79622d32u : 0x6b206574u;
        uint32_t bb = c == 1u ? ka.y : c == 2u ? ka.z : ka.w;
        uint32_t cc = c == 1u ? kb.y : c == 2u ? kb.z : kb.w;
        uint32_t d = c == 1u ? meta.x : c == 2u ? meta.y : 0u;
        chacha20_qr(a, bb, cc, d);
        if (have && round == 0) {
          hc[0] = a; hc[1] = bb; hc[2] = cc; hc[3] = d;
        }
      }
      if constexpr (G == 2) {  // no lanes 1..3 to hold the hoisted columns: the whole block
        // (every lane computes a block, also one whose slot has no packet and whose record is stale: its key
        // index is 0 then, and any index is clamped to the table)
        const uint32_t kidx = have ? min(meta.w >> 8, P.key_slots - 1u) : 0u;
        chacha20_block_full((const uint4*)(P.keys + 8u * kidx), b, meta.x, meta.y, 0u, x);
      } else {
        const uint32_t H[12] = {bcastg<G, 1>(hc[0]), bcastg<G, 1>(hc[1]), bcastg<G, 1>(hc[2]), bcastg<G, 1>(hc[3]),
                                bcastg<G, 2>(hc[0]), bcastg<G, 2>(hc[1]), bcastg<G, 2>(hc[2]), bcastg<G, 2>(hc[3]),
                                bcastg<G, 3>(hc[0]), bcastg<G, 3>(hc[1]), bcastg<G, 3>(hc[2]), bcastg<G, 3>(hc[3])};
        chacha20_block_hoisted(RS(s).key, b, meta.x, meta.y, 0u, H, x);
      }
    }

    const bool mac_pass = !VF || !(meta.w & kDecryptPass);  // the second pass of a verify-first open only decrypts
    if (__any(have && round == 0 && mac_pass)) {  // round 0: lane 0 of the slot holds the one-time key r || s
      const uint32_t lane = opaque_lane(), s = lane >> SH;
      if (have && round == 0 && mac_pass && (lane & JM) == 0) {
        RS(s).R0 = make_uint4(x[0], x[1], x[2], x[3]);  // raw r, replaced by R = r^8 below
        if constexpr (G == 2) {
          RS(s).R1 = make_uint4(0u, x[4], x[5], x[6]);
          RS(s).R2.x = x[7];
        } else {
          RS(s).s = make_uint4(x[4], x[5], x[6], x[7]);
        }
      }
    }

    WG_PH(1);
    // ---- XOR, store, MAC input into the image, one 16-B chunk at a time ----------------------
    {
      const uint32_t lane = opaque_lane(), s = lane >> SH, j = lane & JM;
      const uint32_t b = G * round + j;
      if (have && b < nb && b > 0u) {
        const uint32_t off = 64u * (b - 1u);
        const uint32_t nbytes = min(64u, len - off);
        const uint4 ad = RS(s).addr;
        uint8_t* dst = P.out + (((uint64_t)ad.z | ((uint64_t)ad.w << 32)) + off);
        const uint32_t oal = meta.w & 12u;  // bit 2: 16-B aligned output, bit 3: 4-B aligned
        // the payload DMA (and the staged loads) must have landed in LDS: the compiler does not
        // always see the LDS-DMA -> ds_read dependence, so wait for it explicitly
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) {
          if (16u * q < nbytes) {
            const uint32_t cb = min(16u, nbytes - 16u * q);  // valid bytes in this chunk
            uint4 v = img[64u * q + lane];  // payload (the compiler waits for the DMA before this read)
            // open: the MAC input is the zero-padded ciphertext; seal masks the ciphertext below instead
            if (MODE == WG_MODE_OPEN && cb < 16u) v = mask_chunk(v, cb);
            if constexpr (MODE == WG_MODE_OPEN) {
              if (cb < 16u) img[64u * q + lane] = v;  // the MAC input is the zero-padded ciphertext
            }
            uint4 o = make_uint4(x[4 * q] ^ v.x, x[4 * q + 1] ^ v.y, x[4 * q + 2] ^ v.z, x[4 * q + 3] ^ v.w);
            if constexpr (MODE == WG_MODE_SEAL) {
              if (cb < 16u) o = mask_chunk(o, cb);
              img[64u * q + lane] = o;  // the MAC input is the ciphertext
            }
            if (!VF || (meta.w & (kVerifyFirst | kDecryptPass)) != kVerifyFirst)
              store_chunk(dst + 16u * q, cb, o, oal);
          }
        }
      }
    }
    // the length block le64(0) || le64(len) is MAC chunk nc (the first after the data): the lane
    // whose counter block holds it writes it into the image, so the Horner steps read it like data
    {
      const uint32_t lane = opaque_lane(), j = lane & JM;
      const uint32_t nc = (len + 15u) >> 4;
      if (have && (meta.w & 1u) && G * round + j == (nc >> 2) + 1u) {
        img[64u * (nc & 3u) + lane] = make_uint4(0u, 0u, len, 0u);
      }
    }
    wave_lds_sync();
    WG_PH(2);

    // ---- round 0: r^1..r^G (lane j gets r^(j+1)), R = r^G, W = r^(G-j) --------------------
    // (after the XOR phase, so the 32 registers of keystream and payload are free again)
    if (__any(have && round == 0 && mac_pass)) {
      if (have && round == 0 && mac_pass) {
        const uint32_t lane = opaque_lane(), s = lane >> SH, j = lane & JM;
        const uint4 rr = RS(s).R0;
        uint32_t y[5];
        poly_r_limbs(rr.x, rr.y, rr.z, rr.w, y);
#pragma unroll
        for (uint32_t st = 1; st < G; st <<= 1) {
          uint32_t z[5], zs[5];
#pragma unroll
          for (int i = 0; i < 5; ++i)
            z[i] = st == 1 ? shr_dpp<1>(y[i]) : st == 2 ? shr_dpp<2>(y[i]) : st == 4 ? shr_dpp<4>(y[i]) : shr_dpp<8>(y[i]);
          poly_scale5(z, zs);
          if (j >= st) poly_mul(y, z, zs);
        }
        uint32_t R[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          R[i] = bcastg<G, G - 1>(y[i]);
          W[i] = xorg<G - 1>(y[i]);
          acc[i] = 0;
        }
        if (j == 0) {
#ifdef WG_HORNER2
          // R and Q = R^2 (the two-chunk Horner step); their 5x forms are formed where used
          uint32_t Q[5] = {R[0], R[1], R[2], R[3], R[4]}, Rs[5];
          poly_scale5(R, Rs);
          poly_mul(Q, R, Rs);
          RS(s).R0 = make_uint4(R[0], R[1], R[2], R[3]);
          RS(s).R1 = make_uint4(R[4], Q[0], Q[1], Q[2]);
          RS(s).R2 = make_uint4(Q[3], Q[4], 0u, 0u);
#else
          RS(s).R0 = make_uint4(R[0], R[1], R[2], R[3]);
          if constexpr (G == 2) {
            RS(s).R1.x = R[4];
          } else {
            RS(s).R1 = make_uint4(R[4], 5u * R[1], 5u * R[2], 5u * R[3]);
            RS(s).R2 = make_uint4(5u * R[4], 0u, 0u, 0u);
          }
#endif
        }
      }
      wave_lds_sync();
    }

    WG_PH(3);
    // ---- Poly1305 over this round's chunks ------------------------------------------------------
    if (have && (meta.w & 1u) && mac_pass) {
      const uint32_t lane = opaque_lane(), s = lane >> SH, j = lane & JM;
      {
        const uint32_t nc = (len + 15u) >> 4;
        const uint32_t M = nc + 1u, D = G * ((M + JM) >> SH) - M;
        const uint32_t c_lo = round ? 4u * G * round - 4u : 0u;
        // chunk nc (after the data) is the length block le64(0) || le64(len): taken here when it
        // falls inside this round's window, at the finish otherwise
        const uint32_t c_end = min(nc + 1u, 4u * G * round + 4u * G - 4u);
        const uint32_t c0 = c_lo + ((j - ((c_lo + D) & JM)) & JM);
        // chunk ci of the round sits in lane (ci >> 2) + 1 - G round of the slot, row ci & 3
        const uint4* ip = &img[64u * (c0 & 3u) + (lane & ~JM) + ((c0 + 4u) >> 2) - G * round];
        const uint4 q0 = RS(s).R0, q1 = RS(s).R1, q2 = RS(s).R2;
#ifdef WG_HORNER2
        // (opt-in, -DWG_HORNER2) two chunks per reduction where the round has them:
        // acc = acc R^2 + m_t R + m_(t+1). Bit-exact, but it spills 2 VGPRs in k_step<8> and ran
        // C1 1.2% slower (C2 equal) in an alternating A/B (profiles/r04_horner2_ab.txt)
        const uint32_t R[5] = {q0.x, q0.y, q0.z, q0.w, q1.x};
        const uint32_t Rs[5] = {0u, 5u * q0.y, 5u * q0.z, 5u * q0.w, 5u * q1.x};
        const uint32_t Q[5] = {q1.y, q1.z, q1.w, q2.x, q2.y};
        const uint32_t Qs[5] = {0u, 5u * q1.z, 5u * q1.w, 5u * q2.x, 5u * q2.y};
        const uint32_t nst = c0 < c_end ? min(4u, (c_end - c0 + G - 1u) / G) : 0u;  // chunks this round
#pragma unroll
        for (uint32_t t = 0; t < 4u; t += 2u) {
          if (t < nst) {
            const uint4 v = ip[(G / 4u) * t];
            uint32_t m0[5];
            poly_block_limbs(v.x, v.y, v.z, v.w, 1u << 24, m0);
            if (t + 1u < nst) {
              if (round != 0 || t != 0) {
                poly_mul2(acc, Q, Qs, m0, R, Rs);
              } else {  // a packet's first two chunks: acc = m0 R (acc is still 0)
#pragma unroll
                for (int i = 0; i < 5; ++i) acc[i] = m0[i];
                poly_mul(acc, R, Rs);
              }
              // the second chunk is read after the product (its limbs are not live across it)
              const uint4 w = ip[(G / 4u) * (t + 1u)];
              uint32_t m1[5];
              poly_block_limbs(w.x, w.y, w.z, w.w, 1u << 24, m1);
#pragma unroll
              for (int i = 0; i < 5; ++i) acc[i] += m1[i];
            } else {
              if (round != 0 || t != 0) poly_mul(acc, R, Rs);
#pragma unroll
              for (int i = 0; i < 5; ++i) acc[i] += m0[i];
            }
          }
        }
#else
        const uint32_t R[5] = {q0.x, q0.y, q0.z, q0.w, q1.x};
        const uint32_t Rs[5] = {0u, G == 2 ? 5u * q0.y : q1.y, G == 2 ? 5u * q0.z : q1.z, G == 2 ? 5u * q0.w : q1.w,
                                G == 2 ? 5u * q1.x : q2.x};
#pragma unroll
        for (uint32_t t = 0; t < 4u; ++t) {
          if (c0 + G * t < c_end) {
            // (2-lane slots: chunk c0 + 2 t alternates rows, so its place is computed per step)
            uint4 v = G == 2 ? img[64u * ((c0 + 2u * t) & 3u) + (lane & ~JM) + ((c0 + 2u * t + 4u) >> 2) - G * round]
                             : ip[(G / 4u) * t];
            // acc is still 0 before a packet's first chunk (round 0, t = 0): no product needed
            if (round != 0 || t != 0) poly_mul(acc, R, Rs);
            uint32_t cl[5];
            poly_block_limbs(v.x, v.y, v.z, v.w, 1u << 24, cl);
#pragma unroll
            for (int i = 0; i < 5; ++i) acc[i] += cl[i];
          }
        }
#endif
      }
    }

    WG_PH(4);
    // ---- finish the packets whose last round this was ---------------------------------------
    const bool done = have && G * (round + 1u) >= nb;  // invalid packets (nb = 0) finish at once
    if (__any(done)) {
      if (done) {  // slot-uniform: every lane of a finishing slot is here
        const uint32_t lane = opaque_lane(), s = lane >> SH, j = lane & JM;
        const bool valid = meta.w & 1u;
        if (mac_pass) {
          if (valid) {
            if (j == JM && ((len + 15u) >> 4) >= 4u * G * round + 4u * G - 4u) {  // length block not taken in the loop
              const uint4 q0 = RS(s).R0, q1 = RS(s).R1;
              const uint32_t R[5] = {q0.x, q0.y, q0.z, q0.w, q1.x};
#ifdef WG_HORNER2
              const uint32_t Rs[5] = {0u, 5u * q0.y, 5u * q0.z, 5u * q0.w, 5u * q1.x};
#else
              const uint4 q2 = RS(s).R2;
              const uint32_t Rs[5] = {0u, G == 2 ? 5u * q0.y : q1.y, G == 2 ? 5u * q0.z : q1.z,
                                      G == 2 ? 5u * q0.w : q1.w, G == 2 ? 5u * q1.x : q2.x};
#endif
              poly_mul(acc, R, Rs);
              acc[2] += (len << 12) & M26;  // le64(len) at bit 64: limb 2 holds bits 52..77
              acc[3] += len >> 14;
              acc[4] += 1u << 24;
            }
            uint32_t Ws[5];
            poly_scale5(W, Ws);
            poly_mul(acc, W, Ws);
          }
#pragma unroll
          for (int i = 0; i < 5; ++i) {  // slot sum (every lane of the slot ends with it)
            acc[i] += xor1_dpp(acc[i]);
            if constexpr (G >= 4) acc[i] += xor2_dpp(acc[i]);
            if constexpr (G >= 8) acc[i] += xor4_dpp(acc[i]);
            if constexpr (G == 16) acc[i] += xor8_dpp(acc[i]);
          }
        }
        const uint4 ad = RS(s).addr;
        const uint8_t* inp = P.in + ((uint64_t)ad.x | ((uint64_t)ad.y << 32));
        uint8_t* outp = P.out + ((uint64_t)ad.z | ((uint64_t)ad.w << 32));
        uint32_t bad = valid ? 0u : 1u;
        bool again = false;  // a verify-first open whose tag verified: the decrypt pass comes next
        if (mac_pass && valid && j == 0) {
          const uint4 sv = G == 2 ? make_uint4(RS(s).R1.y, RS(s).R1.z, RS(s).R1.w, RS(s).R2.x) : RS(s).s;
          uint32_t tag[4];
          poly_finish(acc, sv.x, sv.y, sv.z, sv.w, tag);
          if constexpr (MODE == WG_MODE_SEAL) {
            uint8_t* tp = outp + len;
            if ((((uintptr_t)tp) & 15u) == 0) {
              *(uint4*)tp = make_uint4(tag[0], tag[1], tag[2], tag[3]);
            } else {
#pragma unroll
              for (int i = 0; i < 4; ++i) store_u32_any(tp + 4 * i, tag[i]);
            }
          } else {  // all 16 bytes compared, no early exit
            const uint8_t* tp = inp + len;
            uint32_t diff = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) diff |= load_u32_any(tp + 4 * i) ^ tag[i];
            bad = diff ? 1u : 0u;
          }
        }
        if constexpr (MODE == WG_MODE_OPEN) {
          bad = bcastg<G, 0>(bad);
          again = VF && mac_pass && !bad && (meta.w & kVerifyFirst);
        }
        if constexpr (MODE == WG_MODE_OPEN) {
          if (again) {  // decrypt pass: the same rounds again, keystream XOR and stores only
            if (j == 0) RS(s).meta.w = meta.w | kDecryptPass;
            round = ~0u;  // incremented to 0 below
          } else {
            if (j == 0 && P.status) {
              uint32_t st = bad ? WG_PKT_BADTAG : WG_PKT_OK;
              if (!bad && P.rx) {  // fused receive-side check on the plaintext this slot wrote
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's plaintext stores have landed
                st = rx_verdict(*P.rx, outp, len, P.desc[pkt].key_slot);
              }
              P.status[pkt] = st;
            }
            if (bad && valid && (!VF || !(meta.w & kVerifyFirst))) {  // scrub the unauthenticated plaintext written
              for (uint32_t i = j; i < len; i += G) outp[i] = 0;
            }
            have = false;
          }
        } else {
          have = false;
        }
      }
    }
    if (have) ++round;
    wave_lds_sync();  // this round's image and records before the next round rewrites them
    WG_PH(5);
  }
  WG_PH_STORE(blk * TW + wv);
}

// ---- the uniform-wave body (8-lane slots, one packet per slot: the WG_F_UNIFORM plan) -----------------
// Bulk traffic is runs of full-size packets of one session at aligned strides, so every slot of a wave
// usually holds a valid packet of ONE length, with 16-B aligned input and output, under ONE key. A wave
// checks exactly that on its own descriptors (ballots, no hint is trusted) and then runs this body INSTEAD
// of transport_body; a wave that fails any condition runs transport_body unchanged. What is uniform lives
// in SGPRs and is computed by the scalar unit, whose issue the VALU-bound launch does not pay for: the
// length and everything derived from it (block, round and MAC chunk counts, the Horner window), the round
// loop and its trip count, the place of the partial block and of the length block. Left per lane: the
// packet's offsets and counter, the lane's class (a full 64-B block, the one partial block of the packet,
// or none), the Horner start chunk. The arithmetic (ChaCha20 block, Poly1305 steps, r-power scan, slot
// sum, finish) is that of transport_body, bit for bit.
//
// Pieces of a packet's MAC and finish, as transport_body computes them:
// r^1..r^G by a scan over the slot (lane j gets r^(j+1)); R = r^G, W = r^(G-j)
template <int G>
__device__ __forceinline__ void rpow_scan(const uint4 rr, uint32_t j, uint32_t R[5], uint32_t W[5]) {
  uint32_t y[5];
  poly_r_limbs(rr.x, rr.y, rr.z, rr.w, y);
#pragma unroll
  for (uint32_t st = 1; st < G; st <<= 1) {
    uint32_t z[5], zs[5];
#pragma unroll
    for (int i = 0; i < 5; ++i)
      z[i] = st == 1 ? shr_dpp<1>(y[i]) : st == 2 ? shr_dpp<2>(y[i]) : st == 4 ? shr_dpp<4>(y[i]) : shr_dpp<8>(y[i]);
    poly_scale5(z, zs);
    if (j >= st) poly_mul(y, z, zs);
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    R[i] = bcastg<G, G - 1>(y[i]);
    W[i] = xorg<G - 1>(y[i]);
  }
}
// the slot's sum of the lanes' partials (every lane of the slot ends with it)
template <int G>
__device__ __forceinline__ void slot_sum(uint32_t acc[5]) {
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    acc[i] += xor1_dpp(acc[i]);
    if constexpr (G >= 4) acc[i] += xor2_dpp(acc[i]);
    if constexpr (G >= 8) acc[i] += xor4_dpp(acc[i]);
    if constexpr (G == 16) acc[i] += xor8_dpp(acc[i]);
  }
}
// the length block le64(0) || le64(len) as one more Horner step (taken at the finish when it falls outside the
// last round's window)
__device__ __forceinline__ void poly_len_block(uint32_t acc[5], const uint32_t R[5], const uint32_t Rs[5], uint32_t len) {
  poly_mul(acc, R, Rs);
  acc[2] += (len << 12) & M26;  // le64(len) at bit 64: limb 2 holds bits 52..77
  acc[3] += len >> 14;
  acc[4] += 1u << 24;
}
// one lane finishes the tag: seal stores it after the ciphertext, open compares all 16 bytes (no early exit).
// Returns 1 for a tag that does not verify.
template <int MODE>
__device__ __forceinline__ uint32_t tag_finish(uint32_t acc[5], const uint4 sv, const uint8_t* in_tag, uint8_t* out_tag) {
  uint32_t tag[4];
  poly_finish(acc, sv.x, sv.y, sv.z, sv.w, tag);
  if constexpr (MODE == WG_MODE_SEAL) {
    if ((((uintptr_t)out_tag) & 15u) == 0) {
      *(uint4*)out_tag = make_uint4(tag[0], tag[1], tag[2], tag[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) store_u32_any(out_tag + 4 * i, tag[i]);
    }
    return 0u;
  } else {
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) diff |= load_u32_any(in_tag + 4 * i) ^ tag[i];
    return diff ? 1u : 0u;
  }
}
// an opened packet's status (lane 0 of the slot; with WG_F_RX_FILTER the receive-side verdict on the plaintext
// this slot wrote) and, for a tag that did not verify, the scrub of the plaintext written (all lanes of the slot)
template <int G>
__device__ __forceinline__ void open_result(const TransportParams& P, uint32_t pkt, uint32_t j, uint32_t bad, bool scrub,
                                            uint8_t* outp, uint32_t len, uint32_t key_slot) {
  if (j == 0 && P.status) {
    uint32_t st = bad ? WG_PKT_BADTAG : WG_PKT_OK;
    if (!bad && P.rx) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's plaintext stores have landed
      st = rx_verdict(*P.rx, outp, len, key_slot);
    }
    P.status[pkt] = st;
  }
  if (scrub) {
    for (uint32_t i = j; i < len; i += G) outp[i] = 0;
  }
}

// the Horner steps of a lane over the round's image (8-lane slots: the lane's chunks are 2 image columns apart;
// up to four, each tests its chunk against the window's end). first: the packet's first round (scalar), whose
// first step needs no product (acc is still 0).
__device__ __forceinline__ void horner_round8(uint32_t acc[5], const uint4* ip, const uint32_t R[5], const uint32_t Rs[5],
                                              uint32_t c0, uint32_t c_end, bool first) {
#pragma unroll
  for (uint32_t t = 0; t < 4u; ++t) {
    if (c0 + 8u * t < c_end) {
      const uint4 v = ip[2u * t];
      if (t != 0 || !first) poly_mul(acc, R, Rs);
      uint32_t cl[5];
      poly_block_limbs(v.x, v.y, v.z, v.w, 1u << 24, cl);
#pragma unroll
      for (int i = 0; i < 5; ++i) acc[i] += cl[i];
    }
  }
}

// LDS-DMA of chunk Q of this lane's block: 16 B at src + 16 Q to img[64 Q + lane]. The instruction offset is
// added to the global AND the LDS address, so the LDS base (M0, scalar) is taken back by it.
template <uint32_t Q>
__device__ __forceinline__ void dma_chunk(const uint8_t* src, uint4* img) {
  __builtin_amdgcn_global_load_lds((gbl_cvoid*)src, (lds_void*)((char*)img + (1024u - 16u) * Q), 16, 16 * Q, 0);
}

// The body of a wave that passed the test (transport_body_uni): len, ks0 scalar; cw0 / cw1 the packet's
// counter; soff / doff this lane's block of round 0 in the input / output (block 0: 64 B before the packet);
// live: the lane's slot has a packet (the grid's last wave may have fewer than 8).
template <int MODE>
__device__ __forceinline__ void uni_run(const TransportParams& P, uint32_t wg, uint4* const img, SlotRec* const rec,
                                        uint32_t len, uint32_t ks0, uint32_t cw0, uint32_t cw1, uint64_t soff,
                                        uint64_t doff, bool live) {
  constexpr uint32_t G = 8, SH = 3, JM = 7;
  constexpr uint32_t kNone = 0x40000000u;  // "data block" of a lane whose slot has no packet: never a block of any
  WG_PH_DECL
  // everything below that depends only on len is scalar
  const uint32_t nfull = len >> 6, tail = len & 63u;    // full 64-B blocks, bytes of the partial one
  const uint32_t rounds = (((len + 63u) >> 6) + 8u) >> 3;  // counter blocks 0..nblk in rounds of 8
  const uint32_t pround = tail ? (nfull + 1u) >> 3 : ~0u;  // the round that holds the partial block
  const uint32_t nc = (len + 15u) >> 4, M = nc + 1u, D = G * ((M + JM) >> SH) - M;
  // the session key: through the scalar cache into ONE record of the wave, which every lane's block reads as a
  // broadcast
  uint32_t hc[4];
  {
    const uint32_t lane = opaque_lane(), j = lane & JM;
    const WG_CONST uint32_t* kp = (const WG_CONST uint32_t*)P.keys + 8u * ks0;
    uint32_t k[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      k[i] = kp[i];
      asm volatile("" : "+s"(k[i]));
    }
    if (lane == 0) {
      rec[0].key[0] = make_uint4(k[0], k[1], k[2], k[3]);
      rec[0].key[1] = make_uint4(k[4], k[5], k[6], k[7]);
    }
    // the packet's columns 1..3 of the first round, once (lanes 1..3 of the slot feed its blocks)
    const uint32_t c = j & 3u;
    hc[0] = c == 1u ? 0x3320646eu : c == 2u ? 0x79622d32u : 0x6b206574u;
    hc[1] = c == 1u ? k[1] : c == 2u ? k[2] : k[3];
    hc[2] = c == 1u ? k[5] : c == 2u ? k[6] : k[7];
    hc[3] = c == 1u ? cw0 : c == 2u ? cw1 : 0u;
    chacha20_qr(hc[0], hc[1], hc[2], hc[3]);
  }
  const uint32_t bj = live ? (opaque_lane() & JM) - 1u : kNone;  // data block of round 0 (block 0's lane wraps)
  uint32_t acc[5], W[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) acc[i] = W[i] = 0;
  wave_lds_sync();  // the key and the offsets before the lanes read them
  WG_PH(10);

  for (uint32_t round = 0; round < rounds; ++round) {  // a scalar loop
    uint32_t x[16];
    const uint32_t db = G * round + bj;  // this lane's data block (counter block db + 1)
    {
      const uint32_t lane = opaque_lane(), j = lane & JM;
      const uint8_t* src = (P.in + 64u * G * round) + soff;
      if (db < nfull) {
        dma_chunk<0>(src, img);
        dma_chunk<1>(src, img);
        dma_chunk<2>(src, img);
        dma_chunk<3>(src, img);
      }
      if (round == pround) {  // scalar: at most one lane per slot, chunks holding a valid byte read whole
        if (db == nfull) {
          dma_chunk<0>(src, img);
          if (tail > 16u) dma_chunk<1>(src, img);
          if (tail > 32u) dma_chunk<2>(src, img);
          if (tail > 48u) dma_chunk<3>(src, img);
        }
      }
      const uint32_t H[12] = {bcast8<1>(hc[0]), bcast8<1>(hc[1]), bcast8<1>(hc[2]), bcast8<1>(hc[3]),
                              bcast8<2>(hc[0]), bcast8<2>(hc[1]), bcast8<2>(hc[2]), bcast8<2>(hc[3]),
                              bcast8<3>(hc[0]), bcast8<3>(hc[1]), bcast8<3>(hc[2]), bcast8<3>(hc[3])};
      chacha20_block_hoisted(rec[0].key, G * round + j, cw0, cw1, 0u, H, x);
    }
    if (round == 0) {  // lane 0 of the slot holds the one-time key r || s
      const uint32_t lane = opaque_lane(), s = lane >> SH;
      if ((lane & JM) == 0) {
        rec[s].R0 = make_uint4(x[0], x[1], x[2], x[3]);  // raw r, replaced by R = r^8 below
        rec[s].s = make_uint4(x[4], x[5], x[6], x[7]);
      }
    }
    WG_PH(11);
    // ---- XOR, store, MAC input into the image -------------------------------------------------
    {
      const uint32_t lane = opaque_lane();
      uint8_t* dst = (P.out + 64u * G * round) + doff;
      if (db < nfull) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the DMA has landed in LDS
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) {
          const uint4 v = img[64u * q + lane];
          const uint4 o = make_uint4(x[4 * q] ^ v.x, x[4 * q + 1] ^ v.y, x[4 * q + 2] ^ v.z, x[4 * q + 3] ^ v.w);
          if constexpr (MODE == WG_MODE_SEAL) img[64u * q + lane] = o;  // the MAC input is the ciphertext
          *(uint4*)(dst + 16u * q) = o;
        }
      }
      if (round == pround) {
        if (db == nfull) {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          // (once per packet: the chunk arithmetic stays in this lane's registers, as in transport_body; left
          // scalar, every test of it becomes a loop invariant held in SGPRs across the rounds)
          uint32_t tl = tail;
          asm volatile("" : "+v"(tl));
#pragma unroll
          for (uint32_t q = 0; q < 4u; ++q) {
            if (16u * q < tl) {
              const uint32_t cb = min(16u, tl - 16u * q);  // valid bytes in this chunk
              uint4 v = img[64u * q + lane];
              if constexpr (MODE == WG_MODE_OPEN) {
                if (cb < 16u) {  // the MAC input is the zero-padded ciphertext
                  v = mask_chunk(v, cb);
                  img[64u * q + lane] = v;
                }
              }
              uint4 o = make_uint4(x[4 * q] ^ v.x, x[4 * q + 1] ^ v.y, x[4 * q + 2] ^ v.z, x[4 * q + 3] ^ v.w);
              if constexpr (MODE == WG_MODE_SEAL) {
                if (cb < 16u) o = mask_chunk(o, cb);
                img[64u * q + lane] = o;
              }
              store_chunk(dst + 16u * q, cb, o, 12u);
            }
          }
        }
      }
      // the length block is MAC chunk nc: written into the image by the lane whose counter block holds it
      if (round == ((nc >> 2) + 1u) >> 3) {
        if (db == (nc >> 2)) img[64u * (nc & 3u) + lane] = make_uint4(0u, 0u, len, 0u);
      }
    }
    wave_lds_sync();
    WG_PH(12);
    if (round == 0) {
      const uint32_t lane = opaque_lane(), s = lane >> SH, j = lane & JM;
      uint32_t R[5];
      rpow_scan<8>(rec[s].R0, j, R, W);
      if (j == 0) {
        rec[s].R0 = make_uint4(R[0], R[1], R[2], R[3]);
        rec[s].R1 = make_uint4(R[4], 5u * R[1], 5u * R[2], 5u * R[3]);
        rec[s].R2 = make_uint4(5u * R[4], 0u, 0u, 0u);
      }
      wave_lds_sync();
    }
    WG_PH(13);
    // ---- Poly1305 over this round's chunks: the window is scalar, its start chunk per lane ------
    {
      const uint32_t lane = opaque_lane(), s = lane >> SH, j = lane & JM;
      const uint32_t c_lo = round ? 4u * G * round - 4u : 0u;
      const uint32_t c_end = min(nc + 1u, 4u * G * round + 4u * G - 4u);
      const uint32_t c0 = c_lo + ((j - ((c_lo + D) & JM)) & JM);
      const uint4* ip = &img[64u * (c0 & 3u) + (lane & ~JM) + ((c0 + 4u) >> 2) - G * round];
      const uint4 q0 = rec[s].R0, q1 = rec[s].R1, q2 = rec[s].R2;
      const uint32_t R[5] = {q0.x, q0.y, q0.z, q0.w, q1.x};
      const uint32_t Rs[5] = {0u, q1.y, q1.z, q1.w, q2.x};
      horner_round8(acc, ip, R, Rs, c0, c_end, round == 0);
    }
    WG_PH(14);
    wave_lds_sync();  // this round's image before the next round rewrites it
  }

  // ---- finish: every slot's packet ends with the loop -------------------------------------------
  {
    const uint32_t lane = opaque_lane(), s = lane >> SH, j = lane & JM;
    if (nc >= 4u * G * rounds - 4u) {  // length block not taken in the loop (scalar)
      if (j == JM) {
        const uint4 q0 = rec[s].R0, q1 = rec[s].R1, q2 = rec[s].R2;
        const uint32_t R[5] = {q0.x, q0.y, q0.z, q0.w, q1.x};
        const uint32_t Rs[5] = {0u, q1.y, q1.z, q1.w, q2.x};
        poly_len_block(acc, R, Rs, len);
      }
    }
    uint32_t Ws[5];
    poly_scale5(W, Ws);
    poly_mul(acc, W, Ws);
    slot_sum<8>(acc);
    const uint4 ad = rec[s].addr;
    const uint8_t* inp = P.in + ((uint64_t)ad.x | ((uint64_t)ad.y << 32));
    uint8_t* outp = P.out + ((uint64_t)ad.z | ((uint64_t)ad.w << 32));
    uint32_t bad = 0u;
    if (live && j == 0) bad = tag_finish<MODE>(acc, rec[s].s, inp + len, outp + len);
    if constexpr (MODE == WG_MODE_OPEN) {
      bad = bcast8<0>(bad);
      if (live) open_result<8>(P, wg * G + s, j, bad, bad != 0u, outp, len, ks0);
    }
  }
  WG_PH(15);
}

// The test, then one of the two bodies. transport_body has ONE call site, reached with nothing of the test live.
template <int MODE>
__device__ __forceinline__ void transport_body_uni(const TransportParams& P, uint32_t blk, uint32_t wv, uint4* const img,
                                                   SlotRec* const rec, uint32_t& iter) {
  static_assert(MODE == WG_MODE_SEAL || MODE == WG_MODE_OPEN, "transport modes only");
  constexpr uint32_t G = 8, SH = 3, JM = 7;
  const uint32_t wg = blk * TW + wv;
#ifndef WG_HORNER2  // (the two-chunk Horner keeps other slot records)
  // the plan the uniform body assumes, from the launch's own parameters (scalar): batch order, one packet per
  // slot, no issue-priority schedule
  if (P.order == nullptr && P.prio_step == 0u && P.n <= P.slots) {
    const uint32_t lane = opaque_lane(), s = lane >> SH, j = lane & JM;
    const uint32_t g = wg * G + s;
    const bool live = g < P.n;
    if (!__any(live)) return;  // a wave past the batch (the grid is whole workgroups)
    const uint32_t dw = live ? ((const uint32_t*)(P.desc + g))[j] : 0u;
    const uint32_t d0 = bcast8<0>(dw), d1 = bcast8<1>(dw), d2 = bcast8<2>(dw), d3 = bcast8<3>(dw);
    const uint32_t cw0 = bcast8<4>(dw), cw1 = bcast8<5>(dw);
    const uint32_t lv = bcast8<6>(dw), ks = bcast8<7>(dw);
    const uint64_t in_off = (uint64_t)d0 | ((uint64_t)d1 << 32);
    const uint64_t out_off = (uint64_t)d2 | ((uint64_t)d3 << 32);
    const bool valid = transport_valid<MODE>(in_off, out_off, lv, ks, P.max_len, P.key_slots, P.in_size, P.out_size);
    const uintptr_t ia = (uintptr_t)(P.in + in_off), oa = (uintptr_t)(P.out + out_off);
    // lane 0 is live (slots take the batch's positions in order): its packet sets the wave's length and key
    const uint32_t len = __builtin_amdgcn_readfirstlane(lv);
    const uint32_t ks0 = __builtin_amdgcn_readfirstlane(ks);
    const bool ok = valid && lv == len && ks == ks0 && ((ia | oa) & 15u) == 0;
    if (!__any(live && !ok)) {
      if (j == 0) rec[s].addr = make_uint4(d0, d1, d2, d3);
      const uint64_t lo = (uint64_t)(64u * j) - 64u;
      uni_run<MODE>(P, wg, img, rec, len, ks0, cw0, cw1, in_off + lo, out_off + lo, live);
      return;
    }
  }
#endif
  transport_body<MODE, 8, false, 0>(P, blk, wv, img, rec, iter);
}

template <int MODE>
__global__ void __launch_bounds__(64 * TW) __attribute__((amdgpu_waves_per_eu(8))) k_transport_uni(TransportParams P) {
  __shared__ uint4 img_[TW][4 * 64];
  __shared__ SlotRec rec_[TW][8];
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t iter = 0;
  transport_body_uni<MODE>(P, blockIdx.x, wv, img_[wv], rec_[wv], iter);
}

// VF: an open whose input and output buffers overlap (the host checks the two ranges): packets
// that overlap themselves verify first (kVerifyFirst); every other launch takes the one-pass body
template <int MODE, int G = 8, bool VF = false>
__global__ void __launch_bounds__(64 * TW) __attribute__((amdgpu_waves_per_eu(8))) k_transport(TransportParams P) {
  __shared__ uint4 img_[TW][4 * 64];         // 4 KB per wave: [chunk q][lane] = the round's payload / MAC input
  __shared__ SlotRec rec_[TW][64 / G < 8 ? 8 : 64 / G];  // one record per slot: 1 KB per wave (2 KB with 4-lane slots)
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t iter = 0;
  transport_body<MODE, G, VF>(P, blockIdx.x, wv, img_[wv], rec_[wv], iter);
}

// ---- mixed-length batches: 16-lane slots for the long packets, 8- (or 4-) lane slots for the rest ----
// The batch is ordered longest-first (k_lpt_*); the n_long packets at its front (more than
// `split` rounds of 8 blocks) take 16-lane slots, so no slot runs much more than `split` rounds.
// GS: lanes of the short packets' slots (8, or 4 for batches of short packets: half the ChaCha20 lanes
// a 40-B packet leaves idle, and the per-packet work shared by 16 packets of a wave instead of 8).
// Every slot holds ONE packet and the grid has as many workgroups as that takes (more than are
// resident): the hardware dispatcher starts each new workgroup as an old one retires, longest
// packets first. Workgroups [0, b16) run the 16-lane body, [b16, b16 + b8) the 8-lane body; the
// rest of the (host-sized, upper-bound) grid exits at once.
template <int GS = 8, int GT = 0>
__device__ __forceinline__ int mixed_part(const TransportParams& P, uint32_t blk, TransportParams& Q, uint32_t& qblk) {
  Q = P;
  uint32_t nl, nt = 0;
  if (P.bin_cnt) {  // one-launch planning: the bins' counts, the long packets those of keys above the split
    nl = 0;
#pragma unroll
    for (uint32_t k = 0; k < kFastBins; ++k) {
      const uint32_t c = ((const WG_CONST uint32_t*)P.bin_cnt)[k * kCntStride];
      nl += k > P.split ? c : 0u;
      if constexpr (GT != 0) nt += k <= P.split2 ? c : 0u;  // (split2 = 0: only key 0, the invalid packets)
    }
    nl = min(nl, P.n);
    if constexpr (GT != 0) nt = P.split2 ? min(nt, P.n - nl) : 0u;
  } else {
    nl = min(__builtin_amdgcn_readfirstlane(*(const WG_CONST uint32_t*)P.n_long), P.n);
  }
  const uint32_t b16 = (nl + 4u * TW - 1u) / (4u * TW);
  if (blk < b16) {
    Q.n = nl;
    Q.slots = b16 * TW * 4u;
    qblk = blk;
    return 16;
  }
  constexpr uint32_t spw = 64u / GS;  // short slots per wave
  const uint32_t ns = P.n - nl - nt, bs = (ns + spw * TW - 1u) / (spw * TW);
  if (blk - b16 < bs) {
    if (P.bin_cnt) Q.pos_base = nl;  // the sparse order's positions run on past the long packets
    else Q.order = P.order + nl;
    Q.n = ns;
    Q.slots = bs * TW * spw;
    qblk = blk - b16;
    return GS;
  }
  if constexpr (GT != 0) {  // the tiny packets (keys <= split2, at the end of the order) in GT-lane slots
    constexpr uint32_t tpw = 64u / GT;
    const uint32_t bt = (nt + tpw * TW - 1u) / (tpw * TW);
    if (blk - b16 - bs < bt) {
      Q.pos_base = nl + ns;
      Q.n = nt;
      Q.slots = bt * TW * tpw;
      qblk = blk - b16 - bs;
      return GT;
    }
  }
  return 0;
}

template <int MODE, bool VF = false, int GS = 8>
__global__ void __launch_bounds__(64 * TW) __attribute__((amdgpu_waves_per_eu(8))) k_transport_mixed(TransportParams P) {
  __shared__ uint4 img_[TW][4 * 64];
  __shared__ SlotRec rec_[TW][64 / GS];
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  TransportParams Q;
  uint32_t qb = 0, iter = 0;
  const int g = mixed_part<GS>(P, blockIdx.x, Q, qb);
  if (g == 16) transport_body<MODE, 16, VF, (int)kFastBins>(Q, qb, wv, img_[wv], rec_[wv], iter);
  else if (g == GS) transport_body<MODE, GS, VF, (int)kFastBins>(Q, qb, wv, img_[wv], rec_[wv], iter);
}

// GT = 2: a third part after the GS-lane one, the tiny packets (keys <= split2) in 2-lane slots (32 per wave:
// a 40-B packet's two blocks fill its lanes instead of half of a 4-lane slot). Its records need twice the LDS.
template <int GS = 8, int GT = 0>
__global__ void __launch_bounds__(64 * TW) __attribute__((amdgpu_waves_per_eu(8)))
k_step_mixed(TransportParams S, TransportParams O) {
  __shared__ uint4 img_[TW][4 * 64];
  // slot records: 128 B per GS- or 16-lane slot, 80 B per 2-lane slot (transport_body's kRecStride)
  constexpr uint32_t kRecU4 = GT ? ((64 / GS) * 8 > (64 / GT) * 5 ? (64 / GS) * 8 : (64 / GT) * 5) : (64 / GS) * 8;
  __shared__ uint4 recraw_[TW][kRecU4];
  SlotRec* const rec = (SlotRec*)recraw_[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  TransportParams QS, QO;
  uint32_t qb = 0, qb2 = 0, iter = 0;
  const int g = mixed_part<GS, GT>(S, blockIdx.x, QS, qb);
  (void)mixed_part<GS, GT>(O, blockIdx.x, QO, qb2);  // the same split: the open batch has the seal's lengths
  if (g == 16) {
    transport_body<WG_MODE_SEAL, 16, false, (int)kFastBins>(QS, qb, wv, img_[wv], rec, iter);
    asm volatile("s_waitcnt vmcnt(0)\n\tbuffer_inv sc0" ::: "memory");
    transport_body<WG_MODE_OPEN, 16, false, (int)kFastBins>(QO, qb, wv, img_[wv], rec, iter);
  } else if (g == GS) {
    transport_body<WG_MODE_SEAL, GS, false, (int)kFastBins>(QS, qb, wv, img_[wv], rec, iter);
    asm volatile("s_waitcnt vmcnt(0)\n\tbuffer_inv sc0" ::: "memory");
    transport_body<WG_MODE_OPEN, GS, false, (int)kFastBins>(QO, qb, wv, img_[wv], rec, iter);
  } else if constexpr (GT != 0) {
    if (g == GT) {
      transport_body<WG_MODE_SEAL, GT, false, (int)kFastBins>(QS, qb, wv, img_[wv], rec, iter);
      asm volatile("s_waitcnt vmcnt(0)\n\tbuffer_inv sc0" ::: "memory");
      transport_body<WG_MODE_OPEN, GT, false, (int)kFastBins>(QO, qb, wv, img_[wv], rec, iter);
    }
  }
}

// One launch, two directions (wg_duplex_batch): a node's outgoing batch sealed and its
// incoming batch opened side by side. Workgroups [0, 2m) alternate seal / open (m = the
// smaller grid), the rest belong to the larger direction; each half runs exactly the
// k_transport body on its own grid, so the bytes written are those of the two separate
// launches. The two halves share the LDS declared here (one image + records per wave).
__global__ void __launch_bounds__(64 * TW) __attribute__((amdgpu_waves_per_eu(8)))
k_duplex(TransportParams S, TransportParams O, uint32_t seal_blocks, uint32_t open_blocks) {
  __shared__ uint4 img_[TW][4 * 64];
  __shared__ SlotRec rec_[TW][8];
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t m = min(seal_blocks, open_blocks);
  const uint32_t b = blockIdx.x;
  bool seal;
  uint32_t idx;
  if (b < 2u * m) {
    seal = (b & 1u) == 0u;
    idx = b >> 1;
  } else {
    seal = seal_blocks > open_blocks;
    idx = b - m;
  }
  uint32_t iter = 0;
  if (seal) transport_body<WG_MODE_SEAL>(S, idx, wv, img_[wv], rec_[wv], iter);
  else transport_body<WG_MODE_OPEN>(O, idx, wv, img_[wv], rec_[wv], iter);
}

// One launch, one dependent step (wg_duplex_batch with WG_F_AFTER_SEAL): every wave seals its
// packets and then opens the same batch positions of the open batch, which read what its own
// seal wrote (open packet i is ordered after seal packet i, include/wgaead.h). Both halves use one
// grid and one packet order, so slot g opens exactly the packets it sealed. The waves that finish
// sealing first start opening while the others still seal: the seal launch's tail and the open
// launch's start, which two back-to-back launches leave partly idle, overlap.
// WPE: the waves per SIMD the register allocation targets. 8 (64 VGPRs) everywhere, except a grid
// that holds at most half the resident waves anyway (the persistent longest-first pairs of a
// mixed batch: 4 waves per SIMD), which takes the WPE = 4 build (66 VGPRs and no SGPR spills,
// against 64 VGPRs and 12 SGPRs spilled to VGPR lanes).
// Test hook of k_step (WG_TEST_STEP_FLIP, never set in production): between the two halves, lane 0 of
// each slot flips bit 0 of the tag its seal wrote for the slot's first packet (batch position g) when
// that packet's index is a multiple of S.test_flip. The open half then rejects it and the ciphertext
// differs from the reference, so the bench's check of the k_step output it timed must fail
// (tests/test_gpu_bench.py). Outside transport_body: the product body's code is unchanged.
template <int G>
__device__ __forceinline__ void step_test_flip(const TransportParams& S, uint32_t blk, uint32_t wv, uint32_t flip) {
  const uint32_t lane = threadIdx.x & 63u, g = (blk * TW + wv) * (64u / G) + lane / G;
  if ((lane & (G - 1u)) == 0u && g < S.n) {
    const uint32_t i = S.order ? S.order[g] : g;
    const wg_pkt d = S.desc[i];
    if ((i & (flip - 1u)) == 0u &&
        transport_valid<WG_MODE_SEAL>(d.in_off, d.out_off, d.len, d.key_slot, S.max_len, S.key_slots, S.in_size,
                                      S.out_size))
      S.out[d.out_off + d.len] ^= 1u;
  }
  asm volatile("s_waitcnt vmcnt(0)\n\tbuffer_inv sc0" ::: "memory");
}

// FLIP: the test-hook instantiation (WG_TEST_STEP_FLIP), launched only by the test library (WG_TEST_HOOKS);
// the product instantiations carry no hook code at all.
template <int G = 8, int WPE = 8, bool FLIP = false, int MX = 0>
__global__ void __launch_bounds__(64 * TW) __attribute__((amdgpu_waves_per_eu(WPE)))
k_step(TransportParams S, TransportParams O, uint32_t test_flip) {
  __shared__ uint4 img_[TW][4 * 64];
  __shared__ SlotRec rec_[TW][64 / G < 8 ? 8 : 64 / G];
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t iter = 0;  // one issue-priority schedule over both halves (plan_transport: prio_step of the step)
  transport_body<WG_MODE_SEAL, G, false, MX>(S, blockIdx.x, wv, img_[wv], rec_[wv], iter);
  // the open reads the ciphertext and tags this wave just stored: wait until the stores are
  // performed and drop this CU's L1 lines (an in-place seal read the plaintext through them)
  asm volatile("s_waitcnt vmcnt(0)\n\tbuffer_inv sc0" ::: "memory");
  if constexpr (FLIP) step_test_flip<G>(S, blockIdx.x, wv, test_flip);
  transport_body<WG_MODE_OPEN, G, false, MX>(O, blockIdx.x, wv, img_[wv], rec_[wv], iter);
}

// k_step for the uniform plan's 8-lane slots: each half decides for itself, wave by wave, between the
// uniform-wave body and transport_body (transport_body_uni).
template <int WPE = 8>
__global__ void __launch_bounds__(64 * TW) __attribute__((amdgpu_waves_per_eu(WPE)))
k_step_uni(TransportParams S, TransportParams O) {
  __shared__ uint4 img_[TW][4 * 64];
  __shared__ SlotRec rec_[TW][8];
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t iter = 0;
  transport_body_uni<WG_MODE_SEAL>(S, blockIdx.x, wv, img_[wv], rec_[wv], iter);
  asm volatile("s_waitcnt vmcnt(0)\n\tbuffer_inv sc0" ::: "memory");  // as k_step
  transport_body_uni<WG_MODE_OPEN>(O, blockIdx.x, wv, img_[wv], rec_[wv], iter);
}

// ---- longest-first order for mixed-length batches (LPT) ----------------------------------
// key = rounds of the packet (invalid lengths sort last); counting sort into descending keys.
template <int MODE>
__device__ __forceinline__ uint32_t lpt_key(const wg_pkt* d, uint32_t i, uint32_t max_len) {
  const uint32_t len = d[i].len;
  if (len > max_len) return 0u;
  const uint32_t nb = ((len + 63u) >> 6) + 1u;
  return (nb + 7u) >> 3;
}

// Two launches, no global atomics and no memset: k_lpt_hist writes one histogram per block
// over a contiguous range of the batch; k_lpt_scatter (same grid) gives each block its base
// per key from all blocks' histograms (keys above it in every block, this key in the blocks
// before it) and ranks its packets in LDS.
constexpr uint32_t LPT_THREADS = 1024, LPT_MAX_BLOCKS = 64;

__device__ __forceinline__ void lpt_range(uint32_t n, uint32_t& lo, uint32_t& hi) {
  const uint32_t per = (n + gridDim.x - 1) / gridDim.x;
  lo = min(n, blockIdx.x * per);
  hi = min(n, lo + per);
}

template <int MODE>
__global__ void __launch_bounds__(LPT_THREADS) k_lpt_hist(const wg_pkt* d, uint32_t n, uint32_t max_len,
                                                          uint32_t* bh) {
  __shared__ uint32_t h[LPT_BINS];
  for (uint32_t k = threadIdx.x; k < LPT_BINS; k += LPT_THREADS) h[k] = 0;
  __syncthreads();
  uint32_t lo, hi;
  lpt_range(n, lo, hi);
  for (uint32_t i = lo + threadIdx.x; i < hi; i += LPT_THREADS) atomicAdd(&h[lpt_key<MODE>(d, i, max_len)], 1u);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < LPT_BINS; k += LPT_THREADS) bh[blockIdx.x * LPT_BINS + k] = h[k];
}

// order[pos] = packet, keys descending
template <int MODE>
__global__ void __launch_bounds__(LPT_THREADS) k_lpt_scatter(const wg_pkt* d, uint32_t n, uint32_t max_len,
                                                             const uint32_t* bh, uint32_t* order, uint32_t split,
                                                             uint32_t* n_long) {
  __shared__ uint32_t all[LPT_MAX_BLOCKS * LPT_BINS];  // every block's histogram (coalesced load)
  __shared__ uint32_t tot[LPT_BINS], base[LPT_BINS];
  for (uint32_t e = threadIdx.x; e < gridDim.x * LPT_BINS; e += LPT_THREADS) all[e] = bh[e];
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < LPT_BINS; k += LPT_THREADS) {
    uint32_t t = 0, before = 0;
    for (uint32_t b = 0; b < gridDim.x; ++b) {
      const uint32_t v = all[b * LPT_BINS + k];
      t += v;
      before += b < blockIdx.x ? v : 0u;
    }
    tot[k] = t;
    base[k] = before;
  }
  __syncthreads();
  if (threadIdx.x < 64u) {  // packets with a larger key come first: wave 0 scans the keys
    // in descending order, lane l holding positions 3l..3l+2 (key LPT_BINS-1-p)
    static_assert(3u * 64u >= LPT_BINS, "three keys per lane");
    const uint32_t l = threadIdx.x;
    uint32_t v[3], own = 0;
#pragma unroll
    for (uint32_t q = 0; q < 3u; ++q) {
      const uint32_t p = 3u * l + q;
      v[q] = p < LPT_BINS ? tot[LPT_BINS - 1u - p] : 0u;
      own += v[q];
    }
    uint32_t inc = own;
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
      const uint32_t up = __shfl_up(inc, off, 64);
      inc += l >= off ? up : 0u;
    }
    uint32_t acc = inc - own;
#pragma unroll
    for (uint32_t q = 0; q < 3u; ++q) {
      const uint32_t p = 3u * l + q;
      if (p < LPT_BINS) tot[LPT_BINS - 1u - p] = acc;
      acc += v[q];
    }
    // the packets with more than `split` rounds (keys > split) come first: their count is the
    // exclusive prefix at key `split`
    if (n_long && blockIdx.x == 0 && split + 1u < LPT_BINS) {
      const uint32_t p = LPT_BINS - 1u - split;  // position of key `split` in the descending scan
      if (l == p / 3u) {
        uint32_t a = inc - own;
        for (uint32_t q = 0; q < p % 3u; ++q) a += v[q];
        *n_long = a;
      }
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < LPT_BINS; k += LPT_THREADS) base[k] += tot[k];
  __syncthreads();
  uint32_t lo, hi;
  lpt_range(n, lo, hi);
  for (uint32_t i = lo + threadIdx.x; i < hi; i += LPT_THREADS) order[atomicAdd(&base[lpt_key<MODE>(d, i, max_len)], 1u)] = i;
}

// k_lpt_one's counter set per call: kFastBins counts kCntStride words apart, each set on 64-B lines of its own
// (the next set is zeroed while this one takes atomics); two sets used in turn
constexpr uint32_t kPlanSet = (kFastBins * kCntStride + 15u) / 16u * 16u;  // words per set

// One launch instead of k_lpt_hist + k_lpt_scatter, for batches whose keys fit kFastBins (max_len <= 2,048 B,
// the short-packet plan): each block counts its range's keys in LDS, takes its base in every non-empty key
// with ONE atomicAdd on that key's global counter, and ranks its packets into the key's region of a sparse
// order (key k at order[k * n]). No grid-wide barrier: the consumer derives the positions from the counts.
// The counters are double-buffered by call (cnt for this call, zero on entry; cnt_next zeroed here for the
// next), so no memset launch either. Order inside a key: arbitrary (every position of the order is a packet).
// A thread takes KPT packets per trip, their descriptor loads issued together, and when the block's range is
// one trip (the usual case) keeps the keys for the scatter pass: two load latencies per plan, not 2 x trips.
// (THREADS, KPT: the block shape)
template <int MODE, uint32_t THREADS = LPT_THREADS, int KPT = 1>
__global__ void __launch_bounds__(THREADS) k_lpt_one(const wg_pkt* d, uint32_t n, uint32_t max_len, uint32_t* cnt,
                                                     uint32_t* cnt_next, uint32_t* order) {
  constexpr uint32_t NB = kFastBins;
  __shared__ uint32_t h[NB], base[NB];
  if (threadIdx.x < NB) h[threadIdx.x] = 0;
  if (blockIdx.x == 0 && threadIdx.x < NB) cnt_next[threadIdx.x * kCntStride] = 0;  // the next call's counts
  __syncthreads();
  const uint32_t per = (n + gridDim.x - 1u) / gridDim.x;
  const uint32_t lo = min(n, blockIdx.x * per), hi = min(n, lo + per);
  const uint32_t lane = threadIdx.x & 63u, span = THREADS * KPT;
  // LDS atomics are aggregated per wave and key: one ballot per key, then ONE ds_add_rtn in which lane k adds
  // key k's lane count to slots[k] (six independent adds, not a chain of six round trips), one bpermute for
  // each lane's base in its key and mbcnt for its rank among the wave's lanes of that key
  auto wave_rank = [&](uint32_t* slots, uint32_t key) {  // this lane's rank among the wave's lanes of its key
    uint64_t mine = 0;
    uint32_t cnt_k = 0;
#pragma unroll
    for (uint32_t k = 0; k < NB; ++k) {
      const uint64_t m = __ballot(key == k);
      mine = key == k ? m : mine;
      cnt_k = lane == k ? (uint32_t)__popcll(m) : cnt_k;
    }
    uint32_t b = 0;
    if (cnt_k) b = atomicAdd(&slots[lane], cnt_k);  // lanes 0..NB-1 only (cnt_k = 0 elsewhere)
    b = __shfl(b, (int)(key < NB ? key : 0u), 64);
    return b + (uint32_t)__popcll(mine & ((1ull << lane) - 1ull));
  };
  auto keys_at = [&](uint32_t i0, uint32_t (&key)[KPT]) {  // every lane of a wave takes part in each trip
#pragma unroll
    for (int t = 0; t < KPT; ++t) {
      const uint32_t i = i0 + t * THREADS + threadIdx.x;
      key[t] = i < hi ? lpt_key<MODE>(d, i, max_len) : NB;
    }
  };
  uint32_t key[KPT];
  for (uint32_t i0 = lo; i0 < hi; i0 += span) {
    keys_at(i0, key);
#pragma unroll
    for (int t = 0; t < KPT; ++t) (void)wave_rank(h, key[t]);
  }
  __syncthreads();
  if (threadIdx.x < NB) {
    const uint32_t k = threadIdx.x, c = h[k];
    base[k] = k * n + (c ? atomicAdd(&cnt[k * kCntStride], c) : 0u);
  }
  __syncthreads();
  const bool one_trip = hi - lo <= span;
  for (uint32_t i0 = lo; i0 < hi; i0 += span) {
    if (!one_trip) keys_at(i0, key);
#pragma unroll
    for (int t = 0; t < KPT; ++t) {
      const uint32_t i = i0 + t * THREADS + threadIdx.x;
      const uint32_t at = wave_rank(base, key[t]);
      if (i < hi) order[at] = i;
    }
  }
}

// ---- wire framing (TransportPacket.java:18-35) --------------------------------------------
// 16-B transport header {u8 4, u8 0[3], u32 receiver_index, u64 counter}, little-endian,
// written with 4-B or 1-B stores by alignment.
__device__ inline void put_header(uint8_t* h, uint32_t rx, uint64_t ctr) {
  const uint32_t w[4] = {4u, rx, (uint32_t)ctr, (uint32_t)(ctr >> 32)};
  if ((((uintptr_t)h) & 3u) == 0) {
    uint32_t* h32 = (uint32_t*)h;
#pragma unroll
    for (int k = 0; k < 4; ++k) h32[k] = w[k];
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) h[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
  }
}

// One thread per packet: header of every packet the seal kernel accepted (the same
// validity test), at out_off - 16 (UnencryptedOutgoingTransport.java:14-18 writes the
// type and receiver index, EncryptedOutgoingTransport.java:11-14 the counter).
__global__ void __launch_bounds__(256) k_frame_seal(const wg_pkt* __restrict__ d, uint32_t n,
                                                    const uint32_t* __restrict__ rx, uint32_t max_len,
                                                    uint32_t key_slots, uint64_t in_size,
                                                    uint8_t* __restrict__ out, uint64_t out_size) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const wg_pkt p = d[i];
  if (p.out_off < 16 ||
      !transport_valid<WG_MODE_SEAL>(p.in_off, p.out_off, p.len, p.key_slot, max_len, key_slots, in_size, out_size))
    return;
  put_header(out + p.out_off - 16, rx[p.key_slot], p.counter);
}

// Open descriptors straight from received wire packets (UndecryptedIncomingTransport.java:20-33):
// ciphertext at +16, plaintext right after the packet in the same buffer (:30).
__global__ void __launch_bounds__(256) k_parse_open(const uint8_t* __restrict__ wire, uint64_t wire_size,
                                                    const uint64_t* __restrict__ off, const uint32_t* __restrict__ len,
                                                    const uint32_t* __restrict__ slot, uint32_t n,
                                                    wg_pkt* __restrict__ d, uint32_t* __restrict__ st) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint64_t o = off[i];
  const uint32_t wl = len[i];
  wg_pkt p;
  p.in_off = o + 16;
  p.out_off = o + wl;
  p.key_slot = slot[i];
  p.counter = 0;
  p.len = WG_LEN_INVALID;
  // packet [o, o+wl) plus its plaintext [o+wl, o+2wl-32) must lie inside the buffer
  bool ok = wl >= 32 && o <= wire_size && (uint64_t)wl <= wire_size - o && (uint64_t)wl - 32 <= wire_size - o - wl;
  if (ok) {
    const uint8_t* h = wire + o;
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = load_u32_any(h + 4 * k);
    ok = (w[0] & 0xffu) == 4u;  // only the type byte is checked (UndecryptedIncomingTransport.java:24-26)
    if (ok) {
      p.counter = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
      p.len = wl - 32;
    }
  }
  d[i] = p;
  if (st) st[i] = ok ? WG_PKT_OK : WG_PKT_BADHDR;
}

}  // namespace wgt
