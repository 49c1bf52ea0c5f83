// wg_hs.hip — batched BLAKE2s and the handshake admission check, on the device (included by wg_capi.hip).
//
// The reference runs mac1, WireGuard's first admission test, on every incoming initiation and response
// before any Noise work (IncomingInitiation.java:24-40, IncomingResponse.java:20-36): the keyed hash
// BLAKE2s-128(key = BLAKE2s-256("mac1----" || static public key), message without its two MACs)
// (InitiationPacket.calculateMac1, InitiationPacket.java:110-120; ResponsePacket.java:107-117) must equal
// the message's mac1 field, and mac2 must be all zero (IncomingInitiation.java:38-40: no cookies).
// wg_rx_plan lists the type-1 / type-2 datagrams of a UDP ring; wg_hs_check runs that test over the list
// where the ring lies and hands the host the accepted messages as compact records, so the host never
// fetches the ring and never hashes a message that was not meant for this device.
//
// BLAKE2s (RFC 7693), sequential mode, fanout 1, depth 1: parameter word outlen | keylen << 8 |
// 0x01010000 (Blake2s.java:94); a key is the first block, zero-padded (Blake2s.java:95-98). One message
// per lane: h[8], m[16] and v[16] in registers, the ten rounds unrolled with the message schedule as
// compile-time constants, so nothing is indexed dynamically and the kernels use no scratch. The right
// rotations by 16 and 8 are one v_perm_b32 each, those by 12 and 7 one v_alignbit_b32 each (the ChaCha20
// rotates of wg_device.h, turned the other way). Lanes of a wave hash messages of different lengths: the
// wave walks as many blocks as its longest message has.
//
// Message bytes are fetched as whole aligned 32-bit words (those that hold at least one byte of the
// range, never another) and shifted into place, so a message at any alignment costs 17 loads per block
// instead of 64; the bytes behind the range are masked to zero.
//
// Ranks. records[0 .. n_valid) is the stable compaction of the accepted messages; it takes the three
// launches of wg_plan.hip's rank_launch (check, scan, emit), with k_rx_scan called as it is: the check
// launch leaves one 16-B record {valid, initiations, responses, rejected} per range of 256 list
// positions, the scan turns them into exclusive prefixes and writes their totals as the summary, the
// emit launch places. The list's length is read on the device (it is the plan's n_host, written earlier
// on the same stream): the grid is sized from n, and a workgroup past the list writes a zero record and
// exits. Every scratch word is written by the first launch of a call before a later one reads it and
// nothing about a call lives on the host, so a captured plan + check replays. The mac1 key sits at a
// fixed device address (wg_plan.hip, fixed headers): wg_hs_key_set between replays needs no re-capture.
#pragma once

namespace {

struct HsPeerHdr {  // at a fixed device address; wg_hs_peers_set rewrites it (and may move what it names): wg_hs_open.hip
  const uint32_t* slots;   // capacity x (peer + 1), 0: empty
  const uint8_t* publics;  // 32 B per peer: the static public keys, in the caller's order
  const uint8_t* secrets;  // 32 B per peer: X25519(static private key, that peer's public key)
  uint32_t mask;           // capacity - 1; bucket = hs_peer_bucket(first two words of the key) & mask
  uint32_t count;
};

__host__ __device__ inline uint32_t hs_peer_bucket(uint32_t w0, uint32_t w1) { return mix32(w0 ^ mix32(w1)); }

struct HsPskHdr {  // at a fixed device address; wg_hs_peers_set and wg_hs_psks_set rewrite it: wg_hs_initiate.hip
  const uint8_t* psks;  // 32 B per peer: the preshared keys, in the peer table's order
  uint32_t count, _pad;
};

struct HsStamp {  // a peer's greatest accepted timestamp: its 12 bytes as one big-endian number (wg_hs_stamp.hip)
  unsigned long long hi;  // bytes [0, 8)
  uint32_t lo, _pad;      // bytes [8, 12)
};
struct HsStampSel {  // the selection's scratch words of a peer: the greatest candidate of the call, and its lowest entry
  unsigned long long hi;
  uint32_t lo, j;
};
struct HsStampHdr {  // at a fixed device address; wg_hs_peers_set rewrites it (and may move what it names)
  HsStamp* stored;
  HsStampSel* sel;
  uint32_t count, _pad;
};

struct HsCookie {  // a peer's cookie, learned from its reply (wg_hs_cookie.hip)
  uint32_t cookie[4];
  uint32_t have;  // 1: mac2 is written from it
  uint32_t sel;   // wg_hs_cookie_open's selection: the lowest batch index that opened a reply of this peer; ~0 between calls
  uint32_t _pad[2];
};
struct HsCookieHdr {  // at a fixed device address; wg_hs_peers_set rewrites it (and may move what it names)
  HsCookie* entries;
  uint32_t count, _pad;
};

constexpr size_t kHsKeyBytes = 160;

struct HsState {
  // [0, 32) the mac1 key, [32, 64) H(H0 || static public key), [64, 96) the static public key (wg_hs_static_set),
  // [96, 128) the cookie key H("cookie--" || static public key), [128, 160) the cookie secret (wg_hs_cookie.hip)
  // (fixed address)
  DevBuf d_key;
  DevBuf d_priv;   // the static private key, 32 B (fixed address; wg_hs_static_set, wg_x25519.hip)
  DevBuf d_stage;  // wg_hs_key_set: descriptor, "mac1----" || public key, status; wg_hs_static_set: [128, 196), [256, 356)
  DevBuf d_part;   // per range of 256 list positions: {valid, init, resp, rejected}, then their exclusive prefixes
  // wg_hs_open.hip: the peer table's header (fixed address), the table of a context without peers, the current
  // table, the publics behind 32 B that hold the private key while the secrets are computed, the secrets, the
  // k_x25519 descriptors and statuses that compute them; per record the open's results, per range its counts
  DevBuf d_phdr, d_pempty, d_pslots, d_pin, d_psec, d_pdesc, d_ores, d_opart;
  // wg_hs_respond.hip: per entry the three ladders' results (96 B) and the session (176 B), per range its counts
  DevBuf d_rlad, d_rres, d_rpart;
  // wg_hs_initiate.hip: the psks' header (fixed address) and the psks; per entry or record the two ladders' results
  // (64 B), per range its counts; wg_hs_finish's established entries (96 B per record) and its table of pending
  // positions
  DevBuf d_pskhdr, d_ppsk, d_ilad, d_ipart, d_fres, d_ftab;
  // wg_hs_stamp.hip, allocated at the first wg_hs_stamp* call (has_stamps): the stamps' header (fixed address), per
  // peer the stored timestamp and the selection's words, per entry {T, state} (16 B), per range its counts
  DevBuf d_shdr, d_stamps, d_ssel, d_sres, d_spart;
  bool has_stamps = false;
  // wg_hs_cookie.hip: the cookie table's header (fixed address) and the table of wg_hs_peers_set's peers
  DevBuf d_chdr, d_cook;
  bool has_secret = false;
  // wg_hs_ratelimit.hip, allocated by wg_hs_rl_reserve (rl_cap != 0): the limiter's header (fixed address), the
  // table's two buffers (rl_cap + 1 entries each), per bucket the call's count and selection row; per record the
  // call's {bucket, code, key} (16 B), per range its counts
  DevBuf d_rlhdr, d_rlent[2], d_rlcnt, d_rlrows, d_rlrec, d_rlpart;
  uint32_t rl_cap = 0;    // the table's capacity C (the compaction's grid)
  uint32_t rl_burst = 0;  // wg_hs_rl_config_set's burst (0: no config yet): the selection launches of a call
  uint32_t reserved = 0;  // the greatest wg_hs_reserve so far: what the stamp's scratch starts with
  uint32_t n_peers = 0;
  bool has_key = false;
  bool has_priv = false;
  StreamOrder order;  // last check / open / respond: they share the scratch
};

const PlanWords kHsCheckWords{"handshake check", "datagrams", "wg_hs_reserve"};
const PlanWords kHsOpenWords{"handshake open", "records", "wg_hs_reserve"};
const PlanWords kHsRespWords{"handshake respond", "entries", "wg_hs_reserve"};
const PlanWords kHsInitWords{"handshake initiate", "entries", "wg_hs_reserve"};
const PlanWords kHsFinWords{"handshake finish", "records", "wg_hs_reserve"};
const PlanWords kHsStampWords{"handshake stamp", "entries", "wg_hs_reserve"};

// The handshake state, allocated at the first wg_hs_* call. Caller holds c->mu.
int hs_get(wg_ctx* c, HsState** out) {
  if (!c->hs) {
    auto t = std::make_unique<HsState>();
    int rc;
    if ((rc = t->d_key.ensure(kHsKeyBytes)) != WG_OK || (rc = t->d_priv.ensure(32)) != WG_OK ||
        (rc = t->d_stage.ensure(512)) != WG_OK || (rc = t->d_phdr.ensure(sizeof(HsPeerHdr))) != WG_OK ||
        (rc = t->d_pempty.ensure(16 * sizeof(uint32_t))) != WG_OK || (rc = t->d_pskhdr.ensure(sizeof(HsPskHdr))) != WG_OK ||
        (rc = t->d_chdr.ensure(sizeof(HsCookieHdr))) != WG_OK)
      return rc;
    HsPeerHdr H{};  // no peers
    H.slots = (const uint32_t*)t->d_pempty.p;
    H.mask = 15u;
    HsPskHdr K{};  // ... and no psks
    K.psks = (const uint8_t*)t->d_pempty.p;
    HsCookieHdr C{};  // ... and no cookies
    C.entries = (HsCookie*)t->d_pempty.p;
    hipError_t e = t->order.create();
    if (e == hipSuccess) e = hipMemsetAsync(t->d_key.p, 0, kHsKeyBytes, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(t->d_pskhdr.p, &K, sizeof K, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(t->d_chdr.p, &C, sizeof C, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->d_priv.p, 0, 32, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->d_pempty.p, 0, 16 * sizeof(uint32_t), c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(t->d_phdr.p, &H, sizeof H, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(WG_EDEVICE, "handshake state: %s", hipGetErrorString(e));
    c->hs = t.release();
  }
  *out = c->hs;
  return WG_OK;
}

void hs_free(wg_ctx* c) {
  if (!c->hs) return;
  HsState* t = c->hs;
  if (t->d_key.p) {  // the keys are wiped, like the key table
    (void)hipDeviceSynchronize();
    (void)hipMemsetAsync(t->d_key.p, 0, kHsKeyBytes, c->stream);  // the cookie key and secret among them
    if (t->d_priv.p) (void)hipMemsetAsync(t->d_priv.p, 0, 32, c->stream);
    // the peers' static-static secrets, what the last open derived from them, and the last respond's scratch; the
    // psks and the last initiate's and finish's scratch
    // (the stamp's scratch holds timestamps and states, never k or ck, which stay in registers: wiped all the same);
    // the peers' cookies
    for (DevBuf* b : {&t->d_psec, &t->d_pin, &t->d_ores, &t->d_rlad, &t->d_rres, &t->d_ppsk, &t->d_ilad, &t->d_fres, &t->d_sres, &t->d_cook})
      if (b->p) (void)hipMemsetAsync(b->p, 0, b->cap, c->stream);
    (void)hipStreamSynchronize(c->stream);
  }
  delete t;
  c->hs = nullptr;
}

// open: the scratch of wg_hs_open too (per record 112 B of results, per range its counts). d_part holds two rows
// of counts: wg_hs_admit ranks records and replies
bool hs_scratch_fits(const HsState* t, uint32_t n, bool open) {
  const size_t part = (size_t)std::max(rank_blocks(n), 1u) * 16;
  return 2 * part <= t->d_part.cap && (!open || (part <= t->d_opart.cap && (size_t)std::max(n, 1u) * 112 <= t->d_ores.cap));
}
// ... and its growth (plan_reserve), for checks (and opens) of up to n messages
int hs_scratch_grow(HsState* t, uint32_t n, bool open) {
  const size_t part = (size_t)std::max(rank_blocks(n), 1u) * 16;
  int rc;
  if ((rc = t->d_part.ensure(2 * part)) != WG_OK || !open) return rc;
  if (t->d_ores.p && t->d_ores.cap < (size_t)std::max(n, 1u) * 112) HIPTRY(hipMemset(t->d_ores.p, 0, t->d_ores.cap));  // freed: wiped first
  if ((rc = t->d_opart.ensure(part)) != WG_OK) return rc;
  return t->d_ores.ensure((size_t)std::max(n, 1u) * 112);
}

// the scratch of wg_hs_respond for n entries (96 + 176 B per entry, per range its counts), and its growth
bool hs_resp_fits(const HsState* t, uint32_t n) {
  const size_t m = std::max(n, 1u);
  return (size_t)std::max(rank_blocks(n), 1u) * 16 <= t->d_rpart.cap && m * 96 <= t->d_rlad.cap && m * 176 <= t->d_rres.cap;
}
int hs_resp_grow(HsState* t, uint32_t n) {
  const size_t m = std::max(n, 1u);
  int rc;
  for (DevBuf* b : {&t->d_rlad, &t->d_rres})  // freed when they grow: wiped first
    if (b->p) HIPTRY(hipMemset(b->p, 0, b->cap));
  if ((rc = t->d_rpart.ensure((size_t)std::max(rank_blocks(n), 1u) * 16)) != WG_OK || (rc = t->d_rlad.ensure(m * 96)) != WG_OK) return rc;
  return t->d_rres.ensure(m * 176);
}

// the scratch of wg_hs_initiate for n entries and of wg_hs_finish for n records against n_pending entries (64 + 96 B
// per item, per range its counts, the table of pending positions), and its growth
uint32_t hs_fin_capacity(uint32_t n_pending) {
  uint32_t cap = 16;
  while ((uint64_t)cap < 4ull * n_pending) cap <<= 1;
  return cap;
}
bool hs_init_fits(const HsState* t, uint32_t n, uint32_t n_pending) {
  const size_t m = std::max(n, 1u);
  return (size_t)std::max(rank_blocks(n), 1u) * 16 <= t->d_ipart.cap && m * 64 <= t->d_ilad.cap && m * 96 <= t->d_fres.cap &&
         (size_t)hs_fin_capacity(n_pending) * 4 <= t->d_ftab.cap;
}
int hs_init_grow(HsState* t, uint32_t n, uint32_t n_pending) {
  const size_t m = std::max(n, 1u);
  int rc;
  for (DevBuf* b : {&t->d_ilad, &t->d_fres})  // freed when they grow: wiped first
    if (b->p) HIPTRY(hipMemset(b->p, 0, b->cap));
  if ((rc = t->d_ipart.ensure((size_t)std::max(rank_blocks(n), 1u) * 16)) != WG_OK || (rc = t->d_ilad.ensure(m * 64)) != WG_OK ||
      (rc = t->d_fres.ensure(m * 96)) != WG_OK)
    return rc;
  return t->d_ftab.ensure((size_t)hs_fin_capacity(n_pending) * 4);
}

// the scratch of wg_hs_stamp for n entries (16 B per entry, per range its counts), and its growth; a context that
// has never stamped has none
bool hs_stamp_fits(const HsState* t, uint32_t n) {
  return !t->has_stamps || ((size_t)std::max(rank_blocks(n), 1u) * 16 <= t->d_spart.cap && (size_t)std::max(n, 1u) * 16 <= t->d_sres.cap);
}
int hs_stamp_grow(HsState* t, uint32_t n) {
  if (!t->has_stamps) return WG_OK;
  int rc;
  if ((rc = t->d_spart.ensure((size_t)std::max(rank_blocks(n), 1u) * 16)) != WG_OK) return rc;
  return t->d_sres.ensure((size_t)std::max(n, 1u) * 16);
}

// the scratch of wg_hs_ratelimit for n records (16 B per record, per range its counts), and its growth; a context
// without a limiter has none
bool hs_rl_fits(const HsState* t, uint32_t n) {
  return !t->rl_cap || ((size_t)std::max(rank_blocks(n), 1u) * 16 <= t->d_rlpart.cap && (size_t)std::max(n, 1u) * 16 <= t->d_rlrec.cap);
}
int hs_rl_grow(HsState* t, uint32_t n) {
  if (!t->rl_cap) return WG_OK;
  int rc;
  if ((rc = t->d_rlpart.ensure((size_t)std::max(rank_blocks(n), 1u) * 16)) != WG_OK) return rc;
  return t->d_rlrec.ensure((size_t)std::max(n, 1u) * 16);
}

int hs_begin(HsState* t, hipStream_t s, bool capturing, uint32_t n, bool open, const PlanWords& w) {
  return plan_begin(t->order, s, capturing, hs_scratch_fits(t, n, open), [&] { return hs_scratch_grow(t, n, open); }, w, n);
}

int hs_open_rekey(wg_ctx* c, HsState* t, const uint8_t* static_public);  // wg_hs_open.hip
int hs_stamp_peers_reset(wg_ctx* c, HsState* t);                          // wg_hs_stamp.hip
int hs_cookie_peers_reset(wg_ctx* c, HsState* t);                         // wg_hs_cookie.hip

// The buffers of a call (wg_hs_open, wg_hs_respond): an empty range overlaps nothing.
struct HsRange {
  const void* p;
  uint64_t bytes;
};
bool hs_overlap(const HsRange& a, const HsRange& b) {
  const uintptr_t x = (uintptr_t)a.p, y = (uintptr_t)b.p;
  return a.bytes && b.bytes && x < y + b.bytes && y < x + a.bytes;
}
// 0: the outputs are disjoint from one another and from the inputs; 1: the first overlap found, walking the
// outputs in order, is with a later output; 2: it is with an input
template <int NO, int NI>
int hs_ranges_overlap(const HsRange (&out)[NO], const HsRange (&in)[NI]) {
  for (int i = 0; i < NO; ++i) {
    for (int j = i + 1; j < NO; ++j)
      if (hs_overlap(out[i], out[j])) return 1;
    for (int j = 0; j < NI; ++j)
      if (hs_overlap(out[i], in[j])) return 2;
  }
  return 0;
}

}  // namespace

// ---- device -------------------------------------------------------------------------------
namespace wghs {

struct B2sParams {
  const wg_b2s_desc* desc;
  const uint8_t* in;
  uint64_t in_size;
  uint8_t* out;
  uint64_t out_size;
  uint32_t* status;
  uint32_t n;
};

struct HsParams {
  const uint8_t* wire;
  uint64_t wire_size;
  const uint64_t* pkt_off;
  const uint32_t* pkt_len;
  const uint32_t* list;
  const uint32_t* n_list;
  uint32_t* hs_status;
  wg_hs_record* records;
  const uint8_t* key;
  uint4* part;
  uint32_t n;
};

__device__ __forceinline__ uint32_t rotr16(uint32_t x) { return wgd::rotl16(x); }
__device__ __forceinline__ uint32_t rotr12(uint32_t x) { return wgd::rotl(x, 20); }
__device__ __forceinline__ uint32_t rotr8(uint32_t x) { return __builtin_amdgcn_perm(x, x, 0x00030201u); }
__device__ __forceinline__ uint32_t rotr7(uint32_t x) { return wgd::rotl(x, 25); }

#define WG_B2S_G(a, b, c, d, x, y)               \
  v[a] += v[b] + (x); v[d] = rotr16(v[d] ^ v[a]); \
  v[c] += v[d];       v[b] = rotr12(v[b] ^ v[c]); \
  v[a] += v[b] + (y); v[d] = rotr8(v[d] ^ v[a]);  \
  v[c] += v[d];       v[b] = rotr7(v[b] ^ v[c]);
// one round: four columns, four diagonals; s0..s15 = the round's row of the sigma permutation
#define WG_B2S_ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15) \
  WG_B2S_G(0, 4, 8, 12, m[s0], m[s1])                                                      \
  WG_B2S_G(1, 5, 9, 13, m[s2], m[s3])                                                      \
  WG_B2S_G(2, 6, 10, 14, m[s4], m[s5])                                                     \
  WG_B2S_G(3, 7, 11, 15, m[s6], m[s7])                                                     \
  WG_B2S_G(0, 5, 10, 15, m[s8], m[s9])                                                     \
  WG_B2S_G(1, 6, 11, 12, m[s10], m[s11])                                                   \
  WG_B2S_G(2, 7, 8, 13, m[s12], m[s13])                                                    \
  WG_B2S_G(3, 4, 9, 14, m[s14], m[s15])

// RFC 7693 3.2: h = F(h, m, t, last)
__device__ __forceinline__ void b2s_compress(uint32_t h[8], const uint32_t m[16], uint64_t t, bool last) {
  uint32_t v[16];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = h[k];
  v[8] = 0x6A09E667u;
  v[9] = 0xBB67AE85u;
  v[10] = 0x3C6EF372u;
  v[11] = 0xA54FF53Au;
  v[12] = 0x510E527Fu ^ (uint32_t)t;
  v[13] = 0x9B05688Cu ^ (uint32_t)(t >> 32);
  v[14] = 0x1F83D9ABu ^ (last ? 0xFFFFFFFFu : 0u);
  v[15] = 0x5BE0CD19u;
  WG_B2S_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
  WG_B2S_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3)
  WG_B2S_ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4)
  WG_B2S_ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8)
  WG_B2S_ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13)
  WG_B2S_ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9)
  WG_B2S_ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11)
  WG_B2S_ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10)
  WG_B2S_ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5)
  WG_B2S_ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0)
#pragma unroll
  for (int k = 0; k < 8; ++k) h[k] ^= v[k] ^ v[k + 8];
}

// m = the `avail` (0..64) bytes at p as little-endian words, zero behind them. Reads the aligned words
// that hold at least one of those bytes: an index past the last such word is clamped to it, so no load
// is conditional and none leaves the range's own words.
__device__ __forceinline__ void b2s_load(const uint8_t* p, uint32_t avail, uint32_t m[16]) {
  if (avail == 0) {
#pragma unroll
    for (int k = 0; k < 16; ++k) m[k] = 0u;
    return;
  }
  const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
  const uint32_t* base = (const uint32_t*)(p - mis);
  const uint32_t jlast = (mis + avail - 1u) >> 2;  // <= 16
  uint32_t w[17];
#pragma unroll
  for (uint32_t j = 0; j < 17; ++j) w[j] = base[j < jlast ? j : jlast];
  const uint32_t sh = 8u * mis;
#pragma unroll
  for (uint32_t k = 0; k < 16; ++k) {
    const uint32_t x = __builtin_amdgcn_alignbit(w[k + 1], w[k], sh);
    const uint32_t vb = avail > 4u * k ? avail - 4u * k : 0u;
    m[k] = x & (vb >= 4u ? 0xFFFFFFFFu : (1u << (8u * vb)) - 1u);
  }
}

// h = the initial state for a digest of outlen bytes under a key of keylen bytes (RFC 7693 2.5, 3.3)
__device__ __forceinline__ void b2s_init(uint32_t h[8], uint32_t outlen, uint32_t keylen) {
  h[0] = 0x6A09E667u ^ (outlen | (keylen << 8) | 0x01010000u);
  h[1] = 0xBB67AE85u;
  h[2] = 0x3C6EF372u;
  h[3] = 0xA54FF53Au;
  h[4] = 0x510E527Fu;
  h[5] = 0x9B05688Cu;
  h[6] = 0x1F83D9ABu;
  h[7] = 0x5BE0CD19u;
}

// h = the BLAKE2s state after msg[0 .. len) under key[0 .. keylen) for a digest of outlen bytes: the
// digest is the first outlen bytes of h, little-endian.
__device__ __forceinline__ void b2s_hash(const uint8_t* msg, uint32_t len, const uint8_t* key, uint32_t keylen,
                                         uint32_t outlen, uint32_t h[8]) {
  b2s_init(h, outlen, keylen);
  const uint32_t kb = keylen ? 1u : 0u;  // the key block; it is the last block of a keyed empty message
  const uint32_t mb = len ? (len >> 6) + ((len & 63u) ? 1u : 0u) : 1u - kb;
  const uint32_t nb = kb + mb;
  uint64_t t = 0;
  for (uint32_t b = 0; b < nb; ++b) {
    const bool isk = b < kb;
    const uint64_t off = 64ull * (b - kb);
    const uint32_t left = len - (uint32_t)off;
    const uint8_t* p = isk ? key : msg + off;
    const uint32_t avail = isk ? keylen : (left < 64u ? left : 64u);
    t += isk ? 64u : avail;
    uint32_t m[16];
    b2s_load(p, avail, m);
    b2s_compress(h, m, t, b + 1u == nb);
  }
}

__global__ void __launch_bounds__(256) k_b2s(B2sParams P) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P.n) return;
  const uint4* d = (const uint4*)(P.desc + i);
  const uint4 a = d[0], b = d[1];
  const uint64_t in_off = wgrp::u64_of(a.x, a.y), out_off = wgrp::u64_of(a.z, a.w), key_off = wgrp::u64_of(b.x, b.y);
  const uint32_t len = b.z, outlen = b.w & 0xFFu, keylen = (b.w >> 8) & 0xFFu;
  // (off <= size && len <= size - off: no sum that could wrap)
  const bool ok = outlen >= 1u && outlen <= 32u && keylen <= 32u && in_off <= P.in_size &&
                  (uint64_t)len <= P.in_size - in_off && key_off <= P.in_size &&
                  (uint64_t)keylen <= P.in_size - key_off && out_off <= P.out_size &&
                  (uint64_t)outlen <= P.out_size - out_off;
  if (!ok) {
    P.status[i] = WG_B2S_BADDESC;
    return;
  }
  uint32_t h[8];
  b2s_hash(P.in + in_off, len, P.in + key_off, keylen, outlen, h);
  uint8_t* o = P.out + out_off;
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k) {
    if (4u * k + 4u <= outlen) {
      wgt::store_u32_any(o + 4u * k, h[k]);
    } else {  // the digest's last word, partly written (or not at all)
#pragma unroll
      for (uint32_t j = 0; j < 3; ++j)
        if (4u * k + j < outlen) o[4u * k + j] = (uint8_t)(h[k] >> (8u * j));
    }
  }
  P.status[i] = WG_B2S_OK;
}

// list position k -> batch index, and how long the list is (read on the device)
__device__ __forceinline__ uint32_t hs_list_len(const HsParams& P) {
  if (!P.list) return P.n;
  const uint32_t nl = *P.n_list;
  return nl < P.n ? nl : P.n;
}

// steps 1-6 of wg_hs_check for one list position per thread; the range's counts
__global__ void __launch_bounds__(256) k_hs_check(HsParams P) {
  __shared__ uint32_t s_cnt[4][4];
  const uint32_t nl = hs_list_len(P);
  if (blockIdx.x * kRankRange >= nl) {  // past the list (workgroup-uniform): a zero record for the scan
    if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const uint32_t k = blockIdx.x * kRankRange + threadIdx.x;
  const bool in = k < nl;
  uint32_t st = WG_HS_BADLEN, t = 0;
  if (in) {
    const uint32_t i = P.list ? P.list[k] : k;
    bool go = false;
    const uint8_t* msg = P.wire;
    uint32_t L = 0;
    if (i < P.n) {
      const uint64_t o = P.pkt_off[i];
      const uint32_t wl = P.pkt_len[i];
      if (wl != 0 && o <= P.wire_size && (uint64_t)wl <= P.wire_size - o) {
        msg = P.wire + o;
        t = msg[0];
        if (t != 1u && t != 2u) {
          st = WG_HS_BADTYPE;
        } else {
          L = t == 1u ? 148u : 92u;
          go = wl == L;
        }
      }
    }
    if (go) {
      uint32_t h[8];
      b2s_hash(msg, L - 32u, P.key, 32u, 16u, h);
      uint32_t diff = 0, mac2 = 0;  // all 16 bytes of each, no early exit
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        diff |= wgt::load_u32_any(msg + L - 32u + 4u * j) ^ h[j];
        mac2 |= wgt::load_u32_any(msg + L - 16u + 4u * j);
      }
      st = diff ? WG_HS_BADMAC1 : mac2 ? WG_HS_BADMAC2 : WG_HS_OK;
    }
    P.hs_status[k] = st;
  }
  const bool ok = in && st == WG_HS_OK;
  uint32_t r, n_valid, n_init, n_resp, n_rej;
  wgrp::block_rank(ok, s_cnt[0], r, n_valid);
  wgrp::block_rank(ok && t == 1u, s_cnt[1], r, n_init);
  wgrp::block_rank(ok && t == 2u, s_cnt[2], r, n_resp);
  wgrp::block_rank(in && !ok, s_cnt[3], r, n_rej);
  if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4(n_valid, n_init, n_resp, n_rej);
}

// records[slot] = the accepted message of list position k
__device__ __forceinline__ void hs_put_record(const HsParams& P, uint32_t k, uint32_t slot) {
  const uint32_t i = P.list ? P.list[k] : k;
  const uint8_t* msg = P.wire + P.pkt_off[i];
  const uint32_t L = msg[0] == 1u ? 148u : 92u;
  uint4* rec = (uint4*)(P.records + slot);
#pragma unroll
  for (uint32_t g = 0; g < 10; ++g) {  // 160 B: index, len, 37 message words (zero behind a response), _pad
    uint32_t w[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t q = 4u * g + j;
      if (q == 0) w[j] = i;
      else if (q == 1) w[j] = L;
      else if (q == 39) w[j] = 0u;
      else w[j] = 4u * (q - 2u) < L ? wgt::load_u32_any(msg + 4u * (q - 2u)) : 0u;
    }
    rec[g] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// records[prefix of the range + rank in the range] = the accepted message of this list position
__global__ void __launch_bounds__(256) k_hs_emit(HsParams P) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t nl = hs_list_len(P);
  if (blockIdx.x * kRankRange >= nl) return;  // (workgroup-uniform)
  const uint32_t k = blockIdx.x * kRankRange + threadIdx.x;
  const bool ok = k < nl && P.hs_status[k] == WG_HS_OK;
  const uint4 pre = P.part[blockIdx.x];
  uint32_t r, total;
  wgrp::block_rank(ok, s_cnt, r, total);
  if (!ok) return;
  hs_put_record(P, k, pre.x + r);
}

}  // namespace wghs

// ---- C ABI --------------------------------------------------------------------------------
namespace {

int b2s_launch(const wg_b2s_desc* desc, uint32_t n, const uint8_t* in, uint64_t in_size, uint8_t* out, uint64_t out_size,
               uint32_t* status, hipStream_t s) {
  wghs::B2sParams P{};
  P.desc = desc;
  P.in = in;
  P.in_size = in_size;
  P.out = out;
  P.out_size = out_size;
  P.status = status;
  P.n = n;
  hipLaunchKernelGGL(wghs::k_b2s, dim3(rank_blocks(n)), dim3(256), 0, s, P);
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) return fail(WG_EDEVICE, "k_b2s launch: %s", hipGetErrorString(le));
  return WG_OK;
}

// the mac1 key of `static_public` into the fixed key buffer (wg_hs_key_set; wg_hs_static_set with the public key it
// derived). Caller holds c->mu.
int hs_mac1_key_set(wg_ctx* c, HsState* t, const uint8_t* static_public) {
  int rc;
  // stage: [32, 72) "mac1----" || public key (InitiationPacket.java:111-115), [96, 104) the two statuses;
  // [384, 448) the two descriptors of the one launch, [448, 488) "cookie--" || public key. The digests go to
  // [0, 32) and [96, 128) of the key buffer.
  uint8_t host[128] = {0}, host2[128] = {0};
  wg_b2s_desc d[2] = {};
  d[0].in_off = 32;
  d[1].in_off = 448;
  d[1].out_off = 96;
  d[0].len = d[1].len = 40;
  d[0].outlen = d[1].outlen = 32;
  memcpy(host + 32, "mac1----", 8);
  memcpy(host + 40, static_public, 32);
  memcpy(host2, d, sizeof d);
  memcpy(host2 + 64, "cookie--", 8);
  memcpy(host2 + 72, static_public, 32);
  HIPTRY(hipDeviceSynchronize());  // no check queued earlier (on any stream) may still read the old key
  uint8_t* st = (uint8_t*)t->d_stage.p;
  HIPTRY(hipMemcpyAsync(st, host, sizeof host, hipMemcpyHostToDevice, c->stream));
  HIPTRY(hipMemcpyAsync(st + 384, host2, sizeof host2, hipMemcpyHostToDevice, c->stream));
  if ((rc = b2s_launch((const wg_b2s_desc*)(st + 384), 2, st, 512, (uint8_t*)t->d_key.p, 128, (uint32_t*)(st + 96), c->stream)) != WG_OK)
    return rc;
  HIPTRY(hipStreamSynchronize(c->stream));
  t->has_key = true;
  return WG_OK;
}

}  // namespace

extern "C" {

int wg_blake2s_batch(wg_ctx* c, const wg_b2s_desc* desc, uint32_t n, const uint8_t* in, uint64_t in_size, uint8_t* out,
                     uint64_t out_size, uint32_t* status, void* stream) {
  if (!c) return fail(WG_EINVAL, "NULL context");
  if (n == 0) return WG_OK;
  if (!desc || (((uintptr_t)desc) & 15u)) return fail(WG_EINVAL, "descriptor array must be non-NULL and 16-byte aligned");
  if (!in || !out || !status || (((uintptr_t)status) & 3u))
    return fail(WG_EINVAL, "NULL input, output or status array (status: 4-byte aligned)");
  if (open_overlaps(in, in_size, out, out_size)) return fail(WG_EINVAL, "the output buffer must not overlap the input buffer");
  DeviceGuard g(c->device);
  return b2s_launch(desc, n, in, in_size, out, out_size, status, pick_stream(c, stream));
}

int wg_hs_key_set(wg_ctx* c, const uint8_t* static_public) {
  if (!c || !static_public) return fail(WG_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HsState* t;
  int rc;
  if ((rc = hs_get(c, &t)) != WG_OK) return rc;
  return hs_mac1_key_set(c, t, static_public);
}

int wg_hs_reserve(wg_ctx* c, uint32_t max_messages) {
  if (!c) return fail(WG_EINVAL, "NULL context");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HsState* t;
  int rc;
  if ((rc = hs_get(c, &t)) != WG_OK) return rc;
  const uint32_t pend = std::min(max_messages, 0x10000000u);  // (wg_hs_finish takes no more pending entries)
  t->reserved = std::max(t->reserved, max_messages);
  return plan_reserve(hs_scratch_fits(t, max_messages, true) && hs_resp_fits(t, max_messages) && hs_init_fits(t, max_messages, pend) &&
                          hs_stamp_fits(t, max_messages) && hs_rl_fits(t, max_messages),
                      [&] {
                        int grc = hs_scratch_grow(t, max_messages, true);
                        if (grc == WG_OK) grc = hs_resp_grow(t, max_messages);
                        if (grc == WG_OK) grc = hs_stamp_grow(t, max_messages);
                        if (grc == WG_OK) grc = hs_rl_grow(t, max_messages);
                        return grc != WG_OK ? grc : hs_init_grow(t, max_messages, pend);
                      });
}

int wg_hs_check(wg_ctx* c, const wg_hs_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  if (b->_reserved) return fail(WG_EINVAL, "wg_hs_batch._reserved must be 0");
  if (!b->summary || (((uintptr_t)b->summary) & 7u)) return fail(WG_EINVAL, "summary must be non-NULL and 8-byte aligned");
  if ((b->list == nullptr) != (b->n_list == nullptr))
    return fail(WG_EINVAL, "list and n_list go together: both NULL (every datagram) or both set");
  if ((((uintptr_t)b->list) & 3u) || (((uintptr_t)b->n_list) & 3u)) return fail(WG_EINVAL, "list and n_list must be 4-byte aligned");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (!c->hs || !c->hs->has_key) return fail(WG_ENOKEY, "wg_hs_check before any wg_hs_key_set");
  HsState* t = c->hs;
  const bool capturing = stream_capturing(s);
  const uint32_t n = b->n;
  if (n == 0) {
    HIPTRY(hipMemsetAsync(b->summary, 0, sizeof(wg_hs_summary), s));
    return WG_OK;
  }
  if (!b->wire || !b->pkt_off || !b->pkt_len) return fail(WG_EINVAL, "NULL wire ring or packet table");
  if (!b->hs_status || (((uintptr_t)b->hs_status) & 3u) || !b->records || (((uintptr_t)b->records) & 15u))
    return fail(WG_EINVAL, "status / record output must be non-NULL and aligned (4 / 16 bytes)");
  int rc;
  if ((rc = hs_begin(t, s, capturing, n, false, kHsCheckWords)) != WG_OK) return rc;
  wghs::HsParams P{};
  P.wire = b->wire;
  P.wire_size = b->wire_size;
  P.pkt_off = b->pkt_off;
  P.pkt_len = b->pkt_len;
  P.list = b->list;
  P.n_list = b->n_list;
  P.hs_status = b->hs_status;
  P.records = b->records;
  P.key = (const uint8_t*)t->d_key.p;
  P.part = (uint4*)t->d_part.p;
  P.n = n;
  rank_launch(wghs::k_hs_check, wghs::k_hs_emit, P, b->summary, s);
  return plan_end(t->order, s, capturing, kHsCheckWords);
}

}  // extern "C"
