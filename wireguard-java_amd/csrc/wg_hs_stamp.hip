// wg_hs_stamp.hip — the initiations' encrypted timestamp, opened on the device, and the replays refused
// (included by wg_capi.hip after wg_hs_install.hip): wg_hs_stamp, wg_hs_stamps_set, wg_hs_stamps_get.
//
// wg_hs_open authenticates an initiation and mixes the 28 bytes of encrypted_timestamp into the hash without
// opening them, as the reference does (Handshakes.java:233-234). A captured initiation of a known peer, sent
// again, therefore passes every test so far and costs three ladders, five HKDFs, two key slots and a receiver
// index each time. WireGuard's defence is the TAI64N timestamp under the static-static key: a responder answers
// an initiation only if its timestamp is greater than the greatest it has seen from that peer. The reference has
// no such step; like the replay window and cryptokey routing this is a protection the library adds. It sits
// between wg_hs_open and wg_hs_respond: wg_hs_open's entries in, the fresh ones out, in the same layout.
//
// The chain (H, KDFn, CK0, H0 as in wg_hs_open.hip; r = the entry's record, p = its peer, ss = wg_hs_dh's 32 bytes
// of record r, ss_p = the peer table's X25519(S_priv, S_p)):
//   h  = H(H(H(H0 || S_pub) || E) || encrypted_static)
//   ck = KDF1(KDF1(CK0, E), ss)
//   k  = KDF2(ck, ss_p)
//   T  = AEAD-open(k, nonce 0, aad = h, encrypted_timestamp)       (12 bytes)
// This is wg_hs_open's chain once more: the key is KDF2 of the ck BEFORE the static-static step and the aad the
// h before the last mix, and wg_hs_init carries only the final two, which nothing leads back from; its layout is
// wg_hs_respond's input and does not change. encrypted_static is hashed, not opened a second time: the entry
// exists because it was authentic.
//
// k_hs_stamp_chain: one entry per lane, the 28 steps of kStampProgram (wg_hs_chain.h) on the machine of
// wg_hs_chain.hip: ONE loop around ONE b2s_compress, for the reason wg_hs_open.hip gives. The kernel's own
// operations: H(H(H0 || S_pub) || E); the two blocks of H(h || encrypted_static) without the open (OP_SES1, and
// OP_ES2 as k_hs_open has it); the open of the timestamp in front of H(h || encrypted_timestamp) (OP_STS, the
// mirror of k_hs_init_chain's OP_ITS), its key being the T2 that the step before left in the state: two register
// chacha20_blocks and wghc::poly_tag_bytes<1> over aad (32) || ct (12, padded) || LE64(32) || LE64(12), the tag
// compared in all 16 bytes. The lane leaves {T, state} in scratch, and an authentic lane resets its peer's
// selection words (every such lane stores the same 16 bytes). A wave without an entry to open skips the chain.
//
// The rule is WireGuard's, stated so that no thread order enters: REPLAY is T <= the peer's value at the start
// of the call; of the remaining authentic entries of one peer only the greatest T is OK (the lowest position
// among equals), the others are SUPERSEDED. Walking the batch in order under "accept iff greater, then store"
// ends with the same stored value and the same last accepted entry. The selection is four small launches whose
// boundaries give the order, with no workgroup waiting on another:
//   k_hs_stamp_hi      T <= stored: REPLAY. Else a 64-bit atomicMax of T's high 8 bytes into the peer's word.
//   k_hs_stamp_lo      the entries that hold that maximum: a 32-bit atomicMax of the low 4 bytes.
//   k_hs_stamp_j       the entries that still tie: atomicMin of the position.
//   k_hs_stamp_commit  the entry whose position stands there is OK and stores T as the peer's; the others are
//                      SUPERSEDED. Statuses, opened timestamps, and the counts per 256 entries for the scan.
// In the three middle launches a wave issues one atomic per peer among its lanes, not one per lane (wave_by_peer):
// the lanes of a peer reduce their values by butterfly first, so a flood of one peer's initiations does not queue
// its every entry on one address.
// T is compared as one unsigned 96-bit big-endian number (memcmp order): the words are byte-swapped once, in
// the chain kernel's successors, and the stored value is kept as {64-bit, 32-bit} numbers.
//
// Ranks. fresh[0 .. n_ok) is the stable compaction of the OK entries: k_rx_scan as it is over the commit's
// counts, then k_hs_stamp_emit, which copies the entry's 144 bytes. Seven launches in all (chain, hi, lo, j,
// commit, scan, emit). Every scratch word is written before it is read in each call and nothing about a call
// lives on the host, so a captured plan -> check -> dh -> open -> stamp -> respond replays; a replay over the
// same ring finds every timestamp stale. The stored timestamps and the selection words sit behind a header at
// a fixed device address (wg_plan.hip, fixed headers): wg_hs_peers_set between replays needs no re-capture.
//
// Constant time: no branch, address or loop bound depends on ss, on ss_p, on ck or on k, which never leave the
// registers. The program is public and indexed by a public counter. The branches depend on the program, the
// entry's peer and record positions, the record's length, the tag comparison's outcome and the timestamp of
// an authentic message, all public; the static-static secret's ADDRESS depends on which peer it is, not on its
// value.
#pragma once

namespace wgts {

constexpr uint32_t kStampCand = 0x40000000u;  // res[j].w between launches: authentic and not yet decided

struct StampParams {
  const wg_hs_init* inits;
  const uint32_t* n_inits;
  const wg_hs_record* records;
  const uint8_t* shared;
  uint32_t* ts_status;
  uint8_t* opened;
  wg_hs_init* fresh;
  const uint8_t* hs0;  // H(H0 || S_pub), 32 B (fixed address)
  const HsPeerHdr* peers;
  const HsStampHdr* stamps;
  uint4* res;  // per entry {T as three words, state}
  uint4* part;
  uint32_t n, n_rec;
};

__device__ __forceinline__ uint32_t stamp_len(const StampParams& P) { return wgrp::dev_count(P.n_inits, P.n); }
__device__ __forceinline__ uint32_t stamp_peer(const StampParams& P, uint32_t j) { return ((const uint4*)(P.inits + j))[0].w; }
__device__ __forceinline__ uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }
// T as numbers: bytes [0, 8) and [8, 12), big-endian
__device__ __forceinline__ unsigned long long stamp_hi(const uint4 t) { return wgrp::u64_of(bswap32(t.y), bswap32(t.x)); }
__device__ __forceinline__ uint32_t stamp_lo(const uint4 t) { return bswap32(t.z); }

// T = ct ^ keystream when Poly1305(aad || ct || pad || lengths) under `key`, nonce 0, equals the tag; returns the
// OR of the tag's differences (0: authentic). ets = encrypted_timestamp as 7 words: 3 of ciphertext, 4 of tag.
__device__ __forceinline__ uint32_t open_timestamp(const uint32_t key[8], const uint32_t aad[8], const uint32_t ets[7], uint32_t ts[3]) {
  uint32_t ks[16], tag[4];
  const uint32_t ct[4] = {ets[0], ets[1], ets[2], 0u};
  wgd::chacha20_block(key, 0u, 0u, 0u, 0u, ks);
  wghc::poly_tag_bytes<1>(ks, aad, ct, 12u, tag);
  const uint32_t diff = (tag[0] ^ ets[3]) | (tag[1] ^ ets[4]) | (tag[2] ^ ets[5]) | (tag[3] ^ ets[6]);  // all 16 bytes
  wgd::chacha20_block(key, 1u, 0u, 0u, 0u, ks);
#pragma unroll
  for (int j = 0; j < 3; ++j) ts[j] = ets[j] ^ ks[j];
  return diff;
}

// One entry per lane: {T, state} to scratch; the peer's selection words of an authentic lane start again.
__global__ void __launch_bounds__(256) k_hs_stamp_chain(StampParams P) {
  const uint32_t nl = stamp_len(P);
  const uint32_t j = blockIdx.x * kRankRange + threadIdx.x;
  if ((j & ~63u) >= nl) return;  // (wave-uniform) a wave wholly past the entries
  const bool in = j < nl;
  const HsPeerHdr H = *P.peers;
  const HsStampHdr S = *P.stamps;
  uint32_t st_out = WG_HS_TS_BADDESC, p = 0u, r = 0u;
  bool go = false;
  if (in) {
    const uint4 e0 = ((const uint4*)(P.inits + j))[0];  // {index, record, sender_index, peer}
    r = e0.y;
    p = e0.w;
    if (p == WG_HS_NOPEER) st_out = WG_HS_TS_NOPEER;
    else if (p >= H.count || p >= S.count || r >= P.n_rec) st_out = WG_HS_TS_BADDESC;
    else if (((const uint4*)(P.records + r))[0].y != WG_HS_INIT_SIZE) st_out = WG_HS_TS_BADDESC;
    else go = true;
  }
  uint32_t ts[3] = {0u, 0u, 0u};
  bool auth = false;
  if (__ballot(go) != 0ull) {  // (wave-uniform) some lane has a timestamp to open
    // a lane that opens nothing runs the chain over zeros and stores nothing of it
    const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
    const uint4* rec = (const uint4*)(P.records + (go ? r : 0u));
    const uint4* shr = (const uint4*)(P.shared + 32ull * (go ? r : 0u));
    const uint4* sec = (const uint4*)(H.secrets + 32ull * (go ? p : 0u));
    using namespace wghc;
    Chain c;
    clear(c);
    set8(c.ist, wgho::kCk0Ipad);  // KDF1(CK0, E) starts from the constant key-block states
    set8(c.ost, wgho::kCk0Opad);
    Step s = fetch(kStampProgram, 0u);
#pragma unroll 1
    for (uint32_t step = 0; step < kStampSteps; ++step) {
      uint32_t src[8];
      switch (s.arg) {
        case SRC_E: put8(src, go ? rec[1] : z4, go ? rec[2] : z4); break;
        case SRC_SS: put8(src, go ? shr[0] : z4, go ? shr[1] : z4); break;
        case SRC_STATIC: put8(src, go ? sec[0] : z4, go ? sec[1] : z4); break;  // the peer's static-static secret
        default: source(c, s.arg, src); break;
      }
      switch (s.op) {
        case OP_H0: {  // h = H(H(H0 || S_pub) || E)
          const uint4* q = (const uint4*)P.hs0;
          put8(c.m, q[0], q[1]);
          put8(c.m + 8, go ? rec[1] : z4, go ? rec[2] : z4);
          wghs::b2s_init(c.st, 32u, 0u);
          c.t = 64u; c.last = true;
          break;
        }
        case OP_SES1:  // h = H(h || encrypted_static), first block
          set8(c.m, c.hh);
          put8(c.m + 8, go ? rec[3] : z4, go ? rec[4] : z4);
          wghs::b2s_init(c.st, 32u, 0u);
          c.t = 64u; c.last = false;
          break;
        case OP_ES2: {  // ... second block: the tag
          const uint4 tg = go ? rec[5] : z4;
          c.m[0] = tg.x; c.m[1] = tg.y; c.m[2] = tg.z; c.m[3] = tg.w;
#pragma unroll
          for (int k = 4; k < 16; ++k) c.m[k] = 0u;
          c.t = 80u; c.last = true;
          break;
        }
        case OP_STS: {  // st = T2 = the key: open the timestamp; then h = H(h || encrypted_timestamp), 60 bytes
          const uint4 a = go ? rec[6] : z4, b = go ? rec[7] : z4;
          const uint32_t ets[7] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z};
          const uint32_t diff = open_timestamp(c.st, c.hh, ets, ts);
          auth = go && diff == 0u;
          set8(c.m, c.hh);
#pragma unroll
          for (int k = 0; k < 7; ++k) c.m[8 + k] = ets[k];
          c.m[15] = 0u;
          wghs::b2s_init(c.st, 32u, 0u);
          c.t = 60u; c.last = true;
          break;
        }
        default: prepare(c, s, src); break;
      }
      const Step ahead = fetch(kStampProgram, step + 1u);
      wghs::b2s_compress(c.st, c.m, c.t, c.last);
      WG_HSC_PUT(c, s.dst);
      s = ahead;
    }
  }
  if (!in) return;
  if (go) st_out = auth ? kStampCand : WG_HS_TS_BADAUTH;
  P.res[j] = make_uint4(auth ? ts[0] : 0u, auth ? ts[1] : 0u, auth ? ts[2] : 0u, st_out);
  if (auth) ((uint4*)S.sel)[p] = make_uint4(0u, 0u, 0u, 0xFFFFFFFFu);  // {hi = 0, lo = 0, j = none}
}

__device__ __forceinline__ unsigned long long shfl_xor64(unsigned long long v, int d) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
  return wgrp::u64_of(lo, hi);
}

// One atomic per peer and wave instead of one per lane (a flood of one peer's initiations would otherwise queue
// 65,536 atomics on one address): the wave's lanes that take part (`on`) are walked peer by peer, the lowest such
// lane's peer first; the group's values are reduced by butterfly to their maximum (MAX) or minimum, which every
// lane of the group receives in v, and the group's lowest lane returns true: it issues the atomic. The loop's trips
// are wave-uniform (a ballot), one per distinct peer among the lanes. Every lane of the wave must reach the call.
template <bool MAX>
__device__ __forceinline__ bool wave_by_peer(bool on, uint32_t p, unsigned long long& v) {
  const uint32_t lane = threadIdx.x & 63u;
  bool lead = false;
  unsigned long long todo = __ballot(on);
  while (todo) {
    const uint32_t first = (uint32_t)__ffsll((long long)todo) - 1u;
    const uint32_t p0 = (uint32_t)__shfl((int)p, (int)first);
    const bool mine = on && p == p0;
    unsigned long long m = mine ? v : (MAX ? 0ull : ~0ull);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned long long o = shfl_xor64(m, d);
      m = MAX ? (o > m ? o : m) : (o < m ? o : m);
    }
    if (mine) {
      v = m;
      lead = lane == first;
    }
    todo &= ~__ballot(mine);
  }
  return lead;
}

// the entry of this lane for the selection: {T, state}, whether it is still a candidate, its peer
__device__ __forceinline__ bool stamp_cand(const StampParams& P, uint32_t j, uint32_t nl, uint4& t, uint32_t& p) {
  const bool in = j < nl;
  t = in ? P.res[j] : make_uint4(0u, 0u, 0u, 0u);
  const bool cand = in && t.w == kStampCand;
  p = cand ? stamp_peer(P, j) : 0u;
  return cand;
}

// REPLAY against the value at the start of the call; else the maximum of the high 8 bytes
__global__ void __launch_bounds__(256) k_hs_stamp_hi(StampParams P) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x, nl = stamp_len(P);
  if ((j & ~63u) >= nl) return;  // (wave-uniform)
  uint4 t;
  uint32_t p;
  bool cand = stamp_cand(P, j, nl, t, p);
  const HsStampHdr S = *P.stamps;
  unsigned long long v = stamp_hi(t);
  if (cand) {
    const HsStamp have = S.stored[p];
    if (v < have.hi || (v == have.hi && stamp_lo(t) <= have.lo)) {
      P.res[j].w = WG_HS_TS_REPLAY;
      cand = false;
    }
  }
  if (wave_by_peer<true>(cand, p, v)) (void)atomicMax(&S.sel[p].hi, v);
}

// ... of the low 4 bytes among the entries that hold it
__global__ void __launch_bounds__(256) k_hs_stamp_lo(StampParams P) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x, nl = stamp_len(P);
  if ((j & ~63u) >= nl) return;  // (wave-uniform)
  uint4 t;
  uint32_t p;
  const bool cand = stamp_cand(P, j, nl, t, p);
  HsStampSel* sel = P.stamps->sel + p;
  unsigned long long v = stamp_lo(t);
  if (wave_by_peer<true>(cand && stamp_hi(t) == sel->hi, p, v)) (void)atomicMax(&sel->lo, (uint32_t)v);
}

// ... and the lowest position among the entries that still tie
__global__ void __launch_bounds__(256) k_hs_stamp_j(StampParams P) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x, nl = stamp_len(P);
  if ((j & ~63u) >= nl) return;  // (wave-uniform)
  uint4 t;
  uint32_t p;
  const bool cand = stamp_cand(P, j, nl, t, p);
  HsStampSel* sel = P.stamps->sel + p;
  unsigned long long v = j;
  if (wave_by_peer<false>(cand && stamp_hi(t) == sel->hi && stamp_lo(t) == sel->lo, p, v)) (void)atomicMin(&sel->j, (uint32_t)v);
}

// statuses, opened timestamps, the winners' T as their peers' stored value; the range's counts
__global__ void __launch_bounds__(256) k_hs_stamp_commit(StampParams P) {
  __shared__ uint32_t s_cnt[4][4];
  const uint32_t nl = stamp_len(P);
  if (blockIdx.x * kRankRange >= nl) {  // past the entries (workgroup-uniform): a zero record for the scan
    if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const uint32_t j = blockIdx.x * kRankRange + threadIdx.x;
  const bool in = j < nl;
  uint32_t st = WG_HS_TS_BADDESC;
  if (in) {
    const uint4 t = P.res[j];
    st = t.w;
    if (st == kStampCand) {
      const HsStampHdr S = *P.stamps;
      const uint32_t p = stamp_peer(P, j);
      st = S.sel[p].j == j ? WG_HS_TS_OK : WG_HS_TS_SUPERSEDED;
      if (st == WG_HS_TS_OK) S.stored[p] = HsStamp{stamp_hi(t), stamp_lo(t), 0u};
      P.res[j].w = st;  // (the emit reads it)
    }
    P.ts_status[j] = st;
    uint32_t* o = (uint32_t*)(P.opened + 12ull * j);  // (zeros where the tag did not verify: the chain left them)
    o[0] = t.x;
    o[1] = t.y;
    o[2] = t.z;
  }
  uint32_t r, n_ok, n_stale, n_bad, n_skip;
  wgrp::block_rank(in && st == WG_HS_TS_OK, s_cnt[0], r, n_ok);
  wgrp::block_rank(in && (st == WG_HS_TS_REPLAY || st == WG_HS_TS_SUPERSEDED), s_cnt[1], r, n_stale);
  wgrp::block_rank(in && st == WG_HS_TS_BADAUTH, s_cnt[2], r, n_bad);
  wgrp::block_rank(in && (st == WG_HS_TS_NOPEER || st == WG_HS_TS_BADDESC), s_cnt[3], r, n_skip);
  if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4(n_ok, n_stale, n_bad, n_skip);
}

// fresh[prefix of the range + rank in the range] = this OK entry, byte for byte
__global__ void __launch_bounds__(256) k_hs_stamp_emit(StampParams P) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t nl = stamp_len(P);
  if (blockIdx.x * kRankRange >= nl) return;  // (workgroup-uniform)
  const uint32_t j = blockIdx.x * kRankRange + threadIdx.x;
  const bool ok = j < nl && P.res[j].w == WG_HS_TS_OK;
  const uint4 pre = P.part[blockIdx.x];
  uint32_t r, total;
  wgrp::block_rank(ok, s_cnt, r, total);
  if (!ok) return;
  const uint4* in = (const uint4*)(P.inits + j);
  uint4* o = (uint4*)(P.fresh + (pre.x + r));
#pragma unroll
  for (uint32_t g = 0; g < sizeof(wg_hs_init) / 16u; ++g) o[g] = in[g];
}

}  // namespace wgts

// ---- C ABI --------------------------------------------------------------------------------
namespace {

static_assert(sizeof(HsStamp) == 16 && sizeof(HsStampSel) == 16, "a peer's stamp and its selection words are one uint4 each");

// the stamps' header for the current table. Caller holds c->mu and has synchronised the device.
int hs_stamp_header(wg_ctx* c, HsState* t) {
  HsStampHdr S{};
  S.stored = (HsStamp*)t->d_stamps.p;
  S.sel = (HsStampSel*)t->d_ssel.p;
  S.count = t->n_peers;
  HIPTRY(hipMemcpyAsync(t->d_shdr.p, &S, sizeof S, hipMemcpyHostToDevice, c->stream));
  HIPTRY(hipStreamSynchronize(c->stream));
  return WG_OK;
}

// wg_hs_peers_set's part of this stage: a stamp and the selection's words per peer of the new table, all zero.
// Caller holds c->mu and has synchronised the device.
int hs_stamp_peers_reset(wg_ctx* c, HsState* t) {
  const size_t bytes = 16ull * std::max(t->n_peers, 1u);
  int rc;
  if ((rc = t->d_stamps.ensure(bytes)) != WG_OK || (rc = t->d_ssel.ensure(bytes)) != WG_OK) {
    t->d_stamps.release();  // no table of stamps: no peer passes
    t->d_ssel.release();
    const uint32_t keep = t->n_peers;
    t->n_peers = 0;
    (void)hs_stamp_header(c, t);
    t->n_peers = keep;
    return rc;
  }
  HIPTRY(hipMemsetAsync(t->d_stamps.p, 0, t->d_stamps.cap, c->stream));
  HIPTRY(hipMemsetAsync(t->d_ssel.p, 0, t->d_ssel.cap, c->stream));
  return hs_stamp_header(c, t);
}

// The stamps' state, allocated at the first wg_hs_stamp* call. Caller holds c->mu; never on a capturing stream.
int hs_stamp_get(wg_ctx* c, HsState* t) {
  if (t->has_stamps) return WG_OK;
  int rc;
  HIPTRY(hipDeviceSynchronize());
  if ((rc = t->d_shdr.ensure(sizeof(HsStampHdr))) != WG_OK) return rc;
  t->has_stamps = true;
  if ((rc = hs_stamp_grow(t, t->reserved)) == WG_OK) rc = hs_stamp_peers_reset(c, t);
  if (rc != WG_OK) t->has_stamps = false;
  return rc;
}

// the peers' range [first, first + n) of wg_hs_stamps_set / _get, with the state behind it. Caller holds c->mu.
int hs_stamp_range(wg_ctx* c, uint32_t first, uint32_t n, const void* host, HsState** out) {
  if (!host && n) return fail(WG_EINVAL, "NULL argument");
  HsState* t;
  int rc;
  if ((rc = hs_get(c, &t)) != WG_OK || (rc = hs_stamp_get(c, t)) != WG_OK) return rc;
  if ((uint64_t)first + n > t->n_peers) return fail(WG_ERANGE, "stamps [%u, %u + %u) of a peer table of %u", first, first, n, t->n_peers);
  *out = t;
  return WG_OK;
}

}  // namespace

extern "C" {

int wg_hs_stamps_set(wg_ctx* c, uint32_t first_peer, uint32_t n, const uint8_t* stamps) {
  if (!c) return fail(WG_EINVAL, "NULL context");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HsState* t;
  int rc;
  if ((rc = hs_stamp_range(c, first_peer, n, stamps, &t)) != WG_OK || !n) return rc;
  std::vector<HsStamp> v(n);
  for (uint32_t k = 0; k < n; ++k) {
    const uint8_t* b = stamps + 12ull * k;
    unsigned long long hi = 0;
    uint32_t lo = 0;
    for (int i = 0; i < 8; ++i) hi = (hi << 8) | b[i];
    for (int i = 8; i < 12; ++i) lo = (lo << 8) | b[i];
    v[k] = HsStamp{hi, lo, 0u};
  }
  HIPTRY(hipDeviceSynchronize());  // no stamp queued earlier (on any stream) may still read or write the old values
  HIPTRY(hipMemcpyAsync((HsStamp*)t->d_stamps.p + first_peer, v.data(), 16ull * n, hipMemcpyHostToDevice, c->stream));
  HIPTRY(hipStreamSynchronize(c->stream));
  return WG_OK;
}

int wg_hs_stamps_get(wg_ctx* c, uint32_t first_peer, uint32_t n, uint8_t* stamps) {
  if (!c) return fail(WG_EINVAL, "NULL context");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HsState* t;
  int rc;
  if ((rc = hs_stamp_range(c, first_peer, n, stamps, &t)) != WG_OK || !n) return rc;
  std::vector<HsStamp> v(n);
  HIPTRY(hipDeviceSynchronize());  // every stamp queued earlier (on any stream) has stored its timestamps
  HIPTRY(hipMemcpyAsync(v.data(), (const HsStamp*)t->d_stamps.p + first_peer, 16ull * n, hipMemcpyDeviceToHost, c->stream));
  HIPTRY(hipStreamSynchronize(c->stream));
  for (uint32_t k = 0; k < n; ++k) {
    uint8_t* b = stamps + 12ull * k;
    for (int i = 0; i < 8; ++i) b[i] = (uint8_t)(v[k].hi >> (56 - 8 * i));
    for (int i = 0; i < 4; ++i) b[8 + i] = (uint8_t)(v[k].lo >> (24 - 8 * i));
  }
  return WG_OK;
}

int wg_hs_stamp(wg_ctx* c, const wg_hs_stamp_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  if (b->flags || b->_reserved) return fail(WG_EINVAL, "wg_hs_stamp_batch.flags and ._reserved must be 0");
  if (((uintptr_t)b->n_inits) & 3u) return fail(WG_EINVAL, "n_inits must be 4-byte aligned");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (!c->hs || !c->hs->has_priv) return fail(WG_ENOKEY, "wg_hs_stamp before any wg_hs_static_set");
  HsState* t = c->hs;
  const uint32_t n = b->n, n_rec = b->n_rec;
  if (n == 0) return WG_OK;
  if (n > 0x40000000u || n_rec > 0x40000000u) return fail(WG_E2BIG, "handshake stamp of %u entries over %u records", n, n_rec);
  if (!b->inits || (((uintptr_t)b->inits) & 15u) || (n_rec && (!b->records || !b->shared)) || (((uintptr_t)b->records) & 15u) ||
      (((uintptr_t)b->shared) & 15u))
    return fail(WG_EINVAL, "inits / records / shared must be non-NULL and 16-byte aligned");
  if (!b->ts_status || (((uintptr_t)b->ts_status) & 3u) || !b->opened || (((uintptr_t)b->opened) & 3u) || !b->fresh ||
      (((uintptr_t)b->fresh) & 15u) || !b->summary || (((uintptr_t)b->summary) & 7u))
    return fail(WG_EINVAL, "ts_status / opened / fresh / summary must be non-NULL and aligned (4 / 4 / 16 / 8 bytes)");
  {
    const HsRange out[4] = {{b->ts_status, 4ull * n}, {b->opened, 12ull * n}, {b->fresh, sizeof(wg_hs_init) * (uint64_t)n},
                            {b->summary, sizeof(wg_hs_stamp_summary)}};
    const HsRange in[4] = {{b->inits, sizeof(wg_hs_init) * (uint64_t)n}, {b->n_inits, b->n_inits ? 4u : 0u},
                           {b->records, sizeof(wg_hs_record) * (uint64_t)n_rec}, {b->shared, 32ull * n_rec}};
    const int ov = hs_ranges_overlap(out, in);
    if (ov == 1) return fail(WG_EINVAL, "ts_status, opened, fresh and summary must not overlap");
    if (ov == 2) return fail(WG_EINVAL, "an output of wg_hs_stamp must not overlap inits, n_inits, records or shared");
  }
  const bool capturing = stream_capturing(s);
  int rc;
  if (capturing && !t->has_stamps)
    return fail(WG_EINVAL, "the first wg_hs_stamp on a capturing stream: call wg_hs_stamps_set(ctx, 0, 0, NULL) first");
  if ((rc = hs_stamp_get(c, t)) != WG_OK) return rc;
  if ((rc = plan_begin(t->order, s, capturing, hs_stamp_fits(t, n), [&] { return hs_stamp_grow(t, n); }, kHsStampWords, n)) != WG_OK)
    return rc;
  wgts::StampParams P{};
  P.inits = b->inits;
  P.n_inits = b->n_inits;
  P.records = b->records;
  P.shared = b->shared;
  P.ts_status = b->ts_status;
  P.opened = b->opened;
  P.fresh = b->fresh;
  P.hs0 = (const uint8_t*)t->d_key.p + 32;
  P.peers = (const HsPeerHdr*)t->d_phdr.p;
  P.stamps = (const HsStampHdr*)t->d_shdr.p;
  P.res = (uint4*)t->d_sres.p;
  P.part = (uint4*)t->d_spart.p;
  P.n = n;
  P.n_rec = n_rec;
  const uint32_t nb = rank_blocks(n);
  hipLaunchKernelGGL(wgts::k_hs_stamp_chain, dim3(nb), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgts::k_hs_stamp_hi, dim3(nb), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgts::k_hs_stamp_lo, dim3(nb), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgts::k_hs_stamp_j, dim3(nb), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgts::k_hs_stamp_commit, dim3(nb), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgrp::k_rx_scan, dim3(1), dim3(256), 0, s, P.part, nb, (uint2*)b->summary);
  hipLaunchKernelGGL(wgts::k_hs_stamp_emit, dim3(nb), dim3(256), 0, s, P);
  return plan_end(t->order, s, capturing, kHsStampWords);
}

}  // extern "C"
