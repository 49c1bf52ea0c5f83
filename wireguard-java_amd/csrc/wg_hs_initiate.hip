// wg_hs_initiate.hip — the initiator's side of the handshake, on the device (included by wg_capi.hip after
// wg_hs_respond.hip): wg_hs_psks_set, wg_hs_initiate and wg_hs_finish.
//
// The responder's half runs on the device end to end (wg_hs_check, wg_hs_dh, wg_hs_open, wg_hs_respond). A node
// that restarts, or whose sessions expire together, initiates to every peer that has an endpoint
// (SessionManager.attemptInitiatorHandshake, SessionManager.java:170-207): two ladders, four HKDFs, two AEAD
// seals and a keyed BLAKE2s per initiation (InitiatorStageOne's constructor, Handshakes.java:77-117;
// OutgoingInitiation.java:22-38; InitiationPacket.java:110-120), and two ladders, six HKDFs and an AEAD open per
// response (consumeMessageResponse, Handshakes.java:119-151). Both are programs for the machine of
// wg_hs_chain.hip plus a ladder kernel in k_hs_resp_dh's shape. What the device lacks is randomness and the
// clock: the ephemerals and the TAI64N timestamps arrive as buffers.
//
// The chains (H = BLAKE2s-256, KDFn = Crypto.deriveKey(salt, ikm, n); S the static private key, S_pub its public
// key, S_r the peer's static public key and ss_r = X25519(S, S_r) from wg_hs_peers_set's table, e the ephemeral):
//   Epub = X25519(e, 9)       h = H(H(H0 || S_r) || Epub)        ck = KDF1(CK0, Epub)
//   es = X25519(e, S_r)       k = KDF2(ck, es)   ck = KDF1(ck, es)
//   enc_static = AEAD-seal(k, nonce 0, aad = h, S_pub)           h = H(h || enc_static)
//   k = KDF2(ck, ss_r)        ck = KDF1(ck, ss_r)
//   enc_ts = AEAD-seal(k, nonce 0, aad = h, timestamp)           h = H(h || enc_ts)
//   msg = {1, 0,0,0, LE32(local_index), Epub, enc_static, enc_ts,
//          mac1 = BLAKE2s-128(key = H("mac1----" || S_r), msg[0 .. 116)), mac2 = 0^16}
// and, for a response with E_r = msg[12 .. 44), from the pending entry's e, h, ck and the peer's psk:
//   h = H(h || E_r)     ck = KDF1(ck, E_r)     ck = KDF1(ck, X25519(e, E_r))     ck = KDF1(ck, X25519(S, E_r))
//   tau = KDF2(ck, psk)   k = KDF3(ck, psk)   ck = KDF1(ck, psk)       h = H(h || tau)
//   the tag of (aad = h, no ciphertext) under k, nonce 0, must equal msg[44 .. 60)
//   send_key = KDF1(ck, "")      recv_key = KDF2(ck, "")          (:147: the initiator sends with T1)
//
// k_hs_init_dh, k_hs_fin_dh: k_hs_resp_dh's shape with two lanes per item. Lane L runs ladder L % 2 of item L / 2
// (initiate: the base point, S_r; finish: e on E_r, S on E_r) and stores its 32 bytes at scratch + 32 L. Each
// lane decides its item's status for itself (finish: it looks the receiver index up); a lane whose item is not
// worked on, and a lane past the cover, runs the dummy ladder and stores nothing; waves wholly past the cover
// exit.
//
// k_hs_init_chain: one entry per lane, the 35 steps of kInitProgram. kCk0Ipad / kCk0Opad serve the first extract
// as in k_hs_open. The kernel's own operations: H(H0 || S_r); the two seals, each in front of the hash of what
// it made, its key being the T2 that the step before left in the state (OP_IES1, OP_ITS: the way OP_ES1 opens);
// the two blocks of H(h || enc_static) and the one of H(h || enc_ts); the four compressions of mac1 under the
// PEER's key. enc_static's AEAD is two register chacha20_blocks and wghc::poly_tag<2>; the timestamp's
// ciphertext is 12 bytes, a part block: wghc::poly_tag_bytes<1> takes it padded with zeros and puts 12 into
// the length block. The 19 words of the two ciphertexts stay in registers until the record is written. After
// the loop the lane writes record and pending entry, and overwrites its 64 bytes of ladder scratch and its
// consumed ephemeral with zeros. The counts go to k_rx_scan as they do in a rank, and there is no emit: BADPEER
// and NOEPH are the caller's own mistakes, the outputs are aligned to position.
//
// k_hs_fin_chain: one record per lane, the 47 steps of kFinProgram: kRespProgram without mac1, the psk as a
// source where the responder has zeros, and the tag of nothing (wghr::seal_empty, on the same flagged step)
// compared with the response's in all 16 bytes. k_hs_fin_emit places the authentic ones, wipes the keys it moved
// and overwrites each consumed pending entry with zeros. Nothing reads a pending entry in that launch, so two
// authentic records against one entry are both emitted, in record order; a BADAUTH record writes nothing.
//
// The lookup. The response's receiver index names the pending entry. The first two launches of a finish build an
// open-addressing table of pending positions in scratch: k_hs_fin_fill zeroes capacity words (the smallest power
// of two >= max(16, 4 n_pending)), k_hs_fin_insert claims, per live entry (state 1, peer below the table's
// count), the first empty slot from mix32(local_index) & mask with a compare-and-swap; on a slot whose entry has
// the same local_index it takes the minimum position instead, so the lowest position wins whatever order the
// lanes ran in. Probing is linear, as hs_peer's. Every word is written before it is read in each call, nothing
// about a call lives on the host: a captured check + finish replays.
//
// Constant time: no branch, address or loop bound depends on an ephemeral's value, a DH result, ck, tau, k, a psk's
// value or a transport key. The exceptions are the public receiver index and peer position, the all-zero test of
// the raw ephemeral, and the statuses (the tag comparison's outcome among them). Every secret is written with
// plain 16-byte vector stores.
#pragma once

namespace wghi {

constexpr uint32_t kLadU4 = 4;   // ladder scratch per item, in uint4: two results
constexpr uint32_t kRecU4 = 10;  // a wg_hs_record
constexpr uint32_t kPendU4 = 7;  // a wg_hs_pending
constexpr uint32_t kEstU4 = 6;   // a wg_hs_established

// H0 = INITIAL_HASH (Handshakes.java:20-37) as little-endian words: 2211b361...ba079ef3
__device__ constexpr uint32_t kH0[8] = {0x61B31122u, 0x66C51A08u, 0xDB431269u, 0x32D58A45u,
                                        0x666C9C2Du, 0xB7E89322u, 0x659CE10Eu, 0xF39E07BAu};

struct InitParams {
  const uint32_t* peer;
  uint8_t* ephemerals;
  const uint8_t* timestamps;
  const uint32_t* local_index;
  uint32_t* status;
  wg_hs_record* records;
  wg_hs_pending* pending;
  const uint8_t* spub;  // the static public key, 32 B (fixed address)
  const HsPeerHdr* peers;
  uint4* lad;
  uint4* part;
  uint32_t n;
};

struct FinParams {
  const wg_hs_record* records;
  const uint32_t* n_records;
  wg_hs_pending* pending;
  uint32_t* fin_status;
  wg_hs_established* established;
  const uint8_t* priv;  // the static private key, 32 B (fixed address)
  const HsPeerHdr* peers;
  const HsPskHdr* psks;
  uint32_t* tab;
  uint4* lad;
  uint4* res;
  uint4* part;
  uint32_t n;
  uint32_t n_pending;
  uint32_t mask;
};

// ---- wg_hs_initiate ------------------------------------------------------------------------

// the status of entry k (k < n), its peer and its raw ephemeral
__device__ __forceinline__ uint32_t init_status_of(const InitParams& P, uint32_t count, uint32_t k, uint32_t& peer, uint4& e0, uint4& e1) {
  const uint4* ep = (const uint4*)(P.ephemerals + 32ull * k);
  e0 = ep[0];
  e1 = ep[1];
  peer = P.peer[k];
  if (peer >= count) return WG_HS_INIT_BADPEER;
  const uint32_t any = e0.x | e0.y | e0.z | e0.w | e1.x | e1.y | e1.z | e1.w;
  return any ? WG_HS_INIT_OK : WG_HS_INIT_NOEPH;
}

// lane L: ladder L % 2 of entry L / 2 (0: the base point, 1: S_r), its 32 bytes to lad + 2 L
__global__ void __launch_bounds__(64) k_hs_init_dh(InitParams P) {
  const uint64_t lanes = 2ull * P.n;
  if ((uint64_t)blockIdx.x * 64u >= lanes) return;  // (wave-uniform)
  const uint64_t L = (uint64_t)blockIdx.x * 64u + threadIdx.x;
  uint32_t k[8], u[8], out[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    k[j] = 0u;
    u[j] = j == 0 ? 9u : 0u;
  }
  bool go = false;
  if (L < lanes) {
    const HsPeerHdr H = *P.peers;
    const uint32_t i = (uint32_t)(L >> 1), which = (uint32_t)(L & 1u);
    uint32_t peer;
    uint4 e0, e1;
    go = init_status_of(P, H.count, i, peer, e0, e1) == WG_HS_INIT_OK;
    if (go) {
      k[0] = e0.x; k[1] = e0.y; k[2] = e0.z; k[3] = e0.w; k[4] = e1.x; k[5] = e1.y; k[6] = e1.z; k[7] = e1.w;
      if (which) {
        const uint4* pt = (const uint4*)(H.publics + 32ull * peer);
        const uint4 p0 = pt[0], p1 = pt[1];
        u[0] = p0.x; u[1] = p0.y; u[2] = p0.z; u[3] = p0.w; u[4] = p1.x; u[5] = p1.y; u[6] = p1.z; u[7] = p1.w;
      }
    }
  }
  (void)wgx::x25519(out, k, u);
  if (!go) return;
  uint4* o = P.lad + 2ull * L;
  o[0] = make_uint4(out[0], out[1], out[2], out[3]);
  o[1] = make_uint4(out[4], out[5], out[6], out[7]);
}

// es = AEAD-seal(key, nonce 0, aad, the 32 bytes pt): 8 words of ciphertext, 4 of tag
__device__ __forceinline__ void seal_static(const uint32_t key[8], const uint32_t aad[8], const uint32_t pt[8], uint32_t es[12]) {
  uint32_t ks[16];
  wgd::chacha20_block(key, 1u, 0u, 0u, 0u, ks);
#pragma unroll
  for (int j = 0; j < 8; ++j) es[j] = pt[j] ^ ks[j];
  wgd::chacha20_block(key, 0u, 0u, 0u, 0u, ks);
  wghc::poly_tag<2>(ks, aad, es, es + 8);
}

// ets = AEAD-seal(key, nonce 0, aad, the 12 bytes ts): 3 words of ciphertext, 4 of tag
__device__ __forceinline__ void seal_timestamp(const uint32_t key[8], const uint32_t aad[8], const uint32_t ts[3], uint32_t ets[7]) {
  uint32_t ks[16], ct[4];
  wgd::chacha20_block(key, 1u, 0u, 0u, 0u, ks);
#pragma unroll
  for (int j = 0; j < 3; ++j) ets[j] = ct[j] = ts[j] ^ ks[j];
  ct[3] = 0u;
  wgd::chacha20_block(key, 0u, 0u, 0u, 0u, ks);
  wghc::poly_tag_bytes<1>(ks, aad, ct, 12u, ets + 3);
}

// One entry per lane: status, record and pending entry; the range's counts.
__global__ void __launch_bounds__(256) k_hs_init_chain(InitParams P) {
  __shared__ uint32_t s_cnt[3][4];
  const uint32_t nl = P.n;
  const uint32_t k = blockIdx.x * kRankRange + threadIdx.x;
  const bool in = k < nl;
  uint32_t st_out = WG_HS_INIT_NOEPH;
  if ((k & ~63u) < nl) {  // (wave-uniform: a wave wholly past the entries goes straight to the counts)
    const HsPeerHdr H = *P.peers;
    uint32_t peer = 0;
    uint4 e0 = make_uint4(0u, 0u, 0u, 0u), e1 = e0;
    if (in) st_out = init_status_of(P, H.count, k, peer, e0, e1);
    const bool go = in && st_out == WG_HS_INIT_OK;
    // a lane that initiates nothing runs the chain over zeros and stores zeros
    const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
    const uint4* lad = P.lad + (size_t)kLadU4 * (go ? k : 0u);
    const uint4* sr = (const uint4*)(H.publics + 32ull * (go ? peer : 0u));
    using namespace wghc;
    Chain c;
    clear(c);
    set8(c.ist, wgho::kCk0Ipad);  // KDF1(CK0, Epub) starts from the constant key-block states
    set8(c.ost, wgho::kCk0Opad);
    uint32_t es[12], ets[7];
#pragma unroll
    for (int j = 0; j < 12; ++j) es[j] = 0u;
#pragma unroll
    for (int j = 0; j < 7; ++j) ets[j] = 0u;
    const uint32_t li = go ? P.local_index[k] : 0u;
    Step s = fetch(kInitProgram, 0u);
#pragma unroll 1
    for (uint32_t step = 0; step < kInitSteps; ++step) {
      uint32_t src[8];
      switch (s.arg) {
        case SRC_EPUB: put8(src, go ? lad[0] : z4, go ? lad[1] : z4); break;
        case SRC_ES: put8(src, go ? lad[2] : z4, go ? lad[3] : z4); break;
        case SRC_STATIC: {  // the peer's static-static secret
          const uint4* q = (const uint4*)(H.secrets + 32ull * (go ? peer : 0u));
          put8(src, go ? q[0] : z4, go ? q[1] : z4);
          break;
        }
        default: source(c, s.arg, src); break;
      }
      switch (s.op) {
        case OP_IH0:  // H(H0 || S_r)
          set8(c.m, kH0);
          put8(c.m + 8, go ? sr[0] : z4, go ? sr[1] : z4);
          wghs::b2s_init(c.st, 32u, 0u);
          c.t = 64u; c.last = true;
          break;
        case OP_IES1: {  // st = T2 = the key: seal S_pub; then h = H(h || encrypted_static), first block
          uint32_t pt[8];
          const uint4* q = (const uint4*)P.spub;
          put8(pt, q[0], q[1]);
          seal_static(c.st, c.hh, pt, es);
          set8(c.m, c.hh);
          set8(c.m + 8, es);
          wghs::b2s_init(c.st, 32u, 0u);
          c.t = 64u; c.last = false;
          break;
        }
        case OP_IES2:  // ... second block: the tag
          c.m[0] = es[8]; c.m[1] = es[9]; c.m[2] = es[10]; c.m[3] = es[11];
#pragma unroll
          for (int j = 4; j < 16; ++j) c.m[j] = 0u;
          c.t = 80u; c.last = true;
          break;
        case OP_ITS: {  // st = T2 = the key: seal the timestamp; then h = H(h || encrypted_timestamp), 60 bytes
          uint32_t ts[3];
          const uint32_t* q = (const uint32_t*)(P.timestamps + 12ull * (go ? k : 0u));
          ts[0] = go ? q[0] : 0u; ts[1] = go ? q[1] : 0u; ts[2] = go ? q[2] : 0u;
          seal_timestamp(c.st, c.hh, ts, ets);
          set8(c.m, c.hh);
#pragma unroll
          for (int j = 0; j < 7; ++j) c.m[8 + j] = ets[j];
          c.m[15] = 0u;
          wghs::b2s_init(c.st, 32u, 0u);
          c.t = 60u; c.last = true;
          break;
        }
        case OP_MAC1KEY: {  // the mac1 key, H("mac1----" || S_r): 40 bytes
          uint32_t w[8];
          put8(w, go ? sr[0] : z4, go ? sr[1] : z4);
          c.m[0] = 0x3163616Du;
          c.m[1] = 0x2D2D2D2Du;
          set8(c.m + 2, w);
#pragma unroll
          for (int j = 10; j < 16; ++j) c.m[j] = 0u;
          wghs::b2s_init(c.st, 32u, 0u);
          c.t = 40u; c.last = true;
          break;
        }
        case OP_MAC1A:  // mac1 = BLAKE2s-128 under that key (in ist): the key block
          msg32(c.m, c.ist);
          wghs::b2s_init(c.st, 16u, 32u);
          c.t = 64u; c.last = false;
          break;
        case OP_IMAC1B: {  // ... initiation[0 .. 64): type, sender index, Epub, 24 bytes of encrypted_static
          uint32_t w[8];
          put8(w, go ? lad[0] : z4, go ? lad[1] : z4);
          c.m[0] = 1u;
          c.m[1] = li;
          set8(c.m + 2, w);
#pragma unroll
          for (int j = 0; j < 6; ++j) c.m[10 + j] = es[j];
          c.t = 128u; c.last = false;
          break;
        }
        case OP_IMAC1C:  // ... and initiation[64 .. 116): the rest of encrypted_static, encrypted_timestamp
#pragma unroll
          for (int j = 0; j < 6; ++j) c.m[j] = es[6 + j];
#pragma unroll
          for (int j = 0; j < 7; ++j) c.m[6 + j] = ets[j];
          c.m[13] = c.m[14] = c.m[15] = 0u;
          c.t = 180u; c.last = true;
          break;
        default: prepare(c, s, src); break;
      }
      const Step ahead = fetch(kInitProgram, step + 1u);
      wghs::b2s_compress(c.st, c.m, c.t, c.last);
      WG_HSC_PUT(c, s.dst);
      s = ahead;
    }
    if (in) {
      uint4* rec = (uint4*)(P.records + k);
      uint4* pe = (uint4*)(P.pending + k);
      if (go) {
        rec[0] = make_uint4(k, WG_HS_INIT_SIZE, 1u, li);
        rec[1] = lad[0];
        rec[2] = lad[1];
        rec[3] = make_uint4(es[0], es[1], es[2], es[3]);
        rec[4] = make_uint4(es[4], es[5], es[6], es[7]);
        rec[5] = make_uint4(es[8], es[9], es[10], es[11]);
        rec[6] = make_uint4(ets[0], ets[1], ets[2], ets[3]);
        rec[7] = make_uint4(ets[4], ets[5], ets[6], c.st[0]);
        rec[8] = make_uint4(c.st[1], c.st[2], c.st[3], 0u);
        rec[9] = z4;
        pe[0] = make_uint4(1u, peer, li, 0u);
        pe[1] = e0;
        pe[2] = e1;
        pe[3] = make_uint4(c.hh[0], c.hh[1], c.hh[2], c.hh[3]);
        pe[4] = make_uint4(c.hh[4], c.hh[5], c.hh[6], c.hh[7]);
        pe[5] = make_uint4(c.ck[0], c.ck[1], c.ck[2], c.ck[3]);
        pe[6] = make_uint4(c.ck[4], c.ck[5], c.ck[6], c.ck[7]);
        // the ladders' results and the ephemeral are spent
        uint4* wl = P.lad + (size_t)kLadU4 * k;
#pragma unroll
        for (uint32_t g = 0; g < kLadU4; ++g) wl[g] = z4;
        uint4* we = (uint4*)(P.ephemerals + 32ull * k);
        we[0] = z4;
        we[1] = z4;
      } else {
#pragma unroll
        for (uint32_t g = 0; g < kRecU4; ++g) rec[g] = z4;
#pragma unroll
        for (uint32_t g = 0; g < kPendU4; ++g) pe[g] = z4;
      }
      P.status[k] = st_out;
    }
  }
  uint32_t r, n_ok, n_badpeer, n_noeph;
  wgrp::block_rank(in && st_out == WG_HS_INIT_OK, s_cnt[0], r, n_ok);
  wgrp::block_rank(in && st_out == WG_HS_INIT_BADPEER, s_cnt[1], r, n_badpeer);
  wgrp::block_rank(in && st_out == WG_HS_INIT_NOEPH, s_cnt[2], r, n_noeph);
  if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4(n_ok, n_badpeer, n_noeph, 0u);
}

// ---- wg_hs_finish --------------------------------------------------------------------------

__device__ __forceinline__ uint32_t fin_len(const FinParams& P) { return wgrp::dev_count(P.n_records, P.n); }

__global__ void __launch_bounds__(256) k_hs_fin_fill(FinParams P) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i <= P.mask) P.tab[i] = 0u;
}

// pending position p, if live, into the table: position + 1 at the first empty slot from its bucket, or the
// minimum with what an entry of the same local_index left there
__global__ void __launch_bounds__(256) k_hs_fin_insert(FinParams P) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= P.n_pending) return;
  const uint4 q = ((const uint4*)(P.pending + p))[0];  // {state, peer, local_index, 0}
  if (q.x != 1u || q.y >= P.peers->count) return;
  uint32_t b = mix32(q.z);
  for (uint32_t probes = 0; probes <= P.mask; ++probes, ++b) {  // (a table a quarter full ends the walk long before)
    uint32_t* slot = P.tab + (b & P.mask);
    const uint32_t old = atomicCAS(slot, 0u, p + 1u);
    if (!old) return;
    if (((const uint4*)(P.pending + (old - 1u)))[0].z == q.z) {
      (void)atomicMin(slot, p + 1u);
      return;
    }
  }
}

// position + 1 of the live pending entry with this local_index, 0 if there is none
__device__ __forceinline__ uint32_t fin_lookup(const FinParams& P, uint32_t index) {
  uint32_t b = mix32(index);
  for (uint32_t probes = 0; probes <= P.mask; ++probes, ++b) {
    const uint32_t e = P.tab[b & P.mask];
    if (!e) return 0u;
    if (((const uint4*)(P.pending + (e - 1u)))[0].z == index) return e;
  }
  return 0u;
}

// the status of record k (k below the cover) before the tag is looked at: SKIPPED, BADDESC, NOPENDING, or OK with
// pos = the pending entry's position + 1
__device__ __forceinline__ uint32_t fin_status_of(const FinParams& P, uint32_t k, uint32_t& pos) {
  const uint4* rec = (const uint4*)(P.records + k);
  const uint32_t len = rec[0].y;
  pos = 0u;
  if (len == WG_HS_INIT_SIZE) return WG_HS_FIN_SKIPPED;
  if (len != WG_HS_RESP_SIZE) return WG_HS_FIN_BADDESC;
  pos = fin_lookup(P, rec[1].x);  // msg[8 .. 12): the receiver index
  return pos ? WG_HS_FIN_OK : WG_HS_FIN_NOPENDING;
}

// E_r = msg[12 .. 44): bytes 20 .. 52 of the record
__device__ __forceinline__ void fin_remote_ephemeral(const uint4* rec, uint32_t w[8]) {
  const uint4 a = rec[1], b = rec[2];
  w[0] = a.y; w[1] = a.z; w[2] = a.w; w[3] = b.x; w[4] = b.y; w[5] = b.z; w[6] = b.w; w[7] = rec[3].x;
}

// lane L: ladder L % 2 of record L / 2 (0: e on E_r, 1: S on E_r), its 32 bytes to lad + 2 L
__global__ void __launch_bounds__(64) k_hs_fin_dh(FinParams P) {
  const uint64_t lanes = 2ull * fin_len(P);
  if ((uint64_t)blockIdx.x * 64u >= lanes) return;  // (wave-uniform)
  const uint64_t L = (uint64_t)blockIdx.x * 64u + threadIdx.x;
  uint32_t k[8], u[8], out[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    k[j] = 0u;
    u[j] = j == 0 ? 9u : 0u;
  }
  bool go = false;
  if (L < lanes) {
    const uint32_t i = (uint32_t)(L >> 1), which = (uint32_t)(L & 1u);
    uint32_t pos;
    go = fin_status_of(P, i, pos) == WG_HS_FIN_OK;
    if (go) {
      const uint4* sc = which ? (const uint4*)P.priv : (const uint4*)(P.pending + (pos - 1u)) + 1;
      const uint4 s0 = sc[0], s1 = sc[1];
      k[0] = s0.x; k[1] = s0.y; k[2] = s0.z; k[3] = s0.w; k[4] = s1.x; k[5] = s1.y; k[6] = s1.z; k[7] = s1.w;
      fin_remote_ephemeral((const uint4*)(P.records + i), u);
    }
  }
  (void)wgx::x25519(out, k, u);
  if (!go) return;
  uint4* o = P.lad + 2ull * L;
  o[0] = make_uint4(out[0], out[1], out[2], out[3]);
  o[1] = make_uint4(out[4], out[5], out[6], out[7]);
}

// One record per lane: status, and for an authentic one its entry to scratch; the range's counts.
__global__ void __launch_bounds__(256) k_hs_fin_chain(FinParams P) {
  __shared__ uint32_t s_cnt[4][4];
  const uint32_t nl = fin_len(P);
  if (blockIdx.x * kRankRange >= nl) {  // past the records (workgroup-uniform): a zero record for the scan
    if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const uint32_t k = blockIdx.x * kRankRange + threadIdx.x;
  const bool in = k < nl;
  uint32_t st_out = WG_HS_FIN_BADDESC;
  if ((k & ~63u) < nl) {  // (wave-uniform: a wave wholly past the records goes straight to the counts)
    uint32_t pos = 0;
    if (in) st_out = fin_status_of(P, k, pos);
    const bool go = in && st_out == WG_HS_FIN_OK;
    // a lane that finishes nothing runs the chain over zeros and stores nothing
    const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
    const uint4* rec = (const uint4*)(P.records + (go ? k : 0u));
    const uint4* pe = (const uint4*)(P.pending + (go ? pos - 1u : 0u));
    const uint4* lad = P.lad + (size_t)kLadU4 * (go ? k : 0u);
    const uint4 p0 = go ? pe[0] : z4;  // {state, peer, local_index, 0}
    const uint4* psk = (const uint4*)(P.psks->psks + 32ull * p0.y);
    using namespace wghc;
    Chain c;
    clear(c);
    uint32_t tag[4] = {0u, 0u, 0u, 0u}, er[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) er[j] = 0u;
    if (go) {
      put8(c.hh, pe[3], pe[4]);
      put8(c.ck, pe[5], pe[6]);
      fin_remote_ephemeral(rec, er);
    }
    Step s = fetch(kFinProgram, 0u);
#pragma unroll 1
    for (uint32_t step = 0; step < kFinSteps; ++step) {
      uint32_t src[8];
      switch (s.arg) {
        case SRC_ER: set8(src, er); break;
        case SRC_EE: put8(src, go ? lad[0] : z4, go ? lad[1] : z4); break;
        case SRC_ES: put8(src, go ? lad[2] : z4, go ? lad[3] : z4); break;
        case SRC_PSK: put8(src, go ? psk[0] : z4, go ? psk[1] : z4); break;
        default: source(c, s.arg, src); break;
      }
      // the flagged key block: x = k, the tag of nothing under it, before the transport keys' KDF takes x
      if (s.op == OP_PAD && (s.imm & PAD_SEAL)) wghr::seal_empty(c.x, c.hh, tag);
      prepare(c, s, src);
      const Step ahead = fetch(kFinProgram, step + 1u);
      wghs::b2s_compress(c.st, c.m, c.t, c.last);
      WG_HSC_PUT(c, s.dst);
      s = ahead;
    }
    if (go) {
      const uint4 r3 = rec[3], r4 = rec[4];  // msg[44 .. 60): bytes 52 .. 68 of the record
      const uint32_t diff = (tag[0] ^ r3.y) | (tag[1] ^ r3.z) | (tag[2] ^ r3.w) | (tag[3] ^ r4.x);  // all 16 bytes
      st_out = diff ? WG_HS_FIN_BADAUTH : WG_HS_FIN_OK;
      if (!diff) {
        const uint4 r0 = rec[0];  // {index, len, msg[0 .. 4), msg[4 .. 8) = the responder's index}
        uint4* o = P.res + (size_t)kEstU4 * k;
        o[0] = make_uint4(r0.x, k, pos - 1u, p0.y);
        o[1] = make_uint4(p0.z, r0.w, 0u, 0u);
        o[2] = make_uint4(c.ck[0], c.ck[1], c.ck[2], c.ck[3]);
        o[3] = make_uint4(c.ck[4], c.ck[5], c.ck[6], c.ck[7]);
        o[4] = make_uint4(c.x[0], c.x[1], c.x[2], c.x[3]);
        o[5] = make_uint4(c.x[4], c.x[5], c.x[6], c.x[7]);
      }
      // the ladders' results are spent
      uint4* wl = P.lad + (size_t)kLadU4 * k;
#pragma unroll
      for (uint32_t g = 0; g < kLadU4; ++g) wl[g] = z4;
    }
    if (in) P.fin_status[k] = st_out;
  }
  uint32_t r, n_ok, n_nop, n_bad, n_skip;
  wgrp::block_rank(in && st_out == WG_HS_FIN_OK, s_cnt[0], r, n_ok);
  wgrp::block_rank(in && st_out == WG_HS_FIN_NOPENDING, s_cnt[1], r, n_nop);
  wgrp::block_rank(in && st_out == WG_HS_FIN_BADAUTH, s_cnt[2], r, n_bad);
  wgrp::block_rank(in && st_out == WG_HS_FIN_SKIPPED, s_cnt[3], r, n_skip);
  if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4(n_ok, n_nop, n_bad, n_skip);
}

// established[prefix of the range + rank in the range] = the entry of this record; its keys leave the scratch,
// and its pending entry is consumed (nothing reads a pending entry in this launch)
__global__ void __launch_bounds__(256) k_hs_fin_emit(FinParams P) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t nl = fin_len(P);
  if (blockIdx.x * kRankRange >= nl) return;  // (workgroup-uniform)
  const uint32_t k = blockIdx.x * kRankRange + threadIdx.x;
  const bool ok = k < nl && P.fin_status[k] == WG_HS_FIN_OK;
  const uint4 pre = P.part[blockIdx.x];
  uint32_t r, total;
  wgrp::block_rank(ok, s_cnt, r, total);
  if (!ok) return;
  const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
  uint4* in = P.res + (size_t)kEstU4 * k;
  uint4* o = (uint4*)(P.established + (pre.x + r));
  const uint32_t pos = in[0].z;
#pragma unroll
  for (uint32_t g = 0; g < kEstU4; ++g) o[g] = in[g];
#pragma unroll
  for (uint32_t g = 2; g < kEstU4; ++g) in[g] = z4;
  uint4* pe = (uint4*)(P.pending + pos);
#pragma unroll
  for (uint32_t g = 0; g < kPendU4; ++g) pe[g] = z4;
}

}  // namespace wghi

// ---- C ABI --------------------------------------------------------------------------------
extern "C" {

int wg_hs_psks_set(wg_ctx* c, const uint8_t* psks, uint32_t n) {
  if (!c || (!psks && n)) return fail(WG_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const uint32_t have = c->hs ? c->hs->n_peers : 0u;
  if (n != have) return fail(WG_EINVAL, "%u preshared keys for a peer table of %u", n, have);
  if (!n) return WG_OK;
  HsState* t = c->hs;
  HIPTRY(hipDeviceSynchronize());  // no finish queued earlier (on any stream) may still read the old keys
  HIPTRY(hipMemcpyAsync(t->d_ppsk.p, psks, 32ull * n, hipMemcpyHostToDevice, c->stream));
  HIPTRY(hipStreamSynchronize(c->stream));
  return WG_OK;
}

int wg_hs_initiate(wg_ctx* c, const wg_hs_initiate_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  if (b->_reserved) return fail(WG_EINVAL, "wg_hs_initiate_batch._reserved must be 0");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (!c->hs || !c->hs->has_priv) return fail(WG_ENOKEY, "wg_hs_initiate before any wg_hs_static_set");
  HsState* t = c->hs;
  const uint32_t n = b->n;
  if (n == 0) return WG_OK;
  if (n > 0x40000000u) return fail(WG_E2BIG, "handshake initiate of %u entries", n);
  if (!b->peer || (((uintptr_t)b->peer) & 3u) || !b->ephemerals || (((uintptr_t)b->ephemerals) & 15u) || !b->timestamps ||
      (((uintptr_t)b->timestamps) & 3u) || !b->local_index || (((uintptr_t)b->local_index) & 3u))
    return fail(WG_EINVAL, "peer / ephemerals / timestamps / local_index must be non-NULL and aligned (4 / 16 / 4 / 4 bytes)");
  if (!b->status || (((uintptr_t)b->status) & 3u) || !b->records || (((uintptr_t)b->records) & 15u) || !b->pending ||
      (((uintptr_t)b->pending) & 15u) || !b->summary || (((uintptr_t)b->summary) & 7u))
    return fail(WG_EINVAL, "status / records / pending / summary must be non-NULL and aligned (4 / 16 / 16 / 8 bytes)");
  {
    const HsRange out[5] = {{b->ephemerals, 32ull * n},
                            {b->status, 4ull * n},
                            {b->records, sizeof(wg_hs_record) * (uint64_t)n},
                            {b->pending, sizeof(wg_hs_pending) * (uint64_t)n},
                            {b->summary, sizeof(wg_hs_initiate_summary)}};
    const HsRange in[3] = {{b->peer, 4ull * n}, {b->timestamps, 12ull * n}, {b->local_index, 4ull * n}};
    const int ov = hs_ranges_overlap(out, in);
    if (ov == 1) return fail(WG_EINVAL, "ephemerals, status, records, pending and summary must not overlap");
    if (ov == 2) return fail(WG_EINVAL, "an output of wg_hs_initiate must not overlap peer, timestamps or local_index");
  }
  const bool capturing = stream_capturing(s);
  int rc;
  if ((rc = plan_begin(t->order, s, capturing, hs_init_fits(t, n, 0), [&] { return hs_init_grow(t, n, 0); }, kHsInitWords, n)) != WG_OK)
    return rc;
  wghi::InitParams P{};
  P.peer = b->peer;
  P.ephemerals = b->ephemerals;
  P.timestamps = b->timestamps;
  P.local_index = b->local_index;
  P.status = b->status;
  P.records = b->records;
  P.pending = b->pending;
  P.spub = (const uint8_t*)t->d_key.p + 64;
  P.peers = (const HsPeerHdr*)t->d_phdr.p;
  P.lad = (uint4*)t->d_ilad.p;
  P.part = (uint4*)t->d_ipart.p;
  P.n = n;
  const uint32_t nb = rank_blocks(n);
  hipLaunchKernelGGL(wghi::k_hs_init_dh, dim3((uint32_t)((2ull * n + 63u) / 64u)), dim3(64), 0, s, P);
  hipLaunchKernelGGL(wghi::k_hs_init_chain, dim3(nb), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgrp::k_rx_scan, dim3(1), dim3(256), 0, s, P.part, nb, (uint2*)b->summary);
  return plan_end(t->order, s, capturing, kHsInitWords);
}

int wg_hs_finish(wg_ctx* c, const wg_hs_finish_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  if (((uintptr_t)b->n_records) & 3u) return fail(WG_EINVAL, "n_records must be 4-byte aligned");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (!c->hs || !c->hs->has_priv) return fail(WG_ENOKEY, "wg_hs_finish before any wg_hs_static_set");
  HsState* t = c->hs;
  const uint32_t n = b->n, np = b->n_pending;
  if (n == 0) return WG_OK;
  if (n > 0x40000000u) return fail(WG_E2BIG, "handshake finish of %u records", n);
  if (np > 0x10000000u) return fail(WG_E2BIG, "handshake finish against %u pending entries", np);
  if (!b->records || (((uintptr_t)b->records) & 15u) || (np && !b->pending) || (((uintptr_t)b->pending) & 15u))
    return fail(WG_EINVAL, "records / pending must be non-NULL and 16-byte aligned");
  if (!b->fin_status || (((uintptr_t)b->fin_status) & 3u) || !b->established || (((uintptr_t)b->established) & 15u) || !b->summary ||
      (((uintptr_t)b->summary) & 7u))
    return fail(WG_EINVAL, "fin_status / established / summary must be non-NULL and aligned (4 / 16 / 8 bytes)");
  {
    const HsRange out[4] = {{b->pending, sizeof(wg_hs_pending) * (uint64_t)np},
                            {b->fin_status, 4ull * n},
                            {b->established, sizeof(wg_hs_established) * (uint64_t)n},
                            {b->summary, sizeof(wg_hs_finish_summary)}};
    const HsRange in[2] = {{b->records, sizeof(wg_hs_record) * (uint64_t)n}, {b->n_records, b->n_records ? 4u : 0u}};
    const int ov = hs_ranges_overlap(out, in);
    if (ov == 1) return fail(WG_EINVAL, "pending, fin_status, established and summary must not overlap");
    if (ov == 2) return fail(WG_EINVAL, "an output of wg_hs_finish must not overlap records or n_records");
  }
  const bool capturing = stream_capturing(s);
  int rc;
  if ((rc = plan_begin(t->order, s, capturing, hs_init_fits(t, n, np), [&] { return hs_init_grow(t, n, np); }, kHsFinWords, n)) != WG_OK)
    return rc;
  wghi::FinParams P{};
  P.records = b->records;
  P.n_records = b->n_records;
  P.pending = b->pending;
  P.fin_status = b->fin_status;
  P.established = b->established;
  P.priv = (const uint8_t*)t->d_priv.p;
  P.peers = (const HsPeerHdr*)t->d_phdr.p;
  P.psks = (const HsPskHdr*)t->d_pskhdr.p;
  P.tab = (uint32_t*)t->d_ftab.p;
  P.lad = (uint4*)t->d_ilad.p;
  P.res = (uint4*)t->d_fres.p;
  P.part = (uint4*)t->d_ipart.p;
  P.n = n;
  P.n_pending = np;
  P.mask = hs_fin_capacity(np) - 1u;
  hipLaunchKernelGGL(wghi::k_hs_fin_fill, dim3((P.mask + 256u) / 256u), dim3(256), 0, s, P);
  if (np) hipLaunchKernelGGL(wghi::k_hs_fin_insert, dim3(rank_blocks(np)), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wghi::k_hs_fin_dh, dim3((uint32_t)((2ull * n + 63u) / 64u)), dim3(64), 0, s, P);
  rank_launch(wghi::k_hs_fin_chain, wghi::k_hs_fin_emit, P, b->summary, s);
  return plan_end(t->order, s, capturing, kHsFinWords);
}

}  // extern "C"
