// wg_hs_open.hip — the initiations' encrypted static, opened on the device (included by wg_capi.hip after
// wg_hs_chain.hip).
//
// wg_hs_check admits a handshake message on its mac1, which needs only the local static PUBLIC key; wg_hs_dh
// spends a ladder on each admitted initiation. The first test that only a holder of a private key passes comes
// after both: Handshakes.decryptRemoteStatic (Handshakes.java:201-237, called per initiation from
// PeerList.java:80 and SessionManager.java:212) runs the Noise IK hash chain, three HKDFs over HMAC-BLAKE2s
// (Crypto.java:39-99) and the ChaCha20-Poly1305 open of encrypted_static. wg_hs_open is that step over
// wg_hs_check's records and wg_hs_dh's secrets, with the peer lookup behind it and the compaction of what
// survives: the host receives authenticated initiations, by peer, with the Noise state the responder goes on
// from.
//
// The chain (H = BLAKE2s-256, KDFn = Crypto.deriveKey(salt, ikm, n), ss = wg_hs_dh's 32 bytes; state.chainKey
// and the local chainKey are one array, Handshakes.java:203 and :314-316, so this is the ordinary IK chain):
//   h = H(H(H0 || S_pub) || E)                 ck = KDF1(CK0, E)
//   k = KDF2(ck, ss)                           ck = KDF1(ck, ss)
//   remote_static = AEAD-open(k, nonce 0, aad = h, encrypted_static)
//   h = H(h || encrypted_static)
//   known peer: ck = KDF1(ck, X25519(S_priv, remote_static))
//   h = H(h || encrypted_timestamp)            (the reference never opens the timestamp: :233-234)
//
// k_hs_open: one record per lane, 28 BLAKE2s compressions in a row, each taking the one before it. An HMAC
// is four compressions (the two key blocks K ^ 0x36.., K ^ 0x5c.. as words, never bytes; the message; the
// inner digest); with CK0 as the key the two key-block states are the constants below, and KDF2 / KDF1 of one
// salt and ikm share the extract, the key-block states of the expand and T1. The compressions are the steps
// of kOpenProgram (wg_hs_chain.h), written once in the order of the chain above, and run by the machine of
// wg_hs_chain.hip: ONE loop around ONE b2s_compress, in which the step's word names its source, its
// operation and its destination. 28 inlined copies would be some 200 KB of straight-line code that every
// wave streams through the instruction cache once; the loop stays there. The step counter is uniform, so
// the switches are scalar branches and nothing is indexed dynamically. What this kernel adds to the generic
// operations: its sources (the record's ephemeral, ss, the peer's static-static secret), H(H(H0 || S_pub)
// || E), the two blocks of H(h || encrypted_static), H(h || encrypted_timestamp) and "ck if the lane has a
// peer". The AEAD sits in front of the first block of H(h || encrypted_static) (OP_ES1), its key being the
// T2 that the step before left in the state: two register chacha20_blocks (counter 0: the Poly1305 key;
// counter 1: the 32 bytes), wghc::poly_tag over aad (32) || ct (32) || LE64(32) || LE64(32), the tag compared
// in all 16 bytes. Then the probe, for the authentic lanes only; a wave without a known peer jumps over the
// static-static KDF, the eight steps [kOpenStaticBegin, kOpenStaticEnd) that the header finds in the program.
//
// Constant time: no branch, address or loop bound depends on ss, on a derived key or on the static-static
// secret. The program is public and indexed by a public counter. The branches depend on the program, the
// record's length, the statuses, the tag comparison's outcome and the decrypted static key of an authentic
// message (the probe); the static-static secret's ADDRESS depends on which peer it is, not on its value.
//
// Peers. wg_hs_peers_set keeps the peers' static public keys on the device, each peer's X25519(S_priv, peer)
// beside them (one k_x25519 launch), and an open-addressing table over them in wg_rx_sessions_set's manner:
// capacity = the smallest power of two >= max(16, 4 n), 4-byte entries (peer + 1; 0: empty), bucket =
// mix32(w0 ^ mix32(w1)) & mask over the key's first two words, linear probing, a hit confirmed on all 32
// bytes. Its header sits at a fixed device address (wg_plan.hip, fixed headers).
//
// Ranks. inits[0 .. n_emitted) is the stable compaction of the OK and NEWPEER records, in the three launches
// of wg_hs_check: k_hs_open leaves the lane's results in scratch and one 16-B record {emitted, known, badauth,
// skipped} per 256 records, k_rx_scan (as it is) turns them into prefixes and the summary, k_hs_open_emit
// places. No workgroup waits on another; every scratch word is written before it is read in each call.
#pragma once

namespace wgho {

// CK0 = BLAKE2s-256("Noise_IKpsk2_25519_ChaChaPoly_BLAKE2s") = 60e26dae...8b78cd36 and H0 = BLAKE2s-256(CK0 ||
// "WireGuard v1 zx2c4 Jason@zx2c4.com") = 2211b361...ba079ef3 (Handshakes.java:20-37). kCk0Ipad / kCk0Opad:
// the BLAKE2s-256 state after the one block CK0 ^ 0x36.. / CK0 ^ 0x5c.. (t = 64, not last): where every
// HMAC keyed with CK0 starts its inner and outer hash.
__device__ constexpr uint32_t kCk0Ipad[8] = {0x312A9144u, 0xFDD38461u, 0x04BC8B11u, 0x3EE8BD1Eu,
                                             0xF33DD3B5u, 0xCCBC984Fu, 0x85D7DA2Cu, 0xAAF184E1u};
__device__ constexpr uint32_t kCk0Opad[8] = {0x852E4FFCu, 0x77D1B8E9u, 0x04AC82BAu, 0x3F84C25Bu,
                                             0xB4A948DAu, 0x6008756Bu, 0xB06E5F22u, 0xD0A63DB8u};

constexpr uint32_t kOpenResU4 = 7;  // scratch per record, in uint4: remote_static, hash, chain_key, {peer, 0, 0, 0}

struct OpenParams {
  const wg_hs_record* records;
  const uint32_t* n_records;
  const uint8_t* shared;
  const uint32_t* dh_status;
  uint32_t* open_status;
  wg_hs_init* inits;
  const uint8_t* hs0;  // H(H0 || S_pub), 32 B (fixed address)
  const HsPeerHdr* peers;
  uint4* res;
  uint4* part;
  uint32_t n;
};

__device__ __forceinline__ uint32_t open_len(const OpenParams& P) { return wgrp::dev_count(P.n_records, P.n); }

// peer + 1 of a static public key, 0 if the table does not hold it
__device__ __forceinline__ uint32_t hs_peer(const HsPeerHdr& H, const uint32_t w[8]) {
  uint32_t b = hs_peer_bucket(w[0], w[1]);
  for (uint32_t probes = 0; probes <= H.mask; ++probes, ++b) {  // (a table a quarter full ends the walk long before)
    const uint32_t e = H.slots[b & H.mask];
    if (!e) return 0u;
    const uint4* p = (const uint4*)(H.publics + 32ull * (e - 1u));
    const uint4 x = p[0], y = p[1];
    const uint32_t diff = (x.x ^ w[0]) | (x.y ^ w[1]) | (x.z ^ w[2]) | (x.w ^ w[3]) | (y.x ^ w[4]) | (y.y ^ w[5]) |
                          (y.z ^ w[6]) | (y.w ^ w[7]);
    if (!diff) return e;
  }
  return 0u;
}

// remote_static = ct ^ keystream when Poly1305(aad || ct || lengths) under `key`, nonce 0, equals the tag;
// returns the OR of the tag's differences (0: authentic). es = encrypted_static as 12 words.
__device__ __forceinline__ uint32_t open_static(const uint32_t key[8], const uint32_t aad[8], const uint32_t es[12],
                                                uint32_t rs[8]) {
  uint32_t ks[16];
  wgd::chacha20_block(key, 0u, 0u, 0u, 0u, ks);
  uint32_t tag[4];
  wghc::poly_tag<2>(ks, aad, es, tag);
  const uint32_t diff = (tag[0] ^ es[8]) | (tag[1] ^ es[9]) | (tag[2] ^ es[10]) | (tag[3] ^ es[11]);  // all 16 bytes
  wgd::chacha20_block(key, 1u, 0u, 0u, 0u, ks);
#pragma unroll
  for (int j = 0; j < 8; ++j) rs[j] = es[j] ^ ks[j];
  return diff;
}

// One record per lane: status, and for an authentic one its results to scratch; the range's counts.
__global__ void __launch_bounds__(256) k_hs_open(OpenParams P) {
  __shared__ uint32_t s_cnt[4][4];
  const uint32_t nl = open_len(P);
  if (blockIdx.x * kRankRange >= nl) {  // past the records (workgroup-uniform): a zero record for the scan
    if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const uint32_t k = blockIdx.x * kRankRange + threadIdx.x;
  const bool in = k < nl;
  uint32_t st_out = WG_HS_OPEN_BADDESC;
  if ((k & ~63u) < nl) {  // (wave-uniform: a wave wholly past the records goes straight to the counts)
    // a lane past the records, and one whose record is not opened, runs the chain over record 0 and stores nothing
    const uint32_t kk = in ? k : 0u;
    const uint4* rec = (const uint4*)(P.records + kk);
    const uint4* shr = (const uint4*)(P.shared + 32ull * kk);
    bool go = false;
    if (in) {
      const uint32_t len = rec[0].y, ds = P.dh_status[k];
      if (len == WG_HS_RESP_SIZE) st_out = WG_HS_OPEN_SKIPPED;
      else if (len != WG_HS_INIT_SIZE) st_out = WG_HS_OPEN_BADDESC;
      else if (ds == WG_X25519_SKIPPED) st_out = WG_HS_OPEN_SKIPPED;
      else if (ds != WG_X25519_OK && ds != WG_X25519_ZERO) st_out = WG_HS_OPEN_BADDESC;
      else go = true;
    }
    const HsPeerHdr H = *P.peers;
    using namespace wghc;
    Chain c;
    clear(c);
    set8(c.ist, kCk0Ipad);  // KDF1(CK0, E) starts from the constant key-block states
    set8(c.ost, kCk0Opad);
    uint32_t peer = 0;     // peer + 1 of an authentic lane with a known static key
    bool auth = false;
    bool any_known = false;
    Step s = fetch(kOpenProgram, 0u);
#pragma unroll 1
    for (uint32_t step = 0; step < kOpenSteps;) {
      uint32_t src[8];
      switch (s.arg) {
        case SRC_E: put8(src, rec[1], rec[2]); break;
        case SRC_SS: put8(src, shr[0], shr[1]); break;
        case SRC_STATIC: {  // (a lane without a peer: zeros, and the result is dropped)
          uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
          if (peer) {
            const uint4* q = (const uint4*)(H.secrets + 32ull * (peer - 1u));
            a = q[0];
            b = q[1];
          }
          put8(src, a, b);
          break;
        }
        default: source(c, s.arg, src); break;
      }
      switch (s.op) {
        case OP_H0: {  // h = H(H(H0 || S_pub) || E)
          const uint4* q = (const uint4*)P.hs0;
          put8(c.m, q[0], q[1]);
          put8(c.m + 8, rec[1], rec[2]);
          wghs::b2s_init(c.st, 32u, 0u);
          c.t = 64u; c.last = true;
          break;
        }
        case OP_ES1: {  // st = T2 = the key: open encrypted_static; then h = H(h || encrypted_static), first block
          uint32_t es[12], rs[8];
          put8(es, rec[3], rec[4]);
          const uint4 tg = rec[5];
          es[8] = tg.x; es[9] = tg.y; es[10] = tg.z; es[11] = tg.w;
          const uint32_t diff = open_static(c.st, c.hh, es, rs);
          auth = go && diff == 0u;
          if (auth) {
            peer = hs_peer(H, rs);
            uint4* o = P.res + (size_t)kOpenResU4 * k;
            o[0] = make_uint4(rs[0], rs[1], rs[2], rs[3]);
            o[1] = make_uint4(rs[4], rs[5], rs[6], rs[7]);
          }
          any_known = __ballot(peer != 0u) != 0ull;
          set8(c.m, c.hh);
          set8(c.m + 8, es);
          wghs::b2s_init(c.st, 32u, 0u);
          c.t = 64u; c.last = false;
          break;
        }
        case OP_ES2: {  // ... second block: the tag
          const uint4 tg = rec[5];
          c.m[0] = tg.x; c.m[1] = tg.y; c.m[2] = tg.z; c.m[3] = tg.w;
#pragma unroll
          for (int j = 4; j < 16; ++j) c.m[j] = 0u;
          c.t = 80u; c.last = true;
          break;
        }
        case OP_TS: {  // h = H(h || encrypted_timestamp), 60 bytes
          const uint4 a = rec[6], b = rec[7];
          set8(c.m, c.hh);
          c.m[8] = a.x; c.m[9] = a.y; c.m[10] = a.z; c.m[11] = a.w; c.m[12] = b.x; c.m[13] = b.y; c.m[14] = b.z; c.m[15] = 0u;
          wghs::b2s_init(c.st, 32u, 0u);
          c.t = 60u; c.last = true;
          break;
        }
        default: prepare(c, s, src); break;
      }
      uint32_t next = step + 1u;
      if (next == kOpenStaticBegin && !any_known) next = kOpenStaticEnd;  // (wave-uniform) no static-static KDF to run
      const Step ahead = fetch(kOpenProgram, next);
      wghs::b2s_compress(c.st, c.m, c.t, c.last);
      switch (s.dst) {
        case DST_CK_IF_PEER:
#pragma unroll
          for (int j = 0; j < 8; ++j) c.ck[j] = peer ? c.st[j] : c.ck[j];
          break;
        default: WG_HSC_PUT(c, s.dst); break;
      }
      s = ahead;
      step = next;
    }
    if (auth) {
      uint4* o = P.res + (size_t)kOpenResU4 * k;
      o[2] = make_uint4(c.hh[0], c.hh[1], c.hh[2], c.hh[3]);
      o[3] = make_uint4(c.hh[4], c.hh[5], c.hh[6], c.hh[7]);
      o[4] = make_uint4(c.ck[0], c.ck[1], c.ck[2], c.ck[3]);
      o[5] = make_uint4(c.ck[4], c.ck[5], c.ck[6], c.ck[7]);
      o[6] = make_uint4(peer ? peer - 1u : WG_HS_NOPEER, 0u, 0u, 0u);
    }
    if (go) st_out = auth ? (peer ? WG_HS_OPEN_OK : WG_HS_OPEN_NEWPEER) : WG_HS_OPEN_BADAUTH;
    if (in) P.open_status[k] = st_out;
  }
  uint32_t r, n_emit, n_known, n_bad, n_skip;
  wgrp::block_rank(in && (st_out == WG_HS_OPEN_OK || st_out == WG_HS_OPEN_NEWPEER), s_cnt[0], r, n_emit);
  wgrp::block_rank(in && st_out == WG_HS_OPEN_OK, s_cnt[1], r, n_known);
  wgrp::block_rank(in && st_out == WG_HS_OPEN_BADAUTH, s_cnt[2], r, n_bad);
  wgrp::block_rank(in && st_out == WG_HS_OPEN_SKIPPED, s_cnt[3], r, n_skip);
  if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4(n_emit, n_known, n_bad, n_skip);
}

// inits[prefix of the range + rank in the range] = the authentic initiation of this record
__global__ void __launch_bounds__(256) k_hs_open_emit(OpenParams P) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t nl = open_len(P);
  if (blockIdx.x * kRankRange >= nl) return;  // (workgroup-uniform)
  const uint32_t k = blockIdx.x * kRankRange + threadIdx.x;
  bool ok = false;
  if (k < nl) {
    const uint32_t s = P.open_status[k];
    ok = s == WG_HS_OPEN_OK || s == WG_HS_OPEN_NEWPEER;
  }
  const uint4 pre = P.part[blockIdx.x];
  uint32_t r, total;
  wgrp::block_rank(ok, s_cnt, r, total);
  if (!ok) return;
  const uint4* rec = (const uint4*)(P.records + k);
  const uint4* in = P.res + (size_t)kOpenResU4 * k;
  uint4* o = (uint4*)(P.inits + (pre.x + r));
  const uint4 r0 = rec[0];  // {index, len, msg[0 .. 4), msg[4 .. 8) = the sender index}
  o[0] = make_uint4(r0.x, k, r0.w, in[6].x);
  o[1] = rec[1];  // msg[8 .. 40): the ephemeral
  o[2] = rec[2];
#pragma unroll
  for (uint32_t g = 0; g < 6; ++g) o[3 + g] = in[g];
}

}  // namespace wgho

// ---- C ABI --------------------------------------------------------------------------------
namespace {

// Each stored peer's X25519(S_priv, peer) into d_psec, in one k_x25519 launch over the descriptors that
// wg_hs_peers_set left. Caller holds c->mu and has synchronised the device.
int hs_peer_secrets(wg_ctx* c, HsState* t) {
  if (!t->n_peers) return WG_OK;
  const uint32_t n = t->n_peers;
  uint8_t* pin = (uint8_t*)t->d_pin.p;  // [0, 32) the private key for the time of the launch, then the publics
  HIPTRY(hipMemcpyAsync(pin, t->d_priv.p, 32, hipMemcpyDeviceToDevice, c->stream));
  int rc = x25519_launch((const wg_x25519_desc*)t->d_pdesc.p, n, pin, 32ull + 32ull * n, (uint8_t*)t->d_psec.p, 32ull * n,
                         (uint32_t*)((uint8_t*)t->d_pdesc.p + 32ull * n), c->stream);
  hipError_t e = hipMemsetAsync(pin, 0, 32, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (rc != WG_OK) return rc;
  if (e != hipSuccess) return fail(WG_EDEVICE, "peer secrets: %s", hipGetErrorString(e));
  return WG_OK;
}

// wg_hs_static_set's part of this stage: H(H0 || S_pub) beside the mac1 key, and the stored peers' secrets
// under the new private key. Caller holds c->mu.
int hs_open_rekey(wg_ctx* c, HsState* t, const uint8_t* static_public) {
  static const uint8_t kH0[32] = {0x22, 0x11, 0xb3, 0x61, 0x08, 0x1a, 0xc5, 0x66, 0x69, 0x12, 0x43, 0xdb, 0x45, 0x8a, 0xd5, 0x32,
                                  0x2d, 0x9c, 0x6c, 0x66, 0x22, 0x93, 0xe8, 0xb7, 0x0e, 0xe1, 0x9c, 0x65, 0xba, 0x07, 0x9e, 0xf3};
  // stage: [256, 288) the descriptor, [288, 352) H0 || public key (Handshakes.java:205), [352, 356) status
  uint8_t host[128] = {0};
  wg_b2s_desc d{};
  d.in_off = 32;
  d.len = 64;
  d.outlen = 32;
  memcpy(host, &d, sizeof d);
  memcpy(host + 32, kH0, 32);
  memcpy(host + 64, static_public, 32);
  HIPTRY(hipDeviceSynchronize());  // no open queued earlier (on any stream) may still read the old values
  uint8_t* st = (uint8_t*)t->d_stage.p + 256;
  HIPTRY(hipMemcpyAsync(st, host, sizeof host, hipMemcpyHostToDevice, c->stream));
  HIPTRY(hipMemcpyAsync((uint8_t*)t->d_key.p + 64, host + 64, 32, hipMemcpyHostToDevice, c->stream));  // S_pub, for wg_hs_initiate
  int rc;
  if ((rc = b2s_launch((const wg_b2s_desc*)st, 1, st, 128, (uint8_t*)t->d_key.p + 32, 32, (uint32_t*)(st + 96), c->stream)) != WG_OK)
    return rc;
  HIPTRY(hipStreamSynchronize(c->stream));
  return hs_peer_secrets(c, t);
}

}  // namespace

extern "C" {

int wg_hs_peers_set(wg_ctx* c, const uint8_t* publics, uint32_t n) {
  if (!c || (!publics && n)) return fail(WG_EINVAL, "NULL argument");
  if (n > 0x02000000u) return fail(WG_E2BIG, "peer table of %u entries", n);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (!c->hs || !c->hs->has_priv) return fail(WG_ENOKEY, "wg_hs_peers_set before any wg_hs_static_set");
  HsState* t = c->hs;
  HsPeerHdr H{};
  uint32_t cap = 16;
  while ((uint64_t)cap < 4ull * n) cap <<= 1;
  H.mask = cap - 1u;
  H.count = n;
  std::vector<uint32_t> slots(n ? cap : 0, 0u);
  std::vector<wg_x25519_desc> desc(n);
  for (uint32_t k = 0; k < n; ++k) {
    const uint8_t* p = publics + 32ull * k;
    uint32_t w[2];
    memcpy(w, p, 8);
    uint32_t b = hs_peer_bucket(w[0], w[1]) & H.mask;
    while (slots[b]) {
      if (!memcmp(publics + 32ull * (slots[b] - 1u), p, 32)) return fail(WG_EINVAL, "peer %u: its static key repeats peer %u's", k, slots[b] - 1u);
      b = (b + 1u) & H.mask;
    }
    slots[b] = k + 1u;
    desc[k] = wg_x25519_desc{};
    desc[k].point_off = 32ull + 32ull * k;
    desc[k].out_off = 32ull * k;
  }
  HIPTRY(hipDeviceSynchronize());  // the table may move: no open launched earlier (on any stream) may still read it
  int rc = WG_OK;
  if (t->d_psec.p && t->d_psec.cap < 32ull * n) HIPTRY(hipMemset(t->d_psec.p, 0, t->d_psec.cap));  // freed below: wiped first
  t->n_peers = 0;
  if (t->d_ppsk.p) HIPTRY(hipMemset(t->d_ppsk.p, 0, t->d_ppsk.cap));  // every psk is zero again (and the buffer may be freed below)
  if (n) {
    if ((rc = t->d_pslots.ensure(slots.size() * 4)) == WG_OK && (rc = t->d_pin.ensure(32ull + 32ull * n)) == WG_OK &&
        (rc = t->d_psec.ensure(32ull * n)) == WG_OK && (rc = t->d_pdesc.ensure(36ull * n)) == WG_OK &&
        (rc = t->d_ppsk.ensure(32ull * n)) == WG_OK) {
      hipError_t e = hipMemsetAsync(t->d_ppsk.p, 0, t->d_ppsk.cap, c->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(t->d_pslots.p, slots.data(), slots.size() * 4, hipMemcpyHostToDevice, c->stream);
      if (e == hipSuccess) e = hipMemcpyAsync((uint8_t*)t->d_pin.p + 32, publics, 32ull * n, hipMemcpyHostToDevice, c->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(t->d_pdesc.p, desc.data(), 32ull * n, hipMemcpyHostToDevice, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess) rc = fail(WG_EDEVICE, "peer table: %s", hipGetErrorString(e));
      if (rc == WG_OK) {
        t->n_peers = n;
        if ((rc = hs_peer_secrets(c, t)) != WG_OK) t->n_peers = 0;
      }
    }
  }
  if (t->n_peers) {
    H.slots = (const uint32_t*)t->d_pslots.p;
    H.publics = (const uint8_t*)t->d_pin.p + 32;
    H.secrets = (const uint8_t*)t->d_psec.p;
  } else {  // n = 0, or a failure that may have dropped the old table: no peers
    H.slots = (const uint32_t*)t->d_pempty.p;
    H.mask = 15u;
    H.count = 0;
  }
  HsPskHdr K{};
  K.psks = (const uint8_t*)(t->n_peers ? t->d_ppsk.p : t->d_pempty.p);
  K.count = t->n_peers;
  HIPTRY(hipMemcpyAsync(t->d_phdr.p, &H, sizeof H, hipMemcpyHostToDevice, c->stream));
  HIPTRY(hipMemcpyAsync(t->d_pskhdr.p, &K, sizeof K, hipMemcpyHostToDevice, c->stream));
  HIPTRY(hipStreamSynchronize(c->stream));
  if (t->has_stamps) {  // positions are renumbered: every stored timestamp is zero again
    const int src = hs_stamp_peers_reset(c, t);
    if (rc == WG_OK) rc = src;
  }
  const int crc = hs_cookie_peers_reset(c, t);  // ... and every cookie is forgotten
  return rc != WG_OK ? rc : crc;
}

int wg_hs_open(wg_ctx* c, const wg_hs_open_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  if (b->_reserved) return fail(WG_EINVAL, "wg_hs_open_batch._reserved must be 0");
  if (((uintptr_t)b->n_records) & 3u) return fail(WG_EINVAL, "n_records must be 4-byte aligned");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (!c->hs || !c->hs->has_priv) return fail(WG_ENOKEY, "wg_hs_open before any wg_hs_static_set");
  HsState* t = c->hs;
  const uint32_t n = b->n;
  if (n == 0) return WG_OK;
  if (!b->records || (((uintptr_t)b->records) & 15u) || !b->shared || (((uintptr_t)b->shared) & 15u) || !b->dh_status ||
      (((uintptr_t)b->dh_status) & 3u))
    return fail(WG_EINVAL, "records / shared / dh_status must be non-NULL and aligned (16 / 16 / 4 bytes)");
  if (!b->open_status || (((uintptr_t)b->open_status) & 3u) || !b->inits || (((uintptr_t)b->inits) & 15u) || !b->summary ||
      (((uintptr_t)b->summary) & 7u))
    return fail(WG_EINVAL, "open_status / inits / summary must be non-NULL and aligned (4 / 16 / 8 bytes)");
  {
    const HsRange out[3] = {{b->open_status, 4ull * n}, {b->inits, sizeof(wg_hs_init) * (uint64_t)n}, {b->summary, sizeof(wg_hs_open_summary)}};
    const HsRange in[4] = {{b->records, sizeof(wg_hs_record) * (uint64_t)n}, {b->shared, 32ull * n}, {b->dh_status, 4ull * n},
                           {b->n_records, b->n_records ? 4u : 0u}};
    const int ov = hs_ranges_overlap(out, in);
    if (ov == 1) return fail(WG_EINVAL, "open_status, inits and summary must not overlap");
    if (ov == 2) return fail(WG_EINVAL, "an output of wg_hs_open must not overlap records, shared, dh_status or n_records");
  }
  const bool capturing = stream_capturing(s);
  int rc;
  if ((rc = hs_begin(t, s, capturing, n, true, kHsOpenWords)) != WG_OK) return rc;
  wgho::OpenParams P{};
  P.records = b->records;
  P.n_records = b->n_records;
  P.shared = b->shared;
  P.dh_status = b->dh_status;
  P.open_status = b->open_status;
  P.inits = b->inits;
  P.hs0 = (const uint8_t*)t->d_key.p + 32;
  P.peers = (const HsPeerHdr*)t->d_phdr.p;
  P.res = (uint4*)t->d_ores.p;
  P.part = (uint4*)t->d_opart.p;
  P.n = n;
  rank_launch(wgho::k_hs_open, wgho::k_hs_open_emit, P, b->summary, s);
  return plan_end(t->order, s, capturing, kHsOpenWords);
}

}  // extern "C"
