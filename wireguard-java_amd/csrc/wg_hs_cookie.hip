// wg_hs_cookie.hip — cookie replies and mac2 under load, on the device (included by wg_capi.hip after
// wg_hs_stamp.hip): wg_hs_cookie_secret_set, wg_hs_admit, wg_hs_cookie_open, wg_hs_cookies_get / _set, wg_hs_mac2.
//
// mac1 needs only our public key: a flood of fresh valid-mac1 initiations costs a ladder and the open chain each.
// WireGuard's cookie makes a sender prove that it receives at its source address before the ladder is spent. The
// reference has no cookies (IncomingInitiation.java:38-40) and wg_hs_check keeps its rule; this file is what the
// library adds, as wg_hs_stamp.hip added the timestamp rule. With MAC(k, m) = BLAKE2s-128 keyed with k:
//   Kc(P) = H("cookie--" || P)       cookie(src) = MAC(secret, addr || port)       mac2 = MAC(cookie, msg[0 .. L - 16))
//   reply = {3, 0,0,0, receiver, nonce[24], XAEAD(Kc(S_pub of the replier), nonce, cookie, aad = the message's mac1)}
// XAEAD is XChaCha20-Poly1305 (draft-irtf-cfrg-xchacha-03): sub = HChaCha20(K, nonce[0 .. 16)), then the AEAD of
// RFC 8439 under sub with the nonce 0^4 || nonce[16 .. 24). HChaCha20 (wgd::hchacha20) is chacha20_block's rounds over
// {constants, K, nonce16} without the final addition; the AEAD's blocks are wgd::chacha20_block with a non-zero
// nonce, and its Poly1305 (one aad block, one ciphertext block, the lengths) is poly_tag16, a sibling of
// wghc::poly_tag, whose aad is 32 bytes.
//
// wg_hs_admit: wg_hs_check's three launches with a second rank. k_hs_admit runs steps 1-4 as k_hs_check does, then,
// in the lanes whose mac1 verified (public), the cookie of the lane's source address (2 compressions) and the mac2
// under it (1 + 3 for an initiation, 1 + 2 for a response), and leaves two 16-B records per range of 256 positions:
// {valid, init, resp, rejected} and {replies, mac2_ok, nononce, badsrc}. k_rx_scan runs once over each row.
// k_hs_admit_emit places the records (hs_put_record, k_hs_emit's) and, in the NEEDCOOKIE lanes, computes the cookie
// again (it never lies in memory), seals it, writes the reply and zeroes the nonce it used.
//
// wg_hs_cookie_open: wg_hs_finish's table of pending positions (k_hs_fin_fill, k_hs_fin_insert, fin_lookup, as they
// are), then one datagram per lane: Kc of the peer (one compression), the XAEAD open against the mac1 of the
// initiation we sent. An opened cookie goes to scratch and the lane's batch index into its peer's `sel` word with an
// atomicMin; one launch later (after the scan) the lane whose index stands there stores the cookie, sets sel back
// to ~0 and so leaves the table as every call expects it. The scratch's cookies are zeroed by the emit.
//
// wg_hs_mac2: one record per lane, MAC(the peer's cookie, msg[0 .. L - 16)) into the record's last 16 bytes.
//
// Constant time: no branch, address or loop bound depends on the secret, a cookie, a cookie key, a subkey or a
// keystream byte, except the all-zero test of the raw nonce. Source addresses, indices, peer positions, `have` and
// the statuses are public.
#pragma once

namespace {

const PlanWords kHsAdmitWords{"handshake admit", "datagrams", "wg_hs_reserve"};
const PlanWords kHsCkOpenWords{"cookie open", "datagrams", "wg_hs_reserve"};
const PlanWords kHsMac2Words{"handshake mac2", "records", "wg_hs_reserve"};

static_assert(sizeof(HsCookie) == 32, "a peer's cookie entry is two uint4");
static_assert(sizeof(wg_hs_src) == 24 && sizeof(wg_hs_cookie_reply) == 80 && sizeof(wg_hs_learned) == 16, "wgaead.h layouts");

}  // namespace

// ---- device -------------------------------------------------------------------------------
namespace wgck {

constexpr uint32_t kReplyU4 = 5;  // a wg_hs_cookie_reply

struct AdmitParams {
  wghs::HsParams H;  // as k_hs_check takes it; H.part is the first row of counts
  const wg_hs_src* src;
  uint8_t* nonces;
  wg_hs_cookie_reply* replies;
  const uint8_t* kc;      // Kc(local static public key), 32 B (fixed address)
  const uint8_t* secret;  // 32 B (fixed address)
  uint4* part2;           // the second row of counts
};

struct CkOpenParams {
  wghi::FinParams F;  // pending, n_pending, peers, tab, mask: what the lookup reads
  const uint8_t* wire;
  uint64_t wire_size;
  const uint64_t* pkt_off;
  const uint32_t* pkt_len;
  const wg_hs_record* sent;
  uint32_t* ck_status;
  wg_hs_learned* learned;
  const HsCookieHdr* cookies;
  uint4* res;  // per datagram: the opened cookie, {pending position, peer, 0, 0}
  uint4* part;
  uint32_t n;
};

struct Mac2Params {
  wg_hs_record* records;
  const uint32_t* peer;
  uint32_t* mac2_status;
  const HsCookieHdr* cookies;
  uint4* part;
  uint32_t n;
};

// tag = Poly1305(aad (16) || ct (16) || LE64(16) || LE64(16)) under the one-time key ks[0 .. 8): three Horner steps
__device__ __forceinline__ void poly_tag16(const uint32_t ks[16], const uint32_t aad[4], const uint32_t ct[4], uint32_t tag[4]) {
  uint32_t r[5], s5[5], h[5] = {0u, 0u, 0u, 0u, 0u}, c[5];
  wgd::poly_r_limbs(ks[0], ks[1], ks[2], ks[3], r);
  wgd::poly_scale5(r, s5);
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    if (b == 0) wgd::poly_block_limbs(aad[0], aad[1], aad[2], aad[3], 1u << 24, c);
    else if (b == 1) wgd::poly_block_limbs(ct[0], ct[1], ct[2], ct[3], 1u << 24, c);
    else wgd::poly_block_limbs(16u, 0u, 16u, 0u, 1u << 24, c);
#pragma unroll
    for (int j = 0; j < 5; ++j) h[j] += c[j];
    wgd::poly_mul<false>(h, r, s5);
  }
  wgd::poly_finish(h, ks[4], ks[5], ks[6], ks[7], tag);
}

// out[0 .. 4) = the 16 bytes `in` xored with the keystream of the XAEAD under (key, nonce24), tag = the tag over
// (aad, the ciphertext): seal (ct = out) or open (ct = in), by `open`, which is a compile-time constant at each call
template <bool OPEN>
__device__ __forceinline__ void xaead16(const uint32_t key[8], const uint32_t nonce[6], const uint32_t aad[4], const uint32_t in[4],
                                        uint32_t out[4], uint32_t tag[4]) {
  uint32_t sub[8], ks[16];
  wgd::hchacha20(key, nonce, sub);
  wgd::chacha20_block(sub, 1u, 0u, nonce[4], nonce[5], ks);
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = in[j] ^ ks[j];
  wgd::chacha20_block(sub, 0u, 0u, nonce[4], nonce[5], ks);
  poly_tag16(ks, aad, OPEN ? in : out, tag);
}

// h = the BLAKE2s-128 state of msg[0 .. len) (len > 0) under the key kw (its words, zeros behind its keylen bytes)
__device__ __forceinline__ void mac_keyed(const uint8_t* msg, uint32_t len, const uint32_t kw[8], uint32_t keylen, uint32_t h[8]) {
  uint32_t m[16];
  wghs::b2s_init(h, 16u, keylen);
  wghc::msg32(m, kw);
  wghs::b2s_compress(h, m, 64u, false);
  const uint32_t nb = (len + 63u) >> 6;
  for (uint32_t b = 0; b < nb; ++b) {  // (len is public: 132, 76)
    const uint32_t off = 64u * b, left = len - off, avail = left < 64u ? left : 64u;
    wghs::b2s_load(msg + off, avail, m);
    wghs::b2s_compress(h, m, 64u + off + avail, b + 1u == nb);
  }
}

// ck = cookie(src) = MAC(secret, addr || port): a0 .. a3 the address words, pf = port | family << 16 (bytes 16 .. 20 of
// a wg_hs_src). family (4 or 6) is public.
__device__ __forceinline__ void cookie_of(const uint8_t* secret, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t pf,
                                          uint32_t ck[4]) {
  const uint4* sp = (const uint4*)secret;
  uint32_t kw[8], m[16], h[8];
  wghc::put8(kw, sp[0], sp[1]);
  wghs::b2s_init(h, 16u, 32u);
  wghc::msg32(m, kw);
  wghs::b2s_compress(h, m, 64u, false);
  const bool v4 = ((pf >> 16) & 0xFFu) == 4u;
  const uint32_t port = pf & 0xFFFFu;
#pragma unroll
  for (int j = 0; j < 16; ++j) m[j] = 0u;
  m[0] = a0;
  m[1] = v4 ? port : a1;
  m[2] = v4 ? 0u : a2;
  m[3] = v4 ? 0u : a3;
  m[4] = v4 ? 0u : port;
  wghs::b2s_compress(h, m, v4 ? 70u : 82u, true);
#pragma unroll
  for (int j = 0; j < 4; ++j) ck[j] = h[j];
}

// the source of batch index i: its address words and port | family << 16
__device__ __forceinline__ void src_of(const wg_hs_src* src, uint32_t i, uint32_t a[4], uint32_t& pf) {
  const uint2* q = (const uint2*)(src + i);
  const uint2 q0 = q[0], q1 = q[1], q2 = q[2];
  a[0] = q0.x; a[1] = q0.y; a[2] = q1.x; a[3] = q1.y;
  pf = q2.x;
}

// ---- wg_hs_admit ---------------------------------------------------------------------------

// steps 1-8 of wg_hs_admit for one list position per thread; the range's two rows of counts
__global__ void __launch_bounds__(256) k_hs_admit(AdmitParams A) {
  __shared__ uint32_t s_cnt[7][4];
  const wghs::HsParams& P = A.H;
  const uint32_t nl = wghs::hs_list_len(P);
  if (blockIdx.x * kRankRange >= nl) {  // past the list (workgroup-uniform): zero records for the scans
    if (threadIdx.x == 0) {
      P.part[blockIdx.x] = make_uint4(0u, 0u, 0u, 0u);
      A.part2[blockIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    }
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
      wghs::b2s_hash(msg, L - 32u, P.key, 32u, 16u, h);
      uint32_t diff = 0;  // all 16 bytes, no early exit
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) diff |= wgt::load_u32_any(msg + L - 32u + 4u * j) ^ h[j];
      st = WG_HS_BADMAC1;
      if (!diff) {  // (public) the flood's lanes stop here
        uint32_t a[4], pf;
        src_of(A.src, i, a, pf);
        const uint32_t fam = (pf >> 16) & 0xFFu;
        st = WG_HS_BADSRC;
        if (fam == 4u || fam == 6u) {
          uint32_t kw[8];
          cookie_of(A.secret, a[0], a[1], a[2], a[3], pf, kw);
          kw[4] = kw[5] = kw[6] = kw[7] = 0u;
          mac_keyed(msg, L - 16u, kw, 16u, h);
          uint32_t d2 = 0;
#pragma unroll
          for (uint32_t j = 0; j < 4; ++j) d2 |= wgt::load_u32_any(msg + L - 16u + 4u * j) ^ h[j];
          if (!d2) {
            st = WG_HS_OK;
          } else {
            const uint2* nq = (const uint2*)(A.nonces + 24ull * k);
            const uint2 n0 = nq[0], n1 = nq[1], n2 = nq[2];
            st = (n0.x | n0.y | n1.x | n1.y | n2.x | n2.y) ? WG_HS_NEEDCOOKIE : WG_HS_NONONCE;
          }
        }
      }
    }
    P.hs_status[k] = st;
  }
  const bool ok = in && st == WG_HS_OK;
  uint32_t r, n_valid, n_init, n_resp, n_rej, n_rep, n_non, n_bsrc;
  wgrp::block_rank(ok, s_cnt[0], r, n_valid);
  wgrp::block_rank(ok && t == 1u, s_cnt[1], r, n_init);
  wgrp::block_rank(ok && t == 2u, s_cnt[2], r, n_resp);
  wgrp::block_rank(in && !ok, s_cnt[3], r, n_rej);
  wgrp::block_rank(in && st == WG_HS_NEEDCOOKIE, s_cnt[4], r, n_rep);
  wgrp::block_rank(in && st == WG_HS_NONONCE, s_cnt[5], r, n_non);
  wgrp::block_rank(in && st == WG_HS_BADSRC, s_cnt[6], r, n_bsrc);
  if (threadIdx.x == 0) {
    P.part[blockIdx.x] = make_uint4(n_valid, n_init, n_resp, n_rej);
    A.part2[blockIdx.x] = make_uint4(n_rep, n_valid, n_non, n_bsrc);
  }
}

// records[...] = the accepted message of this list position; replies[...] = the sealed cookie of a NEEDCOOKIE one,
// whose nonce is zeroed
__global__ void __launch_bounds__(256) k_hs_admit_emit(AdmitParams A) {
  __shared__ uint32_t s_cnt[2][4];
  const wghs::HsParams& P = A.H;
  const uint32_t nl = wghs::hs_list_len(P);
  if (blockIdx.x * kRankRange >= nl) return;  // (workgroup-uniform)
  const uint32_t k = blockIdx.x * kRankRange + threadIdx.x;
  const uint32_t st = k < nl ? P.hs_status[k] : WG_HS_BADLEN;
  const bool ok = st == WG_HS_OK, need = st == WG_HS_NEEDCOOKIE;
  const uint4 pre = P.part[blockIdx.x], pre2 = A.part2[blockIdx.x];
  uint32_t r, r2, total;
  wgrp::block_rank(ok, s_cnt[0], r, total);
  wgrp::block_rank(need, s_cnt[1], r2, total);
  if (ok) hs_put_record(P, k, pre.x + r);
  if (!need) return;
  const uint32_t i = P.list ? P.list[k] : k;
  const uint8_t* msg = P.wire + P.pkt_off[i];
  const uint32_t L = msg[0] == 1u ? 148u : 92u;
  uint32_t a[4], pf, ck[4], aad[4], nonce[6], kc[8], ct[4], tag[4];
  src_of(A.src, i, a, pf);
  cookie_of(A.secret, a[0], a[1], a[2], a[3], pf, ck);
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) aad[j] = wgt::load_u32_any(msg + L - 32u + 4u * j);
  uint2* nq = (uint2*)(A.nonces + 24ull * k);
  const uint2 n0 = nq[0], n1 = nq[1], n2 = nq[2];
  nonce[0] = n0.x; nonce[1] = n0.y; nonce[2] = n1.x; nonce[3] = n1.y; nonce[4] = n2.x; nonce[5] = n2.y;
  const uint4* kq = (const uint4*)A.kc;
  wghc::put8(kc, kq[0], kq[1]);
  xaead16<false>(kc, nonce, aad, ck, ct, tag);
  uint4* o = (uint4*)(A.replies + (pre2.x + r2));
  o[0] = make_uint4(i, WG_HS_COOKIE_SIZE, 3u, wgt::load_u32_any(msg + 4));
  o[1] = make_uint4(nonce[0], nonce[1], nonce[2], nonce[3]);
  o[2] = make_uint4(nonce[4], nonce[5], ct[0], ct[1]);
  o[3] = make_uint4(ct[2], ct[3], tag[0], tag[1]);
  o[4] = make_uint4(tag[2], tag[3], 0u, 0u);
  const uint2 z2 = make_uint2(0u, 0u);  // the nonce is spent
  nq[0] = z2;
  nq[1] = z2;
  nq[2] = z2;
}

// ---- wg_hs_cookie_open -----------------------------------------------------------------------

// steps 1-6 of wg_hs_cookie_open for one datagram per thread; an opened cookie to scratch, the lane's batch index
// into its peer's selection word; the range's counts
__global__ void __launch_bounds__(256) k_hs_ck_open(CkOpenParams P) {
  __shared__ uint32_t s_cnt[4][4];
  const uint32_t i = blockIdx.x * kRankRange + threadIdx.x;
  const bool in = i < P.n;
  uint32_t st = WG_HS_CK_BADLEN;
  if (in) {
    const uint64_t o = P.pkt_off[i];
    const uint32_t wl = P.pkt_len[i];
    uint32_t pos = 0;
    const uint8_t* msg = P.wire;
    if (wl != 0 && o <= P.wire_size && (uint64_t)wl <= P.wire_size - o) {
      msg = P.wire + o;
      if (msg[0] != 3u) st = WG_HS_CK_SKIPPED;
      else if (wl == WG_HS_COOKIE_SIZE) {
        pos = wghi::fin_lookup(P.F, wgt::load_u32_any(msg + 4));
        // (a live entry's peer is below the peer table's count, which is the cookie table's unless that one could not
        // be allocated: then nobody is waiting)
        st = pos && ((const uint4*)(P.F.pending + (pos - 1u)))[0].y < P.cookies->count ? WG_HS_CK_OK : WG_HS_CK_NOPENDING;
      }
    }
    if (st == WG_HS_CK_OK) {  // (public)
      const HsPeerHdr H = *P.F.peers;
      const uint32_t peer = ((const uint4*)(P.F.pending + (pos - 1u)))[0].y;  // a live entry's: below the table's count
      // Kc = H("cookie--" || S_r): 40 bytes
      const uint4* sr = (const uint4*)(H.publics + 32ull * peer);
      uint32_t m[16], kc[8], w[8];
      wghc::put8(w, sr[0], sr[1]);
      m[0] = 0x6B6F6F63u;  // "cook"
      m[1] = 0x2D2D6569u;  // "ie--"
      wghc::set8(m + 2, w);
#pragma unroll
      for (int j = 10; j < 16; ++j) m[j] = 0u;
      wghs::b2s_init(kc, 32u, 0u);
      wghs::b2s_compress(kc, m, 40u, true);
      // the mac1 of what we sent: msg[116 .. 132), words 31 .. 35 of the record
      const uint32_t* sw = (const uint32_t*)(P.sent + (pos - 1u));
      uint32_t aad[4], nonce[6], ct[4], pt[4], tag[4];
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) aad[j] = sw[31u + j];
#pragma unroll
      for (uint32_t j = 0; j < 6; ++j) nonce[j] = wgt::load_u32_any(msg + 8u + 4u * j);
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) ct[j] = wgt::load_u32_any(msg + 32u + 4u * j);
      xaead16<true>(kc, nonce, aad, ct, pt, tag);
      uint32_t diff = 0;  // all 16 bytes, no early exit
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) diff |= wgt::load_u32_any(msg + 48u + 4u * j) ^ tag[j];
      if (diff) {
        st = WG_HS_CK_BADAUTH;
      } else {
        P.res[2ull * i] = make_uint4(pt[0], pt[1], pt[2], pt[3]);
        P.res[2ull * i + 1u] = make_uint4(pos - 1u, peer, 0u, 0u);
        (void)atomicMin(&P.cookies->entries[peer].sel, i);
      }
    }
    P.ck_status[i] = st;
  }
  uint32_t r, n_ok, n_nop, n_bad, n_skip;
  wgrp::block_rank(in && st == WG_HS_CK_OK, s_cnt[0], r, n_ok);
  wgrp::block_rank(in && st == WG_HS_CK_NOPENDING, s_cnt[1], r, n_nop);
  wgrp::block_rank(in && st == WG_HS_CK_BADAUTH, s_cnt[2], r, n_bad);
  wgrp::block_rank(in && st == WG_HS_CK_SKIPPED, s_cnt[3], r, n_skip);
  if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4(n_ok, n_nop, n_bad, n_skip);
}

// learned[prefix of the range + rank in the range] = this OK datagram; the lane that its peer's selection word names
// stores the cookie and sets the word back; the cookie leaves the scratch
__global__ void __launch_bounds__(256) k_hs_ck_emit(CkOpenParams P) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t i = blockIdx.x * kRankRange + threadIdx.x;
  const bool ok = i < P.n && P.ck_status[i] == WG_HS_CK_OK;
  const uint4 pre = P.part[blockIdx.x];
  uint32_t r, total;
  wgrp::block_rank(ok, s_cnt, r, total);
  if (!ok) return;
  const uint4 cookie = P.res[2ull * i], w = P.res[2ull * i + 1u];  // w = {pending position, peer, 0, 0}
  ((uint4*)P.learned)[pre.x + r] = make_uint4(i, w.x, w.y, 0u);
  P.res[2ull * i] = make_uint4(0u, 0u, 0u, 0u);
  uint4* e = (uint4*)(P.cookies->entries + w.y);
  if (e[1].y == i) {  // (the others of this peer read i's index or ~0 here: neither is theirs)
    e[0] = cookie;
    e[1] = make_uint4(1u, 0xFFFFFFFFu, 0u, 0u);
  }
}

// ---- wg_hs_mac2 ----------------------------------------------------------------------------

// one record per thread: its status, and mac2 under its peer's cookie; the range's counts
__global__ void __launch_bounds__(256) k_hs_mac2(Mac2Params P) {
  __shared__ uint32_t s_cnt[3][4];
  const uint32_t k = blockIdx.x * kRankRange + threadIdx.x;
  const bool in = k < P.n;
  uint32_t st = WG_HS_MAC2_BADDESC;
  if (in) {
    uint32_t* rec = (uint32_t*)(P.records + k);
    const uint32_t L = rec[1];
    if (L == WG_HS_INIT_SIZE || L == WG_HS_RESP_SIZE) {
      const HsCookieHdr C = *P.cookies;
      const uint32_t peer = P.peer[k];
      if (peer >= C.count) {
        st = WG_HS_MAC2_BADPEER;
      } else {
        const uint4* e = (const uint4*)(C.entries + peer);
        if (!e[1].x) {
          st = WG_HS_MAC2_NONE;
        } else {
          st = WG_HS_MAC2_OK;
          const uint4 ck = e[0];
          uint32_t kw[8] = {ck.x, ck.y, ck.z, ck.w, 0u, 0u, 0u, 0u}, h[8];
          mac_keyed((const uint8_t*)(rec + 2), L - 16u, kw, 16u, h);
          uint32_t* o = rec + 2u + ((L - 16u) >> 2);
#pragma unroll
          for (uint32_t j = 0; j < 4; ++j) o[j] = h[j];
        }
      }
    }
    P.mac2_status[k] = st;
  }
  uint32_t r, n_ok, n_none, n_bad;
  wgrp::block_rank(in && st == WG_HS_MAC2_OK, s_cnt[0], r, n_ok);
  wgrp::block_rank(in && st == WG_HS_MAC2_NONE, s_cnt[1], r, n_none);
  wgrp::block_rank(in && (st == WG_HS_MAC2_BADDESC || st == WG_HS_MAC2_BADPEER), s_cnt[2], r, n_bad);
  if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4(n_ok, n_none, n_bad, 0u);
}

}  // namespace wgck

// ---- C ABI --------------------------------------------------------------------------------
namespace {

// wg_hs_peers_set's part of this file: a cookie entry per peer of the new table, all empty, behind the header.
// Caller holds c->mu and has synchronised the device.
int hs_cookie_peers_reset(wg_ctx* c, HsState* t) {
  if (t->d_cook.p) HIPTRY(hipMemset(t->d_cook.p, 0, t->d_cook.cap));  // (it may be freed below: wiped first)
  HsCookieHdr C{};
  C.entries = (HsCookie*)t->d_pempty.p;
  int rc = WG_OK;
  if (t->n_peers && (rc = t->d_cook.ensure(sizeof(HsCookie) * (size_t)t->n_peers)) == WG_OK) {
    HsCookie empty{};
    empty.sel = 0xFFFFFFFFu;
    const std::vector<HsCookie> v(t->n_peers, empty);
    HIPTRY(hipMemcpyAsync(t->d_cook.p, v.data(), sizeof(HsCookie) * v.size(), hipMemcpyHostToDevice, c->stream));
    HIPTRY(hipStreamSynchronize(c->stream));
    C.entries = (HsCookie*)t->d_cook.p;
    C.count = t->n_peers;
  }
  HIPTRY(hipMemcpyAsync(t->d_chdr.p, &C, sizeof C, hipMemcpyHostToDevice, c->stream));
  HIPTRY(hipStreamSynchronize(c->stream));
  return rc;
}

// the peers' range [first, first + n) of wg_hs_cookies_set / _get. Caller holds c->mu.
int hs_cookie_range(wg_ctx* c, uint32_t first, uint32_t n, const void* cookies, const void* have, HsState** out) {
  if ((!cookies || !have) && n) return fail(WG_EINVAL, "NULL argument");
  HsState* t;
  int rc;
  if ((rc = hs_get(c, &t)) != WG_OK) return rc;
  if ((uint64_t)first + n > t->n_peers) return fail(WG_ERANGE, "cookies [%u, %u + %u) of a peer table of %u", first, first, n, t->n_peers);
  *out = t;
  return WG_OK;
}

}  // namespace

extern "C" {

int wg_hs_cookie_secret_set(wg_ctx* c, const uint8_t* secret) {
  if (!c || !secret) return fail(WG_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HsState* t;
  int rc;
  if ((rc = hs_get(c, &t)) != WG_OK) return rc;
  HIPTRY(hipDeviceSynchronize());  // no admit queued earlier (on any stream) may still read the old secret
  HIPTRY(hipMemcpyAsync((uint8_t*)t->d_key.p + 128, secret, 32, hipMemcpyHostToDevice, c->stream));
  HIPTRY(hipStreamSynchronize(c->stream));
  t->has_secret = true;
  return WG_OK;
}

int wg_hs_cookies_set(wg_ctx* c, uint32_t first_peer, uint32_t n, const uint8_t* cookies, const uint8_t* have) {
  if (!c) return fail(WG_EINVAL, "NULL context");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HsState* t;
  int rc;
  if ((rc = hs_cookie_range(c, first_peer, n, cookies, have, &t)) != WG_OK || !n) return rc;
  std::vector<HsCookie> v(n);
  for (uint32_t k = 0; k < n; ++k) {
    v[k] = HsCookie{};
    v[k].sel = 0xFFFFFFFFu;
    if (have[k]) {
      memcpy(v[k].cookie, cookies + 16ull * k, 16);
      v[k].have = 1u;
    }
  }
  HIPTRY(hipDeviceSynchronize());  // nothing queued earlier (on any stream) may still read or write the old entries
  const hipError_t e = hipMemcpyAsync((HsCookie*)t->d_cook.p + first_peer, v.data(), sizeof(HsCookie) * (size_t)n, hipMemcpyHostToDevice, c->stream);
  const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(c->stream) : e;
  memset((void*)v.data(), 0, sizeof(HsCookie) * (size_t)n);
  HIPTRY(e2);
  return WG_OK;
}

int wg_hs_cookies_get(wg_ctx* c, uint32_t first_peer, uint32_t n, uint8_t* cookies, uint8_t* have) {
  if (!c) return fail(WG_EINVAL, "NULL context");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HsState* t;
  int rc;
  if ((rc = hs_cookie_range(c, first_peer, n, cookies, have, &t)) != WG_OK || !n) return rc;
  std::vector<HsCookie> v(n);
  HIPTRY(hipDeviceSynchronize());  // every cookie_open queued earlier (on any stream) has stored its cookies
  HIPTRY(hipMemcpyAsync(v.data(), (const HsCookie*)t->d_cook.p + first_peer, sizeof(HsCookie) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPTRY(hipStreamSynchronize(c->stream));
  for (uint32_t k = 0; k < n; ++k) {
    memcpy(cookies + 16ull * k, v[k].cookie, 16);
    have[k] = v[k].have ? 1 : 0;
  }
  memset((void*)v.data(), 0, sizeof(HsCookie) * (size_t)n);
  return WG_OK;
}

int wg_hs_admit(wg_ctx* c, const wg_hs_admit_batch* a, void* stream) {
  if (!c || !a) return fail(WG_EINVAL, "NULL argument");
  const wg_hs_batch* b = &a->hs;
  if (b->_reserved) return fail(WG_EINVAL, "wg_hs_batch._reserved must be 0");
  if (!b->summary || (((uintptr_t)b->summary) & 7u) || !a->admit_summary || (((uintptr_t)a->admit_summary) & 7u))
    return fail(WG_EINVAL, "summary and admit_summary must be non-NULL and 8-byte aligned");
  if ((b->list == nullptr) != (b->n_list == nullptr))
    return fail(WG_EINVAL, "list and n_list go together: both NULL (every datagram) or both set");
  if ((((uintptr_t)b->list) & 3u) || (((uintptr_t)b->n_list) & 3u)) return fail(WG_EINVAL, "list and n_list must be 4-byte aligned");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (!c->hs || !c->hs->has_key) return fail(WG_ENOKEY, "wg_hs_admit before any wg_hs_key_set");
  if (!c->hs->has_secret) return fail(WG_ENOKEY, "wg_hs_admit before any wg_hs_cookie_secret_set");
  HsState* t = c->hs;
  const bool capturing = stream_capturing(s);
  const uint32_t n = b->n;
  if (n == 0) {
    HIPTRY(hipMemsetAsync(b->summary, 0, sizeof(wg_hs_summary), s));
    HIPTRY(hipMemsetAsync(a->admit_summary, 0, sizeof(wg_hs_admit_summary), s));
    return WG_OK;
  }
  if (!b->wire || !b->pkt_off || !b->pkt_len) return fail(WG_EINVAL, "NULL wire ring or packet table");
  if (!b->hs_status || (((uintptr_t)b->hs_status) & 3u) || !b->records || (((uintptr_t)b->records) & 15u))
    return fail(WG_EINVAL, "status / record output must be non-NULL and aligned (4 / 16 bytes)");
  if (!a->src || (((uintptr_t)a->src) & 7u) || !a->nonces || (((uintptr_t)a->nonces) & 15u) || !a->replies || (((uintptr_t)a->replies) & 15u))
    return fail(WG_EINVAL, "src / nonces / replies must be non-NULL and aligned (8 / 16 / 16 bytes)");
  {
    const HsRange out[6] = {{b->hs_status, 4ull * n},
                            {b->records, sizeof(wg_hs_record) * (uint64_t)n},
                            {b->summary, sizeof(wg_hs_summary)},
                            {a->nonces, 24ull * n},
                            {a->replies, sizeof(wg_hs_cookie_reply) * (uint64_t)n},
                            {a->admit_summary, sizeof(wg_hs_admit_summary)}};
    const HsRange in[6] = {{b->wire, b->wire_size}, {b->pkt_off, 8ull * n}, {b->pkt_len, 4ull * n},
                           {b->list, b->list ? 4ull * n : 0u}, {b->n_list, b->n_list ? 4u : 0u}, {a->src, sizeof(wg_hs_src) * (uint64_t)n}};
    const int ov = hs_ranges_overlap(out, in);
    if (ov == 1) return fail(WG_EINVAL, "hs_status, records, summary, nonces, replies and admit_summary must not overlap");
    if (ov == 2) return fail(WG_EINVAL, "an output of wg_hs_admit must not overlap the ring, the packet table, the list or src");
  }
  int rc;
  if ((rc = hs_begin(t, s, capturing, n, false, kHsAdmitWords)) != WG_OK) return rc;
  const uint32_t nb = rank_blocks(n);
  wgck::AdmitParams P{};
  P.H.wire = b->wire;
  P.H.wire_size = b->wire_size;
  P.H.pkt_off = b->pkt_off;
  P.H.pkt_len = b->pkt_len;
  P.H.list = b->list;
  P.H.n_list = b->n_list;
  P.H.hs_status = b->hs_status;
  P.H.records = b->records;
  P.H.key = (const uint8_t*)t->d_key.p;
  P.H.part = (uint4*)t->d_part.p;
  P.H.n = n;
  P.src = a->src;
  P.nonces = a->nonces;
  P.replies = a->replies;
  P.kc = (const uint8_t*)t->d_key.p + 96;
  P.secret = (const uint8_t*)t->d_key.p + 128;
  P.part2 = P.H.part + nb;
  hipLaunchKernelGGL(wgck::k_hs_admit, dim3(nb), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgrp::k_rx_scan, dim3(1), dim3(256), 0, s, P.H.part, nb, (uint2*)b->summary);
  hipLaunchKernelGGL(wgrp::k_rx_scan, dim3(1), dim3(256), 0, s, P.part2, nb, (uint2*)a->admit_summary);
  hipLaunchKernelGGL(wgck::k_hs_admit_emit, dim3(nb), dim3(256), 0, s, P);
  return plan_end(t->order, s, capturing, kHsAdmitWords);
}

int wg_hs_cookie_open(wg_ctx* c, const wg_hs_cookie_open_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (!c->hs || !c->hs->has_priv) return fail(WG_ENOKEY, "wg_hs_cookie_open before any wg_hs_static_set");
  HsState* t = c->hs;
  const uint32_t n = b->n, np = b->n_pending;
  if (n == 0) return WG_OK;
  if (n > 0x40000000u) return fail(WG_E2BIG, "cookie open of %u datagrams", n);
  if (np > 0x10000000u) return fail(WG_E2BIG, "cookie open against %u pending entries", np);
  if (!b->wire || !b->pkt_off || !b->pkt_len) return fail(WG_EINVAL, "NULL wire ring or packet table");
  if ((np && (!b->pending || !b->sent)) || (((uintptr_t)b->pending) & 15u) || (((uintptr_t)b->sent) & 15u))
    return fail(WG_EINVAL, "sent / pending must be non-NULL and 16-byte aligned");
  if (!b->ck_status || (((uintptr_t)b->ck_status) & 3u) || !b->learned || (((uintptr_t)b->learned) & 15u) || !b->summary ||
      (((uintptr_t)b->summary) & 7u))
    return fail(WG_EINVAL, "ck_status / learned / summary must be non-NULL and aligned (4 / 16 / 8 bytes)");
  {
    const HsRange out[3] = {{b->ck_status, 4ull * n}, {b->learned, sizeof(wg_hs_learned) * (uint64_t)n}, {b->summary, sizeof(wg_hs_cookie_open_summary)}};
    const HsRange in[5] = {{b->wire, b->wire_size}, {b->pkt_off, 8ull * n}, {b->pkt_len, 4ull * n},
                           {b->sent, sizeof(wg_hs_record) * (uint64_t)np}, {b->pending, sizeof(wg_hs_pending) * (uint64_t)np}};
    const int ov = hs_ranges_overlap(out, in);
    if (ov == 1) return fail(WG_EINVAL, "ck_status, learned and summary must not overlap");
    if (ov == 2) return fail(WG_EINVAL, "an output of wg_hs_cookie_open must not overlap the ring, the packet table, sent or pending");
  }
  const bool capturing = stream_capturing(s);
  int rc;
  if ((rc = plan_begin(t->order, s, capturing, hs_init_fits(t, n, np), [&] { return hs_init_grow(t, n, np); }, kHsCkOpenWords, n)) != WG_OK)
    return rc;
  wgck::CkOpenParams P{};
  P.F.pending = const_cast<wg_hs_pending*>(b->pending);  // (the table's kernels only read it)
  P.F.peers = (const HsPeerHdr*)t->d_phdr.p;
  P.F.tab = (uint32_t*)t->d_ftab.p;
  P.F.n_pending = np;
  P.F.mask = hs_fin_capacity(np) - 1u;
  P.wire = b->wire;
  P.wire_size = b->wire_size;
  P.pkt_off = b->pkt_off;
  P.pkt_len = b->pkt_len;
  P.sent = b->sent;
  P.ck_status = b->ck_status;
  P.learned = b->learned;
  P.cookies = (const HsCookieHdr*)t->d_chdr.p;
  P.res = (uint4*)t->d_fres.p;
  P.part = (uint4*)t->d_ipart.p;
  P.n = n;
  hipLaunchKernelGGL(wghi::k_hs_fin_fill, dim3((P.F.mask + 256u) / 256u), dim3(256), 0, s, P.F);
  if (np) hipLaunchKernelGGL(wghi::k_hs_fin_insert, dim3(rank_blocks(np)), dim3(256), 0, s, P.F);
  rank_launch(wgck::k_hs_ck_open, wgck::k_hs_ck_emit, P, b->summary, s);
  return plan_end(t->order, s, capturing, kHsCkOpenWords);
}

int wg_hs_mac2(wg_ctx* c, const wg_hs_mac2_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  if (b->_reserved) return fail(WG_EINVAL, "wg_hs_mac2_batch._reserved must be 0");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HsState* t;
  int rc;
  const uint32_t n = b->n;
  if (n == 0) return WG_OK;
  if (n > 0x40000000u) return fail(WG_E2BIG, "handshake mac2 of %u records", n);
  if (!b->records || (((uintptr_t)b->records) & 15u) || !b->peer || (((uintptr_t)b->peer) & 3u) || !b->mac2_status ||
      (((uintptr_t)b->mac2_status) & 3u) || !b->summary || (((uintptr_t)b->summary) & 7u))
    return fail(WG_EINVAL, "records / peer / mac2_status / summary must be non-NULL and aligned (16 / 4 / 4 / 8 bytes)");
  {
    const HsRange out[3] = {{b->records, sizeof(wg_hs_record) * (uint64_t)n}, {b->mac2_status, 4ull * n}, {b->summary, sizeof(wg_hs_mac2_summary)}};
    const HsRange in[1] = {{b->peer, 4ull * n}};
    const int ov = hs_ranges_overlap(out, in);
    if (ov == 1) return fail(WG_EINVAL, "records, mac2_status and summary must not overlap");
    if (ov == 2) return fail(WG_EINVAL, "an output of wg_hs_mac2 must not overlap peer");
  }
  const bool capturing = stream_capturing(s);
  if (capturing && !c->hs) return fail(WG_EINVAL, "the first wg_hs_* call of a context on a capturing stream");
  if ((rc = hs_get(c, &t)) != WG_OK) return rc;
  if ((rc = plan_begin(t->order, s, capturing, hs_init_fits(t, n, 0), [&] { return hs_init_grow(t, n, 0); }, kHsMac2Words, n)) != WG_OK)
    return rc;
  wgck::Mac2Params P{};
  P.records = b->records;
  P.peer = b->peer;
  P.mac2_status = b->mac2_status;
  P.cookies = (const HsCookieHdr*)t->d_chdr.p;
  P.part = (uint4*)t->d_ipart.p;
  P.n = n;
  const uint32_t nb = rank_blocks(n);
  hipLaunchKernelGGL(wgck::k_hs_mac2, dim3(nb), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgrp::k_rx_scan, dim3(1), dim3(256), 0, s, P.part, nb, (uint2*)b->summary);
  return plan_end(t->order, s, capturing, kHsMac2Words);
}

}  // extern "C"
