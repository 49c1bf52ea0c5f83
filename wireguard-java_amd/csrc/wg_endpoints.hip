// wg_endpoints.hip — where a sealed datagram goes, on the device (included by wg_capi.hip).
//
// The reference gives every session one address, EstablishedSession.outboundPacketAddress: a responder's session gets
// the initiation's origin (SessionManager.java:217-229), an initiator's the configured endpoint (:186, :196), and
// nothing moves it afterwards. WireGuard additionally moves a peer's endpoint to the source of every authenticated
// packet. Here a peer's endpoint is one normalised 24-byte wg_hs_src of a per-peer table, a key slot's peer one word of
// a per-key-slot map, and both sit at fixed device addresses:
//   wg_endpoints_start  behind wg_hs_install: the installed sessions' slots -> peer (wg_session.hip's `installed`), and
//                       the peer's endpoint from the handshake datagram's source.
//   wg_endpoints_learn  behind wg_rx_deliver: roaming; the last authenticated packet of a peer in the ring wins.
//   wg_tx_sendlist      the transmit twin of wg_rx_deliver's items: {wire offset, length, destination} per sealed
//                       datagram, and the gate that refuses a descriptor whose peer has no endpoint.
//   wg_hs_sendlist      the same items for responses, initiations and cookie replies.
// Nothing per packet crosses to the host: it walks `items` with sendmmsg.
//
// No thread order. Of several sessions of one peer in one start the lowest entry gives the endpoint (atomicMin on the
// peer's claim word, read behind a kernel boundary); of a peer's packets in one learn the highest batch index
// (atomicMax). The lists are rank_launch-shaped stable compactions (wg_plan.hip).
#pragma once

namespace {

constexpr uint32_t kEpItems = 1u << 22;  // descriptors per call the reserve sizes the rank scratch for
static_assert(WG_PKT_NOENDPOINT == 12u && sizeof(wg_hs_src) == 24 && sizeof(wg_tx_item) == 48, "endpoint ABI");

struct EndpointsState {
  DevBuf d_ep;     // max_peers x wg_hs_src, normalised (family 0: none)
  DevBuf d_map;    // key_slots x the slot's peer
  DevBuf d_claim;  // start / learn: per peer, the entry or packet that gives the endpoint
  DevBuf d_code;   // learn: per peer {seen, roamed}
  DevBuf d_ctl;    // learn: {n_authentic, n_badsrc}
  DevBuf d_part;   // per range {bytes lo, bytes hi, count, count}, then their prefixes; behind them the totals
  uint32_t max_peers = 0;
  StreamOrder order;  // last start / learn / sendlist / setter
};

const PlanWords kEpStartWords{"endpoints start", "entries", "wg_endpoints_reserve"};
const PlanWords kEpLearnWords{"endpoints learn", "packets", "wg_endpoints_reserve"};
const PlanWords kEpSendWords{"send list", "descriptors", "wg_endpoints_reserve"};

void ep_free(wg_ctx* c) {
  delete c->ep;
  c->ep = nullptr;
}

bool ep_scratch_fits(const EndpointsState* t, uint32_t n) { return ((size_t)rank_blocks(n) + 1u) * 16 <= t->d_part.cap; }

// before a send list of n items on stream s: the rank scratch (it grows on a stream that is not capturing) and the order
int ep_send_begin(EndpointsState* t, hipStream_t s, bool capturing, uint32_t n) {
  const bool fits = ep_scratch_fits(t, n);
  if (capturing && !fits)
    return fail(WG_EINVAL, "send list of %u descriptors on a capturing stream needs more scratch than wg_endpoints_reserve sized (%u): run one call of that size outside the capture first",
                n, kEpItems);
  return plan_begin(t->order, s, capturing, fits, [&] { return t->d_part.ensure(((size_t)rank_blocks(n) + 1u) * 16); }, kEpSendWords, n);
}

// the stored form: IPv4 keeps addr[4 .. 16) zero, _pad is zero, no endpoint is 24 zero bytes
void ep_normalise(wg_hs_src* e) {
  memset(e->_pad, 0, sizeof e->_pad);
  if (e->family == 4) memset(e->addr + 4, 0, 12);
  if (e->family == 0) memset(e, 0, sizeof *e);
}

}  // namespace

// ---- device -------------------------------------------------------------------------------
namespace wgep {

struct EpTables {
  uint64_t* ep;   // 3 words per peer
  uint32_t* map;
  uint32_t K, max_peers;
};

struct EpAddr {
  uint64_t a, b, c;  // addr[0 .. 8), addr[8 .. 16), {port, family, _pad}
};

__device__ __forceinline__ uint32_t ep_family(uint64_t c) { return (uint32_t)(c >> 16) & 0xFFu; }

// the normalised form of *s; false if its family is neither 4 nor 6
__device__ __forceinline__ bool ep_norm(const wg_hs_src* s, EpAddr& o) {
  const uint64_t* w = (const uint64_t*)s;
  o.a = w[0];
  o.b = w[1];
  o.c = w[2] & 0xFFFFFFull;
  const uint32_t fam = ep_family(o.c);
  if (fam == 4u) {
    o.a &= 0xFFFFFFFFull;
    o.b = 0ull;
  }
  return fam == 4u || fam == 6u;
}

__device__ __forceinline__ EpAddr ep_load(const EpTables& T, uint32_t peer) {
  const uint64_t* w = T.ep + (size_t)peer * 3u;
  return EpAddr{w[0], w[1], w[2]};
}

__device__ __forceinline__ void ep_store(const EpTables& T, uint32_t peer, const EpAddr& v) {
  uint64_t* w = T.ep + (size_t)peer * 3u;
  w[0] = v.a;
  w[1] = v.b;
  w[2] = v.c;
}

// a 48-byte wg_tx_item
__device__ __forceinline__ void ep_item(wg_tx_item* it, uint64_t off, uint32_t len, uint32_t slot, uint32_t peer, uint32_t index,
                                        const EpAddr& dst) {
  uint4* o = (uint4*)it;
  o[0] = make_uint4((uint32_t)off, (uint32_t)(off >> 32), len, slot);
  o[1] = make_uint4(peer, index, (uint32_t)dst.a, (uint32_t)(dst.a >> 32));
  o[2] = make_uint4((uint32_t)dst.b, (uint32_t)(dst.b >> 32), (uint32_t)dst.c, (uint32_t)(dst.c >> 32));
}

// ---- start ----
struct EpStartParams {
  EpTables T;
  InstView V;
  const uint32_t* status;
  const wg_hs_src* src;
  uint32_t* claim;
  uint32_t* summary;
  uint32_t n_src, learn;
};

__global__ void __launch_bounds__(256) k_ep_start_map(EpStartParams P) {
  __shared__ uint32_t s_cnt[2][4];
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  uint32_t s, r, peer = 0;
  const bool ok = installed(P.V, P.status, P.T.K, P.T.max_peers, j, s, r, peer);
  if (ok) {
    P.T.map[s] = peer;
    P.T.map[r] = peer;
    if (P.learn && peer != WG_HS_NOPEER) (void)atomicMin(P.claim + peer, j);
  }
  uint32_t rk, n_sessions, n_nopeer;
  wgrp::block_rank(ok, s_cnt[0], rk, n_sessions);
  wgrp::block_rank(ok && peer == WG_HS_NOPEER, s_cnt[1], rk, n_nopeer);
  if (threadIdx.x == 0) {
    if (n_sessions) atomicAdd(P.summary, n_sessions);
    if (n_nopeer) atomicAdd(P.summary + 3, n_nopeer);
  }
}

__global__ void __launch_bounds__(256) k_ep_start_write(EpStartParams P) {
  __shared__ uint32_t s_cnt[2][4];
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  uint32_t s, r, peer;
  bool learned = false, bad = false;
  if (installed(P.V, P.status, P.T.K, P.T.max_peers, j, s, r, peer) && peer != WG_HS_NOPEER) {
    const uint32_t index = inst_entry(P.V, j)[0];  // the datagram's batch index: the first word of both entry formats
    EpAddr a;
    if (index < P.n_src && ep_norm(P.src + index, a)) {
      if (P.claim[peer] == j) {
        ep_store(P.T, peer, a);
        learned = true;
      }
    } else {
      bad = true;
    }
  }
  uint32_t rk, n_learned, n_bad;
  wgrp::block_rank(learned, s_cnt[0], rk, n_learned);
  wgrp::block_rank(bad, s_cnt[1], rk, n_bad);
  if (threadIdx.x == 0) {
    if (n_learned) atomicAdd(P.summary + 1, n_learned);
    if (n_bad) atomicAdd(P.summary + 2, n_bad);
  }
}

// ---- learn ----
struct EpLearnParams {
  EpTables T;
  const wg_pkt* desc;
  const uint32_t* status;
  const wg_hs_src* src;
  uint32_t* roamed;
  uint32_t* summary;
  uint32_t* claim;
  uint32_t* code;
  uint32_t* ctl;
  uint4* part;
  const uint4* tot;  // = part + ranges: the totals, written by k_rx_scan
  uint32_t n, cap;
};

__global__ void __launch_bounds__(256) k_ep_learn_fill(EpLearnParams P) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < P.T.max_peers) P.claim[i] = 0u;
  if (i < 2u) P.ctl[i] = 0u;
}

// claim[p] = 1 + the highest batch index among p's qualifying packets
__global__ void __launch_bounds__(256) k_ep_learn_claim(EpLearnParams P) {
  __shared__ uint32_t s_cnt[2][4];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool q = false, bad = false;
  uint32_t p = 0;
  if (i < P.n) {
    const uint32_t st = P.status[i];
    if (st == WG_PKT_OK || st == WG_PKT_KEEPALIVE) {
      const uint32_t slot = ((const uint32_t*)(P.desc + i))[7];
      if (slot < P.T.K) {
        p = P.T.map[slot];
        if (p < P.T.max_peers) {
          const uint32_t fam = ep_family(((const uint64_t*)(P.src + i))[2]);
          q = fam == 4u || fam == 6u;
          bad = !q;
        }
      }
    }
  }
  // Where every qualifying packet of a wave belongs to one peer (a ring from one peer), the wave's last qualifying
  // lane, which holds its highest index, claims for all 64: one atomic per wave. A lane that finds the word past its
  // index issues none.
  {
    bool for_all;
    const bool mine = wgrp::wave_elect<true>(q, p, for_all);
    if (mine && __hip_atomic_load(P.claim + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < i + 1u) (void)atomicMax(P.claim + p, i + 1u);
  }
  uint32_t r, n_q, n_bad;
  wgrp::block_rank(q, s_cnt[0], r, n_q);
  wgrp::block_rank(bad, s_cnt[1], r, n_bad);
  if (threadIdx.x == 0) {
    if (n_q) atomicAdd(P.ctl, n_q);
    if (n_bad) atomicAdd(P.ctl + 1, n_bad);
  }
}

// peer g, by the one thread that owns its record: the winner against the stored endpoint
__global__ void __launch_bounds__(256) k_ep_learn_judge(EpLearnParams P) {
  __shared__ uint32_t s_cnt[2][4];
  const uint32_t g = blockIdx.x * kRankRange + threadIdx.x;
  uint32_t code = 0;
  if (g < P.T.max_peers) {
    const uint32_t c = P.claim[g];
    if (c) {
      code = 1u;
      EpAddr a;
      (void)ep_norm(P.src + (c - 1u), a);  // (c - 1 < n, and its family was tested by the claim)
      const EpAddr cur = ep_load(P.T, g);
      if (a.a != cur.a || a.b != cur.b || a.c != cur.c) {
        ep_store(P.T, g, a);
        code = 3u;
      }
    }
    P.code[g] = code;
  }
  uint32_t r, n_peers, n_roamed;
  wgrp::block_rank(code & 1u, s_cnt[0], r, n_peers);
  wgrp::block_rank(code & 2u, s_cnt[1], r, n_roamed);
  if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4(n_peers, 0u, n_roamed, 0u);
}

__global__ void __launch_bounds__(256) k_ep_learn_place(EpLearnParams P) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t g = blockIdx.x * kRankRange + threadIdx.x;
  const bool roamed = g < P.T.max_peers && (P.code[g] & 2u);
  const uint4 pre = P.part[blockIdx.x];
  uint32_t r, total;
  wgrp::block_rank(roamed, s_cnt, r, total);
  if (roamed && pre.z + r < P.cap) P.roamed[pre.z + r] = g;
  if (g == 0) {  // (8-B stores: the summary need not be 16-B aligned)
    const uint4 tot = *P.tot;
    uint2* sum = (uint2*)P.summary;
    sum[0] = make_uint2(P.ctl[0], tot.x);
    sum[1] = make_uint2(tot.z, P.ctl[1]);
  }
}

// ---- send lists ----
struct EpSendParams {
  EpTables T;
  wg_pkt* desc;
  uint32_t* status;
  wg_tx_item* items;
  uint4* part;
  uint32_t n, gate;
};

// descriptor i: is it live, and if so listed (then peer and dst are its)
__device__ __forceinline__ bool ep_send_desc(const EpSendParams& P, uint32_t i, uint4& d0, uint4& d1, bool& listed, uint32_t& peer,
                                             EpAddr& dst) {
  listed = false;
  if (i >= P.n) return false;
  const uint4* d = (const uint4*)(P.desc + i);
  d1 = d[1];  // counter lo, counter hi, len, key slot
  if (d1.z == WG_LEN_INVALID || (P.status && P.status[i] != WG_PKT_OK)) return false;
  d0 = d[0];
  if (d1.w < P.T.K) {
    peer = P.T.map[d1.w];
    if (peer < P.T.max_peers) {
      dst = ep_load(P.T, peer);
      listed = ep_family(dst.c) != 0u;
    }
  }
  return true;
}

__global__ void __launch_bounds__(256) k_ep_send_judge(EpSendParams P) {
  __shared__ uint32_t s_cnt[2][4];
  __shared__ uint64_t s_sum[4];
  const uint32_t i = blockIdx.x * kRankRange + threadIdx.x;
  uint4 d0, d1;
  bool listed;
  uint32_t peer;
  EpAddr dst;
  const bool live = ep_send_desc(P, i, d0, d1, listed, peer, dst);
  if (P.gate && live && !listed) {  // refused as the timers' gate refuses: the seal and the framer skip it
    if (P.status) P.status[i] = WG_PKT_NOENDPOINT;
    ((uint32_t*)(P.desc + i))[6] = WG_LEN_INVALID;
  }
  uint32_t r, n_items, n_noep;
  uint64_t ex, bytes;
  wgrp::block_rank(listed, s_cnt[0], r, n_items);
  wgrp::block_rank(live && !listed, s_cnt[1], r, n_noep);
  wgrp::block_scan64(listed ? (uint64_t)(d1.z + 32u) : 0ull, s_sum, ex, bytes);
  if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4((uint32_t)bytes, (uint32_t)(bytes >> 32), n_items, n_noep);
}

// (a descriptor the gate refused is no longer live, one it did not refuse is judged as before)
__global__ void __launch_bounds__(256) k_ep_send_place(EpSendParams P) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t i = blockIdx.x * kRankRange + threadIdx.x;
  uint4 d0, d1;
  bool listed;
  uint32_t peer;
  EpAddr dst;
  (void)ep_send_desc(P, i, d0, d1, listed, peer, dst);
  const uint4 pre = P.part[blockIdx.x];
  uint32_t r, total;
  wgrp::block_rank(listed, s_cnt, r, total);
  if (!listed) return;
  ep_item(P.items + pre.z + r, wgrp::u64_of(d0.z, d0.w) - 16ull, d1.z + 32u, d1.w, peer, i, dst);
}

struct EpHsSendParams {
  EpTables T;
  const uint8_t* entries;
  const uint32_t* n_entries;
  const uint32_t* status;
  const uint32_t* peer;
  const wg_hs_src* src;
  wg_tx_item* items;
  uint4* part;
  uint32_t n, n_src;
};

// entry k of a handshake list: is there a message, and if so has it a destination
template <uint32_t KIND>
__device__ __forceinline__ bool ep_hs_entry(const EpHsSendParams& P, uint32_t k, bool& listed, uint64_t& off, uint32_t& len, uint32_t& peer,
                                            EpAddr& dst) {
  constexpr uint32_t stride = KIND == WG_HS_SEND_RESPONSES ? (uint32_t)sizeof(wg_hs_session)
                              : KIND == WG_HS_SEND_INITIATIONS ? (uint32_t)sizeof(wg_hs_record) : (uint32_t)sizeof(wg_hs_cookie_reply);
  listed = false;
  if (k >= wgrp::dev_count(P.n_entries, P.n)) return false;
  const uint32_t* e = (const uint32_t*)(P.entries + (size_t)k * stride);
  if (KIND == WG_HS_SEND_INITIATIONS) {
    if (P.status[k] != WG_HS_INIT_OK) return false;
    off = (uint64_t)k * stride + offsetof(wg_hs_record, msg);
    len = e[1];
    peer = P.peer[k];
    if (peer < P.T.max_peers) {
      dst = ep_load(P.T, peer);
      listed = ep_family(dst.c) != 0u;
    }
  } else {
    const uint32_t index = e[0];
    if (KIND == WG_HS_SEND_RESPONSES) {
      off = (uint64_t)k * stride + offsetof(wg_hs_session, response);
      len = WG_HS_RESP_SIZE;
      peer = e[2];
    } else {
      off = (uint64_t)k * stride + offsetof(wg_hs_cookie_reply, msg);
      len = e[1];
      peer = WG_HS_NOPEER;
    }
    listed = index < P.n_src && ep_norm(P.src + index, dst);
  }
  return true;
}

template <uint32_t KIND>
__global__ void __launch_bounds__(256) k_ep_hs_judge(EpHsSendParams P) {
  __shared__ uint32_t s_cnt[2][4];
  __shared__ uint64_t s_sum[4];
  const uint32_t k = blockIdx.x * kRankRange + threadIdx.x;
  bool listed;
  uint64_t off;
  uint32_t len = 0, peer;
  EpAddr dst;
  const bool is = ep_hs_entry<KIND>(P, k, listed, off, len, peer, dst);
  uint32_t r, n_items, n_nodst;
  uint64_t ex, bytes;
  wgrp::block_rank(listed, s_cnt[0], r, n_items);
  wgrp::block_rank(is && !listed, s_cnt[1], r, n_nodst);
  wgrp::block_scan64(listed ? (uint64_t)len : 0ull, s_sum, ex, bytes);
  if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4((uint32_t)bytes, (uint32_t)(bytes >> 32), n_items, n_nodst);
}

template <uint32_t KIND>
__global__ void __launch_bounds__(256) k_ep_hs_place(EpHsSendParams P) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t k = blockIdx.x * kRankRange + threadIdx.x;
  bool listed;
  uint64_t off = 0;
  uint32_t len = 0, peer = 0;
  EpAddr dst;
  (void)ep_hs_entry<KIND>(P, k, listed, off, len, peer, dst);
  const uint4 pre = P.part[blockIdx.x];
  uint32_t r, total;
  wgrp::block_rank(listed, s_cnt, r, total);
  if (!listed) return;
  ep_item(P.items + pre.z + r, off, len, 0xFFFFFFFFu, peer, k, dst);
}

}  // namespace wgep

namespace {

wgep::EpTables ep_tables(const wg_ctx* c, const EndpointsState* t) {
  return wgep::EpTables{(uint64_t*)t->d_ep.p, (uint32_t*)t->d_map.p, c->key_slots, t->max_peers};
}

template <uint32_t KIND>
void ep_hs_launch(const wgep::EpHsSendParams& P, void* summary, hipStream_t s) {
  rank_launch(wgep::k_ep_hs_judge<KIND>, wgep::k_ep_hs_place<KIND>, P, summary, s);
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------
extern "C" {

int wg_endpoints_reserve(wg_ctx* c, uint32_t max_peers) {
  if (!c) return fail(WG_EINVAL, "NULL context");
  if (max_peers > 0x40000000u) return fail(WG_E2BIG, "endpoints of %u peers", max_peers);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (c->ep) {
    if (max_peers <= c->ep->max_peers) return WG_OK;
    return fail(WG_EINVAL, "endpoints reserved for %u peers do not grow to %u", c->ep->max_peers, max_peers);
  }
  auto t = std::make_unique<EndpointsState>();
  t->max_peers = max_peers;
  const size_t np = std::max(max_peers, 1u);
  int rc;
  if ((rc = t->d_ep.ensure(np * sizeof(wg_hs_src))) != WG_OK || (rc = t->d_map.ensure((size_t)c->key_slots * 4)) != WG_OK ||
      (rc = t->d_claim.ensure(np * 4)) != WG_OK || (rc = t->d_code.ensure(np * 4)) != WG_OK || (rc = t->d_ctl.ensure(16)) != WG_OK ||
      (rc = t->d_part.ensure(((size_t)std::max(rank_blocks(max_peers), rank_blocks(kEpItems)) + 1u) * 16)) != WG_OK)
    return rc;
  HIPTRY(t->order.create());
  HIPTRY(hipMemsetAsync(t->d_ep.p, 0, np * sizeof(wg_hs_src), c->stream));
  fill_u32(c->stream, t->d_map.p, c->key_slots, WG_HS_NOPEER);
  HIPTRY(hipGetLastError());
  HIPTRY(hipStreamSynchronize(c->stream));
  c->ep = t.release();
  return WG_OK;
}

int wg_endpoints_set(wg_ctx* c, uint32_t first, uint32_t n, const wg_hs_src* endpoints) {
  if (!c || (!endpoints && n)) return fail(WG_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  EndpointsState* t = c->ep;
  if (!t) return fail(WG_EINVAL, "wg_endpoints_set before wg_endpoints_reserve");
  if ((uint64_t)first + n > t->max_peers) return fail(WG_ERANGE, "peers [%u, %u + %u) exceed the %u reserved", first, first, n, t->max_peers);
  for (uint32_t k = 0; k < n; ++k)
    if (endpoints[k].family != 0 && endpoints[k].family != 4 && endpoints[k].family != 6)
      return fail(WG_EINVAL, "peer %u: endpoint family %u is none of 0, 4, 6", first + k, endpoints[k].family);
  if (!n) return WG_OK;
  std::vector<wg_hs_src> v(endpoints, endpoints + n);
  for (auto& e : v) ep_normalise(&e);
  HIPTRY(hipDeviceSynchronize());  // after everything queued, on any stream
  HIPTRY(hipMemcpy((wg_hs_src*)t->d_ep.p + first, v.data(), (size_t)n * sizeof(wg_hs_src), hipMemcpyHostToDevice));
  return WG_OK;
}

int wg_endpoints_get(wg_ctx* c, uint32_t first, uint32_t n, wg_hs_src* out) {
  if (!c || (!out && n)) return fail(WG_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const EndpointsState* t = c->ep;
  return range_copy(t ? t->d_ep.p : nullptr, "wg_endpoints_get before wg_endpoints_reserve", first, n, t ? t->max_peers : 0u, "peers", out, sizeof *out, true);
}

int wg_endpoint_slots_set(wg_ctx* c, uint32_t first, uint32_t n, const uint32_t* peers) {
  if (!c || (!peers && n)) return fail(WG_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  return range_copy(c->ep ? c->ep->d_map.p : nullptr, "wg_endpoint_slots_set before wg_endpoints_reserve", first, n, c->key_slots, "key slots", (void*)peers, 4, false);
}

int wg_endpoint_slots_get(wg_ctx* c, uint32_t first, uint32_t n, uint32_t* peers) {
  if (!c || (!peers && n)) return fail(WG_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  return range_copy(c->ep ? c->ep->d_map.p : nullptr, "wg_endpoint_slots_get before wg_endpoints_reserve", first, n, c->key_slots, "key slots", peers, 4, true);
}

int wg_endpoints_start(wg_ctx* c, const wg_endpoints_start_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  if (b->_reserved) return fail(WG_EINVAL, "wg_endpoints_start_batch._reserved must be 0");
  if (b->flags & ~WG_EP_LEARN_RESPONSE) return fail(WG_EINVAL, "unknown endpoints start flags 0x%x", b->flags);
  if (!b->summary || (((uintptr_t)b->summary) & 7u)) return fail(WG_EINVAL, "summary must be non-NULL and 8-byte aligned");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  EndpointsState* t = c->ep;
  if (!t) return fail(WG_EINVAL, "wg_endpoints_start before wg_endpoints_reserve");
  const uint32_t n = b->n;
  int rc;
  if ((rc = inst_batch_check(*b, "endpoints start")) != WG_OK) return rc;
  const InstView V = inst_view(*b);
  const bool learn = b->source == WG_HS_INSTALL_SESSIONS || (b->flags & WG_EP_LEARN_RESPONSE);
  if (n) {
    if (!b->inst_status || (((uintptr_t)b->inst_status) & 3u)) return fail(WG_EINVAL, "inst_status must be non-NULL and 4-byte aligned");
    if ((b->n_src && !b->src) || (((uintptr_t)b->src) & 7u)) return fail(WG_EINVAL, "src must be non-NULL and 8-byte aligned");
    const HsRange out[] = {{b->summary, sizeof(wg_endpoints_start_summary)}};
    const HsRange in[] = {{b->entries, (uint64_t)n * V.stride}, {b->n_entries, b->n_entries ? 4u : 0u}, {b->inst_status, (uint64_t)n * 4},
                          {b->send_slot, (uint64_t)b->n_slots * 4}, {b->recv_slot, (uint64_t)b->n_slots * 4},
                          {b->src, (uint64_t)b->n_src * sizeof(wg_hs_src)}};
    if (hs_ranges_overlap(out, in)) return fail(WG_EINVAL, "summary must not overlap an input of wg_endpoints_start");
  }
  const bool capturing = stream_capturing(s);
  if ((rc = plan_begin(t->order, s, capturing, true, [] { return WG_OK; }, kEpStartWords, n)) != WG_OK) return rc;
  HIPTRY(hipMemsetAsync(b->summary, 0, sizeof(wg_endpoints_start_summary), s));
  if (n) {
    wgep::EpStartParams P{};
    P.T = ep_tables(c, t);
    P.V = V;
    P.status = b->inst_status;
    P.src = b->src;
    P.claim = (uint32_t*)t->d_claim.p;
    P.summary = (uint32_t*)b->summary;
    P.n_src = b->n_src;
    P.learn = learn ? 1u : 0u;
    const uint32_t nb = rank_blocks(n);
    if (learn) fill_u32(s, P.claim, t->max_peers, 0xFFFFFFFFu);
    hipLaunchKernelGGL(wgep::k_ep_start_map, dim3(nb), dim3(256), 0, s, P);
    if (learn) hipLaunchKernelGGL(wgep::k_ep_start_write, dim3(nb), dim3(256), 0, s, P);
  }
  return plan_end(t->order, s, capturing, kEpStartWords);
}

int wg_endpoints_learn(wg_ctx* c, const wg_endpoints_learn_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  if (!b->summary || (((uintptr_t)b->summary) & 7u)) return fail(WG_EINVAL, "summary must be non-NULL and 8-byte aligned");
  if (b->roamed_cap && (!b->roamed || (((uintptr_t)b->roamed) & 3u))) return fail(WG_EINVAL, "roamed must be non-NULL and 4-byte aligned");
  if (b->roamed_cap > 0x40000000u) return fail(WG_E2BIG, "roamed list of %u peers", b->roamed_cap);
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  EndpointsState* t = c->ep;
  if (!t) return fail(WG_EINVAL, "wg_endpoints_learn before wg_endpoints_reserve");
  const uint32_t n = b->n;
  if (n > 0x40000000u) return fail(WG_E2BIG, "endpoints learn of %u packets", n);
  const bool capturing = stream_capturing(s);
  if (n == 0) {
    HIPTRY(hipMemsetAsync(b->summary, 0, sizeof(wg_endpoints_learn_summary), s));
    return WG_OK;
  }
  if (!b->desc || (((uintptr_t)b->desc) & 15u) || !b->final_status || (((uintptr_t)b->final_status) & 3u) || !b->src || (((uintptr_t)b->src) & 7u))
    return fail(WG_EINVAL, "desc / final_status / src must be non-NULL and aligned (16 / 4 / 8 bytes)");
  {
    const HsRange out[] = {{b->roamed, (uint64_t)b->roamed_cap * 4}, {b->summary, sizeof(wg_endpoints_learn_summary)}};
    const HsRange in[] = {{b->desc, (uint64_t)n * sizeof(wg_pkt)}, {b->final_status, (uint64_t)n * 4}, {b->src, (uint64_t)n * sizeof(wg_hs_src)}};
    const int ov = hs_ranges_overlap(out, in);
    if (ov == 1) return fail(WG_EINVAL, "roamed and summary must not overlap");
    if (ov == 2) return fail(WG_EINVAL, "an output of wg_endpoints_learn must not overlap desc, final_status or src");
  }
  int rc;
  if ((rc = plan_begin(t->order, s, capturing, true, [] { return WG_OK; }, kEpLearnWords, n)) != WG_OK) return rc;
  const uint32_t ranges = std::max(1u, rank_blocks(t->max_peers));
  wgep::EpLearnParams P{};
  P.T = ep_tables(c, t);
  P.desc = b->desc;
  P.status = b->final_status;
  P.src = b->src;
  P.roamed = b->roamed;
  P.summary = (uint32_t*)b->summary;
  P.claim = (uint32_t*)t->d_claim.p;
  P.code = (uint32_t*)t->d_code.p;
  P.ctl = (uint32_t*)t->d_ctl.p;
  P.part = (uint4*)t->d_part.p;
  P.tot = P.part + ranges;
  P.n = n;
  P.cap = b->roamed_cap;
  hipLaunchKernelGGL(wgep::k_ep_learn_fill, dim3(ranges), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgep::k_ep_learn_claim, dim3(rank_blocks(n)), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgep::k_ep_learn_judge, dim3(ranges), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgrp::k_rx_scan, dim3(1), dim3(256), 0, s, P.part, ranges, (uint2*)(P.part + ranges));
  hipLaunchKernelGGL(wgep::k_ep_learn_place, dim3(ranges), dim3(256), 0, s, P);
  return plan_end(t->order, s, capturing, kEpLearnWords);
}

int wg_tx_sendlist(wg_ctx* c, const wg_tx_sendlist_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  if (b->flags & ~WG_SEND_GATE) return fail(WG_EINVAL, "unknown send list flags 0x%x", b->flags);
  if (!b->summary || (((uintptr_t)b->summary) & 7u)) return fail(WG_EINVAL, "summary must be non-NULL and 8-byte aligned");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  EndpointsState* t = c->ep;
  if (!t) return fail(WG_EINVAL, "wg_tx_sendlist before wg_endpoints_reserve");
  const uint32_t n = b->n;
  if (n > 0x40000000u) return fail(WG_E2BIG, "send list of %u descriptors", n);
  if (n == 0) {
    HIPTRY(hipMemsetAsync(b->summary, 0, sizeof(wg_tx_sendlist_summary), s));
    return WG_OK;
  }
  if (!b->desc || (((uintptr_t)b->desc) & 15u) || (((uintptr_t)b->status) & 3u))
    return fail(WG_EINVAL, "desc must be non-NULL and 16-byte aligned (status: 4-byte, or NULL)");
  if (!b->items || (((uintptr_t)b->items) & 15u)) return fail(WG_EINVAL, "items must be non-NULL and 16-byte aligned");
  {
    const bool gate = (b->flags & WG_SEND_GATE) != 0;
    const uint64_t db = (uint64_t)n * sizeof(wg_pkt), sb = b->status ? (uint64_t)n * 4 : 0;
    // (with the gate desc and status are outputs too; they may not overlap anything either way)
    const HsRange out[] = {{b->items, (uint64_t)n * sizeof(wg_tx_item)}, {b->summary, sizeof(wg_tx_sendlist_summary)},
                           {gate ? b->desc : nullptr, gate ? db : 0}, {gate ? b->status : nullptr, gate ? sb : 0}};
    const HsRange in[] = {{b->desc, gate ? 0 : db}, {b->status, gate ? 0 : sb}};
    const int ov = hs_ranges_overlap(out, in);
    if (ov) return fail(WG_EINVAL, "items and summary must overlap neither each other nor desc or status");
  }
  const bool capturing = stream_capturing(s);
  int rc;
  if ((rc = ep_send_begin(t, s, capturing, n)) != WG_OK) return rc;
  wgep::EpSendParams P{};
  P.T = ep_tables(c, t);
  P.desc = b->desc;
  P.status = b->status;
  P.items = b->items;
  P.part = (uint4*)t->d_part.p;
  P.n = n;
  P.gate = (b->flags & WG_SEND_GATE) ? 1u : 0u;
  rank_launch(wgep::k_ep_send_judge, wgep::k_ep_send_place, P, b->summary, s);
  return plan_end(t->order, s, capturing, kEpSendWords);
}

int wg_hs_sendlist(wg_ctx* c, const wg_hs_sendlist_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  if (b->flags) return fail(WG_EINVAL, "unknown handshake send list flags 0x%x (the gate is wg_tx_sendlist's)", b->flags);
  if (b->kind > WG_HS_SEND_COOKIE_REPLIES) return fail(WG_EINVAL, "unknown handshake send list kind %u", b->kind);
  if (!b->summary || (((uintptr_t)b->summary) & 7u)) return fail(WG_EINVAL, "summary must be non-NULL and 8-byte aligned");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  EndpointsState* t = c->ep;
  if (!t) return fail(WG_EINVAL, "wg_hs_sendlist before wg_endpoints_reserve");
  const uint32_t n = b->n;
  if (n > 0x40000000u) return fail(WG_E2BIG, "handshake send list of %u entries", n);
  if (n == 0) {
    HIPTRY(hipMemsetAsync(b->summary, 0, sizeof(wg_hs_sendlist_summary), s));
    return WG_OK;
  }
  const bool inits = b->kind == WG_HS_SEND_INITIATIONS;
  if (!b->entries || (((uintptr_t)b->entries) & 15u) || (((uintptr_t)b->n_entries) & 3u))
    return fail(WG_EINVAL, "entries must be non-NULL and 16-byte aligned (n_entries: 4-byte)");
  if (inits && (!b->status || !b->peer || ((((uintptr_t)b->status) | ((uintptr_t)b->peer)) & 3u)))
    return fail(WG_EINVAL, "initiations need status and peer, non-NULL and 4-byte aligned");
  if (!inits && ((b->n_src && !b->src) || (((uintptr_t)b->src) & 7u))) return fail(WG_EINVAL, "src must be non-NULL and 8-byte aligned");
  if (!b->items || (((uintptr_t)b->items) & 15u)) return fail(WG_EINVAL, "items must be non-NULL and 16-byte aligned");
  {
    const uint64_t stride = b->kind == WG_HS_SEND_RESPONSES ? sizeof(wg_hs_session) : inits ? sizeof(wg_hs_record) : sizeof(wg_hs_cookie_reply);
    const HsRange out[] = {{b->items, (uint64_t)n * sizeof(wg_tx_item)}, {b->summary, sizeof(wg_hs_sendlist_summary)}};
    const HsRange in[] = {{b->entries, (uint64_t)n * stride}, {b->n_entries, b->n_entries ? 4u : 0u}, {b->status, inits ? (uint64_t)n * 4 : 0},
                          {b->peer, inits ? (uint64_t)n * 4 : 0}, {b->src, inits ? 0 : (uint64_t)b->n_src * sizeof(wg_hs_src)}};
    const int ov = hs_ranges_overlap(out, in);
    if (ov == 1) return fail(WG_EINVAL, "items and summary must not overlap");
    if (ov == 2) return fail(WG_EINVAL, "an output of wg_hs_sendlist must not overlap entries, n_entries, status, peer or src");
  }
  const bool capturing = stream_capturing(s);
  int rc;
  if ((rc = ep_send_begin(t, s, capturing, n)) != WG_OK) return rc;
  wgep::EpHsSendParams P{};
  P.T = ep_tables(c, t);
  P.entries = (const uint8_t*)b->entries;
  P.n_entries = b->n_entries;
  P.status = b->status;
  P.peer = b->peer;
  P.src = b->src;
  P.items = b->items;
  P.part = (uint4*)t->d_part.p;
  P.n = n;
  P.n_src = b->n_src;
  if (b->kind == WG_HS_SEND_RESPONSES) ep_hs_launch<WG_HS_SEND_RESPONSES>(P, b->summary, s);
  else if (inits) ep_hs_launch<WG_HS_SEND_INITIATIONS>(P, b->summary, s);
  else ep_hs_launch<WG_HS_SEND_COOKIE_REPLIES>(P, b->summary, s);
  return plan_end(t->order, s, capturing, kEpSendWords);
}

}  // extern "C"
