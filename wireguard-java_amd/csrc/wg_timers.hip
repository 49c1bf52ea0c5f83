// wg_timers.hip — the sessions' lifetime, on the device (included by wg_capi.hip).
//
// The reference decides three things about an established session against the wall clock, with one thread per
// peer: whether it is still used (EstablishedSession.isExpired, EstablishedSession.java:28,:114: 120 s after its
// creation), to whom the node initiates again (SessionManager.sessionInitiationThread, SessionManager.java:92-111,
// which waits for the session to expire and retries 5 s after a failed attempt, :188) and when a keepalive goes out
// (KeepaliveSender.java:29-85: one as soon as the session changes, :69-73, then one per interval). Here a session
// is two records of a per-key-slot table, a peer one record of a per-peer table, and time a tick count the host
// writes into device memory:
//   wg_timers_start  behind wg_hs_install: the records of the sessions it installed (wg_session.hip's `installed`);
//                    the peer's current session.
//   wg_timers_mark   behind wg_rx_deliver / wg_tx_plan: proof of life per key slot, and the gate that refuses a
//                    descriptor on a session that is dead or past its limits.
//   wg_timers_sweep  the tick: the expired sessions (their retirement, and with WIPE their keys zeroed), the peers to initiate to in
//                    wg_hs_initiate's format, the keepalives as ready wg_pkt descriptors.
// Nothing per packet or per session crosses to the host, and nothing about a call lives on the host: a captured
// chain replays with `now` refreshed in place.
//
// No thread order. A stamp is raised by a 64-bit atomicMax. Of several sessions of one peer in one start the lowest
// entry becomes current (atomicMin on the peer's claim word, read behind a kernel boundary). The sweep's verdicts
// are all reached in its first launch, from the state as the call found it; its last launch only places what has
// room and changes the records of what it placed, each record by the one thread that owns it. A peer's verdict
// tests the expiry of its current session itself instead of reading the slot's verdict, so slot i and peer i are
// judged by one thread of one launch and the compaction is one rank_launch-shaped pass over max(key slots, peers)
// positions with the 16-byte record {expired, live, initiate, keepalive} per range.
//
// The configuration sits at a fixed device address and is read when a call runs (wg_plan.hip, fixed headers).
#pragma once

namespace {

struct TimersState {
  DevBuf d_cfg;    // wg_timers_config (fixed address)
  DevBuf d_slots;  // key_slots x wg_timer_slot
  DevBuf d_peers;  // max_peers x wg_timer_peer_state
  DevBuf d_claim;  // start: per peer, the lowest entry that starts a session of it
  DevBuf d_code;   // sweep: per position, its verdict bits
  DevBuf d_part;   // sweep: per range {expired, live, initiate, keepalive}, then their prefixes; behind them the totals
  uint32_t max_peers = 0;
  StreamOrder order;  // last start / mark / sweep / setter
};

const PlanWords kTmStartWords{"timers start", "entries", "wg_timers_reserve"};
const PlanWords kTmMarkWords{"timers mark", "descriptors", "wg_timers_reserve"};
const PlanWords kTmSweepWords{"timers sweep", "positions", "wg_timers_reserve"};

void tm_free(wg_ctx* c) {
  delete c->tm;
  c->tm = nullptr;
}

uint32_t tm_positions(const wg_ctx* c, const TimersState* t) { return std::max(c->key_slots, t->max_peers); }

}  // namespace

// ---- device -------------------------------------------------------------------------------
namespace wgtm {

constexpr uint32_t kExp = 1u, kInit = 2u, kKeep = 4u;  // a position's verdict bits

struct TmTables {
  wg_timer_slot* slots;
  wg_timer_peer_state* peers;
  const wg_timers_config* cfg;
  const uint64_t* now;
  uint32_t K, max_peers;
};

__device__ __forceinline__ bool tm_send(uint32_t state) { return state == WG_TIMER_SEND_INITIATOR || state == WG_TIMER_SEND_RESPONDER; }
__device__ __forceinline__ bool tm_live(uint32_t state) { return tm_send(state) || state == WG_TIMER_RECV; }
__device__ __forceinline__ uint64_t tm_age(uint64_t now, uint64_t t) { return now >= t ? now - t : 0ull; }

__device__ __forceinline__ bool tm_expired(const wg_timer_slot& r, uint64_t counter, const wg_timers_config& C, uint64_t now) {
  return (C.reject_after_time && tm_age(now, r.born) >= C.reject_after_time) ||
         (C.reject_after_messages && counter >= C.reject_after_messages) ||
         (C.linger && r.superseded && tm_age(now, r.superseded) >= C.linger);
}

// a stamp never moves back; a lane that finds it raised already issues no atomic
__device__ __forceinline__ void tm_raise(uint64_t* p, uint64_t now) {
  if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < now) (void)atomicMax((unsigned long long*)p, (unsigned long long)now);
}

// ---- start ----
struct TmStartParams {
  TmTables T;
  InstView V;
  const uint32_t* status;
  uint32_t* claim;
  uint32_t role;
};

// a session ends: both its records are dead, and its peer has no current session if it was that. (Writers of one
// word all write the same value.)
__device__ __forceinline__ void tm_end(const TmTables& T, uint32_t send_slot, uint32_t recv_slot, uint32_t peer) {
  if (send_slot < T.K) T.slots[send_slot].state = WG_TIMER_DEAD;
  if (recv_slot < T.K) T.slots[recv_slot].state = WG_TIMER_DEAD;
  if (peer < T.max_peers && T.peers[peer].current == send_slot) T.peers[peer].current = WG_TIMER_NOSLOT;
}

// the live session that owns `slot` ends (a start takes the slot)
__device__ __forceinline__ void tm_kill(const TmTables& T, uint32_t slot) {
  const uint4 h = *(const uint4*)(T.slots + slot);  // state, peer, local_index, partner
  if (!tm_live(h.x)) return;
  const bool snd = tm_send(h.x);
  tm_end(T, snd ? slot : h.w, snd ? h.w : slot, h.y);
}

__global__ void __launch_bounds__(256) k_tm_start_kill(TmStartParams P) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  uint32_t s, r, peer;
  if (*P.T.now == 0ull || !installed(P.V, P.status, P.T.K, P.T.max_peers, j, s, r, peer)) return;
  tm_kill(P.T, s);
  tm_kill(P.T, r);
  if (peer != WG_HS_NOPEER) (void)atomicMin(P.claim + peer, j);
}

__global__ void __launch_bounds__(256) k_tm_start_write(TmStartParams P) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  const uint64_t now = *P.T.now;
  uint32_t s, r, peer;
  if (now == 0ull || !installed(P.V, P.status, P.T.K, P.T.max_peers, j, s, r, peer)) return;
  const uint32_t index = inst_entry(P.V, j)[P.V.w_local];
  const bool win = peer != WG_HS_NOPEER && P.claim[peer] == j;
  const uint64_t sup = (peer != WG_HS_NOPEER && !win) ? now : 0ull;
  const uint32_t n_lo = (uint32_t)now, n_hi = (uint32_t)(now >> 32);
  uint4* a = (uint4*)(P.T.slots + s);
  a[0] = make_uint4(P.role, peer, index, r);
  a[1] = make_uint4(n_lo, n_hi, 0u, 0u);
  a[2] = make_uint4(0u, 0u, (uint32_t)sup, (uint32_t)(sup >> 32));
  uint4* b = (uint4*)(P.T.slots + r);
  b[0] = make_uint4(WG_TIMER_RECV, peer, index, s);
  b[1] = make_uint4(n_lo, n_hi, 0u, 0u);
  b[2] = make_uint4(0u, 0u, 0u, 0u);
  if (win) {  // (a previous current that lost a slot to this call has been cleared by the kill pass)
    const uint32_t prev = P.T.peers[peer].current;
    if (prev < P.T.K && tm_send(P.T.slots[prev].state)) P.T.slots[prev].superseded = now;
    P.T.peers[peer].current = s;
  }
}

// ---- mark ----
struct TmMarkParams {
  TmTables T;
  wg_pkt* desc;
  uint32_t* status;
  uint32_t* summary;
  uint32_t n, tx, gate, slot_first, slot_count;
};

__global__ void __launch_bounds__(256) k_tm_mark(TmMarkParams P) {
  __shared__ uint32_t s_cnt[2][4];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint64_t now = *P.T.now;
  bool marked = false, refused = false, data = false;
  uint32_t slot = 0;
  if (i < P.n && now != 0ull) {
    const uint32_t st = P.status[i];
    const uint4 d = ((const uint4*)(P.desc + i))[1];  // counter lo, counter hi, len, key slot
    slot = d.w;
    wg_timer_slot* rec = P.T.slots + slot;  // (dereferenced below the bound only)
    if (!P.tx) {
      if ((st == WG_PKT_OK || st == WG_PKT_KEEPALIVE) && slot < P.T.K && rec->state == WG_TIMER_RECV) {
        marked = true;
        data = st == WG_PKT_OK;
      }
    } else if (st == WG_PKT_OK) {
      const bool live = slot < P.T.K && tm_send(rec->state);
      if (P.gate && slot >= P.slot_first && slot - P.slot_first < P.slot_count) {
        const wg_timers_config C = *P.T.cfg;
        refused = !live || (C.reject_after_time && tm_age(now, rec->born) >= C.reject_after_time) ||
                  (C.reject_after_messages && wgrp::u64_of(d.x, d.y) >= C.reject_after_messages);
      }
      if (refused) {
        P.status[i] = WG_PKT_NOSESSION;
        ((uint32_t*)(P.desc + i))[6] = WG_LEN_INVALID;
      } else if (live) {
        marked = true;
        data = d.z > 0u;
      }
    }
  }
  // Where every mark of a wave names one slot (a batch on one session), the wave's first marking lane raises for all
  // 64, last_data if any of them carried data: one atomic per wave and stamp.
  {
    bool for_all;
    const bool mine = wgrp::wave_elect<false>(marked, slot, for_all);
    const uint64_t any_data = __ballot(marked && data);
    if (mine) {
      tm_raise(&P.T.slots[slot].last, now);
      if (for_all ? any_data != 0ull : data) tm_raise(&P.T.slots[slot].last_data, now);
    }
  }
  uint32_t r, n_marked, n_refused;
  wgrp::block_rank(marked, s_cnt[0], r, n_marked);
  wgrp::block_rank(refused, s_cnt[1], r, n_refused);
  if (threadIdx.x == 0) {
    if (n_marked) atomicAdd(P.summary, n_marked);
    if (n_refused) atomicAdd(P.summary + 1, n_refused);
  }
}

// ---- sweep ----
struct TmSweepParams {
  TmTables T;
  uint64_t* send;   // the transmit state's counters
  RxSessHdr* hdr;   // RETIRE: the receiver-index table (NULL: the context has none)
  uint32_t* code;
  uint4* part;
  const uint4* tot;  // = part + ranges: the totals, written by k_rx_scan
  wg_timer_expired* expired;
  uint32_t* initiate;
  wg_pkt* keep;
  uint32_t* summary;
  uint64_t wire_base, wire_stride;
  uint32_t N, cap_exp, cap_init, cap_keep, retire;
  uint32_t pad_keep;  // the keepalive array's own capacity (cap_keep: what of it has a wire slot)
  uint4* keys;        // WIPE: the key table, two 16-B words per slot (NULL: no wipe)
};

__global__ void __launch_bounds__(256) k_tm_sweep_judge(TmSweepParams P) {
  __shared__ uint32_t s_cnt[4][4];
  const uint32_t i = blockIdx.x * kRankRange + threadIdx.x;
  const TmTables& T = P.T;
  const uint64_t now = *T.now;
  const wg_timers_config C = *T.cfg;
  uint32_t code = 0;
  bool live = false;
  if (now != 0ull && i < T.K) {
    const wg_timer_slot r = T.slots[i];
    if (tm_send(r.state)) {
      live = true;
      if (tm_expired(r, P.send[i], C, now)) {
        code |= kExp;
      } else if (r.peer < T.max_peers) {
        const wg_timer_peer_state pr = T.peers[r.peer];
        if (pr.current == i) {
          const uint64_t heard = r.partner < T.K ? T.slots[r.partner].last_data : 0ull;
          const bool persistent = pr.keepalive_interval && (r.last == 0ull || tm_age(now, r.last) >= pr.keepalive_interval);
          const bool passive = C.keepalive_timeout && heard > r.last && tm_age(now, heard) >= C.keepalive_timeout;
          if (persistent || passive) code |= kKeep;
        }
      }
    }
  }
  if (now != 0ull && i < T.max_peers) {
    const wg_timer_peer_state pr = T.peers[i];
    if (pr.flags & WG_TIMER_PEER_CAN_INITIATE) {
      bool need = true;  // no current session, or an expired one
      if (pr.current < T.K) {
        const wg_timer_slot r = T.slots[pr.current];
        const uint64_t sent = P.send[pr.current];
        if (tm_send(r.state) && !tm_expired(r, sent, C, now)) {
          need = (C.rekey_after_time && tm_age(now, r.born) >= C.rekey_after_time) ||
                 (C.rekey_after_messages && sent >= C.rekey_after_messages);
          if ((C.flags & WG_TIMERS_INITIATOR_ONLY) && r.state != WG_TIMER_SEND_INITIATOR) need = false;
        }
      }
      if (need && (pr.rekey_listed == 0ull || tm_age(now, pr.rekey_listed) >= C.rekey_timeout)) code |= kInit;
    }
  }
  if (i < P.N) P.code[i] = code;
  uint32_t r, n_exp, n_live, n_init, n_keep;
  wgrp::block_rank(code & kExp, s_cnt[0], r, n_exp);
  wgrp::block_rank(live, s_cnt[1], r, n_live);
  wgrp::block_rank(code & kInit, s_cnt[2], r, n_init);
  wgrp::block_rank(code & kKeep, s_cnt[3], r, n_keep);
  if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4(n_exp, n_live, n_init, n_keep);
}

// The grid covers max(N, cap_init, pad_keep) positions: the initiate and keepalive lists are padded up to their
// capacities (no peer; a descriptor the seal skips).
__global__ void __launch_bounds__(256) k_tm_sweep_place(TmSweepParams P, uint32_t ranges) {
  __shared__ uint32_t s_cnt[4][4];
  const uint32_t g = blockIdx.x * kRankRange + threadIdx.x;
  const TmTables& T = P.T;
  const uint64_t now = *T.now;
  const uint4 tot = *P.tot;
  const uint32_t code = g < P.N ? P.code[g] : 0u;
  const uint4 pre = blockIdx.x < ranges ? P.part[blockIdx.x] : make_uint4(0u, 0u, 0u, 0u);
  uint32_t re, ri, rk, total;
  wgrp::block_rank(code & kExp, s_cnt[0], re, total);
  wgrp::block_rank(code & kInit, s_cnt[1], ri, total);
  wgrp::block_rank(code & kKeep, s_cnt[2], rk, total);
  const uint32_t n_exp = min(tot.x, P.cap_exp), n_init = min(tot.z, P.cap_init), n_keep = min(tot.w, P.cap_keep);
  bool retired = false;
  if ((code & kExp) && pre.x + re < P.cap_exp) {
    const uint4 h = *(const uint4*)(T.slots + g);  // state, peer, local_index, partner
    *(uint4*)(P.expired + pre.x + re) = make_uint4(g, h.w, h.y, h.z);
    if (P.retire) {
      // (the index's entry only if it still names this session's recv slot: the index may have been installed again)
      if (P.hdr) retired = rx_retire_entry(*P.hdr, h.z, h.w + 1u);
      tm_end(T, g, h.w, h.y);
      if (P.keys) {  // the session's two keys: stores of zero, no key byte is loaded
        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
        P.keys[2u * g] = z;
        P.keys[2u * g + 1u] = z;
        if (h.w < T.K) {
          P.keys[2u * h.w] = z;
          P.keys[2u * h.w + 1u] = z;
        }
      }
    }
  }
  if ((code & kInit) && pre.z + ri < P.cap_init) {
    P.initiate[pre.z + ri] = g;
    T.peers[g].rekey_listed = now;
  }
  if (g >= n_init && g < P.cap_init) P.initiate[g] = 0xFFFFFFFFu;
  if ((code & kKeep) && pre.w + rk < P.cap_keep) {
    const uint32_t j = pre.w + rk;
    const uint64_t counter = P.send[g], out_off = P.wire_base + (uint64_t)j * P.wire_stride + 16u;
    uint4* d = (uint4*)(P.keep + j);
    d[0] = make_uint4(0u, 0u, (uint32_t)out_off, (uint32_t)(out_off >> 32));
    d[1] = make_uint4((uint32_t)counter, (uint32_t)(counter >> 32), 0u, g);
    P.send[g] = counter + 1ull;
    T.slots[g].last = now;  // (due means now > last)
  }
  if (g >= n_keep && g < P.pad_keep) {
    uint4* d = (uint4*)(P.keep + g);
    d[0] = make_uint4(0u, 0u, 0u, 0u);
    d[1] = make_uint4(0u, 0u, WG_LEN_INVALID, 0u);
  }
  uint32_t rr, n_retired;
  wgrp::block_rank(retired, s_cnt[3], rr, n_retired);
  if (threadIdx.x == 0 && n_retired) atomicSub(&P.hdr->count, n_retired);
  if (g == 0) {  // (8-B stores: the summary need not be 16-B aligned)
    uint2* sum = (uint2*)P.summary;
    sum[0] = make_uint2(tot.x, n_exp);
    sum[1] = make_uint2(tot.z, n_init);
    sum[2] = make_uint2(tot.w, n_keep);
    sum[3] = make_uint2(tot.y - (P.retire ? n_exp : 0u), 0u);
  }
}

// setter: keepalive_interval and flags of peers [first, first + n); current and rekey_listed stay
__global__ void __launch_bounds__(256) k_tm_peers_set(wg_timer_peer_state* peers, const wg_timer_peer* in, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  peers[i].keepalive_interval = in[i].keepalive_interval;
  peers[i].flags = in[i].flags;
}

__global__ void __launch_bounds__(256) k_tm_peers_init(wg_timer_peer_state* peers, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) peers[i] = wg_timer_peer_state{WG_TIMER_NOSLOT, 0u, 0ull, 0ull};
}

}  // namespace wgtm

namespace {

wgtm::TmTables tm_tables(const wg_ctx* c, const TimersState* t, const uint64_t* now) {
  return wgtm::TmTables{(wg_timer_slot*)t->d_slots.p, (wg_timer_peer_state*)t->d_peers.p, (const wg_timers_config*)t->d_cfg.p, now,
                        c->key_slots, t->max_peers};
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------
extern "C" {

int wg_timers_reserve(wg_ctx* c, uint32_t max_peers) {
  if (!c) return fail(WG_EINVAL, "NULL context");
  if (max_peers > 0x40000000u) return fail(WG_E2BIG, "timer state for %u peers", max_peers);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (c->tm) {
    if (max_peers <= c->tm->max_peers) return WG_OK;
    return fail(WG_EINVAL, "timer state reserved for %u peers does not grow to %u", c->tm->max_peers, max_peers);
  }
  TxState* x;  // the keepalives' counters are the transmit state's
  int rc;
  if ((rc = tx_get(c, &x)) != WG_OK) return rc;
  auto t = std::make_unique<TimersState>();
  t->max_peers = max_peers;
  const uint32_t N = std::max(c->key_slots, max_peers), nb = std::max(1u, rank_blocks(N));
  if ((rc = t->d_cfg.ensure(sizeof(wg_timers_config))) != WG_OK || (rc = t->d_slots.ensure((size_t)c->key_slots * sizeof(wg_timer_slot))) != WG_OK ||
      (rc = t->d_peers.ensure((size_t)std::max(max_peers, 1u) * sizeof(wg_timer_peer_state))) != WG_OK ||
      (rc = t->d_claim.ensure((size_t)std::max(max_peers, 1u) * 4)) != WG_OK || (rc = t->d_code.ensure((size_t)std::max(N, 1u) * 4)) != WG_OK ||
      (rc = t->d_part.ensure(((size_t)nb + 1u) * 16)) != WG_OK)
    return rc;
  HIPTRY(t->order.create());
  HIPTRY(hipMemsetAsync(t->d_cfg.p, 0, sizeof(wg_timers_config), c->stream));
  HIPTRY(hipMemsetAsync(t->d_slots.p, 0, (size_t)c->key_slots * sizeof(wg_timer_slot), c->stream));
  if (max_peers)
    hipLaunchKernelGGL(wgtm::k_tm_peers_init, dim3(rank_blocks(max_peers)), dim3(256), 0, c->stream, (wg_timer_peer_state*)t->d_peers.p, max_peers);
  HIPTRY(hipGetLastError());
  HIPTRY(hipStreamSynchronize(c->stream));
  c->tm = t.release();
  return WG_OK;
}

int wg_timers_config_set(wg_ctx* c, const wg_timers_config* config) {
  if (!c || !config) return fail(WG_EINVAL, "NULL argument");
  if (config->flags & ~(uint64_t)WG_TIMERS_INITIATOR_ONLY) return fail(WG_EINVAL, "unknown timers flags 0x%llx", (unsigned long long)config->flags);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (!c->tm) return fail(WG_EINVAL, "wg_timers_config_set before wg_timers_reserve");
  HIPTRY(hipDeviceSynchronize());  // after everything queued, on any stream
  HIPTRY(hipMemcpy(c->tm->d_cfg.p, config, sizeof *config, hipMemcpyHostToDevice));
  return WG_OK;
}

int wg_timers_peers_set(wg_ctx* c, uint32_t first, uint32_t n, const wg_timer_peer* peers) {
  if (!c || (!peers && n)) return fail(WG_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  TimersState* t = c->tm;
  if (!t) return fail(WG_EINVAL, "wg_timers_peers_set before wg_timers_reserve");
  if ((uint64_t)first + n > t->max_peers) return fail(WG_ERANGE, "peers [%u, %u + %u) exceed the %u reserved", first, first, n, t->max_peers);
  for (uint32_t k = 0; k < n; ++k)
    if ((peers[k].flags & ~WG_TIMER_PEER_CAN_INITIATE) || peers[k]._zero) return fail(WG_EINVAL, "peer %u: unknown flags", first + k);
  if (!n) return WG_OK;
  HIPTRY(hipDeviceSynchronize());
  DevBuf tmp;
  int rc;
  if ((rc = tmp.ensure((size_t)n * sizeof(wg_timer_peer))) != WG_OK) return rc;
  HIPTRY(hipMemcpyAsync(tmp.p, peers, (size_t)n * sizeof(wg_timer_peer), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(wgtm::k_tm_peers_set, dim3(rank_blocks(n)), dim3(256), 0, c->stream, (wg_timer_peer_state*)t->d_peers.p + first,
                     (const wg_timer_peer*)tmp.p, n);
  HIPTRY(hipGetLastError());
  HIPTRY(hipStreamSynchronize(c->stream));
  return WG_OK;
}

int wg_timers_get(wg_ctx* c, uint32_t first, uint32_t n, wg_timer_slot* out) {
  if (!c || (!out && n)) return fail(WG_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const TimersState* t = c->tm;
  return range_copy(t ? t->d_slots.p : nullptr, "wg_timers_get before wg_timers_reserve", first, n, c->key_slots, "key slots", out, sizeof *out, true);
}

int wg_timers_peers_get(wg_ctx* c, uint32_t first, uint32_t n, wg_timer_peer_state* out) {
  if (!c || (!out && n)) return fail(WG_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const TimersState* t = c->tm;
  return range_copy(t ? t->d_peers.p : nullptr, "wg_timers_peers_get before wg_timers_reserve", first, n, t ? t->max_peers : 0u, "peers", out, sizeof *out, true);
}

int wg_timers_start(wg_ctx* c, const wg_timers_start_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  if (b->_reserved) return fail(WG_EINVAL, "wg_timers_start_batch._reserved must be 0");
  if (!b->now || (((uintptr_t)b->now) & 7u)) return fail(WG_EINVAL, "now must be non-NULL and 8-byte aligned");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  TimersState* t = c->tm;
  if (!t) return fail(WG_EINVAL, "wg_timers_start before wg_timers_reserve");
  const uint32_t n = b->n;
  int rc;
  if ((rc = inst_batch_check(*b, "timers start")) != WG_OK || n == 0) return rc;
  if (!b->inst_status || (((uintptr_t)b->inst_status) & 3u)) return fail(WG_EINVAL, "inst_status must be non-NULL and 4-byte aligned");
  const bool capturing = stream_capturing(s);
  if ((rc = plan_begin(t->order, s, capturing, true, [] { return WG_OK; }, kTmStartWords, n)) != WG_OK) return rc;
  wgtm::TmStartParams P{};
  P.T = tm_tables(c, t, b->now);
  P.V = inst_view(*b);
  P.status = b->inst_status;
  P.claim = (uint32_t*)t->d_claim.p;
  P.role = b->source == WG_HS_INSTALL_SESSIONS ? WG_TIMER_SEND_RESPONDER : WG_TIMER_SEND_INITIATOR;
  const uint32_t nb = rank_blocks(n);
  fill_u32(s, P.claim, t->max_peers, 0xFFFFFFFFu);
  hipLaunchKernelGGL(wgtm::k_tm_start_kill, dim3(nb), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgtm::k_tm_start_write, dim3(nb), dim3(256), 0, s, P);
  return plan_end(t->order, s, capturing, kTmStartWords);
}

int wg_timers_mark(wg_ctx* c, const wg_timers_mark_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  if (b->_reserved) return fail(WG_EINVAL, "wg_timers_mark_batch._reserved must be 0");
  if (b->dir != WG_TIMERS_RX && b->dir != WG_TIMERS_TX) return fail(WG_EINVAL, "unknown mark direction %u", b->dir);
  if ((b->flags & ~WG_TIMERS_GATE) || (b->flags && b->dir != WG_TIMERS_TX)) return fail(WG_EINVAL, "unknown mark flags 0x%x (the gate is the transmit direction's)", b->flags);
  if (!b->now || (((uintptr_t)b->now) & 7u)) return fail(WG_EINVAL, "now must be non-NULL and 8-byte aligned");
  if (!b->summary || (((uintptr_t)b->summary) & 7u)) return fail(WG_EINVAL, "summary must be non-NULL and 8-byte aligned");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  TimersState* t = c->tm;
  if (!t) return fail(WG_EINVAL, "wg_timers_mark before wg_timers_reserve");
  const uint32_t n = b->n;
  if (n && (!b->desc || (((uintptr_t)b->desc) & 15u) || !b->status || (((uintptr_t)b->status) & 3u)))
    return fail(WG_EINVAL, "desc / status must be non-NULL and aligned (16 / 4 bytes)");
  const bool capturing = stream_capturing(s);
  int rc;
  if ((rc = plan_begin(t->order, s, capturing, true, [] { return WG_OK; }, kTmMarkWords, n)) != WG_OK) return rc;
  HIPTRY(hipMemsetAsync(b->summary, 0, sizeof(wg_timers_mark_summary), s));
  if (n) {
    wgtm::TmMarkParams P{};
    P.T = tm_tables(c, t, b->now);
    P.desc = b->desc;
    P.status = b->status;
    P.summary = (uint32_t*)b->summary;
    P.n = n;
    P.tx = b->dir == WG_TIMERS_TX ? 1u : 0u;
    P.gate = (b->flags & WG_TIMERS_GATE) ? 1u : 0u;
    P.slot_first = b->slot_first;
    P.slot_count = b->slot_count;
    hipLaunchKernelGGL(wgtm::k_tm_mark, dim3(rank_blocks(n)), dim3(256), 0, s, P);
  }
  return plan_end(t->order, s, capturing, kTmMarkWords);
}

int wg_timers_sweep(wg_ctx* c, const wg_timers_sweep_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  if ((b->flags & ~(WG_TIMERS_RETIRE | WG_TIMERS_WIPE)) || ((b->flags & WG_TIMERS_WIPE) && !(b->flags & WG_TIMERS_RETIRE)))
    return fail(WG_EINVAL, "unknown sweep flags 0x%x (the wipe goes with the retire)", b->flags);
  if (!b->now || (((uintptr_t)b->now) & 7u)) return fail(WG_EINVAL, "now must be non-NULL and 8-byte aligned");
  if (!b->summary || (((uintptr_t)b->summary) & 7u)) return fail(WG_EINVAL, "summary must be non-NULL and 8-byte aligned");
  if ((b->expired_cap && (!b->expired || (((uintptr_t)b->expired) & 15u))) || (b->initiate_cap && (!b->initiate || (((uintptr_t)b->initiate) & 3u))) ||
      (b->keepalive_cap && (!b->keepalives || (((uintptr_t)b->keepalives) & 15u))))
    return fail(WG_EINVAL, "a list with a capacity must be non-NULL and aligned (expired, keepalives: 16 bytes; initiate: 4)");
  if (b->initiate_cap > 0x40000000u || b->keepalive_cap > 0x40000000u)
    return fail(WG_E2BIG, "list capacities of %u peers / %u keepalives", b->initiate_cap, b->keepalive_cap);
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  TimersState* t = c->tm;
  if (!t) return fail(WG_EINVAL, "wg_timers_sweep before wg_timers_reserve");
  TxState* x = c->tx;  // (wg_timers_reserve created it)
  if (!x) return fail(WG_EINVAL, "wg_timers_sweep without a transmit state");
  const bool retire = (b->flags & WG_TIMERS_RETIRE) != 0;
  RxPlanState* rp = retire ? c->rxp : nullptr;
  const bool capturing = stream_capturing(s);
  const uint32_t N = tm_positions(c, t);
  int rc;
  if ((rc = plan_begin(t->order, s, capturing, true, [] { return WG_OK; }, kTmSweepWords, N)) != WG_OK) return rc;
  if (!capturing && (rc = x->order.after_last(s)) != WG_OK) return rc;
  if (!capturing && rp && (rc = rp->order.after_last(s)) != WG_OK) return rc;
  const uint32_t ranges = std::max(1u, rank_blocks(N));
  const uint64_t wire_slots = (b->wire_stride >= 32u && b->wire_base <= b->out_size) ? (b->out_size - b->wire_base) / b->wire_stride : 0;
  wgtm::TmSweepParams P{};
  P.T = tm_tables(c, t, b->now);
  P.send = (uint64_t*)x->d_send.p;
  P.hdr = rp ? (RxSessHdr*)rp->d_hdr.p : nullptr;
  P.code = (uint32_t*)t->d_code.p;
  P.part = (uint4*)t->d_part.p;
  P.tot = P.part + ranges;
  P.expired = b->expired;
  P.initiate = b->initiate;
  P.keep = b->keepalives;
  P.summary = (uint32_t*)b->summary;
  P.wire_base = b->wire_base;
  P.wire_stride = b->wire_stride;
  P.N = N;
  P.cap_exp = b->expired_cap;
  P.cap_init = b->initiate_cap;
  P.cap_keep = (uint32_t)std::min<uint64_t>(b->keepalive_cap, wire_slots);
  P.retire = retire ? 1u : 0u;
  P.pad_keep = b->keepalive_cap;
  P.keys = (b->flags & WG_TIMERS_WIPE) ? (uint4*)c->keys : nullptr;
  hipLaunchKernelGGL(wgtm::k_tm_sweep_judge, dim3(ranges), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgrp::k_rx_scan, dim3(1), dim3(256), 0, s, P.part, ranges, (uint2*)(P.part + ranges));
  hipLaunchKernelGGL(wgtm::k_tm_sweep_place, dim3(std::max(ranges, rank_blocks(std::max(b->initiate_cap, b->keepalive_cap)))), dim3(256), 0, s, P, ranges);
  if ((rc = plan_end(t->order, s, capturing, kTmSweepWords)) != WG_OK) return rc;
  if (!capturing && (rc = x->order.mark(s)) != WG_OK) return rc;
  if (!capturing && rp && (rc = rp->order.mark(s)) != WG_OK) return rc;
  return WG_OK;
}

}  // extern "C"
