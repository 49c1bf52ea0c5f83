// wg_tx.hip — transmit-side planning before seal, on the device (included by wg_capi.hip).
//
// The reference's outbound path decides three things per tun packet on the host:
// which peers get it (PeerList.broadcastPacketToPeers, PeerList.java:94-106: every peer;
// TransportManager.sendOutgoingTransportNow, TransportManager.java:137-147, drops it for a peer
// without a session), which send counter it takes (SymmetricKeypair.cipher: SEND_COUNTER.getAndAdd(1),
// from 0 for a new keypair, SymmetricKeypair.java:37,:64; written into the header by
// EncryptedOutgoingTransport.java:11-14) and where its wire packet goes
// (UnencryptedOutgoingTransport.java:14-27: header, then ct || tag at +16). wg_tx_plan does the three
// for a whole tun ring and writes the wg_pkt descriptors that wg_seal_batch(WG_F_FRAME) takes; the
// per-session send counters stay on the device, where the nonces are built.
//
// Besides the reference's broadcast it offers WireGuard's cryptokey routing: a longest-prefix match
// of the destination (read as destinationIPOf reads it, TransportManager.java:124-130) over a route
// table. That match is the standard one (/0, /32 and /128 entries match, of equal prefixes the later
// entry wins), NOT IPFilter.search's rule that a full-length entry never matches (wg_rx.hip): the
// reference has no outbound routing, so there is nothing to be faithful to. The table is compiled on
// the host into stride-8 nodes like compile_level in wg_rx.hip, but every entry carries, beside the
// next node, the key slot of the longest prefix that ends inside its byte: a lookup is 4 (IPv4) or
// 16 (IPv6) dependent reads, and the last slot seen on the way wins.
//
// Counters. A routed packet takes send[slot] + (routed packets to the same slot with a lower batch
// index): a stable rank per key slot. It is computed without any wait between workgroups (no spin on
// another block's flag, no assumption about dispatch order), in three launches on the plan's stream:
//   k_tx_classify  the batch is cut into R contiguous runs; ONE wave walks a run in 64-packet steps,
//                  in order: size checks, the route lookup, code[i] (key slot or status) to scratch,
//                  and the lanes of a step that share a slot (wave_match) add their number to the
//                  run's own row of an R x K count matrix (K = key slots; 1 in broadcast mode, whose
//                  only key is "passed the size checks"). Rows are private to a run: no contention.
//   k_tx_scan      per key slot, the column's exclusive prefixes go to a second R x K matrix and the
//                  counts are zeroed again; base[slot] = send[slot], send[slot] += the column's sum
//                  (broadcast: send[peer] += the sum for every peer).
//   k_tx_emit      the same runs, walked again in the same order: rank = the row's prefix + the lanes
//                  of the same slot below me in this step; the row entry then advances by the group's
//                  size; every descriptor is one 32-B record (two 16-B stores) plus its status.
// A run's row is touched by its own wave only, but by different lanes in different steps, so the row
// is updated with (uncontended) atomics, which are performed at the L2 in issue order; what one
// launch leaves for the next is ordered by the kernel boundary. Nothing about a plan lives on the
// host between calls: the count matrix is zero when it is allocated and is zeroed again by its
// consumer (k_tx_scan) in every plan, every other scratch word is written before it is read, so a
// captured plan replays any number of times. R is as large as a 16-MiB matrix and 1,024 rows allow
// (R = n / 64 up to 65,536 packets at 4,096 key slots): a run of one step is one dependent chain of
// loads, and runs are the only parallelism the walk has.
#pragma once

namespace {

constexpr uint32_t kTxMaxRuns = 1024;              // R <= 1024 (k_tx_scan: 64 row chunks of <= 16 rows)
constexpr size_t kTxMatrixBudget = 16u << 20;      // R x K x 4 B <= 16 MiB: R = 64 at 65,536 key slots
constexpr uint32_t kTxCode = 0xFFFFFFF0u;          // code[i] >= kTxCode: not routed, status = code - kTxCode

struct TxRouteHdr {  // at a fixed device address; a route change rewrites it (and may move the nodes)
  const uint2* entries;  // nodes x 256: {next node (0: none), key slot + 1 of the longest prefix ending in this byte (0: none)}
  uint32_t root4, root6; // node index (0: no prefixes of that family)
  uint32_t def4, def6;   // key slot + 1 of the /0 prefix (0: none)
};

struct TxState {
  DevBuf d_send;   // per key slot: u64 send counter
  DevBuf d_peers;  // broadcast peers (key_slots entries, fixed address)
  uint32_t n_peers = 0;
  DevBuf d_rhdr, d_rent;  // TxRouteHdr (fixed address) and its nodes
  DevBuf d_code;   // per packet: key slot or kTxCode + status
  DevBuf d_cnt;    // R x K count matrix: zero between plans (k_tx_scan zeroes what it has read)
  DevBuf d_pre;    // R x K prefixes of the counts, per column (written by k_tx_scan, advanced by k_tx_emit)
  bool cnt_dirty = false;  // a plan's launches failed part-way: the count matrix is zeroed before the next plan
  DevBuf d_base;   // per key slot: the counter before this plan (broadcast: [0] = packets that passed)
  StreamOrder order;  // last plan / counter, peer or route write
};

const PlanWords kTxWords{"transmit plan", "packets", "wg_tx_reserve"};

// runs R and steps per run for a plan of n packets over K keys
void tx_geometry(uint32_t n, uint32_t K, uint32_t* runs, uint32_t* spr) {
  const uint32_t nsteps = (n + 63u) / 64u;
  const uint32_t rmax = (uint32_t)std::max<size_t>(1, std::min<size_t>(kTxMaxRuns, kTxMatrixBudget / 4 / K));
  *spr = std::max(1u, (nsteps + rmax - 1u) / rmax);
  *runs = (nsteps + *spr - 1u) / *spr;
}
// matrix rows to hold for plans of up to n packets (tx_geometry never yields more)
uint32_t tx_max_rows(uint32_t n, uint32_t K) {
  const uint32_t nsteps = (n + 63u) / 64u;
  const uint32_t rmax = (uint32_t)std::max<size_t>(1, std::min<size_t>(kTxMaxRuns, kTxMatrixBudget / 4 / K));
  return std::max(1u, std::min(nsteps, rmax));
}

// The transmit state, allocated at the first wg_tx_* call. Caller holds c->mu.
int tx_get(wg_ctx* c, TxState** out) {
  if (!c->tx) {
    if (c->key_slots > kTxCode) return fail(WG_EINVAL, "key table too large for the transmit planner");
    auto t = std::make_unique<TxState>();
    int rc;
    if ((rc = t->d_send.ensure((size_t)c->key_slots * 8)) != WG_OK ||
        (rc = t->d_peers.ensure((size_t)c->key_slots * 4)) != WG_OK ||
        (rc = t->d_base.ensure((size_t)c->key_slots * 8)) != WG_OK ||
        (rc = t->d_rhdr.ensure(sizeof(TxRouteHdr))) != WG_OK)
      return rc;
    hipError_t e = t->order.create();
    if (e == hipSuccess) e = hipMemsetAsync(t->d_send.p, 0, (size_t)c->key_slots * 8, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->d_rhdr.p, 0, sizeof(TxRouteHdr), c->stream);  // no routes
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(WG_EDEVICE, "transmit state: %s", hipGetErrorString(e));
    c->tx = t.release();
  }
  *out = c->tx;
  return WG_OK;
}

void tx_free(wg_ctx* c) {
  delete c->tx;
  c->tx = nullptr;
}

// zero the send counters of key slots [first, first + n) (a new SymmetricKeypair starts at 0,
// SymmetricKeypair.java:37), in stream order after every plan queued before it; later plans (any
// stream) wait for the reset. Nothing to do before the first wg_tx_* call. Caller holds c->mu.
int tx_reset_slots(wg_ctx* c, uint32_t first, uint32_t n, hipStream_t s) {
  TxState* t = c->tx;
  if (!t || !n) return WG_OK;
  int rc;
  if ((rc = t->order.after_last(s)) != WG_OK) return rc;
  HIPTRY(hipMemsetAsync((uint64_t*)t->d_send.p + first, 0, (size_t)n * 8, s));
  return t->order.mark(s);
}

// scratch for plans of up to n packets: does it fit, and (plan_reserve) its growth
bool tx_scratch_fits(const wg_ctx* c, const TxState* t, uint32_t n) {
  const size_t cnt = (size_t)tx_max_rows(n, c->key_slots) * c->key_slots * 4;
  return (size_t)std::max(n, 1u) * 4 <= t->d_code.cap && cnt <= t->d_cnt.cap && cnt <= t->d_pre.cap;
}
int tx_scratch_grow(wg_ctx* c, TxState* t, uint32_t n) {
  const size_t cnt = (size_t)tx_max_rows(n, c->key_slots) * c->key_slots * 4;
  int rc;
  t->cnt_dirty = true;  // until the (new) count matrix has been zeroed
  if ((rc = t->d_code.ensure((size_t)std::max(n, 1u) * 4)) != WG_OK || (rc = t->d_cnt.ensure(cnt)) != WG_OK ||
      (rc = t->d_pre.ensure(cnt)) != WG_OK)
    return rc;
  HIPTRY(hipMemsetAsync(t->d_cnt.p, 0, t->d_cnt.cap, c->stream));
  HIPTRY(hipStreamSynchronize(c->stream));
  t->cnt_dirty = false;
  return WG_OK;
}

// ---- host: the route table as a binary trie, then stride-8 nodes ---------------------------
struct RouteTrie {
  std::vector<std::array<int32_t, 2>> child{{{-1, -1}}};
  std::vector<uint32_t> slot1{0};  // key slot + 1 of the prefix ending at this node (0: none)
  void insert(const uint8_t* addr, uint32_t prefix_len, uint32_t slot) {
    int32_t node = 0;
    for (uint32_t i = 0; i < prefix_len; ++i) {
      const int bit = (addr[i / 8] >> (7 - i % 8)) & 1;
      if (child[node][bit] < 0) {
        child[node][bit] = (int32_t)child.size();
        child.push_back({-1, -1});
        slot1.push_back(0);
      }
      node = child[node][bit];
    }
    slot1[node] = slot + 1u;  // of equal prefixes the later entry wins
  }
};

// trie node at depth 8L -> 256 entries; returns its index in `out` / 256 (>= 1). An entry's slot is
// that of the longest prefix of length depth + 1 .. depth + 8 on the way to its byte value (the
// prefix of length `depth` itself belongs to the parent's entry, a /0 to the header).
uint32_t route_level(const RouteTrie& t, int32_t bnode, uint32_t depth, uint32_t nbits, std::vector<uint2>& out) {
  const uint32_t me = (uint32_t)(out.size() / 256);
  out.resize(out.size() + 256, make_uint2(0u, 0u));
  for (uint32_t v = 0; v < 256; ++v) {
    uint32_t best = 0;
    int32_t cur = bnode;
    for (uint32_t k = 0; k < 8 && cur >= 0; ++k) {
      cur = t.child[cur][(v >> (7 - k)) & 1];
      if (cur >= 0 && t.slot1[cur]) best = t.slot1[cur];
    }
    uint32_t next = 0;
    if (cur >= 0 && depth + 8 < nbits && (t.child[cur][0] >= 0 || t.child[cur][1] >= 0))
      next = route_level(t, cur, depth + 8, nbits, out);
    out[(size_t)me * 256 + v] = make_uint2(next, best);
  }
  return me;
}

}  // namespace

// ---- device -------------------------------------------------------------------------------
namespace wgtx {

struct TxParams {
  const uint8_t* in;
  uint64_t in_size;
  const uint64_t* pkt_off;
  const uint32_t* pkt_len;
  wg_pkt* desc;
  uint32_t* status;
  uint64_t wire_base, wire_stride;
  uint64_t wire_slots;  // whole wire slots inside out_size (host: (out_size - wire_base) / wire_stride)
  uint32_t n, max_len, route;
  uint32_t runs, spr;   // R runs of spr 64-packet steps
  uint32_t K;           // columns of the count matrix: key slots (route), 1 (broadcast)
  uint32_t n_peers;
  const uint32_t* peers;
  const TxRouteHdr* routes;
  uint64_t* send;
  uint64_t* base;
  uint32_t* code;
  uint32_t* cnt;
  uint32_t* pre;
};

// For every active lane: the lowest lane holding the same key (leader), how many lanes with that key
// lie below it (below) and how many hold it in all (size). Every lane of the wave must reach the
// call; an inactive lane gets leader = itself, below = 0, size = 0. One round per distinct key.
__device__ __forceinline__ void wave_match(bool active, uint32_t key, uint32_t& leader, uint32_t& below,
                                           uint32_t& size) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t mlo = 0, mhi = 0;  // the lanes of my group (the loop only records them: it runs once per distinct key)
  bool todo = active;
  for (;;) {
    const uint64_t act = __ballot(todo);
    if (!act) break;
    const int l = __ffsll((unsigned long long)act) - 1;
    const uint32_t lk = (uint32_t)__builtin_amdgcn_readlane((int)key, l);
    const bool mine = todo && key == lk;
    const uint64_t m = __ballot(mine);
    if (mine) {
      mlo = (uint32_t)m;
      mhi = (uint32_t)(m >> 32);
      todo = false;
    }
  }
  leader = !active ? lane : mlo ? (uint32_t)__ffs((int)mlo) - 1u : 32u + (uint32_t)__ffs((int)mhi) - 1u;
  below = __builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, 0u));
  size = (uint32_t)__popc(mlo) + (uint32_t)__popc(mhi);
}

// key slot of packet i (route mode; 0 in broadcast mode), or kTxCode + its status
__device__ __forceinline__ uint32_t tx_classify_one(const TxParams& P, const TxRouteHdr& H, uint32_t i) {
  const uint64_t off = P.pkt_off[i];
  const uint32_t len = P.pkt_len[i];
  // wire slots up to and including this packet's last one (n_desc < 2^31: no overflow)
  const uint64_t need = P.route ? (uint64_t)i + 1u : ((uint64_t)i + 1u) * P.n_peers;
  const bool fits = len <= P.max_len && off <= P.in_size && (uint64_t)len <= P.in_size - off &&
                    (uint64_t)len + 32u <= P.wire_stride && need <= P.wire_slots;
  if (!fits) return kTxCode + WG_PKT_TOOLONG;
  if (!P.route) return 0u;
  if (len == 0) return kTxCode + WG_PKT_BADIP;
  const uint8_t* p = P.in + off;
  // the IPv4 destination is fetched together with the version byte (one round trip, not two)
  uint32_t d[16];
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) d[k] = len >= 20u ? p[16u + k] : 0u;
  const uint32_t ver = p[0] >> 4;
  uint32_t nbytes, node, best;
  if (ver == 4) {
    if (len < 20u) return kTxCode + WG_PKT_BADIP;
    nbytes = 4, node = H.root4, best = H.def4;
  } else if (ver == 6) {
    if (len < 40u) return kTxCode + WG_PKT_BADIP;
    nbytes = 16, node = H.root6, best = H.def6;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) d[k] = p[24u + k];
  } else {
    return kTxCode + WG_PKT_BADIP;
  }
#pragma unroll
  for (uint32_t L = 0; L < 16; ++L) {
    if (L >= nbytes || !node) break;
    const uint2 e = H.entries[(size_t)node * 256 + d[L]];
    if (e.y) best = e.y;
    node = e.x;
  }
  return best ? best - 1u : kTxCode + WG_PKT_NOROUTE;
}

__device__ __forceinline__ void tx_store(const TxParams& P, uint64_t j, uint64_t in_off, uint32_t len, uint32_t slot,
                                         uint64_t counter, uint32_t status) {
  const uint64_t out_off = P.wire_base + j * P.wire_stride + 16u;
  uint4* d = (uint4*)(P.desc + j);
  d[0] = make_uint4((uint32_t)in_off, (uint32_t)(in_off >> 32), (uint32_t)out_off, (uint32_t)(out_off >> 32));
  d[1] = make_uint4((uint32_t)counter, (uint32_t)(counter >> 32), len, slot);
  P.status[j] = status;
}

__global__ void __launch_bounds__(256) k_tx_classify(TxParams P) {
  const uint32_t run = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (run >= P.runs) return;  // (the whole wave)
  uint32_t* row = P.cnt + (size_t)run * P.K;
  const uint32_t nsteps = (P.n + 63u) / 64u;
  const uint32_t s1 = min((run + 1u) * P.spr, nsteps);
  TxRouteHdr H{};
  if (P.route) H = *P.routes;
  for (uint32_t s = run * P.spr; s < s1; ++s) {
    const uint32_t i = s * 64u + lane;
    const bool in = i < P.n;
    const uint32_t code = in ? tx_classify_one(P, H, i) : kTxCode;
    if (in) P.code[i] = code;
    const bool routed = in && code < kTxCode;
    uint32_t leader, below, size;
    wave_match(routed, code, leader, below, size);
    if (routed && lane == leader) atomicAdd(&row[code], size);
  }
}

// Block = 4 key slots x 64 row chunks: every thread reads its chunk of the column (at most 16 rows,
// loads in flight together) and zeroes it for the next plan, the chunks' sums are combined in LDS,
// and the chunk's exclusive prefixes of the whole column go to the prefix matrix.
__global__ void __launch_bounds__(256) k_tx_scan(TxParams P) {
  __shared__ uint32_t part[64][4];
  __shared__ uint32_t total_s;
  const uint32_t tx = threadIdx.x & 3u, ty = threadIdx.x >> 2;
  const uint32_t col = blockIdx.x * 4u + tx;
  const uint32_t rpt = (P.runs + 63u) / 64u, r0 = ty * rpt;  // rpt <= 16 (R <= 1024)
  uint32_t v[16], sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < 16; ++k) {
    const uint32_t r = r0 + k;
    const bool mine = k < rpt && r < P.runs && col < P.K;
    v[k] = mine ? P.cnt[(size_t)r * P.K + col] : 0u;
    sum += v[k];
  }
#pragma unroll
  for (uint32_t k = 0; k < 16; ++k) {
    const uint32_t r = r0 + k;
    if (k < rpt && r < P.runs && col < P.K && v[k]) P.cnt[(size_t)r * P.K + col] = 0u;
  }
  part[ty][tx] = sum;
  __syncthreads();
  uint32_t pre = 0, total = 0;
  for (uint32_t y = 0; y < 64; ++y) {
    const uint32_t x = part[y][tx];
    pre += y < ty ? x : 0u;
    total += x;
  }
#pragma unroll
  for (uint32_t k = 0; k < 16; ++k) {
    const uint32_t r = r0 + k;
    if (k < rpt && r < P.runs && col < P.K) P.pre[(size_t)r * P.K + col] = pre;
    pre += v[k];
  }
  if (P.route) {
    if (ty == 0 && col < P.K) {
      const uint64_t old = P.send[col];
      P.base[col] = old;
      if (total) P.send[col] = old + total;
    }
    return;
  }
  // broadcast (one column, one block): every peer's counter advances by the packets that passed
  if (threadIdx.x == 0) {
    total_s = total;
    P.base[0] = total;
  }
  __syncthreads();
  const uint32_t passed = total_s;
  for (uint32_t p = threadIdx.x; p < P.n_peers; p += 256u) P.send[P.peers[p]] += passed;  // peers are distinct
}

__global__ void __launch_bounds__(256) k_tx_emit(TxParams P) {
  const uint32_t run = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (run >= P.runs) return;  // (the whole wave)
  uint32_t* row = P.pre + (size_t)run * P.K;
  const uint32_t nsteps = (P.n + 63u) / 64u;
  const uint32_t s1 = min((run + 1u) * P.spr, nsteps);
  for (uint32_t s = run * P.spr; s < s1; ++s) {
    const uint32_t i = s * 64u + lane;
    const bool in = i < P.n;
    const uint32_t code = in ? P.code[i] : kTxCode;
    const uint64_t off = in ? P.pkt_off[i] : 0ull;
    const uint32_t len = in ? P.pkt_len[i] : 0u;
    const bool routed = in && code < kTxCode;
    const uint64_t base = (routed && P.route) ? P.base[code] : 0ull;
    uint32_t leader, below, size;
    wave_match(routed, code, leader, below, size);
    uint32_t rel = 0;
    if (routed && lane == leader) rel = atomicAdd(&row[code], size);  // the row's prefix; the next step's is past this group
    const uint32_t rank = (uint32_t)__shfl((int)rel, (int)leader) + below;
    if (P.route) {
      if (!in) continue;
      if (routed) tx_store(P, i, off, len, code, base + rank, WG_PKT_OK);
      else tx_store(P, i, off, WG_LEN_INVALID, 0u, 0ull, code - kTxCode);
      continue;
    }
    // broadcast: the step's packets x peers descriptors are contiguous; lanes take them in turn
    const uint64_t passed = P.base[0];
    const uint32_t cnt = min(64u, P.n - s * 64u);
    const uint64_t tot = (uint64_t)cnt * P.n_peers;
    for (uint64_t e0 = 0; e0 < tot; e0 += 64u) {  // wave-uniform trips: every lane feeds the shuffles
      const uint64_t e = e0 + lane;
      const bool act = e < tot;
      const uint32_t tl = act ? (uint32_t)(e / P.n_peers) : 0u;
      const uint32_t p = act ? (uint32_t)(e - (uint64_t)tl * P.n_peers) : 0u;
      const uint32_t t_len = (uint32_t)__shfl((int)len, (int)tl);
      const uint32_t t_ok = (uint32_t)__shfl((int)(routed ? 1u : 0u), (int)tl);
      const uint32_t t_rank = (uint32_t)__shfl((int)rank, (int)tl);
      const uint32_t t_code = (uint32_t)__shfl((int)code, (int)tl);
      const uint64_t t_off = (uint64_t)(uint32_t)__shfl((int)(uint32_t)off, (int)tl) |
                             ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(off >> 32), (int)tl) << 32);
      if (!act) continue;
      const uint32_t slot = P.peers[p];
      const uint64_t j = ((uint64_t)s * 64u + tl) * P.n_peers + p;
      // send[] already holds the advanced counter: this plan's first is `passed` below it (mod 2^64)
      if (t_ok) tx_store(P, j, t_off, t_len, slot, P.send[slot] - passed + t_rank, WG_PKT_OK);
      else tx_store(P, j, t_off, WG_LEN_INVALID, slot, 0ull, t_code - kTxCode);
    }
  }
}

}  // namespace wgtx

// ---- C ABI --------------------------------------------------------------------------------
extern "C" {

int wg_tx_peers_set(wg_ctx* c, const uint32_t* slots, uint32_t n) {
  if (!c || (!slots && n)) return fail(WG_EINVAL, "NULL argument");
  if (n > c->key_slots) return fail(WG_EINVAL, "%u peers for %u key slots: a slot repeats", n, c->key_slots);
  std::vector<uint8_t> seen(c->key_slots, 0);
  for (uint32_t k = 0; k < n; ++k) {
    if (slots[k] >= c->key_slots) return fail(WG_ERANGE, "peer %u: key slot %u >= %u", k, slots[k], c->key_slots);
    if (seen[slots[k]]) return fail(WG_EINVAL, "peer %u: key slot %u repeats (it would reuse nonces)", k, slots[k]);
    seen[slots[k]] = 1;
  }
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  TxState* t;
  int rc;
  if ((rc = tx_get(c, &t)) != WG_OK) return rc;
  if ((rc = t->order.after_last(c->stream)) != WG_OK) return rc;  // no queued plan may see half of the new list
  if (n) HIPTRY(hipMemcpyAsync(t->d_peers.p, slots, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  if ((rc = t->order.mark(c->stream)) != WG_OK) return rc;
  HIPTRY(hipStreamSynchronize(c->stream));
  t->n_peers = n;
  return WG_OK;
}

int wg_routes_set(wg_ctx* c, const wg_prefix* prefixes, const uint32_t* slots, uint32_t n) {
  if (!c || ((!prefixes || !slots) && n)) return fail(WG_EINVAL, "NULL argument");
  RouteTrie t4, t6;
  for (uint32_t k = 0; k < n; ++k) {
    const wg_prefix& p = prefixes[k];
    if (slots[k] >= c->key_slots) return fail(WG_ERANGE, "route %u: key slot %u >= %u", k, slots[k], c->key_slots);
    if (p.family == 4 && p.prefix_len <= 32) t4.insert(p.addr, p.prefix_len, slots[k]);
    else if (p.family == 6 && p.prefix_len <= 128) t6.insert(p.addr, p.prefix_len, slots[k]);
    else return fail(WG_EINVAL, "route %u: family %u / length %u", k, p.family, p.prefix_len);
  }
  std::vector<uint2> ent(256, make_uint2(0u, 0u));  // node 0: "none"
  TxRouteHdr H{};
  H.root4 = route_level(t4, 0, 0, 32, ent);
  H.root6 = route_level(t6, 0, 0, 128, ent);
  H.def4 = t4.slot1[0];
  H.def6 = t6.slot1[0];
  if (ent.size() / 256 >= 0x7FFFFFFFu) return fail(WG_E2BIG, "route table too large");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  TxState* t;
  int rc;
  if ((rc = tx_get(c, &t)) != WG_OK) return rc;
  HIPTRY(hipDeviceSynchronize());  // the nodes may move: no plan launched earlier (on any stream) may still read them
  if ((rc = t->d_rent.ensure(ent.size() * sizeof(uint2))) != WG_OK) {
    (void)hipMemsetAsync(t->d_rhdr.p, 0, sizeof(TxRouteHdr), c->stream);  // the old nodes are gone: no routes
    (void)hipStreamSynchronize(c->stream);
    return rc;
  }
  H.entries = (const uint2*)t->d_rent.p;
  HIPTRY(hipMemcpyAsync(t->d_rent.p, ent.data(), ent.size() * sizeof(uint2), hipMemcpyHostToDevice, c->stream));
  HIPTRY(hipMemcpyAsync(t->d_rhdr.p, &H, sizeof H, hipMemcpyHostToDevice, c->stream));
  if ((rc = t->order.mark(c->stream)) != WG_OK) return rc;
  HIPTRY(hipStreamSynchronize(c->stream));
  return WG_OK;
}

int wg_tx_counters_set(wg_ctx* c, uint32_t first, uint32_t n, const uint64_t* counters) {
  if (!c || (!counters && n)) return fail(WG_EINVAL, "NULL argument");
  if ((uint64_t)first + n > c->key_slots) return fail(WG_ERANGE, "key slots out of range");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  TxState* t;
  int rc;
  if ((rc = tx_get(c, &t)) != WG_OK) return rc;
  if (!n) return WG_OK;
  if ((rc = t->order.after_last(c->stream)) != WG_OK) return rc;
  HIPTRY(hipMemcpyAsync((uint64_t*)t->d_send.p + first, counters, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
  if ((rc = t->order.mark(c->stream)) != WG_OK) return rc;
  HIPTRY(hipStreamSynchronize(c->stream));
  return WG_OK;
}

int wg_tx_counters_get(wg_ctx* c, uint32_t first, uint32_t n, uint64_t* counters) {
  if (!c || (!counters && n)) return fail(WG_EINVAL, "NULL argument");
  if ((uint64_t)first + n > c->key_slots) return fail(WG_ERANGE, "key slots out of range");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  TxState* t;
  int rc;
  if ((rc = tx_get(c, &t)) != WG_OK) return rc;
  if (!n) return WG_OK;
  if ((rc = t->order.after_last(c->stream)) != WG_OK) return rc;  // the counters after every queued plan
  HIPTRY(hipMemcpyAsync(counters, (uint64_t*)t->d_send.p + first, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPTRY(hipStreamSynchronize(c->stream));
  return WG_OK;
}

int wg_tx_reserve(wg_ctx* c, uint32_t max_packets) {
  if (!c) return fail(WG_EINVAL, "NULL context");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  TxState* t;
  int rc;
  if ((rc = tx_get(c, &t)) != WG_OK) return rc;
  return plan_reserve(tx_scratch_fits(c, t, max_packets), [&] { return tx_scratch_grow(c, t, max_packets); });
}

int wg_tx_plan(wg_ctx* c, const wg_tx_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  if (b->mode != WG_TX_BROADCAST && b->mode != WG_TX_ROUTE) return fail(WG_EINVAL, "unknown transmit mode %u", b->mode);
  if (b->_reserved) return fail(WG_EINVAL, "wg_tx_batch._reserved must be 0");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const bool capturing = stream_capturing(s);
  if (capturing && !c->tx)
    return fail(WG_EINVAL, "transmit plan on a capturing stream before any wg_tx_* call: call wg_tx_reserve first");
  TxState* t;
  int rc;
  if ((rc = tx_get(c, &t)) != WG_OK) return rc;
  const bool route = b->mode == WG_TX_ROUTE;
  const uint32_t n = b->n, np = route ? 1u : t->n_peers;
  if (n == 0 || np == 0) return WG_OK;
  if ((uint64_t)n * np > 0x7FFFFFFFull) return fail(WG_EINVAL, "%u packets x %u peers: at most 2^31 - 1 descriptors", n, np);
  if (!b->in || !b->pkt_off || !b->pkt_len) return fail(WG_EINVAL, "NULL tun ring or packet table");
  if (!b->desc_out || (((uintptr_t)b->desc_out) & 15u) || !b->tx_status || (((uintptr_t)b->tx_status) & 3u))
    return fail(WG_EINVAL, "descriptor / status output must be non-NULL and aligned (16 / 4 bytes)");
  // (under capture a dirty count matrix counts as scratch that does not fit)
  const bool fits = tx_scratch_fits(c, t, n) && !(capturing && t->cnt_dirty);
  if ((rc = plan_begin(t->order, s, capturing, fits, [&] { return tx_scratch_grow(c, t, n); }, kTxWords, n)) != WG_OK) return rc;
  wgtx::TxParams P{};
  P.in = b->in;
  P.in_size = b->in_size;
  P.pkt_off = b->pkt_off;
  P.pkt_len = b->pkt_len;
  P.desc = b->desc_out;
  P.status = b->tx_status;
  P.wire_base = b->wire_base;
  P.wire_stride = b->wire_stride;
  P.wire_slots = (b->wire_stride && b->wire_base <= b->out_size) ? (b->out_size - b->wire_base) / b->wire_stride : 0;
  P.n = n;
  P.max_len = b->max_len;
  P.route = route ? 1u : 0u;
  P.K = route ? c->key_slots : 1u;
  tx_geometry(n, P.K, &P.runs, &P.spr);
  P.n_peers = np;
  P.peers = (const uint32_t*)t->d_peers.p;
  P.routes = (const TxRouteHdr*)t->d_rhdr.p;
  P.send = (uint64_t*)t->d_send.p;
  P.base = (uint64_t*)t->d_base.p;
  P.code = (uint32_t*)t->d_code.p;
  P.cnt = (uint32_t*)t->d_cnt.p;
  P.pre = (uint32_t*)t->d_pre.p;
  // the count matrix is zero between plans (k_tx_scan cleans it); only after a plan whose launches
  // failed part-way it is zeroed here
  if (t->cnt_dirty) {
    HIPTRY(hipMemsetAsync(t->d_cnt.p, 0, t->d_cnt.cap, s));
    t->cnt_dirty = false;
  }
  const uint32_t wgrid = (P.runs + 3u) / 4u;
  hipLaunchKernelGGL(wgtx::k_tx_classify, dim3(wgrid), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgtx::k_tx_scan, dim3((P.K + 3u) / 4u), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgtx::k_tx_emit, dim3(wgrid), dim3(256), 0, s, P);
  return plan_end(t->order, s, capturing, kTxWords, &t->cnt_dirty);
}

}  // extern "C"
