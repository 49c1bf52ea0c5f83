// wg_rxplan.hip — receive-side planning around open, on the device (included by wg_capi.hip).
//
// The reference's inbound path decides three things per datagram on the host before it can decipher:
// the packet class from the type byte (PacketElement.java:107-113: 1 initiation, 2 response, 4
// transport, anything else throws), the peer of a transport packet's receiver index
// (PeerList.java:53-67, an unknown index is dropped at :61-65) and that peer's session
// (TransportManager.java:70-77, none: dropped at :73-77); UndecryptedIncomingTransport.java:20-33 then
// cuts the packet into counter, ciphertext and the plaintext's place (:30). After decipher,
// TransportManager.processDecryptedTransport (TransportManager.java:98-119) queues what goes to the tun
// device, one packet at a time. wg_rx_plan does the first part for a whole UDP ring and writes the
// wg_pkt descriptors wg_open_batch takes; wg_rx_deliver does the last and writes the list of tun
// writes in arrival order. The host handles the handshake messages the plan lists, and nothing else.
//
// Sessions. receiver index -> key slot is an open-addressing hash table built on the host
// (wg_rx_sessions_set): capacity = the smallest power of two >= max(16, 4 n), 8-B entries {index,
// key slot + 1} (0: empty), bucket = mix(index) & mask with MurmurHash3's 32-bit finaliser as mix (the
// reference's indices are 0, 1, 2, ..., WireGuard's are random, a test's may be multiples of anything: the
// finaliser spreads them all), linear probing; at most a quarter full, so a probe sequence is short (a
// wave walks as long as the longest of its 64) and ends at an empty entry. Its header sits at a fixed
// device address and names the entries (wg_plan.hip, fixed headers). The entry's encoding, its predicates and the
// probe that every walker but the plan's own lookup uses are wg_session.hip's.
//
// A table the device can change. wg_rx_sessions_reserve gives the table a fixed capacity C of the context's
// own entries; wg_hs_install (wg_hs_install.hip) then inserts into it and wg_rx_sessions_retire turns a live
// entry into a retired one, {index, 0xFFFFFFFF}: not empty (a probe walk goes on behind it), not a match.
// `used` counts live + retired entries and never exceeds C / 2, which bounds every walk; a rebuild on the
// host (wg_rx_sessions_set, wg_rx_sessions_reserve) drops the retired ones, and so does wg_rx_sessions_compact
// on the device. A context that never reserves builds exactly the tables it built before there was a reserve.
//
// Compaction. Every kernel reads the entries through the header, so the live entries are rehashed into a second
// buffer of the same capacity (the spare, allocated with the reserve) and the header's pointer is flipped; nothing
// is copied back. Both buffers' addresses sit beside the control words at a fixed device address, and which of
// them is the spare is decided on the device, by what the header names, so nothing about a call lives on the host
// and a captured compaction replays in either parity, and after a host rebuild that moved the buffers. Three launches,
// ordered by kernel boundaries, no workgroup waiting for another:
//   k_rx_compact_clear   the whole spare = empty (16-B stores), in every call, needed or not: the spare holds the
//                  table of two compactions ago, and an entry left there would bring a retired index back.
//                  One thread writes the decision and the counts into the control words.
//   k_rx_compact_rehash  one thread per bucket of the current table (a wave reads 512 contiguous bytes): a live
//                  entry claims the first empty bucket of its probe sequence in the spare by a 64-bit
//                  compare-and-swap against 0. Live indices are unique, so there is nothing to deduplicate;
//                  which bucket of a chain an entry gets depends on thread order, what a lookup answers does not.
//   k_rx_compact_flip    one thread: entries = the spare, used = count; the summary.
//
// Ranks. The plan needs two stable ranks over the batch (the handshake list, the 64-bit prefix of the
// packed plaintext offsets) and the deliver one (the item list). Both are a rank_launch of wg_plan.hip,
// with no wait between workgroups (no spin on another block's flag, no assumption about dispatch order):
//   k_rx_classify / k_rx_merge  one packet per thread, kRankRange = 256 packets per workgroup: the
//                  checks (type byte, probe, header loads; the merge of the two statuses), the
//                  packet's code to scratch so that none of it is done twice, and the workgroup's
//                  sums {bytes, count, count} as ONE 16-B record of the partials array.
//   k_rx_scan      one workgroup walks the partials in chunks of 256, replaces every record by the
//                  exclusive prefix of the records before it, and writes the totals as the summary.
//   k_rx_emit / k_rx_items  the same ranges: rank = the range's prefix + a ballot / scan inside the
//                  workgroup; descriptors as two 16-B stores, items as one.
// What one launch leaves for the next is ordered by the kernel boundary. Every scratch word (code,
// partials) is written by the first launch of a call before a later one reads it, nothing is carried
// from call to call and nothing about a call lives on the host, so a captured plan or deliver replays
// any number of times. In packed mode a packet can fail only once its offset is known (it does not fit
// pt_size), so n_open is summed by the emit launch: the scan writes it as 0 and every workgroup adds
// its count with one atomic (a few hundred adds per 65,536 packets).
#pragma once

namespace {

struct RxInstCtl {  // wg_hs_install's words between its launches (written by its first launch in every call)
  uint32_t used0, n_cand, n_badslot, n_dup;
};

struct RxCompactCtl {  // at a fixed device address
  uint32_t go, live, dropped, _pad;  // the compaction's words between its launches (written by its first launch in every call)
  uint2* buf[2];  // the table's two buffers, written by the host with every table it builds: the header names one,
                  // the other is the spare. (Here and not in the launch: a captured compaction follows a table that moved.)
};

struct RxPlanState {
  DevBuf d_hdr;    // RxSessHdr (fixed address)
  DevBuf d_empty;  // 16 empty entries: the table of a context without sessions
  DevBuf d_ent;    // the entries a host rebuild writes: the current table, or (after a compaction) the spare
  DevBuf d_ent2;   // reserved tables only: the other buffer, of the table's capacity (the device knows which is which)
  uint32_t capacity = 16;  // of the table the host last built (the compaction's grid; its kernels read the header's)
  DevBuf d_code;   // per packet: {status, key slot, counter lo, counter hi}
  DevBuf d_part;   // per workgroup: {bytes lo, bytes hi, count, count}, then their exclusive prefixes
  uint32_t reserved = 0;  // wg_rx_sessions_reserve's capacity C (0: never reserved)
  DevBuf d_claim;  // wg_hs_install: per key slot, the lowest entry that names it
  DevBuf d_ctl;    // wg_hs_install: RxInstCtl
  DevBuf d_cmp;    // wg_rx_sessions_compact: RxCompactCtl
  StreamOrder order;  // last plan / deliver / table write
};

const PlanWords kRxPlanWords{"receive plan", "packets", "wg_rx_reserve"};
const PlanWords kRxDeliverWords{"receive deliver", "packets", "wg_rx_reserve"};
const PlanWords kRxRetireWords{"session retire", "indices", "wg_rx_sessions_reserve"};
const PlanWords kRxCompactWords{"session compaction", "entries", "wg_rx_sessions_reserve"};

uint32_t rxp_capacity(uint32_t n) {  // the smallest power of two >= max(16, 4 n)
  uint32_t cap = 16;
  while ((uint64_t)cap < 4ull * n) cap <<= 1;
  return cap;
}

// a reserved table keeps the context's own entries even when it is empty: the device inserts into them
void rxp_header(const RxPlanState* t, uint32_t n, bool own, RxSessHdr* H) {
  const uint32_t cap = own ? std::max(rxp_capacity(n), t->reserved) : 16u;
  H->entries = (const uint2*)(own ? t->d_ent.p : t->d_empty.p);
  H->mask = cap - 1u;
  H->count = own ? n : 0u;
  H->used = H->count;
  H->_pad = 0u;
}

// The receive-plan state, allocated at the first wg_rx_sessions_set / wg_rx_reserve / wg_rx_plan /
// wg_rx_deliver call. Caller holds c->mu.
int rxp_get(wg_ctx* c, RxPlanState** out) {
  if (!c->rxp) {
    auto t = std::make_unique<RxPlanState>();
    int rc;
    if ((rc = t->d_hdr.ensure(sizeof(RxSessHdr))) != WG_OK || (rc = t->d_empty.ensure(16 * sizeof(uint2))) != WG_OK) return rc;
    RxSessHdr H;
    rxp_header(t.get(), 0, false, &H);
    hipError_t e = t->order.create();
    if (e == hipSuccess) e = hipMemsetAsync(t->d_empty.p, 0, 16 * sizeof(uint2), c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(t->d_hdr.p, &H, sizeof H, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(WG_EDEVICE, "receive plan state: %s", hipGetErrorString(e));
    c->rxp = t.release();
  }
  *out = c->rxp;
  return WG_OK;
}

void rxp_free(wg_ctx* c) {
  delete c->rxp;
  c->rxp = nullptr;
}

// scratch for batches of up to n packets: does it fit, and (plan_reserve) its growth
bool rxp_scratch_fits(const RxPlanState* t, uint32_t n) {
  return (size_t)std::max(n, 1u) * 16 <= t->d_code.cap && (size_t)std::max(rank_blocks(n), 1u) * 16 <= t->d_part.cap;
}
int rxp_scratch_grow(RxPlanState* t, uint32_t n) {
  const int rc = t->d_code.ensure((size_t)std::max(n, 1u) * 16);
  return rc != WG_OK ? rc : t->d_part.ensure((size_t)std::max(rank_blocks(n), 1u) * 16);
}
int rxp_begin(RxPlanState* t, hipStream_t s, bool capturing, uint32_t n, const PlanWords& w) {
  return plan_begin(t->order, s, capturing, rxp_scratch_fits(t, n), [&] { return rxp_scratch_grow(t, n); }, w, n);
}

// Replaces the whole table by n live entries (host pointers), built on the host; nothing changes on a bad
// argument. Synchronous. Caller holds c->mu and the device.
int rxp_table_set(wg_ctx* c, RxPlanState* t, const uint32_t* indices, const uint32_t* slots, uint32_t n) {
  const bool own = n != 0 || t->reserved != 0;
  RxSessHdr H;
  rxp_header(t, n, own, &H);
  std::vector<uint2> ent(own ? (size_t)H.mask + 1 : 0, make_uint2(0u, 0u));
  for (uint32_t k = 0; k < n; ++k) {
    if (slots[k] >= c->key_slots) return fail(WG_ERANGE, "session %u: key slot %u >= %u", k, slots[k], c->key_slots);
    bool placed = false;  // (n entries in >= 4 n buckets: the walk ends at an empty one)
    rx_probe(ent.data(), H.mask, indices[k], [&](uint2* e) {
      if (rx_empty(e->y)) {
        *e = make_uint2(indices[k], slots[k] + 1u);
        placed = true;
      }
      return placed || e->x == indices[k];
    });
    if (!placed) return fail(WG_EINVAL, "session %u: receiver index 0x%08x repeats", k, indices[k]);
  }
  int rc;
  HIPTRY(hipDeviceSynchronize());  // the entries may move: no plan launched earlier (on any stream) may still read them
  if (own) {
    // (a reserved table keeps its spare at the table's capacity: a capturing compaction cannot allocate)
    if ((rc = t->d_ent.ensure(ent.size() * sizeof(uint2))) != WG_OK ||
        (t->reserved && (rc = t->d_ent2.ensure(ent.size() * sizeof(uint2))) != WG_OK)) {
      t->reserved = 0;
      rxp_header(t, 0, false, &H);  // the old entries are gone: no sessions, no reserve
      (void)hipMemcpyAsync(t->d_hdr.p, &H, sizeof H, hipMemcpyHostToDevice, c->stream);
      (void)hipStreamSynchronize(c->stream);
      t->capacity = 16;
      return rc;
    }
    H.entries = (const uint2*)t->d_ent.p;
    HIPTRY(hipMemcpyAsync(t->d_ent.p, ent.data(), ent.size() * sizeof(uint2), hipMemcpyHostToDevice, c->stream));
    if (t->reserved) {  // (wg_rx_sessions_reserve has allocated the control block)
      uint2* const both[2] = {(uint2*)t->d_ent.p, (uint2*)t->d_ent2.p};
      HIPTRY(hipMemcpyAsync((uint8_t*)t->d_cmp.p + offsetof(RxCompactCtl, buf), both, sizeof both, hipMemcpyHostToDevice, c->stream));
    }
  }
  HIPTRY(hipMemcpyAsync(t->d_hdr.p, &H, sizeof H, hipMemcpyHostToDevice, c->stream));
  t->capacity = H.mask + 1u;
  if ((rc = t->order.mark(c->stream)) != WG_OK) return rc;
  HIPTRY(hipStreamSynchronize(c->stream));
  return WG_OK;
}

}  // namespace

// ---- device -------------------------------------------------------------------------------
namespace wgrp {

struct RxPlanParams {
  const uint8_t* wire;
  uint64_t wire_size;
  const uint64_t* pkt_off;
  const uint32_t* pkt_len;
  wg_pkt* desc;
  uint32_t* status;
  uint32_t* host_list;
  wg_rx_summary* summary;
  uint64_t pt_base;
  uint64_t pt_room;  // packed: bytes from pt_base to the end of the buffer
  uint32_t n, max_len, packed;
  uint32_t pt_ok;    // packed: pt_base lies inside the buffer (otherwise nothing fits, not even a keepalive)
  const RxSessHdr* sessions;
  uint4* code;
  uint4* part;
};

struct RxDeliverParams {
  const wg_pkt* desc;
  const uint32_t* plan_status;
  const uint32_t* open_status;
  uint32_t* final_status;
  wg_rx_item* items;
  uint32_t* index_out;
  wg_rx_delivered* delivered;
  uint32_t n;
  uint4* part;
};

// key slot + 1 of a receiver index, 0 if the table does not hold it. Two entries of the probe sequence
// are fetched per round trip (each one 8-B load): a wave walks as long as its longest chain. A retired
// entry is walked over: it is not empty, and it does not match (its index may be live again behind it).
__device__ __forceinline__ uint32_t rx_session(const RxSessHdr& H, uint32_t index) {
  const uint64_t* ent = (const uint64_t*)H.entries;  // {index, key slot + 1} = low, high word
  uint32_t b = mix32(index);
  for (uint32_t probes = 0; probes <= H.mask; probes += 2u) {  // (a table at most half full ends the walk long before)
    const uint64_t e0 = ent[b & H.mask], e1 = ent[(b + 1u) & H.mask];
    const uint32_t h0 = (uint32_t)(e0 >> 32), h1 = (uint32_t)(e1 >> 32);
    if (rx_empty(h0)) return 0u;
    if ((uint32_t)e0 == index && !rx_retired(h0)) return h0;
    if (rx_empty(h1)) return 0u;
    if ((uint32_t)e1 == index && !rx_retired(h1)) return h1;
    b += 2u;
  }
  return 0u;
}

// One index per thread; of equal indices in one call exactly one thread retires the entry (and counts it).
__global__ void __launch_bounds__(256) k_rx_retire(RxSessHdr* hdr, const uint32_t* indices, uint32_t n, uint32_t* n_retired) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const RxSessHdr H = *hdr;
  bool mine = false;
  if (i < n) mine = rx_retire_entry(H, indices[i], 0u);
  uint32_t r, total;
  block_rank(mine, s_cnt, r, total);
  if (threadIdx.x == 0 && total) {
    atomicSub(&hdr->count, total);
    if (n_retired) atomicAdd(n_retired, total);
  }
}

// ---- compaction ----
struct RxCompactParams {
  RxSessHdr* hdr;
  RxCompactCtl* ctl;          // the control words and the table's two buffers
  wg_rx_compact_summary* summary;  // NULL: none (the install's)
  const uint32_t* n_entries;  // install: the ring's count on the device (NULL: all n)
  uint32_t n;                 // install: entries of the ring
  uint32_t min_retired;       // wg_rx_sessions_compact: the threshold
  uint32_t install;           // decided by the install's rule instead
};

__device__ __forceinline__ uint2* rx_spare(const RxCompactParams& P, const uint2* current) {
  uint2* const b0 = P.ctl->buf[0];
  return b0 == current ? P.ctl->buf[1] : b0;
}

// The whole spare = empty, two entries per 16-B store; thread 0 decides. wg_rx_sessions_compact: retired >=
// max(min_retired, 1). wg_hs_install(COMPACT): the ring would not fit (used + m > C / 2) and there is something to drop.
__global__ void __launch_bounds__(256) k_rx_compact_clear(RxCompactParams P) {
  const RxSessHdr H = *P.hdr;
  uint4* spare = (uint4*)rx_spare(P, H.entries);
  const uint32_t pairs = (uint32_t)(((uint64_t)H.mask + 1u) / 2u);  // (a capacity is a power of two >= 16)
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < pairs; i += gridDim.x * 256u) spare[i] = make_uint4(0u, 0u, 0u, 0u);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint32_t retired = H.used - H.count;
    bool go;
    if (P.install) go = retired != 0u && (uint64_t)H.used + dev_count(P.n_entries, P.n) > ((uint64_t)H.mask + 1u) / 2u;
    else go = retired >= (P.min_retired ? P.min_retired : 1u);
    *(uint4*)P.ctl = make_uint4(go ? 1u : 0u, H.count, go ? retired : 0u, 0u);
  }
}

// One bucket of the current table per thread. The walk is bounded by the capacity; the spare holds at most
// `count` <= C / 2 entries, so it ends long before.
__global__ void __launch_bounds__(256) k_rx_compact_rehash(RxCompactParams P) {
  if (!P.ctl->go) return;
  const RxSessHdr H = *P.hdr;
  const unsigned long long* cur = (const unsigned long long*)H.entries;
  unsigned long long* spare = (unsigned long long*)rx_spare(P, H.entries);
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i <= H.mask; i += (uint64_t)gridDim.x * 256u) {
    const unsigned long long v = cur[i];
    if (!rx_live((uint32_t)(v >> 32))) continue;
    rx_probe(spare, H.mask, (uint32_t)v, [v](unsigned long long* e) { return atomicCAS(e, 0ull, v) == 0ull; });
  }
}

__global__ void k_rx_compact_flip(RxCompactParams P) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const uint4 w = *(const uint4*)P.ctl;
  const RxCompactCtl C{w.x, w.y, w.z, 0u, {nullptr, nullptr}};
  if (C.go) {
    P.hdr->entries = rx_spare(P, P.hdr->entries);
    P.hdr->used = C.live;
  }
  if (P.summary) {  // (8-B stores: the summary need not be 16-B aligned)
    uint2* sum = (uint2*)P.summary;
    sum[0] = make_uint2(C.live, C.dropped);
    sum[1] = make_uint2(C.go, 0u);
  }
}

// Steps 1-5 of wg_rx_plan and, in AFTER mode, step 6; writes the packet's code and the range's sums.
__global__ void __launch_bounds__(256) k_rx_classify(RxPlanParams P) {
  __shared__ uint32_t s_cnt[2][4];
  __shared__ uint64_t s_sum[4];
  const uint32_t i = blockIdx.x * kRankRange + threadIdx.x;
  const bool in = i < P.n;
  const RxSessHdr H = *P.sessions;
  uint32_t st = WG_PKT_BADHDR, slot = 0, len = 0, c_lo = 0, c_hi = 0;
  if (in) {
    const uint64_t o = P.pkt_off[i];
    const uint32_t wl = P.pkt_len[i];
    if (wl != 0 && o <= P.wire_size && (uint64_t)wl <= P.wire_size - o) {
      const uint8_t* h = P.wire + o;
      // the whole header in one round trip where the packet holds one (a shorter one: its type byte)
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      if (wl >= 16u) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = wgt::load_u32_any(h + 4 * k);
      } else {
        w[0] = h[0];
      }
      const uint32_t t = w[0] & 0xffu;
      if (t == 1u || t == 2u) {
        st = WG_PKT_HANDSHAKE;
      } else if (t == 4u && wl >= 32u) {
        const uint32_t hit = rx_session(H, w[1]);
        len = wl - 32u;
        if (!hit) {
          st = WG_PKT_NOSESSION;
        } else {
          slot = hit - 1u;
          if (len > P.max_len) st = WG_PKT_TOOLONG;
          else if (!P.packed && (uint64_t)len > P.wire_size - o - wl) st = WG_PKT_BADHDR;  // the plaintext overruns the ring
          else {
            st = WG_PKT_OK;
            c_lo = w[2];
            c_hi = w[3];
          }
        }
      }
    }
    P.code[i] = make_uint4(st, slot, c_lo, c_hi);
  }
  const bool ok = in && st == WG_PKT_OK;
  uint32_t r0, r1, n_ok, n_host;
  uint64_t ex, bytes;
  block_rank(ok && !P.packed, s_cnt[0], r0, n_ok);
  block_rank(in && st == WG_PKT_HANDSHAKE, s_cnt[1], r1, n_host);
  block_scan64(ok && P.packed ? ((uint64_t)len + 15u) & ~15ull : 0ull, s_sum, ex, bytes);
  if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4((uint32_t)bytes, (uint32_t)(bytes >> 32), n_ok, n_host);
}

__global__ void __launch_bounds__(256) k_rx_emit(RxPlanParams P) {
  __shared__ uint32_t s_cnt[2][4];
  __shared__ uint64_t s_sum[4];
  const uint32_t i = blockIdx.x * kRankRange + threadIdx.x;
  const bool in = i < P.n;
  const uint4 c = in ? P.code[i] : make_uint4(WG_PKT_BADHDR, 0u, 0u, 0u);
  const uint64_t o = in ? P.pkt_off[i] : 0ull;
  const uint32_t wl = in ? P.pkt_len[i] : 0u;
  const uint4 pre = P.part[blockIdx.x];
  uint32_t st = c.x;
  const uint32_t len = wl - 32u;  // (meaningful where the code is WG_PKT_OK)
  const bool pass = in && st == WG_PKT_OK;
  uint64_t ex, tot;
  block_scan64(pass && P.packed ? ((uint64_t)len + 15u) & ~15ull : 0ull, s_sum, ex, tot);
  uint64_t out_off = P.packed ? P.pt_base : o + wl;
  if (pass && P.packed) {
    const uint64_t C = u64_of(pre.x, pre.y) + ex;
    if (P.pt_ok && C <= P.pt_room && (uint64_t)len <= P.pt_room - C) out_off = P.pt_base + C;
    else st = WG_PKT_TOOLONG;
  }
  const bool ok = in && st == WG_PKT_OK;
  uint32_t hr, n_host, kr, n_ok;
  block_rank(in && st == WG_PKT_HANDSHAKE, s_cnt[0], hr, n_host);
  block_rank(ok, s_cnt[1], kr, n_ok);
  if (P.packed && threadIdx.x == 0 && n_ok) atomicAdd(&P.summary->n_open, n_ok);
  if (!in) return;
  const uint64_t in_off = o + 16u;
  uint4* d = (uint4*)(P.desc + i);
  d[0] = make_uint4((uint32_t)in_off, (uint32_t)(in_off >> 32), (uint32_t)out_off, (uint32_t)(out_off >> 32));
  d[1] = ok ? make_uint4(c.z, c.w, len, c.y) : make_uint4(0u, 0u, WG_LEN_INVALID, c.y);
  P.status[i] = st;
  if (st == WG_PKT_HANDSHAKE) P.host_list[pre.w + hr] = i;
}

// final status = the plan's unless that is WG_PKT_OK, then the open's; the range's sums
__global__ void __launch_bounds__(256) k_rx_merge(RxDeliverParams P) {
  __shared__ uint32_t s_cnt[2][4];
  __shared__ uint64_t s_sum[4];
  const uint32_t i = blockIdx.x * kRankRange + threadIdx.x;
  const bool in = i < P.n;
  uint32_t st = WG_PKT_BADHDR, len = 0;
  if (in) {
    const uint32_t ps = P.plan_status[i];
    st = ps != WG_PKT_OK ? ps : P.open_status[i];
    P.final_status[i] = st;
    if (st == WG_PKT_OK) len = P.desc[i].len;
  }
  uint32_t r0, r1, n_items, n_keep;
  uint64_t ex, bytes;
  block_rank(in && st == WG_PKT_OK, s_cnt[0], r0, n_items);
  block_rank(in && st == WG_PKT_KEEPALIVE, s_cnt[1], r1, n_keep);
  block_scan64((uint64_t)len, s_sum, ex, bytes);
  if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4((uint32_t)bytes, (uint32_t)(bytes >> 32), n_items, n_keep);
}

__global__ void __launch_bounds__(256) k_rx_items(RxDeliverParams P) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t i = blockIdx.x * kRankRange + threadIdx.x;
  const bool in = i < P.n;
  const bool ok = in && P.final_status[i] == WG_PKT_OK;
  const uint4 pre = P.part[blockIdx.x];
  uint32_t r, total;
  block_rank(ok, s_cnt, r, total);
  if (!ok) return;
  const uint4* d = (const uint4*)(P.desc + i);
  const uint4 a = d[0], b = d[1];
  const uint32_t j = pre.z + r;
  *(uint4*)(P.items + j) = make_uint4(a.z, a.w, b.z, b.w);
  if (P.index_out) P.index_out[j] = i;
}

}  // namespace wgrp

namespace {

// The compaction's three launches on s, for a reserved table (both buffers and the control block exist). The grids
// follow the capacity the host last built; the kernels stride over the header's, and take the buffers from the
// control block, whatever they are when they run.
void rxp_compact_launch(RxPlanState* t, hipStream_t s, wgrp::RxCompactParams P) {
  P.hdr = (RxSessHdr*)t->d_hdr.p;
  P.ctl = (RxCompactCtl*)t->d_cmp.p;
  hipLaunchKernelGGL(wgrp::k_rx_compact_clear, dim3(std::max(1u, rank_blocks(t->capacity / 2u))), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgrp::k_rx_compact_rehash, dim3(std::max(1u, rank_blocks(t->capacity))), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgrp::k_rx_compact_flip, dim3(1), dim3(64), 0, s, P);
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------
extern "C" {

int wg_rx_sessions_compact(wg_ctx* c, uint32_t min_retired, wg_rx_compact_summary* summary_dev, void* stream) {
  if (!c) return fail(WG_EINVAL, "NULL context");
  if (((uintptr_t)summary_dev) & 7u) return fail(WG_EINVAL, "summary must be 8-byte aligned");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  RxPlanState* t = c->rxp;
  if (!t || !t->reserved) return fail(WG_EINVAL, "wg_rx_sessions_compact before wg_rx_sessions_reserve");
  const bool capturing = stream_capturing(s);
  int rc;
  if (!capturing && (rc = t->order.after_last(s)) != WG_OK) return rc;
  wgrp::RxCompactParams P{};
  P.summary = summary_dev;
  P.min_retired = min_retired;
  rxp_compact_launch(t, s, P);
  return plan_end(t->order, s, capturing, kRxCompactWords);
}

int wg_rx_sessions_set(wg_ctx* c, const uint32_t* indices, const uint32_t* slots, uint32_t n) {
  if (!c || ((!indices || !slots) && n)) return fail(WG_EINVAL, "NULL argument");
  if (n > 0x20000000u) return fail(WG_E2BIG, "session table of %u entries", n);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  RxPlanState* t;
  int rc;
  if ((rc = rxp_get(c, &t)) != WG_OK) return rc;
  return rxp_table_set(c, t, indices, slots, n);
}

int wg_rx_sessions_reserve(wg_ctx* c, uint32_t max_sessions) {
  if (!c) return fail(WG_EINVAL, "NULL context");
  if (max_sessions > 0x20000000u) return fail(WG_E2BIG, "session table of %u entries", max_sessions);
  if (c->key_slots >= kRxTransient) return fail(WG_EINVAL, "key table too large for a device-owned session table");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  RxPlanState* t;
  int rc;
  if ((rc = rxp_get(c, &t)) != WG_OK) return rc;
  if ((rc = t->d_claim.ensure((size_t)c->key_slots * 4)) != WG_OK || (rc = t->d_ctl.ensure(sizeof(RxInstCtl))) != WG_OK ||
      (rc = t->d_cmp.ensure(sizeof(RxCompactCtl))) != WG_OK)
    return rc;
  // the live entries of the current table, in table order (retired ones are dropped by the rebuild)
  HIPTRY(hipDeviceSynchronize());
  RxSessHdr H;
  HIPTRY(hipMemcpy(&H, t->d_hdr.p, sizeof H, hipMemcpyDeviceToHost));
  std::vector<uint2> old(H.used ? (size_t)H.mask + 1 : 0);
  if (!old.empty()) HIPTRY(hipMemcpy(old.data(), H.entries, old.size() * sizeof(uint2), hipMemcpyDeviceToHost));
  std::vector<uint32_t> indices, slots;
  for (const uint2& e : old)
    if (rx_live(e.y)) {
      indices.push_back(e.x);
      slots.push_back(e.y - 1u);
    }
  const uint32_t before = t->reserved;
  t->reserved = rxp_capacity(max_sessions);
  if ((rc = rxp_table_set(c, t, indices.data(), slots.data(), (uint32_t)indices.size())) != WG_OK && t->reserved) t->reserved = before;
  return rc;
}

int wg_rx_sessions_retire(wg_ctx* c, const uint32_t* indices_dev, uint32_t n, uint32_t* n_retired_dev, void* stream) {
  if (!c || (!indices_dev && n)) return fail(WG_EINVAL, "NULL argument");
  if ((((uintptr_t)indices_dev) | ((uintptr_t)n_retired_dev)) & 3u) return fail(WG_EINVAL, "indices / n_retired must be 4-byte aligned");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const bool capturing = stream_capturing(s);
  if (capturing && !c->rxp)
    return fail(WG_EINVAL, "session retire on a capturing stream before any wg_rx_* planning call: call wg_rx_sessions_reserve first");
  RxPlanState* t;
  int rc;
  if ((rc = rxp_get(c, &t)) != WG_OK) return rc;
  if (!capturing && (rc = t->order.after_last(s)) != WG_OK) return rc;
  if (n_retired_dev) HIPTRY(hipMemsetAsync(n_retired_dev, 0, 4, s));
  if (n) hipLaunchKernelGGL(wgrp::k_rx_retire, dim3(rank_blocks(n)), dim3(256), 0, s, (RxSessHdr*)t->d_hdr.p, indices_dev, n, n_retired_dev);
  return plan_end(t->order, s, capturing, kRxRetireWords);
}

int wg_rx_sessions_count(wg_ctx* c, uint32_t* live, uint32_t* retired) {
  if (!c) return fail(WG_EINVAL, "NULL context");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  RxSessHdr H{};
  if (c->rxp) {
    HIPTRY(hipDeviceSynchronize());  // after everything queued, on any stream
    HIPTRY(hipMemcpy(&H, c->rxp->d_hdr.p, sizeof H, hipMemcpyDeviceToHost));
  }
  if (live) *live = H.count;
  if (retired) *retired = H.used - H.count;
  return WG_OK;
}

int wg_rx_reserve(wg_ctx* c, uint32_t max_packets) {
  if (!c) return fail(WG_EINVAL, "NULL context");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  RxPlanState* t;
  int rc;
  if ((rc = rxp_get(c, &t)) != WG_OK) return rc;
  return plan_reserve(rxp_scratch_fits(t, max_packets), [&] { return rxp_scratch_grow(t, max_packets); });
}

int wg_rx_plan(wg_ctx* c, const wg_rx_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  if (b->mode != WG_RX_PT_AFTER && b->mode != WG_RX_PT_PACKED) return fail(WG_EINVAL, "unknown receive mode %u", b->mode);
  if (b->_reserved) return fail(WG_EINVAL, "wg_rx_batch._reserved must be 0");
  if (!b->summary || (((uintptr_t)b->summary) & 7u)) return fail(WG_EINVAL, "summary must be non-NULL and 8-byte aligned");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const bool capturing = stream_capturing(s);
  if (capturing && !c->rxp)
    return fail(WG_EINVAL, "receive plan on a capturing stream before any wg_rx_* planning call: call wg_rx_reserve first");
  RxPlanState* t;
  int rc;
  if ((rc = rxp_get(c, &t)) != WG_OK) return rc;
  const uint32_t n = b->n;
  if (n == 0) {
    HIPTRY(hipMemsetAsync(b->summary, 0, sizeof(wg_rx_summary), s));
    return WG_OK;
  }
  if (!b->wire || !b->pkt_off || !b->pkt_len) return fail(WG_EINVAL, "NULL wire ring or packet table");
  if (!b->desc_out || (((uintptr_t)b->desc_out) & 15u) || !b->rx_status || (((uintptr_t)b->rx_status) & 3u) ||
      !b->host_list || (((uintptr_t)b->host_list) & 3u))
    return fail(WG_EINVAL, "descriptor / status / host list output must be non-NULL and aligned (16 / 4 / 4 bytes)");
  if ((rc = rxp_begin(t, s, capturing, n, kRxPlanWords)) != WG_OK) return rc;
  wgrp::RxPlanParams P{};
  P.wire = b->wire;
  P.wire_size = b->wire_size;
  P.pkt_off = b->pkt_off;
  P.pkt_len = b->pkt_len;
  P.desc = b->desc_out;
  P.status = b->rx_status;
  P.host_list = b->host_list;
  P.summary = b->summary;
  P.packed = b->mode == WG_RX_PT_PACKED ? 1u : 0u;
  P.pt_base = P.packed ? b->pt_base : 0;
  P.pt_ok = (P.packed && b->pt_base <= b->pt_size) ? 1u : 0u;
  P.pt_room = P.pt_ok ? b->pt_size - b->pt_base : 0;
  P.n = n;
  P.max_len = b->max_len;
  P.sessions = (const RxSessHdr*)t->d_hdr.p;
  P.code = (uint4*)t->d_code.p;
  P.part = (uint4*)t->d_part.p;
  rank_launch(wgrp::k_rx_classify, wgrp::k_rx_emit, P, b->summary, s);
  return plan_end(t->order, s, capturing, kRxPlanWords);
}

int wg_rx_deliver(wg_ctx* c, const wg_rx_deliver_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  if (b->_reserved) return fail(WG_EINVAL, "wg_rx_deliver_batch._reserved must be 0");
  if (!b->delivered || (((uintptr_t)b->delivered) & 7u)) return fail(WG_EINVAL, "delivered must be non-NULL and 8-byte aligned");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const bool capturing = stream_capturing(s);
  if (capturing && !c->rxp)
    return fail(WG_EINVAL, "receive deliver on a capturing stream before any wg_rx_* planning call: call wg_rx_reserve first");
  RxPlanState* t;
  int rc;
  if ((rc = rxp_get(c, &t)) != WG_OK) return rc;
  const uint32_t n = b->n;
  if (n == 0) {
    HIPTRY(hipMemsetAsync(b->delivered, 0, sizeof(wg_rx_delivered), s));
    return WG_OK;
  }
  if (!b->desc || (((uintptr_t)b->desc) & 15u) || !b->plan_status || !b->open_status || !b->final_status)
    return fail(WG_EINVAL, "NULL (or unaligned) descriptor or status array");
  if (b->final_status == b->plan_status || b->final_status == b->open_status)
    return fail(WG_EINVAL, "final_status may alias neither plan_status nor open_status");
  if (!b->items || (((uintptr_t)b->items) & 15u) || (((uintptr_t)b->index_out) & 3u))
    return fail(WG_EINVAL, "items must be non-NULL and 16-byte aligned (index_out: 4-byte)");
  if ((rc = rxp_begin(t, s, capturing, n, kRxDeliverWords)) != WG_OK) return rc;
  wgrp::RxDeliverParams P{};
  P.desc = b->desc;
  P.plan_status = b->plan_status;
  P.open_status = b->open_status;
  P.final_status = b->final_status;
  P.items = b->items;
  P.index_out = b->index_out;
  P.delivered = b->delivered;
  P.n = n;
  P.part = (uint4*)t->d_part.p;
  rank_launch(wgrp::k_rx_merge, wgrp::k_rx_items, P, b->delivered, s);
  return plan_end(t->order, s, capturing, kRxDeliverWords);
}

}  // extern "C"
