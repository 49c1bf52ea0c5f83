// wg_session.hip — what the session layer shares (included by wg_capi.hip before wg_rxplan.hip): wg_hs_install.hip,
// wg_timers.hip and wg_endpoints.hip read one install batch, and they, wg_rxplan.hip and the sweep walk one
// receiver-index table.
//
// The installed-entry view. A ring of wg_hs_session (wg_hs_respond) or wg_hs_established (wg_hs_finish) entries, its
// count on the device and the host's slot lists are one InstView: filled in one place (inst_view, the only place that
// knows the two layouts), refused in one place (inst_batch_check) and read through inst_entry / inst_count /
// inst_slots. wg_hs_install judges the entries and writes inst_status; the two starts take what it judged
// WG_HS_INST_OK through `installed`.
//
// The index table. 8-B entries {index, high word}, bucket = mix32(index) & mask, linear probing. The high word:
//   0                 empty: a probe walk ends here.
//   key slot + 1      live (a key slot is below 0x80000000: wg_rx_sessions_reserve refuses a larger key table).
//   0x80000000 | j    transient: claimed by entry j of a running wg_hs_install, between two of its launches.
//   0xFFFFFFFF        retired: not empty (a walk goes on behind it), not a match (its index may be live behind it).
// Live is everywhere "non-zero and without the transient bit"; a retired entry carries that bit. A transient entry
// exists only inside a wg_hs_install, and every other walker of the table is ordered against an install by
// RxPlanState::order, so no retire, sweep, compaction or lookup ever meets one.
// rx_probe gives the buckets of an index in probe order, every bucket at most once; wg_rx_plan's lookup (rx_session,
// wg_rxplan.hip) keeps its own two-entries-per-round-trip walk and shares the predicates only.
#pragma once

namespace {

// ---- the index table ----------------------------------------------------------------------
constexpr uint32_t kRxRetired = 0xFFFFFFFFu;    // high word of a retired entry
constexpr uint32_t kRxTransient = 0x80000000u;  // high word 0x80000000 | j: entry j of a running wg_hs_install

struct RxSessHdr {  // at a fixed device address; a table change rewrites it (and may move the entries)
  const uint2* entries;  // capacity x {index, high word}
  uint32_t mask;         // capacity - 1; bucket = mix32(index) & mask
  uint32_t count;        // live entries
  uint32_t used;         // live + retired entries
  uint32_t _pad;
};

__host__ __device__ __forceinline__ bool rx_empty(uint32_t hi) { return hi == 0u; }
__host__ __device__ __forceinline__ bool rx_retired(uint32_t hi) { return hi == kRxRetired; }
__host__ __device__ __forceinline__ bool rx_live(uint32_t hi) { return hi != 0u && !(hi & kRxTransient); }
__host__ __device__ __forceinline__ bool rx_transient(uint32_t hi) { return (hi & kRxTransient) && hi != kRxRetired; }

// visit(bucket) for the buckets of `index` in probe order, until it returns true or every bucket has been seen once
template <class E, class Visit>
__host__ __device__ __forceinline__ void rx_probe(E* ent, uint32_t mask, uint32_t index, Visit visit) {
  uint32_t b = mix32(index);
  for (uint32_t probes = 0; probes <= mask; ++probes, ++b)
    if (visit(ent + (b & mask))) return;
}

// The live entry of `index` becomes a retired one by a 64-bit CAS, so of several threads exactly one retires it (and
// says so). With `want_hi`, only if that is still its high word: the index may have been installed again.
__device__ __forceinline__ bool rx_retire_entry(const RxSessHdr& H, uint32_t index, uint32_t want_hi) {
  bool mine = false;
  rx_probe((unsigned long long*)H.entries, H.mask, index, [&](unsigned long long* e) {
    const unsigned long long v = *e;
    const uint32_t hi = (uint32_t)(v >> 32);
    if (rx_empty(hi)) return true;
    if ((uint32_t)v != index || !rx_live(hi)) return false;
    if (!want_hi || hi == want_hi) mine = atomicCAS(e, v, wgrp::u64_of(index, kRxRetired)) == v;
    return true;
  });
  return mine;
}

// ---- the installed-entry view -------------------------------------------------------------
struct InstView {
  uint8_t* entries;  // (written by the install's WIPE only)
  const uint32_t* n_entries;
  const uint32_t* send_slot;
  const uint32_t* recv_slot;
  uint32_t n, n_slots;
  uint32_t stride, w_pos, w_peer, w_local, w_remote, q_keys;  // the entry's size, its fields as word / 16-B indices
};

// a wg_hs_install_batch, wg_timers_start_batch or wg_endpoints_start_batch
template <class Batch>
InstView inst_view(const Batch& b) {
  const bool sess = b.source == WG_HS_INSTALL_SESSIONS;
#define WG_INST_FIELD(s_field, e_field, unit) \
  (uint32_t)((sess ? offsetof(wg_hs_session, s_field) : offsetof(wg_hs_established, e_field)) / (unit))
  return InstView{(uint8_t*)b.entries, b.n_entries, b.send_slot, b.recv_slot, b.n, b.n_slots,
                  (uint32_t)(sess ? sizeof(wg_hs_session) : sizeof(wg_hs_established)),
                  WG_INST_FIELD(init, pending, 4), WG_INST_FIELD(peer, peer, 4), WG_INST_FIELD(local_index, local_index, 4),
                  WG_INST_FIELD(remote_index, remote_index, 4), WG_INST_FIELD(send_key, send_key, 16)};
#undef WG_INST_FIELD
}

// What every reader of an install batch refuses, in this order. A batch of no entries is read nowhere: only its
// source is judged.
template <class Batch>
int inst_batch_check(const Batch& b, const char* what) {
  if (b.source != WG_HS_INSTALL_SESSIONS && b.source != WG_HS_INSTALL_ESTABLISHED) return fail(WG_EINVAL, "unknown install source %u", b.source);
  if (b.n == 0) return WG_OK;
  if (b.n > 0x40000000u) return fail(WG_E2BIG, "%s of %u entries", what, b.n);
  if (!b.entries || (((uintptr_t)b.entries) & 15u)) return fail(WG_EINVAL, "entries must be non-NULL and 16-byte aligned");
  if (((uintptr_t)b.n_entries) & 3u) return fail(WG_EINVAL, "n_entries must be 4-byte aligned");
  if ((b.n_slots && (!b.send_slot || !b.recv_slot)) || ((((uintptr_t)b.send_slot) | ((uintptr_t)b.recv_slot)) & 3u))
    return fail(WG_EINVAL, "send_slot / recv_slot must be non-NULL and 4-byte aligned");
  return WG_OK;
}

__device__ __forceinline__ const uint32_t* inst_entry(const InstView& V, uint32_t j) {
  return (const uint32_t*)(V.entries + (size_t)j * V.stride);
}
__device__ __forceinline__ uint32_t inst_count(const InstView& V) { return wgrp::dev_count(V.n_entries, V.n); }

// the key slots the host chose for entry e; false: its position is past the slot lists
__device__ __forceinline__ bool inst_slots(const InstView& V, const uint32_t* e, uint32_t& s, uint32_t& r) {
  const uint32_t p = e[V.w_pos];
  if (p >= V.n_slots) return false;
  s = V.send_slot[p];
  r = V.recv_slot[p];
  return true;
}

// entry j installed a session: its slots (in a table of K) and its peer (WG_HS_NOPEER: none in a table of max_peers)
__device__ __forceinline__ bool installed(const InstView& V, const uint32_t* status, uint32_t K, uint32_t max_peers, uint32_t j,
                                          uint32_t& s, uint32_t& r, uint32_t& peer) {
  if (j >= inst_count(V) || status[j] != WG_HS_INST_OK) return false;
  const uint32_t* e = inst_entry(V, j);
  if (!inst_slots(V, e, s, r) || s >= K || r >= K || s == r) return false;
  peer = e[V.w_peer] < max_peers ? e[V.w_peer] : WG_HS_NOPEER;
  return true;
}

}  // namespace
