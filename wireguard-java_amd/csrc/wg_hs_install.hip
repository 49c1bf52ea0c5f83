// wg_hs_install.hip — handshake results become transport sessions, on the device (included by wg_capi.hip).
//
// wg_hs_respond leaves wg_hs_session entries and wg_hs_finish wg_hs_established ones; both carry send_key,
// recv_key, local_index and remote_index. The reference hands them to the transport path on the host
// (SessionManager.setSession: a new EstablishedSession around a new SymmetricKeypair, PeerList's index ->
// peer array). wg_hs_install does that for a ring of entries without a key leaving the device: the keys go
// into the key table, {local_index -> recv slot} into the receive plan's session table
// (wg_rxplan.hip, reserved by wg_rx_sessions_reserve), remote_index into the framer's receiver table, and the
// slots' send counters and replay windows start again, as wg_keys_set starts them. The next wg_tx_plan /
// wg_rx_plan on the same stream already uses the sessions.
//
// The key slots of an entry are the host's choice, made before the handshake chain is launched: send_slot[p],
// recv_slot[p] with p = the position under which the host chose that handshake's local_index (sessions[j].init,
// established[j].pending). Nothing is read back to pick them. The ring is read through wg_session.hip's InstView, as
// wg_timers_start and wg_endpoints_start read it afterwards; the table's encoding and probe are that file's too.
//
// Five launches on the call's stream; a kernel boundary orders each behind the one before, no workgroup waits
// for another, and which of several equal slots or indices wins (the lowest entry) depends on no dispatch order:
//   k_inst_fill    the claim word of every key slot of the call's range = none; the control words.
//   k_inst_claim   step 1 per entry; an entry that passes leaves its position in both slots' claim words by
//                  atomicMin, so a word ends as the lowest entry that names the slot.
//   k_inst_insert  step 2 (both claim words are mine) and step 3: the entry walks its index's probe sequence in
//                  the session table. A live entry of that index: DUPINDEX. An empty one: atomicCAS places the
//                  transient entry {index, 0x80000000 | j}. A transient one of that index: atomicMin on the
//                  64-bit entry (same low word: the lower j stays). An index thus has one bucket, whoever came
//                  first, and the entry notes the bucket in its status word.
//   k_inst_count   an entry whose bucket holds its own j passed steps 1-3: a candidate. Counts.
//   k_inst_commit  a workgroup per entry. used + candidates > C / 2: every candidate is FULL and its transient
//                  entry is emptied again (nothing else was written). Otherwise the candidate's entry becomes
//                  {index, recv slot + 1}, its keys are copied, its counters and windows cleared (256 lanes over
//                  up to 2 x 8 KiB of window), and workgroup 0 adds the candidates to `used`.
// With WG_HS_INSTALL_COMPACT the three launches of wg_rx_sessions_compact (wg_rxplan.hip) run in front of these five:
// if the ring's m = min(*n_entries, n) entries would not fit (used + m > C / 2) and the table holds retired entries,
// it is rebuilt from its live ones first, and k_inst_fill takes used0 from the compacted table. Statuses and summary
// are those of compacting first and installing after.
// More entries than the table has empty buckets (a reserve far too small for the ring) cannot all be placed: an
// entry that has walked the whole table without finding its index or an empty bucket knows that no bucket will
// ever hold its index (an occupied bucket never changes its index during the call), so the lowest of such
// entries with one index is found by comparing with the lower entries directly (k_inst_count); they are all
// FULL, the table being full.
//
// Scratch: the claim words and four control words, allocated by wg_rx_sessions_reserve, each written by the
// call's first launch before a later one reads it; the entries' intermediate states live in inst_status itself.
// Positions and buckets only, never a key byte. Nothing about a call lives on the host, so a captured
// ... -> wg_hs_respond -> wg_hs_install replays.
//
// Constant time: a key is loaded, stored and (WIPE) overwritten with zeros, 16 bytes at a time; no branch,
// address or loop bound depends on a key byte. Slots, indices and positions are public.
#pragma once

namespace {

constexpr uint32_t kInstPass1 = 0x40000000u;        // inst_status between launches: passed step 1
constexpr uint32_t kInstOverflow = 0x7FFFFFFFu;     // passed steps 1-2, live nowhere, and the table is full
constexpr uint32_t kInstOverflowDup = 0x7FFFFFFEu;  // ... and a lower such entry has the same index
// (0x80000000 | bucket: placed in that bucket)

const PlanWords kHsInstWords{"handshake install", "entries", "wg_rx_sessions_reserve"};

}  // namespace

// ---- device -------------------------------------------------------------------------------
namespace wgin {

struct InstParams {
  InstView V;
  uint32_t* receivers;
  uint32_t* status;
  wg_hs_install_summary* summary;
  uint32_t slot_first, slot_count, key_slots, wipe;
  RxSessHdr* hdr;
  uint32_t* claim;
  RxInstCtl* ctl;
  uint4* keys;
  uint64_t* send;                 // send counters (NULL: no transmit state)
  uint64_t *top, *newtop, *bits;  // replay windows (NULL: none enabled)
  uint32_t words;                 // 64-bit words per window
};

__device__ __forceinline__ bool inst_slot_ok(const InstParams& P, uint32_t slot) {
  return slot >= P.slot_first && slot - P.slot_first < P.slot_count && slot < P.key_slots;
}
__device__ __forceinline__ unsigned long long inst_load(const unsigned long long* e) {
  return __hip_atomic_load(e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(256) k_inst_fill(InstParams P, uint32_t lo, uint32_t hi) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < hi - lo) P.claim[lo + i] = 0xFFFFFFFFu;
  if (i == 0) *P.ctl = RxInstCtl{P.hdr->used, 0u, 0u, 0u};
}

__global__ void __launch_bounds__(256) k_inst_claim(InstParams P) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= inst_count(P.V)) return;
  uint32_t s, r;
  const bool ok = inst_slots(P.V, inst_entry(P.V, j), s, r) && inst_slot_ok(P, s) && inst_slot_ok(P, r) && s != r;
  if (ok) {
    (void)atomicMin(P.claim + s, j);
    (void)atomicMin(P.claim + r, j);
  }
  P.status[j] = ok ? kInstPass1 : WG_HS_INST_BADSLOT;
}

__global__ void __launch_bounds__(256) k_inst_insert(InstParams P) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= inst_count(P.V) || P.status[j] != kInstPass1) return;
  const uint32_t* e = inst_entry(P.V, j);
  const uint32_t index = e[P.V.w_local];
  uint32_t s, r;
  (void)inst_slots(P.V, e, s, r);  // (step 1 passed)
  if (P.claim[s] != j || P.claim[r] != j) {
    P.status[j] = WG_HS_INST_DUPSLOT;
    return;
  }
  unsigned long long* ent = (unsigned long long*)P.hdr->entries;
  const unsigned long long mine = wgrp::u64_of(index, kRxTransient | j);
  uint32_t out = kInstOverflow;
  rx_probe(ent, P.hdr->mask, index, [&](unsigned long long* q) {
    unsigned long long v = inst_load(q);
    if (rx_empty((uint32_t)(v >> 32))) {
      const unsigned long long old = atomicCAS(q, v, mine);
      if (old == v) {
        out = kRxTransient | (uint32_t)(q - ent);
        return true;
      }
      v = old;  // another entry took the bucket: look at what it holds
    }
    const uint32_t h = (uint32_t)(v >> 32);
    if ((uint32_t)v != index || rx_retired(h)) return false;
    if (rx_transient(h)) {
      (void)atomicMin(q, mine);
      out = kRxTransient | (uint32_t)(q - ent);
    } else {
      out = WG_HS_INST_DUPINDEX;  // live at the call's start
    }
    return true;
  });
  P.status[j] = out;
}

__global__ void __launch_bounds__(256) k_inst_count(InstParams P) {
  __shared__ uint32_t s_cnt[3][4];
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  const bool in = j < inst_count(P.V);
  uint32_t st = in ? P.status[j] : WG_HS_INST_OK;
  bool cand = false;
  if (in && st == kInstOverflow) {
    const uint32_t index = inst_entry(P.V, j)[P.V.w_local];
    cand = true;
    for (uint32_t k = 0; k < j && cand; ++k) {
      const uint32_t sk = P.status[k];  // (entry k may be turning Overflow into OverflowDup: either says the same here)
      if ((sk == kInstOverflow || sk == kInstOverflowDup) && inst_entry(P.V, k)[P.V.w_local] == index) cand = false;
    }
    if (!cand) P.status[j] = st = kInstOverflowDup;
  } else if (in && (st & kRxTransient)) {
    const unsigned long long v = ((const unsigned long long*)P.hdr->entries)[st & ~kRxTransient];
    cand = (uint32_t)(v >> 32) == (kRxTransient | j);
    if (!cand) P.status[j] = st = WG_HS_INST_DUPINDEX;
  }
  const bool dup = in && (st == WG_HS_INST_DUPSLOT || st == WG_HS_INST_DUPINDEX || st == kInstOverflowDup);
  uint32_t r, n_cand, n_bad, n_dup;
  wgrp::block_rank(cand, s_cnt[0], r, n_cand);
  wgrp::block_rank(in && st == WG_HS_INST_BADSLOT, s_cnt[1], r, n_bad);
  wgrp::block_rank(dup, s_cnt[2], r, n_dup);
  if (threadIdx.x == 0) {
    if (n_cand) atomicAdd(&P.ctl->n_cand, n_cand);
    if (n_bad) atomicAdd(&P.ctl->n_badslot, n_bad);
    if (n_dup) atomicAdd(&P.ctl->n_dup, n_dup);
  }
}

// One workgroup per entry: the window words of an installed entry's two slots are cleared by all 256 lanes.
__global__ void __launch_bounds__(256) k_inst_commit(InstParams P) {
  __shared__ uint32_t s_st;
  const uint32_t j = blockIdx.x, tid = threadIdx.x;
  const RxInstCtl C = *P.ctl;
  const uint32_t mask = P.hdr->mask;
  const bool full = (uint64_t)C.used0 + C.n_cand > ((uint64_t)mask + 1u) / 2u;
  if (j == 0 && tid == 0) {
    uint2* sum = (uint2*)P.summary;  // (8-B stores: the summary need not be 16-B aligned)
    sum[0] = make_uint2(full ? 0u : C.n_cand, C.n_badslot);
    sum[1] = make_uint2(C.n_dup, full ? C.n_cand : 0u);
    if (!full && C.n_cand) {
      P.hdr->used = C.used0 + C.n_cand;
      P.hdr->count += C.n_cand;
    }
  }
  if (j >= inst_count(P.V)) return;
  if (tid == 0) s_st = P.status[j];
  __syncthreads();
  const uint32_t st = s_st;
  if (!(st & kRxTransient)) {  // not a placed candidate: its status is final, or one of the two overflow states
    if (tid == 0 && st == kInstOverflow) P.status[j] = WG_HS_INST_FULL;
    if (tid == 0 && st == kInstOverflowDup) P.status[j] = WG_HS_INST_DUPINDEX;
    return;
  }
  unsigned long long* q = (unsigned long long*)P.hdr->entries + (st & ~kRxTransient);
  if (full) {
    if (tid == 0) {
      *q = 0ull;  // the table as it was
      P.status[j] = WG_HS_INST_FULL;
    }
    return;
  }
  const uint32_t* e = inst_entry(P.V, j);
  const uint32_t index = e[P.V.w_local], remote = e[P.V.w_remote];
  uint32_t s, r;
  (void)inst_slots(P.V, e, s, r);  // (step 1 passed)
  if (tid < 4u) {  // send_key, recv_key: 4 x 16 B, each lane its own
    uint4* k4 = (uint4*)e + P.V.q_keys + tid;
    const uint4 v = *k4;
    P.keys[2u * (tid < 2u ? s : r) + (tid & 1u)] = v;
    if (P.wipe) *k4 = make_uint4(0u, 0u, 0u, 0u);
  }
  if (tid == 0) {
    *q = wgrp::u64_of(index, r + 1u);
    if (P.receivers) P.receivers[s] = remote;
    if (P.send) P.send[s] = P.send[r] = 0ull;
    if (P.top) P.top[s] = P.top[r] = 0ull;
    P.status[j] = WG_HS_INST_OK;
  }
  if (P.top) {
    if (tid >= 64u && tid < 64u + 2u * kTopWays) {
      const uint32_t w = tid - 64u;
      P.newtop[(size_t)(w < kTopWays ? s : r) * kTopWays + (w % kTopWays)] = 0ull;
    }
    for (uint32_t w = tid; w < 2u * P.words; w += 256u)
      P.bits[(size_t)(w < P.words ? s : r) * P.words + (w < P.words ? w : w - P.words)] = 0ull;
  }
}

}  // namespace wgin

// ---- C ABI --------------------------------------------------------------------------------
extern "C" {

int wg_hs_install(wg_ctx* c, const wg_hs_install_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  if (b->flags & ~(WG_HS_INSTALL_WIPE | WG_HS_INSTALL_COMPACT)) return fail(WG_EINVAL, "unknown install flags 0x%x", b->flags);
  if (((uintptr_t)b->n_entries) & 3u) return fail(WG_EINVAL, "n_entries must be 4-byte aligned");  // (of an empty ring too)
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  RxPlanState* t = c->rxp;
  if (!t || !t->reserved) return fail(WG_EINVAL, "wg_hs_install before wg_rx_sessions_reserve");
  const uint32_t n = b->n;
  int rc;
  if ((rc = inst_batch_check(*b, "handshake install")) != WG_OK || n == 0) return rc;
  const InstView V = inst_view(*b);
  if (!b->inst_status || (((uintptr_t)b->inst_status) & 3u) || !b->summary || (((uintptr_t)b->summary) & 7u) ||
      (((uintptr_t)b->receivers) & 3u))
    return fail(WG_EINVAL, "inst_status / summary must be non-NULL and aligned (4 / 8 bytes; receivers: 4)");
  {
    const HsRange out[4] = {{b->entries, (uint64_t)V.stride * n},
                            {b->inst_status, 4ull * n},
                            {b->summary, sizeof(wg_hs_install_summary)},
                            {b->receivers, b->receivers ? 4ull * c->key_slots : 0u}};
    const HsRange in[3] = {{b->n_entries, b->n_entries ? 4u : 0u}, {b->send_slot, 4ull * b->n_slots}, {b->recv_slot, 4ull * b->n_slots}};
    const int ov = hs_ranges_overlap(out, in);
    if (ov == 1) return fail(WG_EINVAL, "entries, inst_status, summary and receivers must not overlap");
    if (ov == 2) return fail(WG_EINVAL, "an output of wg_hs_install must not overlap n_entries, send_slot or recv_slot");
  }
  const bool capturing = stream_capturing(s);
  RxState* r = c->rx && c->rx->window ? c->rx : nullptr;
  TxState* x = c->tx;
  if ((rc = plan_begin(t->order, s, capturing, true, [] { return WG_OK; }, kHsInstWords, n)) != WG_OK) return rc;
  if (!capturing && r && (rc = r->order.after_last(s)) != WG_OK) return rc;
  if (!capturing && x && (rc = x->order.after_last(s)) != WG_OK) return rc;
  // the key slots the device now owns, clipped to the table
  const uint32_t lo = std::min(b->slot_first, c->key_slots);
  const uint32_t hi = (uint32_t)std::min<uint64_t>((uint64_t)b->slot_first + b->slot_count, c->key_slots);
  {  // the host's copy of these keys is no longer the key: the paths that seal with it refuse the slots
    std::lock_guard<std::mutex> lk2(c->keys_mu);
    key_mirror_write(c, lo, hi - lo, nullptr);
  }
  wgin::InstParams P{};
  P.V = V;
  P.receivers = b->receivers;
  P.status = b->inst_status;
  P.summary = b->summary;
  P.slot_first = b->slot_first;
  P.slot_count = b->slot_count;
  P.key_slots = c->key_slots;
  P.wipe = (b->flags & WG_HS_INSTALL_WIPE) ? 1u : 0u;
  P.hdr = (RxSessHdr*)t->d_hdr.p;
  P.claim = (uint32_t*)t->d_claim.p;
  P.ctl = (RxInstCtl*)t->d_ctl.p;
  P.keys = (uint4*)c->keys;
  P.send = x ? (uint64_t*)x->d_send.p : nullptr;
  P.top = r ? (uint64_t*)r->d_top.p : nullptr;
  P.newtop = r ? (uint64_t*)r->d_newtop.p : nullptr;
  P.bits = r ? (uint64_t*)r->d_bits.p : nullptr;
  P.words = r ? r->window / 64u : 0u;
  const uint32_t nb = rank_blocks(n);
  if (b->flags & WG_HS_INSTALL_COMPACT) {  // decided on the device, in front of k_inst_fill: used0 is the compacted table's
    wgrp::RxCompactParams Q{};
    Q.n_entries = b->n_entries;
    Q.n = n;
    Q.install = 1u;
    rxp_compact_launch(t, s, Q);
  }
  hipLaunchKernelGGL(wgin::k_inst_fill, dim3(std::max(1u, rank_blocks(hi - lo))), dim3(256), 0, s, P, lo, hi);
  hipLaunchKernelGGL(wgin::k_inst_claim, dim3(nb), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgin::k_inst_insert, dim3(nb), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgin::k_inst_count, dim3(nb), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgin::k_inst_commit, dim3(n), dim3(256), 0, s, P);
  {  // ... and once more behind the launches, while the device works: a slot of the range that holds a key again is
     // marked again. (Every writer of the mirror takes c->mu today, which this call holds: the pass finds nothing.)
    std::lock_guard<std::mutex> lk2(c->keys_mu);
    for (uint32_t slot = lo; slot < hi; ++slot)
      if (key_is_live(c, slot)) key_mirror_write(c, slot, 1, nullptr);
  }
  if ((rc = plan_end(t->order, s, capturing, kHsInstWords)) != WG_OK) return rc;
  if (!capturing && r && (rc = r->order.mark(s)) != WG_OK) return rc;
  if (!capturing && x && (rc = x->order.mark(s)) != WG_OK) return rc;
  return WG_OK;
}

}  // extern "C"
