// wg_hs_ratelimit.hip — handshakes rate-limited per source, on the device (included by wg_capi.hip after
// wg_hs_cookie.hip): wg_hs_rl_reserve, wg_hs_rl_config_set, wg_hs_ratelimit, wg_hs_rl_compact, wg_hs_rl_dump / _load /
// _count.
//
// wg_hs_admit makes a sender prove that it receives at its source address; a sender that does then sends fresh
// initiations with a valid mac2, a ladder and the open chain each. WireGuard's token bucket per source (20 handshakes
// per second, a burst of 5, by IPv4 address or IPv6 /64) is the rest of its under-load rule, and the reference has none
// of it. The rule, its closed form for a call's records at one `now`, and the statuses are in include/wgaead.h.
//
// The table. C buckets of 32 B {kw, family, tokens, last}, open addressing, linear probing from mix32 of the key, at
// most C / 2 entries, behind RlHdr at a fixed device address (wg_plan.hip, fixed headers). A key is 65 bits (a
// family, and up to 64 bits of address) and the device claims a bucket with one 64-bit compare-and-swap, so:
//   kw      = the address word; an IPv4 one carries bit 32, so that no IPv4 kw is 0 (0 is the empty bucket);
//   family  = written by the claim's winner with a plain store, and the two families claim in two launches
//             (k_rl_claim<4>, then <6>): a bucket whose kw matches holds the other family only if that family's word is
//             already visible, from an earlier launch or call; a word of 0 or of this launch's family is this key's;
//   entry C = the home of the one IPv6 key whose kw is 0 (::/64), claimed through its family word.
//
// A call, 7 + burst launches on its stream, ordered by kernel boundaries, no workgroup waiting for another:
//   (memset)      m = inserted = 0 in the header.
//   k_rl_find     one record per thread: the source's key, the probe (read only). A known source: + 1 in its bucket's
//                 count (wave_elect: one atomic per wave where the wave agrees); an unknown one: m += 1 per record (one
//                 atomic per workgroup). The thread that takes a count from 0 is the source's leader.
//   k_rl_claim<4>, <6>   if used + m <= C / 2, the unknown records claim their buckets and count in them; else they
//                 are FULL and nothing is inserted.
//   k_rl_round x burst   round 0 computes the allowance a = min(max, tokens + age) / cost of each record's source and
//                 marks the sources with c > a > 0 contended. In round j < a every record of a contended source whose
//                 position is above word j - 1 of the bucket's row does an atomicMin into word j (the first lane of
//                 a wave that agrees does it for the wave: positions rise with the lane). Word a - 1 ends as the a-th
//                 lowest position. Rows stand at 0xFFFFFFFF between calls.
//   k_rl_decide, k_rx_scan, k_rl_emit   the rank (wg_plan.hip): status and counts; prefixes and the summary; the OK
//                 records placed, and each leader writes its entry {refilled - min(a, c) cost, max(last, now)},
//                 zeroes the count and restores the row. One thread adds `inserted` to `used`.
// Nothing about a call lives on the host: cost, burst, the table and its buffers are read through the header.
//
// Compaction: wg_rx_sessions_compact's three launches (clear the spare, rehash, flip), keeping the entries with
// (now >= last ? now - last : 0) < max. The rehash's keys are unique, so a claim there needs no second family launch.
//
// Nothing here is secret: addresses, statuses and buckets are public.
#pragma once

namespace {

const PlanWords kHsRlWords{"handshake ratelimit", "records", "wg_hs_reserve"};
const PlanWords kHsRlCompactWords{"ratelimit compaction", "entries", "wg_hs_rl_reserve"};

struct RlEntry {  // 32 B
  unsigned long long kw;  // 0: empty (entry C: see family)
  uint32_t family, _pad;
  unsigned long long tokens, last;
};
static_assert(sizeof(RlEntry) == 32 && sizeof(wg_hs_rl_entry) == 32, "a bucket is two uint4");

struct RlHdr {  // at a fixed device address
  RlEntry* entries;  // the current table: mask + 2 entries
  RlEntry* buf[2];   // the table's two buffers: `entries` is one, the other is the spare
  uint32_t* cnt;     // per entry: the call's records of this source; 0 between calls
  uint32_t* rows;    // per entry: WG_HS_RL_MAX_BURST selection words; 0xFFFFFFFF between calls
  unsigned long long cost;
  uint32_t burst, mask, used, _pad;
  uint32_t m, inserted;         // a call's words between its launches (zeroed by its memset)
  uint32_t go, kept, dropped, _pad2;  // the compaction's (written by its first launch)
};

constexpr unsigned long long kRlV4Bit = 1ull << 32;

__host__ __device__ inline uint32_t rl_start(unsigned long long kw, uint32_t family, uint32_t mask) {
  return mix32((uint32_t)kw ^ mix32((uint32_t)(kw >> 32) ^ (family * 0x9E3779B9u))) & mask;
}

}  // namespace

// ---- device -------------------------------------------------------------------------------
namespace wgrl {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kRow = WG_HS_RL_MAX_BURST;
// a record's code between the launches: bits 8-15 the family, bits 16-20 the allowance
constexpr uint32_t kValid = 1u, kDirect = 2u, kNew = 4u, kFull = 8u, kLeader = 16u, kCont = 32u;

struct RlParams {
  const wg_hs_record* records;
  const uint32_t* n_records;
  const wg_hs_src* src;
  const unsigned long long* now;
  uint32_t* rl_status;
  wg_hs_record* out_records;
  RlHdr* hdr;
  uint4* rec;  // per record: {entry, code, kw}
  uint4* part;
  uint32_t n, n_src, round;
};

struct RlCompactParams {
  RlHdr* hdr;
  const unsigned long long* now;
  wg_hs_rl_compact_summary* summary;  // NULL: none (the call's)
  const uint32_t* n_records;          // the call's: its count on the device (NULL: all n)
  uint32_t n;
  uint32_t in_call;  // decided by the call's rule; otherwise always
};

// min(max, tokens + age), the sum saturating; a new entry is full
__device__ __forceinline__ unsigned long long rl_refilled(const RlEntry* e, bool fresh, unsigned long long now, unsigned long long max) {
  if (fresh) return max;
  const unsigned long long tokens = e->tokens, last = e->last;
  const unsigned long long age = now >= last ? now - last : 0ull;
  const unsigned long long sum = tokens + age;
  return (sum < tokens || sum > max) ? max : sum;
}

// the entry of (kw, family), or kNone. At most C / 2 of the C buckets are taken, so the walk ends at an empty one.
__device__ __forceinline__ uint32_t rl_find(const RlEntry* e, uint32_t mask, unsigned long long kw, uint32_t family) {
  if (!kw) return e[mask + 1u].family == 6u ? mask + 1u : kNone;
  uint32_t i = rl_start(kw, family, mask);
  for (uint32_t step = 0; step <= mask; ++step, i = (i + 1u) & mask) {
    const unsigned long long v = e[i].kw;
    if (!v) return kNone;
    if (v == kw && e[i].family == family) return i;
  }
  return kNone;
}

// + 1 in the count of `slot` for every lane with `act` (one atomic per wave that agrees); whether this lane took the
// count from 0. Every lane of the wave must reach the call.
__device__ __forceinline__ bool rl_count(uint32_t* cnt, bool act, uint32_t slot) {
  const uint64_t am = __ballot(act);
  bool for_all;
  const bool me = wgrp::wave_elect<false>(act, slot, for_all);
  bool leader = false;
  if (me) leader = atomicAdd(cnt + slot, for_all ? (uint32_t)__popcll((unsigned long long)am) : 1u) == 0u;
  return leader;
}

__global__ void __launch_bounds__(256) k_rl_find(RlParams P) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t nl = wgrp::dev_count(P.n_records, P.n);
  if (blockIdx.x * kRankRange >= nl) return;  // (workgroup-uniform)
  const uint32_t k = blockIdx.x * kRankRange + threadIdx.x;
  const bool in = k < nl;
  const RlEntry* ent = P.hdr->entries;
  const uint32_t mask = P.hdr->mask;
  const unsigned long long now = *P.now;
  uint32_t code = 0, slot = 0;
  unsigned long long kw = 0;
  if (in) {
    const uint32_t i = ((const uint32_t*)(P.records + k))[0];
    if (i < P.n_src) {
      uint32_t a[4], pf;
      wgck::src_of(P.src, i, a, pf);
      const uint32_t fam = (pf >> 16) & 0xFFu;
      if (fam == 4u || fam == 6u) {
        code = kValid | (fam << 8);
        kw = fam == 4u ? ((unsigned long long)a[0] | kRlV4Bit) : wgrp::u64_of(a[0], a[1]);
        if (!now) {
          code |= kDirect;
        } else {
          slot = rl_find(ent, mask, kw, fam);
          if (slot == kNone) {
            slot = 0;
            code |= kNew;
          }
        }
      }
    }
  }
  const bool known = (code & kValid) && !(code & (kDirect | kNew));
  if (rl_count(P.hdr->cnt, known, slot)) code |= kLeader;
  uint32_t r, m;
  wgrp::block_rank((code & kNew) != 0u, s_cnt, r, m);
  if (threadIdx.x == 0 && m) (void)atomicAdd(&P.hdr->m, m);
  if (in) P.rec[k] = make_uint4(slot, code, (uint32_t)kw, (uint32_t)(kw >> 32));
}

// the unknown records of family F claim their buckets, or are FULL
template <uint32_t F>
__global__ void __launch_bounds__(256) k_rl_claim(RlParams P) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t nl = wgrp::dev_count(P.n_records, P.n);
  if (blockIdx.x * kRankRange >= nl) return;  // (workgroup-uniform)
  const uint32_t k = blockIdx.x * kRankRange + threadIdx.x;
  const bool in = k < nl;
  RlEntry* ent = P.hdr->entries;
  const uint32_t mask = P.hdr->mask;
  const bool fits = (uint64_t)P.hdr->used + P.hdr->m <= ((uint64_t)mask + 1u) / 2u;  // (both stand still in this launch)
  uint4 rc = in ? P.rec[k] : make_uint4(0u, 0u, 0u, 0u);
  const bool mine = (rc.y & kNew) && ((rc.y >> 8) & 0xFFu) == F;
  bool won = false, placed = false;
  uint32_t slot = 0;
  if (mine && fits) {
    const unsigned long long kw = wgrp::u64_of(rc.z, rc.w);
    if (!kw) {  // (F == 6) ::/64 lives in entry C
      slot = mask + 1u;
      won = atomicCAS(&ent[slot].family, 0u, 6u) == 0u;
      placed = true;
    } else {
      uint32_t i = rl_start(kw, F, mask);
      for (uint32_t step = 0; step <= mask && !placed; ++step, i = (i + 1u) & mask) {
        unsigned long long v = ent[i].kw;  // (a bucket goes from 0 to its key once: a key read here is final)
        if (!v) {
          v = atomicCAS(&ent[i].kw, 0ull, kw);
          if (!v) {
            won = true;
            ent[i].family = F;
            v = kw;
          }
        }
        // the other family's word was stored before this launch; 0 or F is this key, claimed in this launch or mine
        if (v == kw && (won || ent[i].family != (F == 4u ? 6u : 4u))) {
          slot = i;
          placed = true;
        }
      }
    }
  }
  if (mine) rc.y |= placed ? 0u : kFull;  // (with fits, a walk always places: at most C / 2 buckets are taken)
  if (rl_count(P.hdr->cnt, placed, slot)) rc.y |= kLeader;
  uint32_t r, ins;
  wgrp::block_rank(won, s_cnt, r, ins);
  if (threadIdx.x == 0 && ins) (void)atomicAdd(&P.hdr->inserted, ins);
  if (mine) {
    rc.x = slot;
    P.rec[k] = rc;
  }
}

// round P.round of the selection of the lowest positions of the contended sources
__global__ void __launch_bounds__(256) k_rl_round(RlParams P) {
  const uint32_t nl = wgrp::dev_count(P.n_records, P.n);
  if (blockIdx.x * kRankRange >= nl) return;  // (workgroup-uniform)
  const uint32_t k = blockIdx.x * kRankRange + threadIdx.x;
  const bool in = k < nl;
  const uint4 rc = in ? P.rec[k] : make_uint4(0u, 0u, 0u, 0u);
  uint32_t code = rc.y;
  const uint32_t slot = rc.x;
  const bool served = (code & kValid) && !(code & (kDirect | kFull));
  uint32_t* rows = P.hdr->rows;
  if (P.round == 0u && served) {
    const unsigned long long cost = P.hdr->cost;
    const unsigned long long refilled = rl_refilled(P.hdr->entries + slot, (code & kNew) != 0u, *P.now, cost * P.hdr->burst);
    const uint32_t a = (uint32_t)(refilled / cost);  // <= burst
    code |= a << 16;
    if (a && P.hdr->cnt[slot] > a) code |= kCont;
    ((uint32_t*)(P.rec + k))[1] = code;
  }
  const uint32_t a = (code >> 16) & 31u;
  bool go = served && (code & kCont) && P.round < a;
  if (go && P.round) go = k > rows[(size_t)slot * kRow + P.round - 1u];
  bool for_all;
  if (wgrp::wave_elect<false>(go, slot, for_all)) (void)atomicMin(rows + (size_t)slot * kRow + P.round, k);
}

// the status of one record per thread; the range's counts
__global__ void __launch_bounds__(256) k_rl_decide(RlParams P) {
  __shared__ uint32_t s_cnt[4][4];
  const uint32_t nl = wgrp::dev_count(P.n_records, P.n);
  if (blockIdx.x * kRankRange >= nl) {  // past the list (workgroup-uniform): a zero record for the scan
    if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const uint32_t k = blockIdx.x * kRankRange + threadIdx.x;
  const bool in = k < nl;
  uint32_t st = WG_HS_RL_BADSRC;
  if (in) {
    const uint4 rc = P.rec[k];
    const uint32_t code = rc.y, a = (code >> 16) & 31u;
    if (!(code & kValid)) st = WG_HS_RL_BADSRC;
    else if (code & kFull) st = WG_HS_RL_FULL;
    else if (code & kDirect) st = WG_HS_RL_OK;
    else if (!(code & kCont)) st = a ? WG_HS_RL_OK : WG_HS_RL_LIMITED;  // c <= a, or a == 0
    else st = k <= P.hdr->rows[(size_t)rc.x * kRow + a - 1u] ? WG_HS_RL_OK : WG_HS_RL_LIMITED;
    P.rl_status[k] = st;
  }
  uint32_t r, n_ok, n_lim, n_full, n_bad;
  wgrp::block_rank(in && st == WG_HS_RL_OK, s_cnt[0], r, n_ok);
  wgrp::block_rank(in && st == WG_HS_RL_LIMITED, s_cnt[1], r, n_lim);
  wgrp::block_rank(in && st == WG_HS_RL_FULL, s_cnt[2], r, n_full);
  wgrp::block_rank(in && st == WG_HS_RL_BADSRC, s_cnt[3], r, n_bad);
  if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4(n_ok, n_lim, n_full, n_bad);
}

// out_records[prefix of the range + rank in the range] = this OK record; the leaders write their entries and leave
// the bucket's scratch as every call expects it
__global__ void __launch_bounds__(256) k_rl_emit(RlParams P) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t nl = wgrp::dev_count(P.n_records, P.n);
  if (blockIdx.x * kRankRange >= nl) return;  // (workgroup-uniform)
  const uint32_t k = blockIdx.x * kRankRange + threadIdx.x;
  const bool in = k < nl;
  const bool ok = in && P.rl_status[k] == WG_HS_RL_OK;
  const uint4 pre = P.part[blockIdx.x];
  uint32_t r, total;
  wgrp::block_rank(ok, s_cnt, r, total);
  if (blockIdx.x == 0 && threadIdx.x == 0) P.hdr->used += P.hdr->inserted;
  if (ok) {
    const uint4* src = (const uint4*)(P.records + k);
    uint4* dst = (uint4*)(P.out_records + (pre.x + r));
#pragma unroll
    for (uint32_t g = 0; g < sizeof(wg_hs_record) / 16u; ++g) dst[g] = src[g];
  }
  if (!in) return;
  const uint4 rc = P.rec[k];
  if (!(rc.y & kLeader)) return;
  const unsigned long long cost = P.hdr->cost, now = *P.now;
  RlEntry* e = P.hdr->entries + rc.x;
  const bool fresh = (rc.y & kNew) != 0u;
  const unsigned long long refilled = rl_refilled(e, fresh, now, cost * P.hdr->burst);
  const uint32_t a = (rc.y >> 16) & 31u, c = P.hdr->cnt[rc.x];
  const unsigned long long last = fresh ? 0ull : e->last;
  e->tokens = refilled - (unsigned long long)(c < a ? c : a) * cost;
  e->last = now >= last ? now : last;
  if (fresh) e->_pad = 0u;
  P.hdr->cnt[rc.x] = 0u;
  if (rc.y & kCont) {
    uint4* row = (uint4*)(P.hdr->rows + (size_t)rc.x * kRow);
#pragma unroll
    for (uint32_t g = 0; g < kRow / 4u; ++g) row[g] = make_uint4(kNone, kNone, kNone, kNone);
  }
}

// ---- compaction ----

__device__ __forceinline__ RlEntry* rl_spare(const RlHdr* H) { return H->buf[0] == H->entries ? H->buf[1] : H->buf[0]; }

// the whole spare = empty; thread 0 decides
__global__ void __launch_bounds__(256) k_rl_compact_clear(RlCompactParams P) {
  uint4* spare = (uint4*)rl_spare(P.hdr);
  const uint64_t words = 2ull * ((uint64_t)P.hdr->mask + 2u);
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < words; i += (uint64_t)gridDim.x * 256u) spare[i] = make_uint4(0u, 0u, 0u, 0u);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    bool go = true;
    if (P.in_call)
      go = *P.now != 0ull && (uint64_t)P.hdr->used + wgrp::dev_count(P.n_records, P.n) > ((uint64_t)P.hdr->mask + 1u) / 2u;
    P.hdr->go = go ? 1u : 0u;
    P.hdr->kept = 0u;
    P.hdr->dropped = 0u;
  }
}

// one entry of the current table per thread; a kept one claims the first empty bucket of its walk in the spare
__global__ void __launch_bounds__(256) k_rl_compact_rehash(RlCompactParams P) {
  __shared__ uint32_t s_n[2];
  if (!P.hdr->go) return;  // (grid-uniform)
  if (threadIdx.x < 2u) s_n[threadIdx.x] = 0u;
  __syncthreads();
  const RlEntry* cur = P.hdr->entries;
  RlEntry* spare = rl_spare(P.hdr);
  const uint32_t mask = P.hdr->mask;
  const unsigned long long now = *P.now, max = P.hdr->cost * P.hdr->burst;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i <= (uint64_t)mask + 1u; i += (uint64_t)gridDim.x * 256u) {
    const uint4 lo = ((const uint4*)(cur + i))[0], hi = ((const uint4*)(cur + i))[1];
    if (!lo.z) continue;  // no family: empty
    const unsigned long long kw = wgrp::u64_of(lo.x, lo.y), last = wgrp::u64_of(hi.z, hi.w);
    if ((now >= last ? now - last : 0ull) >= max) {
      (void)atomicAdd(&s_n[1], 1u);
      continue;
    }
    (void)atomicAdd(&s_n[0], 1u);
    uint32_t slot = mask + 1u;
    if (kw) {
      uint32_t j = rl_start(kw, lo.z, mask);
      for (uint32_t step = 0; step <= mask; ++step, j = (j + 1u) & mask)
        if (atomicCAS(&spare[j].kw, 0ull, kw) == 0ull) {
          slot = j;
          break;
        }
      if (slot > mask) continue;  // (never: the spare holds at most C / 2 entries)
    }
    uint4* o = (uint4*)(spare + slot);  // (kw is stored again with the rest: the same value)
    o[0] = make_uint4(lo.x, lo.y, lo.z, 0u);
    o[1] = hi;
  }
  __syncthreads();
  if (threadIdx.x < 2u && s_n[threadIdx.x]) (void)atomicAdd(threadIdx.x ? &P.hdr->dropped : &P.hdr->kept, s_n[threadIdx.x]);
}

__global__ void k_rl_compact_flip(RlCompactParams P) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  RlHdr* H = P.hdr;
  const uint32_t go = H->go, kept = go ? H->kept : H->used, dropped = go ? H->dropped : 0u;
  if (go) {
    H->entries = rl_spare(H);
    H->used = kept;
  }
  if (P.summary) {  // (8-B stores: the summary need not be 16-B aligned)
    uint2* sum = (uint2*)P.summary;
    sum[0] = make_uint2(kept, dropped);
    sum[1] = make_uint2(0u, 0u);
  }
}

}  // namespace wgrl

// ---- C ABI --------------------------------------------------------------------------------
namespace {

uint32_t rl_capacity(uint32_t max_sources) {  // the smallest power of two >= max(8, 2 max_sources)
  uint32_t cap = 8;
  while ((uint64_t)cap < 2ull * max_sources) cap <<= 1;
  return cap;
}

// The limiter's state of a context that has reserved one. Caller holds c->mu.
int rl_get(wg_ctx* c, const char* who, HsState** out) {
  if (!c->hs || !c->hs->rl_cap) return fail(WG_ENOKEY, "%s before any wg_hs_rl_reserve", who);
  *out = c->hs;
  return WG_OK;
}

int rl_hdr_read(wg_ctx* c, HsState* t, RlHdr* H) {
  HIPTRY(hipMemcpyAsync(H, t->d_rlhdr.p, sizeof *H, hipMemcpyDeviceToHost, c->stream));
  HIPTRY(hipStreamSynchronize(c->stream));
  return WG_OK;
}
int rl_hdr_write(wg_ctx* c, HsState* t, const RlHdr& H) {
  HIPTRY(hipMemcpyAsync(t->d_rlhdr.p, &H, sizeof H, hipMemcpyHostToDevice, c->stream));
  HIPTRY(hipStreamSynchronize(c->stream));
  return WG_OK;
}

// the table's entries, in table order. Caller holds c->mu and has synchronised the device.
int rl_entries_read(wg_ctx* c, HsState* t, std::vector<wg_hs_rl_entry>* out) {
  RlHdr H;
  int rc;
  if ((rc = rl_hdr_read(c, t, &H)) != WG_OK) return rc;
  std::vector<RlEntry> v((size_t)H.mask + 2u);
  HIPTRY(hipMemcpyAsync(v.data(), H.entries, sizeof(RlEntry) * v.size(), hipMemcpyDeviceToHost, c->stream));
  HIPTRY(hipStreamSynchronize(c->stream));
  out->clear();
  for (const RlEntry& e : v) {
    if (!e.family) continue;
    wg_hs_rl_entry o{};
    const unsigned long long addr = e.family == 4u ? (e.kw & 0xFFFFFFFFull) : e.kw;
    memcpy(o.addr, &addr, 8);
    o.family = (uint8_t)e.family;
    o.tokens = e.tokens;
    o.last = e.last;
    out->push_back(o);
  }
  return WG_OK;
}

// The table of t->rl_cap buckets = these entries (validated first: nothing changes on error), in buffer 0, with the
// config the header holds. Caller holds c->mu and has synchronised the device.
int rl_table_set(wg_ctx* c, HsState* t, const wg_hs_rl_entry* in, uint32_t n, unsigned long long cost, uint32_t burst) {
  const uint32_t cap = t->rl_cap, mask = cap - 1u;
  if (n > cap / 2u) return fail(WG_ERANGE, "%u entries for a ratelimit table of %u buckets (at most %u)", n, cap, cap / 2u);
  std::vector<RlEntry> v((size_t)cap + 1u, RlEntry{});
  for (uint32_t k = 0; k < n; ++k) {
    const wg_hs_rl_entry& e = in[k];
    if (e.family != 4 && e.family != 6) return fail(WG_EINVAL, "ratelimit entry %u: family %u", k, (unsigned)e.family);
    unsigned long long addr;
    memcpy(&addr, e.addr, 8);
    bool pad = false;
    for (int j = 0; j < 7; ++j) pad |= e._pad[j] != 0;
    if (pad || (e.family == 4 && (addr >> 32))) return fail(WG_EINVAL, "ratelimit entry %u: pad or IPv4 tail bytes not zero", k);
    const unsigned long long kw = e.family == 4 ? (addr | kRlV4Bit) : addr;
    uint32_t slot = cap;
    if (kw) {
      uint32_t i = rl_start(kw, e.family, mask);
      for (; v[i].family; i = (i + 1u) & mask)
        if (v[i].kw == kw && v[i].family == e.family) break;
      slot = i;
    }
    if (v[slot].family) return fail(WG_EINVAL, "ratelimit entry %u repeats a key", k);
    v[slot] = RlEntry{kw, e.family, 0u, e.tokens, e.last};
  }
  HIPTRY(hipMemcpyAsync(t->d_rlent[0].p, v.data(), sizeof(RlEntry) * v.size(), hipMemcpyHostToDevice, c->stream));
  HIPTRY(hipMemsetAsync(t->d_rlcnt.p, 0, 4ull * (cap + 1ull), c->stream));
  HIPTRY(hipMemsetAsync(t->d_rlrows.p, 0xFF, 4ull * wgrl::kRow * (cap + 1ull), c->stream));
  RlHdr H{};
  H.entries = (RlEntry*)t->d_rlent[0].p;
  H.buf[0] = H.entries;
  H.buf[1] = (RlEntry*)t->d_rlent[1].p;
  H.cnt = (uint32_t*)t->d_rlcnt.p;
  H.rows = (uint32_t*)t->d_rlrows.p;
  H.cost = cost;
  H.burst = burst;
  H.mask = mask;
  H.used = n;
  return rl_hdr_write(c, t, H);
}

void rl_compact_launch(HsState* t, hipStream_t s, wgrl::RlCompactParams P) {
  P.hdr = (RlHdr*)t->d_rlhdr.p;
  const uint32_t nb = rank_blocks(t->rl_cap + 1u);
  hipLaunchKernelGGL(wgrl::k_rl_compact_clear, dim3(nb), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgrl::k_rl_compact_rehash, dim3(nb), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgrl::k_rl_compact_flip, dim3(1), dim3(64), 0, s, P);
}

}  // namespace

extern "C" {

int wg_hs_rl_reserve(wg_ctx* c, uint32_t max_sources) {
  if (!c) return fail(WG_EINVAL, "NULL context");
  if (max_sources > 0x8000000u) return fail(WG_E2BIG, "ratelimit table for %u sources", max_sources);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HsState* t;
  int rc;
  if ((rc = hs_get(c, &t)) != WG_OK) return rc;
  const uint32_t cap = rl_capacity(max_sources);
  if (cap <= t->rl_cap) return WG_OK;
  HIPTRY(hipDeviceSynchronize());  // the table is reallocated under earlier calls
  std::vector<wg_hs_rl_entry> keep;
  RlHdr H{};
  if (t->rl_cap && ((rc = rl_hdr_read(c, t, &H)) != WG_OK || (rc = rl_entries_read(c, t, &keep)) != WG_OK)) return rc;
  const size_t ents = sizeof(RlEntry) * ((size_t)cap + 1u);
  if ((rc = t->d_rlhdr.ensure(sizeof(RlHdr))) != WG_OK || (rc = t->d_rlent[0].ensure(ents)) != WG_OK ||
      (rc = t->d_rlent[1].ensure(ents)) != WG_OK || (rc = t->d_rlcnt.ensure(4ull * (cap + 1ull))) != WG_OK ||
      (rc = t->d_rlrows.ensure(4ull * wgrl::kRow * (cap + 1ull))) != WG_OK) {
    t->rl_cap = 0;  // (buffers of two sizes: no limiter until a reserve succeeds)
    return rc;
  }
  t->rl_cap = cap;
  if ((rc = hs_rl_grow(t, t->reserved)) == WG_OK) rc = rl_table_set(c, t, keep.data(), (uint32_t)keep.size(), H.cost, H.burst);
  if (rc != WG_OK) t->rl_cap = 0;
  return rc;
}

int wg_hs_rl_config_set(wg_ctx* c, uint64_t cost, uint32_t burst) {
  if (!c) return fail(WG_EINVAL, "NULL context");
  if (cost < 1u || cost > (1ull << 56) || burst < 1u || burst > WG_HS_RL_MAX_BURST)
    return fail(WG_EINVAL, "ratelimit cost %llu (1 .. 2^56) and burst %u (1 .. %u)", (unsigned long long)cost, burst, WG_HS_RL_MAX_BURST);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HsState* t;
  int rc;
  if ((rc = rl_get(c, "wg_hs_rl_config_set", &t)) != WG_OK) return rc;
  HIPTRY(hipDeviceSynchronize());  // no call queued earlier (on any stream) may still read the old values
  RlHdr H;
  if ((rc = rl_hdr_read(c, t, &H)) != WG_OK) return rc;
  H.cost = cost;
  H.burst = burst;
  if ((rc = rl_hdr_write(c, t, H)) != WG_OK) return rc;
  t->rl_burst = burst;
  return WG_OK;
}

int wg_hs_ratelimit(wg_ctx* c, const wg_hs_rl_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  if ((b->flags & ~WG_HS_RL_COMPACT) || b->_reserved) return fail(WG_EINVAL, "unknown ratelimit flags 0x%x, or _reserved not 0", b->flags);
  if (!b->rl_summary || (((uintptr_t)b->rl_summary) & 7u)) return fail(WG_EINVAL, "rl_summary must be non-NULL and 8-byte aligned");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HsState* t;
  int rc;
  if ((rc = rl_get(c, "wg_hs_ratelimit", &t)) != WG_OK) return rc;
  if (!t->rl_burst) return fail(WG_ENOKEY, "wg_hs_ratelimit before any wg_hs_rl_config_set");
  const uint32_t n = b->n;
  if (n == 0) {
    HIPTRY(hipMemsetAsync(b->rl_summary, 0, sizeof(wg_hs_rl_summary), s));
    return WG_OK;
  }
  if (n > 0x40000000u) return fail(WG_E2BIG, "handshake ratelimit of %u records", n);
  if (!b->records || (((uintptr_t)b->records) & 15u) || !b->out_records || (((uintptr_t)b->out_records) & 15u))
    return fail(WG_EINVAL, "records / out_records must be non-NULL and 16-byte aligned");
  if ((b->n_src && !b->src) || (((uintptr_t)b->src) & 7u) || !b->now || (((uintptr_t)b->now) & 7u))
    return fail(WG_EINVAL, "src / now must be non-NULL and 8-byte aligned");
  if (!b->rl_status || (((uintptr_t)b->rl_status) & 3u) || (((uintptr_t)b->n_records) & 3u))
    return fail(WG_EINVAL, "rl_status must be non-NULL, rl_status and n_records 4-byte aligned");
  {
    const HsRange out[3] = {{b->rl_status, 4ull * n}, {b->out_records, sizeof(wg_hs_record) * (uint64_t)n}, {b->rl_summary, sizeof(wg_hs_rl_summary)}};
    const HsRange in[4] = {{b->records, sizeof(wg_hs_record) * (uint64_t)n}, {b->n_records, b->n_records ? 4u : 0u},
                           {b->src, sizeof(wg_hs_src) * (uint64_t)b->n_src}, {b->now, 8u}};
    const int ov = hs_ranges_overlap(out, in);
    if (ov == 1) return fail(WG_EINVAL, "rl_status, out_records and rl_summary must not overlap");
    if (ov == 2) return fail(WG_EINVAL, "an output of wg_hs_ratelimit must not overlap records, n_records, src or now");
  }
  const bool capturing = stream_capturing(s);
  if ((rc = plan_begin(t->order, s, capturing, hs_rl_fits(t, n), [&] { return hs_rl_grow(t, n); }, kHsRlWords, n)) != WG_OK) return rc;
  RlHdr* hdr = (RlHdr*)t->d_rlhdr.p;
  if (b->flags & WG_HS_RL_COMPACT) {  // decided on the device, in front of the find
    wgrl::RlCompactParams Q{};
    Q.now = (const unsigned long long*)b->now;
    Q.n_records = b->n_records;
    Q.n = n;
    Q.in_call = 1u;
    rl_compact_launch(t, s, Q);
  }
  wgrl::RlParams P{};
  P.records = b->records;
  P.n_records = b->n_records;
  P.src = b->src;
  P.now = (const unsigned long long*)b->now;
  P.rl_status = b->rl_status;
  P.out_records = b->out_records;
  P.hdr = hdr;
  P.rec = (uint4*)t->d_rlrec.p;
  P.part = (uint4*)t->d_rlpart.p;
  P.n = n;
  P.n_src = b->n_src;
  const uint32_t nb = rank_blocks(n);
  const hipError_t me = hipMemsetAsync(&hdr->m, 0, 8, s);
  if (me != hipSuccess) return fail(WG_EDEVICE, "handshake ratelimit: %s", hipGetErrorString(me));
  hipLaunchKernelGGL(wgrl::k_rl_find, dim3(nb), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgrl::k_rl_claim<4u>, dim3(nb), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgrl::k_rl_claim<6u>, dim3(nb), dim3(256), 0, s, P);
  for (uint32_t j = 0; j < t->rl_burst; ++j) {
    P.round = j;
    hipLaunchKernelGGL(wgrl::k_rl_round, dim3(nb), dim3(256), 0, s, P);
  }
  rank_launch(wgrl::k_rl_decide, wgrl::k_rl_emit, P, b->rl_summary, s);
  return plan_end(t->order, s, capturing, kHsRlWords);
}

int wg_hs_rl_compact(wg_ctx* c, const uint64_t* now, wg_hs_rl_compact_summary* summary_dev, void* stream) {
  if (!c) return fail(WG_EINVAL, "NULL context");
  if (!now || (((uintptr_t)now) & 7u) || (((uintptr_t)summary_dev) & 7u)) return fail(WG_EINVAL, "now must be non-NULL, now and summary 8-byte aligned");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HsState* t;
  int rc;
  if ((rc = rl_get(c, "wg_hs_rl_compact", &t)) != WG_OK) return rc;
  if (!t->rl_burst) return fail(WG_ENOKEY, "wg_hs_rl_compact before any wg_hs_rl_config_set");
  const bool capturing = stream_capturing(s);
  if (!capturing && (rc = t->order.after_last(s)) != WG_OK) return rc;
  wgrl::RlCompactParams P{};
  P.now = (const unsigned long long*)now;
  P.summary = summary_dev;
  rl_compact_launch(t, s, P);
  return plan_end(t->order, s, capturing, kHsRlCompactWords);
}

int wg_hs_rl_dump(wg_ctx* c, wg_hs_rl_entry* out, uint32_t max_entries, uint32_t* n_out) {
  if (!c || !n_out || (!out && max_entries)) return fail(WG_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HsState* t;
  int rc;
  if ((rc = rl_get(c, "wg_hs_rl_dump", &t)) != WG_OK) return rc;
  HIPTRY(hipDeviceSynchronize());  // every call queued earlier (on any stream) has written its entries
  std::vector<wg_hs_rl_entry> v;
  if ((rc = rl_entries_read(c, t, &v)) != WG_OK) return rc;
  *n_out = (uint32_t)v.size();
  const size_t w = std::min<size_t>(v.size(), max_entries);
  if (w) memcpy(out, v.data(), sizeof(wg_hs_rl_entry) * w);
  return WG_OK;
}

int wg_hs_rl_load(wg_ctx* c, const wg_hs_rl_entry* entries, uint32_t n) {
  if (!c || (!entries && n)) return fail(WG_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HsState* t;
  int rc;
  if ((rc = rl_get(c, "wg_hs_rl_load", &t)) != WG_OK) return rc;
  HIPTRY(hipDeviceSynchronize());  // no call queued earlier (on any stream) may still read or write the old table
  RlHdr H;
  if ((rc = rl_hdr_read(c, t, &H)) != WG_OK) return rc;
  return rl_table_set(c, t, entries, n, H.cost, H.burst);
}

int wg_hs_rl_count(wg_ctx* c, uint32_t* used, uint32_t* capacity) {
  if (!c || !used || !capacity) return fail(WG_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HsState* t;
  int rc;
  if ((rc = rl_get(c, "wg_hs_rl_count", &t)) != WG_OK) return rc;
  HIPTRY(hipDeviceSynchronize());
  RlHdr H;
  if ((rc = rl_hdr_read(c, t, &H)) != WG_OK) return rc;
  *used = H.used;
  *capacity = H.mask + 1u;
  return WG_OK;
}

}  // extern "C"
