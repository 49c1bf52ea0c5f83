// wg_plan.hip — what the device planners share (included by wg_capi.hip before wg_rx.hip): wg_tx.hip,
// wg_rxplan.hip, wg_hs.hip, wg_x25519.hip and wg_hs_open.hip, and the replay check's stream order in wg_rx.hip.
//
// Fixed headers. What a planner's kernels read through a pointer that may move (route nodes, session
// entries, peer table) is named by a small header at a fixed device address; a setter rewrites the header
// behind a device synchronise, and a captured plan reads it when it runs, so a table change needs no
// re-capture (TxRouteHdr, RxSessHdr, HsPeerHdr).
//
// Stream order. A planner's state and scratch belong to the context, its calls may come on any stream:
// StreamOrder makes each call wait for the last one and leaves its own mark.
//
// Capture. A call on a capturing stream may neither allocate nor record the state's event into the graph:
// its scratch must have been reserved (plan_begin says which call reserves it), and it runs unordered
// against other streams, as the graph's owner replays it. Scratch grows only in plan_reserve.
//
// Ranks. A stable compaction over a batch is three launches on the call's stream (rank_launch): a first
// kernel leaves one 16-B record of counts per range of kRankRange items, k_rx_scan turns the records into
// their exclusive prefixes and writes the totals as the call's summary, a last kernel places.
//
// Small parts the session layer's calls share (wg_session.hip has the larger ones): k_fill_u32 / fill_u32,
// wave_elect beside block_rank, and range_copy, the body of the per-slot and per-peer getters and setters.
#pragma once

namespace {

constexpr uint32_t kRankRange = 256;  // items per workgroup of the first and last launch of a rank
uint32_t rank_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + kRankRange - 1u) / kRankRange); }

// MurmurHash3's fmix32
__host__ __device__ inline uint32_t mix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

bool stream_capturing(hipStream_t s) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
}

// The last use of a state that calls on any stream share: after_last orders stream s behind it (it may sit
// on another stream), mark makes what s has queued so far the last use. The owner's lock is held.
struct StreamOrder {
  StreamOrder() = default;
  StreamOrder(const StreamOrder&) = delete;
  StreamOrder& operator=(const StreamOrder&) = delete;
  ~StreamOrder() {
    if (ev) (void)hipEventDestroy(ev);
  }
  // mark creates the event where the owner has not: a state whose constructor path makes no HIP call (RxState)
  hipError_t create() { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
  int after_last(hipStream_t s) {
    if (last != s && last != never()) HIPTRY(hipStreamWaitEvent(s, ev, 0));  // (a stream is ordered behind itself)
    return WG_OK;
  }
  int mark(hipStream_t s) {
    HIPTRY(create());
    HIPTRY(hipEventRecord(ev, s));
    last = s;
    return WG_OK;
  }

 private:
  static hipStream_t never() { return (hipStream_t)-1; }  // no use yet (nullptr is a stream)
  hipEvent_t ev = nullptr;
  hipStream_t last = never();
};

// "<what> of %u <units> ..." / "<what> kernels: ..." in a planner's errors; <reserve> sizes its scratch
struct PlanWords {
  const char *what, *units, *reserve;
};

// The only place where a planner's scratch grows; never on a capturing stream (the caller checks).
template <class Grow>
int plan_reserve(bool fits, Grow grow) {
  if (fits) return WG_OK;
  HIPTRY(hipDeviceSynchronize());  // the scratch is reallocated under earlier calls
  return grow();
}

// Before a planner's launches of n items on stream s: the scratch (`fits`: it holds n items already) and
// the order behind the state's last use.
template <class Grow>
int plan_begin(StreamOrder& order, hipStream_t s, bool capturing, bool fits, Grow grow, const PlanWords& w, uint32_t n) {
  if (capturing) {
    if (!fits)
      return fail(WG_EINVAL, "%s of %u %s on a capturing stream needs more scratch: call %s(%u) first", w.what, n, w.units,
                  w.reserve, n);
    return WG_OK;
  }
  int rc;
  if ((rc = plan_reserve(fits, grow)) != WG_OK) return rc;
  return order.after_last(s);
}

// ... and after them. *launches_failed is set when one did not launch.
int plan_end(StreamOrder& order, hipStream_t s, bool capturing, const PlanWords& w, bool* launches_failed = nullptr) {
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) {
    if (launches_failed) *launches_failed = true;
    return fail(WG_EDEVICE, "%s kernels: %s", w.what, hipGetErrorString(le));
  }
  return capturing ? WG_OK : order.mark(s);
}

}  // namespace

// ---- device -------------------------------------------------------------------------------
namespace wgrp {

__device__ __forceinline__ uint64_t u64_of(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }

// the smaller of *n_dev and n (n if there is no device count): how much of a list a kernel walks
__device__ __forceinline__ uint32_t dev_count(const uint32_t* n_dev, uint32_t n) {
  if (!n_dev) return n;
  const uint32_t nd = *n_dev;
  return nd < n ? nd : n;
}

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, uint32_t d) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d);
  return u64_of(lo, hi);
}

// Over the 256 threads of the workgroup, in thread order: the flagged threads below me (rank) and in
// all (total). Every thread must reach the call; `wsum` is 4 words of LDS of this call's own.
__device__ __forceinline__ void block_rank(bool flag, uint32_t* wsum, uint32_t& rank, uint32_t& total) {
  const uint64_t m = __ballot(flag);
  const uint32_t w = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) wsum[w] = (uint32_t)__popcll((unsigned long long)m);
  __syncthreads();
  rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  total = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t x = wsum[k];
    rank += k < w ? x : 0u;
    total += x;
  }
}

// One atomic per wave where a wave's active lanes agree. Whether this lane should act on its `key`: if every active
// lane holds one key, only the first (LAST: the last) active lane, and `for_all` says that it acts for all of them;
// otherwise every active lane for itself. One ballot decides. Every lane of the wave must reach the call. (A round
// per distinct key was measured and dropped: 64 dependent round trips per wave on a spread batch, docs/EXPERIMENTS.md.)
template <bool LAST>
__device__ __forceinline__ bool wave_elect(bool active, uint32_t key, bool& for_all) {
  const uint64_t act = __ballot(active);
  for_all = false;
  if (!act) return false;
  const uint32_t l = LAST ? 63u - (uint32_t)__clzll((unsigned long long)act) : (uint32_t)__ffsll((unsigned long long)act) - 1u;
  const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)l);
  if (__ballot(active && key != k)) return active;
  for_all = true;
  return (threadIdx.x & 63u) == l;
}

// The same for a 64-bit value: the sum of v over the threads below me (excl) and over all (total).
__device__ __forceinline__ void block_scan64(uint64_t v, uint64_t* wsum, uint64_t& excl, uint64_t& total) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint64_t inc = v;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint64_t up = shfl_up64(inc, d);
    if (lane >= d) inc += up;
  }
  if (lane == 63u) wsum[w] = inc;
  __syncthreads();
  excl = inc - v;
  total = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    const uint64_t x = wsum[k];
    excl += k < w ? x : 0ull;
    total += x;
  }
}

__global__ void __launch_bounds__(256) k_fill_u32(uint32_t* p, uint32_t n, uint32_t value) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) p[i] = value;
}

// Exclusive prefixes of the per-range records, in place, and the totals as the 16-B summary
// {bytes, count, count} (wg_rx_summary / wg_rx_delivered). One workgroup.
__global__ void __launch_bounds__(256) k_rx_scan(uint4* part, uint32_t nb, uint2* summary) {
  __shared__ uint64_t s_sum[4];
  uint64_t run_bytes = 0;
  uint32_t run_a = 0, run_b = 0;
  for (uint32_t b0 = 0; b0 < nb; b0 += 256u) {  // (workgroup-uniform trips)
    const uint32_t b = b0 + threadIdx.x;
    const uint4 v = b < nb ? part[b] : make_uint4(0u, 0u, 0u, 0u);
    // counts of one range are <= 256: their scans run as 64-bit sums of a packed pair
    uint64_t ex, tot, exc, totc;
    block_scan64(u64_of(v.x, v.y), s_sum, ex, tot);
    __syncthreads();  // s_sum is read by every thread before the next scan writes it
    block_scan64(u64_of(v.z, v.w), s_sum, exc, totc);
    __syncthreads();
    if (b < nb) {
      const uint64_t pb = run_bytes + ex;
      part[b] = make_uint4((uint32_t)pb, (uint32_t)(pb >> 32), run_a + (uint32_t)exc, run_b + (uint32_t)(exc >> 32));
    }
    run_bytes += tot;
    run_a += (uint32_t)totc;
    run_b += (uint32_t)(totc >> 32);
  }
  if (threadIdx.x == 0) {  // (8-B stores: the summary need not be 16-B aligned)
    summary[0] = make_uint2((uint32_t)run_bytes, (uint32_t)(run_bytes >> 32));
    summary[1] = make_uint2(run_a, run_b);
  }
}

}  // namespace wgrp

namespace {

// p[0 .. n) = value on stream s: a claim array before its atomicMin, a map before its first entry
void fill_u32(hipStream_t s, void* p, uint32_t n, uint32_t value) {
  if (n) hipLaunchKernelGGL(wgrp::k_fill_u32, dim3(rank_blocks(n)), dim3(256), 0, s, (uint32_t*)p, n, value);
}

// Elements [first, first + n) of a state's device table `dev` (NULL: the state does not exist, and `unreserved` says
// which call creates it) of `limit` elements of `elem` bytes, to the host or from it, behind everything queued on any
// stream. The caller holds the context's lock and device.
int range_copy(void* dev, const char* unreserved, uint32_t first, uint32_t n, uint32_t limit, const char* units, void* host, size_t elem,
               bool to_host) {
  if (!dev) return fail(WG_EINVAL, "%s", unreserved);
  if ((uint64_t)first + n > limit) return fail(WG_ERANGE, "%s out of range", units);
  if (!n) return WG_OK;
  HIPTRY(hipDeviceSynchronize());
  uint8_t* d = (uint8_t*)dev + (size_t)first * elem;
  HIPTRY(hipMemcpy(to_host ? host : d, to_host ? d : host, (size_t)n * elem, to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice));
  return WG_OK;
}

// A rank over P.n items: `first` (one record per range to P.part), k_rx_scan (prefixes, and the totals as
// the 16-B `summary`), `last`; no workgroup waits on another.
template <class Params>
void rank_launch(void (*first)(Params), void (*last)(Params), const Params& P, void* summary, hipStream_t s) {
  const uint32_t nb = rank_blocks(P.n);
  hipLaunchKernelGGL(first, dim3(nb), dim3(256), 0, s, P);
  hipLaunchKernelGGL(wgrp::k_rx_scan, dim3(1), dim3(256), 0, s, P.part, nb, (uint2*)summary);
  hipLaunchKernelGGL(last, dim3(nb), dim3(256), 0, s, P);
}

}  // namespace
