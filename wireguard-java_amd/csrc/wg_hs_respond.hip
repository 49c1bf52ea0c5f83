// wg_hs_respond.hip — the answer to an initiation, on the device (included by wg_capi.hip after wg_hs_open.hip).
//
// wg_hs_open leaves authenticated initiations, by peer, with the Noise hash and chain key the responder goes
// on from. What the reference does next is the dearest part of the handshake: ResponderHandshake.deriveKeypair
// (Handshakes.java:250-287) and OutgoingResponse (OutgoingResponse.java:16-25, ResponsePacket.java:107-117): a
// fresh ephemeral key, three X25519 ladders, five HKDFs, an AEAD seal of nothing and a keyed BLAKE2s. The only
// thing the device lacks for it is randomness, and that arrives as a buffer: 32 bytes per initiation from the
// host's CSPRNG. wg_hs_respond turns wg_hs_open's entries into ready-to-send 92-byte responses and the
// transport key pairs.
//
// The chain (H = BLAKE2s-256, KDFn = Crypto.deriveKey(salt, ikm, n); h, ck, E_i, S_i from the entry; e = the
// clamped ephemeral; psk = 32 zero bytes, as the reference's responder hard-codes at :262):
//   Epub = X25519(e, 9)          h = H(h || Epub)         ck = KDF1(ck, Epub)
//   ck = KDF1(ck, X25519(e, E_i))                         ck = KDF1(ck, X25519(e, S_i))
//   tau = KDF2(ck, psk)   k = KDF3(ck, psk)   ck = KDF1(ck, psk)          (all three from the same ck)
//   h = H(h || tau)       empty = AEAD-seal(k, nonce 0, aad = h, "")       (the 16-byte tag)
//   recv_key = KDF1(ck, "")      send_key = KDF2(ck, "")                   (:286: the responder sends with T2)
//   response = {2, 0,0,0, LE32(local_index), LE32(sender_index), Epub, empty,
//               mac1 = BLAKE2s-128(key = H("mac1----" || S_i), response[0 .. 60)), mac2 = 0^16}
//
// k_hs_resp_dh: k_hs_dh's shape, one ladder per lane, wgx::x25519 as it is. Lane L of the grid runs ladder
// j = L % 3 of entry k = L / 3 (j = 0: the base point, 1: E_i, 2: S_i): the three ladders of one initiation sit
// in three neighbouring lanes and never follow one another in a lane, a wave holds 21 1/3 initiations, and
// lane L stores its 32 bytes at scratch + 32 L, so a wave's stores are one contiguous run and the entry's 96
// bytes are {Epub, e E_i, e S_i}. The three lanes of an entry read the same ephemeral and each decides the
// entry's status for itself. Waves wholly past 3 x cover exit as waves; a NOPEER or NOEPH lane, and a lane
// past the cover, runs the dummy ladder (scalar 0, u = 9) and stores nothing.
//
// k_hs_resp_chain: one entry per lane, 50 BLAKE2s compressions: the steps of kRespProgram (wg_hs_chain.h),
// written once in the order of the chain above, on the machine that k_hs_open runs on (wg_hs_chain.hip): ONE
// loop around ONE b2s_compress, uniform switches on the step's source, operation and destination, nothing
// indexed dynamically. The expands of one extract share the key-block states, and T1 is the message of T2.
// What this kernel adds to the generic operations: its sources (the three ladder results) and the three
// compressions of mac1. Three things do not occur in k_hs_open: KDFn(ck, "") has an empty message, so the
// inner hash's key block ck ^ 0x36.. is its LAST block (OP_PAD with PAD_LAST: t = 64, final); T3 follows T2
// (OP_TN with n = 3), each T_n hashing T_{n-1} || n, 33 bytes behind the key block (t = 97); and the AEAD has
// no ciphertext: the counter-0 chacha20_block gives the Poly1305 key, wghc::poly_tag runs over aad (32) ||
// LE64(32) || LE64(0), and there is no counter-1 block. The seal hangs on the one key-block step that
// carries PAD_SEAL, the last at which x still holds k. After the loop the lane writes its 176-byte session to
// scratch and overwrites the entry's 96 bytes of ladder scratch and its consumed ephemeral with zeros (plain
// 16-byte vector stores).
//
// The loop's bound is the plain constant kRespSteps. An earlier form of this loop, two switches over the step
// counter itself with hand-numbered case lists, came out of hipcc (ROCm 7.2, clang 22, -O3, gfx950) with the
// literal bound 50 computing a wrong encrypted_empty and wrong transport keys for every entry, and carried
// its bound through an empty asm statement to hide it from the optimiser. The cause inside the compiler was
// not found. In this form the switches depend on bytes loaded from the program, not on a counter of known
// range, and the build with the constant bound passes tests/test_gpu_hs_respond.py in full; that test compares
// every byte, so a build that goes wrong again fails there, while tests/test_hs_chain.py tells a wrong
// program from a wrong build without a GPU.
//
// Constant time: no branch, address or loop bound depends on an ephemeral's value, a DH result, ck, tau, k or a
// transport key. The program is public and indexed by a public counter. The two exceptions are the all-zero
// test of the raw ephemeral (NOEPH) and the entry's peer (NOPEER); the branches depend on the program, on
// those statuses and on the counts alone.
//
// Ranks. sessions[0 .. n_ok) is the stable compaction of the OK entries, by rank_launch: k_hs_resp_chain
// leaves the sessions in scratch and one 16-B record {ok, nopeer, noeph, 0} per 256 entries, k_rx_scan (as it
// is) turns them into prefixes and the summary, k_hs_resp_emit places, and wipes the keys it moved. No
// workgroup waits on another; every scratch word is written before it is read in each call.
#pragma once

namespace wghr {

constexpr uint32_t kLadU4 = 6;   // ladder scratch per entry, in uint4: Epub, e E_i, e S_i
constexpr uint32_t kSessU4 = 11; // a wg_hs_session, in uint4

struct RespParams {
  const wg_hs_init* inits;
  const uint32_t* n_inits;
  uint8_t* ephemerals;
  const uint32_t* local_index;
  uint32_t* resp_status;
  wg_hs_session* sessions;
  uint4* lad;
  uint4* res;
  uint4* part;
  uint32_t n;
  uint32_t flags;
};

__device__ __forceinline__ uint32_t resp_len(const RespParams& P) { return wgrp::dev_count(P.n_inits, P.n); }

// the status of entry k (k below the cover), and its raw ephemeral
__device__ __forceinline__ uint32_t resp_status_of(const RespParams& P, uint32_t k, uint4& e0, uint4& e1) {
  const uint4* ep = (const uint4*)(P.ephemerals + 32ull * k);
  e0 = ep[0];
  e1 = ep[1];
  if ((P.flags & WG_HS_RESP_SKIP_NEWPEER) && ((const uint4*)(P.inits + k))[0].w == WG_HS_NOPEER) return WG_HS_RESP_NOPEER;
  const uint32_t any = e0.x | e0.y | e0.z | e0.w | e1.x | e1.y | e1.z | e1.w;
  return any ? WG_HS_RESP_OK : WG_HS_RESP_NOEPH;
}

// lane L: ladder L % 3 of entry L / 3, its 32 bytes to lad + 2 L
__global__ void __launch_bounds__(64) k_hs_resp_dh(RespParams P) {
  const uint64_t lanes = 3ull * resp_len(P);
  if ((uint64_t)blockIdx.x * 64u >= lanes) return;  // (wave-uniform)
  const uint64_t L = (uint64_t)blockIdx.x * 64u + threadIdx.x;
  uint32_t k[8], u[8], out[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    k[j] = 0u;
    u[j] = j == 0 ? 9u : 0u;
  }
  bool go = false;
  if (L < lanes) {
    const uint32_t i = (uint32_t)(L / 3u), which = (uint32_t)(L - 3ull * i);
    uint4 e0, e1;
    go = resp_status_of(P, i, e0, e1) == WG_HS_RESP_OK;
    if (go) {
      k[0] = e0.x; k[1] = e0.y; k[2] = e0.z; k[3] = e0.w; k[4] = e1.x; k[5] = e1.y; k[6] = e1.z; k[7] = e1.w;
      if (which) {  // remote_ephemeral at 16, remote_static at 48 of the entry
        const uint4* pt = (const uint4*)(P.inits + i) + (2u * which - 1u);
        const uint4 p0 = pt[0], p1 = pt[1];
        u[0] = p0.x; u[1] = p0.y; u[2] = p0.z; u[3] = p0.w; u[4] = p1.x; u[5] = p1.y; u[6] = p1.z; u[7] = p1.w;
      }
    }
  }
  (void)wgx::x25519(out, k, u);
  if (!go) return;
  uint4* o = P.lad + 2ull * L;
  o[0] = make_uint4(out[0], out[1], out[2], out[3]);
  o[1] = make_uint4(out[4], out[5], out[6], out[7]);
}

// tag = Poly1305(aad (32) || LE64(32) || LE64(0)) under the one-time key of `key`, nonce 0: the seal of nothing
__device__ __forceinline__ void seal_empty(const uint32_t key[8], const uint32_t aad[8], uint32_t tag[4]) {
  uint32_t ks[16];
  wgd::chacha20_block(key, 0u, 0u, 0u, 0u, ks);
  wghc::poly_tag<0>(ks, aad, nullptr, tag);
}

// One entry per lane: status, and for an OK one its session to scratch; the range's counts.
__global__ void __launch_bounds__(256) k_hs_resp_chain(RespParams P) {
  __shared__ uint32_t s_cnt[3][4];
  const uint32_t nl = resp_len(P);
  if (blockIdx.x * kRankRange >= nl) {  // past the entries (workgroup-uniform): a zero record for the scan
    if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const uint32_t k = blockIdx.x * kRankRange + threadIdx.x;
  const bool in = k < nl;
  uint32_t st_out = WG_HS_RESP_NOEPH;
  if ((k & ~63u) < nl) {  // (wave-uniform: a wave wholly past the entries goes straight to the counts)
    uint4 e0, e1;
    if (in) st_out = resp_status_of(P, k, e0, e1);
    const bool go = in && st_out == WG_HS_RESP_OK;
    // a lane that answers nothing runs the chain over zeros and stores nothing
    const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
    const uint4* ent = (const uint4*)(P.inits + (go ? k : 0u));
    const uint4* lad = P.lad + (size_t)kLadU4 * (go ? k : 0u);
    using namespace wghc;
    Chain c;
    clear(c);
    uint32_t tag[4] = {0u, 0u, 0u, 0u};
    if (go) {
      put8(c.hh, ent[5], ent[6]);
      put8(c.ck, ent[7], ent[8]);
    }
    const uint32_t li = go ? P.local_index[k] : 0u;
    Step s = fetch(kRespProgram, 0u);
#pragma unroll 1
    for (uint32_t step = 0; step < kRespSteps; ++step) {
      uint32_t src[8];
      switch (s.arg) {
        case SRC_EPUB: put8(src, go ? lad[0] : z4, go ? lad[1] : z4); break;
        case SRC_EE: put8(src, go ? lad[2] : z4, go ? lad[3] : z4); break;
        case SRC_ES: put8(src, go ? lad[4] : z4, go ? lad[5] : z4); break;
        default: source(c, s.arg, src); break;
      }
      switch (s.op) {
        case OP_MAC1KEY: {  // the mac1 key, H("mac1----" || S_i): 40 bytes
          uint32_t w[8];
          put8(w, go ? ent[3] : z4, go ? ent[4] : z4);
          c.m[0] = 0x3163616Du;
          c.m[1] = 0x2D2D2D2Du;
          set8(c.m + 2, w);
#pragma unroll
          for (int j = 10; j < 16; ++j) c.m[j] = 0u;
          wghs::b2s_init(c.st, 32u, 0u);
          c.t = 40u; c.last = true;
          break;
        }
        case OP_MAC1A:  // mac1 = BLAKE2s-128 under that key (in ist): the key block
          msg32(c.m, c.ist);
          wghs::b2s_init(c.st, 16u, 32u);
          c.t = 64u; c.last = false;
          break;
        case OP_MAC1B: {  // ... and response[0 .. 60)
          uint32_t w[8];
          put8(w, go ? lad[0] : z4, go ? lad[1] : z4);
          c.m[0] = 2u;
          c.m[1] = li;
          c.m[2] = go ? ent[0].z : 0u;
          set8(c.m + 3, w);
          c.m[11] = tag[0]; c.m[12] = tag[1]; c.m[13] = tag[2]; c.m[14] = tag[3];
          c.m[15] = 0u;
          c.t = 124u; c.last = true;
          break;
        }
        default:
          // the flagged key block: x = k, the seal of nothing under it, before the transport keys' KDF takes x
          if (s.op == OP_PAD && (s.imm & PAD_SEAL)) seal_empty(c.x, c.hh, tag);
          prepare(c, s, src);
          break;
      }
      const Step ahead = fetch(kRespProgram, step + 1u);
      wghs::b2s_compress(c.st, c.m, c.t, c.last);
      WG_HSC_PUT(c, s.dst);
      s = ahead;
    }
    if (go) {
      const uint4 q0 = ent[0];  // {index, record, sender_index, peer}
      const uint4 a = lad[0], b = lad[1];
      uint4* o = P.res + (size_t)kSessU4 * k;
      o[0] = make_uint4(q0.x, k, q0.w, li);
      o[1] = make_uint4(2u, li, q0.z, a.x);
      o[2] = make_uint4(a.y, a.z, a.w, b.x);
      o[3] = make_uint4(b.y, b.z, b.w, tag[0]);
      o[4] = make_uint4(tag[1], tag[2], tag[3], c.st[0]);
      o[5] = make_uint4(c.st[1], c.st[2], c.st[3], 0u);
      o[6] = make_uint4(0u, 0u, 0u, q0.z);
      o[7] = make_uint4(c.x[0], c.x[1], c.x[2], c.x[3]);
      o[8] = make_uint4(c.x[4], c.x[5], c.x[6], c.x[7]);
      o[9] = make_uint4(c.ck[0], c.ck[1], c.ck[2], c.ck[3]);
      o[10] = make_uint4(c.ck[4], c.ck[5], c.ck[6], c.ck[7]);
      // the ladders' results and the ephemeral are spent
      uint4* wl = P.lad + (size_t)kLadU4 * k;
#pragma unroll
      for (uint32_t g = 0; g < kLadU4; ++g) wl[g] = z4;
      uint4* we = (uint4*)(P.ephemerals + 32ull * k);
      we[0] = z4;
      we[1] = z4;
    }
    if (in) P.resp_status[k] = st_out;
  }
  uint32_t r, n_ok, n_nopeer, n_noeph;
  wgrp::block_rank(in && st_out == WG_HS_RESP_OK, s_cnt[0], r, n_ok);
  wgrp::block_rank(in && st_out == WG_HS_RESP_NOPEER, s_cnt[1], r, n_nopeer);
  wgrp::block_rank(in && st_out == WG_HS_RESP_NOEPH, s_cnt[2], r, n_noeph);
  if (threadIdx.x == 0) P.part[blockIdx.x] = make_uint4(n_ok, n_nopeer, n_noeph, 0u);
}

// sessions[prefix of the range + rank in the range] = the session of this entry; its keys leave the scratch
__global__ void __launch_bounds__(256) k_hs_resp_emit(RespParams P) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t nl = resp_len(P);
  if (blockIdx.x * kRankRange >= nl) return;  // (workgroup-uniform)
  const uint32_t k = blockIdx.x * kRankRange + threadIdx.x;
  const bool ok = k < nl && P.resp_status[k] == WG_HS_RESP_OK;
  const uint4 pre = P.part[blockIdx.x];
  uint32_t r, total;
  wgrp::block_rank(ok, s_cnt, r, total);
  if (!ok) return;
  uint4* in = P.res + (size_t)kSessU4 * k;
  uint4* o = (uint4*)(P.sessions + (pre.x + r));
#pragma unroll
  for (uint32_t g = 0; g < kSessU4; ++g) o[g] = in[g];
#pragma unroll
  for (uint32_t g = 7; g < kSessU4; ++g) in[g] = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace wghr

// ---- C ABI --------------------------------------------------------------------------------
extern "C" {

int wg_hs_respond(wg_ctx* c, const wg_hs_respond_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  if (b->flags & ~WG_HS_RESP_SKIP_NEWPEER) return fail(WG_EINVAL, "unknown wg_hs_respond flag bits 0x%x", b->flags & ~WG_HS_RESP_SKIP_NEWPEER);
  if (((uintptr_t)b->n_inits) & 3u) return fail(WG_EINVAL, "n_inits must be 4-byte aligned");
  hipStream_t s = pick_stream(c, stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (!c->hs || !c->hs->has_priv) return fail(WG_ENOKEY, "wg_hs_respond before any wg_hs_static_set");
  HsState* t = c->hs;
  const uint32_t n = b->n;
  if (n == 0) return WG_OK;
  if (n > 0x40000000u) return fail(WG_E2BIG, "handshake respond of %u entries", n);
  if (!b->inits || (((uintptr_t)b->inits) & 15u) || !b->ephemerals || (((uintptr_t)b->ephemerals) & 15u) || !b->local_index ||
      (((uintptr_t)b->local_index) & 3u))
    return fail(WG_EINVAL, "inits / ephemerals / local_index must be non-NULL and aligned (16 / 16 / 4 bytes)");
  if (!b->resp_status || (((uintptr_t)b->resp_status) & 3u) || !b->sessions || (((uintptr_t)b->sessions) & 15u) || !b->summary ||
      (((uintptr_t)b->summary) & 7u))
    return fail(WG_EINVAL, "resp_status / sessions / summary must be non-NULL and aligned (4 / 16 / 8 bytes)");
  {
    const HsRange out[4] = {{b->ephemerals, 32ull * n}, {b->resp_status, 4ull * n}, {b->sessions, sizeof(wg_hs_session) * (uint64_t)n},
                            {b->summary, sizeof(wg_hs_respond_summary)}};
    const HsRange in[3] = {{b->inits, sizeof(wg_hs_init) * (uint64_t)n}, {b->local_index, 4ull * n}, {b->n_inits, b->n_inits ? 4u : 0u}};
    const int ov = hs_ranges_overlap(out, in);
    if (ov == 1) return fail(WG_EINVAL, "ephemerals, resp_status, sessions and summary must not overlap");
    if (ov == 2) return fail(WG_EINVAL, "an output of wg_hs_respond must not overlap inits, local_index or n_inits");
  }
  const bool capturing = stream_capturing(s);
  int rc;
  if ((rc = plan_begin(t->order, s, capturing, hs_resp_fits(t, n), [&] { return hs_resp_grow(t, n); }, kHsRespWords, n)) != WG_OK) return rc;
  wghr::RespParams P{};
  P.inits = b->inits;
  P.n_inits = b->n_inits;
  P.ephemerals = b->ephemerals;
  P.local_index = b->local_index;
  P.resp_status = b->resp_status;
  P.sessions = b->sessions;
  P.lad = (uint4*)t->d_rlad.p;
  P.res = (uint4*)t->d_rres.p;
  P.part = (uint4*)t->d_rpart.p;
  P.n = n;
  P.flags = b->flags;
  hipLaunchKernelGGL(wghr::k_hs_resp_dh, dim3((uint32_t)((3ull * n + 63u) / 64u)), dim3(64), 0, s, P);
  rank_launch(wghr::k_hs_resp_chain, wghr::k_hs_resp_emit, P, b->summary, s);
  return plan_end(t->order, s, capturing, kHsRespWords);
}

}  // extern "C"
