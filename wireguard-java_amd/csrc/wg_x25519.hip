// wg_x25519.hip — batched X25519 (RFC 7748 §5) and the initiations' static DH, on the device (included by
// wg_capi.hip after wg_hs.hip).
//
// After wg_hs_check a UDP ring is a compact list of handshake messages with a correct mac1. mac1 needs only
// the local static PUBLIC key, so anyone who knows it can make such messages at line rate, and the first
// thing the responder does with each is localKeypair.sharedSecret(remoteEphemeral) (Handshakes.java:210): one
// Curve25519 ladder per datagram, independent across datagrams, pure arithmetic. wg_x25519_batch is that
// primitive over descriptors (the analogue of wg_blake2s_batch); wg_hs_dh runs it over wg_hs_check's records
// with the static private key that wg_hs_static_set left at a fixed device address.
//
// Semantics: X25519.scalarMult / calculateAgreement (crypto/internal/X25519.java:24-28, 50-60, 96-155;
// X25519Field.decode :123-128): the scalar is clamped here, bit 255 of u is ignored, a non-canonical u is
// reduced by the arithmetic, the output is the canonical x2 * z2^(p-2) mod p, and an all-zero output is
// written and flagged (NoisePrivateKey.sharedSecret ignores calculateAgreement's false).
//
// One scalar multiplication per lane. A field element is ten limbs of 26 / 25 bits (X25519Field's radix);
// products are (uint64_t)a * b + acc, which the compiler issues as v_mad_u64_u32 chains into 64-bit
// accumulators; squaring is its own routine (55 products). Bounds: a product's or square's output has limbs
// below 2^26 (even) / 2^25 + 2^18 (odd); its inputs may be a sum (below 2^27.1 / 2^26.1) or a biased
// difference (below 2^27.6 / 2^26.6) of two such outputs: the largest factor is then 38 * 2^26.6 < 2^32 and
// an accumulator holds at most 10 * 19 * 2^55.2 < 2^62.8. The ladder is RFC 7748's (5 mul + 4 sqr + one
// x 121665 per step) over 256 bits: the clamped bit 255 is zero, and a step on (1 : 0), (x1 : 1) with a zero
// bit leaves both points where they were, projectively. The inversion is the usual 254-squaring chain.
//
// Constant time: no branch, no address and no loop bound depends on a scalar bit or a field value. The
// conditional swap is a mask on the lane's own bit; the final reduction and the zero test are arithmetic.
// The eight scalar words stay in VGPRs and are walked by an outer loop that shifts them down one register
// and an inner loop over the top word's bits, so no register is indexed dynamically. Lanes past n and
// lanes with a bad descriptor run the same ladder on dummy operands (scalar 0, u = 9) and store nothing;
// wg_hs_dh's waves that lie wholly past the record count exit as whole waves.
#pragma once

namespace wgx {

constexpr uint32_t M26 = 0x3FFFFFFu, M25 = 0x1FFFFFFu;

struct X25519Params {
  const wg_x25519_desc* desc;
  const uint8_t* in;
  uint64_t in_size;
  uint8_t* out;
  uint64_t out_size;
  uint32_t* status;
  uint32_t n;
};

struct DhParams {
  const wg_hs_record* records;
  const uint32_t* n_records;
  uint8_t* shared;
  uint32_t* dh_status;
  const uint8_t* key;
  uint32_t n;
};

// t[0..10) -> limbs: each limb's carry goes into the next accumulator, the top one times 19 into limb 0
__device__ __forceinline__ void fe_carry(uint64_t t[10], uint32_t h[10]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const uint32_t bits = (k & 1) ? 25u : 26u;
    h[k] = (uint32_t)t[k] & ((k & 1) ? M25 : M26);
    t[k + 1] += t[k] >> bits;
  }
  h[9] = (uint32_t)t[9] & M25;
  const uint64_t z = (uint64_t)h[0] + (t[9] >> 25) * 19u;
  h[0] = (uint32_t)z & M26;
  h[1] += (uint32_t)(z >> 26);
}

// h = f * g. h may be f or g.
__device__ __forceinline__ void fe_mul(uint32_t h[10], const uint32_t f[10], const uint32_t g[10]) {
  uint32_t f2[10], g19[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    f2[i] = 2u * f[i];
    g19[i] = 19u * g[i];
  }
  uint64_t t[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    uint64_t acc = 0;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
      const int j = (k - i + 10) % 10;  // i + j = k, or k + 10: that term wraps, times 19
      const uint32_t a = ((i & 1) && (j & 1)) ? f2[i] : f[i];  // two odd limbs: 2^25.5 twice is one bit more
      const uint32_t b = i > k ? g19[j] : g[j];
      acc += (uint64_t)a * b;
    }
    t[k] = acc;
  }
  fe_carry(t, h);
}

// h = f * f: 55 products. h may be f.
__device__ __forceinline__ void fe_sq(uint32_t h[10], const uint32_t f[10]) {
  uint32_t f2[10], f19[10], f38[10];  // (those that no term takes are dropped by the compiler)
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    f2[i] = 2u * f[i];
    f19[i] = 19u * f[i];
    f38[i] = 38u * f[i];
  }
  uint64_t t[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    uint64_t acc = 0;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
      const int j = (k - i + 10) % 10;
      if (i > j) continue;
      const bool odd2 = (i & 1) && (j & 1), wrap = i > k;
      const uint32_t a = i < j ? f2[i] : f[i];  // a cross term counts twice
      const uint32_t b = wrap ? (odd2 ? f38[j] : f19[j]) : (odd2 ? f2[j] : f[j]);
      acc += (uint64_t)a * b;
    }
    t[k] = acc;
  }
  fe_carry(t, h);
}

// h = 121665 f
__device__ __forceinline__ void fe_mul121665(uint32_t h[10], const uint32_t f[10]) {
  uint64_t t[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) t[i] = (uint64_t)f[i] * 121665u;
  fe_carry(t, h);
}

__device__ __forceinline__ void fe_add(uint32_t h[10], const uint32_t f[10], const uint32_t g[10]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) h[i] = f[i] + g[i];
}

// h = f - g + 2p, limb by limb; g is a product's output (below the limbs of 2p)
__device__ __forceinline__ void fe_sub(uint32_t h[10], const uint32_t f[10], const uint32_t g[10]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) h[i] = f[i] + (i == 0 ? 0x7FFFFDAu : (i & 1) ? 0x3FFFFFEu : 0x7FFFFFEu) - g[i];
}

__device__ __forceinline__ void fe_cswap(uint32_t f[10], uint32_t g[10], uint32_t mask) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t x = (f[i] ^ g[i]) & mask;
    f[i] ^= x;
    g[i] ^= x;
  }
}

// h = h^(2^n); the loop is kept a loop (code size)
__device__ __forceinline__ void fe_sqn(uint32_t h[10], uint32_t n) {
#pragma unroll 1
  for (uint32_t k = 0; k < n; ++k) fe_sq(h, h);
}

// out = z^(p - 2): 254 squarings and 11 products
__device__ __forceinline__ void fe_invert(uint32_t out[10], const uint32_t z[10]) {
  uint32_t t0[10], t1[10], t2[10], t3[10];
  fe_sq(t0, z);        // 2
  fe_sq(t1, t0);
  fe_sq(t1, t1);       // 8
  fe_mul(t1, z, t1);   // 9
  fe_mul(t0, t0, t1);  // 11
  fe_sq(t2, t0);       // 22
  fe_mul(t1, t1, t2);  // 2^5 - 1
  fe_sq(t2, t1);
  fe_sqn(t2, 4);
  fe_mul(t1, t2, t1);  // 2^10 - 1
  fe_sq(t2, t1);
  fe_sqn(t2, 9);
  fe_mul(t2, t2, t1);  // 2^20 - 1
  fe_sq(t3, t2);
  fe_sqn(t3, 19);
  fe_mul(t2, t3, t2);  // 2^40 - 1
  fe_sqn(t2, 10);
  fe_mul(t1, t2, t1);  // 2^50 - 1
  fe_sq(t2, t1);
  fe_sqn(t2, 49);
  fe_mul(t2, t2, t1);  // 2^100 - 1
  fe_sq(t3, t2);
  fe_sqn(t3, 99);
  fe_mul(t2, t3, t2);  // 2^200 - 1
  fe_sqn(t2, 50);
  fe_mul(t1, t2, t1);  // 2^250 - 1
  fe_sqn(t1, 5);
  fe_mul(out, t1, t0);  // 2^255 - 21
}

// eight little-endian words -> limbs; bit 255 is dropped (X25519Field.decode)
__device__ __forceinline__ void fe_decode(uint32_t h[10], const uint32_t w[8]) {
  h[0] = w[0] & M26;
  h[1] = __builtin_amdgcn_alignbit(w[1], w[0], 26) & M25;
  h[2] = __builtin_amdgcn_alignbit(w[2], w[1], 19) & M26;
  h[3] = __builtin_amdgcn_alignbit(w[3], w[2], 13) & M25;
  h[4] = w[3] >> 6;
  h[5] = w[4] & M25;
  h[6] = __builtin_amdgcn_alignbit(w[5], w[4], 25) & M26;
  h[7] = __builtin_amdgcn_alignbit(w[6], w[5], 19) & M25;
  h[8] = __builtin_amdgcn_alignbit(w[7], w[6], 12) & M26;
  h[9] = (w[7] >> 6) & M25;
}

// limbs of a product's output -> the canonical value's eight words; returns the OR of them (0: the value is 0)
__device__ __forceinline__ uint32_t fe_encode(uint32_t w[8], uint32_t h[10]) {
  // two plain carry passes: after the first, limbs 1..9 fit and limb 0 is below 2^26 + 19; after the second all fit
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      h[k + 1] += h[k] >> ((k & 1) ? 25u : 26u);
      h[k] &= (k & 1) ? M25 : M26;
    }
    h[0] += 19u * (h[9] >> 25);
    h[9] &= M25;
  }
  // q = (h + 19) >> 255: 1 when h >= p; then h + 19 q mod 2^255 = h - q p
  uint32_t q = (h[0] + 19u) >> 26;
#pragma unroll
  for (int k = 1; k < 10; ++k) q = (h[k] + q) >> ((k & 1) ? 25u : 26u);
  h[0] += 19u * q;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    h[k + 1] += h[k] >> ((k & 1) ? 25u : 26u);
    h[k] &= (k & 1) ? M25 : M26;
  }
  h[9] &= M25;
  w[0] = h[0] | (h[1] << 26);
  w[1] = (h[1] >> 6) | (h[2] << 19);
  w[2] = (h[2] >> 13) | (h[3] << 13);
  w[3] = (h[3] >> 19) | (h[4] << 6);
  w[4] = h[5] | (h[6] << 25);
  w[5] = (h[6] >> 7) | (h[7] << 19);
  w[6] = (h[7] >> 13) | (h[8] << 12);
  w[7] = (h[8] >> 20) | (h[9] << 6);
  return w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7];
}

// out = X25519(k, u) (RFC 7748 5); returns the OR of the output's words
__device__ __forceinline__ uint32_t x25519(uint32_t out[8], const uint32_t scalar[8], const uint32_t u[8]) {
  uint32_t k0 = scalar[0] & 0xFFFFFFF8u, k1 = scalar[1], k2 = scalar[2], k3 = scalar[3], k4 = scalar[4], k5 = scalar[5],
           k6 = scalar[6], k7 = (scalar[7] & 0x7FFFFFFFu) | 0x40000000u;
  uint32_t x1[10], x2[10], z2[10], x3[10], z3[10], a[10], b[10];
  fe_decode(x1, u);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    x2[i] = i == 0 ? 1u : 0u;
    z2[i] = 0u;
    x3[i] = x1[i];
    z3[i] = i == 0 ? 1u : 0u;
  }
  uint32_t swap = 0;
#pragma unroll 1
  for (uint32_t wi = 0; wi < 8; ++wi) {
    uint32_t w = k7;  // the words move down one register: bits 255..224 first
    k7 = k6; k6 = k5; k5 = k4; k4 = k3; k3 = k2; k2 = k1; k1 = k0;
#pragma unroll 1
    for (uint32_t bi = 0; bi < 32; ++bi) {
      const uint32_t bit = w >> 31;
      w <<= 1;
      swap ^= bit;
      const uint32_t mask = 0u - swap;
      fe_cswap(x2, x3, mask);
      fe_cswap(z2, z3, mask);
      swap = bit;
      fe_add(a, x2, z2);   // A
      fe_sub(b, x2, z2);   // B
      fe_add(x2, x3, z3);  // C
      fe_sub(z2, x3, z3);  // D
      fe_mul(z3, z2, a);   // DA
      fe_mul(x3, x2, b);   // CB
      fe_add(x2, z3, x3);
      fe_sub(z2, z3, x3);
      fe_sq(x3, x2);       // x3 = (DA + CB)^2
      fe_sq(z3, z2);
      fe_mul(z3, z3, x1);  // z3 = x1 (DA - CB)^2
      fe_sq(a, a);         // AA
      fe_sq(b, b);         // BB
      fe_mul(x2, a, b);    // x2 = AA BB
      fe_sub(b, a, b);     // E
      fe_mul121665(z2, b);
      fe_add(z2, z2, a);
      fe_mul(z2, z2, b);   // z2 = E (AA + 121665 E)
    }
  }
  const uint32_t mask = 0u - swap;
  fe_cswap(x2, x3, mask);
  fe_cswap(z2, z3, mask);
  fe_invert(z2, z2);
  fe_mul(x2, x2, z2);
  return fe_encode(out, x2);
}

// the 32 bytes at p as eight little-endian words: the aligned words that hold at least one of them, never
// another (an index past the last such word is clamped to it), shifted into place
__device__ __forceinline__ void load32(const uint8_t* p, uint32_t w[8]) {
  const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
  const uint32_t* base = (const uint32_t*)(p - mis);
  const uint32_t jlast = mis ? 8u : 7u;
  uint32_t r[9];
#pragma unroll
  for (uint32_t j = 0; j < 9; ++j) r[j] = base[j < jlast ? j : jlast];
  const uint32_t sh = 8u * mis;
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k) w[k] = __builtin_amdgcn_alignbit(r[k + 1], r[k], sh);
}

// (off <= size && 32 <= size - off: no sum that could wrap)
__device__ __forceinline__ bool in32(uint64_t off, uint64_t size) { return off <= size && 32u <= size - off; }

__global__ void __launch_bounds__(64) k_x25519(X25519Params P) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  uint32_t k[8], u[8], out[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    k[j] = 0u;
    u[j] = j == 0 ? 9u : 0u;
  }
  bool ok = false;
  uint64_t out_off = 0;
  if (i < P.n) {
    const uint4* d = (const uint4*)(P.desc + i);
    const uint4 a = d[0], b = d[1];
    const uint64_t scalar_off = wgrp::u64_of(a.x, a.y), point_off = wgrp::u64_of(a.z, a.w);
    out_off = wgrp::u64_of(b.x, b.y);
    const bool base = (b.z & WG_X25519_BASE) != 0;
    ok = (b.z & ~WG_X25519_BASE) == 0 && b.w == 0 && in32(scalar_off, P.in_size) &&
         (base || in32(point_off, P.in_size)) && in32(out_off, P.out_size);
    if (ok) {
      load32(P.in + scalar_off, k);
      if (!base) load32(P.in + point_off, u);
    }
  }
  const uint32_t any = x25519(out, k, u);
  if (i >= P.n) return;
  if (ok) {
    uint8_t* o = P.out + out_off;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) wgt::store_u32_any(o + 4u * j, out[j]);
  }
  P.status[i] = !ok ? WG_X25519_BADDESC : any ? WG_X25519_OK : WG_X25519_ZERO;
}

// record k < min(*n_records, n): an initiation's ephemeral under the static private key
__global__ void __launch_bounds__(64) k_hs_dh(DhParams P) {
  const uint32_t nl = wgrp::dev_count(P.n_records, P.n);
  if (blockIdx.x * 64u >= nl) return;  // (wave-uniform)
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  uint32_t k[8], u[8], out[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    k[j] = 0u;
    u[j] = j == 0 ? 9u : 0u;
  }
  const bool in = i < nl;
  uint32_t len = 0;
  if (in) {
    const uint4* rec = (const uint4*)(P.records + i);
    len = rec[0].y;
    if (len == WG_HS_INIT_SIZE) {  // msg[8 .. 40) = bytes 16 .. 48 of the record (InitiationPacket.java:35-44)
      const uint4 e0 = rec[1], e1 = rec[2];
      const uint4 s0 = ((const uint4*)P.key)[0], s1 = ((const uint4*)P.key)[1];
      u[0] = e0.x; u[1] = e0.y; u[2] = e0.z; u[3] = e0.w; u[4] = e1.x; u[5] = e1.y; u[6] = e1.z; u[7] = e1.w;
      k[0] = s0.x; k[1] = s0.y; k[2] = s0.z; k[3] = s0.w; k[4] = s1.x; k[5] = s1.y; k[6] = s1.z; k[7] = s1.w;
    }
  }
  const uint32_t any = x25519(out, k, u);
  if (!in) return;
  uint4* sh = (uint4*)(P.shared + 32ull * i);
  if (len == WG_HS_INIT_SIZE) {
    sh[0] = make_uint4(out[0], out[1], out[2], out[3]);
    sh[1] = make_uint4(out[4], out[5], out[6], out[7]);
    P.dh_status[i] = any ? WG_X25519_OK : WG_X25519_ZERO;
  } else if (len == WG_HS_RESP_SIZE) {  // the host holds that handshake's ephemeral private key (Handshakes.java:125)
    sh[0] = make_uint4(0u, 0u, 0u, 0u);
    sh[1] = make_uint4(0u, 0u, 0u, 0u);
    P.dh_status[i] = WG_X25519_SKIPPED;
  } else {
    P.dh_status[i] = WG_X25519_BADDESC;
  }
}

}  // namespace wgx

// ---- C ABI --------------------------------------------------------------------------------
namespace {

int x25519_launch(const wg_x25519_desc* desc, uint32_t n, const uint8_t* in, uint64_t in_size, uint8_t* out,
                  uint64_t out_size, uint32_t* status, hipStream_t s) {
  wgx::X25519Params P{};
  P.desc = desc;
  P.in = in;
  P.in_size = in_size;
  P.out = out;
  P.out_size = out_size;
  P.status = status;
  P.n = n;
  hipLaunchKernelGGL(wgx::k_x25519, dim3((n + 63u) / 64u), dim3(64), 0, s, P);
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) return fail(WG_EDEVICE, "k_x25519 launch: %s", hipGetErrorString(le));
  return WG_OK;
}

}  // namespace

extern "C" {

int wg_x25519_batch(wg_ctx* c, const wg_x25519_desc* desc, uint32_t n, const uint8_t* in, uint64_t in_size, uint8_t* out,
                    uint64_t out_size, uint32_t* status, void* stream) {
  if (!c) return fail(WG_EINVAL, "NULL context");
  if (n == 0) return WG_OK;
  if (!desc || (((uintptr_t)desc) & 15u)) return fail(WG_EINVAL, "descriptor array must be non-NULL and 16-byte aligned");
  if (!in || !out || !status || (((uintptr_t)status) & 3u))
    return fail(WG_EINVAL, "NULL input, output or status array (status: 4-byte aligned)");
  if (open_overlaps(in, in_size, out, out_size)) return fail(WG_EINVAL, "the output buffer must not overlap the input buffer");
  DeviceGuard g(c->device);
  return x25519_launch(desc, n, in, in_size, out, out_size, status, pick_stream(c, stream));
}

int wg_hs_static_set(wg_ctx* c, const uint8_t* static_private, uint8_t* static_public_out) {
  if (!c || !static_private) return fail(WG_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  HsState* t;
  int rc;
  if ((rc = hs_get(c, &t)) != WG_OK) return rc;
  // stage: [128, 160) the descriptor (BASE, scalar at 0 of the key buffer), [160, 192) the public key, [192, 196) status
  wg_x25519_desc d{};
  d.flags = WG_X25519_BASE;
  HIPTRY(hipDeviceSynchronize());  // no DH queued earlier (on any stream) may still read the old key
  uint8_t* st = (uint8_t*)t->d_stage.p;
  HIPTRY(hipMemcpyAsync(t->d_priv.p, static_private, 32, hipMemcpyHostToDevice, c->stream));
  HIPTRY(hipMemcpyAsync(st + 128, &d, sizeof d, hipMemcpyHostToDevice, c->stream));
  if ((rc = x25519_launch((const wg_x25519_desc*)(st + 128), 1, (const uint8_t*)t->d_priv.p, 32, st + 160, 32,
                          (uint32_t*)(st + 192), c->stream)) != WG_OK)
    return rc;
  uint8_t pub[32];
  HIPTRY(hipMemcpyAsync(pub, st + 160, 32, hipMemcpyDeviceToHost, c->stream));
  HIPTRY(hipStreamSynchronize(c->stream));
  t->has_priv = true;
  if ((rc = hs_mac1_key_set(c, t, pub)) != WG_OK) return rc;  // as wg_hs_key_set(public)
  if ((rc = hs_open_rekey(c, t, pub)) != WG_OK) return rc;    // H(H0 || public), the stored peers' secrets
  if (static_public_out) memcpy(static_public_out, pub, 32);
  return WG_OK;
}

int wg_hs_dh(wg_ctx* c, const wg_hs_dh_batch* b, void* stream) {
  if (!c || !b) return fail(WG_EINVAL, "NULL argument");
  if (b->_reserved) return fail(WG_EINVAL, "wg_hs_dh_batch._reserved must be 0");
  if (((uintptr_t)b->n_records) & 3u) return fail(WG_EINVAL, "n_records must be 4-byte aligned");
  hipStream_t s = pick_stream(c, stream);
  const uint8_t* key;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->hs || !c->hs->has_priv) return fail(WG_ENOKEY, "wg_hs_dh before any wg_hs_static_set");
    key = (const uint8_t*)c->hs->d_priv.p;
  }
  if (b->n == 0) return WG_OK;
  if (!b->records || (((uintptr_t)b->records) & 15u) || !b->shared || (((uintptr_t)b->shared) & 15u) || !b->dh_status ||
      (((uintptr_t)b->dh_status) & 3u))
    return fail(WG_EINVAL, "records / shared / dh_status must be non-NULL and aligned (16 / 16 / 4 bytes)");
  DeviceGuard g(c->device);
  wgx::DhParams P{};
  P.records = b->records;
  P.n_records = b->n_records;
  P.shared = b->shared;
  P.dh_status = b->dh_status;
  P.key = key;
  P.n = b->n;
  hipLaunchKernelGGL(wgx::k_hs_dh, dim3((b->n + 63u) / 64u), dim3(64), 0, s, P);
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) return fail(WG_EDEVICE, "k_hs_dh launch: %s", hipGetErrorString(le));
  return WG_OK;
}

}  // extern "C"
