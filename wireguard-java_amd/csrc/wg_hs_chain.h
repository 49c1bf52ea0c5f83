// wg_hs_chain.h — the Noise chains of the handshake as data: the step record, its enums, the builders and the
// programs of k_hs_open (wg_hs_open.hip), k_hs_resp_chain (wg_hs_respond.hip), the initiator's k_hs_init_chain
// and k_hs_fin_chain (wg_hs_initiate.hip) and k_hs_stamp_chain (wg_hs_stamp.hip). Included by wg_hs_chain.hip, which holds the machine that runs them. A
// host compiler reads this file too: tests/test_hs_chain.py and tests/test_hs_initiate.py print the programs and
// run them through a Python interpreter of the operations against the models, so a wrong table fails without a
// GPU.
//
// A step is one BLAKE2s compression: `op` says what is hashed, `arg` names the 32 bytes it takes (SRC_*), `imm`
// is the operation's small constant, `dst` says where the eight state words go afterwards. The programs are
// public constants and are indexed by a public counter.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define WG_HSC_DEVICE __device__
#else
#define WG_HSC_DEVICE
#endif

namespace wghc {

struct alignas(4) Step {
  uint8_t op, arg, imm, dst;
};

enum Op : uint8_t {
  // the generic operations (wghc::prepare)
  OP_PAD,   // an HMAC key block of arg: arg ^ ipad, or arg ^ opad (imm & PAD_OPAD); the LAST block with imm & PAD_LAST
  OP_IN32,  // the 32 bytes arg behind the inner key-block state (ist), t = 96
  OP_OUT,   // the outer hash: the digest in st behind the outer key-block state (ost)
  OP_T1,    // the inner hash of HMAC(PRK, 0x01)
  OP_TN,    // the inner hash of HMAC(PRK, T_{n-1} || n): T_{n-1} = arg, n = imm
  OP_H2,    // H(h || arg)
  // k_hs_open's own
  OP_H0,    // H(H(H0 || S_pub) || E)
  OP_ES1,   // the AEAD open of encrypted_static under st, the probe; H(h || encrypted_static), first block
  OP_ES2,   // ... its second block: the tag
  OP_TS,    // H(h || encrypted_timestamp)
  // k_hs_resp_chain's own
  OP_MAC1KEY,  // H("mac1----" || S_i)
  OP_MAC1A,    // BLAKE2s-128 under that key (in ist): the key block
  OP_MAC1B,    // ... and response[0 .. 60)
  // k_hs_init_chain's own (it has its own OP_MAC1KEY and OP_MAC1A too: the key is the peer's)
  OP_IH0,     // H(H0 || S_r)
  OP_IES1,    // the AEAD seal of S_pub under st; H(h || encrypted_static), first block
  OP_IES2,    // ... its second block: the tag
  OP_ITS,     // the AEAD seal of the timestamp under st; H(h || encrypted_timestamp)
  OP_IMAC1B,  // mac1's message, initiation[0 .. 64)
  OP_IMAC1C,  // ... and initiation[64 .. 116)
  // k_hs_stamp_chain's own (wg_hs_stamp.hip; it has its own OP_H0 and OP_ES2 too, over the same bytes)
  OP_SES1,  // H(h || encrypted_static), first block, and nothing else: encrypted_static was opened by k_hs_open
  OP_STS,   // the AEAD open of encrypted_timestamp under st (OP_ITS's mirror); H(h || encrypted_timestamp)
};

enum Src : uint8_t {
  SRC_ZERO,  // 32 zero bytes (the psk); also what a step that takes no bytes names
  SRC_CK,
  SRC_X,
  // k_hs_open's
  SRC_E,       // the record's ephemeral
  SRC_SS,      // wg_hs_dh's shared secret
  SRC_STATIC,  // the peer's static-static secret (zeros for a lane without a peer)
  // k_hs_resp_chain's: the three ladder results
  SRC_EPUB,
  SRC_EE,
  SRC_ES,  // (k_hs_init_chain: e S_r; k_hs_fin_chain: S E_r)
  // k_hs_fin_chain's: the response's ephemeral and the peer's preshared key (its ladder results are SRC_EE, SRC_ES)
  SRC_ER,
  SRC_PSK,
};

enum Imm : uint8_t {
  PAD_IPAD = 0,
  PAD_OPAD = 1,
  PAD_LAST = 2,   // the key block is the whole message: KDF(ck, "")
  PAD_SEAL = 128, // k_hs_resp_chain: seal_empty(x, h) before this step, while x still holds k (k_hs_fin_chain: the
                  // same tag, compared with the response's)
};

enum Dst : uint8_t {
  DST_NONE,  // stays in st
  DST_H,
  DST_X,
  DST_CK,
  DST_IST,
  DST_OST,
  DST_CK_IF_PEER,  // k_hs_open: ck, in the lanes that have a peer
};

// HMAC(ck, src) -> x: the extract. Four steps.
#define WG_HSC_EXTRACT(src) \
  {OP_PAD, SRC_CK, PAD_IPAD, DST_IST}, {OP_PAD, SRC_CK, PAD_OPAD, DST_OST}, {OP_IN32, src, 0, DST_NONE}, {OP_OUT, SRC_ZERO, 0, DST_X}
// T1 = HMAC(x, 0x01) -> dst; leaves the key-block states of x for EXPANDN. Four steps.
#define WG_HSC_EXPAND1(dst) \
  {OP_PAD, SRC_X, PAD_IPAD, DST_IST}, {OP_PAD, SRC_X, PAD_OPAD, DST_OST}, {OP_T1, SRC_ZERO, 0, DST_NONE}, {OP_OUT, SRC_ZERO, 0, dst}
// Tn = HMAC(PRK, prev || n) -> dst, with the key-block states EXPAND1 left. Two steps.
#define WG_HSC_EXPANDN(prev, n, dst) {OP_TN, prev, n, DST_NONE}, {OP_OUT, SRC_ZERO, 0, dst}

// k_hs_open. h = H(H(H0 || S_pub) || E); ck = KDF1(CK0, E), from the constant key-block states of CK0;
// k = KDF2(ck, ss) (left in st for the AEAD) and ck = KDF1(ck, ss); h = H(h || encrypted_static);
// known peer: ck = KDF1(ck, static-static); h = H(h || encrypted_timestamp).
WG_HSC_DEVICE constexpr Step kOpenProgram[] = {
    {OP_H0, SRC_ZERO, 0, DST_H},
    {OP_IN32, SRC_E, 0, DST_NONE}, {OP_OUT, SRC_ZERO, 0, DST_X}, WG_HSC_EXPAND1(DST_CK),
    WG_HSC_EXTRACT(SRC_SS), WG_HSC_EXPAND1(DST_CK), WG_HSC_EXPANDN(SRC_CK, 2, DST_NONE),
    {OP_ES1, SRC_ZERO, 0, DST_NONE}, {OP_ES2, SRC_ZERO, 0, DST_H},
    WG_HSC_EXTRACT(SRC_STATIC), WG_HSC_EXPAND1(DST_CK_IF_PEER),
    {OP_TS, SRC_ZERO, 0, DST_H},
};

// k_hs_resp_chain. h = H(h || Epub); ck = KDF1(ck, Epub); ck = KDF1(ck, e E_i); ck = KDF1(ck, e S_i);
// ck, tau, k = KDF3(ck, psk) with tau and then k in x; h = H(h || tau); the seal of nothing under k;
// recv_key, send_key = KDF2(ck, "") in ck and x; mac1 (its key through ist).
WG_HSC_DEVICE constexpr Step kRespProgram[] = {
    {OP_H2, SRC_EPUB, 0, DST_H},
    WG_HSC_EXTRACT(SRC_EPUB), WG_HSC_EXPAND1(DST_CK),
    WG_HSC_EXTRACT(SRC_EE), WG_HSC_EXPAND1(DST_CK),
    WG_HSC_EXTRACT(SRC_ES), WG_HSC_EXPAND1(DST_CK),
    WG_HSC_EXTRACT(SRC_ZERO), WG_HSC_EXPAND1(DST_CK), WG_HSC_EXPANDN(SRC_CK, 2, DST_X),
    {OP_H2, SRC_X, 0, DST_H},
    WG_HSC_EXPANDN(SRC_X, 3, DST_X),
    {OP_PAD, SRC_CK, PAD_OPAD | PAD_SEAL, DST_OST}, {OP_PAD, SRC_CK, PAD_IPAD | PAD_LAST, DST_NONE}, {OP_OUT, SRC_ZERO, 0, DST_X},
    WG_HSC_EXPAND1(DST_CK),
    WG_HSC_EXPANDN(SRC_CK, 2, DST_X),
    {OP_MAC1KEY, SRC_ZERO, 0, DST_IST}, {OP_MAC1A, SRC_ZERO, 0, DST_NONE}, {OP_MAC1B, SRC_ZERO, 0, DST_NONE},
};

// k_hs_init_chain. h = H(H(H0 || S_r) || Epub); ck = KDF1(CK0, Epub), from the constant key-block states of CK0;
// k = KDF2(ck, e S_r) (left in st for the seal of S_pub) and ck = KDF1; h = H(h || encrypted_static); k = KDF2(ck,
// static-static) (in st for the seal of the timestamp) and ck = KDF1; h = H(h || encrypted_timestamp); mac1 under
// the peer's key over the 116 bytes.
WG_HSC_DEVICE constexpr Step kInitProgram[] = {
    {OP_IH0, SRC_ZERO, 0, DST_H}, {OP_H2, SRC_EPUB, 0, DST_H},
    {OP_IN32, SRC_EPUB, 0, DST_NONE}, {OP_OUT, SRC_ZERO, 0, DST_X}, WG_HSC_EXPAND1(DST_CK),
    WG_HSC_EXTRACT(SRC_ES), WG_HSC_EXPAND1(DST_CK), WG_HSC_EXPANDN(SRC_CK, 2, DST_NONE),
    {OP_IES1, SRC_ZERO, 0, DST_NONE}, {OP_IES2, SRC_ZERO, 0, DST_H},
    WG_HSC_EXTRACT(SRC_STATIC), WG_HSC_EXPAND1(DST_CK), WG_HSC_EXPANDN(SRC_CK, 2, DST_NONE),
    {OP_ITS, SRC_ZERO, 0, DST_H},
    {OP_MAC1KEY, SRC_ZERO, 0, DST_IST}, {OP_MAC1A, SRC_ZERO, 0, DST_NONE}, {OP_IMAC1B, SRC_ZERO, 0, DST_NONE},
    {OP_IMAC1C, SRC_ZERO, 0, DST_NONE},
};

// k_hs_fin_chain: kRespProgram without mac1, over the initiator's operands. h = H(h || E_r); ck = KDF1(ck, E_r);
// ck = KDF1(ck, e E_r); ck = KDF1(ck, S E_r); ck, tau, k = KDF3(ck, psk); h = H(h || tau); the tag of nothing
// under k, which the kernel compares; send_key, recv_key = KDF2(ck, "") in ck and x.
WG_HSC_DEVICE constexpr Step kFinProgram[] = {
    {OP_H2, SRC_ER, 0, DST_H},
    WG_HSC_EXTRACT(SRC_ER), WG_HSC_EXPAND1(DST_CK),
    WG_HSC_EXTRACT(SRC_EE), WG_HSC_EXPAND1(DST_CK),
    WG_HSC_EXTRACT(SRC_ES), WG_HSC_EXPAND1(DST_CK),
    WG_HSC_EXTRACT(SRC_PSK), WG_HSC_EXPAND1(DST_CK), WG_HSC_EXPANDN(SRC_CK, 2, DST_X),
    {OP_H2, SRC_X, 0, DST_H},
    WG_HSC_EXPANDN(SRC_X, 3, DST_X),
    {OP_PAD, SRC_CK, PAD_OPAD | PAD_SEAL, DST_OST}, {OP_PAD, SRC_CK, PAD_IPAD | PAD_LAST, DST_NONE}, {OP_OUT, SRC_ZERO, 0, DST_X},
    WG_HSC_EXPAND1(DST_CK),
    WG_HSC_EXPANDN(SRC_CK, 2, DST_X),
};

// k_hs_stamp_chain: k_hs_open's chain again up to the timestamp's key, which wg_hs_init does not carry.
// h = H(H(H0 || S_pub) || E); ck = KDF1(CK0, E); ck = KDF1(ck, ss) (no k: encrypted_static is not opened a second
// time); h = H(h || encrypted_static); k = KDF2(ck, static-static) (left in st for the open of the timestamp)
// and ck = KDF1; h = H(h || encrypted_timestamp), which ends at wg_hs_init's hash.
WG_HSC_DEVICE constexpr Step kStampProgram[] = {
    {OP_H0, SRC_ZERO, 0, DST_H},
    {OP_IN32, SRC_E, 0, DST_NONE}, {OP_OUT, SRC_ZERO, 0, DST_X}, WG_HSC_EXPAND1(DST_CK),
    WG_HSC_EXTRACT(SRC_SS), WG_HSC_EXPAND1(DST_CK),
    {OP_SES1, SRC_ZERO, 0, DST_NONE}, {OP_ES2, SRC_ZERO, 0, DST_H},
    WG_HSC_EXTRACT(SRC_STATIC), WG_HSC_EXPAND1(DST_CK), WG_HSC_EXPANDN(SRC_CK, 2, DST_NONE),
    {OP_STS, SRC_ZERO, 0, DST_H},
};

constexpr uint32_t kOpenSteps = sizeof(kOpenProgram) / sizeof(Step);
constexpr uint32_t kRespSteps = sizeof(kRespProgram) / sizeof(Step);
static_assert(sizeof(Step) == 4, "a step is one 32-bit word");
static_assert(kOpenSteps == 28, "k_hs_open: 28 compressions");
static_assert(kRespSteps == 50, "k_hs_resp_chain: 50 compressions");
constexpr uint32_t kInitSteps = sizeof(kInitProgram) / sizeof(Step);
constexpr uint32_t kFinSteps = sizeof(kFinProgram) / sizeof(Step);
static_assert(kInitSteps == 35, "k_hs_init_chain: 35 compressions");
static_assert(kFinSteps == 47, "k_hs_fin_chain: 47 compressions");
constexpr uint32_t kStampSteps = sizeof(kStampProgram) / sizeof(Step);
static_assert(kStampSteps == 28, "k_hs_stamp_chain: 28 compressions");

// the first step of `op` in a program
template <uint32_t N>
constexpr uint32_t step_of(const Step (&prog)[N], Op op) {
  for (uint32_t k = 0; k < N; ++k)
    if (prog[k].op == op) return k;
  return N;
}
// k_hs_open's static-static KDF: the steps between H(h || encrypted_static) and H(h || encrypted_timestamp),
// which a wave without a known peer jumps over
constexpr uint32_t kOpenStaticBegin = step_of(kOpenProgram, OP_ES2) + 1u;
constexpr uint32_t kOpenStaticEnd = step_of(kOpenProgram, OP_TS);
static_assert(kOpenStaticEnd - kOpenStaticBegin == 8, "an extract and an expand");
static_assert(kOpenProgram[kOpenStaticEnd - 1].dst == DST_CK_IF_PEER, "the KDF's result is the one conditional store");

}  // namespace wghc
