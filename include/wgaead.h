/*
 * wgaead.h — C-ABI of libwgaead.so, the MI355X (gfx950) transport-data AEAD.
 *
 * This is the drop-in boundary for the reference's ChaCha20-Poly1305 path in
 * module ax.xz.wireguard.noise. Every entry point below names the reference
 * interface it replaces (file:line, paths relative to the reference root,
 * abbreviated: NOISE = ax.xz.wireguard.noise/src/main/java/ax/xz/wireguard/noise).
 * The Java host binds these through Panama exactly as the reference binds
 * libchacha / libpoly1305-donna today (NOISE/crypto/ChaCha20.java:14-42,
 * NOISE/crypto/Poly1305.java:24-77); see INTEGRATION.md.
 *
 * Conventions
 *  - Plain C types only; no exceptions cross the ABI.
 *  - Every function returns 0 (WG_OK) or a negative WG_E* code. A per-packet
 *    authentication failure is NOT an error return: it is reported in the
 *    status array (WG_PKT_BADTAG), mirroring the per-packet
 *    AEADBadTagException of NOISE/crypto/ChaCha20Poly1305.java:51-53.
 *  - "batch" calls take DEVICE pointers and are asynchronous on `stream`
 *    (a hipStream_t passed as void*, used as-is: NULL is HIP's default stream;
 *    wg_ctx_stream(ctx) returns the context's own non-blocking stream).
 *    The "host" calls take host pointers and return after completion.
 *  - Packets are independent (no cross-packet state): a batch shards freely
 *    across devices; no collective is involved (one wg_ctx per device).
 *  - Nonce layout of transport packets is the reference's, not the WireGuard
 *    spec's: nonce = LE64(counter) || 00 00 00 00 (NOISE/handshake/SymmetricKeypair.java:52-61).
 */
#ifndef WGAEAD_H
#define WGAEAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WG_OK 0
#define WG_EINVAL (-22)    /* bad argument (NULL, n mismatch, unaligned key slot, ...) */
#define WG_ENOMEM (-12)    /* device or pinned allocation failed */
#define WG_ERANGE (-34)    /* key slot / buffer bound exceeded by a descriptor */
#define WG_E2BIG (-7)      /* packet longer than WG_MAX_PACKET */
#define WG_EDEVICE (-5)    /* HIP runtime error (message via wg_last_error) */
#define WG_ESELFTEST (-74) /* known-answer self test failed */
#define WG_EAGAIN (-11)    /* wg_submit_*: no free queue slot within the queue's submit timeout */
/* wg_seal1 / wg_open1 / wg_submit_*: the key slot holds no key (never set, or zeroed by wg_keys_zero).
 * SymmetricKeypair.clean() closes its key arena, so a later cipher() / decipher() throws instead of
 * encrypting (SymmetricKeypair.java:85-93); these paths refuse the packet the same way rather than
 * sealing it under the publicly known all-zero key. */
#define WG_ENOKEY (-126)

#define WG_PKT_OK 0u
#define WG_PKT_BADTAG 1u
/* (2 = WG_PKT_BADHDR, the parse status of wg_parse_open) */
/* written by wg_rx_check (receive-side checks after open; only WG_PKT_OK packets are examined) */
#define WG_PKT_KEEPALIVE 3u /* zero-length plaintext: a keepalive, not forwarded */
#define WG_PKT_BADIP 4u     /* IP version nibble not 4 or 6, or too short for the destination address */
#define WG_PKT_FILTERED 5u  /* destination outside the key slot's AllowedIPs filter */
#define WG_PKT_REPLAY 6u    /* counter replayed, too old for the window, or >= 2^64 - 2^13 - 1 */
/* a queued packet whose key slot was zeroed between its submit's check and its copy into the ring:
 * never sealed or opened (its output is untouched) */
#define WG_PKT_NOKEY 7u
/* a queued packet (wg_submit_*) whose batch could not run (launch or stream error) */
#define WG_PKT_FAILED 255u

#define WG_TAG_SIZE 16   /* Crypto.ChaChaPoly1305Overhead (NOISE/crypto/Crypto.java:14) */
#define WG_NONCE_SIZE 12 /* Crypto.ChaChaPoly1305NonceSize (NOISE/crypto/Crypto.java:13) */
#define WG_KEY_SIZE 32
#define WG_MAX_PACKET 65535u /* largest payload one workgroup tile accepts */

/* Transport packet descriptor (32 bytes). One per packet of a batch.
 *  seal: reads  in[in_off .. in_off+len)            plaintext
 *        writes out[out_off .. out_off+len+16)     ciphertext || tag
 *        (SymmetricKeypair.cipher: dst = ct || tag, SymmetricKeypair.java:63-74)
 *  open: reads  in[in_off .. in_off+len+16)         ciphertext || tag
 *        writes out[out_off .. out_off+len)         plaintext, only if the tag verifies;
 *        on a bad tag the plaintext range is zero-filled and status = WG_PKT_BADTAG;
 *        when the plaintext range overlaps in[in_off .. in_off+len+16) (in place, or moved back),
 *        the tag is verified before any byte is written and a forged packet's bytes stay as they
 *        were (ChaCha20Poly1305.java:40-56); an overlap that moves the plaintext forward is undefined
 *        (SymmetricKeypair.decipher: L = src.size - 16, SymmetricKeypair.java:76-83)
 *  counter: the 64-bit transport counter (TransportPacket.java:53-55); nonce built on device.
 *  key_slot: index into the context's device key table (wg_keys_set). */
typedef struct wg_pkt {
  uint64_t in_off;
  uint64_t out_off;
  uint64_t counter;
  uint32_t len;
  uint32_t key_slot;
} wg_pkt;

/* General AEAD / primitive descriptor (64 bytes) for the reference's static
 * crypto API (ChaCha20Poly1305, ChaCha20, Poly1305 classes): explicit 12-byte
 * nonce words, optional AAD, explicit initial block counter. */
typedef struct wg_aead_desc {
  uint64_t in_off;
  uint64_t out_off;
  uint64_t aad_off;   /* into the aad buffer (AEAD modes only) */
  uint32_t len;       /* payload bytes (excl. tag) */
  uint32_t aad_len;   /* 0 = no AAD (poly1305AeadEncrypt(key, nonce, ...) overloads) */
  uint32_t key_slot;  /* ChaCha key (AEAD, CIPHER) or 32-byte one-time key (MAC) */
  uint32_t ctr0;      /* CIPHER mode: initial 32-bit block counter (ChaCha20.chacha20(..., counter)) */
  uint32_t nonce[3];  /* state words 13..15, little-endian (ChaCha20.java:73) */
  uint32_t _reserved[3];
} wg_aead_desc;

typedef struct wg_ctx wg_ctx;

/* ---- library / context -------------------------------------------------- */

/* Known-answer self test on the device (RFC 8439 2.3.2/2.4.2/2.5.2/2.6.2/2.8.2
 * and the donna vectors). Returns 1 if all pass, like poly1305_power_on_self_test
 * which Poly1305.<clinit> checks (Poly1305.java:62-76). Creates and destroys a
 * temporary context on `device`. */
int wg_aead_selftest(int device);

/* Create a context bound to HIP device `device` with a key table of
 * `key_slots` 32-byte entries (zero-initialised).
 * Scheduling overrides read here from the environment, for A/B measurements only (none changes
 * a byte of output): WG_SLOT16=0|1, WG_SLOT4=0|1|2, WG_SLOT2=k, WG_MIXED_SPLIT=R, WG_UNIFORM16=k,
 * WG_PRIO=0|1, WG_LPT_ONE=0|1, WG_STREAM_WS=0|1, WG_UNI=0|1 (0: the WG_F_UNIFORM plan's 8-lane launches
 * without the uniform-wave body); unset, the transport kernel plans
 * every batch from its size and the WG_F_UNIFORM hint. Each selects a kernel the product path also takes
 * for some batch; the variants that lost their A/B are not in the library (docs/EXPERIMENTS.md). */
int wg_ctx_create(int device, uint32_t key_slots, wg_ctx** out);
int wg_ctx_destroy(wg_ctx* ctx); /* zeroes the key table first */
int wg_ctx_device(const wg_ctx* ctx);
uint32_t wg_ctx_key_slots(const wg_ctx* ctx);
void* wg_ctx_stream(wg_ctx* ctx);       /* the context's hipStream_t */
int wg_sync(wg_ctx* ctx, void* stream); /* hipStreamSynchronize */
const char* wg_last_error(void);        /* thread-local text for the last error */
const char* wg_version(void);

/* NUMA node of HIP device `device`'s PCI function (sysfs), or -1 if unknown. A queue's dispatcher
 * thread runs on that node's CPUs (wg_queue_create); callers feeding the GPU from many threads
 * should place them there too (TransportManager's pools: numactl --cpunodebind, or a thread
 * factory that sets the affinity). */
int wg_device_numa_node(int device);

/* Transport kernel used by this context's wg_seal_batch / wg_open_batch / *_host calls
 * (a test and A/B hook beside the reference interface). name: "default"
 * or NULL or "transport" (k_transport, the product kernel), "wave1" (the round-1
 * k_wave kernel, kept as the performance baseline) or "tile" (k_tile, the general
 * AEAD kernel run on transport descriptors). lanes is ignored (kept for ABI stability).
 * variant (transport kernel only): 0 = a WG_F_AFTER_SEAL step is ONE k_step launch (each wave
 * seals its packets, then opens them); 1 = the same step as two launches, seal then open.
 * Every kernel and variant computes identical bytes; they differ only in speed. */
int wg_ctx_set_kernel(wg_ctx* ctx, const char* name, uint32_t lanes, uint32_t variant);

/* ---- keys: SymmetricKeypair(byte[] send, byte[] recv) and clean() ---------
 * (SymmetricKeypair.java:39-50 copies keys into a shared Arena; :85-93 zeroes them) */
int wg_keys_set(wg_ctx* ctx, uint32_t first_slot, uint32_t n, const uint8_t* keys_host /* n*32 */);
int wg_keys_zero(wg_ctx* ctx, uint32_t first_slot, uint32_t n);

/* ---- batched transport seal / open (device pointers) ----------------------
 * Replaces the per-packet ForkJoinPool fan-out of SymmetricKeypair.cipher /
 * decipher (TransportManager.java:41,70-93,137-158). `in_size` / `out_size`
 * are the byte sizes of the buffers; every descriptor is bounds-checked on
 * device against them (an out-of-range packet is skipped with status
 * WG_PKT_BADTAG on open / untouched output on seal, and the call returns 0).
 * `max_len`: every packet's len must be <= max_len (longer ones are treated
 * as out of range). Flags: WG_F_UNIFORM declares the lengths (nearly) equal: the
 * packets are taken in order; without it a mixed-length batch is first ordered
 * longest-first on the device, so every slot of the kernel gets a similar share of
 * rounds. Unknown flag bits are rejected (WG_EINVAL); wg_open_batch takes only
 * WG_F_UNIFORM and needs a status array when n > 0. Calls with mixed-length batches
 * on one context use a shared plan workspace: calls on different streams are ordered
 * by the library (the later one waits for the earlier one's plan). */
#define WG_F_UNIFORM 1u
/* WG_F_FRAME (wg_seal_batch only): also write the 16-B transport header at
 * out_off - 16 of every packet, exactly as wg_frame_seal does, from the receiver
 * table given to wg_ctx_set_receivers (k_frame_seal launched after the seal kernel
 * on the same stream). */
#define WG_F_FRAME 2u
/* WG_F_RX_FILTER (wg_open_batch only): the open kernel also runs wg_rx_check's WG_RX_FILTER
 * checks (keepalive, IP version, AllowedIPs of the key slot) on every packet whose tag verified
 * and writes the refined status itself, in the same launch; the replay window
 * stays a wg_rx_check call. */
#define WG_F_RX_FILTER 8u
/* Device array of receiver_index per key slot (n >= key_slots entries, device memory
 * of this context's device, 4-byte aligned, caller-owned, must outlive the seals that
 * use it); NULL clears it. */
int wg_ctx_set_receivers(wg_ctx* ctx, const uint32_t* receivers_dev, uint32_t n);
int wg_seal_batch(wg_ctx* ctx, const wg_pkt* desc_dev, uint32_t n, const uint8_t* in_dev, uint64_t in_size,
                  uint8_t* out_dev, uint64_t out_size, uint32_t max_len, uint32_t flags, void* stream);
int wg_open_batch(wg_ctx* ctx, const wg_pkt* desc_dev, uint32_t n, const uint8_t* in_dev, uint64_t in_size,
                  uint8_t* out_dev, uint64_t out_size, uint32_t* status_dev, uint32_t max_len, uint32_t flags,
                  void* stream);

/* ---- both directions in one launch (device pointers) ----------------------
 * A node seals its outgoing batch and opens its incoming batch at the same time: the
 * reference runs both on one ForkJoinPool (TransportManager.java:41 outgoing cipher,
 * :79 incoming decipher). wg_duplex_batch(seal, open) computes exactly what
 * wg_seal_batch(seal...) and wg_open_batch(open...) compute, in ONE kernel launch whose
 * workgroups alternate between the two batches, so neither batch's launch start and tail
 * leaves the device idle. The two batches run concurrently: the open batch must not read
 * bytes the seal batch writes in the same call (open the previous call's ciphertext).
 * seal->flags: WG_F_UNIFORM, WG_F_FRAME (as wg_seal_batch); seal->status is ignored.
 * open->flags: WG_F_UNIFORM, WG_F_AFTER_SEAL; open->status is required when open->n > 0.
 * Either n may be 0.
 * WG_F_AFTER_SEAL (open->flags): the open batch DOES read what the seal batch writes: open packet i
 *   is ordered after seal packet i, and after no other seal packet, so it may read what seal packet
 *   i writes but not what another seal packet of the call writes (same n in both batches; e.g. two
 *   peers in loopback, or a verify pass over what was just sealed). With the transport kernel and
 *   equal max_len / WG_F_UNIFORM on both sides (and no WG_F_FRAME) the step is ONE k_step launch in
 *   which every wave seals its packets and then opens the same batch positions; otherwise the seal
 *   launch and then the open launch run on `stream`. A mixed-length batch is ordered longest-first
 *   once, for both (its packets have the same lengths). Such a step on a mixed batch of max_len <= 2048
 *   plans in a workspace of its stream's own (up to 8 streams; WG_STREAM_WS=0: the shared one), so steps
 *   on different streams do not wait for each other. */
#define WG_F_AFTER_SEAL 4u
typedef struct wg_batch {
  const wg_pkt* desc; /* device, 16-byte aligned */
  const uint8_t* in;
  uint8_t* out;
  uint32_t* status;   /* open: WG_PKT_* per packet */
  uint64_t in_size;
  uint64_t out_size;
  uint32_t n;
  uint32_t max_len;
  uint32_t flags;
  uint32_t _reserved;
} wg_batch;
int wg_duplex_batch(wg_ctx* ctx, const wg_batch* seal, const wg_batch* open, void* stream);

/* ---- general AEAD + primitives (device pointers) --------------------------
 * WG_MODE_SEAL / WG_MODE_OPEN: ChaCha20Poly1305.poly1305AeadEncrypt / Decrypt
 *   with optional AAD and explicit nonce (ChaCha20Poly1305.java:31-60).
 * WG_MODE_CIPHER: ChaCha20.chacha20(key, nonce, in, out, counter) (ChaCha20.java:116-131)
 *   = libchacha chacha_cipher with state word 12 = ctr0 (chacha-generic.c:104-108).
 * WG_MODE_MAC: Poly1305 init/update/finish one-shot with a 32-byte one-time key
 *   (Poly1305.java:94-166 over poly1305-donna.c:26-69); tag at out[out_off]. */
#define WG_MODE_SEAL 0
#define WG_MODE_OPEN 1
#define WG_MODE_CIPHER 2
#define WG_MODE_MAC 3
int wg_aead_batch(wg_ctx* ctx, int mode, const wg_aead_desc* desc_dev, uint32_t n, const uint8_t* in_dev,
                  uint64_t in_size, const uint8_t* aad_dev, uint64_t aad_size, uint8_t* out_dev, uint64_t out_size,
                  uint32_t* status_dev, uint32_t max_len, void* stream);

/* ---- transport wire framing on device (device pointers) -------------------
 * Wire packet = 16-B header {u8 type=4, u8 zero[3], u32 receiver_index (LE),
 * u64 counter (LE)} followed by ct||tag (TransportPacket.java:18-35).
 * wg_frame_seal: for each desc[i] writes that header at out[desc[i].out_off - 16]
 *   with receiver_index = receivers_dev[desc[i].key_slot] and counter =
 *   desc[i].counter — UnencryptedOutgoingTransport.java:14-18 (type, receiver
 *   index) plus EncryptedOutgoingTransport.java:11-14 (counter). A header is
 *   written only for the packets the seal accepts (the same test: len <= max_len,
 *   key_slot < the context's key slots, in_off + len <= in_size, out_off + len + 16
 *   <= out_size) that also have out_off >= 16; every other packet is left untouched.
 *   Launch it on the same stream as wg_seal_batch, with the same in_size / max_len.
 * wg_parse_open: builds open descriptors from received wire packets without a
 *   host parse (UndecryptedIncomingTransport.java:20-33): wire packet i starts
 *   at wire_dev[pkt_off_dev[i]] and is pkt_len_dev[i] bytes long; desc_out[i] =
 *   {in_off = off + 16, out_off = off + pkt_len (plaintext right after the
 *   ciphertext in the same buffer, :30), counter = header counter, len =
 *   pkt_len - 32, key_slot = key_slot_dev[i]}. A packet whose type byte is not
 *   4, that is shorter than 32 bytes, or whose packet + plaintext overruns
 *   wire_size gets len = WG_LEN_INVALID (wg_open_batch then skips it with
 *   WG_PKT_BADTAG) and parse_status_dev[i] = WG_PKT_BADHDR (else WG_PKT_OK);
 *   parse_status_dev may be NULL. desc_out_dev must be 16-byte aligned. */
#define WG_PKT_BADHDR 2u
#define WG_LEN_INVALID 0xffffffffu
int wg_frame_seal(wg_ctx* ctx, const wg_pkt* desc_dev, uint32_t n, const uint32_t* receivers_dev, uint8_t* out_dev,
                  uint64_t out_size, uint64_t in_size, uint32_t max_len, void* stream);
int wg_parse_open(wg_ctx* ctx, const uint8_t* wire_dev, uint64_t wire_size, const uint64_t* pkt_off_dev,
                  const uint32_t* pkt_len_dev, const uint32_t* key_slot_dev, uint32_t n, wg_pkt* desc_out_dev,
                  uint32_t* parse_status_dev, void* stream);

/* ---- host-buffer entry points -----------------------------------------------
 * wg_seal1 / wg_open1 back the unchanged per-packet SymmetricKeypair API:
 *   cipher(src, dst): wg_seal1(ctx, send_slot, counter, src, L, dst) with dst of L+16 bytes
 *   decipher(counter, src, dst): wg_open1(ctx, recv_slot, counter, src, L, dst) with src of L+16 bytes
 *   returns WG_OK, or 1 for a bad tag (dst untouched, as NOISE/crypto/ChaCha20Poly1305.java:51-55).
 *   Thread-safe and synchronous per call (the per-packet ForkJoinPool fan-out of
 *   TransportManager.java:41,79,152-158), served without a kernel launch per packet: the
 *   packet (with its key, from a host mirror of the key table) goes into any free entry of a
 *   pinned 512-entry ring and is published by toggling the entry's doorbell bit; a persistent
 *   device kernel (k_pp, W waves, wave w owning entries [w 512/W, (w+1) 512/W)) polls the
 *   doorbells over PCIe, serves every published entry of its range in any order, and writes the
 *   result and a completion word back into pinned memory, on which the caller spins. A caller
 *   held up between claiming and publishing delays no other call. The kernel leaves the device
 *   as a whole after idle_us without work anywhere in it (and after at most 250 ms) and the next
 *   call relaunches it. A call that fails after publishing (a refused launch) leaves its entry to
 *   the next server, which completes it; the entry is then reused. Packets longer than 4080 bytes
 *   (past the reference pipeline's 4-KB buffers) take the host batch path.
 * wg_pp_config(ctx, waves, idle_us): waves of that kernel (a power of two, 1..64, default 16) and
 *   its idle timeout (µs, default 20000; 0 = default). Changing it stops a running server first.
 * wg_batcher_config(ctx, max_batch, window_us): the round-2 batcher's knobs; accepted and ignored
 *   (the persistent server has no batch size or window).
 * wg_batcher_stats: server launches and packets served by the per-packet path.
 * wg_seal_host / wg_open_host: a batch in host memory (tun ring in, UDP ring out).
 *   If `in` and `out` are pinned, device-mapped host memory (wg_host_alloc /
 *   wg_host_register) the kernel reads and writes them directly over PCIe
 *   (zero-copy); otherwise the batch moves through device mirrors in chunks with
 *   H2D, kernel and D2H overlapped on three streams. Only packet bytes are written
 *   to `out_host` (bytes between packets — wire headers, ring slack — are kept).
 *   On a bad tag the plaintext range is zero-filled and status[i] = WG_PKT_BADTAG.
 *   flags: WG_F_UNIFORM only. */
/* ---- receive side after open: keepalives, AllowedIPs, replay window -------
 * TransportManager.processDecryptedTransport (TransportManager.java:98-119) for a whole
 * opened batch, on the device: a packet whose status is WG_PKT_OK becomes
 *   WG_PKT_KEEPALIVE  if len == 0 (:103-105, not forwarded to the tun device);
 *   WG_PKT_BADIP      if its first nibble is not 4 or 6, or it is shorter than the
 *                     destination address's end (destinationIPOf, :124-130, throws);
 *   WG_PKT_FILTERED   if its key slot has an AllowedIPs filter (wg_slot_filters_set) and
 *                     the destination (bytes 16..19 of IPv4, 24..39 of IPv6) is not in it
 *                     (destinationFilter.search, :106-108; util/IPFilter.java:49-61);
 * and stays WG_PKT_OK otherwise (forwarded). Flags: WG_RX_FILTER runs those checks;
 * WG_RX_REPLAY first applies the key slot's replay window (wg_replay_enable), which the
 * reference does not have: a packet is WG_PKT_REPLAY if its counter is >= 2^64 - 2^13 - 1,
 * repeats an earlier WG_PKT_OK packet of the same key slot in this batch, is more than
 * window_bits behind the highest counter accepted before this batch, or was already
 * accepted; the window then advances past this batch's accepted counters (the window slides
 * between batches). Asynchronous on `stream`; run it after wg_open_batch on
 * the same stream. pt / pt_size: the open's output buffer (plaintexts at out_off). With
 * WG_RX_REPLAY a batch holds at most 2^30 packets; checks on different streams of one context
 * are ordered by the library (they share the window's scratch).
 *
 * wg_filter_set: AllowedIPs filter `filter_id` (< WG_MAX_FILTERS) from n prefixes, exactly as
 *   IPFilter.insert builds its trie (util/IPFilter.java:30-42), including its search rule:
 *   a prefix matches an address if the trie walk passes the prefix's node at a depth below
 *   the address width, so /32 (IPv4) and /128 (IPv6) entries never match - as in the
 *   reference, whose IPFilter.allowingAll() (0.0.0.0/32, ::/128) lets nothing through.
 *   Replaces any earlier filter with that id. A key slot without a filter passes every
 *   destination; a slot mapped to an id never set drops every destination (an empty
 *   IPFilter, :9-16).
 * wg_slot_filters_set: filter id per key slot for slots [first_slot, first_slot + n)
 *   (WG_NO_FILTER: none); the reference keeps one filter per peer (TransportManager.java:44,53).
 * wg_replay_enable: window of window_bits (a multiple of 64, <= 65536; 0 disables) per key
 *   slot, all windows empty. wg_keys_set / wg_keys_zero and wg_replay_reset empty the
 *   windows of the slots they touch (a new key is a new session).
 * wg_replay_state: a slot's window (top = highest accepted counter + 1, 0 if none; bits =
 *   window_bits / 64 words, bit (c mod window_bits) set for accepted counter c in the window). */
#define WG_MAX_FILTERS 65536u
#define WG_NO_FILTER 0xFFFFFFFFu
#define WG_RX_FILTER 1u
#define WG_RX_REPLAY 2u
typedef struct wg_prefix {
  uint8_t family;     /* 4 or 6 */
  uint8_t prefix_len; /* 0..32 or 0..128 */
  uint8_t addr[16];   /* network byte order; IPv4 in addr[0..3] */
} wg_prefix;
int wg_filter_set(wg_ctx* ctx, uint32_t filter_id, const wg_prefix* prefixes, uint32_t n);
int wg_slot_filters_set(wg_ctx* ctx, uint32_t first_slot, uint32_t n, const uint32_t* filter_ids_host);
int wg_replay_enable(wg_ctx* ctx, uint32_t window_bits);
int wg_replay_reset(wg_ctx* ctx, uint32_t first_slot, uint32_t n);
int wg_replay_state(wg_ctx* ctx, uint32_t slot, uint64_t* top, uint64_t* bits, uint32_t words);
int wg_rx_check(wg_ctx* ctx, const wg_pkt* desc_dev, uint32_t n, const uint8_t* pt_dev, uint64_t pt_size,
                uint32_t* status_dev, uint32_t flags, void* stream);

/* ---- transmit side before seal: peer selection, send counters, wire slots ----
 * The device counterpart of the reference's outbound path for a whole tun ring:
 * which peers get a tun packet (PeerList.broadcastPacketToPeers, PeerList.java:94-106, hands every
 * packet to every peer; TransportManager.sendOutgoingTransportNow, TransportManager.java:137-147,
 * drops it for a peer without a session), the send counter (SymmetricKeypair.cipher claims it with
 * SEND_COUNTER.getAndAdd(1), starting at 0 for a new keypair, SymmetricKeypair.java:37,:64;
 * EncryptedOutgoingTransport.java:11-14 writes it into the header) and where the wire packet goes
 * (UnencryptedOutgoingTransport.java:14-27: the header, then ct || tag at +16). wg_tx_plan writes the
 * wg_pkt descriptors that wg_seal_batch(..., WG_F_FRAME) takes, so a tun ring becomes a UDP ring
 * without per-packet host work, and the per-session send counters live where the nonces are built.
 * Never claim counters for one session both here and on the host (SymmetricKeypair.claimCounters).
 *
 * wg_tx_plan(ctx, b, stream): tun packet t is in[pkt_off[t] .. +pkt_len[t]); wire slot j is
 *   [wire_base + j * wire_stride, + wire_stride) of the seal's output buffer of out_size bytes.
 *   Packet t passes the size checks if pkt_len <= max_len, pkt_off + pkt_len <= in_size,
 *   pkt_len + 32 <= wire_stride and its last wire slot ends within out_size; otherwise its
 *   descriptors get WG_PKT_TOOLONG. pkt_len = 0 passes: a keepalive (KeepaliveSender.java:39).
 *   WG_TX_BROADCAST: n_desc = n * n_peers; descriptor j = t * n_peers + p is {in_off = pkt_off[t],
 *     out_off = wire_base + j * wire_stride + 16, len = pkt_len[t], key_slot = peers[p], counter =
 *     send[peers[p]] + r}, r = the number of packets before t in the batch that pass the size checks;
 *     tx_status[j] = WG_PKT_OK. Afterwards send[peers[p]] += the number of packets that passed.
 *   WG_TX_ROUTE: n_desc = n, j = t. A packet that passes the size checks is routed by its
 *     destination address, read as destinationIPOf reads it (TransportManager.java:124-130: version
 *     nibble 4: bytes 16..19, nibble 6: bytes 24..39): another nibble, or a packet that ends before
 *     the address does (a keepalive too), gets WG_PKT_BADIP; no prefix of wg_routes_set covering the
 *     address, WG_PKT_NOROUTE. A routed packet gets the key slot of the longest matching prefix,
 *     status WG_PKT_OK and counter = send[slot] + the number of routed packets to the same slot with
 *     a lower batch index; every slot then advances by its count, so counters stay dense per slot,
 *     a peer sees them in the order its packets were read, and two runs from one state give the same
 *     bytes.
 *   Every one of the n_desc descriptors and statuses is written. A descriptor whose status is not
 *   WG_PKT_OK has len = WG_LEN_INVALID (the seal and the framer skip it and leave its wire slot
 *   untouched), counter 0, in_off and out_off as above (modulo 2^64) and key_slot = peers[p]
 *   (broadcast) or 0 (route); it consumes no counter. Counters are 64-bit and wrap like a Java long.
 *   desc_out: 16-byte aligned. n_desc must stay below 2^31. n = 0, or no peers, writes nothing.
 *   Asynchronous on `stream`; run wg_seal_batch(desc_out, n_desc, ..., WG_F_FRAME) on the same stream.
 *   Plans on different streams of one context are ordered by the library (they share the counters
 *   and the scratch). Graphs: a plan may be captured (after wg_tx_reserve: a capturing stream cannot
 *   allocate, WG_EINVAL) and replayed any number of times; each replay continues the counters. The
 *   peer list, the route table header and the counters have fixed device addresses for the life of
 *   the context, so wg_routes_set, wg_tx_counters_set and a wg_tx_peers_set with the SAME number of
 *   peers need no re-capture (another number of peers changes n_desc: capture again). The library
 *   does not order a graph launch against eager plans on other streams: the caller does.
 * wg_tx_peers_set: the peers of broadcast mode as key slots, in PeerList iteration order; list only
 *   peers with a session. A slot >= the key table is WG_ERANGE, a repeated slot WG_EINVAL (it would
 *   use every nonce twice). Synchronous, like wg_keys_set.
 * wg_routes_set: replaces the whole cryptokey-routing table (n = 0 clears it): prefix k routes to
 *   key_slots_host[k]. Standard longest-prefix match: a prefix of length L matches an address whose
 *   first L bits equal it, so /0, /32 and /128 entries match; of equal prefixes the later entry
 *   wins. This is NOT IPFilter.search's rule (wg_filter_set), under which a full-length entry never
 *   matches: the reference has no outbound routing (it broadcasts), so there is nothing to be
 *   faithful to, and WireGuard's cryptokey routing is plain longest-prefix match. Synchronous.
 * wg_tx_counters_set / wg_tx_counters_get: the send counters of slots [first_slot, first_slot + n),
 *   ordered after every plan queued before the call (get waits for them). Counters are zero at
 *   creation; wg_keys_set / wg_keys_zero zero the counters of the slots they touch (a new
 *   SymmetricKeypair starts at 0), ordered after every plan queued before them.
 * wg_tx_reserve: scratch for plans of up to max_packets tun packets (either mode). A plan that needs
 *   more allocates it, except on a capturing stream. The counters and the scratch are allocated at
 *   the first wg_tx_* call: a context that never plans pays nothing. */
#define WG_PKT_NOROUTE 8u   /* route mode: no prefix covers the destination */
#define WG_PKT_TOOLONG 9u   /* len > max_len, packet overruns in_size, or its wire slot overruns stride / out_size */
#define WG_TX_BROADCAST 0u
#define WG_TX_ROUTE 1u
typedef struct wg_tx_batch {
  const uint8_t* in;       /* tun ring (device) */
  uint64_t in_size;
  const uint64_t* pkt_off; /* device, n entries */
  const uint32_t* pkt_len; /* device, n entries */
  wg_pkt* desc_out;        /* device, 16-byte aligned, n_desc entries */
  uint32_t* tx_status;     /* device, n_desc entries, WG_PKT_* */
  uint64_t wire_base;
  uint64_t wire_stride;
  uint64_t out_size;
  uint32_t n;
  uint32_t max_len;
  uint32_t mode;           /* WG_TX_BROADCAST or WG_TX_ROUTE */
  uint32_t _reserved;
} wg_tx_batch;
int wg_tx_peers_set(wg_ctx* ctx, const uint32_t* key_slots_host, uint32_t n);
int wg_routes_set(wg_ctx* ctx, const wg_prefix* prefixes, const uint32_t* key_slots_host, uint32_t n);
int wg_tx_counters_set(wg_ctx* ctx, uint32_t first_slot, uint32_t n, const uint64_t* counters_host);
int wg_tx_counters_get(wg_ctx* ctx, uint32_t first_slot, uint32_t n, uint64_t* counters_host);
int wg_tx_reserve(wg_ctx* ctx, uint32_t max_packets);
int wg_tx_plan(wg_ctx* ctx, const wg_tx_batch* batch, void* stream);

/* ---- receive side before and after open: sessions by index, tun delivery list ----
 * The device counterpart of the reference's inbound path around decipher, for a whole UDP ring, so that
 * a UDP ring becomes a plaintext ring and an ordered list of tun writes without per-packet host work:
 *  - the type byte that picks the packet class (PacketElement.java:107-113: 1 initiation, 2 response,
 *    4 transport, anything else throws);
 *  - the session of a transport packet's receiver index (PeerList.java:53-67 drops an unknown index at
 *    :61-65; TransportManager.java:70-77 drops a peer without a session at :73-77);
 *  - the open descriptor (UndecryptedIncomingTransport.java:20-33), as wg_parse_open builds it;
 *  - after the open, which packets go to the tun device and in which order
 *    (TransportManager.processDecryptedTransport, TransportManager.java:98-119, queues them one by one).
 *
 * wg_rx_sessions_set(ctx, indices, key_slots, n): replaces the whole receiver index -> key slot table
 *   (PeerList's index -> peer array, PeerList.java:53-67,:157-173, plus the peer's session,
 *   TransportManager.java:70-77); n = 0 clears it. Indices are arbitrary 32-bit values (the reference's
 *   small array indices and WireGuard's random ones, 0 and 0xFFFFFFFF included). A repeated index is
 *   WG_EINVAL, a key slot >= the key table WG_ERANGE; nothing changes on error. Synchronous, like
 *   wg_routes_set, and ordered after every receive plan queued before it. On the device the table is an
 *   open-addressing hash table built on the host: capacity = the smallest power of two >= max(16, 4 n),
 *   8-byte entries {index, key_slot + 1} (0: empty), bucket = fmix32(index) & (capacity - 1) with
 *   MurmurHash3's 32-bit finaliser, linear probing. Its header (entries, mask, count) keeps one device address for
 *   the life of the context, so a captured plan needs no re-capture after a table change. Without
 *   wg_rx_sessions_reserve there is no single-entry insert or remove, and rekeying one peer sends the table
 *   again; with it the device inserts and retires entries ("handshake sessions installed on the device" below).
 *
 * wg_rx_plan(ctx, b, stream): wire packet i is wire[o .. o + wl), o = pkt_off[i], wl = pkt_len[i]. The
 *   checks, in this order:
 *   1. wl == 0, o > wire_size or wl > wire_size - o: WG_PKT_BADHDR.
 *   2. t = wire[o]: 1 or 2 (InitiationPacket.TYPE, ResponsePacket.TYPE): WG_PKT_HANDSHAKE whatever its
 *      length (the host validates and handles it); any other t != 4: WG_PKT_BADHDR (PacketElement.java:112).
 *   3. t == 4 and wl < 32: WG_PKT_BADHDR; otherwise len = wl - 32 (only the type byte of the header is
 *      checked, UndecryptedIncomingTransport.java:24-26).
 *   4. the receiver index (LE32 at o + 4) is not in the session table: WG_PKT_NOSESSION.
 *   5. len > max_len: WG_PKT_TOOLONG.
 *   6. placement. WG_RX_PT_AFTER (the reference's layout, UndecryptedIncomingTransport.java:30): out_off
 *      = o + wl in the wire buffer; a plaintext that overruns wire_size is WG_PKT_BADHDR, as in
 *      wg_parse_open; pt_used = 0. WG_RX_PT_PACKED: out_off = pt_base + C_i, C_i = the sum of
 *      align16(len_j) over all j < i that passed steps 1-5; a packet with out_off + len > pt_size is
 *      WG_PKT_TOOLONG but still counts in C; pt_used = the final C. Every out_off is 16-byte aligned
 *      when pt_base is, and the plaintexts to copy back are the first min(pt_used, pt_size - pt_base)
 *      bytes at pt_base.
 *   A packet that passes has rx_status WG_PKT_OK and desc = {in_off = o + 16, out_off, counter = LE64
 *   at o + 8, len, key_slot}. Every other packet has len = WG_LEN_INVALID (wg_open_batch skips it with
 *   WG_PKT_BADTAG), counter = 0, in_off = o + 16 (modulo 2^64), out_off = o + wl (AFTER, modulo 2^64) or
 *   pt_base (PACKED), and key_slot = the session's slot if step 4 succeeded, else 0. All n descriptors
 *   and statuses are written. host_list[0 .. n_host) holds the batch indices of the WG_PKT_HANDSHAKE
 *   packets in ascending order; n_open counts the WG_PKT_OK ones. n = 0 writes only the summary (zeros).
 *   desc_out: 16-byte aligned; summary: 8-byte aligned. Asynchronous on `stream`; run wg_open_batch
 *   on desc_out on the same stream, with a status array of its own (wg_rx_deliver merges the two).
 *
 * wg_rx_deliver(ctx, b, stream): after wg_open_batch and wg_rx_check on the same stream. final_status[i]
 *   = plan_status[i] if that is not WG_PKT_OK, else open_status[i] (final_status may alias neither).
 *   items[0 .. n_items) is the stable compaction, in batch order, of the packets whose final status is
 *   WG_PKT_OK: {off = desc[i].out_off, len, key_slot}; index_out (may be NULL) holds their batch indices.
 *   delivered = {bytes = the sum of len over the items, n_items, n_keepalive = packets whose final
 *   status is WG_PKT_KEEPALIVE}. The host writes n_items packets to the tun device in arrival order and
 *   never looks at a status. items: 16-byte aligned; delivered: 8-byte aligned.
 *
 * Both calls rank over the whole batch without any wait between workgroups (a pass of per-workgroup
 * sums, one small scan, a pass that places); their scratch is written before it is read in every call
 * and nothing about a call lives on the host, so a captured plan or deliver replays any number of times.
 * Calls on different streams of one context are ordered by the library (they share the scratch); a
 * graph launch is the caller's to order. wg_rx_reserve(ctx, max_packets): scratch for batches of up to
 * max_packets; a call that needs more allocates it, except on a capturing stream (WG_EINVAL: reserve
 * first). The table and the scratch are allocated at the first of these four calls: a context that
 * never plans pays nothing. */
#define WG_PKT_NOSESSION 10u /* transport packet whose receiver index is not in the session table */
#define WG_PKT_HANDSHAKE 11u /* type 1 or 2: a handshake message, listed in host_list for the host */
#define WG_RX_PT_AFTER 0u
#define WG_RX_PT_PACKED 1u
typedef struct wg_rx_summary {
  uint64_t pt_used; /* PACKED: bytes of the plaintext ring this batch takes (may exceed what fits) */
  uint32_t n_open;  /* packets with rx_status WG_PKT_OK */
  uint32_t n_host;  /* entries of host_list */
} wg_rx_summary;
typedef struct wg_rx_batch {
  const uint8_t* wire;     /* UDP ring (device) */
  uint64_t wire_size;
  const uint64_t* pkt_off; /* device, n entries */
  const uint32_t* pkt_len; /* device, n entries */
  wg_pkt* desc_out;        /* device, 16-byte aligned, n entries: for wg_open_batch */
  uint32_t* rx_status;     /* device, n entries, WG_PKT_* */
  uint32_t* host_list;     /* device, n entries: batch indices of handshake messages, ascending */
  wg_rx_summary* summary;  /* device, 16 bytes */
  uint64_t pt_base;        /* WG_RX_PT_PACKED: where this batch's plaintexts start in the open's output buffer */
  uint64_t pt_size;        /* WG_RX_PT_PACKED: size of that buffer */
  uint32_t n;
  uint32_t max_len;
  uint32_t mode;           /* WG_RX_PT_AFTER or WG_RX_PT_PACKED */
  uint32_t _reserved;
} wg_rx_batch;
typedef struct wg_rx_item {
  uint64_t off; /* of the plaintext in the open's output buffer (= desc.out_off) */
  uint32_t len;
  uint32_t key_slot;
} wg_rx_item;
typedef struct wg_rx_delivered {
  uint64_t bytes;       /* sum of len over the items */
  uint32_t n_items;
  uint32_t n_keepalive; /* final status WG_PKT_KEEPALIVE */
} wg_rx_delivered;
typedef struct wg_rx_deliver_batch {
  const wg_pkt* desc;          /* device, n entries: the plan's desc_out */
  const uint32_t* plan_status; /* device, n entries: the plan's rx_status */
  const uint32_t* open_status; /* device, n entries: the open's status after wg_rx_check */
  uint32_t* final_status;      /* device, n entries */
  wg_rx_item* items;           /* device, 16-byte aligned, n entries */
  uint32_t* index_out;         /* device, n entries, or NULL */
  wg_rx_delivered* delivered;  /* device, 16 bytes */
  uint32_t n;
  uint32_t _reserved;
} wg_rx_deliver_batch;
int wg_rx_sessions_set(wg_ctx* ctx, const uint32_t* indices_host, const uint32_t* key_slots_host, uint32_t n);
int wg_rx_reserve(wg_ctx* ctx, uint32_t max_packets);
int wg_rx_plan(wg_ctx* ctx, const wg_rx_batch* batch, void* stream);
int wg_rx_deliver(wg_ctx* ctx, const wg_rx_deliver_batch* batch, void* stream);

/* ---- handshake admission: batched BLAKE2s, mac1 and mac2 on the device ----
 * The device counterpart of the first thing the reference does with an incoming initiation or response,
 * before any Noise work (IncomingInitiation.java:24-40, IncomingResponse.java:20-36): mac1 =
 * BLAKE2s-128(key = BLAKE2s-256("mac1----" || local static public key), the message without its two
 * MACs) (InitiationPacket.calculateMac1, InitiationPacket.java:110-120; ResponsePacket.java:107-117) must
 * equal the message's mac1 field, and its mac2 field must be all zero (IncomingInitiation.java:38-40:
 * cookies are not implemented). wg_rx_plan lists the handshake datagrams of a UDP ring; wg_hs_check
 * tests them where they lie and compacts the accepted ones into records, so the host copies back
 * 16 + 160 n_valid bytes and starts Noise on those; it never fetches the ring. The initiations' static DH
 * and the open of their encrypted static follow in the next two sections; the rest of the Noise state
 * machine and its timers stay on the host. wg_hs_admit ("cookie replies and mac2 under load" below) is the
 * same check for a responder that demands cookies.
 *
 * wg_blake2s_batch(ctx, desc, n, in, in_size, out, out_size, status, stream): BLAKE2s (RFC 7693),
 *   sequential mode, fanout 1, depth 1, parameter word outlen | keylen << 8 | 0x01010000
 *   (Blake2s.java:94). out[out_off .. out_off + outlen) = the digest of size outlen of in[in_off ..
 *   in_off + len) under the key in[key_off .. key_off + keylen) (keylen 0: unkeyed): what
 *   Crypto.BLAKE2s256 and new Blake2s(n, key) compute. Every offset may have any alignment. status[i] is
 *   WG_B2S_OK, or WG_B2S_BADDESC when outlen is 0 or above 32, keylen above 32, or one of the three
 *   ranges leaves its buffer (each tested as off <= size && len <= size - off, which cannot overflow;
 *   the key range of an unkeyed descriptor is the empty range at key_off); a BADDESC leaves the output
 *   untouched. desc: device, 16-byte aligned. n = 0 is a no-op; out must not overlap in (WG_EINVAL).
 *   Asynchronous on `stream`, no host state, can be captured. The kernel reads the input as aligned
 *   32-bit words: those that hold at least one byte of a range, never another.
 *
 * wg_hs_key_set(ctx, static_public): derives the mac1 key of the local static public key, on the
 *   device (the library has no host hash), into a 32-byte device buffer that keeps its address for the
 *   life of the context: a captured check reads the key when it runs, so a new key needs no re-capture.
 *   Synchronous, and ordered after every check queued before it, like wg_rx_sessions_set. The key is
 *   wiped by wg_ctx_destroy. wg_hs_check without a key returns WG_ENOKEY.
 *
 * wg_hs_check(ctx, b, stream): wire / wire_size / pkt_off / pkt_len / n as in wg_rx_batch. list is a
 *   device array of batch indices (the plan's host_list) and n_list a device pointer to its length
 *   (&summary->n_host of the plan); the length is read on the device (at most n entries are looked
 *   at), so nothing is synchronised between plan and check. list = NULL (then n_list must be NULL too)
 *   is the identity list: every one of the n datagrams. For list position k, i = list[k], o =
 *   pkt_off[i], wl = pkt_len[i], in this order:
 *   1. i >= n, wl == 0, o > wire_size or wl > wire_size - o: WG_HS_BADLEN.
 *   2. t = wire[o] is neither 1 nor 2: WG_HS_BADTYPE (only a caller-made or the identity list gets here).
 *   3. wl != L, L = 148 for t = 1 and 92 for t = 2 (InitiationPacket.HEADER_LAYOUT,
 *      ResponsePacket.HEADER_LAYOUT): WG_HS_BADLEN. The reference never looks at the received length of
 *      a handshake message: it reads the layout out of a pooled buffer (PacketElement.java:102-113),
 *      whatever was received. That cannot be restated over a ring; WireGuard's own rule, the exact
 *      size, is applied instead.
 *   4. BLAKE2s-128(mac1 key, msg[0 .. L - 32)) != msg[L - 32 .. L - 16): WG_HS_BADMAC1. All 16 bytes
 *      are compared, without an early exit.
 *   5. msg[L - 16 .. L) is not all zero: WG_HS_BADMAC2.
 *   6. WG_HS_OK.
 *   hs_status[k] is written for every k < the list's length and nothing behind it. records[0 ..
 *   n_valid) is the stable compaction, in list order, of the WG_HS_OK messages: {index = i, len = L,
 *   msg = the message, zero-filled behind a response, _pad = 0}; every byte of a written record is
 *   defined and nothing behind n_valid records is touched. summary = {n_valid, n_init, n_resp (the
 *   accepted messages of type 1 / 2), n_rejected}. n = 0 writes only the summary (zeros). records:
 *   16-byte aligned; summary: 8-byte aligned. The rank takes three launches (check, scan, emit) with no
 *   wait between workgroups; the scratch is written before it is read in every call and nothing about a
 *   call lives on the host, so a captured plan + check replays. Calls on different streams of one
 *   context are ordered by the library; a graph launch is the caller's to order.
 *   wg_hs_reserve(ctx, max_messages): scratch for checks of up to max_messages datagrams; a call that
 *   needs more allocates it, except on a capturing stream (WG_EINVAL: reserve first). */
#define WG_B2S_OK 0u
#define WG_B2S_BADDESC 1u
#define WG_HS_OK 0u
#define WG_HS_BADLEN 1u  /* index or datagram out of bounds, or not the exact size of its type */
#define WG_HS_BADTYPE 2u /* the type byte is neither 1 nor 2 */
#define WG_HS_BADMAC1 3u
#define WG_HS_BADMAC2 4u /* mac2 is not all zero */
#define WG_HS_INIT_SIZE 148u
#define WG_HS_RESP_SIZE 92u
typedef struct wg_b2s_desc { /* 32 bytes, 16-byte aligned */
  uint64_t in_off, out_off, key_off;
  uint32_t len;
  uint8_t outlen, keylen, _pad[2];
} wg_b2s_desc;
typedef struct wg_hs_record { /* 160 bytes */
  uint32_t index; /* batch index of the datagram */
  uint32_t len;   /* 148 or 92 */
  uint8_t msg[148];
  uint32_t _pad;
} wg_hs_record;
typedef struct wg_hs_summary {
  uint32_t n_valid, n_init, n_resp, n_rejected;
} wg_hs_summary;
typedef struct wg_hs_batch {
  const uint8_t* wire;     /* UDP ring (device) */
  uint64_t wire_size;
  const uint64_t* pkt_off; /* device, n entries */
  const uint32_t* pkt_len; /* device, n entries */
  const uint32_t* list;    /* device, batch indices (the plan's host_list), or NULL: all n datagrams */
  const uint32_t* n_list;  /* device, the list's length (&wg_rx_summary.n_host); NULL with list = NULL */
  uint32_t* hs_status;     /* device, n entries, WG_HS_*, indexed by list position */
  wg_hs_record* records;   /* device, 16-byte aligned, n entries */
  wg_hs_summary* summary;  /* device, 16 bytes */
  uint32_t n;
  uint32_t _reserved;
} wg_hs_batch;
int wg_blake2s_batch(wg_ctx* ctx, const wg_b2s_desc* desc_dev, uint32_t n, const uint8_t* in_dev, uint64_t in_size,
                     uint8_t* out_dev, uint64_t out_size, uint32_t* status_dev, void* stream);
int wg_hs_key_set(wg_ctx* ctx, const uint8_t* static_public /* 32 bytes */);
int wg_hs_reserve(wg_ctx* ctx, uint32_t max_messages);
int wg_hs_check(wg_ctx* ctx, const wg_hs_batch* batch, void* stream);

/* ---- batched X25519 and the initiations' static DH, on the device ----
 * mac1 needs only the local static PUBLIC key, so whoever knows it can fill a ring with messages that pass
 * wg_hs_check; the first thing the responder then does with each initiation is
 * localKeypair.sharedSecret(remoteEphemeral) (Handshakes.java:210), one Curve25519 ladder per datagram.
 * wg_x25519_batch is that primitive over descriptors, the analogue of wg_blake2s_batch; wg_hs_dh runs it
 * over wg_hs_check's records with the static private key of wg_hs_static_set, at the end of the plan ->
 * check chain. The KDF and hash chain up to the initiator's static key and the open of encrypted_static
 * follow in the next section (wg_hs_open), the response in the one after it (wg_hs_respond); the state
 * machine, cookies and timers stay on the host.
 *
 * wg_x25519_batch(ctx, desc, n, in, in_size, out, out_size, status, stream): out[out_off .. out_off + 32)
 *   = X25519(in[scalar_off .. + 32), in[point_off .. + 32)) as X25519.scalarMult computes it
 *   (crypto/internal/X25519.java:24-28, 50-60, 96-155; RFC 7748 5): the scalar is clamped on the device
 *   (k[0] &= 0xF8, k[31] &= 0x7F, k[31] |= 0x40), bit 255 of u is ignored (X25519Field.decode :123-128), a
 *   non-canonical u (p <= u < 2^255) is accepted and reduced by the arithmetic, and the output is the
 *   canonical little-endian x2 * z2^(p-2) mod p. WG_X25519_BASE in flags takes the base point u = 9
 *   (point_off is ignored): what generatePublicKey gives. status[i] is WG_X25519_OK; WG_X25519_ZERO when
 *   the result is all zero (a low-order point): the 32 zero bytes are written all the same, as
 *   NoisePrivateKey.sharedSecret (NoisePrivateKey.java:48-52) ignores calculateAgreement's false; or
 *   WG_X25519_BADDESC when an unknown flag bit is set, _pad is not 0, or the scalar range, the point
 *   range (unless BASE) or the output range of 32 bytes leaves its buffer (each tested as off <= size &&
 *   32 <= size - off): a BADDESC leaves the output untouched. Every offset may have any alignment; the
 *   kernel reads operands as aligned 32-bit words: those that hold at least one byte of a range, never
 *   another. desc: device, 16-byte aligned. n = 0 is a no-op; out must not overlap in (WG_EINVAL).
 *   Asynchronous on `stream`, no host state, no scratch, can be captured. One ladder per lane, in
 *   constant time: no branch, address or loop bound depends on a scalar bit or a field value; lanes with
 *   a bad descriptor run the same code on dummy operands.
 *
 * wg_hs_static_set(ctx, static_private, static_public_out): copies the local static private key into a
 *   32-byte device buffer that keeps its address for the life of the context (a captured wg_hs_dh reads
 *   the key when it runs, so a new key needs no re-capture), derives the public key on the device
 *   (WG_X25519_BASE), returns it in static_public_out (32 bytes; may be NULL) and sets the mac1 key from
 *   it exactly as wg_hs_key_set(public) would. Synchronous, and ordered after every check or DH queued
 *   before it. wg_ctx_destroy wipes the private key. A later wg_hs_key_set replaces only the mac1 key.
 *   wg_hs_dh without a private key returns WG_ENOKEY.
 *
 * wg_hs_dh(ctx, b, stream): for every k < min(*n_records, n) (n_records: a device pointer, usually
 *   &summary->n_valid of the check, read on the device, so plan -> check -> dh run back to back with no
 *   host read; NULL: all n): a record with len == 148 gives shared[32 k .. 32 k + 32) = X25519(static
 *   private, msg[8 .. 40)), the initiation's unencrypted_ephemeral (InitiationPacket.java:35-44), and
 *   dh_status[k] = WG_X25519_OK or WG_X25519_ZERO; a record with len == 92 (a response: the host holds
 *   that handshake's ephemeral private key, Handshakes.java:125) gives 32 zero bytes and
 *   WG_X25519_SKIPPED; any other len gives WG_X25519_BADDESC and leaves the 32 bytes untouched. Nothing
 *   behind min(*n_records, n) entries is written, in either array. No scratch and no reserve call: a
 *   captured plan + check + dh replays. */
#define WG_X25519_OK 0u
#define WG_X25519_BADDESC 1u
#define WG_X25519_ZERO 2u    /* the result is all zero (a low-order point): written, and flagged */
#define WG_X25519_SKIPPED 3u /* wg_hs_dh only: the record is a response */
#define WG_X25519_BASE 1u    /* desc.flags: the point is the base point u = 9; point_off is ignored */
typedef struct wg_x25519_desc { /* 32 bytes, 16-byte aligned */
  uint64_t scalar_off, point_off, out_off;
  uint32_t flags, _pad;
} wg_x25519_desc;
typedef struct wg_hs_dh_batch {
  const wg_hs_record* records; /* device, 16-byte aligned: wg_hs_check's records */
  const uint32_t* n_records;   /* device: &wg_hs_summary.n_valid; NULL: all n */
  uint8_t* shared;             /* device, 16-byte aligned, n * 32 bytes */
  uint32_t* dh_status;         /* device, n entries, WG_X25519_* */
  uint32_t n, _reserved;
} wg_hs_dh_batch;
int wg_x25519_batch(wg_ctx* ctx, const wg_x25519_desc* desc_dev, uint32_t n, const uint8_t* in_dev, uint64_t in_size,
                    uint8_t* out_dev, uint64_t out_size, uint32_t* status_dev, void* stream);
int wg_hs_static_set(wg_ctx* ctx, const uint8_t* static_private /* 32 bytes */, uint8_t* static_public_out /* 32 bytes, may be NULL */);
int wg_hs_dh(wg_ctx* ctx, const wg_hs_dh_batch* batch, void* stream);

/* ---- the initiations' encrypted static, opened on the device ----
 * What rejects a forged initiation comes after mac1 and the DH: Handshakes.decryptRemoteStatic
 * (Handshakes.java:201-237; per initiation from PeerList.java:80 and SessionManager.java:212). wg_hs_open is
 * that step over wg_hs_check's records and wg_hs_dh's secrets, bit-exact, with the peer lookup behind it:
 * the host receives the authenticated initiations, by peer, with the Noise state the responder goes on
 * from, and reads nothing in between. With H = BLAKE2s-256, KDFn(salt, ikm) = Crypto.deriveKey(salt, ikm,
 * n) (HKDF over HMAC-BLAKE2s, 64-byte block, empty info: Crypto.java:39-99), CK0 = INITIAL_CHAIN_KEY, H0 =
 * INITIAL_HASH (Handshakes.java:20-37), E = msg[8 .. 40), es = msg[40 .. 88), ets = msg[88 .. 116)
 * (InitiationPacket.java:21-45) and ss = shared[32 k .. 32 k + 32):
 *     h  = H(H(H0 || S_pub) || E)      ck = KDF1(CK0, E)
 *     k  = KDF2(ck, ss)                ck = KDF1(ck, ss)
 *     remote_static = ChaCha20-Poly1305-open(k, nonce 0^12, aad = h, es), else WG_HS_OPEN_BADAUTH
 *     h  = H(h || es)
 *     known peer: ck = KDF1(ck, X25519(S_priv, remote_static))
 *     h  = H(h || ets)
 *   (state.chainKey and decryptRemoteStatic's local chainKey are one array, Handshakes.java:203 and
 *   :314-316, so this is the ordinary Noise IK chain.) Like the reference, the step never opens ets: its 28
 *   bytes are only mixed into the hash (:233-234). A record whose dh_status is WG_X25519_ZERO goes through
 *   like any other (the reference ignores the agreement's false).
 *
 * wg_hs_peers_set(ctx, publics, n): replaces the whole table of the peers' static public keys (host
 *   pointer, 32 n bytes) and computes, in one launch, each peer's X25519(static private key, public key),
 *   which stays on the device. A peer is named by its position in `publics`. Keys are compared in all 32
 *   bytes (bit 255 as the byte it is); two equal keys are WG_EINVAL and nothing changes. n = 0 empties the
 *   table. Without a private key: WG_ENOKEY. The table sits behind a header at a fixed device address: a
 *   captured open sees the new table without re-capture. Synchronous, and ordered after everything queued
 *   before it. A later wg_hs_static_set recomputes the stored peers' secrets under the new key, and keeps
 *   H(H0 || S_pub) beside the mac1 key; wg_hs_key_set touches neither. wg_ctx_destroy wipes the secrets.
 *
 * wg_hs_open(ctx, b, stream): for every k < min(*n_records, n) (n_records as in wg_hs_dh; NULL: all n),
 *   with len = records[k].len and ds = dh_status[k], in this order:
 *   1. len == 92: WG_HS_OPEN_SKIPPED (a response). 2. len != 148: WG_HS_OPEN_BADDESC.
 *   3. ds == WG_X25519_SKIPPED: WG_HS_OPEN_SKIPPED. 4. ds is neither WG_X25519_OK nor WG_X25519_ZERO:
 *   WG_HS_OPEN_BADDESC. 5. the tag of es does not verify (all 16 bytes compared, no early exit):
 *   WG_HS_OPEN_BADAUTH. 6. remote_static is in the table: WG_HS_OPEN_OK, else WG_HS_OPEN_NEWPEER (the
 *   reference adds such a peer, PeerList.java:85-86: the host decides).
 *   open_status[k] is written for those k and nothing behind them. inits[0 .. n_emitted) is the stable
 *   compaction, in record order, of the OK and NEWPEER records: {index = records[k].index, record = k,
 *   sender_index = msg[4 .. 8), peer = the position in the table or WG_HS_NOPEER, remote_ephemeral = E,
 *   remote_static, hash = the final h, chain_key = the final ck; for a NEWPEER the ck BEFORE the
 *   static-static step, which one ladder and one KDF1 on the host finish}. Every byte of a written entry is
 *   defined; nothing behind n_emitted entries is touched, and nothing but its status is written for any
 *   other record. summary = {n_emitted, n_known (OK), n_badauth, n_skipped}. n = 0 is a no-op. Works with an
 *   empty or never-set table (every authentic initiation is NEWPEER). Without a private key: WG_ENOKEY.
 *   records, shared, inits: 16-byte aligned; summary: 8; the others: 4. An output that overlaps another
 *   output or an input: WG_EINVAL. Scratch (112 bytes per record) is sized by wg_hs_reserve; a call that
 *   needs more allocates it, except on a capturing stream (WG_EINVAL: reserve first). Three launches
 *   (open, scan, emit) with no wait between workgroups and nothing about a call on the host: a captured
 *   plan + check + dh + open replays, and wg_hs_peers_set / wg_hs_static_set between replays need no
 *   re-capture. One record per lane; no branch, address or loop bound depends on ss, on a derived key or
 *   on a static-static secret. */
#define WG_HS_OPEN_OK 0u
#define WG_HS_OPEN_NEWPEER 1u /* authentic; the static key is not in the peer table */
#define WG_HS_OPEN_BADAUTH 2u
#define WG_HS_OPEN_SKIPPED 3u /* a response, or dh_status is WG_X25519_SKIPPED */
#define WG_HS_OPEN_BADDESC 4u /* any other record length, or dh_status is WG_X25519_BADDESC */
#define WG_HS_NOPEER 0xFFFFFFFFu
typedef struct wg_hs_init { /* 144 bytes */
  uint32_t index;        /* batch index of the datagram */
  uint32_t record;       /* position in wg_hs_check's records */
  uint32_t sender_index; /* msg[4 .. 8) */
  uint32_t peer;         /* position in wg_hs_peers_set's table, or WG_HS_NOPEER */
  uint8_t remote_ephemeral[32];
  uint8_t remote_static[32];
  uint8_t hash[32];
  uint8_t chain_key[32];
} wg_hs_init;
typedef struct wg_hs_open_summary {
  uint32_t n_emitted, n_known, n_badauth, n_skipped;
} wg_hs_open_summary;
typedef struct wg_hs_open_batch {
  const wg_hs_record* records; /* device, 16-byte aligned: wg_hs_check's records */
  const uint32_t* n_records;   /* device: &wg_hs_summary.n_valid; NULL: all n */
  const uint8_t* shared;       /* device, 16-byte aligned, n * 32 bytes: wg_hs_dh's */
  const uint32_t* dh_status;   /* device, n entries: wg_hs_dh's */
  uint32_t* open_status;       /* device, n entries, WG_HS_OPEN_* */
  wg_hs_init* inits;           /* device, 16-byte aligned, n entries */
  wg_hs_open_summary* summary; /* device, 16 bytes, 8-byte aligned */
  uint32_t n, _reserved;
} wg_hs_open_batch;
int wg_hs_peers_set(wg_ctx* ctx, const uint8_t* publics_host /* 32 n bytes */, uint32_t n);
int wg_hs_open(wg_ctx* ctx, const wg_hs_open_batch* batch, void* stream);

/* ---- the answer to an initiation, on the device ----
 * After wg_hs_open the dearest part of the handshake is left: ResponderHandshake.deriveKeypair
 * (Handshakes.java:250-287) and OutgoingResponse (OutgoingResponse.java:16-25, ResponsePacket.java:107-117):
 * a fresh ephemeral key, three X25519 ladders, five HKDFs, an AEAD seal of nothing and a keyed BLAKE2s per
 * initiation. The device lacks only the randomness, which the host hands in as a buffer. wg_hs_respond turns
 * wg_hs_open's entries into ready-to-send 92-byte responses and the transport key pairs, bit-exact. With H,
 * KDFn as in the section above, h / ck / E_i / S_i = the entry's hash / chain_key / remote_ephemeral /
 * remote_static, e = the clamped ephemeral and psk = 32 zero bytes (the reference's responder, :262):
 *     Epub = X25519(e, 9)          h = H(h || Epub)         ck = KDF1(ck, Epub)
 *     ck = KDF1(ck, X25519(e, E_i))                         ck = KDF1(ck, X25519(e, S_i))
 *     tau = KDF2(ck, psk)   k = KDF3(ck, psk)   ck = KDF1(ck, psk)      (all three from the same ck)
 *     h = H(h || tau)       empty = ChaCha20-Poly1305-seal(k, nonce 0^12, aad = h, "")   (the 16-byte tag)
 *     recv_key = KDF1(ck, "")      send_key = KDF2(ck, "")               (:286: the responder sends with T2)
 *     response = {2, 0,0,0, LE32(local_index), LE32(sender_index), Epub, empty,
 *                 mac1 = BLAKE2s-128(key = H("mac1----" || S_i), response[0 .. 60)), mac2 = 0^16}
 *   A low-order E_i or S_i gives an all-zero secret and goes through (the reference ignores the agreement's
 *   false). The final h is needed by nobody and is not stored.
 *
 * wg_hs_respond(ctx, b, stream): for every k < min(*n_inits, n) (n_inits: a device pointer, usually
 *   &wg_hs_open_summary.n_emitted; NULL: all n), in this order:
 *   1. flags has WG_HS_RESP_SKIP_NEWPEER and inits[k].peer == WG_HS_NOPEER: WG_HS_RESP_NOPEER (wg_hs_open left
 *   that entry's chain_key before the static-static step: the chain must not go on from it). Without the flag
 *   the caller vouches that every entry's chain_key is final, and peer is only copied through.
 *   2. the 32 bytes ephemerals[32 k ..) are all zero, tested before clamping: WG_HS_RESP_NOEPH. 3. WG_HS_RESP_OK.
 *   ephemerals holds fresh private keys from the host's CSPRNG, clamped on the device as every scalar is; it
 *   is input AND output: the call zeroes each one it consumed and leaves a non-OK entry's untouched, so a
 *   replay of a captured graph without a refresh answers nothing (all NOEPH). local_index[k] is the
 *   responder's new session index, as allocateNewSessionIndex would choose it on the host. resp_status[k] is
 *   written for the covered k and nothing behind them. sessions[0 .. n_ok) is the stable compaction of the
 *   OK entries: {index = inits[k].index, init = k, peer = inits[k].peer, local_index = local_index[k],
 *   response, remote_index = inits[k].sender_index, send_key, recv_key}; every byte of a written session is
 *   defined and nothing behind n_ok sessions is touched. summary = {n_ok, n_nopeer, n_noeph, 0}. n = 0 is a
 *   no-op. Without a private key: WG_ENOKEY. Unknown flag bits: WG_EINVAL. n above 2^30: WG_E2BIG. inits, ephemerals, sessions:
 *   16-byte aligned; summary: 8; the others: 4. An output (ephemerals among them) that overlaps another output
 *   or an input: WG_EINVAL. Scratch (272 bytes per entry, holding DH results and keys only for the time of
 *   the call) is sized by wg_hs_reserve; a call that needs more allocates it, except on a capturing stream
 *   (WG_EINVAL: reserve first); wg_ctx_destroy wipes it. Four launches (ladders, chain, scan, emit), no wait
 *   between workgroups, nothing about a call on the host: a captured plan + check + dh + open + respond
 *   replays; between replays the host refreshes ephemerals and local_index in place. The three ladders of an
 *   entry run in three neighbouring lanes. No branch, address or loop bound depends on an ephemeral's value, a
 *   DH result, ck, tau, k or a transport key, except the all-zero test of the raw ephemeral. wg_hs_install
 *   ("handshake sessions installed on the device" below) turns the sessions into transport sessions. */
#define WG_HS_RESP_OK 0u
#define WG_HS_RESP_NOPEER 1u       /* SKIP_NEWPEER, and the entry's peer is WG_HS_NOPEER */
#define WG_HS_RESP_NOEPH 2u        /* the entry's ephemeral is all zero */
#define WG_HS_RESP_SKIP_NEWPEER 1u /* flags: do not answer an entry whose peer is WG_HS_NOPEER */
typedef struct wg_hs_session { /* 176 bytes */
  uint32_t index;       /* batch index of the initiation's datagram */
  uint32_t init;        /* position in inits */
  uint32_t peer;        /* inits[init].peer */
  uint32_t local_index; /* the responder's session index used */
  uint8_t response[92]; /* the wire message */
  uint32_t remote_index; /* inits[init].sender_index */
  uint8_t send_key[32];
  uint8_t recv_key[32];
} wg_hs_session;
typedef struct wg_hs_respond_summary {
  uint32_t n_ok, n_nopeer, n_noeph, _zero;
} wg_hs_respond_summary;
typedef struct wg_hs_respond_batch {
  const wg_hs_init* inits;        /* device, 16-byte aligned: wg_hs_open's entries, or the caller's */
  const uint32_t* n_inits;        /* device: &wg_hs_open_summary.n_emitted; NULL: all n */
  uint8_t* ephemerals;            /* device, 16-byte aligned, n * 32 bytes; in and out */
  const uint32_t* local_index;    /* device, n entries */
  uint32_t* resp_status;          /* device, n entries, WG_HS_RESP_* */
  wg_hs_session* sessions;        /* device, 16-byte aligned, n entries */
  wg_hs_respond_summary* summary; /* device, 16 bytes, 8-byte aligned */
  uint32_t n, flags;
} wg_hs_respond_batch;
int wg_hs_respond(wg_ctx* ctx, const wg_hs_respond_batch* batch, void* stream);

/* ---- the initiator's side, on the device ----
 * A node that restarts, or whose sessions expire together, initiates to every peer that has an endpoint
 * (SessionManager.attemptInitiatorHandshake, SessionManager.java:170-207). wg_hs_initiate is InitiatorStageOne's
 * constructor and OutgoingInitiation (Handshakes.java:77-117, OutgoingInitiation.java:22-38,
 * InitiationPacket.java:110-120) over a batch; wg_hs_finish is consumeMessageResponse (Handshakes.java:119-151)
 * over wg_hs_check's records on the initiator's context. Both bit-exact. With H, KDFn, CK0, H0 as above, S the
 * static private key, S_pub its public key, S_r = the peer's static public key in wg_hs_peers_set's table, ss_r =
 * that table's stored X25519(S, S_r), e = the ephemeral:
 *     Epub = X25519(e, 9)       h = H(H(H0 || S_r) || Epub)        ck = KDF1(CK0, Epub)
 *     es = X25519(e, S_r)       k = KDF2(ck, es)   ck = KDF1(ck, es)
 *     enc_static = ChaCha20-Poly1305-seal(k, nonce 0^12, aad = h, S_pub)   (48 B)     h = H(h || enc_static)
 *     k = KDF2(ck, ss_r)        ck = KDF1(ck, ss_r)
 *     enc_ts = ChaCha20-Poly1305-seal(k, nonce 0^12, aad = h, timestamp)   (28 B)     h = H(h || enc_ts)
 *     msg = {1, 0,0,0, LE32(local_index), Epub, enc_static, enc_ts,
 *            mac1 = BLAKE2s-128(key = H("mac1----" || S_r), msg[0 .. 116)), mac2 = 0^16}
 *   and for a response with E_r = msg[12 .. 44), h / ck / e from the pending entry, psk = the peer's:
 *     h = H(h || E_r)     ck = KDF1(ck, E_r)     ck = KDF1(ck, X25519(e, E_r))     ck = KDF1(ck, X25519(S, E_r))
 *     tau = KDF2(ck, psk)   k = KDF3(ck, psk)   ck = KDF1(ck, psk)       h = H(h || tau)
 *     the Poly1305 tag of (aad = h, no ciphertext) under k, nonce 0^12, must equal msg[44 .. 60)
 *     send_key = KDF1(ck, "")      recv_key = KDF2(ck, "")            (:147: the initiator sends with T1)
 *
 * wg_hs_psks_set(ctx, psks, n): the peers' preshared keys (connectionInfo.presharedKey(), SessionManager.java:172;
 *   host pointer, 32 n bytes, by position in the peer table). n must equal the table's count, else WG_EINVAL.
 *   wg_hs_peers_set resets every psk to 32 zero bytes. Synchronous, and ordered after everything queued before
 *   it. The psks sit behind a header at a fixed device address: a captured finish sees new psks without
 *   re-capture. wg_ctx_destroy wipes them. The reference's responder, and wg_hs_respond, use the zero psk
 *   (Handshakes.java:262): only a zero-psk initiator interoperates with them.
 *
 * wg_hs_initiate(ctx, b, stream): for every k < n, in this order:
 *   1. peer[k] >= the table's count: WG_HS_INIT_BADPEER. 2. the 32 bytes ephemerals[32 k ..) are all zero,
 *   tested before clamping: WG_HS_INIT_NOEPH. 3. WG_HS_INIT_OK. Both failures are the caller's own mistakes,
 *   not traffic: the outputs are aligned to position, not compacted. status[k]; records[k] = {index = k, len =
 *   148, msg, _pad = 0} (what wg_hs_dh and wg_hs_open read), 160 zero bytes for a non-OK entry; pending[k] =
 *   {state = 1, peer, local_index, 0, ephemeral = the raw private key, hash = the final h, chain_key = the final
 *   ck}, 112 zero bytes for a non-OK entry; summary = {n_ok, n_badpeer, n_noeph, 0}. Every byte of every output
 *   up to n is defined, nothing behind n is touched. ephemerals (fresh private keys from the host's CSPRNG,
 *   clamped on the device) is input AND output: an OK entry's 32 bytes are zeroed, the others left alone, so a
 *   replayed graph without fresh keys initiates nothing (all NOEPH). timestamps: 12 bytes each, the host's
 *   TAI64N. n = 0 is a no-op. Without a private key: WG_ENOKEY. n above 2^30: WG_E2BIG. ephemerals, records,
 *   pending: 16-byte aligned; summary: 8; the others: 4. An output (ephemerals among them) that overlaps another
 *   output or an input: WG_EINVAL. Scratch (64 bytes per entry, holding the ladders' results only for the time
 *   of the call) is sized by wg_hs_reserve; a call that needs more allocates it, except on a capturing stream
 *   (WG_EINVAL: reserve first); wg_ctx_destroy wipes it. Three launches (ladders, chain, scan). The two ladders
 *   of an entry run in two neighbouring lanes.
 *
 * wg_hs_finish(ctx, b, stream): for every k < min(*n_records, n) (n_records as in wg_hs_dh; NULL: all n), in this
 *   order: 1. records[k].len == 148: WG_HS_FIN_SKIPPED (an initiation). 2. len != 92: WG_HS_FIN_BADDESC. 3. no
 *   live pending entry (state == 1 and peer below the table's count) has local_index == msg[8 .. 12):
 *   WG_HS_FIN_NOPENDING; if several live entries share a local_index, the lowest position is the one found.
 *   4. the tag does not verify (all 16 bytes compared, no early exit): WG_HS_FIN_BADAUTH. 5. WG_HS_FIN_OK.
 *   fin_status[k] is written for the covered k and nothing behind them. established[0 .. n_ok) is the stable
 *   compaction of the OK records: {index = records[k].index, record = k, pending = the entry's position, peer,
 *   local_index, remote_index = msg[4 .. 8), 0, 0, send_key, recv_key}; nothing behind n_ok entries is touched.
 *   summary = {n_ok, n_nopending, n_badauth, n_skipped}. pending (n_pending entries) is input AND output: an OK
 *   record's entry is overwritten with zeros, so a replayed response, or a replayed graph, finds nothing
 *   (NOPENDING); a BADAUTH record leaves its entry byte for byte as it was (mac1 needs only the public key: a
 *   forger must not be able to cancel a handshake). If two records of one call authenticate against the same
 *   pending entry, both are emitted, in record order and with the same `pending` field; the host keeps the
 *   first. n = 0 is a no-op. Without a private key: WG_ENOKEY. n above 2^30 or n_pending above 2^28: WG_E2BIG.
 *   records, pending, established: 16-byte aligned; summary: 8; the others: 4. An output (pending among them)
 *   that overlaps another output or an input: WG_EINVAL. The receiver index is matched on the device: an
 *   open-addressing table of pending positions in scratch (the smallest power of two >= max(16, 4 n_pending)
 *   words), filled and built by the call's first two launches; the lowest position wins a shared local_index.
 *   Scratch (160 bytes per record, 16 per pending entry) by wg_hs_reserve(max(n, n_pending)), as above. Six
 *   launches (fill, insert, ladders, chain, scan, emit; the emit zeroes the consumed entries), no wait between workgroups, nothing about a
 *   call on the host: a captured check + finish replays.
 *   For both calls: no branch, address or loop bound depends on an ephemeral's value, a DH result, ck, tau, k, a
 *   psk's value or a transport key, except the all-zero test of the raw ephemeral; the receiver index and the
 *   peer position are public. wg_hs_install ("handshake sessions installed on the device" below) turns the
 *   established entries into transport sessions. */
#define WG_HS_INIT_OK 0u
#define WG_HS_INIT_BADPEER 1u /* peer[k] is not a position in the peer table */
#define WG_HS_INIT_NOEPH 2u   /* the entry's ephemeral is all zero */
#define WG_HS_FIN_OK 0u
#define WG_HS_FIN_NOPENDING 1u /* no live pending entry has the response's receiver index */
#define WG_HS_FIN_BADAUTH 2u
#define WG_HS_FIN_SKIPPED 3u /* an initiation */
#define WG_HS_FIN_BADDESC 4u /* any other record length */
typedef struct wg_hs_pending { /* 112 bytes */
  uint32_t state;       /* 1: live, 0: empty */
  uint32_t peer;        /* position in wg_hs_peers_set's table */
  uint32_t local_index; /* the sender index of the initiation */
  uint32_t _zero;
  uint8_t ephemeral[32]; /* the raw ephemeral private key */
  uint8_t hash[32];
  uint8_t chain_key[32];
} wg_hs_pending;
typedef struct wg_hs_established { /* 96 bytes */
  uint32_t index;        /* batch index of the response's datagram */
  uint32_t record;       /* position in wg_hs_check's records */
  uint32_t pending;      /* position in pending */
  uint32_t peer;
  uint32_t local_index;  /* the initiator's session index: msg[8 .. 12) */
  uint32_t remote_index; /* the responder's: msg[4 .. 8) */
  uint32_t _zero[2];
  uint8_t send_key[32];
  uint8_t recv_key[32];
} wg_hs_established;
typedef struct wg_hs_initiate_summary {
  uint32_t n_ok, n_badpeer, n_noeph, _zero;
} wg_hs_initiate_summary;
typedef struct wg_hs_initiate_batch {
  const uint32_t* peer;            /* device, n entries */
  uint8_t* ephemerals;             /* device, 16-byte aligned, n * 32 bytes; in and out */
  const uint8_t* timestamps;       /* device, 4-byte aligned, n * 12 bytes */
  const uint32_t* local_index;     /* device, n entries */
  uint32_t* status;                /* device, n entries, WG_HS_INIT_* */
  wg_hs_record* records;           /* device, 16-byte aligned, n entries */
  wg_hs_pending* pending;          /* device, 16-byte aligned, n entries */
  wg_hs_initiate_summary* summary; /* device, 16 bytes, 8-byte aligned */
  uint32_t n, _reserved;
} wg_hs_initiate_batch;
typedef struct wg_hs_finish_summary {
  uint32_t n_ok, n_nopending, n_badauth, n_skipped;
} wg_hs_finish_summary;
typedef struct wg_hs_finish_batch {
  const wg_hs_record* records;    /* device, 16-byte aligned: wg_hs_check's records */
  const uint32_t* n_records;      /* device: &wg_hs_summary.n_valid; NULL: all n */
  wg_hs_pending* pending;         /* device, 16-byte aligned, n_pending entries; in and out */
  uint32_t* fin_status;           /* device, n entries, WG_HS_FIN_* */
  wg_hs_established* established; /* device, 16-byte aligned, n entries */
  wg_hs_finish_summary* summary;  /* device, 16 bytes, 8-byte aligned */
  uint32_t n, n_pending;
} wg_hs_finish_batch;
int wg_hs_psks_set(wg_ctx* ctx, const uint8_t* psks_host /* 32 n bytes */, uint32_t n);
int wg_hs_initiate(wg_ctx* ctx, const wg_hs_initiate_batch* batch, void* stream);
int wg_hs_finish(wg_ctx* ctx, const wg_hs_finish_batch* batch, void* stream);

/* ---- the initiations' timestamps, opened on the device; replays refused ----
 * One captured 148-byte initiation of a known peer, sent again, passes mac1 and authenticates in wg_hs_open; it then
 * costs wg_hs_respond three ladders and five HKDFs, and wg_hs_install two key slots and a receiver-index entry,
 * every time. WireGuard's defence is the TAI64N timestamp sealed under the static-static key: a responder answers
 * an initiation only if its timestamp is greater than the greatest seen from that peer. The reference never opens
 * the timestamp (Handshakes.java:233-234) and has no such rule: like the replay window and cryptokey routing, this
 * is a protection the library ADDS, and there is nothing in the reference to be bit-exact with beyond the chain
 * that sealed the bytes (Handshakes.java:99-105, wg_hs_initiate). wg_hs_stamp sits between wg_hs_open and
 * wg_hs_respond. For entry j, with r = inits[j].record, p = inits[j].peer, E / es / ets = records[r].msg[8 .. 40) /
 * [40 .. 88) / [88 .. 116), ss = shared[32 r .. 32 r + 32), ss_p = the peer table's stored X25519(S_priv, S_p), and
 * H, KDFn, CK0, H0 as above:
 *     h  = H(H(H(H0 || S_pub) || E) || es)
 *     ck = KDF1(KDF1(CK0, E), ss)
 *     k  = KDF2(ck, ss_p)
 *     T  = ChaCha20-Poly1305-open(k, nonce 0^12, aad = h, ets)     (12 bytes; all 16 tag bytes compared, no early exit)
 *   This is wg_hs_open's chain once more (28 compressions): the key comes from the ck BEFORE the static-static step
 *   and the aad is the h before the last mix, and wg_hs_init, whose layout is fixed, carries only the final two. es is
 *   hashed, not verified again. T is read as ONE unsigned 96-bit big-endian number (memcmp order), which suits
 *   standard TAI64N and the reference's Crypto.TAI64N() (Crypto.java:19-27) alike.
 *
 * wg_hs_stamp(ctx, b, stream): for every j < min(*n_inits, n) (n_inits: a device pointer, usually
 *   &wg_hs_open_summary.n_emitted; NULL: all n), in this order:
 *   1. p == WG_HS_NOPEER: WG_HS_TS_NOPEER (no static-static secret on the device; the host finishes that chain
 *   itself, and the entry stays in inits for it). 2. p >= the table's count, r >= n_rec, or records[r].len != 148:
 *   WG_HS_TS_BADDESC. 3. the tag does not verify: WG_HS_TS_BADAUTH. 4. T <= stored[p], the peer's value at the START
 *   of the call: WG_HS_TS_REPLAY (an all-zero T is therefore never accepted). 5. among the entries of this call that
 *   passed 1-3 and have the same p, another has a greater T, or an equal T at a lower j: WG_HS_TS_SUPERSEDED.
 *   6. WG_HS_TS_OK, and stored[p] = T.
 *   Answering only the newest initiation of a peer leaves the same stored value and the same final session as
 *   WireGuard's one-by-one rule (accept iff T > stored, then stored = T) over the batch in arrival order; it spends
 *   no ladders on initiations that the next one overrides, and it depends on no dispatch order.
 *   ts_status[j] and opened[12 j .. 12 j + 12) are written for every covered j and nothing behind them: opened holds
 *   T where the tag verified (steps 4-6) and 12 zero bytes otherwise. fresh[0 .. n_ok) is the stable compaction of
 *   the OK entries, each a byte-for-byte copy of its 144-byte wg_hs_init; nothing behind n_ok entries is touched.
 *   summary = {n_ok, n_stale (REPLAY + SUPERSEDED), n_badauth, n_skipped (NOPEER + BADDESC)}.
 *   wg_hs_respond(inits = fresh, n_inits = &summary->n_ok) then runs as it always has; its sessions' `init` field,
 *   and so wg_hs_install's position p, is now the position in FRESH: the host's local_index, send_slot and recv_slot
 *   arrays are by that position. n = 0 is a no-op. Without a private key: WG_ENOKEY. flags or _reserved not 0:
 *   WG_EINVAL. n or n_rec above 2^30: WG_E2BIG. inits, records, shared, fresh: 16-byte aligned; summary: 8; the
 *   others: 4. An output that overlaps another output or an input: WG_EINVAL.
 *
 * State. Each peer of wg_hs_peers_set's table has 12 bytes of stored timestamp and the selection's scratch words,
 *   behind a header at a fixed device address: a captured wg_hs_stamp survives a change of the table without
 *   re-capture. The state is allocated at the first wg_hs_stamp / wg_hs_stamps_set / wg_hs_stamps_get; a context that
 *   never stamps pays nothing. A capturing stream cannot allocate: the first wg_hs_stamp there is WG_EINVAL, and an
 *   earlier wg_hs_stamps_set(ctx, 0, 0, NULL), which is valid, is the way to allocate. wg_hs_peers_set resets every
 *   stamp to zero, as it does the psks, because positions are renumbered; wg_hs_static_set and wg_hs_key_set leave
 *   them alone. Scratch (16 bytes per entry: T and a state, never k or ck, which do not leave the registers) is
 *   sized by wg_hs_reserve once the state exists, and the state starts with what was reserved before; a call that
 *   needs more allocates it, except on a capturing stream (WG_EINVAL: reserve first). wg_ctx_destroy wipes it.
 *
 * wg_hs_stamps_set / wg_hs_stamps_get(ctx, first_peer, n, stamps): the stored timestamps of peers [first_peer,
 *   first_peer + n), 12 bytes each (host pointer), as wg_hs_stamp's `opened` holds them. Synchronous, and ordered
 *   after everything queued before them, like wg_hs_psks_set. A range past the table's count: WG_ERANGE. A host
 *   saves the stamps with get and restores them with set across a restart; until it has, every captured initiation
 *   of the last 2^64 seconds is fresh again.
 *
 * Ordering and graphs. Calls on different streams of one context are ordered by the library (they share the stamps
 *   and the scratch). Seven launches (chain; three of the selection: a 64-bit atomicMax of T's high 8 bytes, a 32-bit
 *   atomicMax of the low 4 among those that tie, an atomicMin of j among those that still tie; commit; scan; emit),
 *   whose boundaries give the order: no workgroup waits on another. Every scratch word is written before it is read
 *   in each call and nothing about a call lives on the host, so a captured plan + check + dh + open + stamp +
 *   respond + install replays; a replay over the same ring finds every timestamp stale, wg_hs_respond answers
 *   nothing and consumes no ephemeral. One entry per lane; no branch, address or loop bound depends on ss, ss_p, ck
 *   or k. T of an authentic message, the tag's outcome, p and r are public. */
#define WG_HS_TS_OK 0u
#define WG_HS_TS_REPLAY 1u     /* not greater than the peer's stored timestamp */
#define WG_HS_TS_SUPERSEDED 2u /* another authentic entry of this peer in the call is newer, or as new and lower */
#define WG_HS_TS_BADAUTH 3u
#define WG_HS_TS_NOPEER 4u     /* inits[j].peer == WG_HS_NOPEER: no static-static secret on the device */
#define WG_HS_TS_BADDESC 5u    /* peer >= the table's count, record >= n_rec, or records[record].len != 148 */
typedef struct wg_hs_stamp_summary {
  uint32_t n_ok, n_stale /* REPLAY + SUPERSEDED */, n_badauth, n_skipped /* NOPEER + BADDESC */;
} wg_hs_stamp_summary;
typedef struct wg_hs_stamp_batch {
  const wg_hs_init* inits;      /* device, 16-byte aligned: wg_hs_open's entries */
  const uint32_t* n_inits;      /* device: &wg_hs_open_summary.n_emitted; NULL: all n */
  const wg_hs_record* records;  /* device, 16-byte aligned: the records wg_hs_open read (n_rec entries) */
  const uint8_t* shared;        /* device, 16-byte aligned, 32 n_rec bytes: wg_hs_dh's */
  uint32_t* ts_status;          /* device, n entries, WG_HS_TS_* */
  uint8_t* opened;              /* device, 4-byte aligned, 12 n bytes, by position j */
  wg_hs_init* fresh;            /* device, 16-byte aligned, n entries: what wg_hs_respond takes */
  wg_hs_stamp_summary* summary; /* device, 16 bytes, 8-byte aligned */
  uint32_t n, n_rec, flags /* must be 0 */, _reserved;
} wg_hs_stamp_batch;
int wg_hs_stamp(wg_ctx* ctx, const wg_hs_stamp_batch* batch, void* stream);
int wg_hs_stamps_set(wg_ctx* ctx, uint32_t first_peer, uint32_t n, const uint8_t* stamps_host /* 12 n bytes */);
int wg_hs_stamps_get(wg_ctx* ctx, uint32_t first_peer, uint32_t n, uint8_t* stamps_host /* 12 n bytes */);

/* ---- cookie replies and mac2 under load, on the device ----
 * mac1 needs only our public key, and wg_hs_stamp stops captured initiations, not fresh ones: a sender that never
 * proved it owns its source address still costs a ladder and the open chain per message. WireGuard's answer is the
 * cookie. A responder under load answers a valid-mac1 message whose mac2 does not verify with a 64-byte type-3
 * reply that carries a MAC of the sender's source address, sealed so that only the sender of THAT message can open
 * it; the sender repeats its message with mac2 keyed by the cookie, and only then is the ladder spent. The reference
 * has none of this (IncomingInitiation.java:38-40), wg_hs_check keeps the reference's rule (mac2 all zero) bit for
 * bit, and these calls are what the library ADDS, as it added wg_hs_stamp. With MAC(k, m) = BLAKE2s-128 keyed with
 * k, and H = BLAKE2s-256:
 *     Kc(P)       = H("cookie--" || P)                          for a static public key P (one compression)
 *     cookie(src) = MAC(secret, A)      A = addr[0 .. 4) || port (family 4, 6 bytes), addr[0 .. 16) || port (family 6,
 *                                       18 bytes); the port's 2 bytes in network order
 *     mac2        = MAC(cookie, msg[0 .. L - 16))                the 16-byte cookie is the key
 *     XAEAD(K, nonce24, pt, aad): sub = HChaCha20(K, nonce24[0 .. 16)) (the 20 ChaCha rounds over {constants, K,
 *                   nonce16} without the final addition; state words 0-3 and 12-15), then RFC 8439
 *                   ChaCha20-Poly1305 under sub with the nonce 0^4 || nonce24[16 .. 24)
 *                   (draft-irtf-cfrg-xchacha-03). Here pt is the 16-byte cookie and aad the message's 16-byte mac1.
 *     reply (64 B) = {3, 0,0,0, receiver = the message's sender index msg[4 .. 8), nonce[24],
 *                     XAEAD(Kc(the replier's static public key), nonce, cookie, aad = msg's mac1)[32]}
 *
 * wg_hs_cookie_secret_set(ctx, secret): the responder's 32-byte secret (host pointer), from the host's CSPRNG. The
 *   host rotates it by its own clock (WireGuard: every 120 s); the library has no clock. Synchronous, and ordered
 *   after everything queued before it. The secret sits at a device address that is fixed for the life of the
 *   context: a captured admit sees a new secret without re-capture. wg_ctx_destroy wipes it. Kc(local static public
 *   key) is derived on the device by wg_hs_key_set (and wg_hs_static_set), in the launch that derives the mac1 key.
 *
 * wg_hs_admit(ctx, b, stream): wg_hs_check under load. b->hs is a wg_hs_batch with the same meaning of every field.
 *   src: n entries BY BATCH INDEX (8-byte aligned); nonces: 24 bytes per LIST POSITION, fresh from the host's CSPRNG
 *   (16-byte aligned), input AND output; replies: n entries (16-byte aligned); admit_summary: 8-byte aligned. For
 *   list position k with i = list[k], steps 1-4 are those of wg_hs_check (bounds, type, exact size, mac1). Then:
 *   5. src[i].family is neither 4 nor 6: WG_HS_BADSRC.
 *   6. msg[L - 16 .. L) == MAC(cookie(src[i]), msg[0 .. L - 16)): WG_HS_OK. All 16 bytes are compared, without an
 *      early exit.
 *   7. the 24 nonce bytes of position k are all zero: WG_HS_NONONCE; no reply is written.
 *   8. WG_HS_NEEDCOOKIE: a reply is emitted, and the 24 nonce bytes of position k are overwritten with zeros.
 *   A message with an all-zero mac2 lands in 7 or 8. hs_status, records and summary are as in wg_hs_check: records is
 *   the stable compaction of the WG_HS_OK messages and n_rejected counts every other position, NEEDCOOKIE included;
 *   wg_hs_dh and the rest of the chain run on records unchanged (they never read the MAC fields). replies[0 ..
 *   n_replies) is the stable compaction, in list order, of the NEEDCOOKIE positions: {index = i, len = 64, msg,
 *   _pad = 0}; every byte of a written entry is defined and nothing behind n_replies entries is touched.
 *   admit_summary = {n_replies, n_mac2_ok (= n_valid), n_nononce, n_badsrc}. A consumed nonce is zeroed, as
 *   wg_hs_initiate zeroes its ephemerals: a replayed graph without fresh nonces sends no reply (every position that
 *   needs a cookie answers NONONCE), so a nonce is never used twice under one key. n = 0 writes only the two
 *   summaries (zeros). Without a mac1 key or without a secret: WG_ENOKEY. An output (hs_status, records, summary,
 *   nonces, replies, admit_summary) that overlaps another output or an input: WG_EINVAL. Limits, alignment and
 *   scratch follow wg_hs_check: wg_hs_reserve sizes the scratch, and a capturing stream that would have to allocate
 *   gets WG_EINVAL. Four launches (admit, two scans, emit; the emit seals the replies), no wait between workgroups,
 *   nothing about a call on the host: a captured plan + admit replays. Streams of one context are ordered by the
 *   library. Lanes whose mac1 failed (public) skip the cookie and mac2 work.
 *
 * wg_hs_cookie_open(ctx, b, stream): the initiator's side. The call scans all n datagrams of the ring itself (the
 *   plan does not list type 3). sent: wg_hs_initiate's records, aligned by position with pending (n_pending entries
 *   each); pending is READ ONLY here. For datagram i, o = pkt_off[i], wl = pkt_len[i], in this order:
 *   1. wl == 0, o > wire_size or wl > wire_size - o: WG_HS_CK_BADLEN. 2. wire[o] != 3: WG_HS_CK_SKIPPED. 3. wl != 64:
 *   WG_HS_CK_BADLEN. 4. no live pending entry (state == 1 and peer below the table's count) has local_index ==
 *   msg[4 .. 8): WG_HS_CK_NOPENDING; the lowest position wins a shared index (wg_hs_finish's lookup table, built by
 *   the call's first two launches). 5. the XAEAD open under Kc(the peer's static public key) with aad =
 *   sent[p].msg[116 .. 132) fails (all 16 tag bytes compared): WG_HS_CK_BADAUTH, and nothing changes. 6.
 *   WG_HS_CK_OK: the 16 opened bytes become the peer's cookie. ck_status[n] is by batch index; learned[0 .. n_ok) is
 *   the stable compaction of the OK datagrams, {index = i, pending = p, peer, 0}; summary = {n_ok, n_nopending,
 *   n_badauth, n_skipped}. Two OK replies for one peer in one ring: the one with the lowest batch index is stored,
 *   whatever the dispatch order (an atomicMin per peer, read one launch later). A pending entry is never consumed or
 *   altered: the handshake goes on with a retransmission. n = 0 is a no-op. Without a private key: WG_ENOKEY. n above 2^30 or
 *   n_pending above 2^28: WG_E2BIG. learned: 16-byte aligned; summary: 8; ck_status: 4. An output that overlaps
 *   another output or an input: WG_EINVAL. Scratch as wg_hs_finish (wg_hs_reserve(max(n, n_pending))); it holds the
 *   opened cookies for the time of the call. Five launches (fill, insert, open, scan, emit).
 *
 * The cookie table: one {cookie[16], have} per position of wg_hs_peers_set's table, on the device behind a header at
 *   a fixed address. wg_hs_cookies_get / wg_hs_cookies_set(ctx, first_peer, n, cookies_host (16 n bytes), have_host
 *   (n bytes)) read and write it; both synchronous and ordered after everything queued before them; a range past the
 *   table's count: WG_ERANGE. have = 0 clears an entry (its cookie bytes are stored as zeros): the host expires a
 *   cookie after 120 s by its own clock. A new peer table clears every cookie, as it resets every psk.
 *   wg_ctx_destroy wipes the table.
 *
 * wg_hs_mac2(ctx, b, stream): after wg_hs_initiate, or over stored records before a retransmission. records is input
 *   AND output; peer[k] is record k's position in the peer table. For every k < n, in this order: 1. records[k].len is
 *   neither 148 nor 92: WG_HS_MAC2_BADDESC. 2. peer[k] >= the table's count: WG_HS_MAC2_BADPEER. 3. the peer holds no
 *   cookie: WG_HS_MAC2_NONE; the record is untouched. 4. WG_HS_MAC2_OK: msg[L - 16 .. L) = MAC(cookie, msg[0 ..
 *   L - 16)), exactly those 16 bytes. summary = {n_ok, n_none, n_bad (BADDESC + BADPEER), 0}. n = 0 is a no-op. n above
 *   2^30: WG_E2BIG. records: 16-byte aligned; summary: 8; the others: 4. Two launches (mac2, scan). A captured
 *   initiate + mac2 replays and follows the table without re-capture.
 *
 * For all of these calls, no branch, address or loop bound depends on the secret, a cookie, a cookie key, a subkey or
 *   a keystream byte; the one exception is the all-zero test of a raw nonce. Source addresses, indices, peer
 *   positions and the statuses (the comparisons' outcomes among them) are public. Not here: the "under load"
 *   decision (the host chooses wg_hs_check or wg_hs_admit per ring; the rate limiter that goes with it is
 *   wg_hs_ratelimit, below), expiry and rotation (the host's clock, through the setters), mac2 inside
 *   wg_hs_respond's sessions (wg_hs_mac2 takes 92-byte records if the host copies them), and type 3 in
 *   wg_rx_plan's lists. */
#define WG_HS_BADSRC 5u     /* wg_hs_admit: src.family is neither 4 nor 6 */
#define WG_HS_NONONCE 6u    /* wg_hs_admit: a cookie is needed and the position's nonce is all zero */
#define WG_HS_NEEDCOOKIE 7u /* wg_hs_admit: mac2 does not verify; a cookie reply was emitted */
#define WG_HS_COOKIE_SIZE 64u
#define WG_HS_CK_OK 0u
#define WG_HS_CK_NOPENDING 1u /* no live pending entry has the reply's receiver index */
#define WG_HS_CK_BADAUTH 2u
#define WG_HS_CK_SKIPPED 3u /* not a type-3 datagram */
#define WG_HS_CK_BADLEN 4u  /* datagram out of bounds, or a type-3 datagram that is not 64 bytes */
#define WG_HS_MAC2_OK 0u
#define WG_HS_MAC2_NONE 1u    /* the peer holds no cookie */
#define WG_HS_MAC2_BADDESC 2u /* the record's len is neither 148 nor 92 */
#define WG_HS_MAC2_BADPEER 3u /* peer[k] is not a position in the peer table */
typedef struct wg_hs_src { /* 24 bytes; by batch index, filled by the host's receive loop */
  uint8_t addr[16];        /* IPv4 in addr[0..4) */
  uint8_t port[2];         /* network order */
  uint8_t family;          /* 4 or 6 */
  uint8_t _pad[5];
} wg_hs_src;
typedef struct wg_hs_cookie_reply { /* 80 bytes */
  uint32_t index;                   /* batch index of the datagram it answers */
  uint32_t len;                     /* 64 */
  uint8_t msg[64];
  uint32_t _pad[2];
} wg_hs_cookie_reply;
typedef struct wg_hs_admit_summary {
  uint32_t n_replies, n_mac2_ok, n_nononce, n_badsrc;
} wg_hs_admit_summary;
typedef struct wg_hs_admit_batch {
  wg_hs_batch hs;                     /* as wg_hs_check takes it */
  const wg_hs_src* src;               /* device, 8-byte aligned, n entries, by batch index */
  uint8_t* nonces;                    /* device, 16-byte aligned, n * 24 bytes, by list position; in and out */
  wg_hs_cookie_reply* replies;        /* device, 16-byte aligned, n entries */
  wg_hs_admit_summary* admit_summary; /* device, 16 bytes, 8-byte aligned */
} wg_hs_admit_batch;
typedef struct wg_hs_learned { /* 16 bytes */
  uint32_t index;              /* batch index of the reply's datagram */
  uint32_t pending;            /* position in pending (and in sent) */
  uint32_t peer;
  uint32_t _zero;
} wg_hs_learned;
typedef struct wg_hs_cookie_open_summary {
  uint32_t n_ok, n_nopending, n_badauth, n_skipped;
} wg_hs_cookie_open_summary;
typedef struct wg_hs_cookie_open_batch {
  const uint8_t* wire;                /* UDP ring (device) */
  uint64_t wire_size;
  const uint64_t* pkt_off;            /* device, n entries */
  const uint32_t* pkt_len;            /* device, n entries */
  const wg_hs_record* sent;           /* device, 16-byte aligned, n_pending entries: wg_hs_initiate's records */
  const wg_hs_pending* pending;       /* device, 16-byte aligned, n_pending entries; read only */
  uint32_t* ck_status;                /* device, n entries, WG_HS_CK_*, by batch index */
  wg_hs_learned* learned;             /* device, 16-byte aligned, n entries */
  wg_hs_cookie_open_summary* summary; /* device, 16 bytes, 8-byte aligned */
  uint32_t n, n_pending;
} wg_hs_cookie_open_batch;
typedef struct wg_hs_mac2_summary {
  uint32_t n_ok, n_none, n_bad /* BADDESC + BADPEER */, _zero;
} wg_hs_mac2_summary;
typedef struct wg_hs_mac2_batch {
  wg_hs_record* records;       /* device, 16-byte aligned, n entries; in and out */
  const uint32_t* peer;        /* device, n entries */
  uint32_t* mac2_status;       /* device, n entries, WG_HS_MAC2_* */
  wg_hs_mac2_summary* summary; /* device, 16 bytes, 8-byte aligned */
  uint32_t n, _reserved;
} wg_hs_mac2_batch;
int wg_hs_cookie_secret_set(wg_ctx* ctx, const uint8_t* secret /* 32 bytes */);
int wg_hs_admit(wg_ctx* ctx, const wg_hs_admit_batch* batch, void* stream);
int wg_hs_cookie_open(wg_ctx* ctx, const wg_hs_cookie_open_batch* batch, void* stream);
int wg_hs_cookies_get(wg_ctx* ctx, uint32_t first_peer, uint32_t n, uint8_t* cookies_host /* 16 n */, uint8_t* have_host /* n */);
int wg_hs_cookies_set(wg_ctx* ctx, uint32_t first_peer, uint32_t n, const uint8_t* cookies_host /* 16 n */,
                      const uint8_t* have_host /* n */);
int wg_hs_mac2(wg_ctx* ctx, const wg_hs_mac2_batch* batch, void* stream);

/* ---- handshakes rate-limited per source, on the device ----
 * wg_hs_admit stops a spoofed flood; a sender that owns its address completes one cookie round trip and then sends
 * fresh initiations with a valid mac2, each of which costs a ladder and the open chain. WireGuard's second half of
 * its under-load rule: a message with a valid cookie still has to pass a token bucket of its source before any curve
 * work is spent (20 handshakes per second, a burst of 5, keyed by the IPv4 address or the IPv6 /64). The reference
 * has no limiter; this is what the library ADDS, after wg_hs_stamp and wg_hs_admit, and no other call changes.
 *
 * The rule. A limiter is `cost` ticks per handshake and `burst` handshakes: max = burst * cost, 1 <= burst <=
 *   WG_HS_RL_MAX_BURST, 1 <= cost <= 2^56. The key of a source is {family, addr[0 .. 4)} (family 4) or {family,
 *   addr[0 .. 8)} (family 6): not the port, not the bytes of wg_hs_src.addr behind an IPv4 address, not the low 64
 *   bits of an IPv6 address. An entry is {key, tokens, last}. One record at tick `now`:
 *   1. the key has no entry: create {tokens = max, last = now}.  2. age = now >= last ? now - last : 0.
 *   3. tokens = min(max, tokens + age) (the sum saturates).  4. last = now only if now >= last (a clock that steps
 *   back ages nothing and moves nothing, like the session timers).  5. tokens >= cost: tokens -= cost, the record
 *   passes; otherwise WG_HS_RL_LIMITED.
 *   A call applies this to its records IN LIST ORDER, ALL AT ONE now, which has a closed form: a source with c records
 *   in the call has the allowance a = min(max, tokens + age) / cost; its min(a, c) records with the LOWEST positions
 *   pass, whatever the dispatch order, the others are LIMITED, and its entry ends as {refilled - min(a, c) * cost,
 *   max(last, now)}. An entry with now - last >= max is indistinguishable from no entry, so dropping such entries
 *   (the compaction below) only reclaims space WHILE THE CLOCK DOES NOT STEP BACK: after a step back a dropped
 *   entry would have kept its `last`, and its source gets a full bucket earlier than the sequential rule gives it.
 *
 * wg_hs_rl_reserve(ctx, max_sources): an open-addressing table of C buckets, C the smallest power of two >= max(8, 2 *
 *   max_sources), behind a header at a fixed device address, a second buffer of the same size for the compaction,
 *   and per bucket the call's scratch (a count and WG_HS_RL_MAX_BURST words); the per-record scratch is sized with
 *   wg_hs_reserve. The table never holds more than C / 2 entries. A smaller or equal max_sources later is a no-op,
 *   a larger one rebuilds the table with its entries kept. max_sources above 2^27: WG_E2BIG. Synchronous.
 * wg_hs_rl_config_set(ctx, cost, burst): synchronous and ordered after everything queued before it. Both values live
 *   on the device: a new cost needs no re-capture. A call runs `burst` selection launches, fixed when it is queued or
 *   captured: a captured call must be captured again after a GREATER burst (a smaller one replays correctly). Values
 *   out of range: WG_EINVAL.
 * wg_hs_ratelimit(ctx, b, stream): records are wg_hs_check's or wg_hs_admit's; n_records a device count
 *   (&wg_hs_summary.n_valid) or NULL (all n); src is the ring's wg_hs_src[n_src] by BATCH INDEX; now a device tick
 *   count (8-byte aligned). For every position k < min(*n_records, n), rl_status[k] is, in this order:
 *   1. WG_HS_RL_BADSRC: records[k].index >= n_src, or the source's family is neither 4 nor 6.
 *   2. WG_HS_RL_FULL: with U the entries of the table before the call and m the records of the call (records, not
 *      distinct sources) whose key has no entry before the call, U + m > C / 2: each of those m records is FULL and the
 *      call inserts nothing. Records of known sources are served as usual. (wg_hs_install's rule for a full table.)
 *   3. WG_HS_RL_LIMITED, by the rule above.   4. WG_HS_RL_OK.
 *   out_records[0 .. n_passed) is the stable compaction of the OK records, copied whole; nothing behind it is touched.
 *   rl_summary = {n_passed, n_limited, n_full, n_badsrc}: its first word is what wg_hs_dh_batch.n_records takes next.
 *   *now == 0 ("never", like the session timers): every record with a valid source passes and the table is neither
 *   read nor written. n = 0 writes only the summary. WG_HS_RL_COMPACT in flags: the call first drops the stale
 *   entries (wg_hs_rl_compact's launches) exactly when U + min(*n_records, n) > C / 2 and *now != 0. Without a
 *   reserve or a config: WG_ENOKEY. records, out_records: 16-byte aligned; src, now, rl_summary: 8; the others: 4.
 *   An output (rl_status, out_records, rl_summary) that overlaps another output or an input: WG_EINVAL. n above
 *   2^30: WG_E2BIG. A capturing stream that would have to allocate: WG_EINVAL. 7 + burst launches (+ 3 with
 *   WG_HS_RL_COMPACT), fixed by the call and the config and never by the data; no workgroup waits for another;
 *   nothing about a call lives on the host, so a captured admit + ratelimit + dh replays with only *now refreshed.
 *   Streams of one context are ordered by the library.
 * wg_hs_rl_compact(ctx, now, summary_dev, stream): rebuilds the table from the entries with (*now >= last ? *now -
 *   last : 0) < max into the second buffer and flips the header's pointer (as wg_rx_sessions_compact does).
 *   summary_dev (8-byte aligned, may be NULL) = {kept, dropped, 0, 0}. Three launches; capturable.
 * wg_hs_rl_dump(ctx, out_host, max_entries, &n_out): the table's entries in table order, 32 bytes each; *n_out is
 *   the table's count, of which the first min(count, max_entries) are written. wg_hs_rl_load(ctx, entries_host, n)
 *   REPLACES the table's content (save and restore; n above C / 2: WG_ERANGE; a repeated key, a family that is
 *   neither 4 nor 6, a non-zero pad byte or IPv4 tail: WG_EINVAL, nothing changes). wg_hs_rl_count(ctx, &used,
 *   &capacity). All three are synchronous and ordered after everything queued before them.
 * wg_ctx_destroy frees the table. Source addresses, statuses and bucket contents are public: nothing here touches a
 *   secret, and there is no constant-time claim to make. The probe's hash is not keyed: a sender that chooses its
 *   addresses can lengthen the walks of a table (never past C / 2 + 1 steps), not change an answer. */
#define WG_HS_RL_MAX_BURST 16u
#define WG_HS_RL_OK 0u
#define WG_HS_RL_LIMITED 1u /* the source's bucket holds less than cost */
#define WG_HS_RL_FULL 2u    /* an unknown source, and the table cannot take the call's unknown records */
#define WG_HS_RL_BADSRC 3u  /* index >= n_src, or src.family is neither 4 nor 6 */
#define WG_HS_RL_COMPACT 1u /* flags: drop the stale entries first if the call's records might not fit */
typedef struct wg_hs_rl_entry { /* 32 bytes */
  uint8_t addr[8];              /* the key's bytes: addr[0..4) and zeros (family 4), addr[0..8) (family 6) */
  uint8_t family;               /* 4 or 6 */
  uint8_t _pad[7];
  uint64_t tokens;
  uint64_t last;
} wg_hs_rl_entry;
typedef struct wg_hs_rl_summary {
  uint32_t n_passed, n_limited, n_full, n_badsrc;
} wg_hs_rl_summary;
typedef struct wg_hs_rl_compact_summary {
  uint32_t kept, dropped, _zero[2];
} wg_hs_rl_compact_summary;
typedef struct wg_hs_rl_batch {
  const wg_hs_record* records;  /* device, 16-byte aligned, n entries */
  const uint32_t* n_records;    /* device (&wg_hs_summary.n_valid), or NULL: all n */
  const wg_hs_src* src;         /* device, 8-byte aligned, n_src entries, by batch index */
  const uint64_t* now;          /* device, 8-byte aligned: the tick count */
  uint32_t* rl_status;          /* device, n entries, WG_HS_RL_*, by record position */
  wg_hs_record* out_records;    /* device, 16-byte aligned, n entries */
  wg_hs_rl_summary* rl_summary; /* device, 16 bytes, 8-byte aligned */
  uint32_t n, n_src;
  uint32_t flags;               /* WG_HS_RL_COMPACT */
  uint32_t _reserved;
} wg_hs_rl_batch;
int wg_hs_rl_reserve(wg_ctx* ctx, uint32_t max_sources);
int wg_hs_rl_config_set(wg_ctx* ctx, uint64_t cost, uint32_t burst);
int wg_hs_ratelimit(wg_ctx* ctx, const wg_hs_rl_batch* batch, void* stream);
int wg_hs_rl_compact(wg_ctx* ctx, const uint64_t* now_dev, wg_hs_rl_compact_summary* summary_dev, void* stream);
int wg_hs_rl_dump(wg_ctx* ctx, wg_hs_rl_entry* out_host, uint32_t max_entries, uint32_t* n_out);
int wg_hs_rl_load(wg_ctx* ctx, const wg_hs_rl_entry* entries_host, uint32_t n);
int wg_hs_rl_count(wg_ctx* ctx, uint32_t* used, uint32_t* capacity);

/* ---- handshake sessions installed on the device ----
 * What the reference does with a finished handshake (SessionManager.setSession: a new EstablishedSession around a
 * new SymmetricKeypair(send, recv), reachable under its local index through PeerList) for a ring of wg_hs_session
 * or wg_hs_established entries, without a key leaving the device: the next wg_tx_plan / wg_seal_batch(WG_F_FRAME)
 * and wg_rx_plan / wg_open_batch / wg_rx_check on the same stream already use the new sessions.
 *
 * wg_rx_sessions_reserve(ctx, max_sessions): gives the receiver-index table a fixed capacity C, the smallest power
 *   of two >= max(16, 4 max_sessions), of the context's own entries (a table that is empty too), and allocates the
 *   install's scratch (one word per key slot, four control words). Synchronous, like wg_rx_sessions_set; the
 *   table's current live entries are rebuilt into the new capacity and its retired entries are dropped.
 *   Afterwards wg_rx_sessions_set builds into max(C, the capacity of its own rule). A context that never
 *   reserves builds exactly the tables described above. max_sessions above 2^29: WG_E2BIG.
 *   The table's header gains `used`, the number of live + retired entries. A retired entry is {index,
 *   0xFFFFFFFF} in the same 8-byte format: a lookup walks over it (it is not empty) and never matches it. No
 *   key slot is 0xFFFFFFFE, so no table built by wg_rx_sessions_set holds one.
 * wg_rx_sessions_retire(ctx, indices_dev, n, n_retired_dev, stream): asynchronous on `stream`. Every index of
 *   the device array that is live in the table becomes a retired entry, by a 64-bit compare-and-swap on the
 *   entry, so equal indices in one call retire it once. *n_retired_dev (device, 4-byte aligned, may be NULL) =
 *   the number of entries the call retired. There is no per-position status: nothing depends on thread order.
 *   A retired index plans as WG_PKT_NOSESSION; the entries behind it in its probe sequence are still found.
 *   `used` does not fall: a rebuild (wg_rx_sessions_set, wg_rx_sessions_reserve) reclaims retired entries, and so
 *   does wg_rx_sessions_compact on the device ("the end of a session on the device", below).
 *   The keys are not touched: wg_keys_zero is the host's call, WG_TIMERS_WIPE the sweep's.
 * wg_rx_sessions_count(ctx, &live, &retired): synchronous, after everything queued on the device (either
 *   pointer may be NULL).
 *
 * wg_hs_install(ctx, b, stream): entries = wg_hs_respond's sessions (source WG_HS_INSTALL_SESSIONS, 176 B) or
 *   wg_hs_finish's established (WG_HS_INSTALL_ESTABLISHED, 96 B); n_entries a device pointer to their number
 *   (&wg_hs_respond_summary.n_ok / &wg_hs_finish_summary.n_ok; NULL: all n), read on the device. The position p of
 *   entry j is sessions[j].init or established[j].pending: the index under which the host chose local_index for
 *   that handshake. Under the same index it chooses, before it launches the chain, the entry's two key slots
 *   send_slot[p] and recv_slot[p] (n_slots entries each), so nothing is read back to pick slots. For every j <
 *   min(*n_entries, n), in this order, each step's test being against all entries that passed the steps before
 *   it, whether or not they pass later ones, and the lower j winning:
 *   1. WG_HS_INST_BADSLOT: p >= n_slots; or one of the two slots is outside [slot_first, slot_first + slot_count),
 *      the slot range this call may write, or >= the key table; or send_slot[p] == recv_slot[p].
 *   2. WG_HS_INST_DUPSLOT: a lower j that passed step 1 names one of this entry's slots, as send or as recv.
 *      (Two authentic responses to one pending entry, which wg_hs_finish emits both: the first is installed.)
 *   3. WG_HS_INST_DUPINDEX: local_index is live in the table at the call's start, or it is the local_index of a
 *      lower j that passed steps 1-2. A retired entry of that index does not count.
 *   4. WG_HS_INST_FULL, all or nothing: if used + (the entries that passed 1-3) > C / 2, every one of them is FULL
 *      and the table is unchanged. The table is thus never more than half full, which bounds every probe walk.
 *   5. WG_HS_INST_OK. keys[send_slot] = send_key, keys[recv_slot] = recv_key; the send counters of both slots
 *      become 0 and their replay windows empty (top, every window word), as after wg_keys_set; {local_index ->
 *      recv_slot} is inserted and `used` grows by one; receivers[send_slot] = remote_index when receivers (the
 *      table given to wg_ctx_set_receivers, >= key_slots entries) is not NULL; with WG_HS_INSTALL_WIPE the
 *      entry's 64 key bytes are zeroed. A refused entry keeps its keys: the host can fall back to wg_keys_set.
 *   inst_status[j] is written for the covered j and nothing behind them; nothing else of a refused entry is
 *   written. summary = {n_ok, n_badslot, n_dup (DUPSLOT + DUPINDEX), n_full}.
 *   n = 0 is a no-op. Without wg_rx_sessions_reserve: WG_EINVAL. Unknown flags or source, entries not 16-byte
 *   aligned (summary: 8; the others: 4), or an output (entries, inst_status, summary, receivers) that overlaps
 *   another output or an input: WG_EINVAL. n above 2^30: WG_E2BIG.
 *   Which of several equal slots or indices wins depends on no thread order: a launch over the claim words, one
 *   in which every entry leaves its position in its slots' words (atomicMin), one that places transient table
 *   entries {index, 0x80000000 | j} (compare-and-swap to claim a bucket, atomicMin on the position), one that
 *   counts the entries that passed steps 1-3, and the commit, with one workgroup per entry (the window clear is
 *   up to 8 KiB per slot). Kernel boundaries order them; no workgroup waits for another. Every scratch word is
 *   written before it is read in each call and nothing about a call lives on the host, so a captured ... ->
 *   wg_hs_respond -> wg_hs_install replays; the host refreshes ephemerals, local_index and the two slot arrays in
 *   place between replays. The scratch holds positions only, never key bytes. A ring with more new indices than
 *   the table has empty buckets is handled (all FULL), but slowly: reserve for the sessions you mean to hold.
 *   Constant time: keys move by straight copies (load, store, zero); no branch, address or loop bound depends on
 *   a key byte. Slots, indices and positions are public.
 *   The host's copy of a key. wg_seal1 / wg_open1 and the queues (wg_submit_*) seal with the host's mirror of the
 *   key table, which a device install cannot update. The call therefore marks the mirror of every slot of
 *   [slot_first, slot_first + slot_count) as holding no key, when it is made (or captured): those paths then
 *   return WG_ENOKEY on such a slot instead of sealing under a stale key, until a later wg_keys_set on the slot,
 *   which works as before. Device-installed slots are batch-path only.
 *   Ordering. The call waits for, and is waited for by, the receive plans, the replay checks (if a window is
 *   enabled) and the transmit plans (if the transmit state exists) of every stream. Send counters or windows that
 *   do not exist when the call is made or captured are not reset (they start at zero when they are created); a
 *   captured install holds the windows' addresses, so enabling a larger window afterwards needs a new capture. The
 *   key table itself has no ordering with seals and opens on other streams, today or with this call: install on
 *   the stream that seals and opens next, or synchronise. */
#define WG_HS_INST_OK 0u
#define WG_HS_INST_BADSLOT 1u  /* position or slot out of range, or send slot == recv slot */
#define WG_HS_INST_DUPSLOT 2u  /* a lower entry names one of the slots */
#define WG_HS_INST_DUPINDEX 3u /* local_index is live in the table, or a lower entry's */
#define WG_HS_INST_FULL 4u     /* the call's new entries would fill the table past C / 2: none is installed */
#define WG_HS_INSTALL_SESSIONS 0u    /* source: wg_hs_session[] */
#define WG_HS_INSTALL_ESTABLISHED 1u /* source: wg_hs_established[] */
#define WG_HS_INSTALL_WIPE 1u        /* flags: zero an installed entry's send_key and recv_key */
#define WG_HS_INSTALL_COMPACT 4u     /* flags: compact the table first if the ring would not fit ("the end of a session on
                                        the device"). 4, not 2: flags == 2 and 0x80000001 stay WG_EINVAL */
typedef struct wg_hs_install_summary {
  uint32_t n_ok, n_badslot, n_dup, n_full;
} wg_hs_install_summary;
typedef struct wg_hs_install_batch {
  void* entries;             /* device, 16-byte aligned: wg_hs_session[] or wg_hs_established[]; in and out with WIPE */
  const uint32_t* n_entries; /* device: &wg_hs_respond_summary.n_ok / &wg_hs_finish_summary.n_ok; NULL: all n */
  const uint32_t* send_slot; /* device, n_slots entries, by position */
  const uint32_t* recv_slot; /* device, n_slots entries */
  uint32_t* receivers;       /* device, >= key_slots entries (the table of wg_ctx_set_receivers), or NULL */
  uint32_t* inst_status;     /* device, n entries, WG_HS_INST_* */
  wg_hs_install_summary* summary; /* device, 16 bytes, 8-byte aligned */
  uint32_t n, n_slots;
  uint32_t slot_first, slot_count; /* the device-owned slot range of this call */
  uint32_t source;           /* WG_HS_INSTALL_SESSIONS or WG_HS_INSTALL_ESTABLISHED */
  uint32_t flags;            /* WG_HS_INSTALL_WIPE | WG_HS_INSTALL_COMPACT */
} wg_hs_install_batch;
int wg_rx_sessions_reserve(wg_ctx* ctx, uint32_t max_sessions);
int wg_rx_sessions_retire(wg_ctx* ctx, const uint32_t* indices_dev, uint32_t n, uint32_t* n_retired_dev, void* stream);
int wg_rx_sessions_count(wg_ctx* ctx, uint32_t* live, uint32_t* retired);
int wg_hs_install(wg_ctx* ctx, const wg_hs_install_batch* batch, void* stream);

/* ---- session timers on the device ----
 * The lifetime of the installed sessions: when a session stops being used (EstablishedSession.isExpired,
 * EstablishedSession.java:28,:114), to whom the node initiates again (SessionManager.sessionInitiationThread,
 * SessionManager.java:92-111; the retry after 5 s, :188) and when a keepalive is due (KeepaliveSender.java:29-85).
 * The reference runs one thread per peer against the wall clock; here the host supplies a clock value and nothing
 * per packet or per session, and a captured receive chain, transmit chain and tick replay with only `now` refreshed
 * in place. A context that never calls wg_timers_* allocates nothing and behaves exactly as before.
 *
 * Time is a 64-bit tick count in a unit the host chooses, read on the device from `now` (device memory, 8-byte
 * aligned) when a call runs. Tick 0 means "never": a call that reads *now == 0 changes no state, writes a zero
 * summary (and, the sweep, an initiate list of padding only). An age is now >= t ? now - t : 0, so a clock that steps
 * back ages nothing. The library has no clock of its own.
 *
 * State (wg_timers_reserve(ctx, max_peers); synchronous; it also creates the transmit state and reserves the
 * sweep's scratch, so every call below can be captured; a second call with max_peers not above the first is a no-op,
 * a larger one is WG_EINVAL: the state does not grow; max_peers above 2^30: WG_E2BIG):
 *   per key slot a wg_timer_slot {state, peer, local_index, partner, born, last, last_data, superseded}. A session is
 *     two records, the send slot's (state SEND_INITIATOR or SEND_RESPONDER) and the recv slot's (RECV), each naming
 *     the other as `partner`. born: the tick of wg_timers_start. last: the last packet sent (send record) or
 *     authenticated (recv record); last_data: the last one that was not a keepalive. superseded (send record): the
 *     tick at which a newer session of the same peer became the peer's current one, 0: not superseded. It lives in
 *     the session's own record because several superseded sessions of one peer can linger at once. DEAD: the session
 *     was retired by the sweep or its other slot was taken by a newer session.
 *   per peer (position in wg_hs_peers_set's table) a wg_timer_peer_state {current, flags, keepalive_interval,
 *     rekey_listed}: current = the send slot of the session the peer transmits on (WG_TIMER_NOSLOT: none),
 *     rekey_listed = the tick at which the sweep last listed the peer for initiation.
 *   the configuration, a wg_timers_config at a fixed device address: a captured call sees a new configuration
 *     without re-capture. Every field is a uint64, 0 = off: rekey_after_time, reject_after_time, rekey_timeout,
 *     keepalive_timeout, linger, rekey_after_messages, reject_after_messages; flags: WG_TIMERS_INITIATOR_ONLY.
 * wg_timers_config_set, wg_timers_peers_set (keepalive_interval and flags: WG_TIMER_PEER_CAN_INITIATE; a peer's
 *   current and rekey_listed are kept), wg_timers_get and wg_timers_peers_get (host pointers) are synchronous and
 *   ordered after everything queued on the device, like wg_tx_counters_get. Before wg_timers_reserve: WG_EINVAL; a
 *   range past the key table / max_peers: WG_ERANGE. wg_ctx_destroy frees the state.
 *
 * The four calls are asynchronous on `stream` and capturable; each writes every output word it covers and nothing
 * behind it, and depends on no thread order. They wait for, and are waited for by, each other on every stream.
 *
 * wg_timers_start(ctx, b, stream): after wg_hs_install on the same stream, with the install's own arrays. For every
 *   j < min(*n_entries, n) with inst_status[j] == WG_HS_INST_OK (and, checked again, position < n_slots, both slots
 *   inside the key table and different): the send slot's record = {SEND_INITIATOR for WG_HS_INSTALL_ESTABLISHED,
 *   SEND_RESPONDER for WG_HS_INSTALL_SESSIONS; peer; local_index; partner = recv slot; born = now; 0; 0; superseded},
 *   the recv slot's = {RECV, peer, local_index, partner = send slot, born = now, 0, 0, 0}. It reads position, peer
 *   and local_index only, which WG_HS_INSTALL_WIPE leaves in place. A live session that owned either slot before
 *   is killed first: its other record becomes DEAD, and the peer whose current it was has none. The session becomes
 *   its peer's current and the previous current is superseded at `now`; of several OK entries of one peer in one
 *   call the lowest j becomes current and the others start superseded at `now`. A peer at or past max_peers: the
 *   records carry WG_HS_NOPEER; such a session can expire but is never rekeyed or kept alive. Three launches (the
 *   peers' claim words = none; kill, and atomicMin of j on the peer's claim word; write), ordered by kernel
 *   boundaries. n = 0 is a no-op.
 *
 * wg_timers_mark(ctx, b, stream): the per-packet part, over n descriptors and their statuses.
 *   WG_TIMERS_RX, after wg_rx_deliver with its desc and final_status: WG_PKT_OK raises last and last_data of the
 *     descriptor's key slot to now, WG_PKT_KEEPALIVE raises last only; only a RECV record is marked.
 *   WG_TIMERS_TX, between wg_tx_plan and wg_seal_batch with desc_out and tx_status: a WG_PKT_OK descriptor raises
 *     last of its key slot, and last_data if len > 0; only a live SEND record is marked. With WG_TIMERS_GATE a
 *     WG_PKT_OK descriptor whose slot lies in [slot_first, slot_first + slot_count) is refused when the slot holds
 *     no live SEND record (a slot past the key table holds none), or reject_after_time is set and the session's age
 *     has reached it, or reject_after_messages is set and desc.counter has reached it: status = WG_PKT_NOSESSION,
 *     len = WG_LEN_INVALID, so the seal and the framer skip it, and nothing is marked. Its claimed counter is lost,
 *     which is harmless. Transmission on an old session thus stops at the packet, not at the next tick.
 *   A raise is a 64-bit atomic maximum: marks on streams with different clocks cannot move a stamp back. Slots
 *   outside the key table, records of any other state and every other status are ignored. summary = {n_marked,
 *   n_refused}. desc and status are in and out in TX direction with the gate, inputs otherwise. n = 0 writes a
 *   zero summary.
 *
 * wg_timers_sweep(ctx, b, stream): the tick, over every slot record and every peer record. Three lists, each with a
 *   capacity; what does not fit is neither listed nor changed and stays due. A session (a live SEND record) is
 *   EXPIRED when reject_after_time is set and its age has reached it, or reject_after_messages is set and its send
 *   counter has reached it, or linger is set and it was superseded linger or more ticks ago.
 *   expired[0 .. n_expired): the expired sessions in ascending send-slot order, {send_slot, recv_slot, peer,
 *     local_index}. With WG_TIMERS_RETIRE each listed session's local_index is retired in the receiver-index table
 *     (the compare-and-swap of wg_rx_sessions_retire), both records become DEAD, and the peer whose current it was
 *     has none. Without the flag it is listed at every sweep. An expired session is listed for nothing else.
 *   initiate[0 .. n_initiate): in ascending order the peers that have WG_TIMER_PEER_CAN_INITIATE, and no current
 *     session or an expired one (whether or not this sweep's list had room to retire it), or one whose age has
 *     reached rekey_after_time or whose send counter has reached rekey_after_messages and, under
 *     WG_TIMERS_INITIATOR_ONLY, that we initiated; and rekey_listed == 0 or now - rekey_listed >= rekey_timeout.
 *     rekey_listed = now for a listed peer. initiate[n_initiate .. initiate_cap) = 0xFFFFFFFF, so a captured
 *     wg_hs_initiate over the whole capacity answers them WG_HS_INIT_BADPEER and consumes no ephemeral.
 *   keepalives[0 .. n_keepalive): in ascending send-slot order, for sessions that are their peer's current and not
 *     expired. Persistent: the peer's keepalive_interval > 0 and the send record's last == 0 (KeepaliveSender.java:
 *     69-73 sends one as soon as the session changes) or now - last >= interval. Passive: keepalive_timeout > 0, the
 *     recv record's last_data > the send record's last (equal ticks count as answered) and now - last_data >=
 *     keepalive_timeout. Entry j = {in_off = 0, out_off = wire_base + j * wire_stride + 16, counter = send[slot], len
 *     = 0, key_slot = slot}; then send[slot] += 1 and last = now. wg_seal_batch(keepalives, n_keepalive, ...,
 *     WG_F_FRAME) sends them, in route mode too. Wire slots that overrun out_size (counted as wg_tx_plan counts
 *     them; wire_stride < 32: none fits) lower the capacity. keepalives[n_keepalive .. keepalive_cap) = {0, 0, 0,
 *     WG_LEN_INVALID, 0}, which the seal and the framer skip: a captured seal over the whole capacity sends exactly
 *     the listed ones, so a tick -> seal chain replays with no read-back either.
 *   summary = {n_expired_due, n_expired, n_initiate_due, n_initiate, n_keepalive_due, n_keepalive, n_live (sessions
 *   alive after the sweep), 0}. The call waits for, and is waited for by, the transmit plans, and with
 *   WG_TIMERS_RETIRE the receive plans, of every stream. Three launches: every record's verdict and one 16-byte
 *   record {expired, live, initiate, keepalive} per 256 positions (position i is key slot i and peer i; a peer's
 *   verdict tests its current session's expiry itself, so it waits for no slot's), their prefixes, the placing. */
#define WG_TIMER_NONE 0u
#define WG_TIMER_SEND_INITIATOR 1u
#define WG_TIMER_SEND_RESPONDER 2u
#define WG_TIMER_RECV 3u
#define WG_TIMER_DEAD 4u
#define WG_TIMER_NOSLOT 0xFFFFFFFFu
#define WG_TIMERS_INITIATOR_ONLY 1u   /* wg_timers_config.flags */
#define WG_TIMER_PEER_CAN_INITIATE 1u /* wg_timer_peer.flags */
#define WG_TIMERS_RX 0u               /* wg_timers_mark_batch.dir */
#define WG_TIMERS_TX 1u
#define WG_TIMERS_GATE 1u             /* wg_timers_mark_batch.flags */
#define WG_TIMERS_RETIRE 1u           /* wg_timers_sweep_batch.flags */
#define WG_TIMERS_WIPE 2u             /* wg_timers_sweep_batch.flags, with RETIRE only: zero the retired sessions' keys */
typedef struct wg_timers_config { /* 64 bytes; 0 = off */
  uint64_t rekey_after_time, reject_after_time, rekey_timeout, keepalive_timeout, linger;
  uint64_t rekey_after_messages, reject_after_messages;
  uint64_t flags; /* WG_TIMERS_INITIATOR_ONLY */
} wg_timers_config;
typedef struct wg_timer_slot { /* 48 bytes */
  uint32_t state, peer, local_index, partner;
  uint64_t born, last, last_data, superseded;
} wg_timer_slot;
typedef struct wg_timer_peer { /* 16 bytes */
  uint64_t keepalive_interval;
  uint32_t flags; /* WG_TIMER_PEER_CAN_INITIATE */
  uint32_t _zero;
} wg_timer_peer;
typedef struct wg_timer_peer_state { /* 24 bytes */
  uint32_t current; /* send slot, or WG_TIMER_NOSLOT */
  uint32_t flags;
  uint64_t keepalive_interval, rekey_listed;
} wg_timer_peer_state;
typedef struct wg_timer_expired { /* 16 bytes */
  uint32_t send_slot, recv_slot, peer, local_index;
} wg_timer_expired;
typedef struct wg_timers_start_batch {
  const void* entries;         /* device: the install's entries */
  const uint32_t* n_entries;   /* device, or NULL: all n */
  const uint32_t* inst_status; /* device, n entries: the install's */
  const uint32_t* send_slot;   /* device, n_slots entries */
  const uint32_t* recv_slot;   /* device, n_slots entries */
  const uint64_t* now;         /* device, 8-byte aligned */
  uint32_t n, n_slots;
  uint32_t source;             /* WG_HS_INSTALL_SESSIONS or WG_HS_INSTALL_ESTABLISHED */
  uint32_t _reserved;
} wg_timers_start_batch;
typedef struct wg_timers_mark_summary {
  uint32_t n_marked, n_refused;
} wg_timers_mark_summary;
typedef struct wg_timers_mark_batch {
  wg_pkt* desc;                    /* device, 16-byte aligned, n entries; in and out with WG_TIMERS_GATE */
  uint32_t* status;                /* device, n entries: final_status / tx_status; in and out with WG_TIMERS_GATE */
  const uint64_t* now;             /* device, 8-byte aligned */
  wg_timers_mark_summary* summary; /* device, 8 bytes, 8-byte aligned */
  uint32_t n;
  uint32_t dir;                    /* WG_TIMERS_RX or WG_TIMERS_TX */
  uint32_t flags;                  /* WG_TIMERS_GATE (TX only) */
  uint32_t slot_first, slot_count; /* the gated key slots */
  uint32_t _reserved;
} wg_timers_mark_batch;
typedef struct wg_timers_sweep_summary {
  uint32_t n_expired_due, n_expired, n_initiate_due, n_initiate, n_keepalive_due, n_keepalive, n_live, _zero;
} wg_timers_sweep_summary;
typedef struct wg_timers_sweep_batch {
  const uint64_t* now;              /* device, 8-byte aligned */
  wg_timer_expired* expired;        /* device, 16-byte aligned, expired_cap entries */
  uint32_t* initiate;               /* device, initiate_cap entries: wg_hs_initiate_batch.peer */
  wg_pkt* keepalives;               /* device, 16-byte aligned, keepalive_cap entries */
  wg_timers_sweep_summary* summary; /* device, 32 bytes, 8-byte aligned */
  uint64_t wire_base, wire_stride, out_size; /* the keepalives' wire slots, as in wg_tx_batch */
  uint32_t expired_cap, initiate_cap, keepalive_cap;
  uint32_t flags;                   /* WG_TIMERS_RETIRE | WG_TIMERS_WIPE */
} wg_timers_sweep_batch;
int wg_timers_reserve(wg_ctx* ctx, uint32_t max_peers);
int wg_timers_config_set(wg_ctx* ctx, const wg_timers_config* config);
int wg_timers_peers_set(wg_ctx* ctx, uint32_t first_peer, uint32_t n, const wg_timer_peer* peers_host);
int wg_timers_get(wg_ctx* ctx, uint32_t first_slot, uint32_t n, wg_timer_slot* out_host);
int wg_timers_peers_get(wg_ctx* ctx, uint32_t first_peer, uint32_t n, wg_timer_peer_state* out_host);
int wg_timers_start(wg_ctx* ctx, const wg_timers_start_batch* batch, void* stream);
int wg_timers_mark(wg_ctx* ctx, const wg_timers_mark_batch* batch, void* stream);
int wg_timers_sweep(wg_ctx* ctx, const wg_timers_sweep_batch* batch, void* stream);

/* ---- the end of a session on the device ----
 * What the reference does when a session ends, EstablishedSession.close() -> keypair.clean()
 * (EstablishedSession.java:74-77, SymmetricKeypair.java:85-93: both keys are zeroed), and what a table that only
 * fills needs besides: the retired entries of the receiver-index table are reclaimed, and an expired session's keys
 * are zeroed, without a host round trip. All of it is opt-in: a context that uses none of it behaves as before.
 *
 * wg_rx_sessions_compact(ctx, min_retired, summary_dev, stream): asynchronous on `stream` and capturable; it waits
 *   for, and is waited for by, the receive plans, installs and retires of every stream, as wg_rx_sessions_retire
 *   does. On the device: if used - count (the retired entries) >= max(min_retired, 1), the table is rebuilt from its
 *   live entries; afterwards used == count, every live index resolves to the key slot it resolved to before and
 *   every other index is absent. Otherwise nothing changes. summary (device, 16 bytes, 8-byte aligned, may be NULL)
 *   = {live, dropped, compacted, 0}: {count, the retired entries dropped, 1, 0} or {count, 0, 0, 0}.
 *   Without wg_rx_sessions_reserve: WG_EINVAL. NULL context, misaligned summary: WG_EINVAL.
 *   The live entries are rehashed into a second buffer of the table's capacity, which wg_rx_sessions_reserve
 *   allocates (a capturing stream cannot) and wg_rx_sessions_set keeps at the capacity of the table it builds, and
 *   the header's pointer is flipped: every kernel reads the entries through the header. The two buffers' addresses
 *   sit at a fixed device address and which of them is the spare is decided on the device, so nothing about a call
 *   lives on the host or in the launch: a captured compaction replays any number of times, and after a
 *   wg_rx_sessions_set that grew the table and moved the buffers. A wg_rx_sessions_set or wg_rx_sessions_reserve
 *   that returned an error (an allocation failed: the table is empty and the reserve is gone, and with the spare
 *   there are two allocations that can fail) is the exception: a compaction or an install captured before it
 *   must be captured again after the next successful wg_rx_sessions_reserve.
 *   Three launches, ordered by kernel boundaries, no workgroup waiting for another: the whole spare is cleared (in
 *   every call: it holds the table of two compactions ago) and one thread decides; one thread per bucket of the
 *   current table places a live entry by a 64-bit compare-and-swap against 0 along its probe sequence in the spare
 *   (live indices are unique); one thread flips the pointer, sets used = count and writes the summary. Which
 *   bucket of a chain an entry lands in depends on thread order; no lookup, count or later status does.
 *
 * WG_HS_INSTALL_COMPACT (wg_hs_install_batch.flags): the same compaction, decided on the device in front of the
 *   install's step 3. With m = min(*n_entries, n): if used + m > C / 2 and used > count, the table is compacted
 *   first (the three launches above, in front of the install's own). Statuses and summary are exactly those of
 *   wg_rx_sessions_compact followed by the plain install: step 4's `used` is the compacted table's, so FULL then
 *   means live + passing > C / 2. A captured ... -> wg_hs_respond -> wg_hs_install still replays.
 *
 * WG_TIMERS_WIPE (wg_timers_sweep_batch.flags; only together with WG_TIMERS_RETIRE, alone it is WG_EINVAL): for
 *   every session the sweep lists and retires, the 32 key bytes of its send slot and of its recv slot (if that is
 *   inside the key table) are zeroed, by stores of zero only: no key byte is loaded. A session that is due but does
 *   not fit expired_cap is neither listed nor wiped and stays due. Every output and the summary are what they are
 *   without the flag.
 *   - The key table has no ordering with seals and opens on other streams, as for wg_hs_install: sweep on the stream
 *     that seals and opens next, or synchronise.
 *   - An all-zero key is a known key. A wiped send slot must never be sealed on again: wg_timers_mark(WG_TIMERS_TX,
 *     WG_TIMERS_GATE) refuses its descriptors, because the record is DEAD.
 *   - A wiped recv slot must never be opened on again: its index is retired in the receiver-index table, so
 *     wg_rx_plan answers WG_PKT_NOSESSION.
 *   - The host's mirror of the key table (wg_seal1 / wg_open1, the queues) is not touched: the sweep's slots are
 *     known on the device only. Slots written by wg_hs_install have no key in the mirror already (those paths answer
 *     WG_ENOKEY). A slot whose key the host set with wg_keys_set keeps that key in host memory, and the per-packet
 *     paths go on using it, until the host calls wg_keys_zero or wg_keys_set on it: wipe sessions whose keys came
 *     through wg_hs_install, or follow the expired list with wg_keys_zero.
 *   - Open: a session killed by wg_timers_start because one of its slots was reused keeps the key in its other slot
 *     until that slot is reused or the host calls wg_keys_zero. */
typedef struct wg_rx_compact_summary { /* 16 bytes */
  uint32_t live, dropped, compacted, _zero;
} wg_rx_compact_summary;
int wg_rx_sessions_compact(wg_ctx* ctx, uint32_t min_retired, wg_rx_compact_summary* summary_dev, void* stream);

/* ---- endpoints on the device: learn, roam, and the send lists ----
 * Where a sealed datagram goes. The reference gives every session one address, EstablishedSession.
 * outboundPacketAddress: a responder's session gets the initiation's origin (SessionManager.java:217-229), an
 * initiator's the configured endpoint (:186, :196), and nothing moves it. WireGuard additionally moves a peer's
 * endpoint to the source of every authenticated packet (roaming). Both rules are here, per call, and the transmit side
 * gets what wg_rx_deliver's items are for the receive side: a list the host walks with sendmmsg, so neither tx_status
 * nor a descriptor is read back and the host keeps no slot -> peer -> address table. Configuration (Endpoint =), DNS
 * and the sockets stay on the host. A context that never calls wg_endpoints_* allocates nothing and behaves exactly as
 * before.
 *
 * State (wg_endpoints_reserve(ctx, max_peers); synchronous; a second call with max_peers not above the first is a
 * no-op, a larger one is WG_EINVAL: the state does not grow; max_peers above 2^30: WG_E2BIG), all of it at device
 * addresses that are fixed for the life of the context, so a setter needs no re-capture:
 *   per peer (position in wg_hs_peers_set's table) one 24-byte wg_hs_src, the endpoint; family 0: none (24 zero bytes,
 *     the state at creation). The stored form is normalised: family 4 keeps addr[4 .. 16) zero, and _pad is zero, so
 *     two endpoints are equal exactly when their 24 bytes are.
 *   per key slot the peer it belongs to (uint32; WG_HS_NOPEER at creation).
 *   scratch: one claim word per peer, and the send lists' ranks for 2^22 descriptors per call; a larger call grows
 *     them, except on a capturing stream (WG_EINVAL: run one call of that size outside the capture first).
 * wg_endpoints_set / wg_endpoints_get(ctx, first_peer, n, wg_hs_src*) and wg_endpoint_slots_set / wg_endpoint_slots_get
 *   (ctx, first_slot, n, uint32_t* peers; for sessions keyed with wg_keys_set) take host pointers, are synchronous and
 *   ordered after everything queued on the device, like wg_tx_counters_set. The setter stores the normalised form; a
 *   family outside {0, 4, 6}: WG_EINVAL with nothing changed. A range past max_peers / the key table: WG_ERANGE.
 *   Every call of this section before wg_endpoints_reserve: WG_EINVAL. wg_keys_set / wg_keys_zero do NOT touch the
 *   map: a host that re-keys a slot by hand sets the slot's peer by hand. wg_ctx_destroy frees the state.
 *
 * The four calls below are asynchronous on `stream` and capturable after the reserve; each writes every output word it
 * covers and nothing behind it, writes every scratch word before it reads it, depends on no thread order, and waits
 * for, and is waited for by, the others on every stream. n above 2^30: WG_E2BIG. Summaries are 8-byte aligned, src
 * arrays 8, items and descriptors and entries 16, everything else 4; a misaligned pointer, or an output that overlaps
 * another output or an input, is WG_EINVAL.
 *
 * wg_endpoints_start(ctx, b, stream): after wg_hs_install on the same stream, with the install's own arrays, as
 *   wg_timers_start; src / n_src is the ring's wg_hs_src array by batch index. For every j < min(*n_entries, n) with
 *   inst_status[j] == WG_HS_INST_OK (and, checked again, position < n_slots, both slots inside the key table and
 *   different): the map entries of both slots become the entry's peer, WG_HS_NOPEER for a peer at or past max_peers
 *   (n_nopeer counts those sessions). The endpoint: with WG_HS_INSTALL_SESSIONS, endpoint[peer] = the normalised
 *   src[entry.index], the reference's initiation.originAddress(); with WG_HS_INSTALL_ESTABLISHED it is unchanged (the
 *   reference keeps connectionInfo.endpoint()) unless WG_EP_LEARN_RESPONSE is set (WireGuard: the response's source).
 *   An entry whose index >= n_src, or whose src.family is neither 4 nor 6, leaves the endpoint alone and is counted in
 *   n_badsrc. Of several OK entries of one peer in one call the lowest j, the entry wg_timers_start makes current,
 *   gives the endpoint (if its source is unusable, none does). summary = {n_sessions, n_learned (endpoints written),
 *   n_badsrc, n_nopeer}; n_learned and n_badsrc are 0 where nothing is learned. Up to three launches (the peers' claim
 *   words = none; the map, and atomicMin of j on the peer's claim word; the endpoints). n = 0 writes a zero summary.
 *
 * wg_endpoints_learn(ctx, b, stream): roaming, after wg_rx_deliver with its desc and final_status; src by batch index.
 *   Packet i qualifies if final_status[i] is WG_PKT_OK or WG_PKT_KEEPALIVE (authenticated and past the replay check),
 *   desc[i].key_slot is inside the key table, the slot's peer p < max_peers, and src[i].family is 4 or 6 (a packet
 *   that fails only the last test is counted in n_badsrc). For each peer with qualifying packets the one with the
 *   highest batch index wins, the last to arrive, whatever the dispatch order (an atomicMax per peer, read one launch
 *   later; a wave whose qualifying lanes all name one peer issues one atomic). If the normalised winner differs from
 *   endpoint[p] it replaces it and p has roamed. roamed[0 .. min(n_roamed, roamed_cap)) = the roamed peers in
 *   ascending order; a peer that does not fit is still updated. summary = {n_authentic (qualifying packets), n_peers
 *   (peers with one), n_roamed, n_badsrc}. Five launches (claim words = 0; claim; judge and update, one thread per
 *   peer; prefixes; place). n = 0 writes a zero summary. The reference never roams: a node that wants its behaviour
 *   does not call this.
 *
 * wg_tx_sendlist(ctx, b, stream): over n descriptors and, optionally, their statuses: wg_tx_plan's desc_out /
 *   tx_status (after an optional wg_timers_mark gate), or wg_timers_sweep's keepalives with status = NULL. Descriptor
 *   j is LIVE if len != WG_LEN_INVALID and, when status is given, status[j] == WG_PKT_OK. A live descriptor is LISTED
 *   if its key slot is inside the key table, the slot's peer p < max_peers and endpoint[p].family != 0. items[0 ..
 *   n_items) is the stable compaction of the listed descriptors in j order, as 48-byte wg_tx_item {off = out_off - 16
 *   (the wire packet's start in the seal's output buffer), len = desc.len + 32 (header, ciphertext, tag), key_slot,
 *   peer, index = j, dst = endpoint[p]}. A live descriptor that is not listed is counted in n_noendpoint. With
 *   WG_SEND_GATE, valid only BEFORE the seal on the same stream, such a descriptor is refused as the timers' gate
 *   refuses: status[j] = WG_PKT_NOENDPOINT (when status is given), len = WG_LEN_INVALID, so the seal and the framer
 *   skip it; its claimed counter is lost, which is harmless. summary = {bytes (the sum of the items' len), n_items,
 *   n_noendpoint}. desc and status are in and out with the gate, inputs otherwise. Three launches (judge, prefixes,
 *   place). n = 0 writes a zero summary.
 *
 * wg_hs_sendlist(ctx, b, stream): the same items for the handshake messages, which lie in struct arrays: off is
 *   relative to the start of `entries`, key_slot = 0xFFFFFFFF, index = the entry's position k. By kind:
 *   WG_HS_SEND_RESPONSES: entries = wg_hs_respond's sessions, n_entries = &wg_hs_respond_summary.n_ok; off = 176 k +
 *     16, len = 92, peer = sessions[k].peer, dst = the normalised src[sessions[k].index].
 *   WG_HS_SEND_INITIATIONS: entries = wg_hs_initiate's records with its status and peer arrays; only WG_HS_INIT_OK
 *     entries; off = 160 k + 8, len = records[k].len, peer = peer[k], dst = endpoint[peer[k]].
 *   WG_HS_SEND_COOKIE_REPLIES: entries = wg_hs_admit's replies, n_entries = &wg_hs_admit_summary.n_replies; off =
 *     80 k + 8, len = replies[k].len, peer = WG_HS_NOPEER, dst = the normalised src[replies[k].index].
 *   An entry below min(*n_entries, n) without a usable destination (an index >= n_src, a family that is neither 4 nor
 *   6, a peer at or past max_peers or without an endpoint) is skipped and counted in n_nodst. summary = {bytes,
 *   n_items, n_nodst}. flags must be 0 (the gate is wg_tx_sendlist's): WG_EINVAL. Three launches. n = 0 writes a zero
 *   summary. */
/* 12, the status after WG_PKT_HANDSHAKE: wg_tx_sendlist with WG_SEND_GATE, the descriptor's peer has no endpoint */
#define WG_PKT_NOENDPOINT (WG_PKT_HANDSHAKE + 1u)
#define WG_EP_LEARN_RESPONSE 1u /* wg_endpoints_start_batch.flags */
#define WG_SEND_GATE 1u         /* wg_tx_sendlist_batch.flags */
#define WG_HS_SEND_RESPONSES 0u /* wg_hs_sendlist_batch.kind */
#define WG_HS_SEND_INITIATIONS 1u
#define WG_HS_SEND_COOKIE_REPLIES 2u
typedef struct wg_tx_item { /* 48 bytes */
  uint64_t off;             /* into the seal's output buffer (wg_tx_sendlist) or from `entries` (wg_hs_sendlist) */
  uint32_t len;             /* datagram bytes */
  uint32_t key_slot;        /* 0xFFFFFFFF: a handshake message */
  uint32_t peer;
  uint32_t index;           /* position of the descriptor or entry */
  wg_hs_src dst;
} wg_tx_item;
typedef struct wg_endpoints_start_summary {
  uint32_t n_sessions, n_learned, n_badsrc, n_nopeer;
} wg_endpoints_start_summary;
typedef struct wg_endpoints_start_batch {
  const void* entries;         /* device: the install's entries */
  const uint32_t* n_entries;   /* device, or NULL: all n */
  const uint32_t* inst_status; /* device, n entries: the install's */
  const uint32_t* send_slot;   /* device, n_slots entries */
  const uint32_t* recv_slot;   /* device, n_slots entries */
  const wg_hs_src* src;        /* device, 8-byte aligned, n_src entries, by batch index */
  wg_endpoints_start_summary* summary; /* device, 16 bytes, 8-byte aligned */
  uint32_t n, n_slots, n_src;
  uint32_t source;             /* WG_HS_INSTALL_SESSIONS or WG_HS_INSTALL_ESTABLISHED */
  uint32_t flags;              /* WG_EP_LEARN_RESPONSE */
  uint32_t _reserved;
} wg_endpoints_start_batch;
typedef struct wg_endpoints_learn_summary {
  uint32_t n_authentic, n_peers, n_roamed, n_badsrc;
} wg_endpoints_learn_summary;
typedef struct wg_endpoints_learn_batch {
  const wg_pkt* desc;           /* device, 16-byte aligned, n entries */
  const uint32_t* final_status; /* device, n entries */
  const wg_hs_src* src;         /* device, 8-byte aligned, n entries, by batch index */
  uint32_t* roamed;             /* device, roamed_cap entries */
  wg_endpoints_learn_summary* summary; /* device, 16 bytes, 8-byte aligned */
  uint32_t n, roamed_cap;
} wg_endpoints_learn_batch;
typedef struct wg_tx_sendlist_summary {
  uint64_t bytes;
  uint32_t n_items, n_noendpoint;
} wg_tx_sendlist_summary;
typedef struct wg_tx_sendlist_batch {
  wg_pkt* desc;      /* device, 16-byte aligned, n entries; in and out with WG_SEND_GATE */
  uint32_t* status;  /* device, n entries, or NULL; in and out with WG_SEND_GATE */
  wg_tx_item* items; /* device, 16-byte aligned, n entries */
  wg_tx_sendlist_summary* summary; /* device, 16 bytes, 8-byte aligned */
  uint32_t n;
  uint32_t flags;    /* WG_SEND_GATE */
} wg_tx_sendlist_batch;
typedef struct wg_hs_sendlist_summary {
  uint64_t bytes;
  uint32_t n_items, n_nodst;
} wg_hs_sendlist_summary;
typedef struct wg_hs_sendlist_batch {
  const void* entries;       /* device, 16-byte aligned: wg_hs_session[], wg_hs_record[] or wg_hs_cookie_reply[] */
  const uint32_t* n_entries; /* device, or NULL: all n */
  const uint32_t* status;    /* device, n entries: wg_hs_initiate's (initiations only) */
  const uint32_t* peer;      /* device, n entries: wg_hs_initiate's (initiations only) */
  const wg_hs_src* src;      /* device, 8-byte aligned, n_src entries, by batch index (responses, cookie replies) */
  wg_tx_item* items;         /* device, 16-byte aligned, n entries */
  wg_hs_sendlist_summary* summary; /* device, 16 bytes, 8-byte aligned */
  uint32_t n, n_src;
  uint32_t kind;             /* WG_HS_SEND_* */
  uint32_t flags;            /* 0 */
} wg_hs_sendlist_batch;
int wg_endpoints_reserve(wg_ctx* ctx, uint32_t max_peers);
int wg_endpoints_set(wg_ctx* ctx, uint32_t first_peer, uint32_t n, const wg_hs_src* endpoints_host);
int wg_endpoints_get(wg_ctx* ctx, uint32_t first_peer, uint32_t n, wg_hs_src* endpoints_host);
int wg_endpoint_slots_set(wg_ctx* ctx, uint32_t first_slot, uint32_t n, const uint32_t* peers_host);
int wg_endpoint_slots_get(wg_ctx* ctx, uint32_t first_slot, uint32_t n, uint32_t* peers_host);
int wg_endpoints_start(wg_ctx* ctx, const wg_endpoints_start_batch* batch, void* stream);
int wg_endpoints_learn(wg_ctx* ctx, const wg_endpoints_learn_batch* batch, void* stream);
int wg_tx_sendlist(wg_ctx* ctx, const wg_tx_sendlist_batch* batch, void* stream);
int wg_hs_sendlist(wg_ctx* ctx, const wg_hs_sendlist_batch* batch, void* stream);

int wg_seal1(wg_ctx* ctx, uint32_t key_slot, uint64_t counter, const uint8_t* pt, uint32_t len, uint8_t* out);
int wg_open1(wg_ctx* ctx, uint32_t key_slot, uint64_t counter, const uint8_t* in, uint32_t len, uint8_t* pt);
int wg_pp_config(wg_ctx* ctx, uint32_t waves, uint32_t idle_us);
/* Diagnostic: the stages of the calling thread's last wg_seal1 / wg_open1, in ns (out[0..7]: total,
 * claim, publish, wait for the completion, device service time, copy-out, slept on the futex 0/1,
 * relaunched the server 0/1); recorded only when WG_PP_CALL_STAMPS=1 is set before the context's
 * first per-packet call (zeros otherwise); tools/batcher_bench stamps=1 reports the slowest call's. */
int wg_pp_last_call(uint64_t* out, uint32_t n);
int wg_batcher_config(wg_ctx* ctx, uint32_t max_batch, uint32_t window_us);
int wg_batcher_stats(wg_ctx* ctx, uint64_t* launches, uint64_t* packets);
int wg_seal_host(wg_ctx* ctx, const wg_pkt* desc_host, uint32_t n, const uint8_t* in_host, uint64_t in_size,
                 uint8_t* out_host, uint64_t out_size, uint32_t max_len, uint32_t flags);
int wg_open_host(wg_ctx* ctx, const wg_pkt* desc_host, uint32_t n, const uint8_t* in_host, uint64_t in_size,
                 uint8_t* out_host, uint64_t out_size, uint32_t* status_host, uint32_t max_len, uint32_t flags);
/* ---- asynchronous batch submission -----------------------
 * The reference's TransportManager hands every packet to a ForkJoinPool worker that calls
 * cipher / decipher synchronously and then queues the result for the UDP / tun worker
 * (TransportManager.java:41,70-93,137-158; EstablishedSession.java:88-90). A queue replaces
 * that synchronous call: producers enqueue packets and return at once, one host thread per
 * queue batches whatever is waiting into k_transport launches over a pinned, device-mapped
 * ring (zero-copy), and the consumer reaps the results from a completion queue.
 *   wg_queue_create(ctx, mode, capacity, max_len, max_batch, &q): a seal (WG_MODE_SEAL) or open
 *     (WG_MODE_OPEN) queue of `capacity` slots (rounded up to a power of two; 0 = 65536) for
 *     payloads of at most max_len bytes (0 = 2032, the reference pipeline's incoming limit;
 *     at most WG_QUEUE_MAX_LEN), batches of at most max_batch packets (0 = 8192).
 *   wg_submit_seal(q, key_slot, counter, pt, len, user): copies the plaintext into a free slot
 *     and queues it; the nonce is LE64(counter) || 0^4 (SymmetricKeypair.java:52-61), the key
 *     the one key_slot holds at the time of the submit (copied into the slot with the packet, as the
 *     reference's synchronous cipher() uses the key it holds when called: a later wg_keys_set /
 *     wg_keys_zero of the slot does not change a queued packet; the copy is wiped when the packet's
 *     batch completes). A slot without a key (never set, or zeroed) is refused: WG_ENOKEY. Blocks only while every slot is in
 *     use (until the consumer calls wg_reap_done), and then at most the queue's submit timeout:
 *     returns WG_EAGAIN after it. Thread-safe: any number of producers.
 *   wg_submit_open(q, key_slot, counter, ct_tag, len, user): the same for ct || tag (len + 16 B).
 *   wg_submit_seal_n / wg_submit_open_n(q, p, n): n packets in one call, as n wg_submit_* calls in
 *     order from one thread, but with one lane lock and one publication per run of free slots.
 *     Returns how many were queued: n, or fewer (at least 1) when the submit timeout ran out
 *     partway; WG_EAGAIN when it ran out before the first. Every entry is checked first: a bad one
 *     fails the call (WG_EINVAL / WG_E2BIG / WG_ERANGE) with nothing queued. While it copies packet
 *     k it prefetches the bytes of packet k + 2 (WG_QUEUE_PREFETCH=0..8 sets the distance), so
 *     handing over completions of another queue (GPU-written, not in this core's caches) is fast.
 *   wg_reap(q, out, max, timeout_us): up to max completions (waits up to timeout_us for the
 *     first); returns how many, or a negative error. completion.data points into the queue's
 *     pinned ring: ct || tag (len + 16 B) for a seal, the plaintext (len B, valid when status is
 *     WG_PKT_OK; WG_PKT_BADTAG: rejected, ChaCha20Poly1305.java:51-55) for an open. Completions
 *     come back in batch order, not in submission order.
 *   wg_reap_done(q, c, n): the consumer is done with these completions (their slots are reused);
 *     each completion exactly once (a slot handed back twice would be given to two producers).
 *   wg_queue_set_submit_timeout(q, timeout_us): how long wg_submit_* waits for a free slot before it
 *     returns WG_EAGAIN (0, the default: without bound). A consumer that stalls then cannot wedge the
 *     producers (ForkJoinPool workers) for good.
 *   wg_queue_destroy: waits for the batches in flight; unreaped completions are dropped. Call it
 *     only once no thread is inside (or can still enter) wg_submit_* / wg_reap* on this queue.
 * A producer thread keeps up to 32 slots taken from other lanes in its lane's stash; slots stashed
 * by a thread that exits are used by the next thread that maps to the same lane. */
#define WG_QUEUE_MAX_LEN 16384u
typedef struct wg_queue wg_queue;
typedef struct wg_completion {
  uint64_t user;      /* the submitter's tag */
  uint64_t counter;
  uint8_t* data;      /* result in the pinned ring (see above) */
  uint32_t len;       /* payload bytes */
  uint32_t status;    /* WG_PKT_OK, WG_PKT_BADTAG (open), WG_PKT_NOKEY or WG_PKT_FAILED */
  uint32_t key_slot;
  uint32_t slot;      /* ring slot (handed back by wg_reap_done) */
  uint64_t submit_ns; /* steady-clock time of the submit (latency accounting) */
} wg_completion;
int wg_queue_create(wg_ctx* ctx, int mode, uint32_t capacity, uint32_t max_len, uint32_t max_batch, wg_queue** q);
int wg_queue_destroy(wg_queue* q);
int wg_submit_seal(wg_queue* q, uint32_t key_slot, uint64_t counter, const uint8_t* pt, uint32_t len, uint64_t user);
int wg_submit_open(wg_queue* q, uint32_t key_slot, uint64_t counter, const uint8_t* ct_tag, uint32_t len,
                   uint64_t user);
typedef struct wg_submit {
  uint64_t user;        /* the submitter's tag (echoed in the completion) */
  uint64_t counter;     /* nonce = LE64(counter) || 0^4 */
  const uint8_t* data;  /* seal: the plaintext (len B); open: ct || tag (len + 16 B) */
  uint32_t len;         /* payload bytes */
  uint32_t key_slot;
} wg_submit;
int wg_submit_seal_n(wg_queue* q, const wg_submit* p, uint32_t n);
int wg_submit_open_n(wg_queue* q, const wg_submit* p, uint32_t n);
int wg_reap(wg_queue* q, wg_completion* out, uint32_t max, uint32_t timeout_us);
int wg_reap_done(wg_queue* q, const wg_completion* done, uint32_t n);
int wg_queue_stats(wg_queue* q, uint64_t* batches, uint64_t* packets);
int wg_queue_set_submit_timeout(wg_queue* q, uint32_t timeout_us);
/* Diagnostic: ring slots whose copy of a session key is not all zero. A slot's key copy is wiped as
 * soon as its batch has completed, so with nothing in flight this is 0 (no key outlives the packets
 * that used it in pinned memory, as clean() leaves none, SymmetricKeypair.java:85-89). */
uint32_t wg_queue_key_residue(const wg_queue* q);

/* Pinned host rings for the host path (the reference's packet buffers come from
 * a native pool, Pool.java:96; pinning them makes wg_seal_host/wg_open_host zero-copy).
 * wg_host_alloc: page-locked, device-mapped, portable across devices.
 * wg_host_register: pin existing memory (e.g. a Java Arena segment) in place. */
int wg_host_alloc(wg_ctx* ctx, uint64_t bytes, void** out);
int wg_host_free(wg_ctx* ctx, void* p);
int wg_host_register(wg_ctx* ctx, void* p, uint64_t bytes);
int wg_host_unregister(wg_ctx* ctx, void* p);
/* General AEAD / primitives on host buffers with a per-call key list
 * (desc[i].key_slot indexes keys_host[nkeys][32]); the device copy of the keys
 * is zeroed before returning. */
int wg_aead_host(wg_ctx* ctx, int mode, const wg_aead_desc* desc_host, uint32_t n, const uint8_t* keys_host,
                 uint32_t nkeys, const uint8_t* in_host, uint64_t in_size, const uint8_t* aad_host, uint64_t aad_size,
                 uint8_t* out_host, uint64_t out_size, uint32_t* status_host);

/* ---- instrumentation -------------------------------------------------------
 * Average duration (ms) of the last `wg_timing_launches` kernel launches made
 * by batch calls on this context, measured with HIP events on the launch
 * stream (used by bench.py for the roofline `achieved` figure). */
int wg_timing_enable(wg_ctx* ctx, int on);
int wg_timing_read(wg_ctx* ctx, double* total_ms, uint64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* WGAEAD_H */
