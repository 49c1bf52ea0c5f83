"""ctypes binding of libwgaead.so — the C-ABI declared in include/wgaead.h.

The product path has no CPU fallback: if the shared library (built in-tree by
``make -C wireguard-java_amd/csrc``) is missing or no HIP device is usable, the
calls below raise ``WgError`` instead of computing anything on the host.
"""
from __future__ import annotations

import ctypes
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WG_LIB_PATH") or os.path.join(HERE, "libwgaead.so")

WG_OK = 0
WG_EINVAL = -22
WG_ENOMEM = -12
WG_ERANGE = -34
WG_E2BIG = -7
WG_EDEVICE = -5
WG_ESELFTEST = -74
WG_EAGAIN = -11
WG_ENOKEY = -126
WG_PKT_OK = 0
WG_PKT_BADTAG = 1
WG_PKT_BADHDR = 2
WG_PKT_KEEPALIVE = 3
WG_PKT_BADIP = 4
WG_PKT_FILTERED = 5
WG_PKT_REPLAY = 6
WG_PKT_NOKEY = 7
WG_PKT_NOROUTE = 8
WG_PKT_TOOLONG = 9
WG_PKT_NOSESSION = 10
WG_PKT_HANDSHAKE = 11
WG_PKT_NOENDPOINT = 12
WG_PKT_FAILED = 255
WG_QUEUE_MAX_LEN = 16384
WG_RX_FILTER = 1
WG_RX_REPLAY = 2
WG_TX_BROADCAST = 0
WG_TX_ROUTE = 1
WG_RX_PT_AFTER = 0
WG_RX_PT_PACKED = 1
WG_B2S_OK = 0
WG_B2S_BADDESC = 1
WG_HS_OK = 0
WG_HS_BADLEN = 1
WG_HS_BADTYPE = 2
WG_HS_BADMAC1 = 3
WG_HS_BADMAC2 = 4
WG_HS_BADSRC = 5
WG_HS_NONONCE = 6
WG_HS_NEEDCOOKIE = 7
WG_HS_COOKIE_SIZE = 64
WG_HS_CK_OK = 0
WG_HS_CK_NOPENDING = 1
WG_HS_CK_BADAUTH = 2
WG_HS_CK_SKIPPED = 3
WG_HS_CK_BADLEN = 4
WG_HS_MAC2_OK = 0
WG_HS_MAC2_NONE = 1
WG_HS_MAC2_BADDESC = 2
WG_HS_MAC2_BADPEER = 3
WG_HS_RL_MAX_BURST = 16
WG_HS_RL_OK = 0
WG_HS_RL_LIMITED = 1
WG_HS_RL_FULL = 2
WG_HS_RL_BADSRC = 3
WG_HS_RL_COMPACT = 1
WG_HS_INIT_SIZE = 148
WG_HS_RESP_SIZE = 92
WG_X25519_OK = 0
WG_X25519_BADDESC = 1
WG_X25519_ZERO = 2
WG_X25519_SKIPPED = 3
WG_X25519_BASE = 1
WG_HS_OPEN_OK = 0
WG_HS_OPEN_NEWPEER = 1
WG_HS_OPEN_BADAUTH = 2
WG_HS_OPEN_SKIPPED = 3
WG_HS_OPEN_BADDESC = 4
WG_HS_NOPEER = 0xFFFFFFFF
WG_HS_RESP_OK = 0
WG_HS_RESP_NOPEER = 1
WG_HS_RESP_NOEPH = 2
WG_HS_RESP_SKIP_NEWPEER = 1
WG_HS_INIT_OK = 0
WG_HS_INIT_BADPEER = 1
WG_HS_INIT_NOEPH = 2
WG_HS_FIN_OK = 0
WG_HS_FIN_NOPENDING = 1
WG_HS_FIN_BADAUTH = 2
WG_HS_FIN_SKIPPED = 3
WG_HS_FIN_BADDESC = 4
WG_HS_INST_OK = 0
WG_HS_INST_BADSLOT = 1
WG_HS_INST_DUPSLOT = 2
WG_HS_INST_DUPINDEX = 3
WG_HS_INST_FULL = 4
WG_HS_INSTALL_SESSIONS = 0
WG_HS_INSTALL_ESTABLISHED = 1
WG_HS_INSTALL_WIPE = 1
WG_HS_INSTALL_COMPACT = 4
WG_TIMER_NONE, WG_TIMER_SEND_INITIATOR, WG_TIMER_SEND_RESPONDER, WG_TIMER_RECV, WG_TIMER_DEAD = 0, 1, 2, 3, 4
WG_TIMER_NOSLOT = 0xFFFFFFFF
WG_TIMERS_INITIATOR_ONLY = 1
WG_TIMER_PEER_CAN_INITIATE = 1
WG_TIMERS_RX, WG_TIMERS_TX = 0, 1
WG_TIMERS_GATE = 1
WG_TIMERS_RETIRE = 1
WG_TIMERS_WIPE = 2
WG_EP_LEARN_RESPONSE = 1
WG_SEND_GATE = 1
WG_HS_SEND_RESPONSES, WG_HS_SEND_INITIATIONS, WG_HS_SEND_COOKIE_REPLIES = 0, 1, 2
WG_HS_TS_OK = 0
WG_HS_TS_REPLAY = 1
WG_HS_TS_SUPERSEDED = 2
WG_HS_TS_BADAUTH = 3
WG_HS_TS_NOPEER = 4
WG_HS_TS_BADDESC = 5
WG_MAX_FILTERS = 65536
WG_NO_FILTER = 0xFFFFFFFF
WG_LEN_INVALID = 0xFFFFFFFF
WG_TAG_SIZE = 16
WG_NONCE_SIZE = 12
WG_KEY_SIZE = 32
WG_MAX_PACKET = 65535
WG_F_UNIFORM = 1
WG_F_FRAME = 2
WG_F_AFTER_SEAL = 4
WG_F_RX_FILTER = 8
WG_MODE_SEAL, WG_MODE_OPEN, WG_MODE_CIPHER, WG_MODE_MAC = 0, 1, 2, 3

_ERRNAMES = {WG_EINVAL: "EINVAL", WG_ENOMEM: "ENOMEM", WG_ERANGE: "ERANGE", WG_E2BIG: "E2BIG",
             WG_EDEVICE: "EDEVICE", WG_ESELFTEST: "ESELFTEST", WG_EAGAIN: "EAGAIN", WG_ENOKEY: "ENOKEY"}


class WgError(RuntimeError):
    """A negative return code of libwgaead (mirrors the RuntimeException the reference's
    FFM wrappers raise on a failed downcall, ChaCha20.java:102,110,141)."""

    def __init__(self, code: int, msg: str = ""):
        super().__init__(f"libwgaead {_ERRNAMES.get(code, code)}: {msg}")
        self.code = code


class WgPkt(ctypes.Structure):
    _fields_ = [("in_off", ctypes.c_uint64), ("out_off", ctypes.c_uint64), ("counter", ctypes.c_uint64),
                ("len", ctypes.c_uint32), ("key_slot", ctypes.c_uint32)]


class WgAeadDesc(ctypes.Structure):
    _fields_ = [("in_off", ctypes.c_uint64), ("out_off", ctypes.c_uint64), ("aad_off", ctypes.c_uint64),
                ("len", ctypes.c_uint32), ("aad_len", ctypes.c_uint32), ("key_slot", ctypes.c_uint32),
                ("ctr0", ctypes.c_uint32), ("nonce", ctypes.c_uint32 * 3), ("_reserved", ctypes.c_uint32 * 3)]


class WgPrefix(ctypes.Structure):
    _fields_ = [("family", ctypes.c_uint8), ("prefix_len", ctypes.c_uint8), ("addr", ctypes.c_uint8 * 16)]


class WgBatch(ctypes.Structure):
    """wg_batch: one direction of wg_duplex_batch (device pointers)."""
    _fields_ = [("desc", ctypes.c_void_p), ("in_", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("status", ctypes.c_void_p), ("in_size", ctypes.c_uint64), ("out_size", ctypes.c_uint64),
                ("n", ctypes.c_uint32), ("max_len", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("_reserved", ctypes.c_uint32)]


class WgTxBatch(ctypes.Structure):
    """wg_tx_batch: one wg_tx_plan call (device pointers)."""
    _fields_ = [("in_", ctypes.c_void_p), ("in_size", ctypes.c_uint64), ("pkt_off", ctypes.c_void_p),
                ("pkt_len", ctypes.c_void_p), ("desc_out", ctypes.c_void_p), ("tx_status", ctypes.c_void_p),
                ("wire_base", ctypes.c_uint64), ("wire_stride", ctypes.c_uint64), ("out_size", ctypes.c_uint64),
                ("n", ctypes.c_uint32), ("max_len", ctypes.c_uint32), ("mode", ctypes.c_uint32),
                ("_reserved", ctypes.c_uint32)]


class WgRxSummary(ctypes.Structure):
    """wg_rx_summary: what wg_rx_plan leaves beside the descriptors."""
    _fields_ = [("pt_used", ctypes.c_uint64), ("n_open", ctypes.c_uint32), ("n_host", ctypes.c_uint32)]


class WgRxBatch(ctypes.Structure):
    """wg_rx_batch: one wg_rx_plan call (device pointers)."""
    _fields_ = [("wire", ctypes.c_void_p), ("wire_size", ctypes.c_uint64), ("pkt_off", ctypes.c_void_p),
                ("pkt_len", ctypes.c_void_p), ("desc_out", ctypes.c_void_p), ("rx_status", ctypes.c_void_p),
                ("host_list", ctypes.c_void_p), ("summary", ctypes.c_void_p), ("pt_base", ctypes.c_uint64),
                ("pt_size", ctypes.c_uint64), ("n", ctypes.c_uint32), ("max_len", ctypes.c_uint32),
                ("mode", ctypes.c_uint32), ("_reserved", ctypes.c_uint32)]


class WgRxItem(ctypes.Structure):
    """wg_rx_item: one tun write of wg_rx_deliver's list."""
    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint32), ("key_slot", ctypes.c_uint32)]


class WgRxDelivered(ctypes.Structure):
    """wg_rx_delivered: totals of one wg_rx_deliver call."""
    _fields_ = [("bytes", ctypes.c_uint64), ("n_items", ctypes.c_uint32), ("n_keepalive", ctypes.c_uint32)]


class WgRxDeliverBatch(ctypes.Structure):
    """wg_rx_deliver_batch: one wg_rx_deliver call (device pointers)."""
    _fields_ = [("desc", ctypes.c_void_p), ("plan_status", ctypes.c_void_p), ("open_status", ctypes.c_void_p),
                ("final_status", ctypes.c_void_p), ("items", ctypes.c_void_p), ("index_out", ctypes.c_void_p),
                ("delivered", ctypes.c_void_p), ("n", ctypes.c_uint32), ("_reserved", ctypes.c_uint32)]


class WgB2sDesc(ctypes.Structure):
    """wg_b2s_desc: one message of wg_blake2s_batch."""
    _fields_ = [("in_off", ctypes.c_uint64), ("out_off", ctypes.c_uint64), ("key_off", ctypes.c_uint64),
                ("len", ctypes.c_uint32), ("outlen", ctypes.c_uint8), ("keylen", ctypes.c_uint8),
                ("_pad", ctypes.c_uint8 * 2)]


class WgHsRecord(ctypes.Structure):
    """wg_hs_record: one accepted handshake message of wg_hs_check."""
    _fields_ = [("index", ctypes.c_uint32), ("len", ctypes.c_uint32), ("msg", ctypes.c_uint8 * 148),
                ("_pad", ctypes.c_uint32)]


class WgHsSummary(ctypes.Structure):
    """wg_hs_summary: totals of one wg_hs_check call."""
    _fields_ = [("n_valid", ctypes.c_uint32), ("n_init", ctypes.c_uint32), ("n_resp", ctypes.c_uint32),
                ("n_rejected", ctypes.c_uint32)]


class WgHsBatch(ctypes.Structure):
    """wg_hs_batch: one wg_hs_check call (device pointers)."""
    _fields_ = [("wire", ctypes.c_void_p), ("wire_size", ctypes.c_uint64), ("pkt_off", ctypes.c_void_p),
                ("pkt_len", ctypes.c_void_p), ("list", ctypes.c_void_p), ("n_list", ctypes.c_void_p),
                ("hs_status", ctypes.c_void_p), ("records", ctypes.c_void_p), ("summary", ctypes.c_void_p),
                ("n", ctypes.c_uint32), ("_reserved", ctypes.c_uint32)]


class WgX25519Desc(ctypes.Structure):
    """wg_x25519_desc: one scalar multiplication of wg_x25519_batch."""
    _fields_ = [("scalar_off", ctypes.c_uint64), ("point_off", ctypes.c_uint64), ("out_off", ctypes.c_uint64),
                ("flags", ctypes.c_uint32), ("_pad", ctypes.c_uint32)]


class WgHsDhBatch(ctypes.Structure):
    """wg_hs_dh_batch: one wg_hs_dh call (device pointers)."""
    _fields_ = [("records", ctypes.c_void_p), ("n_records", ctypes.c_void_p), ("shared", ctypes.c_void_p),
                ("dh_status", ctypes.c_void_p), ("n", ctypes.c_uint32), ("_reserved", ctypes.c_uint32)]


class WgHsInit(ctypes.Structure):
    """wg_hs_init: one authenticated initiation of wg_hs_open."""
    _fields_ = [("index", ctypes.c_uint32), ("record", ctypes.c_uint32), ("sender_index", ctypes.c_uint32),
                ("peer", ctypes.c_uint32), ("remote_ephemeral", ctypes.c_uint8 * 32),
                ("remote_static", ctypes.c_uint8 * 32), ("hash", ctypes.c_uint8 * 32),
                ("chain_key", ctypes.c_uint8 * 32)]


class WgHsOpenSummary(ctypes.Structure):
    """wg_hs_open_summary: totals of one wg_hs_open call."""
    _fields_ = [("n_emitted", ctypes.c_uint32), ("n_known", ctypes.c_uint32), ("n_badauth", ctypes.c_uint32),
                ("n_skipped", ctypes.c_uint32)]


class WgHsOpenBatch(ctypes.Structure):
    """wg_hs_open_batch: one wg_hs_open call (device pointers)."""
    _fields_ = [("records", ctypes.c_void_p), ("n_records", ctypes.c_void_p), ("shared", ctypes.c_void_p),
                ("dh_status", ctypes.c_void_p), ("open_status", ctypes.c_void_p), ("inits", ctypes.c_void_p),
                ("summary", ctypes.c_void_p), ("n", ctypes.c_uint32), ("_reserved", ctypes.c_uint32)]


class WgHsSession(ctypes.Structure):
    """wg_hs_session: one answered initiation of wg_hs_respond."""
    _fields_ = [("index", ctypes.c_uint32), ("init", ctypes.c_uint32), ("peer", ctypes.c_uint32),
                ("local_index", ctypes.c_uint32), ("response", ctypes.c_uint8 * 92), ("remote_index", ctypes.c_uint32),
                ("send_key", ctypes.c_uint8 * 32), ("recv_key", ctypes.c_uint8 * 32)]


class WgHsRespondSummary(ctypes.Structure):
    """wg_hs_respond_summary: totals of one wg_hs_respond call."""
    _fields_ = [("n_ok", ctypes.c_uint32), ("n_nopeer", ctypes.c_uint32), ("n_noeph", ctypes.c_uint32),
                ("_zero", ctypes.c_uint32)]


class WgHsRespondBatch(ctypes.Structure):
    """wg_hs_respond_batch: one wg_hs_respond call (device pointers)."""
    _fields_ = [("inits", ctypes.c_void_p), ("n_inits", ctypes.c_void_p), ("ephemerals", ctypes.c_void_p),
                ("local_index", ctypes.c_void_p), ("resp_status", ctypes.c_void_p), ("sessions", ctypes.c_void_p),
                ("summary", ctypes.c_void_p), ("n", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class WgHsPending(ctypes.Structure):
    """wg_hs_pending: one initiation awaiting its response (wg_hs_initiate, wg_hs_finish)."""
    _fields_ = [("state", ctypes.c_uint32), ("peer", ctypes.c_uint32), ("local_index", ctypes.c_uint32),
                ("_zero", ctypes.c_uint32), ("ephemeral", ctypes.c_uint8 * 32), ("hash", ctypes.c_uint8 * 32),
                ("chain_key", ctypes.c_uint8 * 32)]


class WgHsEstablished(ctypes.Structure):
    """wg_hs_established: one completed handshake of wg_hs_finish."""
    _fields_ = [("index", ctypes.c_uint32), ("record", ctypes.c_uint32), ("pending", ctypes.c_uint32),
                ("peer", ctypes.c_uint32), ("local_index", ctypes.c_uint32), ("remote_index", ctypes.c_uint32),
                ("_zero", ctypes.c_uint32 * 2), ("send_key", ctypes.c_uint8 * 32), ("recv_key", ctypes.c_uint8 * 32)]


class WgHsInitiateBatch(ctypes.Structure):
    """wg_hs_initiate_batch: one wg_hs_initiate call (device pointers)."""
    _fields_ = [("peer", ctypes.c_void_p), ("ephemerals", ctypes.c_void_p), ("timestamps", ctypes.c_void_p),
                ("local_index", ctypes.c_void_p), ("status", ctypes.c_void_p), ("records", ctypes.c_void_p),
                ("pending", ctypes.c_void_p), ("summary", ctypes.c_void_p), ("n", ctypes.c_uint32),
                ("_reserved", ctypes.c_uint32)]


class WgHsFinishBatch(ctypes.Structure):
    """wg_hs_finish_batch: one wg_hs_finish call (device pointers)."""
    _fields_ = [("records", ctypes.c_void_p), ("n_records", ctypes.c_void_p), ("pending", ctypes.c_void_p),
                ("fin_status", ctypes.c_void_p), ("established", ctypes.c_void_p), ("summary", ctypes.c_void_p),
                ("n", ctypes.c_uint32), ("n_pending", ctypes.c_uint32)]


class WgHsStampSummary(ctypes.Structure):
    """wg_hs_stamp_summary: totals of one wg_hs_stamp call."""
    _fields_ = [("n_ok", ctypes.c_uint32), ("n_stale", ctypes.c_uint32), ("n_badauth", ctypes.c_uint32),
                ("n_skipped", ctypes.c_uint32)]


class WgHsStampBatch(ctypes.Structure):
    """wg_hs_stamp_batch: one wg_hs_stamp call (device pointers)."""
    _fields_ = [("inits", ctypes.c_void_p), ("n_inits", ctypes.c_void_p), ("records", ctypes.c_void_p),
                ("shared", ctypes.c_void_p), ("ts_status", ctypes.c_void_p), ("opened", ctypes.c_void_p),
                ("fresh", ctypes.c_void_p), ("summary", ctypes.c_void_p), ("n", ctypes.c_uint32),
                ("n_rec", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("_reserved", ctypes.c_uint32)]


class WgHsSrc(ctypes.Structure):
    """wg_hs_src: the source address of one datagram (wg_hs_admit)."""
    _fields_ = [("addr", ctypes.c_uint8 * 16), ("port", ctypes.c_uint8 * 2), ("family", ctypes.c_uint8),
                ("_pad", ctypes.c_uint8 * 5)]


class WgHsCookieReply(ctypes.Structure):
    """wg_hs_cookie_reply: one cookie reply of wg_hs_admit."""
    _fields_ = [("index", ctypes.c_uint32), ("len", ctypes.c_uint32), ("msg", ctypes.c_uint8 * 64),
                ("_pad", ctypes.c_uint32 * 2)]


class WgHsAdmitSummary(ctypes.Structure):
    """wg_hs_admit_summary: the cookie side's totals of one wg_hs_admit call."""
    _fields_ = [("n_replies", ctypes.c_uint32), ("n_mac2_ok", ctypes.c_uint32), ("n_nononce", ctypes.c_uint32),
                ("n_badsrc", ctypes.c_uint32)]


class WgHsAdmitBatch(ctypes.Structure):
    """wg_hs_admit_batch: one wg_hs_admit call (device pointers)."""
    _fields_ = [("hs", WgHsBatch), ("src", ctypes.c_void_p), ("nonces", ctypes.c_void_p), ("replies", ctypes.c_void_p),
                ("admit_summary", ctypes.c_void_p)]


class WgHsLearned(ctypes.Structure):
    """wg_hs_learned: one opened cookie reply of wg_hs_cookie_open."""
    _fields_ = [("index", ctypes.c_uint32), ("pending", ctypes.c_uint32), ("peer", ctypes.c_uint32),
                ("_zero", ctypes.c_uint32)]


class WgHsCookieOpenSummary(ctypes.Structure):
    """wg_hs_cookie_open_summary: totals of one wg_hs_cookie_open call."""
    _fields_ = [("n_ok", ctypes.c_uint32), ("n_nopending", ctypes.c_uint32), ("n_badauth", ctypes.c_uint32),
                ("n_skipped", ctypes.c_uint32)]


class WgHsCookieOpenBatch(ctypes.Structure):
    """wg_hs_cookie_open_batch: one wg_hs_cookie_open call (device pointers)."""
    _fields_ = [("wire", ctypes.c_void_p), ("wire_size", ctypes.c_uint64), ("pkt_off", ctypes.c_void_p),
                ("pkt_len", ctypes.c_void_p), ("sent", ctypes.c_void_p), ("pending", ctypes.c_void_p),
                ("ck_status", ctypes.c_void_p), ("learned", ctypes.c_void_p), ("summary", ctypes.c_void_p),
                ("n", ctypes.c_uint32), ("n_pending", ctypes.c_uint32)]


class WgHsMac2Summary(ctypes.Structure):
    """wg_hs_mac2_summary: totals of one wg_hs_mac2 call."""
    _fields_ = [("n_ok", ctypes.c_uint32), ("n_none", ctypes.c_uint32), ("n_bad", ctypes.c_uint32),
                ("_zero", ctypes.c_uint32)]


class WgHsMac2Batch(ctypes.Structure):
    """wg_hs_mac2_batch: one wg_hs_mac2 call (device pointers)."""
    _fields_ = [("records", ctypes.c_void_p), ("peer", ctypes.c_void_p), ("mac2_status", ctypes.c_void_p),
                ("summary", ctypes.c_void_p), ("n", ctypes.c_uint32), ("_reserved", ctypes.c_uint32)]


class WgHsRlEntry(ctypes.Structure):
    """wg_hs_rl_entry: one source's bucket of the rate limiter (wg_hs_rl_dump / wg_hs_rl_load)."""
    _fields_ = [("addr", ctypes.c_uint8 * 8), ("family", ctypes.c_uint8), ("_pad", ctypes.c_uint8 * 7),
                ("tokens", ctypes.c_uint64), ("last", ctypes.c_uint64)]


class WgHsRlSummary(ctypes.Structure):
    """wg_hs_rl_summary: totals of one wg_hs_ratelimit call."""
    _fields_ = [("n_passed", ctypes.c_uint32), ("n_limited", ctypes.c_uint32), ("n_full", ctypes.c_uint32),
                ("n_badsrc", ctypes.c_uint32)]


class WgHsRlCompactSummary(ctypes.Structure):
    """wg_hs_rl_compact_summary: totals of one wg_hs_rl_compact call."""
    _fields_ = [("kept", ctypes.c_uint32), ("dropped", ctypes.c_uint32), ("_zero", ctypes.c_uint32 * 2)]


class WgHsRlBatch(ctypes.Structure):
    """wg_hs_rl_batch: one wg_hs_ratelimit call (device pointers)."""
    _fields_ = [("records", ctypes.c_void_p), ("n_records", ctypes.c_void_p), ("src", ctypes.c_void_p),
                ("now", ctypes.c_void_p), ("rl_status", ctypes.c_void_p), ("out_records", ctypes.c_void_p),
                ("rl_summary", ctypes.c_void_p), ("n", ctypes.c_uint32), ("n_src", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("_reserved", ctypes.c_uint32)]


class WgHsInstallSummary(ctypes.Structure):
    """wg_hs_install_summary: totals of one wg_hs_install call."""
    _fields_ = [("n_ok", ctypes.c_uint32), ("n_badslot", ctypes.c_uint32), ("n_dup", ctypes.c_uint32),
                ("n_full", ctypes.c_uint32)]


class WgHsInstallBatch(ctypes.Structure):
    """wg_hs_install_batch: one wg_hs_install call (device pointers)."""
    _fields_ = [("entries", ctypes.c_void_p), ("n_entries", ctypes.c_void_p), ("send_slot", ctypes.c_void_p),
                ("recv_slot", ctypes.c_void_p), ("receivers", ctypes.c_void_p), ("inst_status", ctypes.c_void_p),
                ("summary", ctypes.c_void_p), ("n", ctypes.c_uint32), ("n_slots", ctypes.c_uint32),
                ("slot_first", ctypes.c_uint32), ("slot_count", ctypes.c_uint32), ("source", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


class WgRxCompactSummary(ctypes.Structure):
    """wg_rx_compact_summary: what one wg_rx_sessions_compact call found and did."""
    _fields_ = [("live", ctypes.c_uint32), ("dropped", ctypes.c_uint32), ("compacted", ctypes.c_uint32),
                ("_zero", ctypes.c_uint32)]


class WgTimersConfig(ctypes.Structure):
    """wg_timers_config: the session timers' limits in ticks and messages (0 = off)."""
    _fields_ = [("rekey_after_time", ctypes.c_uint64), ("reject_after_time", ctypes.c_uint64),
                ("rekey_timeout", ctypes.c_uint64), ("keepalive_timeout", ctypes.c_uint64), ("linger", ctypes.c_uint64),
                ("rekey_after_messages", ctypes.c_uint64), ("reject_after_messages", ctypes.c_uint64),
                ("flags", ctypes.c_uint64)]


class WgTimerSlot(ctypes.Structure):
    """wg_timer_slot: one key slot's timer record."""
    _fields_ = [("state", ctypes.c_uint32), ("peer", ctypes.c_uint32), ("local_index", ctypes.c_uint32),
                ("partner", ctypes.c_uint32), ("born", ctypes.c_uint64), ("last", ctypes.c_uint64),
                ("last_data", ctypes.c_uint64), ("superseded", ctypes.c_uint64)]


class WgTimerPeer(ctypes.Structure):
    """wg_timer_peer: what wg_timers_peers_set sets per peer."""
    _fields_ = [("keepalive_interval", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("_zero", ctypes.c_uint32)]


class WgTimerPeerState(ctypes.Structure):
    """wg_timer_peer_state: one peer's timer record."""
    _fields_ = [("current", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("keepalive_interval", ctypes.c_uint64),
                ("rekey_listed", ctypes.c_uint64)]


class WgTimersStartBatch(ctypes.Structure):
    """wg_timers_start_batch: one wg_timers_start call (device pointers)."""
    _fields_ = [("entries", ctypes.c_void_p), ("n_entries", ctypes.c_void_p), ("inst_status", ctypes.c_void_p),
                ("send_slot", ctypes.c_void_p), ("recv_slot", ctypes.c_void_p), ("now", ctypes.c_void_p),
                ("n", ctypes.c_uint32), ("n_slots", ctypes.c_uint32), ("source", ctypes.c_uint32),
                ("_reserved", ctypes.c_uint32)]


class WgTimersMarkBatch(ctypes.Structure):
    """wg_timers_mark_batch: one wg_timers_mark call (device pointers)."""
    _fields_ = [("desc", ctypes.c_void_p), ("status", ctypes.c_void_p), ("now", ctypes.c_void_p),
                ("summary", ctypes.c_void_p), ("n", ctypes.c_uint32), ("dir", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("slot_first", ctypes.c_uint32), ("slot_count", ctypes.c_uint32),
                ("_reserved", ctypes.c_uint32)]


class WgTimersSweepBatch(ctypes.Structure):
    """wg_timers_sweep_batch: one wg_timers_sweep call (device pointers)."""
    _fields_ = [("now", ctypes.c_void_p), ("expired", ctypes.c_void_p), ("initiate", ctypes.c_void_p),
                ("keepalives", ctypes.c_void_p), ("summary", ctypes.c_void_p), ("wire_base", ctypes.c_uint64),
                ("wire_stride", ctypes.c_uint64), ("out_size", ctypes.c_uint64), ("expired_cap", ctypes.c_uint32),
                ("initiate_cap", ctypes.c_uint32), ("keepalive_cap", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class WgTxItem(ctypes.Structure):
    """wg_tx_item: one datagram of a send list (wg_tx_sendlist / wg_hs_sendlist)."""
    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint32), ("key_slot", ctypes.c_uint32),
                ("peer", ctypes.c_uint32), ("index", ctypes.c_uint32), ("dst", WgHsSrc)]


class WgEndpointsStartSummary(ctypes.Structure):
    """wg_endpoints_start_summary: totals of one wg_endpoints_start call."""
    _fields_ = [("n_sessions", ctypes.c_uint32), ("n_learned", ctypes.c_uint32), ("n_badsrc", ctypes.c_uint32),
                ("n_nopeer", ctypes.c_uint32)]


class WgEndpointsStartBatch(ctypes.Structure):
    """wg_endpoints_start_batch: one wg_endpoints_start call (device pointers)."""
    _fields_ = [("entries", ctypes.c_void_p), ("n_entries", ctypes.c_void_p), ("inst_status", ctypes.c_void_p),
                ("send_slot", ctypes.c_void_p), ("recv_slot", ctypes.c_void_p), ("src", ctypes.c_void_p),
                ("summary", ctypes.c_void_p), ("n", ctypes.c_uint32), ("n_slots", ctypes.c_uint32),
                ("n_src", ctypes.c_uint32), ("source", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("_reserved", ctypes.c_uint32)]


class WgEndpointsLearnSummary(ctypes.Structure):
    """wg_endpoints_learn_summary: totals of one wg_endpoints_learn call."""
    _fields_ = [("n_authentic", ctypes.c_uint32), ("n_peers", ctypes.c_uint32), ("n_roamed", ctypes.c_uint32),
                ("n_badsrc", ctypes.c_uint32)]


class WgEndpointsLearnBatch(ctypes.Structure):
    """wg_endpoints_learn_batch: one wg_endpoints_learn call (device pointers)."""
    _fields_ = [("desc", ctypes.c_void_p), ("final_status", ctypes.c_void_p), ("src", ctypes.c_void_p),
                ("roamed", ctypes.c_void_p), ("summary", ctypes.c_void_p), ("n", ctypes.c_uint32),
                ("roamed_cap", ctypes.c_uint32)]


class WgTxSendlistSummary(ctypes.Structure):
    """wg_tx_sendlist_summary: totals of one wg_tx_sendlist call."""
    _fields_ = [("bytes", ctypes.c_uint64), ("n_items", ctypes.c_uint32), ("n_noendpoint", ctypes.c_uint32)]


class WgTxSendlistBatch(ctypes.Structure):
    """wg_tx_sendlist_batch: one wg_tx_sendlist call (device pointers)."""
    _fields_ = [("desc", ctypes.c_void_p), ("status", ctypes.c_void_p), ("items", ctypes.c_void_p),
                ("summary", ctypes.c_void_p), ("n", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class WgHsSendlistSummary(ctypes.Structure):
    """wg_hs_sendlist_summary: totals of one wg_hs_sendlist call."""
    _fields_ = [("bytes", ctypes.c_uint64), ("n_items", ctypes.c_uint32), ("n_nodst", ctypes.c_uint32)]


class WgHsSendlistBatch(ctypes.Structure):
    """wg_hs_sendlist_batch: one wg_hs_sendlist call (device pointers)."""
    _fields_ = [("entries", ctypes.c_void_p), ("n_entries", ctypes.c_void_p), ("status", ctypes.c_void_p),
                ("peer", ctypes.c_void_p), ("src", ctypes.c_void_p), ("items", ctypes.c_void_p),
                ("summary", ctypes.c_void_p), ("n", ctypes.c_uint32), ("n_src", ctypes.c_uint32),
                ("kind", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class WgCompletion(ctypes.Structure):
    """wg_completion: one reaped packet of a wg_queue."""
    _fields_ = [("user", ctypes.c_uint64), ("counter", ctypes.c_uint64), ("data", ctypes.c_void_p),
                ("len", ctypes.c_uint32), ("status", ctypes.c_uint32), ("key_slot", ctypes.c_uint32),
                ("slot", ctypes.c_uint32), ("submit_ns", ctypes.c_uint64)]


class WgSubmit(ctypes.Structure):
    """wg_submit: one packet of wg_submit_seal_n / wg_submit_open_n."""
    _fields_ = [("user", ctypes.c_uint64), ("counter", ctypes.c_uint64), ("data", ctypes.c_void_p),
                ("len", ctypes.c_uint32), ("key_slot", ctypes.c_uint32)]


assert ctypes.sizeof(WgBatch) == 64 and ctypes.sizeof(WgCompletion) == 48 and ctypes.sizeof(WgSubmit) == 32
assert ctypes.sizeof(WgTxBatch) == 88
assert ctypes.sizeof(WgRxBatch) == 96 and ctypes.sizeof(WgRxDeliverBatch) == 64
assert ctypes.sizeof(WgRxSummary) == 16 and ctypes.sizeof(WgRxItem) == 16 and ctypes.sizeof(WgRxDelivered) == 16
assert ctypes.sizeof(WgB2sDesc) == 32 and ctypes.sizeof(WgHsRecord) == 160 and ctypes.sizeof(WgHsSummary) == 16
assert ctypes.sizeof(WgHsBatch) == 80
assert ctypes.sizeof(WgX25519Desc) == 32 and ctypes.sizeof(WgHsDhBatch) == 40
assert ctypes.sizeof(WgHsInit) == 144 and ctypes.sizeof(WgHsOpenSummary) == 16 and ctypes.sizeof(WgHsOpenBatch) == 64
assert ctypes.sizeof(WgHsSession) == 176 and ctypes.sizeof(WgHsRespondSummary) == 16 and ctypes.sizeof(WgHsRespondBatch) == 64
assert ctypes.sizeof(WgHsInstallSummary) == 16 and ctypes.sizeof(WgHsInstallBatch) == 80
assert ctypes.sizeof(WgRxCompactSummary) == 16
assert ctypes.sizeof(WgTimersConfig) == 64 and ctypes.sizeof(WgTimerSlot) == 48 and ctypes.sizeof(WgTimerPeer) == 16
assert ctypes.sizeof(WgTimerPeerState) == 24 and ctypes.sizeof(WgTimersStartBatch) == 64
assert ctypes.sizeof(WgTimersMarkBatch) == 56 and ctypes.sizeof(WgTimersSweepBatch) == 80
assert ctypes.sizeof(WgTxItem) == 48 and ctypes.sizeof(WgEndpointsStartBatch) == 80 and ctypes.sizeof(WgEndpointsLearnBatch) == 48
assert ctypes.sizeof(WgTxSendlistBatch) == 40 and ctypes.sizeof(WgHsSendlistBatch) == 72 and ctypes.sizeof(WgTxSendlistSummary) == 16
assert ctypes.sizeof(WgEndpointsStartSummary) == 16 and ctypes.sizeof(WgEndpointsLearnSummary) == 16 and ctypes.sizeof(WgHsSendlistSummary) == 16
assert ctypes.sizeof(WgHsStampSummary) == 16 and ctypes.sizeof(WgHsStampBatch) == 80
assert ctypes.sizeof(WgHsSrc) == 24 and ctypes.sizeof(WgHsCookieReply) == 80 and ctypes.sizeof(WgHsAdmitSummary) == 16
assert ctypes.sizeof(WgHsAdmitBatch) == 112 and ctypes.sizeof(WgHsLearned) == 16 and ctypes.sizeof(WgHsCookieOpenSummary) == 16
assert ctypes.sizeof(WgHsCookieOpenBatch) == 80 and ctypes.sizeof(WgHsMac2Summary) == 16 and ctypes.sizeof(WgHsMac2Batch) == 40
assert ctypes.sizeof(WgPkt) == 32 and ctypes.sizeof(WgAeadDesc) == 64 and ctypes.sizeof(WgPrefix) == 18

# (name, restype, argtypes) for every symbol include/wgaead.h declares
_VP, _U32, _U64, _I, _D = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_double
SIGNATURES = [
    ("wg_aead_selftest", _I, [_I]),
    ("wg_ctx_create", _I, [_I, _U32, ctypes.POINTER(_VP)]),
    ("wg_ctx_destroy", _I, [_VP]),
    ("wg_ctx_device", _I, [_VP]),
    ("wg_ctx_key_slots", _U32, [_VP]),
    ("wg_ctx_stream", _VP, [_VP]),
    ("wg_sync", _I, [_VP, _VP]),
    ("wg_last_error", ctypes.c_char_p, []),
    ("wg_version", ctypes.c_char_p, []),
    ("wg_device_numa_node", _I, [_I]),
    ("wg_ctx_set_kernel", ctypes.c_int, [_VP, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32]),
    ("wg_keys_set", _I, [_VP, _U32, _U32, _VP]),
    ("wg_keys_zero", _I, [_VP, _U32, _U32]),
    ("wg_seal_batch", _I, [_VP, _VP, _U32, _VP, _U64, _VP, _U64, _U32, _U32, _VP]),
    ("wg_open_batch", _I, [_VP, _VP, _U32, _VP, _U64, _VP, _U64, _VP, _U32, _U32, _VP]),
    ("wg_duplex_batch", _I, [_VP, ctypes.POINTER(WgBatch), ctypes.POINTER(WgBatch), _VP]),
    ("wg_ctx_set_receivers", _I, [_VP, _VP, _U32]),
    ("wg_frame_seal", _I, [_VP, _VP, _U32, _VP, _VP, _U64, _U64, _U32, _VP]),
    ("wg_parse_open", _I, [_VP, _VP, _U64, _VP, _VP, _VP, _U32, _VP, _VP, _VP]),
    ("wg_aead_batch", _I, [_VP, _I, _VP, _U32, _VP, _U64, _VP, _U64, _VP, _U64, _VP, _U32, _VP]),
    ("wg_filter_set", _I, [_VP, _U32, _VP, _U32]),
    ("wg_slot_filters_set", _I, [_VP, _U32, _U32, _VP]),
    ("wg_replay_enable", _I, [_VP, _U32]),
    ("wg_replay_reset", _I, [_VP, _U32, _U32]),
    ("wg_replay_state", _I, [_VP, _U32, ctypes.POINTER(_U64), _VP, _U32]),
    ("wg_rx_check", _I, [_VP, _VP, _U32, _VP, _U64, _VP, _U32, _VP]),
    ("wg_tx_peers_set", _I, [_VP, _VP, _U32]),
    ("wg_routes_set", _I, [_VP, _VP, _VP, _U32]),
    ("wg_tx_counters_set", _I, [_VP, _U32, _U32, _VP]),
    ("wg_tx_counters_get", _I, [_VP, _U32, _U32, _VP]),
    ("wg_tx_reserve", _I, [_VP, _U32]),
    ("wg_tx_plan", _I, [_VP, ctypes.POINTER(WgTxBatch), _VP]),
    ("wg_rx_sessions_set", _I, [_VP, _VP, _VP, _U32]),
    ("wg_rx_reserve", _I, [_VP, _U32]),
    ("wg_rx_plan", _I, [_VP, ctypes.POINTER(WgRxBatch), _VP]),
    ("wg_rx_deliver", _I, [_VP, ctypes.POINTER(WgRxDeliverBatch), _VP]),
    ("wg_blake2s_batch", _I, [_VP, _VP, _U32, _VP, _U64, _VP, _U64, _VP, _VP]),
    ("wg_hs_key_set", _I, [_VP, _VP]),
    ("wg_hs_reserve", _I, [_VP, _U32]),
    ("wg_hs_check", _I, [_VP, ctypes.POINTER(WgHsBatch), _VP]),
    ("wg_x25519_batch", _I, [_VP, _VP, _U32, _VP, _U64, _VP, _U64, _VP, _VP]),
    ("wg_hs_static_set", _I, [_VP, _VP, _VP]),
    ("wg_hs_dh", _I, [_VP, ctypes.POINTER(WgHsDhBatch), _VP]),
    ("wg_hs_peers_set", _I, [_VP, _VP, _U32]),
    ("wg_hs_open", _I, [_VP, ctypes.POINTER(WgHsOpenBatch), _VP]),
    ("wg_hs_respond", _I, [_VP, ctypes.POINTER(WgHsRespondBatch), _VP]),
    ("wg_hs_psks_set", _I, [_VP, _VP, _U32]),
    ("wg_hs_initiate", _I, [_VP, ctypes.POINTER(WgHsInitiateBatch), _VP]),
    ("wg_hs_finish", _I, [_VP, ctypes.POINTER(WgHsFinishBatch), _VP]),
    ("wg_hs_stamp", _I, [_VP, ctypes.POINTER(WgHsStampBatch), _VP]),
    ("wg_hs_stamps_set", _I, [_VP, _U32, _U32, _VP]),
    ("wg_hs_stamps_get", _I, [_VP, _U32, _U32, _VP]),
    ("wg_hs_cookie_secret_set", _I, [_VP, _VP]),
    ("wg_hs_admit", _I, [_VP, ctypes.POINTER(WgHsAdmitBatch), _VP]),
    ("wg_hs_cookie_open", _I, [_VP, ctypes.POINTER(WgHsCookieOpenBatch), _VP]),
    ("wg_hs_cookies_get", _I, [_VP, _U32, _U32, _VP, _VP]),
    ("wg_hs_cookies_set", _I, [_VP, _U32, _U32, _VP, _VP]),
    ("wg_hs_mac2", _I, [_VP, ctypes.POINTER(WgHsMac2Batch), _VP]),
    ("wg_hs_rl_reserve", _I, [_VP, _U32]),
    ("wg_hs_rl_config_set", _I, [_VP, _U64, _U32]),
    ("wg_hs_ratelimit", _I, [_VP, ctypes.POINTER(WgHsRlBatch), _VP]),
    ("wg_hs_rl_compact", _I, [_VP, _VP, _VP, _VP]),
    ("wg_hs_rl_dump", _I, [_VP, _VP, _U32, ctypes.POINTER(_U32)]),
    ("wg_hs_rl_load", _I, [_VP, _VP, _U32]),
    ("wg_hs_rl_count", _I, [_VP, ctypes.POINTER(_U32), ctypes.POINTER(_U32)]),
    ("wg_rx_sessions_reserve", _I, [_VP, _U32]),
    ("wg_rx_sessions_retire", _I, [_VP, _VP, _U32, _VP, _VP]),
    ("wg_rx_sessions_count", _I, [_VP, ctypes.POINTER(_U32), ctypes.POINTER(_U32)]),
    ("wg_rx_sessions_compact", _I, [_VP, _U32, _VP, _VP]),
    ("wg_hs_install", _I, [_VP, ctypes.POINTER(WgHsInstallBatch), _VP]),
    ("wg_timers_reserve", _I, [_VP, _U32]),
    ("wg_timers_config_set", _I, [_VP, ctypes.POINTER(WgTimersConfig)]),
    ("wg_timers_peers_set", _I, [_VP, _U32, _U32, _VP]),
    ("wg_timers_get", _I, [_VP, _U32, _U32, _VP]),
    ("wg_timers_peers_get", _I, [_VP, _U32, _U32, _VP]),
    ("wg_timers_start", _I, [_VP, ctypes.POINTER(WgTimersStartBatch), _VP]),
    ("wg_timers_mark", _I, [_VP, ctypes.POINTER(WgTimersMarkBatch), _VP]),
    ("wg_timers_sweep", _I, [_VP, ctypes.POINTER(WgTimersSweepBatch), _VP]),
    ("wg_endpoints_reserve", _I, [_VP, _U32]),
    ("wg_endpoints_set", _I, [_VP, _U32, _U32, _VP]),
    ("wg_endpoints_get", _I, [_VP, _U32, _U32, _VP]),
    ("wg_endpoint_slots_set", _I, [_VP, _U32, _U32, _VP]),
    ("wg_endpoint_slots_get", _I, [_VP, _U32, _U32, _VP]),
    ("wg_endpoints_start", _I, [_VP, ctypes.POINTER(WgEndpointsStartBatch), _VP]),
    ("wg_endpoints_learn", _I, [_VP, ctypes.POINTER(WgEndpointsLearnBatch), _VP]),
    ("wg_tx_sendlist", _I, [_VP, ctypes.POINTER(WgTxSendlistBatch), _VP]),
    ("wg_hs_sendlist", _I, [_VP, ctypes.POINTER(WgHsSendlistBatch), _VP]),
    ("wg_seal1", _I, [_VP, _U32, _U64, _VP, _U32, _VP]),
    ("wg_open1", _I, [_VP, _U32, _U64, _VP, _U32, _VP]),
    ("wg_pp_config", _I, [_VP, _U32, _U32]),
    ("wg_pp_last_call", _I, [ctypes.POINTER(_U64), _U32]),
    ("wg_batcher_config", _I, [_VP, _U32, _U32]),
    ("wg_batcher_stats", _I, [_VP, ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    ("wg_queue_create", _I, [_VP, _I, _U32, _U32, _U32, ctypes.POINTER(_VP)]),
    ("wg_queue_destroy", _I, [_VP]),
    ("wg_submit_seal", _I, [_VP, _U32, _U64, _VP, _U32, _U64]),
    ("wg_submit_open", _I, [_VP, _U32, _U64, _VP, _U32, _U64]),
    ("wg_submit_seal_n", _I, [_VP, ctypes.POINTER(WgSubmit), _U32]),
    ("wg_submit_open_n", _I, [_VP, ctypes.POINTER(WgSubmit), _U32]),
    ("wg_reap", _I, [_VP, ctypes.POINTER(WgCompletion), _U32, _U32]),
    ("wg_reap_done", _I, [_VP, ctypes.POINTER(WgCompletion), _U32]),
    ("wg_queue_stats", _I, [_VP, ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    ("wg_queue_set_submit_timeout", _I, [_VP, _U32]),
    ("wg_queue_key_residue", _U32, [_VP]),
    ("wg_seal_host", _I, [_VP, _VP, _U32, _VP, _U64, _VP, _U64, _U32, _U32]),
    ("wg_open_host", _I, [_VP, _VP, _U32, _VP, _U64, _VP, _U64, _VP, _U32, _U32]),
    ("wg_host_alloc", _I, [_VP, _U64, ctypes.POINTER(_VP)]),
    ("wg_host_free", _I, [_VP, _VP]),
    ("wg_host_register", _I, [_VP, _VP, _U64]),
    ("wg_host_unregister", _I, [_VP, _VP]),
    ("wg_aead_host", _I, [_VP, _I, _VP, _U32, _VP, _U32, _VP, _U64, _VP, _U64, _VP, _U64, _VP]),
    ("wg_timing_enable", _I, [_VP, _I]),
    ("wg_timing_read", _I, [_VP, ctypes.POINTER(_D), ctypes.POINTER(_U64)]),
]

_lib = None
_lock = threading.Lock()


def lib() -> ctypes.CDLL:
    """Load libwgaead.so (once). Raises WgError(EDEVICE) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise WgError(WG_EDEVICE, f"{LIB_PATH} not built (run `make -C wireguard-java_amd/csrc`)")
            L = ctypes.CDLL(LIB_PATH)
            for name, res, args in SIGNATURES:
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            _lib = L
    return _lib


def last_error() -> str:
    msg = lib().wg_last_error()
    return msg.decode() if msg else ""


def check(rc: int) -> int:
    if rc < 0:
        raise WgError(rc, last_error())
    return rc
