"""Device context and the batched transport API over libwgaead.

``Engine`` owns one ``wg_ctx`` (one HIP device, its stream and device key
table). It is the MI355X-side counterpart of the reference's per-packet
ForkJoinPool dispatch (TransportManager.java:41,70-93,137-158): packets are
sealed/opened in batches that stay resident in HBM.

Descriptors are ``wg_pkt`` records (include/wgaead.h). On the torch side a
batch of them is an int64 tensor of shape [n, 4]: (in_off, out_off, counter,
len | key_slot << 32) — byte-identical to the C struct array.
"""
from __future__ import annotations

import ctypes
import threading

import numpy as np

from . import _lib as L

WG_PKT_DTYPE = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("counter", "<u8"), ("len", "<u4"),
                         ("key_slot", "<u4")])


def pack_desc(in_off, out_off, counter, length, key_slot) -> np.ndarray:
    """Build a wg_pkt array (numpy structured) from per-packet columns."""
    n = len(np.atleast_1d(in_off))
    d = np.zeros(n, WG_PKT_DTYPE)
    d["in_off"], d["out_off"], d["counter"] = in_off, out_off, counter
    d["len"], d["key_slot"] = length, key_slot
    return d


WG_AEAD_DTYPE = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("aad_off", "<u8"), ("len", "<u4"),
                          ("aad_len", "<u4"), ("key_slot", "<u4"), ("ctr0", "<u4"), ("nonce", "<u4", (3,)),
                          ("_reserved", "<u4", (3,))])


WG_B2S_DTYPE = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("key_off", "<u8"), ("len", "<u4"), ("outlen", "u1"),
                         ("keylen", "u1"), ("_pad", "u1", (2,))])
WG_HS_RECORD_DTYPE = np.dtype([("index", "<u4"), ("len", "<u4"), ("msg", "u1", (148,)), ("_pad", "<u4")])
WG_HS_INIT_DTYPE = np.dtype([("index", "<u4"), ("record", "<u4"), ("sender_index", "<u4"), ("peer", "<u4"),
                             ("remote_ephemeral", "u1", (32,)), ("remote_static", "u1", (32,)), ("hash", "u1", (32,)),
                             ("chain_key", "u1", (32,))])
WG_HS_SESSION_DTYPE = np.dtype([("index", "<u4"), ("init", "<u4"), ("peer", "<u4"), ("local_index", "<u4"),
                                ("response", "u1", (92,)), ("remote_index", "<u4"), ("send_key", "u1", (32,)),
                                ("recv_key", "u1", (32,))])
WG_HS_PENDING_DTYPE = np.dtype([("state", "<u4"), ("peer", "<u4"), ("local_index", "<u4"), ("_zero", "<u4"),
                                ("ephemeral", "u1", (32,)), ("hash", "u1", (32,)), ("chain_key", "u1", (32,))])
WG_HS_ESTABLISHED_DTYPE = np.dtype([("index", "<u4"), ("record", "<u4"), ("pending", "<u4"), ("peer", "<u4"),
                                    ("local_index", "<u4"), ("remote_index", "<u4"), ("_zero", "<u4", (2,)),
                                    ("send_key", "u1", (32,)), ("recv_key", "u1", (32,))])
WG_HS_SRC_DTYPE = np.dtype([("addr", "u1", (16,)), ("port", "u1", (2,)), ("family", "u1"), ("_pad", "u1", (5,))])
WG_HS_COOKIE_REPLY_DTYPE = np.dtype([("index", "<u4"), ("len", "<u4"), ("msg", "u1", (64,)), ("_pad", "<u4", (2,))])
WG_HS_LEARNED_DTYPE = np.dtype([("index", "<u4"), ("pending", "<u4"), ("peer", "<u4"), ("_zero", "<u4")])
WG_HS_RL_ENTRY_DTYPE = np.dtype([("addr", "u1", (8,)), ("family", "u1"), ("_pad", "u1", (7,)), ("tokens", "<u8"),
                                 ("last", "<u8")])
WG_TX_ITEM_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("key_slot", "<u4"), ("peer", "<u4"), ("index", "<u4"),
                             ("dst", WG_HS_SRC_DTYPE)])
WG_TIMER_SLOT_DTYPE = np.dtype([("state", "<u4"), ("peer", "<u4"), ("local_index", "<u4"), ("partner", "<u4"),
                                ("born", "<u8"), ("last", "<u8"), ("last_data", "<u8"), ("superseded", "<u8")])
WG_TIMER_PEER_DTYPE = np.dtype([("keepalive_interval", "<u8"), ("flags", "<u4"), ("_zero", "<u4")])
WG_TIMER_PEER_STATE_DTYPE = np.dtype([("current", "<u4"), ("flags", "<u4"), ("keepalive_interval", "<u8"),
                                      ("rekey_listed", "<u8")])
WG_TIMER_EXPIRED_DTYPE = np.dtype([("send_slot", "<u4"), ("recv_slot", "<u4"), ("peer", "<u4"), ("local_index", "<u4")])


class TimersConfig:
    """wg_timers_config: the session timers' limits, times in ticks, 0 = off."""
    FIELDS = ("rekey_after_time", "reject_after_time", "rekey_timeout", "keepalive_timeout", "linger",
              "rekey_after_messages", "reject_after_messages", "flags")

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, int(kw.pop(f, 0)))
        if kw:
            raise TypeError(f"unknown timers fields {sorted(kw)}")

    @classmethod
    def reference(cls, ticks_per_s: int) -> "TimersConfig":
        """The reference's rules: a session expires 120 s after its creation (EstablishedSession.java:28,:114), which
        only makes the node initiate again (SessionManager.java:92-111), and a failed attempt is retried after 5 s
        (SessionManager.java:188). It never stops using a session: everything else is off."""
        return cls(rekey_after_time=120 * ticks_per_s, rekey_timeout=5 * ticks_per_s)

    @classmethod
    def wireguard(cls, ticks_per_s: int) -> "TimersConfig":
        """WireGuard's constants: REKEY_AFTER_TIME 120 s, REJECT_AFTER_TIME 180 s, REKEY_TIMEOUT 5 s, KEEPALIVE_TIMEOUT
        10 s, a superseded session lingers for 180 s, REKEY_AFTER_MESSAGES 2^60, REJECT_AFTER_MESSAGES 2^64 - 2^13 - 1;
        only the initiator of a session rekeys it."""
        t = ticks_per_s
        return cls(rekey_after_time=120 * t, reject_after_time=180 * t, rekey_timeout=5 * t, keepalive_timeout=10 * t,
                   linger=180 * t, rekey_after_messages=1 << 60, reject_after_messages=(1 << 64) - (1 << 13) - 1,
                   flags=L.WG_TIMERS_INITIATOR_ONLY)

    def as_struct(self) -> "L.WgTimersConfig":
        return L.WgTimersConfig(*(getattr(self, f) for f in self.FIELDS))


class RateLimitConfig:
    """The handshake rate limiter's two numbers (wg_hs_rl_config_set): `cost` ticks per handshake, `burst` handshakes."""

    def __init__(self, cost: int, burst: int):
        self.cost, self.burst = int(cost), int(burst)

    @classmethod
    def wireguard(cls, ticks_per_second: int) -> "RateLimitConfig":
        """WireGuard's constants: 20 handshakes per second and source, a burst of 5."""
        return cls(ticks_per_second // 20, 5)

    @property
    def max(self) -> int:
        return self.cost * self.burst


def pack_b2s_desc(in_off, out_off, key_off, length, outlen, keylen) -> np.ndarray:
    """Build a wg_b2s_desc array (numpy structured) from per-message columns."""
    n = len(np.atleast_1d(in_off))
    d = np.zeros(n, WG_B2S_DTYPE)
    d["in_off"], d["out_off"], d["key_off"] = in_off, out_off, key_off
    d["len"], d["outlen"], d["keylen"] = length, outlen, keylen
    return d


WG_X25519_DTYPE = np.dtype([("scalar_off", "<u8"), ("point_off", "<u8"), ("out_off", "<u8"), ("flags", "<u4"),
                            ("_pad", "<u4")])


def pack_x25519_desc(scalar_off, point_off, out_off, flags=0) -> np.ndarray:
    """Build a wg_x25519_desc array (numpy structured) from per-operand columns."""
    n = len(np.atleast_1d(scalar_off))
    d = np.zeros(n, WG_X25519_DTYPE)
    d["scalar_off"], d["point_off"], d["out_off"], d["flags"] = scalar_off, point_off, out_off, flags
    return d


def desc_as_int64(d: np.ndarray) -> np.ndarray:
    """wg_pkt array viewed as int64 [n, 4] (for torch.from_numpy)."""
    d = np.ascontiguousarray(d)
    return d.view(np.int64).reshape(-1, d.dtype.itemsize // 8)


class Engine:
    """One HIP device: stream, key table (``key_slots`` x 32 bytes) and batch entry points."""

    def __init__(self, device: int = 0, key_slots: int = 1024):
        self._lib = L.lib()
        ctx = ctypes.c_void_p()
        L.check(self._lib.wg_ctx_create(device, key_slots, ctypes.byref(ctx)))
        self.ctx = ctx
        self.device = device
        self.key_slots = key_slots
        self._free = set(range(key_slots))
        self._slot_lock = threading.Lock()
        self._pinned = {}

    # ---- lifecycle --------------------------------------------------------------
    def close(self):
        if self.ctx:
            for p in self._pinned.values():
                self._lib.wg_host_free(self.ctx, p)
            self._pinned.clear()
            self._lib.wg_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_kernel(self, name: str | None = "default", lanes: int = 0, variant: int = 0) -> None:
        """Transport kernel for this engine's seal/open calls (wg_ctx_set_kernel): "default"
        (k_transport), "wave1" (the round-1 kernel) or "tile"; every kernel computes the
        same bytes, only the speed differs."""
        L.check(self._lib.wg_ctx_set_kernel(self.ctx, None if name is None else name.encode(), lanes, variant))

    @property
    def stream(self) -> int:
        return self._lib.wg_ctx_stream(self.ctx)

    def sync(self, stream: int | None = None):
        L.check(self._lib.wg_sync(self.ctx, stream))

    # ---- keys (SymmetricKeypair.java:39-50, 85-93) ------------------------------
    def alloc_slots(self, n: int) -> list[int]:
        """Claim n free key slots (lowest first). Callers upload each slot's key on its
        own (set_keys(slot, key)): claimed slots need not be adjacent after frees."""
        with self._slot_lock:
            if len(self._free) < n:
                raise L.WgError(L.WG_ERANGE, "key table full")
            got = sorted(self._free)[:n]
            self._free.difference_update(got)
            return got

    def free_slots(self, slots):
        """Zero and release slots claimed with alloc_slots (SymmetricKeypair.clean). A slot
        that is not currently claimed is an error, so a double release cannot hand one
        slot to two keypairs."""
        with self._slot_lock:
            bad = [s for s in slots if s in self._free or not 0 <= s < self.key_slots]
            if bad or len(set(slots)) != len(slots):
                raise L.WgError(L.WG_EINVAL, f"key slots {slots} are not all claimed")
        for s in slots:
            self.zero_keys(s, 1)
        with self._slot_lock:
            self._free.update(slots)

    def set_keys(self, first_slot: int, keys) -> None:
        k = np.ascontiguousarray(np.frombuffer(bytes(keys), np.uint8) if not isinstance(keys, np.ndarray) else keys,
                                 dtype=np.uint8)
        assert k.size % 32 == 0
        L.check(self._lib.wg_keys_set(self.ctx, first_slot, k.size // 32, k.ctypes.data))

    def zero_keys(self, first_slot: int, n: int) -> None:
        L.check(self._lib.wg_keys_zero(self.ctx, first_slot, n))

    # ---- device-resident batches (torch tensors on this device) -------------------
    def seal(self, desc, inp, out, max_len: int, uniform: bool = False, stream: int | None = None,
             frame: bool = False):
        """wg_seal_batch over torch tensors: desc int64 [n,4], inp/out uint8 (device).
        frame=True also writes each packet's transport header (WG_F_FRAME)."""
        n = desc.shape[0]
        flags = (L.WG_F_UNIFORM if uniform else 0) | (L.WG_F_FRAME if frame else 0)
        L.check(self._lib.wg_seal_batch(self.ctx, desc.data_ptr(), n, inp.data_ptr(), inp.numel(), out.data_ptr(),
                                        out.numel(), max_len, flags,
                                        stream if stream is not None else _torch_stream()))

    def open(self, desc, inp, out, status, max_len: int, uniform: bool = False, stream: int | None = None,
             rx_filter: bool = False):
        """wg_open_batch; `status` is an int32/uint32 device tensor of n entries (0 ok, 1 bad tag).
        rx_filter (WG_F_RX_FILTER): the receive-side keepalive / IP / AllowedIPs verdict of
        wg_rx_check(WG_RX_FILTER) written by the open kernel itself."""
        n = desc.shape[0]
        flags = (L.WG_F_UNIFORM if uniform else 0) | (L.WG_F_RX_FILTER if rx_filter else 0)
        L.check(self._lib.wg_open_batch(self.ctx, desc.data_ptr(), n, inp.data_ptr(), inp.numel(), out.data_ptr(),
                                        out.numel(), status.data_ptr(), max_len, flags,
                                        stream if stream is not None else _torch_stream()))

    def duplex(self, seal_desc, seal_in, seal_out, seal_max_len: int, open_desc, open_in, open_out, status,
               open_max_len: int, uniform: bool = False, frame: bool = False, stream: int | None = None,
               after_seal: bool = False):
        """wg_duplex_batch: seal one batch and open another in one launch. Without after_seal the
        open batch must not read what the seal batch writes; with it (WG_F_AFTER_SEAL) open packet i
        is ordered after seal packet i (k_step for uniform batches). Same tensors as seal() / open()."""
        u = L.WG_F_UNIFORM if uniform else 0
        sb = L.WgBatch(seal_desc.data_ptr(), seal_in.data_ptr(), seal_out.data_ptr(), None, seal_in.numel(),
                       seal_out.numel(), seal_desc.shape[0], seal_max_len, u | (L.WG_F_FRAME if frame else 0), 0)
        ob = L.WgBatch(open_desc.data_ptr(), open_in.data_ptr(), open_out.data_ptr(),
                       status.data_ptr() if status is not None else None, open_in.numel(), open_out.numel(),
                       open_desc.shape[0], open_max_len, u | (L.WG_F_AFTER_SEAL if after_seal else 0), 0)
        L.check(self._lib.wg_duplex_batch(self.ctx, ctypes.byref(sb), ctypes.byref(ob),
                                          stream if stream is not None else _torch_stream()))

    def prepare_duplex(self, seal_desc, seal_in, seal_out, seal_max_len: int, open_desc, open_in, open_out, status,
                       open_max_len: int, uniform: bool = False, after_seal: bool = False, stream: int | None = None):
        """The same wg_duplex_batch call as duplex(), with its argument structs built once: returns a
        zero-argument callable that issues the launch on `stream` (default: torch's current stream when
        prepared). A caller that re-launches one batch layout over and over (a pipeline stage, a bench
        step) so pays one foreign call per launch instead of rebuilding the arguments. The tensors must
        stay alive and in place while the callable is used."""
        u = L.WG_F_UNIFORM if uniform else 0
        sb = L.WgBatch(seal_desc.data_ptr(), seal_in.data_ptr(), seal_out.data_ptr(), None, seal_in.numel(),
                       seal_out.numel(), seal_desc.shape[0], seal_max_len, u, 0)
        ob = L.WgBatch(open_desc.data_ptr(), open_in.data_ptr(), open_out.data_ptr(),
                       status.data_ptr() if status is not None else None, open_in.numel(), open_out.numel(),
                       open_desc.shape[0], open_max_len, u | (L.WG_F_AFTER_SEAL if after_seal else 0), 0)
        fn, ctx = self._lib.wg_duplex_batch, self.ctx
        ps, po = ctypes.byref(sb), ctypes.byref(ob)
        st = stream if stream is not None else _torch_stream()
        keep = (sb, ob, seal_desc, seal_in, seal_out, open_desc, open_in, open_out, status)

        def launch():
            rc = fn(ctx, ps, po, st)
            if rc < 0:
                L.check(rc)
            return keep  # (holds the structs and tensors for as long as the callable lives)
        return launch

    # ---- receive side after open (wg_rx_check) -------------------------------------
    def filter_set(self, filter_id: int, prefixes) -> None:
        """wg_filter_set from (address string or ipaddress object, prefix_len) pairs, as
        IPFilter.insert(InetAddress, int) takes them (util/IPFilter.java:30-42)."""
        import ipaddress
        arr = (L.WgPrefix * max(1, len(prefixes)))()
        for k, (addr, plen) in enumerate(prefixes):
            a = ipaddress.ip_address(addr) if isinstance(addr, str) else addr
            arr[k].family = 4 if a.version == 4 else 6
            arr[k].prefix_len = plen
            b = a.packed
            for i, x in enumerate(b):
                arr[k].addr[i] = x
        L.check(self._lib.wg_filter_set(self.ctx, filter_id, ctypes.addressof(arr), len(prefixes)))

    def slot_filters_set(self, first_slot: int, filter_ids) -> None:
        ids = np.ascontiguousarray(np.asarray(filter_ids, dtype=np.uint32))
        L.check(self._lib.wg_slot_filters_set(self.ctx, first_slot, len(ids), ids.ctypes.data))

    def replay_enable(self, window_bits: int = 8192) -> None:
        L.check(self._lib.wg_replay_enable(self.ctx, window_bits))

    def replay_reset(self, first_slot: int, n: int) -> None:
        L.check(self._lib.wg_replay_reset(self.ctx, first_slot, n))

    def replay_state(self, slot: int, window_bits: int):
        """(top, bitmap words as uint64 numpy array) of one key slot's window."""
        top = ctypes.c_uint64()
        bits = np.zeros(window_bits // 64, np.uint64)
        L.check(self._lib.wg_replay_state(self.ctx, slot, ctypes.byref(top), bits.ctypes.data, len(bits)))
        return top.value, bits

    def rx_check(self, desc, pt, status, flags: int = 1, stream: int | None = None) -> None:
        """wg_rx_check after open(desc, ..., out=pt, status) on the same stream."""
        n = desc.shape[0]
        L.check(self._lib.wg_rx_check(self.ctx, desc.data_ptr(), n, pt.data_ptr(), pt.numel(), status.data_ptr(),
                                      flags, stream if stream is not None else _torch_stream()))

    # ---- transmit side before seal (wg_tx_plan) ---------------------------------------
    def tx_peers_set(self, key_slots) -> None:
        """wg_tx_peers_set: the peers of broadcast mode as key slots, in PeerList iteration order
        (PeerList.java:94-106); list only peers with a session."""
        ids = np.ascontiguousarray(np.asarray(key_slots, dtype=np.uint32))
        L.check(self._lib.wg_tx_peers_set(self.ctx, ids.ctypes.data, len(ids)))

    def routes_set(self, routes) -> None:
        """wg_routes_set: the whole cryptokey-routing table from (address string or ipaddress
        object, prefix_len, key_slot) triples; longest prefix wins, of equal prefixes the later."""
        import ipaddress
        arr = (L.WgPrefix * max(1, len(routes)))()
        slots = np.zeros(max(1, len(routes)), np.uint32)
        for k, (addr, plen, slot) in enumerate(routes):
            a = ipaddress.ip_address(addr) if isinstance(addr, str) else addr
            arr[k].family = 4 if a.version == 4 else 6
            arr[k].prefix_len = plen
            for i, x in enumerate(a.packed):
                arr[k].addr[i] = x
            slots[k] = slot
        L.check(self._lib.wg_routes_set(self.ctx, ctypes.addressof(arr), slots.ctypes.data, len(routes)))

    def tx_counters_set(self, first_slot: int, counters) -> None:
        """wg_tx_counters_set: the send counters of slots [first_slot, first_slot + len(counters))."""
        v = np.ascontiguousarray(np.asarray(counters, dtype=np.uint64))
        L.check(self._lib.wg_tx_counters_set(self.ctx, first_slot, len(v), v.ctypes.data))

    def tx_counters_get(self, first_slot: int, n: int) -> np.ndarray:
        """wg_tx_counters_get: the send counters after every plan queued so far (uint64 array)."""
        v = np.zeros(max(n, 1), np.uint64)
        L.check(self._lib.wg_tx_counters_get(self.ctx, first_slot, n, v.ctypes.data))
        return v[:n]

    def tx_reserve(self, max_packets: int) -> None:
        """wg_tx_reserve: scratch for plans of up to max_packets tun packets (needed before a plan
        is captured into a graph: a capturing stream cannot allocate)."""
        L.check(self._lib.wg_tx_reserve(self.ctx, max_packets))

    def tx_plan(self, tun, pkt_off, pkt_len, desc_out, tx_status, wire_stride: int, out_size: int, max_len: int,
                route: bool = False, wire_base: int = 0, stream: int | None = None) -> None:
        """wg_tx_plan over torch tensors: tun uint8 ring, pkt_off int64 [n], pkt_len int32 [n],
        desc_out int64 [n_desc, 4] (wg_pkt records for seal()), tx_status int32 [n_desc]; n_desc = n in
        route mode, n x peers in broadcast mode. Wire slot j is out[wire_base + j * wire_stride ...) of the
        seal's output buffer of out_size bytes; the send counters live on the device."""
        b = L.WgTxBatch(tun.data_ptr(), tun.numel(), pkt_off.data_ptr(), pkt_len.data_ptr(), desc_out.data_ptr(),
                        tx_status.data_ptr(), wire_base, wire_stride, out_size, pkt_off.shape[0], max_len,
                        L.WG_TX_ROUTE if route else L.WG_TX_BROADCAST, 0)
        L.check(self._lib.wg_tx_plan(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    def tx_seal(self, tun, pkt_off, pkt_len, desc_out, tx_status, out, wire_stride: int, max_len: int,
                route: bool = False, wire_base: int = 0, uniform: bool = False, stream: int | None = None) -> None:
        """tun ring -> UDP ring on one stream: tx_plan, then seal(desc_out, tun, out, frame=True). The
        receiver table (set_receivers) must be set; packets the plan rejects leave their wire slot untouched."""
        st = stream if stream is not None else _torch_stream()
        self.tx_plan(tun, pkt_off, pkt_len, desc_out, tx_status, wire_stride, out.numel(), max_len, route=route,
                     wire_base=wire_base, stream=st)
        self.seal(desc_out, tun, out, max_len, uniform=uniform, stream=st, frame=True)

    # ---- receive side around open (wg_rx_plan / wg_rx_deliver) ---------------------------
    def rx_sessions_set(self, indices, key_slots) -> None:
        """wg_rx_sessions_set: the whole receiver index -> key slot table (PeerList.java:53-67,
        TransportManager.java:70-77); an empty list clears it."""
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.uint32))
        ks = np.ascontiguousarray(np.asarray(key_slots, dtype=np.uint32))
        if len(idx) != len(ks):
            raise L.WgError(L.WG_EINVAL, f"{len(idx)} receiver indices for {len(ks)} key slots")
        L.check(self._lib.wg_rx_sessions_set(self.ctx, idx.ctypes.data, ks.ctypes.data, len(idx)))

    def rx_reserve(self, max_packets: int) -> None:
        """wg_rx_reserve: scratch for receive plans / delivers of up to max_packets packets (needed before
        one is captured into a graph: a capturing stream cannot allocate)."""
        L.check(self._lib.wg_rx_reserve(self.ctx, max_packets))

    def rx_sessions_reserve(self, max_sessions: int) -> None:
        """wg_rx_sessions_reserve: a session table of fixed capacity (the smallest power of two >= max(16,
        4 max_sessions)) that hs_install() inserts into and rx_sessions_retire() retires from, and the install's
        scratch; the current live entries are kept. Needed before hs_install()."""
        L.check(self._lib.wg_rx_sessions_reserve(self.ctx, max_sessions))

    def rx_sessions_retire(self, indices, n_retired=None, stream: int | None = None) -> None:
        """wg_rx_sessions_retire over torch tensors: indices int32 [n] (receiver indices; the live ones become
        retired entries), n_retired int32 [1] or None (how many the call retired). Asynchronous."""
        L.check(self._lib.wg_rx_sessions_retire(self.ctx, indices.data_ptr() if indices.shape[0] else None,
                                                indices.shape[0], n_retired.data_ptr() if n_retired is not None else None,
                                                stream if stream is not None else _torch_stream()))

    def rx_sessions_count(self) -> tuple[int, int]:
        """wg_rx_sessions_count: (live, retired) entries of the session table, after everything queued."""
        live, retired = ctypes.c_uint32(), ctypes.c_uint32()
        L.check(self._lib.wg_rx_sessions_count(self.ctx, ctypes.byref(live), ctypes.byref(retired)))
        return live.value, retired.value

    def rx_sessions_compact(self, min_retired: int = 1, summary=None, stream: int | None = None) -> None:
        """wg_rx_sessions_compact: if the session table holds at least max(min_retired, 1) retired entries it is
        rebuilt on the device from its live ones (used == count afterwards); summary int32 [4] or None (live,
        dropped, compacted, 0). Asynchronous and capturable. Needs rx_sessions_reserve()."""
        L.check(self._lib.wg_rx_sessions_compact(self.ctx, min_retired, summary.data_ptr() if summary is not None else None,
                                                 stream if stream is not None else _torch_stream()))

    def hs_install(self, entries, summary_n, send_slot, recv_slot, inst_status, summary, slot_first: int,
                   slot_count: int, source: int, receivers=None, wipe: bool = True, stream: int | None = None,
                   compact: bool = False) -> None:
        """wg_hs_install over torch tensors: entries uint8 [n, 176] as hs_respond() wrote its sessions (source
        WG_HS_INSTALL_SESSIONS) or [n, 96] as hs_finish() wrote established (WG_HS_INSTALL_ESTABLISHED); summary_n
        that call's summary, int32 [4], whose n_ok is read on the device (None: all n entries); send_slot /
        recv_slot int32 [n_slots], the key slots by position (sessions[j].init / established[j].pending);
        inst_status int32 [n] (WG_HS_INST_*); summary int32 [4] (n_ok, n_badslot, n_dup, n_full); [slot_first,
        slot_first + slot_count) the key slots the call may write (seal1 / open1 / the queues refuse them
        afterwards); receivers the int32 table of set_receivers(), or None; wipe zeroes the installed entries'
        keys; compact rebuilds the session table from its live entries first when the ring would not fit beside the
        retired ones (WG_HS_INSTALL_COMPACT). Needs rx_sessions_reserve(). The next tx_plan / rx_plan on the same
        stream uses the sessions."""
        n_entries = summary_n.data_ptr() if summary_n is not None else None  # n_ok is the summaries' first word
        b = L.WgHsInstallBatch(entries.data_ptr(), n_entries, send_slot.data_ptr() if send_slot.shape[0] else None,
                               recv_slot.data_ptr() if recv_slot.shape[0] else None,
                               receivers.data_ptr() if receivers is not None else None, inst_status.data_ptr(),
                               summary.data_ptr(), entries.shape[0], send_slot.shape[0], slot_first, slot_count, source,
                               (L.WG_HS_INSTALL_WIPE if wipe else 0) | (L.WG_HS_INSTALL_COMPACT if compact else 0))
        L.check(self._lib.wg_hs_install(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    # ---- session timers (wg_timers_*) --------------------------------------------------------
    def timers_reserve(self, max_peers: int) -> None:
        """wg_timers_reserve: the timer records of every key slot and of max_peers peers, the transmit state and the
        sweep's scratch. Needed before every other timers_* call."""
        L.check(self._lib.wg_timers_reserve(self.ctx, max_peers))

    def timers_config_set(self, config: "TimersConfig") -> None:
        """wg_timers_config_set: a TimersConfig; captured calls see it without re-capture."""
        c = config.as_struct()
        L.check(self._lib.wg_timers_config_set(self.ctx, ctypes.byref(c)))

    def timers_peers_set(self, first_peer: int, peers) -> None:
        """wg_timers_peers_set: peers = [(keepalive_interval, can_initiate), ...] from first_peer on."""
        v = np.zeros(len(peers), WG_TIMER_PEER_DTYPE)
        for k, (interval, can) in enumerate(peers):
            v[k] = (interval, L.WG_TIMER_PEER_CAN_INITIATE if can else 0, 0)
        L.check(self._lib.wg_timers_peers_set(self.ctx, first_peer, len(v), v.ctypes.data if len(v) else None))

    def timers_get(self, first_slot: int, n: int) -> np.ndarray:
        """wg_timers_get: the timer records of key slots [first_slot, first_slot + n), after everything queued
        (WG_TIMER_SLOT_DTYPE array)."""
        v = np.zeros(max(n, 1), WG_TIMER_SLOT_DTYPE)
        L.check(self._lib.wg_timers_get(self.ctx, first_slot, n, v.ctypes.data))
        return v[:n]

    def timers_peers_get(self, first_peer: int, n: int) -> np.ndarray:
        """wg_timers_peers_get: the peers' timer records (WG_TIMER_PEER_STATE_DTYPE array)."""
        v = np.zeros(max(n, 1), WG_TIMER_PEER_STATE_DTYPE)
        L.check(self._lib.wg_timers_peers_get(self.ctx, first_peer, n, v.ctypes.data))
        return v[:n]

    def timers_start(self, entries, summary_n, inst_status, send_slot, recv_slot, now, source: int,
                     stream: int | None = None) -> None:
        """wg_timers_start over the tensors hs_install() was given, behind it on the same stream; now int64 [1]."""
        b = L.WgTimersStartBatch(entries.data_ptr(), summary_n.data_ptr() if summary_n is not None else None,
                                 inst_status.data_ptr(), send_slot.data_ptr() if send_slot.shape[0] else None,
                                 recv_slot.data_ptr() if recv_slot.shape[0] else None, now.data_ptr(), entries.shape[0],
                                 send_slot.shape[0], source, 0)
        L.check(self._lib.wg_timers_start(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    def timers_mark(self, desc, status, now, summary, tx: bool = False, gate: bool = False, slot_first: int = 0,
                    slot_count: int = 0, stream: int | None = None) -> None:
        """wg_timers_mark over torch tensors: desc int64 [n, 4] and status int32 [n] as rx_deliver() (final_status) or
        tx_plan() left them, now int64 [1], summary int32 [2] (n_marked, n_refused). tx=True with gate=True refuses
        descriptors on dead or worn-out sessions of key slots [slot_first, slot_first + slot_count) before the seal."""
        n = desc.shape[0]
        b = L.WgTimersMarkBatch(desc.data_ptr() if n else None, status.data_ptr() if n else None, now.data_ptr(),
                                summary.data_ptr(), n, L.WG_TIMERS_TX if tx else L.WG_TIMERS_RX,
                                L.WG_TIMERS_GATE if gate else 0, slot_first, slot_count, 0)
        L.check(self._lib.wg_timers_mark(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    def timers_sweep(self, now, expired, initiate, keepalives, summary, wire_stride: int = 0, out_size: int = 0,
                     wire_base: int = 0, retire: bool = False, stream: int | None = None, wipe: bool = False) -> None:
        """wg_timers_sweep over torch tensors: expired int32 [cap, 4] (send slot, recv slot, peer, local index),
        initiate int32 [cap] (hs_initiate()'s peer array, padded with -1), keepalives int64 [cap, 4] (wg_pkt records for
        seal(frame=True) into wire slots of wire_stride bytes of a ring of out_size bytes), summary int32 [8]
        (expired due / listed, initiate due / listed, keepalives due / listed, live sessions, 0). wipe (with retire
        only) zeroes both keys of every session the sweep retires (WG_TIMERS_WIPE)."""
        b = L.WgTimersSweepBatch(now.data_ptr(), expired.data_ptr() if expired.shape[0] else None,
                                 initiate.data_ptr() if initiate.shape[0] else None,
                                 keepalives.data_ptr() if keepalives.shape[0] else None, summary.data_ptr(), wire_base,
                                 wire_stride, out_size, expired.shape[0], initiate.shape[0], keepalives.shape[0],
                                 (L.WG_TIMERS_RETIRE if retire else 0) | (L.WG_TIMERS_WIPE if wipe else 0))
        L.check(self._lib.wg_timers_sweep(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    def timers_tick(self, now, expired, initiate, keepalives, summary, out, wire_stride: int, wire_base: int = 0,
                    retire: bool = True, stream: int | None = None, wipe: bool = False) -> None:
        """The tick on one stream, next to rx_open and tx_seal: timers_sweep, then the keepalives it listed are sealed
        and framed into `out` (the sweep pads the list with descriptors the seal skips: nothing is read back). The receiver table
        (set_receivers) must be set."""
        st = stream if stream is not None else _torch_stream()
        self.timers_sweep(now, expired, initiate, keepalives, summary, wire_stride=wire_stride, out_size=out.numel(),
                          wire_base=wire_base, retire=retire, stream=st, wipe=wipe)
        if keepalives.shape[0]:
            self.seal(keepalives, out, out, 16, stream=st, frame=True)

    # ---- endpoints and send lists (wg_endpoints_*, wg_tx_sendlist, wg_hs_sendlist) --------------
    def endpoints_reserve(self, max_peers: int) -> None:
        """wg_endpoints_reserve: one endpoint per peer, one peer per key slot, and the send lists' scratch. Needed
        before every other endpoints_* / *_sendlist call."""
        L.check(self._lib.wg_endpoints_reserve(self.ctx, max_peers))

    def endpoints_set(self, first_peer: int, endpoints) -> None:
        """wg_endpoints_set: endpoints = a WG_HS_SRC_DTYPE array, or a list of (address string or ipaddress object,
        port) pairs and None (no endpoint), from first_peer on. Captured calls see them without re-capture."""
        if isinstance(endpoints, np.ndarray):
            v = np.ascontiguousarray(endpoints, dtype=WG_HS_SRC_DTYPE)
        else:
            import ipaddress
            v = np.zeros(len(endpoints), WG_HS_SRC_DTYPE)
            for k, e in enumerate(endpoints):
                if e is None:
                    continue
                a = ipaddress.ip_address(e[0]) if isinstance(e[0], str) else e[0]
                v["addr"][k, :len(a.packed)] = np.frombuffer(a.packed, np.uint8)
                v["port"][k] = (e[1] >> 8, e[1] & 255)
                v["family"][k] = 4 if a.version == 4 else 6
        L.check(self._lib.wg_endpoints_set(self.ctx, first_peer, len(v), v.ctypes.data if len(v) else None))

    def endpoints_get(self, first_peer: int, n: int) -> np.ndarray:
        """wg_endpoints_get: the endpoints of peers [first_peer, first_peer + n), after everything queued
        (WG_HS_SRC_DTYPE array; family 0: none)."""
        v = np.zeros(max(n, 1), WG_HS_SRC_DTYPE)
        L.check(self._lib.wg_endpoints_get(self.ctx, first_peer, n, v.ctypes.data))
        return v[:n]

    def endpoint_slots_set(self, first_slot: int, peers) -> None:
        """wg_endpoint_slots_set: the peers of key slots [first_slot, first_slot + len(peers)), for sessions keyed
        with set_keys() (hs_install() + endpoints_start() set them on the device)."""
        v = np.ascontiguousarray(np.asarray(peers, dtype=np.uint32))
        L.check(self._lib.wg_endpoint_slots_set(self.ctx, first_slot, len(v), v.ctypes.data if len(v) else None))

    def endpoint_slots_get(self, first_slot: int, n: int) -> np.ndarray:
        """wg_endpoint_slots_get: the key slots' peers (uint32 array; WG_HS_NOPEER: none)."""
        v = np.zeros(max(n, 1), np.uint32)
        L.check(self._lib.wg_endpoint_slots_get(self.ctx, first_slot, n, v.ctypes.data))
        return v[:n]

    def endpoints_start(self, entries, summary_n, inst_status, send_slot, recv_slot, src, summary, source: int,
                        learn_response: bool = False, stream: int | None = None) -> None:
        """wg_endpoints_start over the tensors hs_install() was given, behind it on the same stream; src uint8
        [n_src, 24] (the ring's wg_hs_src by batch index) or None, summary int32 [4] (sessions, learned, bad source,
        no peer)."""
        n_src = src.shape[0] if src is not None else 0
        b = L.WgEndpointsStartBatch(entries.data_ptr(), summary_n.data_ptr() if summary_n is not None else None,
                                    inst_status.data_ptr(), send_slot.data_ptr() if send_slot.shape[0] else None,
                                    recv_slot.data_ptr() if recv_slot.shape[0] else None, src.data_ptr() if n_src else None,
                                    summary.data_ptr(), entries.shape[0], send_slot.shape[0], n_src, source,
                                    L.WG_EP_LEARN_RESPONSE if learn_response else 0, 0)
        L.check(self._lib.wg_endpoints_start(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    def endpoints_learn(self, desc, final_status, src, roamed, summary, stream: int | None = None) -> None:
        """wg_endpoints_learn over torch tensors, after rx_deliver(): desc int64 [n, 4], final_status int32 [n], src
        uint8 [n, 24] by batch index, roamed int32 [cap] (the peers whose endpoint moved, ascending), summary int32 [4]
        (authentic, peers, roamed, bad source)."""
        n = desc.shape[0]
        b = L.WgEndpointsLearnBatch(desc.data_ptr() if n else None, final_status.data_ptr() if n else None,
                                    src.data_ptr() if n else None, roamed.data_ptr() if roamed.shape[0] else None,
                                    summary.data_ptr(), n, roamed.shape[0])
        L.check(self._lib.wg_endpoints_learn(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    def tx_sendlist(self, desc, status, items, summary, gate: bool = False, stream: int | None = None) -> None:
        """wg_tx_sendlist over torch tensors: desc int64 [n, 4] and status int32 [n] as tx_plan() left them (status
        None over timers_sweep()'s keepalives), items uint8 [n, 48] (wg_tx_item: off, len, key slot, peer, index,
        destination), summary int64 [2] (bytes, n_items | n_noendpoint << 32). gate=True, before the seal only, refuses
        the descriptors whose peer has no endpoint."""
        n = desc.shape[0]
        b = L.WgTxSendlistBatch(desc.data_ptr() if n else None, status.data_ptr() if n and status is not None else None,
                                items.data_ptr() if n else None, summary.data_ptr(), n, L.WG_SEND_GATE if gate else 0)
        L.check(self._lib.wg_tx_sendlist(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    def hs_sendlist(self, kind: int, entries, summary_n, items, summary, src=None, status=None, peer=None,
                    stream: int | None = None) -> None:
        """wg_hs_sendlist over torch tensors: kind WG_HS_SEND_RESPONSES (entries = hs_respond()'s sessions, src),
        WG_HS_SEND_INITIATIONS (entries = hs_initiate()'s records, with its status and peer) or
        WG_HS_SEND_COOKIE_REPLIES (entries = hs_admit()'s replies, src); summary_n the tensor whose first word is the
        entries' number on the device, or None; items uint8 [n, 48] with off relative to entries; summary int64 [2]
        (bytes, n_items | n_nodst << 32)."""
        n = entries.shape[0]
        n_src = src.shape[0] if src is not None else 0
        b = L.WgHsSendlistBatch(entries.data_ptr() if n else None, summary_n.data_ptr() if summary_n is not None else None,
                                status.data_ptr() if n and status is not None else None,
                                peer.data_ptr() if n and peer is not None else None, src.data_ptr() if n_src else None,
                                items.data_ptr() if n else None, summary.data_ptr(), n, n_src, kind, 0)
        L.check(self._lib.wg_hs_sendlist(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    def tx_send(self, tun, pkt_off, pkt_len, desc_out, tx_status, out, items, send_summary, wire_stride: int,
                max_len: int, route: bool = False, wire_base: int = 0, uniform: bool = False,
                stream: int | None = None) -> None:
        """tun ring -> UDP ring and its send list on one stream: tx_plan, tx_sendlist with the gate (a packet whose
        peer has no endpoint is not sealed), seal(frame=True). The host sends items[:n_items] with sendmmsg and reads
        nothing else back."""
        st = stream if stream is not None else _torch_stream()
        self.tx_plan(tun, pkt_off, pkt_len, desc_out, tx_status, wire_stride, out.numel(), max_len, route=route,
                     wire_base=wire_base, stream=st)
        self.tx_sendlist(desc_out, tx_status, items, send_summary, gate=True, stream=st)
        self.seal(desc_out, tun, out, max_len, uniform=uniform, stream=st, frame=True)

    def rx_plan(self, wire, pkt_off, pkt_len, desc_out, rx_status, host_list, summary, max_len: int,
                packed: bool = False, pt_base: int = 0, pt_size: int = 0, stream: int | None = None) -> None:
        """wg_rx_plan over torch tensors: wire uint8 UDP ring, pkt_off int64 [n], pkt_len int32 [n], desc_out
        int64 [n, 4] (wg_pkt records for open()), rx_status / host_list int32 [n], summary int64 [2]
        (wg_rx_summary: pt_used, n_open | n_host << 32). packed=False puts every plaintext right after its
        packet in `wire` (the reference's layout); packed=True packs them, 16-B aligned, from pt_base of the
        open's output buffer of pt_size bytes."""
        b = L.WgRxBatch(wire.data_ptr(), wire.numel(), pkt_off.data_ptr(), pkt_len.data_ptr(), desc_out.data_ptr(),
                        rx_status.data_ptr(), host_list.data_ptr(), summary.data_ptr(), pt_base, pt_size,
                        pkt_off.shape[0], max_len, L.WG_RX_PT_PACKED if packed else L.WG_RX_PT_AFTER, 0)
        L.check(self._lib.wg_rx_plan(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    def rx_deliver(self, desc, plan_status, open_status, final_status, items, delivered, index_out=None,
                   stream: int | None = None) -> None:
        """wg_rx_deliver over torch tensors: final_status int32 [n], items int64 [n, 2] (wg_rx_item: off,
        len | key_slot << 32), delivered int64 [2] (wg_rx_delivered: bytes, n_items | n_keepalive << 32),
        index_out int32 [n] or None."""
        b = L.WgRxDeliverBatch(desc.data_ptr(), plan_status.data_ptr(), open_status.data_ptr(),
                               final_status.data_ptr(), items.data_ptr(),
                               index_out.data_ptr() if index_out is not None else None, delivered.data_ptr(),
                               desc.shape[0], 0)
        L.check(self._lib.wg_rx_deliver(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    def rx_open(self, wire, pkt_off, pkt_len, desc_out, rx_status, host_list, summary, out, open_status,
                final_status, items, delivered, max_len: int, packed: bool = True, pt_base: int = 0,
                index_out=None, replay: bool = False, uniform: bool = False, stream: int | None = None) -> None:
        """UDP ring -> plaintext ring and tun list on one stream, the mirror of tx_seal: rx_plan, then
        open(desc_out, wire, out, open_status, rx_filter=True), rx_check(WG_RX_REPLAY) if `replay`, then
        rx_deliver. packed=False needs out to be the wire ring itself (plaintext after each packet)."""
        st = stream if stream is not None else _torch_stream()
        self.rx_plan(wire, pkt_off, pkt_len, desc_out, rx_status, host_list, summary, max_len, packed=packed,
                     pt_base=pt_base, pt_size=out.numel(), stream=st)
        self.open(desc_out, wire, out, open_status, max_len, uniform=uniform, stream=st, rx_filter=True)
        if replay:
            self.rx_check(desc_out, out, open_status, L.WG_RX_REPLAY, stream=st)
        self.rx_deliver(desc_out, rx_status, open_status, final_status, items, delivered, index_out=index_out,
                        stream=st)

    # ---- handshake admission (wg_blake2s_batch / wg_hs_check) -------------------------------
    def blake2s(self, desc, inp, out, status, stream: int | None = None) -> None:
        """wg_blake2s_batch over torch tensors: desc int64 [n, 4] (wg_b2s_desc records, pack_b2s_desc),
        inp / out uint8 (device, not overlapping), status int32 [n] (WG_B2S_*). Keys are read from inp."""
        n = desc.shape[0]
        L.check(self._lib.wg_blake2s_batch(self.ctx, desc.data_ptr(), n, inp.data_ptr(), inp.numel(), out.data_ptr(),
                                           out.numel(), status.data_ptr(),
                                           stream if stream is not None else _torch_stream()))

    def blake2s_host(self, messages) -> list[bytes]:
        """BLAKE2s of host byte strings through one wg_blake2s_batch call: messages = [(data, key,
        outlen)]; returns the digests. For the noise mirror and tests; a data path keeps its bytes on
        the device and calls blake2s()."""
        import torch
        if not messages:
            return []
        dev = torch.device("cuda", self.device)
        buf, rows, out_off = bytearray(), [], 0
        for data, key, outlen in messages:
            if not 1 <= outlen <= 32 or len(key) > 32:
                raise L.WgError(L.WG_EINVAL, "digest length must be in [1, 32], key length at most 32")
            rows.append((len(buf), out_off, len(buf) + len(data), len(data), outlen, len(key)))
            buf += bytes(data) + bytes(key)
            out_off += 32
        d = pack_b2s_desc(*(np.array(c, np.uint64) for c in zip(*rows)))
        d_desc = torch.from_numpy(desc_as_int64(d)).to(dev)
        d_in = torch.from_numpy(np.frombuffer(bytes(buf) + b"\0", np.uint8).copy()).to(dev)
        d_out = torch.zeros(out_off, dtype=torch.uint8, device=dev)
        d_st = torch.zeros(len(rows), dtype=torch.int32, device=dev)
        st = _torch_stream()
        self.blake2s(d_desc, d_in, d_out, d_st, stream=st)
        self.sync(st)
        if int(d_st.abs().sum().item()):
            raise L.WgError(L.WG_EINVAL, "wg_blake2s_batch refused a descriptor")
        out = d_out.cpu().numpy().tobytes()
        return [out[32 * k:32 * k + m[2]] for k, m in enumerate(messages)]

    def hs_key_set(self, static_public) -> None:
        """wg_hs_key_set: the mac1 key of the local static public key (32 bytes), derived on the device."""
        pub = np.frombuffer(bytes(static_public), np.uint8).copy()
        if pub.size != 32:
            raise L.WgError(L.WG_EINVAL, f"static public key of {pub.size} bytes")
        L.check(self._lib.wg_hs_key_set(self.ctx, pub.ctypes.data))

    def hs_reserve(self, max_messages: int) -> None:
        """wg_hs_reserve: scratch for checks, opens and responds of up to max_messages datagrams (needed before
        one is captured into a graph: a capturing stream cannot allocate)."""
        L.check(self._lib.wg_hs_reserve(self.ctx, max_messages))

    def hs_check(self, wire, pkt_off, pkt_len, hs_status, records, hs_summary, host_list=None, rx_summary=None,
                 stream: int | None = None) -> None:
        """wg_hs_check over torch tensors: wire / pkt_off / pkt_len as rx_plan() took them, hs_status int32
        [n], records uint8 [n, 160] (wg_hs_record, WG_HS_RECORD_DTYPE), hs_summary int32 [4] (n_valid,
        n_init, n_resp, n_rejected). host_list and rx_summary are the tensors rx_plan() wrote: the check
        reads the list's length (wg_rx_summary.n_host) on the device, so plan and check run back to back
        on one stream. Without them every one of the n datagrams is checked."""
        if (host_list is None) != (rx_summary is None):
            raise L.WgError(L.WG_EINVAL, "host_list and rx_summary go together")
        n_list = rx_summary.data_ptr() + L.WgRxSummary.n_host.offset if rx_summary is not None else None
        b = L.WgHsBatch(wire.data_ptr(), wire.numel(), pkt_off.data_ptr(), pkt_len.data_ptr(),
                        host_list.data_ptr() if host_list is not None else None, n_list, hs_status.data_ptr(),
                        records.data_ptr(), hs_summary.data_ptr(), pkt_off.shape[0], 0)
        L.check(self._lib.wg_hs_check(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    # ---- X25519 (wg_x25519_batch / wg_hs_static_set / wg_hs_dh) -------------------------------
    def x25519(self, desc, inp, out, status, stream: int | None = None) -> None:
        """wg_x25519_batch over torch tensors: desc int64 [n, 4] (wg_x25519_desc records, pack_x25519_desc),
        inp / out uint8 (device, not overlapping), status int32 [n] (WG_X25519_*). Scalars and points are
        read from inp; the scalars are clamped on the device."""
        n = desc.shape[0]
        L.check(self._lib.wg_x25519_batch(self.ctx, desc.data_ptr(), n, inp.data_ptr(), inp.numel(), out.data_ptr(),
                                          out.numel(), status.data_ptr(),
                                          stream if stream is not None else _torch_stream()))

    def x25519_host(self, pairs) -> list:
        """X25519 of host byte strings through one wg_x25519_batch call: pairs = [(scalar, point)], a point of
        None is the base point; returns [(32 bytes, WG_X25519_* status)]. The device copies of the scalars are
        zeroed before it returns. For the noise mirror and tests; a data path keeps its bytes on the device
        and calls x25519()."""
        import torch
        if not pairs:
            return []
        dev = torch.device("cuda", self.device)
        n = len(pairs)
        buf = bytearray(64 * n)
        flags = np.zeros(n, np.uint32)
        for k, (scalar, point) in enumerate(pairs):
            if len(scalar) != 32 or (point is not None and len(point) != 32):
                raise L.WgError(L.WG_EINVAL, "X25519 scalars and points are 32 bytes")
            buf[64 * k:64 * k + 32] = bytes(scalar)
            if point is None:
                flags[k] = L.WG_X25519_BASE
            else:
                buf[64 * k + 32:64 * k + 64] = bytes(point)
        at = 64 * np.arange(n, dtype=np.uint64)
        d = pack_x25519_desc(at, at + np.uint64(32), 32 * np.arange(n, dtype=np.uint64), flags)
        d_desc = torch.from_numpy(desc_as_int64(d)).to(dev)
        d_in = torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).to(dev)
        d_out = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
        d_st = torch.zeros(n, dtype=torch.int32, device=dev)
        st = _torch_stream()
        try:
            self.x25519(d_desc, d_in, d_out, d_st, stream=st)
            self.sync(st)
        finally:
            d_in.zero_()
            torch.cuda.synchronize(dev)
            buf[:] = bytes(len(buf))
        status = d_st.cpu().numpy().tolist()
        if L.WG_X25519_BADDESC in status:
            raise L.WgError(L.WG_EINVAL, "wg_x25519_batch refused a descriptor")
        out = d_out.cpu().numpy().tobytes()
        return [(out[32 * k:32 * k + 32], int(status[k])) for k in range(n)]

    def hs_static_set(self, static_private) -> bytes:
        """wg_hs_static_set: the local static private key (32 bytes) into its device buffer; returns the public
        key, derived on the device, and sets the mac1 key from it as hs_key_set(public) would."""
        priv = np.frombuffer(bytes(static_private), np.uint8).copy()
        if priv.size != 32:
            raise L.WgError(L.WG_EINVAL, f"static private key of {priv.size} bytes")
        pub = np.zeros(32, np.uint8)
        try:
            L.check(self._lib.wg_hs_static_set(self.ctx, priv.ctypes.data, pub.ctypes.data))
        finally:
            priv[:] = 0
        return pub.tobytes()

    def hs_dh(self, records, hs_summary, shared, dh_status, stream: int | None = None) -> None:
        """wg_hs_dh over torch tensors: records uint8 [n, 160] and hs_summary int32 [4] as hs_check() wrote
        them (the record count, n_valid, is read on the device: check and dh run back to back on one stream;
        hs_summary None: all n records), shared uint8 [n, 32] or [n * 32], dh_status int32 [n] (WG_X25519_*)."""
        n_records = hs_summary.data_ptr() + L.WgHsSummary.n_valid.offset if hs_summary is not None else None
        b = L.WgHsDhBatch(records.data_ptr(), n_records, shared.data_ptr(), dh_status.data_ptr(), records.shape[0], 0)
        L.check(self._lib.wg_hs_dh(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    # ---- the initiations' encrypted static (wg_hs_peers_set / wg_hs_open) ---------------------
    def hs_peers_set(self, publics) -> None:
        """wg_hs_peers_set: the peers' static public keys (32 n bytes, or a sequence of 32-byte keys) onto the
        device, with each peer's static-static secret under the key of hs_static_set. A peer is named by its
        position; two equal keys are refused."""
        if not isinstance(publics, (bytes, bytearray, memoryview, np.ndarray)):
            publics = b"".join(bytes(p) for p in publics)
        pk = np.frombuffer(bytes(publics), np.uint8).copy()
        if pk.size % 32:
            raise L.WgError(L.WG_EINVAL, f"{pk.size} bytes of static public keys: not a multiple of 32")
        L.check(self._lib.wg_hs_peers_set(self.ctx, pk.ctypes.data if pk.size else None, pk.size // 32))

    def hs_open(self, records, hs_summary, shared, dh_status, open_status, inits, open_summary,
                stream: int | None = None) -> None:
        """wg_hs_open over torch tensors: records and hs_summary as hs_check() wrote them (hs_summary None: all
        n records), shared and dh_status as hs_dh() wrote them, open_status int32 [n] (WG_HS_OPEN_*), inits
        uint8 [n, 144] (wg_hs_init, WG_HS_INIT_DTYPE), open_summary int32 [4] (n_emitted, n_known, n_badauth,
        n_skipped). Check, dh and open run back to back on one stream."""
        n_records = hs_summary.data_ptr() + L.WgHsSummary.n_valid.offset if hs_summary is not None else None
        b = L.WgHsOpenBatch(records.data_ptr(), n_records, shared.data_ptr(), dh_status.data_ptr(),
                            open_status.data_ptr(), inits.data_ptr(), open_summary.data_ptr(), records.shape[0], 0)
        L.check(self._lib.wg_hs_open(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    def hs_open_host(self, remote_ephemeral, encrypted_static, encrypted_timestamp):
        """One initiation's fields through hs_dh + hs_open under the key of hs_static_set: returns (WG_HS_OPEN_*
        status, the wg_hs_init entry as a WG_HS_INIT_DTYPE scalar, or None when nothing was emitted). For the
        noise mirror and tests; a data path runs the chain over a ring."""
        import torch
        if len(remote_ephemeral) != 32 or len(encrypted_static) != 48 or len(encrypted_timestamp) != 28:
            raise L.WgError(L.WG_EINVAL, "an initiation carries 32 + 48 + 28 bytes")
        dev = torch.device("cuda", self.device)
        rec = np.zeros(1, WG_HS_RECORD_DTYPE)
        rec["len"] = L.WG_HS_INIT_SIZE
        msg = bytes([1, 0, 0, 0, 0, 0, 0, 0]) + bytes(remote_ephemeral) + bytes(encrypted_static) + bytes(encrypted_timestamp)
        rec["msg"][0, :len(msg)] = np.frombuffer(msg, np.uint8)
        d_rec = torch.from_numpy(rec.view(np.uint8).reshape(1, 160)).to(dev)
        d_sh = torch.zeros(32, dtype=torch.uint8, device=dev)
        d_ds, d_os = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2))
        d_init = torch.zeros((1, 144), dtype=torch.uint8, device=dev)
        d_sum = torch.zeros(4, dtype=torch.int32, device=dev)
        st = _torch_stream()
        try:
            self.hs_dh(d_rec, None, d_sh, d_ds, stream=st)
            self.hs_open(d_rec, None, d_sh, d_ds, d_os, d_init, d_sum, stream=st)
            self.sync(st)
        finally:
            d_sh.zero_()
            torch.cuda.synchronize(dev)
        status = int(d_os.cpu().numpy()[0])
        if not int(d_sum.cpu().numpy()[0]):
            return status, None
        return status, d_init.cpu().numpy().reshape(-1).view(WG_HS_INIT_DTYPE)[0]

    # ---- the answer to an initiation (wg_hs_respond) ------------------------------------------
    def hs_respond(self, inits, open_summary, ephemerals, local_index, resp_status, sessions, resp_summary,
                   skip_newpeer: bool = True, stream: int | None = None) -> None:
        """wg_hs_respond over torch tensors: inits uint8 [n, 144] and open_summary int32 [4] as hs_open() wrote
        them (the entry count, n_emitted, is read on the device: open and respond run back to back on one stream;
        open_summary None: all n entries), ephemerals uint8 [n, 32] or [n * 32] (fresh private keys from the
        host's CSPRNG; the call zeroes each one it consumed), local_index int32 [n] (the responder's new session
        indices), resp_status int32 [n] (WG_HS_RESP_*), sessions uint8 [n, 176] (wg_hs_session,
        WG_HS_SESSION_DTYPE), resp_summary int32 [4] (n_ok, n_nopeer, n_noeph, 0). skip_newpeer: an entry without
        a peer is not answered (its chain_key is not final); without it the caller vouches for every chain_key."""
        n_inits = open_summary.data_ptr() + L.WgHsOpenSummary.n_emitted.offset if open_summary is not None else None
        b = L.WgHsRespondBatch(inits.data_ptr(), n_inits, ephemerals.data_ptr(), local_index.data_ptr(),
                               resp_status.data_ptr(), sessions.data_ptr(), resp_summary.data_ptr(), inits.shape[0],
                               L.WG_HS_RESP_SKIP_NEWPEER if skip_newpeer else 0)
        L.check(self._lib.wg_hs_respond(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    def hs_respond_host(self, init_entry, ephemeral, local_index: int):
        """One wg_hs_init entry (a WG_HS_INIT_DTYPE scalar whose chain_key is final) through hs_respond with this
        ephemeral private key (32 bytes) and session index: returns (WG_HS_RESP_* status, the wg_hs_session as a
        WG_HS_SESSION_DTYPE scalar, or None when nothing was answered). The device copies of the ephemeral and
        of the session are zeroed before it returns. For the noise mirror and tests."""
        import torch
        if len(ephemeral) != 32:
            raise L.WgError(L.WG_EINVAL, "an ephemeral private key is 32 bytes")
        dev = torch.device("cuda", self.device)
        ent = np.zeros(1, WG_HS_INIT_DTYPE)
        ent[0] = init_entry
        d_init = torch.from_numpy(ent.view(np.uint8).reshape(1, 144)).to(dev)
        d_eph = torch.from_numpy(np.frombuffer(bytes(ephemeral), np.uint8).copy()).to(dev)
        d_li = torch.from_numpy(np.array([local_index & 0xFFFFFFFF], np.uint32).view(np.int32)).to(dev)
        d_st = torch.zeros(1, dtype=torch.int32, device=dev)
        d_sess = torch.zeros((1, 176), dtype=torch.uint8, device=dev)
        d_sum = torch.zeros(4, dtype=torch.int32, device=dev)
        st = _torch_stream()
        try:
            self.hs_respond(d_init, None, d_eph, d_li, d_st, d_sess, d_sum, skip_newpeer=False, stream=st)
            self.sync(st)
            status = int(d_st.cpu().numpy()[0])
            sess = d_sess.cpu().numpy().reshape(-1).view(WG_HS_SESSION_DTYPE)[0].copy() if int(d_sum.cpu().numpy()[0]) else None
        finally:
            d_eph.zero_()
            d_sess.zero_()
            d_init.zero_()
            torch.cuda.synchronize(dev)
        return status, sess

    # ---- the initiator's side (wg_hs_psks_set / wg_hs_initiate / wg_hs_finish) -----------------
    def hs_psks_set(self, psks) -> None:
        """wg_hs_psks_set: the peers' preshared keys (32 n bytes, or a sequence of 32-byte keys), by position in
        the table of hs_peers_set, which resets them all to zero; the count must equal the table's."""
        if not isinstance(psks, (bytes, bytearray, memoryview, np.ndarray)):
            psks = b"".join(bytes(p) for p in psks)
        pk = np.frombuffer(bytes(psks), np.uint8).copy()
        if pk.size % 32:
            raise L.WgError(L.WG_EINVAL, f"{pk.size} bytes of preshared keys: not a multiple of 32")
        try:
            L.check(self._lib.wg_hs_psks_set(self.ctx, pk.ctypes.data if pk.size else None, pk.size // 32))
        finally:
            pk[:] = 0

    def hs_initiate(self, peer, ephemerals, timestamps, local_index, status, records, pending, summary,
                    stream: int | None = None) -> None:
        """wg_hs_initiate over torch tensors: peer int32 [n] (positions in the peer table), ephemerals uint8
        [n, 32] or [n * 32] (fresh private keys from the host's CSPRNG; the call zeroes each one it consumed),
        timestamps uint8 [n, 12] or [n * 12] (TAI64N), local_index int32 [n] (the new sender indices), status
        int32 [n] (WG_HS_INIT_*), records uint8 [n, 160] (WG_HS_RECORD_DTYPE), pending uint8 [n, 112]
        (WG_HS_PENDING_DTYPE), summary int32 [4] (n_ok, n_badpeer, n_noeph, 0)."""
        b = L.WgHsInitiateBatch(peer.data_ptr(), ephemerals.data_ptr(), timestamps.data_ptr(), local_index.data_ptr(),
                                status.data_ptr(), records.data_ptr(), pending.data_ptr(), summary.data_ptr(),
                                peer.shape[0], 0)
        L.check(self._lib.wg_hs_initiate(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    def hs_finish(self, records, hs_summary, pending, fin_status, established, fin_summary,
                  stream: int | None = None) -> None:
        """wg_hs_finish over torch tensors: records uint8 [n, 160] and hs_summary int32 [4] as hs_check() wrote
        them on this (the initiator's) context (hs_summary None: all n records), pending uint8 [n_pending, 112] as
        hs_initiate() wrote it (the call zeroes each entry it consumed), fin_status int32 [n] (WG_HS_FIN_*),
        established uint8 [n, 96] (WG_HS_ESTABLISHED_DTYPE), fin_summary int32 [4] (n_ok, n_nopending, n_badauth,
        n_skipped). Check and finish run back to back on one stream."""
        n_records = hs_summary.data_ptr() + L.WgHsSummary.n_valid.offset if hs_summary is not None else None
        b = L.WgHsFinishBatch(records.data_ptr(), n_records, pending.data_ptr() if pending.shape[0] else None,
                              fin_status.data_ptr(), established.data_ptr(), fin_summary.data_ptr(), records.shape[0],
                              pending.shape[0])
        L.check(self._lib.wg_hs_finish(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    def hs_initiate_host(self, peer: int, ephemeral, timestamp, local_index: int):
        """One initiation to the peer at this position of the table, with this ephemeral private key (32 bytes),
        TAI64N timestamp (12 bytes) and sender index: returns (WG_HS_INIT_* status, the 148-byte message, the
        wg_hs_pending entry as a WG_HS_PENDING_DTYPE scalar; None, None when nothing was initiated). The device
        copies of the ephemeral and of the pending entry are zeroed before it returns. For the noise mirror and
        tests."""
        import torch
        if len(ephemeral) != 32 or len(timestamp) != 12:
            raise L.WgError(L.WG_EINVAL, "an ephemeral private key is 32 bytes, a timestamp 12")
        dev = torch.device("cuda", self.device)
        d_peer = torch.from_numpy(np.array([peer & 0xFFFFFFFF], np.uint32).view(np.int32)).to(dev)
        d_eph = torch.from_numpy(np.frombuffer(bytes(ephemeral), np.uint8).copy()).to(dev)
        d_ts = torch.from_numpy(np.frombuffer(bytes(timestamp), np.uint8).copy()).to(dev)
        d_li = torch.from_numpy(np.array([local_index & 0xFFFFFFFF], np.uint32).view(np.int32)).to(dev)
        d_st = torch.zeros(1, dtype=torch.int32, device=dev)
        d_rec = torch.zeros((1, 160), dtype=torch.uint8, device=dev)
        d_pend = torch.zeros((1, 112), dtype=torch.uint8, device=dev)
        d_sum = torch.zeros(4, dtype=torch.int32, device=dev)
        st = _torch_stream()
        try:
            self.hs_initiate(d_peer, d_eph, d_ts, d_li, d_st, d_rec, d_pend, d_sum, stream=st)
            self.sync(st)
            status = int(d_st.cpu().numpy()[0])
            if status != L.WG_HS_INIT_OK:
                return status, None, None
            msg = d_rec.cpu().numpy().reshape(-1).view(WG_HS_RECORD_DTYPE)[0]["msg"].tobytes()
            pend = d_pend.cpu().numpy().reshape(-1).view(WG_HS_PENDING_DTYPE)[0].copy()
        finally:
            d_eph.zero_()
            d_pend.zero_()
            torch.cuda.synchronize(dev)
        return status, msg, pend

    def hs_finish_host(self, pending_entry, response):
        """One 92-byte response against one wg_hs_pending entry (a WG_HS_PENDING_DTYPE scalar) through hs_finish:
        returns (WG_HS_FIN_* status, the wg_hs_established entry as a WG_HS_ESTABLISHED_DTYPE scalar, or None).
        The device copies of the pending entry and of the keys are zeroed before it returns. For the noise mirror
        and tests."""
        import torch
        if len(response) != 92:
            raise L.WgError(L.WG_EINVAL, "a response is 92 bytes")
        dev = torch.device("cuda", self.device)
        rec = np.zeros(1, WG_HS_RECORD_DTYPE)
        rec["len"] = L.WG_HS_RESP_SIZE
        rec["msg"][0, :92] = np.frombuffer(bytes(response), np.uint8)
        pe = np.zeros(1, WG_HS_PENDING_DTYPE)
        pe[0] = pending_entry
        d_rec = torch.from_numpy(rec.view(np.uint8).reshape(1, 160)).to(dev)
        d_pend = torch.from_numpy(pe.view(np.uint8).reshape(1, 112)).to(dev)
        d_st = torch.zeros(1, dtype=torch.int32, device=dev)
        d_est = torch.zeros((1, 96), dtype=torch.uint8, device=dev)
        d_sum = torch.zeros(4, dtype=torch.int32, device=dev)
        st = _torch_stream()
        try:
            self.hs_finish(d_rec, None, d_pend, d_st, d_est, d_sum, stream=st)
            self.sync(st)
            status = int(d_st.cpu().numpy()[0])
            est = d_est.cpu().numpy().reshape(-1).view(WG_HS_ESTABLISHED_DTYPE)[0].copy() if int(d_sum.cpu().numpy()[0]) else None
        finally:
            d_pend.zero_()
            d_est.zero_()
            pe[:] = 0
            torch.cuda.synchronize(dev)
        return status, est

    # ---- the initiations' timestamps (wg_hs_stamp / wg_hs_stamps_set / wg_hs_stamps_get) --------
    def hs_stamps_set(self, first_peer: int, stamps) -> None:
        """wg_hs_stamps_set: the stored timestamps of peers [first_peer, first_peer + n) (12 n bytes, or a sequence
        of 12-byte timestamps), as hs_stamps_get() returned them before a restart. An empty sequence only allocates
        the stamps' state, which a capturing stream cannot do."""
        if not isinstance(stamps, (bytes, bytearray, memoryview, np.ndarray)):
            stamps = b"".join(bytes(t) for t in stamps)
        ts = np.frombuffer(bytes(stamps), np.uint8).copy()
        if ts.size % 12:
            raise L.WgError(L.WG_EINVAL, f"{ts.size} bytes of timestamps: not a multiple of 12")
        L.check(self._lib.wg_hs_stamps_set(self.ctx, first_peer, ts.size // 12, ts.ctypes.data if ts.size else None))

    def hs_stamps_get(self, first_peer: int, n: int) -> list:
        """wg_hs_stamps_get: the stored timestamps of peers [first_peer, first_peer + n), 12 bytes each (all zero:
        nothing accepted from that peer yet)."""
        out = np.zeros(12 * n, np.uint8)
        L.check(self._lib.wg_hs_stamps_get(self.ctx, first_peer, n, out.ctypes.data if n else None))
        raw = out.tobytes()
        return [raw[12 * k:12 * k + 12] for k in range(n)]

    def hs_stamp(self, inits, open_summary, records, shared, ts_status, opened, fresh, stamp_summary,
                 stream: int | None = None) -> None:
        """wg_hs_stamp over torch tensors: inits uint8 [n, 144] and open_summary int32 [4] as hs_open() wrote them
        (the entry count, n_emitted, is read on the device: open and stamp run back to back on one stream;
        open_summary None: all n entries), records uint8 [n_rec, 160] and shared uint8 [n_rec, 32] or [n_rec * 32]
        as hs_open() read them, ts_status int32 [n] (WG_HS_TS_*), opened uint8 [n, 12] or [n * 12] (the opened
        timestamps, by position), fresh uint8 [n, 144] (the fresh entries, compacted: what hs_respond() takes, with
        stamp_summary in open_summary's place), stamp_summary int32 [4] (n_ok, n_stale, n_badauth, n_skipped)."""
        n_inits = open_summary.data_ptr() + L.WgHsOpenSummary.n_emitted.offset if open_summary is not None else None
        n_rec = records.shape[0]
        b = L.WgHsStampBatch(inits.data_ptr(), n_inits, records.data_ptr() if n_rec else None,
                             shared.data_ptr() if n_rec else None, ts_status.data_ptr(), opened.data_ptr(),
                             fresh.data_ptr(), stamp_summary.data_ptr(), inits.shape[0], n_rec, 0, 0)
        L.check(self._lib.wg_hs_stamp(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    # ---- cookies and mac2 under load (wg_hs_cookie_secret_set / wg_hs_admit / wg_hs_cookie_open / wg_hs_mac2) ----
    def hs_cookie_secret_set(self, secret) -> None:
        """wg_hs_cookie_secret_set: the responder's 32-byte cookie secret, from the host's CSPRNG; the host rotates
        it by its own clock (WireGuard: every 120 s)."""
        sec = np.frombuffer(bytes(secret), np.uint8).copy()
        if sec.size != 32:
            raise L.WgError(L.WG_EINVAL, f"cookie secret of {sec.size} bytes")
        try:
            L.check(self._lib.wg_hs_cookie_secret_set(self.ctx, sec.ctypes.data))
        finally:
            sec[:] = 0

    def hs_admit(self, wire, pkt_off, pkt_len, src, nonces, hs_status, records, hs_summary, replies, admit_summary,
                 host_list=None, rx_summary=None, stream: int | None = None) -> None:
        """wg_hs_admit over torch tensors: hs_check() under load. wire / pkt_off / pkt_len / hs_status / records /
        hs_summary / host_list / rx_summary as hs_check() takes them; src uint8 [n, 24] (wg_hs_src,
        WG_HS_SRC_DTYPE, by batch index), nonces uint8 [n, 24] or [n * 24] (fresh random bytes by list position;
        the call zeroes each one it consumed), replies uint8 [n, 80] (wg_hs_cookie_reply,
        WG_HS_COOKIE_REPLY_DTYPE), admit_summary int32 [4] (n_replies, n_mac2_ok, n_nononce, n_badsrc)."""
        if (host_list is None) != (rx_summary is None):
            raise L.WgError(L.WG_EINVAL, "host_list and rx_summary go together")
        n_list = rx_summary.data_ptr() + L.WgRxSummary.n_host.offset if rx_summary is not None else None
        hs = L.WgHsBatch(wire.data_ptr(), wire.numel(), pkt_off.data_ptr(), pkt_len.data_ptr(),
                         host_list.data_ptr() if host_list is not None else None, n_list, hs_status.data_ptr(),
                         records.data_ptr(), hs_summary.data_ptr(), pkt_off.shape[0], 0)
        b = L.WgHsAdmitBatch(hs, src.data_ptr(), nonces.data_ptr(), replies.data_ptr(), admit_summary.data_ptr())
        L.check(self._lib.wg_hs_admit(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    def hs_cookie_open(self, wire, pkt_off, pkt_len, sent, pending, ck_status, learned, summary,
                       stream: int | None = None) -> None:
        """wg_hs_cookie_open over torch tensors: wire / pkt_off / pkt_len as rx_plan() took them (every datagram is
        looked at), sent uint8 [n_pending, 160] and pending uint8 [n_pending, 112] as hs_initiate() wrote them
        (pending is only read), ck_status int32 [n] (WG_HS_CK_*, by batch index), learned uint8 [n, 16]
        (WG_HS_LEARNED_DTYPE), summary int32 [4] (n_ok, n_nopending, n_badauth, n_skipped). The opened cookies
        go to the device's cookie table (hs_cookies_get)."""
        np_ = pending.shape[0]
        b = L.WgHsCookieOpenBatch(wire.data_ptr(), wire.numel(), pkt_off.data_ptr(), pkt_len.data_ptr(),
                                  sent.data_ptr() if np_ else None, pending.data_ptr() if np_ else None,
                                  ck_status.data_ptr(), learned.data_ptr(), summary.data_ptr(), pkt_off.shape[0], np_)
        L.check(self._lib.wg_hs_cookie_open(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    def hs_cookies_get(self, first_peer: int, n: int):
        """wg_hs_cookies_get: (cookies, have) of peers [first_peer, first_peer + n): a list of 16-byte cookies and
        a list of bools."""
        ck = np.zeros(16 * n, np.uint8)
        have = np.zeros(n, np.uint8)
        L.check(self._lib.wg_hs_cookies_get(self.ctx, first_peer, n, ck.ctypes.data if n else None,
                                            have.ctypes.data if n else None))
        raw = ck.tobytes()
        return [raw[16 * k:16 * k + 16] for k in range(n)], [bool(h) for h in have]

    def hs_cookies_set(self, first_peer: int, cookies, have) -> None:
        """wg_hs_cookies_set: the cookies of peers [first_peer, first_peer + n) (a sequence of 16-byte cookies, or
        16 n bytes) and their `have` flags; have = False clears an entry (the host expires a cookie after 120 s)."""
        if not isinstance(cookies, (bytes, bytearray, memoryview, np.ndarray)):
            cookies = b"".join(bytes(x) for x in cookies)
        ck = np.frombuffer(bytes(cookies), np.uint8).copy()
        hv = np.array([1 if h else 0 for h in have], np.uint8)
        if ck.size != 16 * hv.size:
            raise L.WgError(L.WG_EINVAL, f"{ck.size} bytes of cookies for {hv.size} flags")
        try:
            L.check(self._lib.wg_hs_cookies_set(self.ctx, first_peer, hv.size, ck.ctypes.data if hv.size else None,
                                                hv.ctypes.data if hv.size else None))
        finally:
            ck[:] = 0

    def hs_mac2(self, records, peer, mac2_status, summary, stream: int | None = None) -> None:
        """wg_hs_mac2 over torch tensors: records uint8 [n, 160] as hs_initiate() wrote them (the call writes mac2
        into each record whose peer holds a cookie), peer int32 [n] (positions in the peer table), mac2_status
        int32 [n] (WG_HS_MAC2_*), summary int32 [4] (n_ok, n_none, n_bad, 0)."""
        b = L.WgHsMac2Batch(records.data_ptr(), peer.data_ptr(), mac2_status.data_ptr(), summary.data_ptr(),
                            records.shape[0], 0)
        L.check(self._lib.wg_hs_mac2(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    # ---- handshakes rate-limited per source (wg_hs_rl_* / wg_hs_ratelimit) ----
    def hs_rl_reserve(self, max_sources: int) -> None:
        """wg_hs_rl_reserve: the limiter's table, for up to max_sources sources at once (capacity: the smallest power
        of two >= max(8, 2 max_sources)), with its spare and scratch. hs_reserve() sizes the per-record scratch."""
        L.check(self._lib.wg_hs_rl_reserve(self.ctx, max_sources))

    def hs_rl_config_set(self, config, burst: int | None = None) -> None:
        """wg_hs_rl_config_set: a RateLimitConfig, or (cost, burst). A new cost needs no re-capture of a captured
        hs_ratelimit(); a greater burst does."""
        cost, burst = (config.cost, config.burst) if burst is None else (config, burst)
        if cost < 0 or cost >= 1 << 64 or burst < 0 or burst >= 1 << 32:
            raise L.WgError(L.WG_EINVAL, f"ratelimit cost {cost}, burst {burst}")
        L.check(self._lib.wg_hs_rl_config_set(self.ctx, cost, burst))

    def hs_ratelimit(self, records, hs_summary, src, now, rl_status, out_records, rl_summary, compact: bool = False,
                     stream: int | None = None) -> None:
        """wg_hs_ratelimit over torch tensors: records uint8 [n, 160] as hs_check() / hs_admit() wrote them, hs_summary
        the int32 [4] tensor whose first word is their count (n_valid), or None for all n; src uint8 [n_src, 24]
        (WG_HS_SRC_DTYPE, by batch index), now int64 [1] (ticks; 0: nothing is limited), rl_status int32 [n]
        (WG_HS_RL_*, by record position), out_records uint8 [n, 160] (the OK records, in order), rl_summary int32 [4]
        (n_passed, n_limited, n_full, n_badsrc): hs_dh() takes it as its hs_summary. compact: drop the stale entries
        first if the call's records might not fit the table."""
        b = L.WgHsRlBatch(records.data_ptr(), hs_summary.data_ptr() if hs_summary is not None else None,
                          src.data_ptr() if src.shape[0] else None, now.data_ptr(), rl_status.data_ptr(),
                          out_records.data_ptr(), rl_summary.data_ptr(), records.shape[0], src.shape[0],
                          L.WG_HS_RL_COMPACT if compact else 0, 0)
        L.check(self._lib.wg_hs_ratelimit(self.ctx, ctypes.byref(b), stream if stream is not None else _torch_stream()))

    def hs_rl_compact(self, now, summary=None, stream: int | None = None) -> None:
        """wg_hs_rl_compact: rebuild the limiter's table from the entries that are not stale at *now (int64 [1]);
        summary int32 [4] (kept, dropped, 0, 0) or None."""
        L.check(self._lib.wg_hs_rl_compact(self.ctx, now.data_ptr(), summary.data_ptr() if summary is not None else None,
                                           stream if stream is not None else _torch_stream()))

    def hs_rl_count(self) -> tuple[int, int]:
        """wg_hs_rl_count: (entries, capacity) of the limiter's table."""
        used, cap = ctypes.c_uint32(0), ctypes.c_uint32(0)
        L.check(self._lib.wg_hs_rl_count(self.ctx, ctypes.byref(used), ctypes.byref(cap)))
        return used.value, cap.value

    def hs_rl_dump(self) -> np.ndarray:
        """wg_hs_rl_dump: the limiter's entries, in table order (WG_HS_RL_ENTRY_DTYPE)."""
        used, _ = self.hs_rl_count()
        out = np.zeros(used, WG_HS_RL_ENTRY_DTYPE)
        n = ctypes.c_uint32(0)
        L.check(self._lib.wg_hs_rl_dump(self.ctx, out.ctypes.data if used else None, used, ctypes.byref(n)))
        return out[:min(used, n.value)]

    def hs_rl_load(self, entries) -> None:
        """wg_hs_rl_load: replace the limiter's entries with these (WG_HS_RL_ENTRY_DTYPE, as hs_rl_dump() returned
        them): save and restore."""
        ent = np.ascontiguousarray(entries, WG_HS_RL_ENTRY_DTYPE)
        L.check(self._lib.wg_hs_rl_load(self.ctx, ent.ctypes.data if ent.size else None, ent.size))

    def hs_stamp_host(self, init_entry, record, shared):
        """One wg_hs_init entry (a WG_HS_INIT_DTYPE scalar, as hs_open_host() returned it) with the record it came
        from (a WG_HS_RECORD_DTYPE scalar, or the 148-byte initiation) and wg_hs_dh's 32 bytes for it, through
        hs_stamp: returns (WG_HS_TS_* status, the 12 opened bytes, or None when the tag did not verify). The
        entry's `record` field is taken as 0. An OK status has stored the timestamp as the peer's. The device copy
        of the shared secret is zeroed before it returns. For the noise mirror and tests."""
        import torch
        if len(shared) != 32:
            raise L.WgError(L.WG_EINVAL, "a shared secret is 32 bytes")
        dev = torch.device("cuda", self.device)
        rec = np.zeros(1, WG_HS_RECORD_DTYPE)
        if isinstance(record, (bytes, bytearray, memoryview)):
            if len(record) != L.WG_HS_INIT_SIZE:
                raise L.WgError(L.WG_EINVAL, "an initiation is 148 bytes")
            rec["len"] = L.WG_HS_INIT_SIZE
            rec["msg"][0] = np.frombuffer(bytes(record), np.uint8)
        else:
            rec[0] = record
        ent = np.zeros(1, WG_HS_INIT_DTYPE)
        ent[0] = init_entry
        ent["record"] = 0
        d_init = torch.from_numpy(ent.view(np.uint8).reshape(1, 144)).to(dev)
        d_rec = torch.from_numpy(rec.view(np.uint8).reshape(1, 160)).to(dev)
        d_sh = torch.from_numpy(np.frombuffer(bytes(shared), np.uint8).copy()).to(dev)
        d_st = torch.zeros(1, dtype=torch.int32, device=dev)
        d_ts = torch.zeros(12, dtype=torch.uint8, device=dev)
        d_fresh = torch.zeros((1, 144), dtype=torch.uint8, device=dev)
        d_sum = torch.zeros(4, dtype=torch.int32, device=dev)
        st = _torch_stream()
        try:
            self.hs_stamp(d_init, None, d_rec, d_sh, d_st, d_ts, d_fresh, d_sum, stream=st)
            self.sync(st)
            status = int(d_st.cpu().numpy()[0])
            opened = d_ts.cpu().numpy().tobytes()
        finally:
            d_sh.zero_()
            d_init.zero_()
            d_fresh.zero_()
            torch.cuda.synchronize(dev)
        return status, (opened if status in (L.WG_HS_TS_OK, L.WG_HS_TS_REPLAY, L.WG_HS_TS_SUPERSEDED) else None)

    def set_receivers(self, receivers) -> None:
        """wg_ctx_set_receivers: device tensor of receiver_index per key slot for
        seal(..., frame=True) — contiguous, 4-byte integers, on this engine's device, at
        least key_slots entries; the engine keeps it alive while seals use it."""
        if receivers is None:
            L.check(self._lib.wg_ctx_set_receivers(self.ctx, None, 0))
            self._receivers = None
            return
        if receivers.device.type != "cuda" or receivers.device.index not in (None, self.device):
            raise L.WgError(L.WG_EINVAL, f"receiver table on {receivers.device}, engine on cuda:{self.device}")
        if not receivers.is_contiguous() or receivers.element_size() != 4:
            raise L.WgError(L.WG_EINVAL, "receiver table must be a contiguous int32/uint32 tensor")
        if receivers.numel() < self.key_slots:
            raise L.WgError(L.WG_ERANGE, f"receiver table has {receivers.numel()} entries for {self.key_slots} slots")
        L.check(self._lib.wg_ctx_set_receivers(self.ctx, receivers.data_ptr(), receivers.numel()))
        self._receivers = receivers

    def frame_seal(self, desc, receivers, out, in_size: int, max_len: int, stream: int | None = None):
        """wg_frame_seal: write the 16-B transport header {4, 0, 0, 0, receiver_index, counter}
        in front of every packet the seal accepts (UnencryptedOutgoingTransport.java:14-18,
        EncryptedOutgoingTransport.java:11-14). `receivers` is a uint32/int32 device tensor
        indexed by key slot; in_size / max_len are the seal call's."""
        n = desc.shape[0]
        L.check(self._lib.wg_frame_seal(self.ctx, desc.data_ptr(), n, receivers.data_ptr(), out.data_ptr(),
                                        out.numel(), in_size, max_len,
                                        stream if stream is not None else _torch_stream()))

    def parse_open(self, wire, pkt_off, pkt_len, key_slot, desc_out, parse_status=None, stream: int | None = None):
        """wg_parse_open: open descriptors from received wire packets on device
        (UndecryptedIncomingTransport.java:20-33); plaintext lands right after each
        packet's ciphertext in `wire`. pkt_off int64, pkt_len / key_slot int32 device tensors."""
        n = pkt_off.shape[0]
        L.check(self._lib.wg_parse_open(self.ctx, wire.data_ptr(), wire.numel(), pkt_off.data_ptr(),
                                        pkt_len.data_ptr(), key_slot.data_ptr(), n, desc_out.data_ptr(),
                                        parse_status.data_ptr() if parse_status is not None else None,
                                        stream if stream is not None else _torch_stream()))

    def aead(self, mode: int, desc, inp, aad, out, status, max_len: int, stream: int | None = None):
        """wg_aead_batch over torch tensors: desc int64 [n, 8] (wg_aead_desc records)."""
        n = desc.shape[0]
        L.check(self._lib.wg_aead_batch(self.ctx, mode, desc.data_ptr(), n, inp.data_ptr() if inp is not None else None,
                                        inp.numel() if inp is not None else 0,
                                        aad.data_ptr() if aad is not None else None,
                                        aad.numel() if aad is not None else 0, out.data_ptr(), out.numel(),
                                        status.data_ptr() if status is not None else None, max_len,
                                        stream if stream is not None else _torch_stream()))

    # ---- host buffers ---------------------------------------------------------------
    def seal_host(self, desc: np.ndarray, inp, out, max_len: int, uniform: bool = False):
        """wg_seal_host: a batch in host memory. ``inp``/``out`` are numpy arrays (pageable:
        chunked copy pipeline) or pinned buffers from :meth:`host_alloc` (zero-copy)."""
        d = np.ascontiguousarray(desc)
        ip, isz = _host_buf(inp)
        op, osz = _host_buf(out)
        L.check(self._lib.wg_seal_host(self.ctx, d.ctypes.data, len(d), ip, isz, op, osz, max_len,
                                       L.WG_F_UNIFORM if uniform else 0))

    def open_host(self, desc: np.ndarray, inp, out, max_len: int, uniform: bool = False) -> np.ndarray:
        d = np.ascontiguousarray(desc)
        status = np.zeros(len(d), np.uint32)
        ip, isz = _host_buf(inp)
        op, osz = _host_buf(out)
        L.check(self._lib.wg_open_host(self.ctx, d.ctypes.data, len(d), ip, isz, op, osz, status.ctypes.data, max_len,
                                       L.WG_F_UNIFORM if uniform else 0))
        return status

    def host_alloc(self, nbytes: int) -> np.ndarray:
        """A pinned, device-mapped host ring (wg_host_alloc) as a uint8 numpy array; freed
        with :meth:`host_free` (or when the engine closes)."""
        p = ctypes.c_void_p()
        L.check(self._lib.wg_host_alloc(self.ctx, nbytes, ctypes.byref(p)))
        arr = np.ctypeslib.as_array((ctypes.c_uint8 * max(nbytes, 1)).from_address(p.value))[:nbytes]
        self._pinned[arr.ctypes.data] = p
        return arr

    def host_free(self, arr: np.ndarray) -> None:
        p = self._pinned.pop(arr.ctypes.data, None)
        if p is not None:
            L.check(self._lib.wg_host_free(self.ctx, p))

    def aead_host(self, mode: int, descs, keys: bytes, inp: bytes, aad: bytes, out_size: int):
        """General AEAD / primitive batch on host buffers (wg_aead_host). Returns (out, status)."""
        arr = (L.WgAeadDesc * len(descs))(*descs)
        kb = np.frombuffer(keys, np.uint8).copy()
        ib = np.frombuffer(inp, np.uint8).copy() if inp else np.zeros(1, np.uint8)
        ab = np.frombuffer(aad, np.uint8).copy() if aad else np.zeros(1, np.uint8)
        out = np.zeros(max(out_size, 1), np.uint8)
        status = np.zeros(len(descs), np.uint32)
        L.check(self._lib.wg_aead_host(self.ctx, mode, ctypes.addressof(arr), len(descs), kb.ctypes.data,
                                       kb.size // 32, ib.ctypes.data, len(inp), ab.ctypes.data, len(aad),
                                       out.ctypes.data, out_size, status.ctypes.data))
        return out[:out_size].tobytes(), status

    def queue(self, mode: str, capacity: int = 0, max_len: int = 0, max_batch: int = 0) -> "Queue":
        """wg_queue_create: an asynchronous seal ("seal") or open ("open") queue on this context."""
        return Queue(self, mode, capacity, max_len, max_batch)

    def seal1(self, slot: int, counter: int, pt: bytes) -> bytes:
        src = np.frombuffer(pt, np.uint8).copy() if pt else np.zeros(1, np.uint8)
        out = np.zeros(len(pt) + 16, np.uint8)
        L.check(self._lib.wg_seal1(self.ctx, slot, counter, src.ctypes.data, len(pt), out.ctypes.data))
        return out.tobytes()

    def open1(self, slot: int, counter: int, ct_tag: bytes) -> bytes | None:
        n = len(ct_tag) - 16
        src = np.frombuffer(ct_tag, np.uint8).copy()
        out = np.zeros(max(n, 1), np.uint8)
        rc = L.check(self._lib.wg_open1(self.ctx, slot, counter, src.ctypes.data, n, out.ctypes.data))
        return None if rc == 1 else out[:n].tobytes()

    def pp_config(self, waves: int = 16, idle_us: int = 20000) -> None:
        """wg_pp_config: waves of the persistent per-packet server (k_pp) that serves
        seal1/open1 (a power of two), and how long it stays resident without work (microseconds)."""
        L.check(self._lib.wg_pp_config(self.ctx, waves, idle_us))

    batcher_config = pp_config  # round-3 name

    def batcher_stats(self) -> tuple[int, int]:
        """(server launches, packets served) of the per-packet path so far."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        L.check(self._lib.wg_batcher_stats(self.ctx, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    # ---- instrumentation ----------------------------------------------------------
    def timing(self, on: bool):
        L.check(self._lib.wg_timing_enable(self.ctx, 1 if on else 0))

    def timing_read(self) -> tuple[float, int]:
        ms = ctypes.c_double()
        k = ctypes.c_uint64()
        L.check(self._lib.wg_timing_read(self.ctx, ctypes.byref(ms), ctypes.byref(k)))
        return ms.value, k.value


def _torch_stream() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream


def selftest(device: int = 0) -> bool:
    """wg_aead_selftest: the reference's known-answer vectors, on the device (Poly1305.java:62-76)."""
    return L.lib().wg_aead_selftest(device) == 1


_default: dict[int, Engine] = {}
_default_lock = threading.Lock()


def default_engine(device: int | None = None) -> Engine:
    """Process-wide engine per device, created on first use (like the reference's static initialisers)."""
    import os
    dev = int(os.environ.get("WG_DEVICE", "0")) if device is None else device
    with _default_lock:
        if dev not in _default:
            _default[dev] = Engine(dev, key_slots=int(os.environ.get("WG_KEY_SLOTS", "65536")))
        return _default[dev]


def _host_buf(x):
    """(pointer, nbytes) of a host buffer: numpy array or CPU torch tensor (pinned or not)."""
    if isinstance(x, np.ndarray):
        assert x.flags.c_contiguous
        return x.ctypes.data, x.nbytes
    return x.data_ptr(), x.numel() * x.element_size()


class Queue:
    """wg_queue: producers submit packets without waiting for the crypto (wg_submit_seal /
    wg_submit_open), a consumer reaps the results (wg_reap, wg_reap_done). The batching
    replacement for TransportManager's per-packet ForkJoinPool submission
    (TransportManager.java:41,70-93,137-158)."""

    def __init__(self, engine: Engine, mode: str, capacity: int = 0, max_len: int = 0, max_batch: int = 0):
        self._lib = engine._lib
        self.mode = {"seal": L.WG_MODE_SEAL, "open": L.WG_MODE_OPEN}[mode]
        q = ctypes.c_void_p()
        L.check(self._lib.wg_queue_create(engine.ctx, self.mode, capacity, max_len, max_batch, ctypes.byref(q)))
        self.q = q.value
        self._buf = (L.WgCompletion * 4096)()

    def submit(self, key_slot: int, counter: int, data: bytes, user: int = 0) -> None:
        """seal: data = plaintext; open: data = ct || tag."""
        n = len(data) - (16 if self.mode == L.WG_MODE_OPEN else 0)
        if n < 0:
            raise ValueError("open needs ct || tag (at least 16 bytes)")
        src = np.frombuffer(bytes(data), np.uint8) if data else np.zeros(1, np.uint8)
        fn = self._lib.wg_submit_seal if self.mode == L.WG_MODE_SEAL else self._lib.wg_submit_open
        L.check(fn(self.q, key_slot, counter, src.ctypes.data, n, user))

    def submit_n(self, packets) -> int:
        """wg_submit_seal_n / wg_submit_open_n: packets = [(key_slot, counter, data, user)] queued in
        one call (data as for submit()); returns how many were queued (fewer than len(packets) only
        when the submit timeout ran out partway)."""
        arr = (L.WgSubmit * max(1, len(packets)))()
        keep = []
        for k, (key_slot, counter, data, user) in enumerate(packets):
            n = len(data) - (16 if self.mode == L.WG_MODE_OPEN else 0)
            if n < 0:
                raise ValueError("open needs ct || tag (at least 16 bytes)")
            src = np.frombuffer(bytes(data), np.uint8) if data else np.zeros(1, np.uint8)
            keep.append(src)
            arr[k].user, arr[k].counter, arr[k].data = user, counter, src.ctypes.data
            arr[k].len, arr[k].key_slot = n, key_slot
        fn = self._lib.wg_submit_seal_n if self.mode == L.WG_MODE_SEAL else self._lib.wg_submit_open_n
        return L.check(fn(self.q, arr, len(packets)))

    def reap(self, max_n: int = 4096, timeout_us: int = 100000):
        """[(user, counter, status, result bytes)], the slots handed back at once; the result is
        ct || tag for a seal, the plaintext for an open (None unless status is WG_PKT_OK)."""
        m = min(max_n, len(self._buf))
        n = L.check(self._lib.wg_reap(self.q, self._buf, m, timeout_us))
        out = []
        for k in range(n):
            c = self._buf[k]
            size = c.len + (16 if self.mode == L.WG_MODE_SEAL else 0)
            ok = c.status == L.WG_PKT_OK
            data = ctypes.string_at(c.data, size) if ok and size else (b"" if ok else None)
            out.append((c.user, c.counter, c.status, data))
        L.check(self._lib.wg_reap_done(self.q, self._buf, n))
        return out

    def set_submit_timeout(self, timeout_us: int) -> None:
        """wg_queue_set_submit_timeout: submit() raises WgError(EAGAIN) once no slot has been free for
        timeout_us (0: it waits without bound, the default)."""
        L.check(self._lib.wg_queue_set_submit_timeout(self.q, timeout_us))

    def stats(self) -> tuple[int, int]:
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        L.check(self._lib.wg_queue_stats(self.q, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def close(self) -> None:
        if self.q:
            L.check(self._lib.wg_queue_destroy(self.q))
            self.q = None
