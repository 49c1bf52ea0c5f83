"""ax.xz.wireguard.noise.handshake mirror: SymmetricKeypair, the drop-in boundary,
Handshakes.decryptRemoteStatic / ResponderHandshake, the responder's two phases on the device, and
Handshakes.initiateHandshake / InitiatorStageOne, the initiator's two.

Keeps the reference API (SymmetricKeypair.java:20-94): cipher(src, dst) -> counter,
decipher(counter, src, dst) raising BadPaddingException (AEADBadTagException),
clean(). Keys live in the device key table of the engine; the nonce is the
reference layout LE64(counter) || 0^4, built on the device. An additive batch
API (cipher_batch / decipher_batch) feeds whole device-resident batches.
"""
from __future__ import annotations

import os
import threading

import numpy as np

from .. import _lib as L
from ..engine import Engine, default_engine, desc_as_int64, pack_desc
from .crypto import AEADBadTagException, Crypto, IllegalStateException, _bytes, _size, _write
from .keys import NoisePresharedKey, NoisePrivateKey, NoisePublicKey


class Handshakes:
    """Handshakes.java: the responder's first phase, on the device."""

    @staticmethod
    def decryptRemoteStatic(localKeypair: NoisePrivateKey, remoteEphemeral: NoisePublicKey, encryptedStatic,
                            encryptedTimestamp, engine: Engine | None = None) -> NoisePublicKey:
        """Handshakes.decryptRemoteStatic (Handshakes.java:47-50, 201-237): the initiator's static public key,
        or AEADBadTagException (a BadPaddingException) when encryptedStatic does not verify. Like the
        reference it returns the key whether or not a peer holds it, and never opens encryptedTimestamp.
        One record through wg_hs_dh + wg_hs_open; localKeypair becomes the engine's static key
        (hs_static_set), as a responder has one."""
        eng = engine or default_engine()
        eng.hs_static_set(localKeypair.data())
        status, init = eng.hs_open_host(remoteEphemeral.data(), _bytes(encryptedStatic), _bytes(encryptedTimestamp))
        if status == L.WG_HS_OPEN_BADAUTH:
            raise AEADBadTagException("Tag mismatch")
        if init is None:
            raise L.WgError(L.WG_EINVAL, f"wg_hs_open status {status}")
        return NoisePublicKey(init["remote_static"].tobytes())

    @staticmethod
    def openTimestamp(localKeypair: NoisePrivateKey, remoteEphemeral: NoisePublicKey, encryptedStatic,
                      encryptedTimestamp, engine: Engine | None = None) -> bytes:
        """The 12 bytes the initiator sealed as its timestamp, or AEADBadTagException when encryptedStatic or
        encryptedTimestamp does not verify. This mirrors NOTHING in the reference, whose responder mixes
        encryptedTimestamp into the hash unopened (Handshakes.java:233-234): it is the responder's state of
        decryptRemoteStatic taken one step further, through wg_hs_dh + wg_hs_open + wg_hs_stamp. localKeypair
        becomes the engine's static key and the initiator's static key its one peer, whose stored timestamp
        starts at zero: the call opens, it does not judge freshness (Engine.hs_stamp over a ring does)."""
        eng = engine or default_engine()
        eng.hs_static_set(localKeypair.data())
        fields = (remoteEphemeral.data(), _bytes(encryptedStatic), _bytes(encryptedTimestamp))
        status, init = eng.hs_open_host(*fields)
        if status == L.WG_HS_OPEN_BADAUTH:
            raise AEADBadTagException("Tag mismatch")
        if init is None:
            raise L.WgError(L.WG_EINVAL, f"wg_hs_open status {status}")
        eng.hs_peers_set([init["remote_static"].tobytes()])
        status, init = eng.hs_open_host(*fields)
        if status != L.WG_HS_OPEN_OK:
            raise L.WgError(L.WG_EINVAL, f"wg_hs_open status {status}")
        (ss, _), = eng.x25519_host([(localKeypair.data(), remoteEphemeral.data())])
        msg = (bytes([1, 0, 0, 0, 0, 0, 0, 0]) + b"".join(bytes(f) for f in fields)).ljust(L.WG_HS_INIT_SIZE, b"\0")
        ts_status, opened = eng.hs_stamp_host(init, msg, ss)
        if ts_status == L.WG_HS_TS_BADAUTH:
            raise AEADBadTagException("Tag mismatch")
        if opened is None:
            raise L.WgError(L.WG_EINVAL, f"wg_hs_stamp status {ts_status}")
        return opened

    @staticmethod
    def responderHandshake(localKeypair: NoisePrivateKey, remoteEphemeral: NoisePublicKey, encryptedStatic,
                           encryptedTimestamp, engine: Engine | None = None, ephemeral=None,
                           localIndex: int = 0) -> "ResponderHandshake":
        """Handshakes.responderHandshake (Handshakes.java:47-50): both phases of the responder, on the device."""
        return ResponderHandshake(localKeypair, remoteEphemeral, encryptedStatic, encryptedTimestamp, engine, ephemeral,
                                  localIndex)

    @staticmethod
    def initiateHandshake(localKeypair: NoisePrivateKey, remotePublicKey: NoisePublicKey,
                          presharedKey: NoisePresharedKey | None = None, engine: Engine | None = None, ephemeral=None,
                          timestamp=None, senderIndex: int = 0) -> "InitiatorStageOne":
        """Handshakes.initiateHandshake (Handshakes.java:43-45): the initiator's first stage, on the device."""
        return InitiatorStageOne(localKeypair, remotePublicKey, presharedKey, engine, ephemeral, timestamp, senderIndex)


class InitiatorStageOne:
    """Handshakes.InitiatorStageOne (Handshakes.java:52-164): the constructor's chain and the initiation message
    through wg_hs_initiate, consumeMessageResponse through wg_hs_finish. localKeypair becomes the engine's static
    key, remotePublicKey its one peer and presharedKey (None: zero) that peer's psk. `ephemeral` is the fresh
    ephemeral private key (None: 32 bytes of os.urandom, as NoisePrivateKey.newPrivateKey draws them), `timestamp`
    the 12 bytes that are sealed (None: Crypto.TAI64N() now)."""

    def __init__(self, localKeypair: NoisePrivateKey, remotePublicKey: NoisePublicKey,
                 presharedKey: NoisePresharedKey | None = None, engine: Engine | None = None, ephemeral=None, timestamp=None,
                 senderIndex: int = 0):
        eng = self._engine = engine or default_engine()
        self._local, self._remote = localKeypair, remotePublicKey
        self._psk = presharedKey if presharedKey is not None else NoisePresharedKey.zero()
        self._install()
        eph = bytes(ephemeral.data() if isinstance(ephemeral, NoisePrivateKey) else ephemeral) if ephemeral is not None \
            else os.urandom(32)
        ts = bytes(timestamp) if timestamp is not None else Crypto.TAI64N()
        status, msg, pending = eng.hs_initiate_host(0, eph, ts, senderIndex)
        if msg is None:
            raise L.WgError(L.WG_EINVAL, f"wg_hs_initiate status {status}")
        self._message, self._pending = msg, pending
        self._ephemeral_private = eph

    def _install(self):
        eng = self._engine
        eng.hs_static_set(self._local.data())
        eng.hs_peers_set([self._remote.data()])
        eng.hs_psks_set([self._psk.data()])

    def initiation(self, senderIndex: int | None = None) -> bytes:
        """The 148-byte message (OutgoingInitiation.java:22-38). Another senderIndex than the constructor's is
        written into it, with mac1 computed again (InitiationPacket.java:110-120)."""
        if senderIndex is None or (senderIndex & 0xFFFFFFFF) == int(self._pending["local_index"]):
            return self._message
        from .crypto import calculate_mac1
        head = self._message[:4] + (senderIndex & 0xFFFFFFFF).to_bytes(4, "little") + self._message[8:116]
        return head + calculate_mac1(head, self._remote.data()) + bytes(16)

    def consumeMessageResponse(self, remoteEphemeral: NoisePublicKey, encryptedEmpty) -> "SymmetricKeypair":
        """Handshakes.java:119-151: the transport keys, or AEADBadTagException (a BadPaddingException) when
        encryptedEmpty does not verify; the stage can then be tried on another response, as the reference's can
        not (its hash and chain key are spent either way)."""
        empty = _bytes(encryptedEmpty)
        if len(empty) != 16:
            raise AEADBadTagException("Tag mismatch")
        self._install()
        response = bytes([2, 0, 0, 0]) + bytes(4) + int(self._pending["local_index"]).to_bytes(4, "little") + \
            remoteEphemeral.data() + empty + bytes(32)
        status, est = self._engine.hs_finish_host(self._pending, response)
        if status == L.WG_HS_FIN_BADAUTH:
            raise AEADBadTagException("Tag mismatch")
        if est is None:
            raise L.WgError(L.WG_EINVAL, f"wg_hs_finish status {status}")
        kp = SymmetricKeypair(est["send_key"].tobytes(), est["recv_key"].tobytes(), engine=self._engine)
        est["send_key"] = 0
        est["recv_key"] = 0
        return kp

    def getLocalEphemeral(self) -> NoisePrivateKey:
        return NoisePrivateKey(self._ephemeral_private, NoisePublicKey(self._message[8:40]))

    def getEncryptedStatic(self) -> bytes:
        return self._message[40:88]

    def getEncryptedTimestamp(self) -> bytes:
        return self._message[88:116]


class ResponderHandshake:
    """Handshakes.ResponderHandshake (Handshakes.java:166-303): decryptRemoteStatic through wg_hs_dh + wg_hs_open,
    deriveKeypair and the response message through wg_hs_respond. `ephemeral` is the fresh ephemeral private key
    (None: 32 bytes of os.urandom, as NoisePrivateKey.newPrivateKey draws them); localIndex is the responder's
    session index in the response. Like the reference it answers an initiator no peer table holds: for such an
    entry wg_hs_open stops before the static-static step, which one ladder and one KDF1 finish here."""

    def __init__(self, localKeypair: NoisePrivateKey, remoteEphemeral: NoisePublicKey, encryptedStatic, encryptedTimestamp,
                 engine: Engine | None = None, ephemeral=None, localIndex: int = 0):
        eng = engine or default_engine()
        eng.hs_static_set(localKeypair.data())
        status, init = eng.hs_open_host(remoteEphemeral.data(), _bytes(encryptedStatic), _bytes(encryptedTimestamp))
        if status == L.WG_HS_OPEN_BADAUTH:
            raise AEADBadTagException("Tag mismatch")
        if init is None:
            raise L.WgError(L.WG_EINVAL, f"wg_hs_open status {status}")
        init = init.copy()
        if status == L.WG_HS_OPEN_NEWPEER:  # Handshakes.java:232-233
            (ss, _), = eng.x25519_host([(localKeypair.data(), init["remote_static"].tobytes())])
            init["chain_key"] = np.frombuffer(Crypto.deriveKey(init["chain_key"].tobytes(), ss), np.uint8)
        eph = bytes(ephemeral.data() if isinstance(ephemeral, NoisePrivateKey) else ephemeral) if ephemeral is not None \
            else os.urandom(32)
        rs, sess = eng.hs_respond_host(init, eph, localIndex)
        if sess is None:
            raise L.WgError(L.WG_EINVAL, f"wg_hs_respond status {rs}")
        self.response = sess["response"].tobytes()
        self._remote = NoisePublicKey(init["remote_static"].tobytes())
        self._keypair = SymmetricKeypair(sess["send_key"].tobytes(), sess["recv_key"].tobytes(), engine=eng)
        sess["send_key"] = 0
        sess["recv_key"] = 0

    def getKeypair(self) -> "SymmetricKeypair":
        return self._keypair

    def getRemotePublicKey(self) -> NoisePublicKey:
        return self._remote

    def getEncryptedEmpty(self) -> bytes:
        return self.response[44:60]

    def getLocalEphemeral(self) -> NoisePublicKey:
        return NoisePublicKey(self.response[12:44])


class SymmetricKeypair:
    def __init__(self, sendKey: bytes, receiveKey: bytes, engine: Engine | None = None):
        """SymmetricKeypair(byte[] sendKeyBytes, byte[] receiveKeyBytes) (SymmetricKeypair.java:39-50)."""
        self._engine = engine or default_engine()
        self._send_slot, self._recv_slot = self._engine.alloc_slots(2)
        # one upload per slot: after frees the two claimed slots need not be adjacent
        self._engine.set_keys(self._send_slot, bytes(sendKey))
        self._engine.set_keys(self._recv_slot, bytes(receiveKey))
        self._counter = 0  # volatile long sendCounter = 0 (:37)
        self._lock = threading.Lock()
        self._clean = False

    @property
    def send_slot(self) -> int:
        return self._send_slot

    @property
    def receive_slot(self) -> int:
        return self._recv_slot

    def _next(self, n: int = 1) -> int:
        with self._lock:  # SEND_COUNTER.getAndAdd(this, n) (:64)
            c = self._counter
            self._counter += n
            return c

    def _live(self):
        if self._clean:  # the reference's keys live in a closed Arena after clean() (:85-93)
            raise IllegalStateException("SymmetricKeypair used after clean()")

    def cipher(self, src, dst) -> int:
        """dst = ct || tag (L + 16 bytes); returns the counter used (SymmetricKeypair.java:63-74)."""
        self._live()
        counter = self._next()
        pt = _bytes(src)
        if _size(dst) < len(pt) + 16:
            raise IndexError("dst too small for ciphertext and tag")
        _write(dst, self._engine.seal1(self._send_slot, counter, pt))
        return counter

    def decipher(self, counter: int, src, dst) -> None:
        """src = ct || tag; plaintext of L = |src| - 16 bytes into dst (SymmetricKeypair.java:76-83)."""
        self._live()
        data = _bytes(src)
        if len(data) < 16:
            raise IndexError("ciphertext shorter than the 16-byte tag")  # asSlice(textLength, 16) fails
        pt = self._engine.open1(self._recv_slot, counter, data)
        if pt is None:
            raise AEADBadTagException("Invalid tag")
        _write(dst, pt)

    def clean(self) -> None:
        """Zero both keys (SymmetricKeypair.java:85-93). Runs once: a second clean() is a
        no-op, so the slots cannot be released twice."""
        with self._lock:
            if self._clean:
                return
            self._clean = True
        self._engine.free_slots([self._send_slot, self._recv_slot])

    # ---- additive batch API (device-resident) --------------------------------------
    def cipher_batch(self, inp, in_offsets, lengths, out, out_offsets, uniform: bool = False, stream=None):
        """Seal n packets of the torch uint8 device buffer `inp` into `out` (ct || tag each).
        Consumes n consecutive counters; returns (first_counter, desc_tensor)."""
        import torch
        self._live()
        n = len(lengths)
        c0 = self._next(n)
        d = pack_desc(in_offsets, out_offsets, np.arange(c0, c0 + n, dtype=np.uint64), lengths, self._send_slot)
        dt = torch.from_numpy(desc_as_int64(d)).to(inp.device)
        max_len = int(np.max(lengths)) if n else 0
        self._engine.seal(dt, inp, out, max_len, uniform=uniform, stream=stream)
        return c0, dt

    def decipher_batch(self, inp, in_offsets, counters, lengths, out, out_offsets, uniform: bool = False,
                       stream=None):
        """Open n packets (ct || tag at in_offsets, L = lengths); returns the device status tensor."""
        import torch
        self._live()
        n = len(lengths)
        d = pack_desc(in_offsets, out_offsets, counters, lengths, self._recv_slot)
        dt = torch.from_numpy(desc_as_int64(d)).to(inp.device)
        status = torch.empty(n, dtype=torch.int32, device=inp.device)
        max_len = int(np.max(lengths)) if n else 0
        self._engine.open(dt, inp, out, status, max_len, uniform=uniform, stream=stream)
        return status
