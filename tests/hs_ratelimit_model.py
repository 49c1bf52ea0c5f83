"""Pure-Python model of the handshake rate limiter on the device (include/wgaead.h, wg_hs_rl_* and wg_hs_ratelimit):
the batched closed form that the kernels follow, with the BADSRC, FULL and COMPACT rules, compaction, dump and load.

A call judges its records at one `now`: a source with c records has the allowance a = min(max, tokens + age) // cost,
its min(a, c) lowest positions pass, and its entry ends as {refilled - min(a, c) cost, max(last, now)}. The sequential
rule this is the closed form of is noise.RateLimiter; tests/test_hs_ratelimit.py holds the two together.

Dump order. The device dumps in table order, and which bucket of a probe chain an entry holds depends on the order in
which threads claimed them; what a lookup answers does not. The model's dump is therefore SORTED (family, address
bytes), and a device dump is compared after the same sort (sorted_dump)."""
import numpy as np

RL_OK, RL_LIMITED, RL_FULL, RL_BADSRC = 0, 1, 2, 3
MAX_BURST = 16
U64 = (1 << 64) - 1
HS_SRC = np.dtype([("addr", "u1", (16,)), ("port", "u1", (2,)), ("family", "u1"), ("_pad", "u1", (5,))])
RL_ENTRY = np.dtype([("addr", "u1", (8,)), ("family", "u1"), ("_pad", "u1", (7,)), ("tokens", "<u8"), ("last", "<u8")])


def capacity(max_sources: int) -> int:
    """The smallest power of two >= max(8, 2 max_sources)."""
    cap = 8
    while cap < 2 * max_sources:
        cap <<= 1
    return cap


def key_of(s):
    """The bucket's key of one HS_SRC entry, or None: {family, addr[0 .. 4)} or {family, addr[0 .. 8)}."""
    fam = int(s["family"])
    if fam not in (4, 6):
        return None
    return fam, bytes(s["addr"][:4 if fam == 4 else 8])


def src_array(sources) -> np.ndarray:
    """HS_SRC entries from (family, addr bytes, port) tuples; addr is padded with zeros to 16 bytes."""
    out = np.zeros(len(sources), HS_SRC)
    for j, (fam, addr, port) in enumerate(sources):
        out[j]["addr"][:len(addr)] = np.frombuffer(bytes(addr), np.uint8)
        out[j]["port"] = [port >> 8, port & 0xFF]
        out[j]["family"] = fam
    return out


def sorted_dump(entries: np.ndarray) -> np.ndarray:
    """A dump in the model's order."""
    e = np.asarray(entries, RL_ENTRY).reshape(-1)
    order = sorted(range(len(e)), key=lambda j: (int(e[j]["family"]), bytes(e[j]["addr"])))
    return e[order]


class Limiter:
    def __init__(self, max_sources: int, cost: int = 0, burst: int = 0):
        self.C = capacity(max_sources)
        self.cost, self.burst = cost, burst
        self.entries = {}  # key -> [tokens, last]

    @property
    def max(self) -> int:
        return self.cost * self.burst

    def config_set(self, cost: int, burst: int) -> None:
        assert 1 <= cost <= 1 << 56 and 1 <= burst <= MAX_BURST
        self.cost, self.burst = cost, burst

    def _age(self, last: int, now: int) -> int:
        return now - last if now >= last else 0

    def stale(self, key, now: int) -> bool:
        return self._age(self.entries[key][1], now) >= self.max

    def compact(self, now: int):
        """wg_hs_rl_compact: (kept, dropped)."""
        drop = [k for k in self.entries if self.stale(k, now)]
        for k in drop:
            del self.entries[k]
        return len(self.entries), len(drop)

    def ratelimit(self, indices, src, now: int, n_records=None, compact: bool = False):
        """One wg_hs_ratelimit over the records whose batch indices are `indices`: (status per position below
        min(n_records, n), the passing positions in order, the summary dict)."""
        n = len(indices)
        nl = n if n_records is None else min(n_records, n)
        st = [RL_BADSRC] * nl
        keys = []
        for k in range(nl):
            i = int(indices[k])
            keys.append(key_of(src[i]) if i < len(src) else None)
        if n and now == 0:
            st = [RL_OK if keys[k] is not None else RL_BADSRC for k in range(nl)]
        elif n:
            if compact and len(self.entries) + nl > self.C // 2:
                self.compact(now)
            m = sum(1 for k in range(nl) if keys[k] is not None and keys[k] not in self.entries)
            full = len(self.entries) + m > self.C // 2
            by_key = {}
            for k in range(nl):
                if keys[k] is None:
                    continue
                if keys[k] not in self.entries and full:
                    st[k] = RL_FULL
                    continue
                by_key.setdefault(keys[k], []).append(k)
            for key, pos in by_key.items():
                tokens, last = self.entries.get(key, (self.max, now))
                refilled = min(self.max, min(U64, tokens + self._age(last, now)))
                a = refilled // self.cost
                take = min(a, len(pos))
                for j, k in enumerate(pos):  # (positions rise)
                    st[k] = RL_OK if j < take else RL_LIMITED
                self.entries[key] = [refilled - take * self.cost, max(last, now)]
        passed = [k for k in range(nl) if st[k] == RL_OK]
        summary = dict(n_passed=len(passed), n_limited=st.count(RL_LIMITED), n_full=st.count(RL_FULL),
                       n_badsrc=st.count(RL_BADSRC))
        return st, passed, summary

    def dump(self) -> np.ndarray:
        out = np.zeros(len(self.entries), RL_ENTRY)
        for j, ((fam, addr), (tokens, last)) in enumerate(sorted(self.entries.items())):
            out[j]["addr"][:len(addr)] = np.frombuffer(addr, np.uint8)
            out[j]["family"] = fam
            out[j]["tokens"], out[j]["last"] = tokens, last
        return out

    def load(self, entries) -> None:
        e = np.asarray(entries, RL_ENTRY).reshape(-1)
        assert len(e) <= self.C // 2
        self.entries = {}
        for x in e:
            fam = int(x["family"])
            key = (fam, bytes(x["addr"][:4 if fam == 4 else 8]))
            assert fam in (4, 6) and key not in self.entries
            self.entries[key] = [int(x["tokens"]), int(x["last"])]
