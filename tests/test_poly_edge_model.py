"""poly_edge_model on its own (no GPU): every steered ciphertext has the residue it claims under an independent
evaluation, both oracles accept it, the retries stay under the cap, the limb models agree with the big-integer
tag, and the per-packet path has cases whose modelled representation enters poly_finish in [p, 2^130)."""
import random

import pytest

import poly_edge_model as PM
from wgtest import oracle, splitmix_bytes

O = oracle()
LENGTHS = [48, 64, 100, 448, 1424]  # the smallest, a round number of chunks, a partial last block, two round ends
AAD = bytes(range(0x40, 0x4C))


def _case(ti, fi, L):
    seed = 1000 * ti + 10 * fi + L
    key = splitmix_bytes(0xED6E00 + seed, 32)
    counter = int.from_bytes(splitmix_bytes(0xC0 + seed, 8), "little")
    return key, counter, (ti + fi + L // 16) % (L // 16), random.Random(seed)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("fill", PM.FILLS)
def test_steered_ciphertexts_have_their_residue(L, fill):
    worst = 0
    for ti, target in enumerate(PM.TARGETS):
        key, counter, free, rng = _case(ti, PM.FILLS.index(fill), L)
        H = PM.resolve(target, key, counter)
        ct, tries = PM.steer_tries(key, counter, L, free, H, fill, rng)
        worst = max(worst, tries)
        assert len(ct) == L, PM.label(target)
        otk = PM.one_time_key(key, counter)
        # independent evaluation: the oracle's Poly1305 over the padded MAC input with the s half zeroed
        tag0 = O.py_poly1305(otk[:16] + bytes(16), PM.mac_input(ct))
        assert int.from_bytes(tag0, "little") == H & PM.M128, PM.label(target)
        assert PM.residue(otk, PM.mac_input(ct)) == H, PM.label(target)
        tag = PM.tag_of(key, counter, ct)
        if target[0] == "T":
            assert tag == target[1]
        nonce = O.transport_nonce(counter)
        pt = O.py_aead_open(key, nonce, ct + tag)
        assert pt is not None and pt == O.py_chacha20(key, nonce, 1, ct), PM.label(target)
        assert O.c_aead_open(key, nonce, ct + tag) == pt, PM.label(target)
        if fill != "rand":  # whatever is neither the free nor a redrawn salt block is the fill
            other = [b for b in range(L // 16) if b != free and b != (0 if free else 1)]
            want = {"ff": 0xFF, "00": 0}[fill]
            assert all(x == want for b in other for x in ct[16 * b:16 * b + 16]) and all(x == want for x in ct[L & ~15:])
    assert worst < PM.MAX_TRIES


def test_steer_takes_aad_blocks_and_an_explicit_nonce():
    for ti, target in enumerate(PM.TARGETS[::4]):
        key, _, free, rng = _case(ti, 0, 64)
        nonce = splitmix_bytes(0xA0 + ti, 12)
        H = PM.resolve(target, key, 0, nonce)
        ct = PM.steer(key, 0, 64, free, H, "rand", rng, aad=AAD, nonce=nonce)
        otk = PM.one_time_key(key, 0, nonce)
        assert PM.residue(otk, PM.mac_input(ct, AAD)) == H
        tag = PM.tag_of(key, 0, ct, AAD, nonce)
        assert tag == O.py_aead_tag(key, nonce, AAD, ct)
        assert O.py_aead_open(key, nonce, ct + tag, AAD) is not None
        assert O.c_aead_open(key, nonce, ct + tag, AAD) == O.py_aead_open(key, nonce, ct + tag, AAD)


def test_steer_gives_up_at_the_cap():
    class Stuck:
        def getrandbits(self, n):
            return 0
    key = splitmix_bytes(1, 32)
    hits = 0
    for H in range(7, 40):
        try:
            PM.steer(key, 0, 48, 2, H, "00", Stuck())
            hits += 1
        except RuntimeError:
            pass
    assert 0 < hits < 33  # a salt that never changes: the misses raise, about one target in four hits


def test_tag_target_lists_every_residue_of_a_tag():
    key, counter = splitmix_bytes(2, 32), 77
    _, s = PM.r_s(PM.one_time_key(key, counter))
    for T in (bytes(16), b"\xff" * 16, splitmix_bytes(3, 16)):
        c = PM.tag_target(key, counter, T)
        assert len(c) in (3, 4) and c == sorted(set(c))
        assert all(h < PM.P and ((h + s) & PM.M128) == int.from_bytes(T, "little") for h in c)
        assert [h >> 128 for h in c] == list(range(len(c)))


# ---- the limb models ----------------------------------------------------------------------------------------

def test_finish_model_selects_g_from_p_on():
    s = int.from_bytes(splitmix_bytes(4, 16), "little")
    # from 2^130 on the wrapping carry passes fold the value before the select sees it
    for v, took, seen in [(0, False, 0), (4, False, 4), (PM.P - 1, False, PM.P - 1), (PM.P, True, PM.P),
                          (PM.P + 4, True, PM.P + 4), (1 << 130, False, 5), ((1 << 130) + 70, False, 75)]:
        tag, got, norm = PM.finish(PM.limbs(v), s)
        assert (got, norm) == (took, seen)
        assert int.from_bytes(tag, "little") == (v % PM.P + s) & PM.M128
    # the widest limbs a kernel hands over: 63 partial products of limbs < 2^26 + 2^8 (the first carry pass adds
    # up to 63 to a limb in 32 bits, so 2^32 - 64 is the most poly_finish can take)
    for wide in ([63 * ((1 << 26) + (1 << 8))] * 5, [(1 << 32) - 64] * 5):
        tag, _, _ = PM.finish(wide, s)
        assert int.from_bytes(tag, "little") == (PM.value(wide) % PM.P + s) & PM.M128


@pytest.mark.parametrize("L", [48, 1424])
def test_limb_models_give_the_oracles_tag(L):
    for ti, target in enumerate(PM.TARGETS):
        key, counter, free, rng = _case(ti, 0, L)
        ct = PM.steer(key, counter, L, free, PM.resolve(target, key, counter), "rand", rng)
        otk = PM.one_time_key(key, counter)
        s = PM.r_s(otk)[1]
        want = PM.tag_of(key, counter, ct)
        assert PM.finish(PM.serial_prefinish(otk, PM.mac_input(ct)), s)[0] == want
        if L == 48 or ti % 3 == 0:
            assert PM.finish(PM.pp_prefinish(otk, ct), s)[0] == want


@pytest.mark.parametrize("L", [48, 1424])
def test_per_packet_cases_that_enter_finish_at_or_above_p(L):
    found = PM.pp_select_cases(L)
    assert len(found) >= 4
    for key, counter, ct, H in found:  # on these, a select that keeps h gives another tag
        otk = PM.one_time_key(key, counter)
        s = PM.r_s(otk)[1]
        kept = ((PM.P + H) + s) & PM.M128
        assert kept != int.from_bytes(PM.tag_of(key, counter, ct), "little")


def test_serial_form_also_reaches_the_select():
    """poly_tag's form: at residues 0 .. 4 the Horner loop leaves residue + p."""
    n = 0
    for seed in range(16):
        key, counter = splitmix_bytes(0x7A6 + seed, 32), seed
        ct = PM.steer(key, counter, 64, seed % 4, seed % 5, "rand", random.Random(seed))
        otk = PM.one_time_key(key, counter)
        _, took, v = PM.finish(PM.serial_prefinish(otk, PM.mac_input(ct)), 0)
        n += took and v == PM.P + seed % 5
    assert n >= 4


# ---- raw one-time keys ------------------------------------------------------------------------------------------

def test_raw_mac_cases_are_what_they_were_built_for():
    names = set()
    for name, otk, msg, H in PM.raw_mac_cases():
        assert name not in names
        names.add(name)
        tag = O.py_poly1305(otk, msg)
        assert O.c_poly1305(otk, msg) == tag, name
        if H is not None:
            r, s = PM.r_s(otk)
            assert len(msg) % 16 == 0 and PM.residue(otk, msg) == H, name
            assert int.from_bytes(tag, "little") == (H + s) & PM.M128, name
    by = {c[0]: c for c in PM.raw_mac_cases()}
    assert O.py_poly1305(by["r1_sum_p"][1], by["r1_sum_p"][2]) == b"\xff" * 16
    assert O.py_poly1305(by["r1_ripple"][1], by["r1_ripple"][2]) == bytes(16)
    assert O.py_poly1305(by["r1_ripple_k3"][1], by["r1_ripple_k3"][2]) == bytes(16)
    assert O.py_poly1305(by["r2_ff"][1], by["r2_ff"][2]) == (3).to_bytes(16, "little")
