"""MT19937 on word positions and its GF(2) polynomial arithmetic, restated in plain Python (integers as bit sets): what
transflow_amd/csrc/mt19937_common.h is held to in tests/test_mt_ref.py, itself anchored to numpy's RandomState there.

The raw (untempered) words obey  x[k + 624] = x[k + 397] ^ twist(x[k], x[k + 1])  at every k, so any 624 consecutive raw
words are a state.  A polynomial is an int: bit i is the coefficient of t^i."""
from __future__ import annotations

NW, MW, DEG = 624, 397, 19937
UPPER, LOWER, MAG = 0x80000000, 0x7FFFFFFF, 0x9908B0DF
M32 = 0xFFFFFFFF


def seed_key(seed: int) -> list:
    """init_genrand: the key numpy.random.seed(seed) makes (pos = 624)."""
    key = [seed & M32]
    for i in range(1, NW):
        key.append((1812433253 * (key[-1] ^ (key[-1] >> 30)) + i) & M32)
    return key


def next_word(a: int, b: int, c: int) -> int:
    y = (a & UPPER) | (b & LOWER)
    return c ^ (y >> 1) ^ (MAG if b & 1 else 0)


def temper(y: int) -> int:
    y ^= y >> 11
    y ^= (y << 7) & 0x9D2C5680
    y ^= (y << 15) & 0xEFC60000
    y ^= y >> 18
    return y & M32


def raw_stream(key, count: int) -> list:
    """x[0 .. count) of the stream whose first 624 words are key."""
    x = [int(v) for v in key[:NW]]
    while len(x) < count:
        k = len(x) - NW
        x.append(next_word(x[k], x[k + 1], x[k + MW]))
    return x[:count] if count < NW else x


def window_at(key, pos: int) -> list:
    """x[pos .. pos + 623]: the state numpy's (key, pos) stands for, as 624 raw words from the next one handed out."""
    return raw_stream(key, NW + pos)[pos:pos + NW]


def to_double_bits(a: int, b: int) -> int:
    """The uint64 pattern of numpy's double ((a >> 5) * 2^26 + (b >> 6)) / 2^53."""
    import struct
    v = ((a >> 5) << 26) | (b >> 6)
    return struct.unpack("<Q", struct.pack("<d", v / 9007199254740992.0))[0]


def _parity(v: int) -> int:
    return bin(v).count("1") & 1


def berlekamp_massey(bits) -> tuple:
    """(L, C): the shortest recurrence bits[k] = XOR over i = 1 .. L of C_i bits[k - i], C_0 = 1."""
    C, B, L, m, R = 1, 1, 0, 1, 0
    for k, bit in enumerate(bits):
        R = (R << 1) | bit                      # bit i of R = bits[k - i]
        if _parity(C & R & ((1 << (L + 1)) - 1)):
            if 2 * L <= k:
                C, B, L, m = C ^ (B << m), C, k + 1 - L, 1
            else:
                C ^= B << m
                m += 1
        else:
            m += 1
    return L, C


_PHI = None


def charpoly() -> int:
    """The characteristic polynomial (degree 19937, the leading coefficient included), from one output bit."""
    global _PHI
    if _PHI is None:
        n = 2 * DEG + 64
        x = raw_stream(seed_key(4357), NW + n)
        L, C = berlekamp_massey([temper(v) >> 31 for v in x[NW:]])
        assert L == DEG, L
        _PHI = sum(1 << (L - i) for i in range(L + 1) if (C >> i) & 1)
    return _PHI


def _reduce(p: int, phi: int) -> int:
    for d in range(p.bit_length() - 1, DEG - 1, -1):
        if (p >> d) & 1:
            p ^= phi << (d - DEG)
    return p


def jump_poly(J: int) -> int:
    """t^J mod phi by square-and-multiply."""
    phi, r = charpoly(), 1
    for bit in bin(J)[2:]:
        r = _reduce(int("0".join(bin(r)[2:]), 2), phi)      # squaring over GF(2) spreads the bits
        if bit == "1":
            r = _reduce(r << 1, phi)
    return r


def poly_words(p: int, words: int = 312) -> list:
    return [(p >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(words)]
