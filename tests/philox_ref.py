"""NumPy restatement of what the throughput-mode kernels draw: hiprand's Philox4x32-10 (rocrand's
philox4x32_10_engine) and the transforms the kernels apply to its words.

Stream model (rocrand_init(seed, subsequence, offset)): key = (seed & 0xffffffff, seed >> 32); the 128-bit counter
of block b of subsequence s is (b mod 2^32, b >> 32, s mod 2^32, s >> 32) with the block index b in the low 64 bits;
word p of the subsequence is word p % 4 of block p // 4.  rocrand_init puts the state at word `offset` (substate
offset % 4), and every draw -- rocrand, rocrand4 (which straddles blocks when the substate is not 0), the uniform and
normal transforms -- takes the next words in order.  So a keyed stream is a flat sequence of 32-bit words, and each
draw is a function of the words at its positions.

Transforms (rocrand_uniform.h, rocrand_normal.h):
  uniform_double(w0, w1)  2^-53 + (w0 | (w1 >> 11) << 32) 2^-53, in (0, 1]; exact in float64
  box_muller(x, y)        u = 2^-32 + f32(x) 2^-32 and v = c + f32(y) c (c = 2 pi 2^-32 rounded to float32), both in
                          float32 as rocrand forms them; then s = sqrt(-2 log u), (sin(v) s, cos(v) s).  Here log,
                          sqrt, sin and cos are taken in float64 and the result is rounded to float32 once, so a value
                          is within a few float32 ulp of any float32 evaluation (host logf / sinf, device __sincosf).
  normal4 (rocrand4)      box_muller(w0, w1), box_muller(w2, w3)
  rocrand_normal          box_muller of the next two words: returns the first value and caches the second, which the
                          next rocrand_normal returns without drawing (other draws leave the cache alone)

Generator adapters: LaneStream (LaneGen<RNG_PHILOX>, one stateful hiprand state per walker) and WaveStream
(WaveGen<RNG_PHILOX>, wide.hip: every draw at a block-aligned position computed from a fresh state) serve one walker's
stream through the interface the oracle's proposal functions call (random, uniform, standard_normal, integers,
shuffle), in the order the kernels draw; each counts the words it consumes.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)

F32_2POW32_INV = np.float32(2.3283064e-10)        # ROCRAND_2POW32_INV: 2^-32 exactly
F32_2POW32_INV_2PI = np.float32(1.46291807e-09)   # ROCRAND_2POW32_INV_2PI
TWO_POW_M53 = 2.0**-53                            # ROCRAND_2POW53_INV_DOUBLE (1.1102230246251565e-16 = 2^-53)
assert float(F32_2POW32_INV) == 2.0**-32


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox_blocks(seed, seq, block):
    """Philox4x32-10 of the counters (block, seq) under key `seed` (broadcast arrays of Python ints / uint64):
    uint32 array [..., 4], the block's four words in stream order."""
    seed, seq, block = np.broadcast_arrays(_u64(seed), _u64(seq), _u64(block))
    k0, k1 = seed & MASK32, seed >> S32
    c0, c1 = block & MASK32, block >> S32
    c2, c3 = seq & MASK32, seq >> S32
    with np.errstate(over="ignore"):
        for r in range(10):
            if r:
                k0 = (k0 + W0) & MASK32
                k1 = (k1 + W1) & MASK32
            p0 = M0 * c0  # 32 x 32 -> 64 bits: no wrap in uint64
            p1 = M1 * c2
            c0, c1, c2, c3 = ((p1 >> S32) ^ c1 ^ k0), (p1 & MASK32), ((p0 >> S32) ^ c3 ^ k1), (p0 & MASK32)
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def philox_block_int(seed, seq, block):
    """philox_blocks for one counter in Python integers (the adapters' scalar path): tuple of four words."""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    c0, c1, c2, c3 = block & 0xFFFFFFFF, (block >> 32) & 0xFFFFFFFF, seq & 0xFFFFFFFF, (seq >> 32) & 0xFFFFFFFF
    for r in range(10):
        if r:
            k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
            k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
    return c0, c1, c2, c3


def words(seed, seq, pos, n):
    """Words pos .. pos + n - 1 of the subsequences `seq` (array) under `seed`: uint32 [len(seq), n].  `pos` is a
    scalar or one start per subsequence."""
    seq = np.atleast_1d(_u64(seq))
    pos = np.broadcast_to(_u64(pos), seq.shape)
    first = pos >> np.uint64(2)
    nb = (int(n) + 3) // 4 + 1
    blk = philox_blocks(seed, seq[:, None], first[:, None] + np.arange(nb, dtype=np.uint64)[None, :])
    flat = blk.reshape(len(seq), 4 * nb)
    sub = (pos & np.uint64(3)).astype(np.int64)
    idx = sub[:, None] + np.arange(int(n))[None, :]
    return np.take_along_axis(flat, idx, axis=1)


# ---- transforms ---------------------------------------------------------------------------------------------------
def uniform_double(w0, w1):
    """rocrand's uniform_distribution_double(v1, v2): (0, 1], exact."""
    m = _u64(w0) | ((_u64(w1) >> np.uint64(11)) << S32)
    return TWO_POW_M53 + m.astype(np.float64) * TWO_POW_M53


def box_muller(x, y):
    """rocrand's box_muller(x, y) as a float32 pair (first, second).  u and v are formed in float32 exactly as rocrand
    forms them (v = c + f32(y) c with the product and the sum each rounded, as written); the transcendental part is
    evaluated in float64 and rounded once."""
    xf = np.asarray(x, dtype=np.uint32).astype(np.float32)
    yf = np.asarray(y, dtype=np.uint32).astype(np.float32)
    u = np.float32(F32_2POW32_INV + xf * F32_2POW32_INV)
    v = np.float32(F32_2POW32_INV_2PI + np.float32(yf * F32_2POW32_INV_2PI))
    s = np.sqrt(-2.0 * np.log(u.astype(np.float64)))
    vd = v.astype(np.float64)
    return (np.sin(vd) * s).astype(np.float32), (np.cos(vd) * s).astype(np.float32)


def normal4(w):
    """rocrand's normal_distribution4 of words [..., 4] -> float32 [..., 4]."""
    a, b = box_muller(w[..., 0], w[..., 1])
    c, d = box_muller(w[..., 2], w[..., 3])
    return np.stack([a, b, c, d], axis=-1)


def interval_mask(mx):
    mask = int(mx)
    for s in (1, 2, 4, 8, 16):
        mask |= mask >> s
    return mask


# ---- generator adapters -------------------------------------------------------------------------------------------
class _Stream:
    """One walker's keyed word stream with a position and a word counter."""

    def __init__(self, seed, seq, offset):
        self.seed, self.seq, self.pos = int(seed), int(seq), int(offset)
        self.start = self.pos
        self._blk, self._blk_i = None, -1

    @property
    def consumed(self):
        return self.pos - self.start

    def take(self, n):
        """The next n words (uint32 array)."""
        out = np.empty(n, dtype=np.uint32)
        for j in range(n):
            b = (self.pos + j) >> 2
            if b != self._blk_i:
                self._blk, self._blk_i = philox_block_int(self.seed, self.seq, b), b
            out[j] = self._blk[(self.pos + j) & 3]
        self.pos += n
        return out

    def words_at(self, p, n):
        return words(self.seed, [self.seq], p, n)[0]


class LaneStream(_Stream):
    """LaneGen<RNG_PHILOX>: one hiprand state per walker (walk.hip, walk2.hip, walkq.hip).

    flip=True: uniforms are 1 - hiprand_uniform_double, in [0, 1) (LaneGen::uniform, the slice and unit-cube / bound
    kernels); flip=False: hiprand_uniform_double itself, in (0, 1] (the rwalk kernels' radius and non-clustered
    coordinates).  normal_mode='normal4': a vector of n normals is ceil(n / 4) hiprand_normal4 calls (rwalk);
    'cached': n hiprand_normal calls with rocrand's cached second value (LaneGen::normal, the slice kernels)."""

    def __init__(self, seed, seq, offset, flip=True, normal_mode="normal4"):
        super().__init__(seed, seq, offset)
        self.flip, self.normal_mode = flip, normal_mode
        self.cache = None

    def _u(self):
        w = self.take(2)
        u = float(uniform_double(w[0], w[1]))
        return 1.0 - u if self.flip else u

    def random(self, size=None):
        if size is None:
            return self._u()
        return np.array([self._u() for _ in range(int(np.prod(size)))]).reshape(size)

    def uniform(self, size=None):
        return self.random(size)

    def normal(self):
        if self.cache is not None:
            z, self.cache = self.cache, None
            return z
        w = self.take(2)
        a, b = box_muller(w[0], w[1])
        self.cache = float(b)
        return float(a)

    def standard_normal(self, size=None):
        n = 1 if size is None else int(np.prod(size))
        if self.normal_mode == "normal4":
            nb = (n + 3) // 4
            z = normal4(self.take(4 * nb).reshape(nb, 4)).reshape(-1)[:n].astype(np.float64)
        else:
            z = np.array([self.normal() for _ in range(n)])
        return float(z[0]) if size is None else z.reshape(size)

    def interval(self, mx):
        if mx == 0:
            return 0
        mask = interval_mask(mx)
        while True:
            v = int(self.take(1)[0]) & mask
            if v <= mx:
                return v

    def integers(self, low, high=None, size=None):
        if high is None:
            low, high = 0, low
        if size is None:
            return low + self.interval(high - 1 - low)
        return np.array([low + self.interval(high - 1 - low) for _ in range(int(np.prod(size)))]).reshape(size)

    def shuffle(self, x):
        """numpy's Generator.shuffle order (Fisher-Yates from the end, j = interval(i)): walk2.hip's SliceSampler."""
        for i in range(len(x) - 1, 0, -1):
            j = self.interval(i)
            x[i], x[j] = x[j], x[i]


class WaveStream(_Stream):
    """WaveGen<RNG_PHILOX> (wide.hip): one stream per walker, `pos` advancing in whole blocks from the key's offset
    rounded up to a multiple of 4 (the wide entry points round it so).  A scalar uniform takes
    a whole 4-word block (the first two words); an interval takes blocks until one of the block's four words passes;
    n doubles take 2 ceil(n / 2) words, the pair i, i + 1 from pos + 2 i (hiprand_uniform2_double); n normals take
    4 ceil(n / 4) words, the four from pos + i (hiprand_normal4).  Uniforms are 1 - hiprand's."""

    def __init__(self, seed, seq, offset):
        super().__init__(seed, seq, (int(offset) + 3) & ~3)

    def _u(self):
        w = self.take(4)
        return 1.0 - float(uniform_double(w[0], w[1]))

    def random(self, size=None):
        if size is None:
            return self._u()
        return self.doubles(int(np.prod(size))).reshape(size)

    def uniform(self, size=None):
        return self.random(size)

    def doubles(self, n):
        w = self.take(4 * ((n + 1) // 2)).reshape(-1, 4)
        d = np.stack([uniform_double(w[:, 0], w[:, 1]), uniform_double(w[:, 2], w[:, 3])], axis=-1).reshape(-1)
        return 1.0 - d[:n]

    def standard_normal(self, size=None):
        n = 1 if size is None else int(np.prod(size))
        nb = (n + 3) // 4
        z = normal4(self.take(4 * nb).reshape(nb, 4)).reshape(-1)[:n].astype(np.float64)
        return float(z[0]) if size is None else z.reshape(size)

    def interval(self, mx):
        if mx == 0:
            return 0
        mask = interval_mask(mx)
        while True:
            for v in self.take(4):
                if int(v) & mask <= mx:
                    return int(v) & mask

    def integers(self, low, high=None, size=None):
        if high is None:
            low, high = 0, low
        if size is None:
            return low + self.interval(high - 1 - low)
        return np.array([low + self.interval(high - 1 - low) for _ in range(int(np.prod(size)))]).reshape(size)

    def shuffle(self, x):
        for i in range(len(x) - 1, 0, -1):
            j = self.interval(i)
            x[i], x[j] = x[j], x[i]
