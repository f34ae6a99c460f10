"""The three ring samplers of the reference restated in plain Python, as functions of the byte stream their PRNG serves: the words
written, and -- through Source.pos -- the bytes consumed.  Written from reading ring/sampler_uniform.go, ring/sampler_gaussian.go
and ring/sampler_ternary.go (file:line cited per step).  Integers are Python integers; the float32 steps of the ziggurat are numpy
float32 scalars (one rounding per operation); exp and log are injectable, so that a test can move them by a few ulps.

A polynomial is a list of limbs, each a list of N integers.  `pol` given: ReadAndAdd (f = CRed(a + b, c)); absent: Read."""
from __future__ import annotations

import math

import numpy as np

MASK64 = (1 << 64) - 1


class Source:
    """An io.Reader over a deterministic stream: gen(offset, n) -> the n bytes at `offset`.  pos counts the bytes read."""

    def __init__(self, gen):
        self.gen, self.pos = gen, 0

    def read(self, n: int) -> bytes:
        out = self.gen(self.pos, n)
        assert len(out) == n
        self.pos += n
        return out


def bytes_source(data: bytes, fill: int = 0) -> Source:
    """the bytes of `data`, then the byte `fill` for ever"""
    def gen(off, n):
        head = data[off:off + n]
        return head + bytes([fill]) * (n - len(head))
    return Source(gen)


def seeded_source(seed: int) -> Source:
    """a random stream that is a function of (seed, offset) alone, whatever the sizes of the reads: 4096-byte pages of PCG64"""
    pages = {}

    def page(k):
        if k not in pages:
            if len(pages) > 64:
                pages.clear()
            pages[k] = np.random.Generator(np.random.PCG64([seed, k])).integers(0, 256, 4096, dtype=np.uint8).tobytes()
        return pages[k]

    def gen(off, n):
        out = bytearray()
        while n:
            k, o = divmod(off, 4096)
            take = min(n, 4096 - o)
            out += page(k)[o:o + take]
            off += take
            n -= take
        return bytes(out)
    return Source(gen)


def cred(a, q):  # ring/modular_reduction.go:200-205, on a 64-bit word
    a &= MASK64
    return a - q if a >= q else a


def mform(a, q):  # MForm: a 2^64 mod q, canonical
    return (a << 64) % q


def _store(pol, add, j, i, w, q):
    pol[j][i] = cred(pol[j][i] + w, q) if add else w


# ---- ring/sampler_uniform.go -------------------------------------------------------------------------------------------------
def uniform_read(src: Source, N: int, moduli, pol=None):
    """UniformSampler.read (:44-99)"""
    add = pol is not None
    if not add:
        pol = [[0] * N for _ in moduli]
    buf = src.read(1024)  # :56
    ptr = 0
    for j, qi in enumerate(moduli):  # :61
        mask = (1 << (qi - 1).bit_length()) - 1  # SubRing.Mask, ring/subring.go:63
        for i in range(N):
            while True:
                if ptr == 1024:  # :77-83
                    buf = src.read(1024)
                    ptr = 0
                r = int.from_bytes(buf[ptr:ptr + 8], "big") & mask  # :86
                ptr += 8
                if r < qi:  # :90
                    break
            _store(pol, add, j, i, r, qi)  # :95
    return pol


def uniform_read_qp(src: Source, N: int, moduliQ, moduliP, pol=None):
    """ringqp.UniformSampler.Read (ring/ringqp/samplers.go:47-55): a Read on Q, then a Read on P"""
    q = uniform_read(src, N, moduliQ, None if pol is None else pol[0])
    p = uniform_read(src, N, moduliP, None if pol is None else pol[1])
    return q, p


# ---- ring/sampler_gaussian.go ------------------------------------------------------------------------------------------------
RN = 3.442619855899  # :13


def ziggurat_tables():
    """kn, wn, fn (:267 on) from their construction (Marsaglia and Tsang 2000): 128 strips, r = 3.442619855899,
    v = 9.91256303526217e-3, m1 = 2^31; the doubles rounded once to uint32 / float32"""
    dn = tn = RN
    vn, m1 = 9.91256303526217e-3, 2147483648.0
    kn, wn, fn = [0] * 128, [0.0] * 128, [0.0] * 128
    q = vn / math.exp(-.5 * dn * dn)
    kn[0], kn[1] = int((dn / q) * m1), 0
    wn[0], wn[127] = q / m1, dn / m1
    fn[0], fn[127] = 1.0, math.exp(-.5 * dn * dn)
    for i in range(126, 0, -1):
        dn = math.sqrt(-2. * math.log(vn / dn + math.exp(-.5 * dn * dn)))
        kn[i + 1] = int((dn / tn) * m1)
        tn = dn
        fn[i] = math.exp(-.5 * dn * dn)
        wn[i] = dn / m1
    return np.array(kn, dtype=np.uint32), np.array(wn, dtype=np.float32), np.array(fn, dtype=np.float32)


KN, WN, FN = ziggurat_tables()


def _log(x):
    return -math.inf if x == 0 else math.log(x)  # math.Log(0) = -Inf


class GaussTrace:
    """what a Gaussian Read went through: the count of draws by exit, and the longest sample in stream words"""

    def __init__(self):
        self.strip = self.tail = self.wedge_accept = self.wedge_reject = self.bound_reject = 0
        self.longest = 0


def gaussian_read(src: Source, N: int, moduli, sigma: float, bound: float, montgomery: bool, pol=None, exp=math.exp, log=_log,
                  trace: GaussTrace | None = None):
    """GaussianSampler.read, the float64 branch (:68-90, :158-180), with normFloat64 (:192-265)"""
    add = pol is not None
    if not add:
        pol = [[0] * N for _ in moduli]
    tr = trace or GaussTrace()
    st = {"buf": src.read(1024), "ptr": 0, "words": 0}  # :80

    def read():  # :198-206
        if st["ptr"] == 1024:
            st["buf"] = src.read(1024)
            st["ptr"] = 0

    def rand_u32():  # :208-213: four bytes read, eight skipped
        read()
        x = int.from_bytes(st["buf"][st["ptr"]:st["ptr"] + 4], "little")
        st["ptr"] += 8
        st["words"] += 1
        return x

    def rand_f64():  # :215-220
        read()
        x = float(int.from_bytes(st["buf"][st["ptr"]:st["ptr"] + 8], "little") & 0x1fffffffffffff) / float(0x1fffffffffffff)
        st["ptr"] += 8
        st["words"] += 1
        return x

    def norm_float64():  # :222-264
        while True:
            ju = rand_u32()
            j = ju & 0x7fffffff
            sign = ju >> 31
            i = j & 0x7F
            x = float(j) * float(WN[i])
            if j < int(KN[i]):  # :236
                tr.strip += 1
                return x, sign
            if i == 0:  # :242-257
                while True:
                    x = -log(rand_f64()) * (1.0 / RN)
                    y = -log(rand_f64())
                    if y + y >= x * x:
                        break
                tr.tail += 1
                return x + RN, sign
            lhs = FN[i] + np.float32(rand_f64()) * (FN[i - 1] - FN[i])  # :260, float32 throughout
            if lhs < np.float32(exp(-0.5 * x * x)):
                tr.wedge_accept += 1
                return x, sign
            tr.wedge_reject += 1

    for i in range(N):  # :160
        st["words"] = 0
        while True:
            norm, sign = norm_float64()
            v = norm * sigma  # :165
            if v <= bound:
                c = int(v + 0.5)  # :166
                break
            tr.bound_reject += 1
        tr.longest = max(tr.longest, st["words"])
        for j, qi in enumerate(moduli):  # :171-173
            w = ((c * sign) | ((qi - c) * (sign ^ 1))) & MASK64
            _store(pol, add, j, i, w, qi)
    if montgomery:  # :177-179: the whole polynomial
        for j, qi in enumerate(moduli):
            pol[j] = [mform(w, qi) for w in pol[j]]
    return pol


def shifted(f, ulps: int):
    """f moved by `ulps` units in the last place (up for positive), infinities and zeros left alone"""
    def g(x):
        y = f(x)
        if math.isinf(y) or math.isnan(y):
            return y
        for _ in range(abs(ulps)):
            y = math.nextafter(y, math.inf if ulps > 0 else -math.inf)
        return y
    return g


# ---- ring/sampler_ternary.go -------------------------------------------------------------------------------------------------
PRECISION = 56  # :11


class WalkOutOfColumns(Exception):
    """matrixProba[row][55]: an index panic in the reference"""


def ternary_matrix(p: float):
    """computeMatrixTernary(p) (:106-128), p = the inverse density"""
    m = [[0] * (PRECISION - 1) for _ in range(2)]
    for row, g in ((0, p), (1, 1 - p)):
        x = int(g * 2.0 ** PRECISION)  # uint64(g) truncates
        for j in range(PRECISION - 1):
            m[row][j] = (x >> (PRECISION - j - 1)) & 1
    return m


def matrix_values(moduli, montgomery: bool):
    """initializeMatrix (:82-104)"""
    return [[0, mform(1, q) if montgomery else 1, mform(q - 1, q) if montgomery else q - 1] for q in moduli]


class KyTrace:
    def __init__(self):
        self.restarts = self.sign_from_next_byte = self.refills = 0
        self.longest_walk = 0


def matrix_from_words(x0: int, x1: int):
    return [[(x >> (PRECISION - j - 1)) & 1 for j in range(PRECISION - 1)] for x in (x0, x1)]


def ternary_read(src: Source, N: int, moduli, P: float, montgomery: bool, pol=None, trace: KyTrace | None = None, words=None):
    """TernarySampler.sampleProba (:130-196) for Ternary{P: P}; words = (x0, x1): the walk over matrix_from_words instead"""
    add = pol is not None
    if not add:
        pol = [[0] * N for _ in moduli]
    tr = trace or KyTrace()
    inv_density = 1 - P  # :34
    lut = matrix_values(moduli, montgomery)
    if inv_density == 0.5 and words is None:  # :147-171
        rc = src.read(N >> 3)
        rs = src.read(N >> 3)
        for i in range(N):
            coeff = (rc[i >> 3] >> (i & 7)) & 1
            sign = (rs[i >> 3] >> (i & 7)) & 1
            index = (coeff & (sign ^ 1)) | ((sign & coeff) << 1)
            for j, qi in enumerate(moduli):
                _store(pol, add, j, i, lut[j][index], qi)
        return pol
    m = ternary_matrix(inv_density) if words is None else matrix_from_words(*words)
    st = {"buf": src.read(N)}  # :175-183

    def refill():
        st["buf"] = src.read(N)
        tr.refills += 1

    def kysampling(pointer, byte_pointer):  # :266-336
        d = col = 0
        cols = 0
        while True:
            i = pointer
            while i < 8:  # :277
                d = (d << 1) + 1 - ((st["buf"][byte_pointer] >> i) & 1)
                if d > 1:  # :283-285: again from this bit
                    tr.restarts += 1
                    d, col = 1 - ((st["buf"][byte_pointer] >> i) & 1), 0
                if col > PRECISION - 2:
                    raise WalkOutOfColumns()
                for row in (1, 0):  # :287
                    d -= m[row][col]
                    if d == -1:
                        if i == 7:  # :294-307
                            pointer = 0
                            byte_pointer += 1
                            if byte_pointer >= N:
                                byte_pointer = 0
                                refill()
                            sign = st["buf"][byte_pointer] & 1
                            tr.sign_from_next_byte += 1
                        else:  # :309-313
                            pointer = i
                            sign = (st["buf"][byte_pointer] >> (i + 1)) & 1
                        tr.longest_walk = max(tr.longest_walk, cols + 1)
                        return row, sign, pointer + 1, byte_pointer  # :316
                col += 1  # :320
                cols += 1
                i += 1
            pointer = 0  # :324-334
            byte_pointer += 1
            if byte_pointer >= N:
                byte_pointer = 0
                refill()

    pointer = byte_pointer = 0
    for i in range(N):  # :185
        coeff, sign, pointer, byte_pointer = kysampling(pointer, byte_pointer)
        index = (coeff & (sign ^ 1)) | ((sign & coeff) << 1)
        for j, qi in enumerate(moduli):
            _store(pol, add, j, i, lut[j][index], qi)
    return pol
