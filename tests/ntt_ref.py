"""A plain restatement of the transforms the NTT passes compute, independent of oracle/p2oracle.c and of the library.

Roots come from pyref.W32 (goldilocks_field.rs:87), the coset shift from pyref.G.  The transforms are radix-2 over numpy object
arrays of Python integers (field/src/fft.rs semantics: natural order in and out); where even that is too slow (2^17 and up) the
closed forms below give single output positions: an impulse's transform is a power of the root, and any output is one polynomial
evaluation, done by an exact vectorised Goldilocks multiply on uint64 arrays (`mul`, self-tested against Python integers).
"""
import numpy as np

from tests import pyref

P = pyref.P
G = pyref.G
_P64 = np.uint64(P)
_M32 = np.uint64(0xFFFFFFFF)
_EPS = np.uint64(0xFFFFFFFF)  # 2^64 mod P


def root(log_n, inverse=False):
    w = pyref.root_of_unity(log_n)
    return pow(w, P - 2, P) if inverse else w


# ---------------------------------------------------------------- radix-2 transforms on Python integers
def _obj(a):
    return np.array([int(x) % P for x in a], dtype=object)


def fft(coeffs, inverse=False):
    """out[i] = sum_t c[t] w^(+-i t) (fft.rs:215-249 fft / evaluate); inverse=True is fft.rs:68-91 ifft (the 1/n included).
    Any 64-bit representatives in, canonical Python integers out."""
    a = _obj(coeffs)
    n = len(a)
    log_n = n.bit_length() - 1
    assert n == 1 << log_n
    a = a[[pyref.bitrev(i, log_n) for i in range(n)]]  # decimation in time: bit-reversed in, natural out
    for s in range(1, log_n + 1):
        h = 1 << (s - 1)
        wm = root(s, inverse)
        tw = np.empty(h, dtype=object)
        t = 1
        for j in range(h):
            tw[j] = t
            t = t * wm % P
        blk = a.reshape(-1, 2, h)
        u = blk[:, 0, :]
        v = blk[:, 1, :] * tw % P
        a = np.stack([(u + v) % P, (u - v) % P], axis=1).reshape(-1)
    if inverse:
        ninv = pow(n, P - 2, P)
        a = a * ninv % P
    return [int(x) for x in a]


def ifft(values):
    return fft(values, inverse=True)


def coset_ifft(values, shift):
    """PolynomialValues::coset_ifft (polynomial/mod.rs:63-73): the coefficients of p with p(shift * w^i) = values[i]"""
    c = ifft(values)
    si = pow(shift, P - 2, P)
    out, s = [], 1
    for x in c:
        out.append(x * s % P)
        s = s * si % P
    return out


def coset_lde_rows(coeffs, rate_bits, shift, row_begin=0, row_count=None):
    """Rows [row_begin, row_begin + row_count) of the coset LDE in the engine's (committed) order: row L holds
    p(shift * w_N^bitrev(L, log N)) (pyref.naive_coset_lde_rows).  Row block b (n rows) is the coset s_b = shift * w_N^bitrev(b):
    its rows are the bit-reversed transform of c[t] * s_b^t, one n-point fft per block."""
    n = len(coeffs)
    log_n = n.bit_length() - 1
    N = n << rate_bits
    if row_count is None:
        row_count = N - row_begin
    assert row_begin % n == 0 and row_count % n == 0 and row_begin + row_count <= N
    wN = pyref.root_of_unity(log_n + rate_bits)
    c = [int(x) % P for x in coeffs]
    rows = []
    for b in range(row_begin // n, (row_begin + row_count) // n):
        sb = shift * pow(wN, pyref.bitrev(b, rate_bits), P) % P
        scaled, s = [], 1
        for x in c:
            scaled.append(x * s % P)
            s = s * sb % P
        f = fft(scaled)
        rows += [f[pyref.bitrev(r, log_n)] for r in range(n)]
    return rows


# ---------------------------------------------------------------- exact Goldilocks arithmetic on uint64 arrays
def mul(a, b):
    """a * b mod P elementwise, canonical; a, b any uint64 representatives (arrays or scalars)"""
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    with np.errstate(over="ignore"):
        a0, a1 = a & _M32, a >> np.uint64(32)
        b0, b1 = b & _M32, b >> np.uint64(32)
        p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
        mid = p01 + p10
        cmid = (mid < p01).astype(np.uint64)  # carry out of the middle sum: worth 2^96
        lo = p00 + (mid << np.uint64(32))
        clo = (lo < p00).astype(np.uint64)
        hi = p11 + (mid >> np.uint64(32)) + (cmid << np.uint64(32)) + clo
        # lo + hi * 2^64 with 2^64 = 2^32 - 1 and 2^96 = -1 (mod P)
        hh, hl = hi >> np.uint64(32), hi & _M32
        t0 = lo - hh
        t0 = np.where(lo < hh, t0 - _EPS, t0)  # borrow: the wrap added 2^64 = 2^32 - 1 (mod P); take it back
        t1 = hl * _EPS
        r = t0 + t1
        r = np.where(r < t1, r + _EPS, r)      # carry: 2^64 = 2^32 - 1
        return np.where(r >= _P64, r - _P64, r)


def add(a, b):
    """a + b mod P elementwise, canonical; a, b canonical uint64"""
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    with np.errstate(over="ignore"):
        r = a + b
        r = np.where(r < a, r + _EPS, r)  # carry: 2^64 = 2^32 - 1
    return reduce(r)


def reduce(a):
    a = np.asarray(a, dtype=np.uint64)
    return np.where(a >= _P64, a - _P64, a)


def sum_mod(a):
    """sum of uint64 field elements mod P, exact: the 32-bit halves are summed apart (below 2^64 for fewer than 2^32 terms)"""
    a = np.asarray(a, dtype=np.uint64).reshape(-1)
    assert a.size < 2**32
    lo = int((a & _M32).sum(dtype=np.uint64))
    hi = int((a >> np.uint64(32)).sum(dtype=np.uint64))
    return (lo + (hi << 32)) % P


def powers(x, count):
    """[x^0, .., x^(count - 1)] mod P as uint64, through a two-level table (count a power of two)"""
    log_c = max(count - 1, 0).bit_length()
    lo_bits = (log_c + 1) // 2
    n_lo, n_hi = 1 << lo_bits, 1 << (log_c - lo_bits)
    t_lo = np.array([pow(x, i, P) for i in range(n_lo)], dtype=np.uint64)
    step = pow(x, n_lo, P)
    t_hi = np.array([pow(step, i, P) for i in range(n_hi)], dtype=np.uint64)
    return mul(t_hi[:, None], t_lo[None, :]).reshape(-1)[:count]


def eval_poly(coeffs, x):
    """sum_t c[t] x^t mod P for a uint64 coefficient array (any representatives)"""
    c = np.asarray(coeffs, dtype=np.uint64)
    return sum_mod(mul(reduce(c), powers(x % P, len(c))))


def fft_at(coeffs, i, inverse=False):
    """output i of fft (inverse=True: of ifft) of the uint64 array `coeffs`: one polynomial evaluation"""
    n = len(coeffs)
    log_n = n.bit_length() - 1
    v = eval_poly(coeffs, pow(root(log_n, inverse), i, P))
    return v * pow(n, P - 2, P) % P if inverse else v


def lde_row_at(coeffs, rate_bits, shift, row):
    """row `row` of the coset LDE in the engine's order (coset_lde_rows), by one evaluation"""
    n = len(coeffs)
    lg = n.bit_length() - 1 + rate_bits
    return eval_poly(coeffs, shift * pow(pyref.root_of_unity(lg), pyref.bitrev(row, lg), P) % P)


def impulse_fft(log_n, k, inverse=False):
    """fft (inverse=True: ifft) of the impulse delta_k of length 2^log_n: output i is w^(+-i k) (times 1/n for ifft), as uint64"""
    n = 1 << log_n
    w = root(log_n, inverse)
    e = (np.arange(n, dtype=np.uint64) * np.uint64(k)) & np.uint64(n - 1)  # i * k mod n (n <= 2^32: no overflow below 2^64)
    lo_bits = (log_n + 1) // 2
    t_lo = np.array([pow(w, i, P) for i in range(1 << lo_bits)], dtype=np.uint64)
    t_hi = np.array([pow(w, i << lo_bits, P) for i in range(1 << (log_n - lo_bits))], dtype=np.uint64)
    out = mul(t_lo[e & np.uint64((1 << lo_bits) - 1)], t_hi[e >> np.uint64(lo_bits)])
    return mul(out, np.uint64(pow(n, P - 2, P))) if inverse else out


def alternating_fft(log_n, a, b, inverse=False):
    """fft (inverse=True: ifft) of [a, b, a, b, ...] (a == b: a constant vector): the sum over even and odd positions leaves
    n/2 (a + b) at 0 and n/2 (a - b) at n/2 (w^(n/2) = -1), zero elsewhere; ifft divides by n.  Length 1: [a]."""
    n = 1 << log_n
    out = np.zeros(n, dtype=np.uint64)
    if n == 1:
        out[0] = a % P
        return out
    scale = pow(2, P - 2, P) if inverse else n // 2
    out[0] = (a + b) * scale % P
    out[n // 2] = (a - b) * scale % P
    return out


def is_geometric(got, first, ratio):
    """got[0] == first and got[i + 1] == got[i] * ratio for every i: got[i] = first * ratio^i, checked in one multiply pass"""
    got = np.asarray(got, dtype=np.uint64)
    return int(got[0]) == first % P and bool((mul(got[:-1], np.uint64(ratio % P)) == got[1:]).all())
