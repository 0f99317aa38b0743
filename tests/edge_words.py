"""Edge words for the composed kernels: matrices whose every column holds the whole edge grid of the field, a different word in
every lane, handed to the kernels as they are -- no interpolation and no LDE in front, which would canonicalise them and would
put one value into every lane.  (Shared helper of tests/test_edge_words.py; a module, not a conftest.)

The kernels behind p2hot_gate_sums*, p2hot_quotient_polys* and p2hot_stark_quotient_polys* are pointwise in the LDE row, and
p2hot_batch_wrap_dev makes a commitment handle of any device matrix, so `wrap` turns an edge matrix into the "LDE" those calls
read.  The values then belong to no polynomial: the callers ask for the per-point values (values_out) and never for chunks.

Non-canonical words in a wrapped matrix.  include/p2hot.h, Conventions, lines 10-12: "Field elements are uint64_t ... Inputs may
be any representative < 2^64; every value written to an output buffer is canonical".  The comment on p2hot_batch_wrap_dev
(lines 366-367) names the outputs of p2hot_commit_dev as the usual source of the buffers and adds no requirement of its own, and
csrc/gl.hpp states the same rule for the device code ("any u64 is a valid representative").  So a wrapped matrix may hold
words of [P, 2^64) and the tests run BOTH modes: canonical=True draws from CANON, canonical=False from all of GRID.

The references take the rows through vanishing_ref.Leaves (which reduces every word % P on entry) and vanishing_ref's row
helpers: point i of the quotient coset is committed row bitrev(i * step), its "next" row the one of i + 2^qbits."""
import ctypes as C

import numpy as np

from tests import test_exec_fixups as tx
from tests import vanishing_ref as vr
from tests.conftest import P

E32 = 2**32
# the reference's grid (field/src/prime_field_testing.rs:8-17) as tests/test_exec_fixups.py::operands restates it
GRID24 = [0, 1, 2, 3, E32 - 2, E32 - 1, E32, E32 + 1, 2**63 - 1, 2**63, 2**63 + 1, P - E32, P - 2, P - 1, P, P + 1,
          P + E32 - 2, 2**64 - E32, 2**64 - 2, 2**64 - 1, 0xFFFFFFFF_00000000, 0x00000000_FFFFFFFF,
          0xFFFFFFFE_FFFFFFFF, 0x80000000_80000000]
# the operands that force the carry / borrow flags of the multiply streams (both flag values each), and the lone borrow
FLAG_FORCING = [v for pair in list(tx.CASES.values()) + [tx.LONE_BORROW] for v in pair]
GRID = list(dict.fromkeys(GRID24 + FLAG_FORCING))
CANON = [v for v in GRID if v < P]
assert GRID24 == tx.operands()[0][192:192 + 24 * 24:24]      # (operands(): 192 constructed lanes, then every grid word 24 times)
# (the grid names P - 1 three times and P - 2, 2^32 - 1 and 2^64 - 1 twice: 19 different words)
assert P - 1 == 2**64 - E32 == 0xFFFFFFFF_00000000 and P - 2 == 0xFFFFFFFE_FFFFFFFF and P + E32 - 2 == 2**64 - 1
assert len(set(GRID24)) == 19 and set(GRID24) <= set(GRID) and len(GRID) == 23 and len(CANON) == 19
assert {2**48, 0xFFFF * 2**48, 2**40, 2**57 + 2**24} <= set(CANON) and set(GRID) - set(CANON) == {P, P + 1, 2**64 - 2, 2**64 - 1}


def grid(canonical):
    return CANON if canonical else GRID


def edge_matrix(rng, cols, rows, canonical):
    """[cols][rows] uint64: every word of the grid at least once in every column, at most a quarter of the words uniformly random
    (of [0, P) or of [0, 2^64)), the rest further grid words; consecutive rows of a column differ, and the columns are shuffled
    independently, so neighbouring lanes and the operands that meet in one lane take different paths"""
    g = grid(canonical)
    assert rows >= len(g), "every grid value must fit into a column: %d rows, %d values" % (rows, len(g))
    n_rand = min(rows // 4, rows - len(g))
    out = np.zeros((cols, rows), dtype=np.uint64)
    for c in range(cols):
        more = [g[int(k)] for k in rng.integers(0, len(g), rows - len(g) - n_rand)]
        rand = [int(v) for v in rng.integers(0, P if canonical else 2**64, n_rand, dtype=np.uint64)]
        col = np.array(g + more + rand, dtype=np.uint64)
        rng.shuffle(col)
        for _ in range(100 * rows):      # a word equal to the one above it changes places with one that fits both places
            same = np.flatnonzero(col[1:] == col[:-1])
            if not len(same):
                break
            i, j = int(same[0]) + 1, int(rng.integers(0, rows))
            around = lambda k, v: all(col[t] != v for t in (k - 1, k + 1) if 0 <= t < rows and t not in (i, j))
            if abs(i - j) > 1 and around(i, col[j]) and around(j, col[i]):
                col[i], col[j] = col[j], col[i]
        assert (col[1:] != col[:-1]).all()
        assert set(g) <= set(int(v) for v in col)
        out[c] = col
    assert bool((out < np.uint64(P)).all()) == canonical
    return out


def meet(matrix, cols, value, ok=lambda row: True):
    """make `value` stand in one row of all of `cols` (in place): in a row where cols[0] has it and ok(row) holds, the other
    columns exchange that row's word with their own `value`.  Every column keeps its words, and neighbouring rows still differ.
    Returns the row."""
    value = np.uint64(value)
    for r in (int(r) for r in np.flatnonzero(matrix[cols[0]] == value) if ok(int(r))):
        trial = matrix.copy()
        for c in cols[1:]:
            s = int(np.flatnonzero(trial[c] == value)[0])
            trial[c][r], trial[c][s] = trial[c][s], trial[c][r]
        if all((trial[c][1:] != trial[c][:-1]).all() for c in cols):
            matrix[...] = trial
            return r
    raise AssertionError("no row in which the columns can meet")


def place(matrix, col, row, value):
    """bring the column's own `value` into `row` (in place, by exchanging two of its words); neighbouring rows must still differ"""
    s = int(np.flatnonzero(matrix[col] == np.uint64(value))[0])
    matrix[col][row], matrix[col][s] = matrix[col][s], matrix[col][row]
    assert (matrix[col][1:] != matrix[col][:-1]).all(), "choose another row or seed"


class Wrapped:
    """a p2hot_batch over caller-owned device buffers (p2hot_batch_wrap_dev); quacks like fri.oracle.PolynomialBatch where the
    marshalling helpers of plonky2_amd.plonk / .stark / .fri read one (_h, _W, _coeffs, degree_log, rate_bits, engine)"""

    def __init__(self, eng, h, lde, coeffs, digests, log_n, rate_bits, cap_height):
        self.engine, self._h, self.lde, self._coeffs, self._digests = eng, h, lde, coeffs, digests
        self._W, self.degree_log, self.rate_bits, self.cap_height, self.salt_size = lde.shape[0], log_n, rate_bits, cap_height, 0

    def __del__(self):
        try:
            if self._h and getattr(self.engine, "_ctx", None):
                self.engine.lib.p2hot_batch_free(self._h)
        except Exception:
            pass
        self._h = None


def _same_names_as_polynomial_batch():
    """the attributes Wrapped stands in with are PolynomialBatch's own: a rename there fails HERE, by name, and not somewhere in a
    marshalling helper"""
    import inspect
    from plonky2_amd.fri.oracle import PolynomialBatch
    init = inspect.getsource(PolynomialBatch.__init__)
    for name in ("engine", "lde", "_coeffs", "_W", "degree_log", "rate_bits", "cap_height", "salt_size"):
        assert "self.%s = " % name in init, "PolynomialBatch no longer sets .%s: tests/edge_words.py Wrapped mirrors it" % name
    assert isinstance(PolynomialBatch._h, property), "PolynomialBatch._h is no property any more: tests/edge_words.py Wrapped mirrors it"


def wrap(eng, lde_words, log_n, rate_bits, cap_height=0, coeffs=None):
    """lde_words [W][n << rate_bits] in committed order -> a Wrapped handle whose LDE matrix is exactly these words.  The
    coefficients ([W][n], zero unless given: the FRI cases pass edge words there) and the digests (the full tree's array, zero)
    have the sizes the call's argument checks ask for (csrc/host_prover.hpp: both non-null for W > 0, the digests non-null
    whenever the tree has any)."""
    _same_names_as_polynomial_batch()
    lde_words = np.ascontiguousarray(lde_words, dtype=np.uint64)
    W, N = lde_words.shape
    n = 1 << log_n
    assert N == n << rate_bits and W > 0
    d_lde = eng.dev(lde_words)
    d_co = eng.mem.zeros(W, n) if coeffs is None else eng.dev(np.ascontiguousarray(coeffs, dtype=np.uint64))
    assert tuple(d_co.shape) == (W, n)
    d_dig = eng.mem.zeros(max(eng.num_digests(log_n + rate_bits, cap_height), 1), 4)
    h = C.c_void_p()
    eng.check(eng.lib.p2hot_batch_wrap_dev(eng.ctx, eng.ptr(d_co), eng.ptr(d_lde), eng.ptr(d_dig), W, log_n, rate_bits, cap_height, C.byref(h)))
    return Wrapped(eng, h, d_lde, d_co, d_dig, log_n, rate_bits, cap_height)


def leaves(lde_words, log_n, rate_bits):
    """the reference's view of a wrapped matrix: vanishing_ref.Leaves over its transpose (row L = committed row L, reduced % P)"""
    return vr.Leaves(np.ascontiguousarray(np.asarray(lde_words, dtype=np.uint64).T), log_n, rate_bits)


def point_rows(i, log_n, rate_bits, qbits):
    """(committed row of point i, committed row of its "next" point): vanishing_ref.quotient_rows + get_lde_values' bit reversal"""
    (li, step), (ni, _) = vr.quotient_rows(i, log_n, rate_bits, qbits)
    bits = log_n + rate_bits
    return vr.bitrev(li * step, bits), vr.bitrev(ni * step, bits)


def u64p(keep, v):
    a = np.ascontiguousarray(np.asarray(v, dtype=np.uint64))
    keep.append(a)
    return a.ctypes.data_as(C.c_void_p)
