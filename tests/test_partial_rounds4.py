"""The partial rounds four to a dense pass (poseidon.hpp partial_rounds4) and the wide row fold (gl_mul3.hpp fold3w / fold1w).

Restated here with Python integers from the reference constants (oracle/poseidon_constants.h):
  * bounds: every row of every pass the permutation runs fits its two 32x32+64 chains, and a fifth application would not;
  * algebra: the kernel's schedule (first pass = round 3's MDS + partial rounds 4..6, four batches of four, a tail batch of three
    carrying round 26's constant vector), chains on 32-bit halves and all, equals the plain 30-round permutation on the reference
    KATs and on random and edge states, with every accumulator checked against its fold's precondition;
  * the wide fold: the Python mirror of its instruction stream and the shipped stream itself (through the emulator's instruction
    interpreter, and on the MI355X with -m gpu) on an edge grid of accumulators up to 2^64 - 1.
"""
import numpy as np
import pytest

from tests import pyref
from tests.conftest import P
from tests.test_asm_streams import emu_asm, tier  # noqa: F401  (fixtures: the emulator with its instruction interpreter on)

W = 12
MASK = 2**64 - 1
E32 = 2**32
RC, CIRC, DIAG = pyref.RC, pyref.CIRC, pyref.DIAG
M = [[CIRC[(c - r) % W] + (DIAG[r] if r == c else 0) for c in range(W)] for r in range(W)]
MD = [[0 if c == 0 else M[r][c] for c in range(W)] for r in range(W)]


def mat_mul(a, b):
    return [[sum(a[r][k] * b[k][c] for k in range(W)) for c in range(W)] for r in range(W)]


# PW[k] = (MD)^k M: the matrix a pass of k + 1 applications multiplies the state by
PW = [M]
for _ in range(5):
    PW.append(mat_mul(MD, PW[-1]))


def col0(a):
    return [a[r][0] for r in range(W)]


def pass_rows(k):
    """coefficient rows of the dense pass over k + 1 applications: (MD)^k M, then the column-0 terms of the in-batch S-box outputs
    s1 .. sk, which multiply (MD)^(k-1) M e0, .., M e0"""
    return [PW[k][r] + [PW[k - j][r][0] for j in range(1, k + 1)] for r in range(W)]


def pushed_constants():
    """tools/gen_poseidon_constants.py pushed_constants: rounds 4..25 add one scalar to word 0, round 26 the pushed remainder"""
    fused = [RC[W * r:W * (r + 1)] for r in range(30)]
    cur = fused[4][:]
    for r in range(4, 26):
        passive = [0] + cur[1:]
        fused[r] = [cur[0]] + [0] * (W - 1)
        nxt = [sum(M[i][j] * passive[j] for j in range(W)) % P for i in range(W)]
        cur = [(a + b) % P for a, b in zip(RC[W * (r + 1):W * (r + 2)], nxt)]
    fused[26] = cur
    return fused


PUSHED = pushed_constants()


# ---------------------------------------------------------------- the row folds, mirrored from their instruction streams
def fold_narrow(al, ah):
    """gl::fold3 / fold1: al, ah < 2^63 (the first multiply-add must not carry)"""
    assert 0 <= al < 2**63 and 0 <= ah < 2**63, (al, ah)
    t = (ah >> 32) * 0xFFFFFFFF + al
    assert t < 2**64
    t2 = t + ((ah & 0xFFFFFFFF) << 32)
    c = t2 >> 64
    r = (t2 & MASK) + (0xFFFFFFFF if c else 0)
    assert r < 2**64
    return r


def fold_wide(al, ah):
    """gl::fold3w / fold1w (and fold_row_wide_c): any al, ah < 2^64; both carries absorbed, result below 2^64"""
    assert 0 <= al < 2**64 and 0 <= ah < 2**64, (al, ah)
    t = (ah >> 32) * 0xFFFFFFFF + al  # 1: multiply-add, carry c1
    c1, t = t >> 64, t & MASK
    t += 0xFFFFFFFF if c1 else 0  # 2-3: cndmask, multiply-add (no carry)
    assert t < 2**64
    u = t + ((ah & 0xFFFFFFFF) << 32)  # 4: high-word add, carry c2
    c2, u = u >> 64, u & MASK
    u += 0xFFFFFFFF if c2 else 0  # 5-6: cndmask, multiply-add (no carry)
    assert u < 2**64
    return u


# ---------------------------------------------------------------- bounds
def row_fits(coef_sum, const=True):
    """a chain sums 32-bit halves times the coefficients (+ one constant half): its largest value"""
    return coef_sum * (E32 - 1) + (E32 - 1 if const else 0)


def test_pass_rows_fit_their_chains():
    # single rows (narrow fold): y1[0], y2[0], y3[0] of a batch of four (the same rows serve the batch of three)
    for k in range(3):
        row = pass_rows(k)[0]
        assert all(e < E32 for e in row)
        assert row_fits(sum(row)) < 2**63, k
    # the tail batch of three: narrow fold on every row, with a constant half in every row (round 26's vector)
    for row in pass_rows(2):
        assert all(e < E32 for e in row)
        assert row_fits(sum(row)) < 2**63
    # the passes of four: wide fold; every row over 2^63 (the narrow fold would be wrong) and below 2^64
    sums = [sum(row) for row in pass_rows(3)]
    for row, s in zip(pass_rows(3), sums):
        assert all(e < E32 for e in row)
        assert 2**63 < row_fits(s) < 2**64
    assert max(sums) == 3535450306  # 2^31.72, row 8
    assert sums.index(max(sums)) == 8
    # five applications would not fit, in any row
    for row in pass_rows(4):
        assert row_fits(sum(row), const=False) >= 2**64


# ---------------------------------------------------------------- the schedule
def halves(x):
    return x & 0xFFFFFFFF, x >> 32


def rep(rng, v):
    """a 64-bit representative of v the way the kernel may hold it: canonical or v + P"""
    return v + P if rng is not None and v + P < 2**64 and rng.integers(0, 2) else v


def chain_row(coefs, words, const):
    """a row as the kernel computes it: two multiply-add chains over the 32-bit halves of the words, the constant's halves as
    starting addends"""
    cl, ch = halves(const)
    al = cl + sum(c * halves(w)[0] for c, w in zip(coefs, words))
    ah = ch + sum(c * halves(w)[1] for c, w in zip(coefs, words))
    return al, ah


def sbox(rng, x):
    return rep(rng, pow(x % P, 7, P))


def mds_full(rng, s, cv):
    return [rep(rng, (sum(M[r][c] * s[c] for c in range(W)) + (cv[r] if cv else 0)) % P) for r in range(W)]


def batch(rng, s, k, first, consts, cv):
    """k + 1 applications of M in one pass: consts = the scalars of the batch's second .. last round, cv = the vector fused into
    the pass's rows (the next pass's first scalar in row 0, or round 26's vector)"""
    z = list(s)
    if not first:
        z[0] = sbox(rng, z[0])
    ss = []
    for j in range(k):  # the single rows y1[0] .. yk[0] and their S-boxes
        row = PW[j][0] + [PW[j - 1 - i][0][0] for i in range(j)]
        al, ah = chain_row(row, z + ss, consts[j])
        ss.append(sbox(rng, fold_narrow(al, ah)))
    fold = fold_wide if k == 3 else fold_narrow
    out = []
    for r, row in enumerate(pass_rows(k)):
        al, ah = chain_row(row, z + ss, cv[r])
        out.append(fold(al, ah))
    return out


def permute_scheduled(state, rng=None):
    s = [rep(rng, (x + c) % P) for x, c in zip(state, RC[:W])]
    for r in range(3):
        s = mds_full(rng, [sbox(rng, x) for x in s], RC[W * (r + 1):W * (r + 2)])
    s = [sbox(rng, x) for x in s]
    scal = [PUSHED[r][0] for r in range(26)]
    e0 = lambda c: [c] + [0] * (W - 1)  # noqa: E731
    s = batch(rng, s, 3, True, scal[4:7], e0(scal[7]))
    for r in (7, 11, 15, 19):
        s = batch(rng, s, 3, False, scal[r + 1:r + 4], e0(scal[r + 4]))
    s = batch(rng, s, 2, False, scal[24:26], PUSHED[26])
    for r in range(26, 29):
        s = mds_full(rng, [sbox(rng, x) for x in s], RC[W * (r + 1):W * (r + 2)])
    s = mds_full(rng, [sbox(rng, x) for x in s], None)
    return [x % P for x in s]


def test_schedule_covers_the_partial_rounds():
    # first pass (round 3's MDS + rounds 4..6) + four batches of four (7..22) + a batch of three (23..25): 1 + 22 applications
    assert 4 + 4 * 4 + 3 == 1 + 22


def test_scheduled_permutation_matches_the_reference_kats(kats):
    for k in kats["poseidon12"]:
        assert permute_scheduled(k["input"]) == [int(x) for x in k["output"]]
        assert pyref.poseidon_naive(k["input"]) == [int(x) for x in k["output"]]


def test_scheduled_permutation_on_random_and_edge_states():
    rng = np.random.default_rng(44)
    edge = [0, 1, P - 1, P, 2**64 - 1, E32 - 1, E32, P - E32, 2**63]
    states = [[e] * W for e in edge] + [[edge[(i + j) % len(edge)] for i in range(W)] for j in range(len(edge))]
    states += [[int(v) for v in rng.integers(0, 2**64, W, dtype=np.uint64)] for _ in range(24)]
    for st in states:
        want = pyref.poseidon_naive(st)
        assert permute_scheduled(st) == want
        assert permute_scheduled(st, rng) == want  # intermediate words as non-canonical representatives where they fit


# ---------------------------------------------------------------- the wide fold
def wide_fold_grid():
    half = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF]
    vals = {0, 1, 2**63 - 1, 2**63, 2**63 + 1, 2**64 - 1, 2**64 - 2, P - 1, P, E32 - 1, E32, 2**64 - E32}
    vals |= {(h << 32) | l for h in half for l in half}
    vals |= {row_fits(sum(row)) for row in pass_rows(3)}  # the exact per-row maxima of the passes of four
    vals |= {row_fits(sum(row)) - 1 for row in pass_rows(3)}
    vals = sorted(vals)
    al = [a for a in vals for _ in vals]
    ah = [b for _ in vals for b in vals]
    return al, ah


def test_wide_fold_model_on_the_edge_grid():
    al, ah = wide_fold_grid()
    carries = set()
    for a, h in zip(al, ah):
        assert fold_wide(a, h) % P == (a + h * E32) % P
        t = (h >> 32) * 0xFFFFFFFF + a
        carries.add((t >> 64, ((t & MASK) + (0xFFFFFFFF if t >> 64 else 0) + ((h & 0xFFFFFFFF) << 32)) >> 64))
    assert carries == {(0, 0), (0, 1), (1, 0), (1, 1)}  # the grid forces each carry alone and both together


def _run_selftest(eng, al, ah):
    n = len(al)
    da, db = eng.dev(np.array(al, dtype=np.uint64)), eng.dev(np.array(ah, dtype=np.uint64))
    out = eng.mem.zeros(6, n)
    eng.check(eng.lib.p2hot_field_selftest_dev(eng.ctx, eng.ptr(da), eng.ptr(db), n, eng.ptr(out)))
    return eng.host(out)


def test_wide_fold_streams_through_the_asm(emu_asm):  # noqa: F811
    """gl::fold3w / fold1w as shipped, decoded and executed by the instruction interpreter (flag 1024 of the field self-test)"""
    al, ah = wide_fold_grid()
    o = _run_selftest(emu_asm, al, ah)
    assert (o[5] & 1024 == 0).all()
    assert (o[5] == 0).all()


@pytest.mark.gpu
def test_wide_fold_streams_on_the_gpu(gpu):
    al, ah = wide_fold_grid()
    rng = np.random.default_rng(9)
    al += [int(v) for v in rng.integers(0, 2**64, 4096, dtype=np.uint64)]
    ah += [int(v) for v in rng.integers(0, 2**64, 4096, dtype=np.uint64)]
    o = _run_selftest(gpu, al, ah)
    assert (o[5] == 0).all()
