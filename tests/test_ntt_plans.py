"""Every NTT pass plan and kernel variant against a plain transform (tests/ntt_ref.py), not only against the oracle.

plan_ntt (p2hot.hip) picks every pass's kernel from the size and the context's knobs, run_dif launches them:
  * plan_passes(log_n, P2HOT_NTT_STRIDED_BITS): strided passes of log_r bits, then the 12-bit contiguous pass;
  * limb_supported (Pass::kernel): strided log_r 4..10 and the contiguous pass run nttl::ntt_limbpass_kernel (one instantiation per log_r), strided
    log_r 1..3 and 11 the word-based ntt_regpass_kernel; above 2^24 the first pass has no inter-pass table and runs the word kernel;
  * NttPlan::limb_all (every pass a limb pass, log_n <= 24) moves the inverse's 1/n from the first pass (SCALE_CONST) to the last (LAST_CONST);
  * the coset LDE's first pass scales by a table (LAST_TILE when strided, LAST_UNIT when contiguous), may read a bit-reversed source
    (from_values, NttPlan::lde_reads_bitrev, P2HOT_LDE_BITREV_SRC) and loops over the cosets in one workgroup (zloop, P2HOT_NTT_ZLOOP_MIN);
  * the contiguous limb pass stages its tables once for 2^tiles_log tiles (P2HOT_LIMB_TILES_LOG) when >= 4096 workgroups remain;
  * P2HOT_NTT_XCD_REMAP, P2HOT_NTT_LIMB and p2hot_tune_ntt modes 0 / 4 / 8 / 3.
Each knob variant runs on a context of its own (environment set, engine made, environment restored).  Inputs stress the limb
arithmetic: non-canonical random words, boundary words, constant P - 1 and 2^64 - 1, alternating 2^64 - 1 / 0, and impulses on
both sides of every pass boundary (each pins one pass's twiddle index).  The CPU tier runs the emulator up to 2^22; the MI355X
(-m gpu) runs every plan up to 2^25.  The last section restates the limb unit's bounds (nttl.hpp split, bias, dft_limbs).
"""
import os
import re

import numpy as np
import pytest

from tests import ntt_ref, pyref
from tests.conftest import P, ROOT, rand_field

U64 = np.uint64
EDGE = np.array([0, 1, 2**32 - 1, 2**32, 2**32 + 1, P - 1, P, P + 1, 2**63, 2**64 - 2**32, 2**64 - 1], dtype=np.uint64)
SHIFT = pow(pyref.G, 4, P)   # a FRI round's coset shift (shift^arity), not the default one
STRIDED_BITS = (10, 6, 7, 11)  # the default and the knob's extremes / odd values


def is_gpu(eng):
    return not eng.lib.p2hot_is_emulated()


_VARIANTS = {}


def variant(eng, **env):
    """an engine of the same backend whose context was created under P2HOT_<name>=value (cached per backend and setting)"""
    if not env:
        return eng
    env = {"P2HOT_" + k: str(v) for k, v in env.items()}
    key = (is_gpu(eng), tuple(sorted(env.items())))
    if key not in _VARIANTS:
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            if is_gpu(eng):
                from plonky2_amd import Engine
                _VARIANTS[key] = Engine(0)
            else:
                from tests.emu_backend import emu_engine
                _VARIANTS[key] = emu_engine()
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k)
                else:
                    os.environ[k] = v
    return _VARIANTS[key]


def plan(log_n, strided_bits=10):
    """p2hot.hip plan_passes: the strided passes' log_r, as even as possible, largest first, then the 12-bit contiguous pass"""
    if log_n <= 12:
        return [log_n]
    rem = log_n - 12
    k = -(-rem // strided_bits)
    out = []
    for i in range(k):
        part = -(-rem // (k - i))
        out.append(part)
        rem -= part
    return out + [12]


def kernels(log_n, strided_bits=10):
    """which kernel plan_ntt gives each pass (Pass::kernel, default knobs): 'limb' or 'word'"""
    out, nblk = [], log_n
    for i, r in enumerate(plan(log_n, strided_bits)):
        strided = i + 1 < len(plan(log_n, strided_bits))
        ok = (4 <= r <= 10 and nblk <= 24) if strided else (r == 12)
        out.append("limb" if ok else "word")
        nblk -= r
    return out


def distinct_plans(log_n, bits=STRIDED_BITS):
    """{strided bits: plan} keeping the first knob value of every distinct plan"""
    seen, out = set(), {}
    for b in bits:
        p = tuple(plan(log_n, b))
        if p not in seen:
            seen.add(p)
            out[b] = p
    return out


def boundary_impulses(log_n, widths):
    """k = 0, 1, n - 1 and 2^s - 1, 2^s for every cumulative pass width s, counted from either end of the index"""
    n = 1 << log_n
    ks = {0, 1, n - 1}
    s = 0
    for w in widths[:-1]:
        s += w
        for e in (s, log_n - s):
            if 0 < e < log_n:
                ks |= {(1 << e) - 1, 1 << e}
    return sorted(k for k in ks if k < n)


def stress_rows(log_n, full=True):
    """(label, row): random non-canonical words, boundary words, constant P - 1 and 2^64 - 1, alternating 2^64 - 1 / 0"""
    n = 1 << log_n
    rng = np.random.default_rng(1000 + log_n)
    rows = [("random", rand_field(rng, n, noncanonical=True))]
    if full:
        rows.append(("edges", EDGE[rng.integers(0, len(EDGE), n)]))
        rows.append(("const:p-1", np.full(n, P - 1, dtype=U64)))
        rows.append(("const:max", np.full(n, 2**64 - 1, dtype=U64)))
        rows.append(("alt:max/0", np.resize(np.array([2**64 - 1, 0], dtype=U64), n)))
    return rows


def impulse_rows(log_n, ks):
    n = 1 << log_n
    out = []
    for k in ks:
        r = np.zeros(n, dtype=U64)
        r[k] = 1
        out.append(("imp:%d" % k, r))
    return out


PROFILE_NAME = {"fft": "ntt_fwd", "ifft": "ntt_intt", "coset_ifft": "ntt_intt"}


def run(e, kind, rows, log_n):
    """one batched launch sequence of `kind` on the rows; returns (outputs, profile)"""
    a = np.ascontiguousarray(np.stack(rows))
    d = e.dev(a.copy())
    e.profile(True)
    e.profile_results(reset=True)
    if kind == "fft":
        e.fft(d, log_n)
    elif kind == "ifft":
        e.ifft(d, log_n)
    else:
        e.check(e.lib.p2hot_coset_ifft_dev(e.ctx, e.ptr(d), a.shape[0], a.shape[1], log_n, SHIFT))
    out = e.host(d)
    prof = e.profile_results(reset=True)
    e.profile(False)
    return out, prof


def launches(prof, name):
    return prof.get(name, {}).get("launches", 0)


_EXPECT = {}


def expected(kind, log_n, label, row, ora):
    """the exact output of `kind` on `row`, or None where only sampled / closed-form checks are affordable (2^23 and up).
    ntt_ref in full up to 2^16, the oracle above (pinned to ntt_ref by sampled positions in check_row)"""
    key = (kind, log_n, label)
    if key in _EXPECT:
        return _EXPECT[key]
    n = 1 << log_n
    inv = kind != "fft"
    ex = None
    if label.startswith("imp:") and log_n <= 16:
        ex = ntt_ref.impulse_fft(log_n, int(label[4:]), inverse=inv)
    elif label.startswith("imps:") and log_n <= 16:
        ex = np.zeros(n, dtype=U64)
        for j, k in enumerate(map(int, label[5:].split(","))):
            ex = ntt_ref.add(ex, ntt_ref.mul(ntt_ref.impulse_fft(log_n, k, inverse=inv), U64(2**64 - 1 - j)))
    elif label.startswith(("const:", "alt:")):
        a, b = int(row[0]), int(row[1 % n])
        ex = ntt_ref.alternating_fft(log_n, a, b, inverse=inv)
    elif label.startswith("imp:"):
        ex = None  # geometric check
    elif log_n <= 16:
        ex = np.array((ntt_ref.fft(row) if kind == "fft" else ntt_ref.ifft(row)), dtype=U64)
    elif log_n <= 22:
        ex = ntt_ref.reduce(ora.fft(row.copy()) if kind == "fft" else ora.ifft(row.copy()))
    if ex is not None and kind == "coset_ifft":
        ex = ntt_ref.mul(ex, ntt_ref.powers(pow(SHIFT, P - 2, P), n))
    _EXPECT[key] = ex
    return ex


def check_row(kind, log_n, label, row, got, ora, tag):
    n = 1 << log_n
    ex = expected(kind, log_n, label, row, ora)
    if ex is not None:
        bad = np.nonzero(got != ex)[0]
        assert bad.size == 0, (tag, kind, label, "first mismatch at", int(bad[0]) if bad.size else None)
    if label.startswith("imp:") and ex is None:
        k = int(label[4:])
        w = ntt_ref.root(log_n, kind != "fft")
        first, ratio = 1, pow(w, k, P)
        if kind != "fft":
            first = pow(n, P - 2, P)
        if kind == "coset_ifft":
            ratio = ratio * pow(SHIFT, P - 2, P) % P
        assert ntt_ref.is_geometric(got, first, ratio), (tag, kind, label)
    if label == "random" and log_n > 16:
        # pin the oracle (or, above 2^22, the engine alone) to the plain evaluation at a position from each half
        for i in ((n - 1 - (n >> 3), 3 + (n >> 2)) if log_n <= 22 else (3 + (n >> 2),)):
            v = ntt_ref.fft_at(row, i, inverse=kind != "fft")
            if kind == "coset_ifft":
                v = v * pow(SHIFT, (P - 2) * i, P) % P
            assert int(got[i]) == v, (tag, kind, label, i)


def check_plan(e, ora, log_n, widths, rows, tag, kinds=("fft", "ifft", "coset_ifft")):
    """fft, ifft and coset_ifft of the rows in one batch each, against the references; the profile shows the planned passes"""
    n = 1 << log_n
    strided = len(widths) - 1
    for kind in kinds:
        got, prof = run(e, kind, [r for _, r in rows], log_n)
        name = PROFILE_NAME[kind]
        assert launches(prof, name + "_strided") == strided and launches(prof, name + "_contig") == 1, (tag, kind, prof)
        for (label, row), g in zip(rows, got):
            check_row(kind, log_n, label, row, g, ora, tag)
        if log_n > 22 and kind == "fft":  # no full reference: the round trip closes it
            back, _ = run(e, "ifft", list(got), log_n)
            for (label, row), b in zip(rows, back):
                assert (b == ntt_ref.reduce(row)).all(), (tag, "ifft(fft(x))", label)
    return n


# ---------------------------------------------------------------- the reference itself
def test_ntt_ref_matches_naive_evaluation():
    rng = np.random.default_rng(3)
    for log_n in range(7):
        c = [int(x) for x in rng.integers(0, 2**64, 1 << log_n, dtype=U64)]
        assert ntt_ref.fft(c) == pyref.naive_ntt([x % P for x in c]), log_n
        assert ntt_ref.ifft(ntt_ref.fft(c)) == [x % P for x in c], log_n
        assert ntt_ref.coset_ifft(pyref.naive_coset_lde_rows(c, 0) if log_n == 0 else
                                  [pyref.eval_poly(c, SHIFT * pow(pyref.root_of_unity(log_n), i, P) % P) for i in range(1 << log_n)],
                                  SHIFT) == [x % P for x in c], log_n
    for log_n, rb in ((0, 2), (2, 1), (3, 3), (4, 2)):
        c = [int(x) for x in rng.integers(0, P, 1 << log_n, dtype=U64)]
        assert ntt_ref.coset_lde_rows(c, rb, pyref.G) == pyref.naive_coset_lde_rows(c, rb), (log_n, rb)
        n = 1 << log_n
        rows = ntt_ref.coset_lde_rows(c, rb, SHIFT, row_begin=n * ((1 << rb) - 1), row_count=n)
        assert rows == ntt_ref.coset_lde_rows(c, rb, SHIFT)[-n:]
        assert rows[-1] == ntt_ref.lde_row_at(np.array(c, dtype=U64), rb, SHIFT, (n << rb) - 1)


def test_ntt_ref_vectorised_multiply_and_closed_forms():
    rng = np.random.default_rng(4)
    a = np.concatenate([EDGE.repeat(len(EDGE)), rng.integers(0, 2**64, 20000, dtype=U64)])
    b = np.concatenate([np.tile(EDGE, len(EDGE)), rng.integers(0, 2**64, 20000, dtype=U64)])
    got = ntt_ref.mul(a, b)
    assert [int(x) for x in got] == [int(x) * int(y) % P for x, y in zip(a, b)]
    ca, cb = ntt_ref.reduce(a), ntt_ref.reduce(b)
    assert [int(x) for x in ntt_ref.add(ca, cb)] == [(int(x) + int(y)) % P for x, y in zip(a, b)]
    assert ntt_ref.sum_mod(np.full(1000, 2**64 - 1, dtype=U64)) == 1000 * (2**64 - 1) % P
    x = 0x123456789ABCDEF
    assert [int(v) for v in ntt_ref.powers(x, 64)] == [pow(x, i, P) for i in range(64)]
    for log_n in (0, 1, 5, 10):
        n = 1 << log_n
        v = rng.integers(0, 2**64, n, dtype=U64)
        f = ntt_ref.fft(v)
        assert all(ntt_ref.fft_at(v, i) == f[i] for i in {0, 1, n - 1, n // 3} if i < n)
        for k in {0, n - 1, n // 2, min(1, n - 1)}:
            imp = [0] * n
            imp[k] = 1
            assert [int(y) for y in ntt_ref.impulse_fft(log_n, k)] == ntt_ref.fft(imp)
            assert [int(y) for y in ntt_ref.impulse_fft(log_n, k, True)] == ntt_ref.ifft(imp)
            assert ntt_ref.is_geometric(ntt_ref.impulse_fft(log_n, k), 1, pow(ntt_ref.root(log_n), k, P))
        for a0, b0 in ((P - 1, P - 1), (2**64 - 1, 0), (3, 2**63)):
            alt = [a0, b0] * (n // 2) if n > 1 else [a0]
            assert [int(y) for y in ntt_ref.alternating_fft(log_n, a0, b0)] == ntt_ref.fft(alt)
            assert [int(y) for y in ntt_ref.alternating_fft(log_n, a0, b0, True)] == ntt_ref.ifft(alt)
    assert not ntt_ref.is_geometric(np.array([1, 2, 4, 9], dtype=U64), 1, 2)


def test_plan_model_covers_every_pass_kind():
    """the matrix below reaches every limb instantiation (strided log_r 4..10 and the contiguous 12), the word kernel at strided
    log_r 1..3 and 11 and above 2^24, and three-pass plans below 2^23"""
    limb, word, three = set(), set(), set()
    for log_n in range(0, 26):
        for b, p in distinct_plans(log_n).items():
            for r, k in zip(p, kernels(log_n, b)):
                (limb if k == "limb" else word).add(r if log_n <= 24 or r != p[0] else ("first", log_n))
            if len(p) == 3 and log_n < 23:
                three.add(log_n)
    assert limb == {4, 5, 6, 7, 8, 9, 10, 12}
    assert {1, 2, 3, 11} <= word and ("first", 25) in word
    assert three == {19, 20, 21, 22}
    assert plan(22) == [10, 12] and plan(23) == [6, 5, 12] and plan(25, 6) == [5, 4, 4, 12] and plan(23, 11) == [11, 12]


# ---------------------------------------------------------------- pass plans x stress inputs
CPU_FULL_MAX = 19     # the CPU tier: every stress row to 2^19, impulses one per row to 2^18
CPU_IMPULSE_MAX = 18


def impulse_sum_row(log_n, ks):
    """the impulses of one plan in one row, weights 2^64 - 1 - j (the CPU tier's large sizes: one emulated row instead of many)"""
    r = np.zeros(1 << log_n, dtype=U64)
    for j, k in enumerate(ks):
        r[k] = 2**64 - 1 - j
    return ("imps:" + ",".join(map(str, ks)), r)


@pytest.mark.parametrize("log_n", list(range(0, 26)))
def test_pass_plans_against_plain_transform(eng, ora, log_n):
    """fft, ifft and coset_ifft (shift g^4) under every distinct plan of P2HOT_NTT_STRIDED_BITS in {10 (default), 6, 7, 11}, on the
    stress rows and on impulses at both sides of every pass boundary.  Both sides of the limb_all cutoff: 2^24 (1/n in the last
    pass, LAST_CONST) and 2^25 (first pass on the word kernel, SCALE_CONST).  The CPU tier runs every plan to 2^22: all stress rows
    to 2^19 (one random row above, default plan), one impulse per row to 2^18 and all of a plan's impulses in one row above, and
    coset_ifft (the inverse passes + a scale) to 2^19"""
    gpu = is_gpu(eng)
    if not gpu and log_n > 22:
        pytest.skip("2^23 and up: GPU tier (-m gpu)")
    for b, widths in distinct_plans(log_n).items():
        e = variant(eng) if b == 10 else variant(eng, NTT_STRIDED_BITS=b)
        tag = ("bits", b, "plan", widths, kernels(log_n, b))
        ks = boundary_impulses(log_n, list(widths))
        if gpu or log_n <= CPU_FULL_MAX:
            stress = stress_rows(log_n)
        else:
            stress = stress_rows(log_n, full=False) if b == 10 else []
        imps = impulse_rows(log_n, ks) if gpu or log_n <= CPU_IMPULSE_MAX else [impulse_sum_row(log_n, ks)]
        kinds = ("fft", "ifft", "coset_ifft") if gpu or log_n <= CPU_FULL_MAX else ("fft", "ifft")
        if log_n > 22:  # 2^25 words are 256 MiB a row: two batches
            check_plan(e, ora, log_n, list(widths), stress, tag, kinds)
            check_plan(e, ora, log_n, list(widths), imps, tag, kinds)
        else:
            check_plan(e, ora, log_n, list(widths), stress + imps, tag, kinds)


# ---------------------------------------------------------------- coset LDE
def lde_expected_blocks(co, log_n, rb, shift, b0, zc, ora):
    """rows [b0 n, (b0 + zc) n) per column: ntt_ref up to 2^14, above that one oracle fft per block (+ ntt_ref pins by the caller)"""
    n = 1 << log_n
    if log_n <= 14:
        return np.array([ntt_ref.coset_lde_rows(list(c), rb, shift, b0 * n, zc * n) for c in co], dtype=U64)
    rev = np.array([pyref.bitrev(i, log_n) for i in range(n)]) if log_n <= 16 else \
        _bitrev_index(log_n)
    wN = pyref.root_of_unity(log_n + rb)
    out = np.empty((len(co), zc * n), dtype=U64)
    for z in range(zc):
        sb = shift * pow(wN, pyref.bitrev(b0 + z, rb), P) % P
        pw = ntt_ref.powers(sb, n)
        for c in range(len(co)):
            out[c, z * n:(z + 1) * n] = ntt_ref.reduce(ora.fft(ntt_ref.mul(co[c], pw)))[rev]
    return out


def _bitrev_index(log_n):
    r = np.zeros(1 << log_n, dtype=np.int64)
    for b in range(log_n):
        r |= ((np.arange(1 << log_n) >> b) & 1) << (log_n - 1 - b)
    return r


def lde_cases(log_n, gpu):
    """(rate_bits, first block, blocks, W): whole-block row ranges, most of them starting past block 0"""
    if gpu or log_n <= 14:
        W = 2 if log_n < 20 else 1
        return [(rb, (1 << rb) // 2, (1 << rb) - (1 << rb) // 2 if rb < 4 else 3, W) for rb in range(5)]
    return {15: [(2, 1, 2, 2)], 16: [(1, 0, 2, 2), (4, 9, 2, 1)], 17: [(3, 5, 2, 1)], 18: [(0, 0, 1, 1)],
            19: [(2, 2, 2, 1)], 20: [(1, 1, 1, 1)], 21: [(1, 0, 2, 1)], 22: [(1, 0, 2, 2)]}[log_n]


@pytest.mark.parametrize("zloop", ["default", "1"])
@pytest.mark.parametrize("log_n", list(range(12, 23)))
def test_coset_lde_rows_against_plain_transform(eng, ora, log_n, zloop):
    """p2hot_coset_lde_dev with shift g^4 on whole-block row ranges, rate_bits 0..4: the first pass's scale table (LAST_TILE when
    strided: tile rows 2^4 .. 2^10 at 2^16 .. 2^22, LAST_UNIT when contiguous), with the cosets looped inside one workgroup
    (P2HOT_NTT_ZLOOP_MIN=1 and, at 2^22 x 2 columns x 2 blocks on the CPU tier, the default 2048) and in grid.z"""
    gpu = is_gpu(eng)
    e = variant(eng) if zloop == "default" else variant(eng, NTT_ZLOOP_MIN=zloop)
    rng = np.random.default_rng(77 + log_n)
    n = 1 << log_n
    for rb, b0, zc, W in lde_cases(log_n, gpu):
        if zloop == "1" and zc < 2:
            continue
        co = rand_field(rng, W, n, noncanonical=True)
        got = e.host(e.coset_lde(e.dev(co), log_n, rb, SHIFT, row_begin=b0 * n, row_count=zc * n))
        exp = lde_expected_blocks(co, log_n, rb, SHIFT, b0, zc, ora)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, (log_n, rb, b0, zc, W, zloop, "first mismatch (column, row)", bad[0].tolist() if bad.size else None)
        if log_n > 14:
            for r in (0, zc * n - 1 - (n >> 2)):
                assert int(got[W - 1, r]) == ntt_ref.lde_row_at(co[W - 1], rb, SHIFT, b0 * n + r), (log_n, rb, r)


@pytest.mark.parametrize("bitrev_src", ["0", "1"])
@pytest.mark.parametrize("log_n", list(range(16, 23)))
def test_from_values_lde_bit_reversed_source(eng, ora, log_n, bitrev_src):
    """from_values (fri/oracle.rs:65-69 then :91-98) at every two-pass size: with P2HOT_LDE_BITREV_SRC=1 (the default) the LDE's
    first pass reads the inverse transform's bit-reversed output (BRIN) and writes the natural coefficients; with 0 a stand-alone
    bit reversal runs.  Coefficients and LDE rows against ntt_ref's ifft / coset LDE (oracle per block above 2^14)."""
    gpu = is_gpu(eng)
    if not gpu and log_n == 21 and bitrev_src == "0":
        pytest.skip("CPU tier: 2^21 runs the bit-reversed source only")
    e = variant(eng, LDE_BITREV_SRC=bitrev_src)
    rng = np.random.default_rng(5 + log_n)
    n = 1 << log_n
    W, rb = (2, 1) if gpu or log_n <= 18 else (1, 1)
    vals = rand_field(rng, W, n, noncanonical=True)
    N = n << rb
    e.profile(True)
    e.profile_results(reset=True)
    r = e.commit(e.dev(vals), log_n, rb, N.bit_length() - 1, True)
    coeffs, lde = e.host(r["coeffs"]), e.host(r["lde"])
    prof = e.profile_results(reset=True)
    e.profile(False)
    assert ("bitrev_permute" in prof) == (bitrev_src == "0"), prof
    for c in range(W):
        assert (coeffs[c] == ntt_ref.reduce(ora.ifft(vals[c].copy()))).all(), (log_n, c)
        assert int(coeffs[c, n // 3]) == ntt_ref.fft_at(vals[c], n // 3, inverse=True)
    exp = lde_expected_blocks(coeffs, log_n, rb, pyref.G, 0, 1 << rb, ora)
    assert (lde == exp).all(), (log_n, bitrev_src)
    assert int(lde[0, N - 5]) == ntt_ref.lde_row_at(coeffs[0], rb, pyref.G, N - 5)


@pytest.mark.parametrize("log_n,bits,mode,reads_bitrev", [(13, 10, 3, False), (16, 10, 3, True), (19, 6, 3, False),
                                                          (16, 10, 0, False), (16, 10, 4, False), (16, 10, 8, False)])
def test_from_values_bit_reversal_follows_the_plan(eng, ora, log_n, bits, mode, reads_bitrev):
    """from_values skips the stand-alone bit reversal exactly when the planned LDE is two limb passes (NttPlan::lde_reads_bitrev, read by
    commit_dev_impl and run_dif alike): [1, 12] = word, limb and [4, 3, 12] = limb, word, limb run it, [4, 12] = limb, limb does not --
    unless p2hot_tune_ntt 0 / 4 / 8 switches the limb kernels off.  The smallest size of every branch; coefficients and LDE rows
    against ntt_ref / the oracle each time"""
    ks = kernels(log_n, bits) if mode == 3 else ["word"] * len(plan(log_n, bits))
    assert (ks == ["limb", "limb"]) == reads_bitrev, (plan(log_n, bits), ks)
    e = variant(eng) if bits == 10 else variant(eng, NTT_STRIDED_BITS=bits)
    rng = np.random.default_rng(50 + log_n + mode)
    n, W, rb = 1 << log_n, 2, 1
    vals = rand_field(rng, W, n, noncanonical=True)
    N = n << rb
    try:
        e.check(e.lib.p2hot_tune_ntt(e.ctx, mode))
        e.profile(True)
        e.profile_results(reset=True)
        r = e.commit(e.dev(vals), log_n, rb, N.bit_length() - 1, True)
        coeffs, lde = e.host(r["coeffs"]), e.host(r["lde"])
        prof = e.profile_results(reset=True)
        e.profile(False)
    finally:
        e.check(e.lib.p2hot_tune_ntt(e.ctx, 3))
    assert ("bitrev_permute" in prof) == (not reads_bitrev), (ks, prof)
    for c in range(W):
        assert (coeffs[c] == ntt_ref.reduce(ora.ifft(vals[c].copy()))).all(), (log_n, mode, c)
        assert int(coeffs[c, n // 3]) == ntt_ref.fft_at(vals[c], n // 3, inverse=True)
    exp = lde_expected_blocks(coeffs, log_n, rb, pyref.G, 0, 1 << rb, ora)
    assert (lde == exp).all(), (log_n, bits, mode)
    assert int(lde[0, N - 5]) == ntt_ref.lde_row_at(coeffs[0], rb, pyref.G, N - 5)


# ---------------------------------------------------------------- contiguous-pass table staging (tiles_log)
def tiles_log(log_n, groups, limit=4):
    """launch_limb_pass: how many tiles a contiguous-pass workgroup keeps its staged tables for (groups = batch x cosets)"""
    t, gx = 0, 1 << (log_n - 12)
    while t < limit and (gx >> (t + 1)) >= 1 and (gx >> (t + 1)) * groups >= 4096:
        t += 1
    return t


@pytest.mark.parametrize("shape", [(16, 512), (16, 1024), (16, 2048), (16, 4096), (13, 4096)])
def test_contiguous_pass_staged_tables(eng, ora, shape):
    """fft / ifft batches that drive tiles_log through 1..4 (2^16 x 512 .. 4096; 2^13 x 4096 on the CPU tier: tiles_log 1),
    with P2HOT_LIMB_TILES_LOG at 4 (default) and 0: the same outputs, and rows of every staged tile group against the oracle"""
    log_n, batch = shape
    if not is_gpu(eng) and shape != (13, 4096):
        pytest.skip("2^28-word batches: GPU tier (-m gpu)")
    assert tiles_log(log_n, batch) == {512: 1, 1024: 2, 2048: 3, 4096: 4}[batch] if log_n == 16 else tiles_log(log_n, batch) == 1
    rng = np.random.default_rng(batch + log_n)
    a = rand_field(rng, batch, 1 << log_n, noncanonical=True)
    a[1] = 2**64 - 1
    a[batch - 1] = np.resize(np.array([2**64 - 1, 0], dtype=U64), 1 << log_n)
    e4, e0 = variant(eng), variant(eng, LIMB_TILES_LOG=0)
    d4, d0 = e4.dev(a), e0.dev(a)
    e4.fft(d4, log_n)
    e0.fft(d0, log_n)
    e4.sync()
    e0.sync()
    assert bool((d4 == d0).all()), (shape, "staged != unstaged")  # (on the device: 2 GiB at 2^16 x 4096)
    picks = sorted({0, 1, 2, batch // 2 + 1, batch - 2, batch - 1})
    for i in picks:
        assert (e4.host(d4[i:i + 1])[0] == ntt_ref.reduce(ora.fft(a[i].copy()))).all(), (shape, i)
    e4.ifft(d4, log_n)
    for i in picks:
        assert (e4.host(d4[i:i + 1])[0] == ntt_ref.reduce(a[i])).all(), (shape, "ifft(fft(x))", i)


# ---------------------------------------------------------------- kernel variants
TUNE_SIZES_CPU = ((12, 10), (14, 10), (17, 10), (19, 6))   # contiguous only; word strided 2; limb strided 5; limb 4 + word 3
TUNE_SIZES_GPU = TUNE_SIZES_CPU + ((22, 10), (20, 6), (23, 10))


def test_tune_modes_per_pass_shape(eng, ora):
    """p2hot_tune_ntt 0 (ntt_pass_kernel, LDS radix-2), 4 (radix 16), 8 (radix 8 on words), 3 (limbs, default): one size per pass
    shape, the stress rows and the boundary impulses"""
    gpu = is_gpu(eng)
    for log_n, b in (TUNE_SIZES_GPU if gpu else TUNE_SIZES_CPU):
        e = variant(eng) if b == 10 else variant(eng, NTT_STRIDED_BITS=b)
        widths = plan(log_n, b)
        rows = stress_rows(log_n, full=log_n <= 22) if log_n <= 22 else stress_rows(log_n)[:1]
        rows += impulse_rows(log_n, boundary_impulses(log_n, widths))
        try:
            for mode in (0, 4, 8, 3):
                e.check(e.lib.p2hot_tune_ntt(e.ctx, mode))
                check_plan(e, ora, log_n, widths, rows, ("tune", mode, "bits", b))
        finally:
            e.check(e.lib.p2hot_tune_ntt(e.ctx, 3))


def _runs_standalone_bitrev(e, log_n=16):
    """a from_values commit at a two-pass size runs the stand-alone bit reversal exactly when the LDE cannot read the bit-reversed
    source -- i.e. when the limb passes are off"""
    rng = np.random.default_rng(9)
    vals = rand_field(rng, 1, 1 << log_n)
    e.profile(True)
    e.profile_results(reset=True)
    e.commit(e.dev(vals), log_n, 0, log_n, True)
    prof = e.profile_results(reset=True)
    e.profile(False)
    return "bitrev_permute" in prof


def test_ntt_limb_off_stays_off_and_matches(eng, ora):
    """P2HOT_NTT_LIMB=0 selects the word kernels and is sticky: p2hot_tune_ntt(ctx, 3) does not switch the limb passes back on
    (p2hot.hip force_no_limb); P2HOT_NTT_XCD_REMAP=0 changes only the placement of strided workgroups.  Both compute the same
    transforms at one size per pass shape"""
    e = variant(eng, NTT_LIMB=0)
    assert not _runs_standalone_bitrev(variant(eng))
    assert _runs_standalone_bitrev(e)
    e.check(e.lib.p2hot_tune_ntt(e.ctx, 3))
    assert _runs_standalone_bitrev(e)
    sizes = (12, 14, 16, 19, 22) if is_gpu(eng) else (12, 14, 16, 19)
    for knob in ({"NTT_LIMB": 0}, {"NTT_XCD_REMAP": 0}):
        e = variant(eng, **knob)
        for log_n in sizes:
            widths = plan(log_n)
            rows = stress_rows(log_n) + impulse_rows(log_n, boundary_impulses(log_n, widths))
            check_plan(e, ora, log_n, widths, rows, knob)


# ---------------------------------------------------------------- the limb unit's bounds (nttl.hpp), restated
NTTL = open(os.path.join(ROOT, "plonky2_amd", "csrc", "nttl.hpp")).read()
B = 1 << 24


def _c(expr, env):
    """a C integer expression of nttl.hpp in Python (u / ull suffixes and (u32) casts dropped: every value here fits)"""
    expr = re.sub(r"\b(0x[0-9A-Fa-f]+|\d+)u(ll)?\b", r"\1", expr.replace("(u32)", "").replace("gl::P", str(P)))
    return eval(expr, {"__builtins__": {}}, env)


def limb_constants():
    """B1..B3, BIAS_S, BIAS_R and the bias limbs O0..O3 as nttl.hpp defines them"""
    env = {}
    for name in ("B1", "B2", "B3"):
        env[name] = _c(re.search(r"\b%s = ([^,;]+)[,;]" % name, NTTL).group(1), env)
    for name in ("BIAS_S", "BIAS_R"):
        env[name] = _c(re.search(r"constexpr u64 %s = ([^;]+);" % name, NTTL).group(1), env)
    decl = re.search(r"constexpr u32 (O0 = .*?);", NTTL, re.S).group(1)
    for part in re.split(r",\s*(?=O\d = )", decl):
        name, expr = part.split("=", 1)
        env[name.strip()] = _c(expr, env)
    return env


K = limb_constants()
BIAS = [K["O0"], K["O1"], K["O2"], K["O3"]]
SPLIT_MAX = [B - 1, B - 1, 2**16 - 1, 0]   # split(x): l0, l1 < 2^24, l2 = x >> 48 < 2^16, l3 = 0


def split(x):
    return [x & (B - 1), (x >> 24) & (B - 1), x >> 48, 0]


def subrot(a, b, R):
    """(a - b) * B^R in Z[B]/(B^4 + 1): limb i lands in slot (i + R) mod 4, negated once per wrap"""
    r = [None] * 4
    for i in range(4):
        j, neg = (i + R) & 3, ((i + R) >> 2) & 1
        r[j] = b[i] - a[i] if neg else a[i] - b[i]
    return r


def dft_limbs(x, p, inv):
    """nttl.hpp dft_limbs<P, INV>: the butterflies in place, DIF, bit-reversed output; works on any limb objects with + and -"""
    x = list(x)
    rot = (lambda R: (8 - R) & 7) if inv else (lambda R: R)

    def bf(q, d, R):
        a, b = x[q], x[q + d]
        x[q] = [u + v for u, v in zip(a, b)]
        x[q + d] = subrot(a, b, rot(R))
    if p == 3:
        for q in range(4):
            bf(q, 4, q)
        for q, R in ((0, 0), (1, 2), (4, 0), (5, 2)):
            bf(q, 2, R)
        for q in range(0, 8, 2):
            bf(q, 1, 0)
    elif p == 2:
        bf(0, 2, 0)
        bf(1, 2, 2)
        for q in range(0, 4, 2):
            bf(q, 1, 0)
    else:
        bf(0, 1, 0)
    return x


def unit(words, p, inv):
    """the limb unit on 64-bit words: split, bias on input 0, butterflies -> output limbs (plain integers, any sign)"""
    x = [split(w) for w in words]
    x[0] = [l + o for l, o in zip(x[0], BIAS)]
    return dft_limbs(x, p, inv)


def limb_value(l):
    return sum(v * pow(B, i, P) for i, v in enumerate(l)) % P


def unit_bounds(p, inv):
    """exact [min, max] of every output limb over all split inputs: each output limb is the bias term plus a +-1 combination of
    input limbs (a linear form), so its extremes sit at the vertices of the input box; also returns the extreme vertices"""
    n = 1 << p
    nv = 4 * n
    forms = [[[1 if v == 4 * q + i else 0 for v in range(nv)] + [BIAS[i] if q == 0 else 0] for i in range(4)] for q in range(n)]
    out = dft_limbs([[np.array(f, dtype=object) for f in limbs] for limbs in forms], p, inv)
    vmax = [SPLIT_MAX[v % 4] for v in range(nv)]
    res = []
    for q in range(n):
        for i in range(4):
            f = out[q][i]
            lo = f[-1] + sum(c * m for c, m in zip(f[:-1], vmax) if c < 0)
            hi = f[-1] + sum(c * m for c, m in zip(f[:-1], vmax) if c > 0)
            assert set(f[:-1]) <= {-1, 0, 1}
            v_lo = [m if c < 0 else 0 for c, m in zip(f[:-1], vmax)]
            v_hi = [m if c > 0 else 0 for c, m in zip(f[:-1], vmax)]
            res.append((q, i, lo, hi, v_lo, v_hi))
    return res


def words_of(limb_vertex):
    """the 64-bit words whose split is this vertex (l3 = 0 always)"""
    return [limb_vertex[4 * q] + (limb_vertex[4 * q + 1] << 24) + (limb_vertex[4 * q + 2] << 48) for q in range(len(limb_vertex) // 4)]


def test_limb_bias_represents_zero():
    """nttl.hpp: B^4 = -1 (mod P), B1..B3 = B^i mod P, and the bias limbs O0..O3 (2^27 + the digits of -BIAS_S) represent 0"""
    assert (B**4 + 1) % P == 0
    assert [K["B1"], K["B2"], K["B3"]] == [pow(B, i, P) for i in (1, 2, 3)]
    assert K["BIAS_R"] == P - K["BIAS_S"] and K["BIAS_S"] == sum(BIAS[3] * pow(B, i, P) for i in range(4)) % P
    assert sum(o * B**i for i, o in enumerate(BIAS)) % P == 0
    assert all(0 <= o < 2**32 for o in BIAS)


@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("inv", [False, True])
def test_limb_unit_limbs_stay_in_range(p, inv):
    """every output limb of a 2^p-point unit stays in [0, 2^29) over all split inputs (exact linear-form bounds, checked on the
    extreme vertices themselves and -- for p = 1, 2 -- on every vertex of the input box), so the conversions' accumulators stay
    below 2^63 (nttl.hpp convmul, conv_unit)"""
    bounds = unit_bounds(p, inv)
    lmax = [0] * 4
    for q, i, lo, hi, v_lo, v_hi in bounds:
        assert 0 <= lo and hi < 2**29, ("limb", q, i, "range", lo, hi, "bias", BIAS)
        assert unit(words_of(v_lo), p, inv)[q][i] == lo and unit(words_of(v_hi), p, inv)[q][i] == hi
        lmax[i] = max(lmax[i], hi)
    if p < 3:
        import itertools
        nvar = 3 << p
        for signs in itertools.product((0, 1), repeat=nvar):
            v = [0] * (4 << p)
            for j, s in enumerate(signs):
                q, i = divmod(j, 3)
                v[4 * q + i] = SPLIT_MAX[i] * s
            out = unit(words_of(v), p, inv)
            assert all(0 <= l < 2**29 for limbs in out for l in limbs), signs
    # convmul: al = sum L_i * lo32(W_i), ah = sum L_i * hi32(W_i), halves of any 64-bit table word
    acc = sum(lmax[i] * (2**32 - 1) for i in range(4))
    assert acc < 2**63, acc
    # conv_unit: al = L3 * lo32(B3) + L0 + (L1 << 24), ah = L3 * hi32(B3) + (L2 << 16), and al + ah 2^32 = sum L_i B^i (mod P)
    b3 = K["B3"]
    al = lmax[3] * (b3 & 0xFFFFFFFF) + lmax[0] + (lmax[1] << 24)
    ah = lmax[3] * (b3 >> 32) + (lmax[2] << 16)
    assert al < 2**63 and ah < 2**63, (al, ah)
    rng = np.random.default_rng(p)
    for _ in range(200):
        l = [int(rng.integers(0, m + 1)) for m in lmax]
        al = l[3] * (b3 & 0xFFFFFFFF) + l[0] + (l[1] << 24)
        ah = l[3] * (b3 >> 32) + (l[2] << 16)
        assert (al + (ah << 32)) % P == limb_value(l)


@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("inv", [False, True])
def test_limb_unit_is_the_dft(p, inv):
    """the restated unit (split, bias, butterflies with B-power rotations) is the 2^p-point DFT mod P with root w = B^(8 / 2^p)
    (B^-1 for the inverse), outputs bit-reversed: on random words, boundary words and every extreme vertex"""
    n = 1 << p
    w = pow(B, 8 >> p, P)
    if inv:
        w = pow(w, P - 2, P)
    rng = np.random.default_rng(10 + p)
    cases = [[int(x) for x in rng.integers(0, 2**64, n, dtype=U64)] for _ in range(100)]
    cases += [[int(x) for x in EDGE[rng.integers(0, len(EDGE), n)]] for _ in range(100)]
    cases += [words_of(v) for *_, v_lo, v_hi in unit_bounds(p, inv) for v in (v_lo, v_hi)]
    for xs in cases:
        out = unit(xs, p, inv)
        for k in range(n):
            want = sum(x * pow(w, q * k, P) for q, x in enumerate(xs)) % P
            assert limb_value(out[pyref.bitrev(k, p)]) == want, (xs, k)
