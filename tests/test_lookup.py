"""The lookup argument on the device -- p2hot_lookup_polys (lookup::lookup_rows_kernel + its scans), p2hot_quotient_polys_lookup
(lookup::lookup_terms_kernel in front of the unchanged plonk::quotient_perm_kernel) and p2hot_cols_concat -- against
tests/lookup_ref.py, a big-integer restatement of compute_lookup_polys / check_lookup_constraints / get_lut_poly and the lookup
selectors that shares no code with the library or the CPU oracle; and the quotient the device produced put through the verifier's
identity (plonk/verifier.rs:83-98) with the lookup terms in the restated vanishing polynomial."""
import ctypes as C

import numpy as np
import pytest

from tests import lookup_ref as lr
from tests import vanishing_ref as vr
from tests.conftest import P, rand_field
from tests.pyref import G

NUM_CONSTANTS = 2            # constants_sigmas: [c0, c1, the 4 + num_luts lookup selectors, sigma_0 ...]
SEL_FIRST = NUM_CONSTANTS

# num_routed, lookup_degree (= quotient degree factor - 1): LU slots, S, LUT slots, lut_degree
#   12, 3:  6, 2,  4, 2
#   14, 2:  7, 4,  4, 1     the last LU group has one slot
#   20, 2: 10, 5,  6, 2     LUT groups 3 and 4 are empty
#   80, 7: 40, 6, 26, 5     the standard config
SHAPES = [(12, 3), (14, 2), (20, 2), (80, 7)]


def _rand(rng, *shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


def _deltas(rng, nc):
    return [[int(v) for v in _rand(rng, 4)] for _ in range(nc)]


def _regions(num_routed, spec):
    """spec: per LUT (last_lu_row, number of LU rows, table length) -> lookup_rows (last_lu, last_lut, first_lut)"""
    lut_slots = lr.num_lut_slots(num_routed)
    rows = []
    for last_lu, lu_rows, table_len in spec:
        last_lut = last_lu + lu_rows
        rows.append((last_lu, last_lut, last_lut + lr.div_ceil(table_len, lut_slots) - 1))
    return rows


def _fill_lookups(rng, wires, num_routed, spec):
    """a satisfied lookup witness in `wires` (in place): per LUT a table of distinct u16 inputs, laid out from first_lut_row down and
    padded with its first entry; looking pairs drawn from it, the last LU row padded with the first entry too; multiplicities = the
    counts, at the first place the pair stands in the table.  Returns (lookup_rows, luts)"""
    lu_slots, lut_slots = lr.num_lu_slots(num_routed), lr.num_lut_slots(num_routed)
    rows, luts = _regions(num_routed, spec), []
    for (last_lu, last_lut, first_lut), (_, lu_rows, table_len) in zip(rows, spec):
        inputs = rng.choice(1 << 16, size=table_len, replace=False)
        lut = [(int(a), int(b)) for a, b in zip(inputs, rng.integers(0, 1 << 16, size=table_len))]
        luts.append(lut)
        counts = [0] * table_len
        looking = lu_rows * lu_slots - lu_slots // 3        # the last LU row (the lowest: filled last) is partly padding
        slot = 0
        for row in range(last_lut - 1, last_lu - 1, -1):
            for s in range(lu_slots):
                k = int(rng.integers(0, table_len)) if slot < looking else 0
                counts[k] += 1
                wires[2 * s][row], wires[2 * s + 1][row] = lut[k]
                slot += 1
        # (the LU rows' other routed wires keep their random values: LookupGate has no constraints of its own)
        for row in range(first_lut, last_lut - 1, -1):
            for s in range(lut_slots):
                k = (first_lut - row) * lut_slots + s
                wires[3 * s][row], wires[3 * s + 1][row] = lut[k] if k < table_len else lut[0]
                wires[3 * s + 2][row] = counts[k] if k < table_len else 0
    return rows, luts


def _spec_for(num_routed, log_n, adjacent=False):
    """two LUTs in 2^log_n >= 16 rows: A = rows 1.., B behind it -- separated by at least one row, or B.last_lu == A.first_lut + 1"""
    lut_slots = lr.num_lut_slots(num_routed)
    a = (1, 2, lut_slots + 1)                    # two LU rows, a table of two LUT rows (the second mostly padding)
    a_first = _regions(num_routed, [a])[0][2]
    b = (a_first + (1 if adjacent else 3), 1, lut_slots - 1)
    assert _regions(num_routed, [b])[0][2] + 1 < 1 << log_n
    return [a, b]


# ------------------------------------------------------------------ 4. the restatement on its own
@pytest.mark.parametrize("num_routed,lookup_degree", SHAPES)
def test_ref_satisfied_witness_closes(num_routed, lookup_degree):
    """on a satisfied witness the last SLDC polynomial is 0 at last_lu_row (Sum(end) = LDC(end)) and RE at last_lut_row is
    get_lut_poly(delta); every lookup term vanishes on H; one wrong multiplicity breaks the first"""
    rng = np.random.default_rng(num_routed)
    log_n = 5
    n = 1 << log_n
    wires = _rand(rng, num_routed, n).astype(object)
    rows, luts = _fill_lookups(rng, wires, num_routed, _spec_for(num_routed, log_n))
    deltas = _deltas(rng, 1)
    qdf = lookup_degree + 1
    polys = lr.compute_lookup_polys(wires, deltas[0], rows, num_routed, qdf)
    S = lr.div_ceil(lr.num_lu_slots(num_routed), lookup_degree)
    assert len(polys) == S + 1
    for (last_lu, last_lut, first_lut), lut in zip(rows, luts):
        assert polys[S][last_lu] == 0
        assert polys[0][last_lut] == lr.lut_re_poly_eval(lut, lr.num_lut_slots(num_routed), deltas[0])
    sel = lr.selectors_lookup(n, rows) + lr.selector_ends_lookups(n, rows)
    for i in range(n):
        t = lr.check_lookup_constraints(vr.BASE, [int(wires[j][i]) for j in range(num_routed)], [p[i] for p in polys],
                                        [p[(i + 1) % n] for p in polys], [s[i] for s in sel], deltas[0], luts, num_routed, qdf)
        assert len(t) == 4 + len(luts) + 2 * S and not any(t), i
    wires[2][rows[0][2]] = (int(wires[2][rows[0][2]]) + 1) % P
    assert lr.compute_lookup_polys(wires, deltas[0], rows, num_routed, qdf)[S][rows[0][0]] != 0


def test_ref_leave_one_out_sums_are_the_streamed_ones():
    """sum_i m_i prod_{j != i} d_j by the recurrence S <- S d + m P, P <- P d (what the kernels run) = the O(d^2) form"""
    rng = np.random.default_rng(1)
    for cnt in (0, 1, 2, 7):
        d, m = [int(v) for v in _rand(rng, cnt)], [int(v) for v in _rand(rng, cnt)]
        plain = 0
        for i in range(cnt):
            t = m[i]
            for j in range(cnt):
                if j != i:
                    t = t * d[j] % P
            plain = (plain + t) % P
        prod, s = 1, 0
        for di, mi in zip(d, m):
            s, prod = (s * di + mi * prod) % P, prod * di % P
        assert s == plain


# ------------------------------------------------------------------ 1. - 3. the lookup polynomials
def _library_polys(eng, wires, rows, deltas, num_routed, lookup_degree):
    from plonky2_amd.plonk.prover import all_lookup_polys
    cols, host = all_lookup_polys(np.asarray(wires, dtype=np.uint64), rows, deltas, lr.num_lu_slots(num_routed),
                                  lr.num_lut_slots(num_routed), lookup_degree, want_host=True, engine=eng)
    return cols, host


@pytest.mark.parametrize("adjacent", [False, True])
@pytest.mark.parametrize("nc", [1, 2])
@pytest.mark.parametrize("num_routed,lookup_degree,log_n", [(12, 3, 5), (14, 2, 5), (20, 2, 5), (80, 7, 6)])
def test_lookup_polys_vs_restatement(eng, num_routed, lookup_degree, log_n, nc, adjacent):
    from plonky2_amd.fri.oracle import DeviceColumns, PolynomialBatch
    from plonky2_amd.plonk.prover import concat_columns
    rng = np.random.default_rng(num_routed * 100 + nc * 10 + adjacent)
    n = 1 << log_n
    wires = _rand(rng, num_routed, n).astype(object)
    rows, _ = _fill_lookups(rng, wires, num_routed, _spec_for(num_routed, log_n, adjacent))
    if adjacent:
        assert rows[1][0] == rows[0][2] + 1
    deltas = _deltas(rng, nc)
    exp = np.asarray(lr.compute_all_lookup_polys(wires, deltas, rows, num_routed, lookup_degree + 1), dtype=np.uint64)
    cols, host = _library_polys(eng, wires, rows, deltas, num_routed, lookup_degree)
    S = lr.div_ceil(lr.num_lu_slots(num_routed), lookup_degree)
    assert exp.shape == (nc * (S + 1), n) and host.shape == exp.shape
    assert (host == exp).all()
    assert (cols.host() == exp).all()
    inside = np.zeros(n, dtype=bool)
    for last_lu, _, first_lut in rows:
        inside[last_lu:first_lut + 1] = True
    assert not host[:, ~inside].any() and host[:, inside].any()
    # the prover's next step (prover.rs:237-241): behind the Zs / partial products, into one commitment
    zs = _rand(rng, 3, n)
    both = concat_columns(DeviceColumns.upload(zs, eng), cols, eng)
    b = PolynomialBatch.from_values(both, 1, False, 0, engine=eng)
    ref = PolynomialBatch.from_values(np.concatenate([zs, exp]), 1, False, 0, engine=eng)
    assert b.merkle_tree.cap.entries.any() and (b.merkle_tree.cap.entries == ref.merkle_tree.cap.entries).all()


def _carries_per(region):
    """chunks per thread of lookup::lookup_carries_kernel for one region: SCAN_CHUNK = 4 rows per chunk (csrc/lookup.hpp), one block
    of 1024 threads over the chunks (its launch in p2hot_lookup_polys, csrc/host_plonk.hpp)"""
    last_lu, _, first_lut = region
    n_chunks = lr.div_ceil(first_lut - last_lu + 1, 4)
    return n_chunks, lr.div_ceil(n_chunks, 1024)


def test_lookup_polys_scan_boundaries(eng):
    """a LUT region of 300 rows under an LU region of 3000 rows: both span several workgroups of the scan kernels and (the LU one)
    of the row kernel, and the carries cross from one to the other.  Random wires: the values are defined for any witness.

    Second case, 2^13 rows: a region of 8002 rows = 2001 chunks, so every thread of the carries kernel reduces and replays TWO
    chunks, thread 1000 one (its `hi` is clamped) and threads 1001.. none (`lo` clamped).  Its 1102 LookupTable rows end inside
    chunk 275, the second chunk of thread 137's pair.  It is processed after an adjacent region made of LookupTable rows only, whose
    last row is this one's first_lut + 1: both seeds (RE and the last SLDC) are nonzero."""
    rng = np.random.default_rng(12)
    num_routed, lookup_degree, log_n = 12, 3, 12
    wires = _rand(rng, num_routed, 1 << log_n)
    rows = [(500, 3500, 3799)]
    assert _carries_per(rows[0])[1] == 1
    for nc in (1, 2):
        deltas = _deltas(rng, nc)
        exp = np.asarray(lr.compute_all_lookup_polys(wires, deltas, rows, num_routed, lookup_degree + 1), dtype=np.uint64)
        _, host = _library_polys(eng, wires, rows, deltas, num_routed, lookup_degree)
        assert (host == exp).all()
        assert not host[:, :500].any() and not host[:, 3800:].any() and host[1:3, 500].all() and not host[0, :3500].any()
    log_n = 13
    wires = _rand(rng, num_routed, 1 << log_n)
    big, above = (101, 7001, 8102), (8103, 8103, 8150)
    n_chunks, per = _carries_per(big)
    len_lut = big[2] - big[1] + 1
    assert per == 2 and 1024 < n_chunks <= 2048 and n_chunks % 2 == 1 and len_lut % 4 and len_lut % 8
    assert (len_lut // 4) % 2 == 1          # the chunk that holds the LookupTable / Lookup boundary is the second of a thread's two
    assert above[0] == big[2] + 1 and _carries_per(above)[1] == 1
    rows = [above, big]
    for nc in (1, 2):
        deltas = _deltas(rng, nc)
        exp = np.asarray(lr.compute_all_lookup_polys(wires, deltas, rows, num_routed, lookup_degree + 1), dtype=np.uint64)
        _, host = _library_polys(eng, wires, rows, deltas, num_routed, lookup_degree)
        S = lr.div_ceil(lr.num_lu_slots(num_routed), lookup_degree)
        assert exp[::S + 1, big[2] + 1].all() and exp[S::S + 1, big[2] + 1].all()      # the seeds: RE and the last SLDC of every challenge
        assert (host == exp).all()
        assert not host[:, :big[0]].any() and not host[:, above[2] + 1:].any() and not host[::S + 1, big[0]:big[1]].any()


def test_lookup_polys_noncanonical_host_words(eng):
    """the caller's words are raw GoldilocksField(u64): wires in [P, 2^64) -- 2^64 - 1 and P among them -- give the polynomials of
    the reduced words, canonical; deltas handed over as delta + P give the same bytes"""
    rng = np.random.default_rng(77)
    num_routed, lookup_degree, log_n, nc = 12, 3, 5, 2
    rows = _regions(num_routed, _spec_for(num_routed, log_n, adjacent=True))
    wires = rand_field(rng, num_routed, 1 << log_n, noncanonical=True)
    (last_lu, last_lut, first_lut) = rows[0]
    wires[1][last_lu] = (1 << 64) - 1          # a looking output, a looked input
    wires[3][first_lut] = P
    assert (wires >= P).sum() > 2
    reduced = np.asarray([[int(v) % P for v in col] for col in wires], dtype=object)
    small = rng.integers(1, (1 << 32) - 1, size=4, dtype=np.uint64)
    deltas = [[int(v) for v in small], [int(v) for v in _rand(rng, 4)]]
    deltas[1][lr.DELTA] = int(small[0]) // 2 + 7
    exp = np.asarray(lr.compute_all_lookup_polys(reduced, deltas, rows, num_routed, lookup_degree + 1), dtype=np.uint64)
    cols, host = _library_polys(eng, wires, rows, deltas, num_routed, lookup_degree)
    assert (host < P).all() and (host == exp).all() and (cols.host() == exp).all()
    shifted = [[d + P if d + P < 1 << 64 else d for d in ds] for ds in deltas]
    assert sum(a != b for da, db in zip(deltas, shifted) for a, b in zip(da, db)) == 5
    cols2, host2 = _library_polys(eng, wires, rows, shifted, num_routed, lookup_degree)
    assert host2.tobytes() == host.tobytes() and cols2.host().tobytes() == host.tobytes()


def test_lookup_polys_follow_the_callers_region_order(eng):
    """adjacent regions on an invalid witness: processed [A, B], A reads zeros at its first_lut + 1 and B overwrites that row later;
    processed [B, A], A's SLDC carry-in is B's final value (RE there stays 0: B's LU rows never set it)"""
    rng = np.random.default_rng(3)
    num_routed, lookup_degree, log_n = 12, 3, 5
    wires = _rand(rng, num_routed, 1 << log_n)
    a, b = _regions(num_routed, _spec_for(num_routed, log_n, adjacent=True))
    assert b[0] == a[2] + 1
    deltas = _deltas(rng, 2)
    got = {}
    for name, rows in (("ab", [a, b]), ("ba", [b, a])):
        exp = np.asarray(lr.compute_all_lookup_polys(wires, deltas, rows, num_routed, lookup_degree + 1), dtype=np.uint64)
        _, got[name] = _library_polys(eng, wires, rows, deltas, num_routed, lookup_degree)
        assert (got[name] == exp).all(), name
    assert (got["ab"] != got["ba"]).any()
    assert (got["ab"][:, b[0]:] == got["ba"][:, b[0]:]).all()      # B's own rows do not depend on the order


# ------------------------------------------------------------------ 5. - 7. the quotient
def _instance(rng, nc, qdf, num_routed, rate_bits, log_n, satisfied=True, zero_selectors=False):
    """values on H of the three committed batches of a lookup circuit.  wires = [routed..., one free wire, e, f] with e = w0 w1 and
    f = w0 + w1 on H (vr.gate_constraints: its constraints sit on the two non-lookup wires e, f); identity permutation
    (sigma_j(w^i) = k_j w^i), so any wire values satisfy the copy constraints; constants_sigmas = [c0, c1, lookup selectors,
    sigmas]; zs = Zs, partial products (the restatement's), lookup polynomials (the restatement's)"""
    n = 1 << log_n
    routed = _rand(rng, num_routed, n).astype(object)
    spec = _spec_for(num_routed, log_n)
    if satisfied:
        rows, luts = _fill_lookups(rng, routed, num_routed, spec)
    else:
        rows = _regions(num_routed, spec)
        luts = [[(int(a), int(b)) for a, b in rng.integers(0, 1 << 16, size=(t, 2))] for _, _, t in spec]
    routed = routed.astype(np.uint64)
    free = _rand(rng, 1, n)
    w = np.concatenate([routed, free])
    w0, w1 = [int(v) for v in w[0]], [int(v) for v in w[1]]
    ef = np.asarray([[a * b % P for a, b in zip(w0, w1)], [(a + b) % P for a, b in zip(w0, w1)]], dtype=np.uint64)
    wires = np.concatenate([w, ef if satisfied else _rand(rng, 2, n)])
    k_is = [pow(G, j, P) for j in range(num_routed)]
    sub = vr.subgroup(log_n)
    sigmas = np.asarray([[k * x % P for x in sub] for k in k_is], dtype=np.uint64)
    sel = np.asarray(lr.selectors_lookup(n, rows) + lr.selector_ends_lookups(n, rows), dtype=np.uint64)
    if zero_selectors:
        sel[:] = 0
    cs = np.concatenate([_rand(rng, NUM_CONSTANTS, n), sel, sigmas])
    betas, gammas, alphas = ([int(v) for v in _rand(rng, nc)] for _ in range(3))
    deltas = _deltas(rng, nc)
    zpp = vr.zs_partial_products_batch(routed, sigmas, k_is, betas, gammas, qdf)
    lk = lr.compute_all_lookup_polys(routed, deltas, rows, num_routed, qdf)
    zs = np.asarray(zpp + lk, dtype=np.uint64)
    evals = [[lr.lut_re_poly_eval(lut, lr.num_lut_slots(num_routed), d) for lut in luts] for d in deltas]
    return dict(nc=nc, qdf=qdf, num_routed=num_routed, rate_bits=rate_bits, log_n=log_n, n=n, k_is=k_is, betas=betas, gammas=gammas,
                alphas=alphas, deltas=deltas, wires=wires, cs=cs, zs=zs, rows=rows, luts=luts, evals=evals, num_zpp=len(zpp),
                sigmas_first=SEL_FIRST + 4 + len(luts), lu_slots=lr.num_lu_slots(num_routed), lut_slots=lr.num_lut_slots(num_routed),
                S=lr.div_ceil(lr.num_lu_slots(num_routed), qdf - 1))


def _ref_ldes(q):
    return {name: vr.Lde(vr.interpolate_columns(q[name]), q["log_n"], q["rate_bits"]) for name in ("wires", "cs", "zs")}


def _ref_quotient(q, ldes, with_gates, variant=None):
    return lr.quotient_values(ldes["wires"], ldes["cs"], ldes["zs"], SEL_FIRST, len(q["luts"]), q["sigmas_first"], q["k_is"], q["qdf"],
                              q["betas"], q["gammas"], q["alphas"], q["deltas"], q["luts"], with_gates, variant)


def _gate_sums(q, lde_w, lde_cs):
    qbits = vr.log2_ceil(q["qdf"])
    m = q["n"] << qbits
    out = np.zeros((q["nc"], m), dtype=np.uint64)
    for i in range(m):
        (li, step), _ = vr.quotient_rows(i, q["log_n"], q["rate_bits"], qbits)
        t = vr.gate_constraints(vr.BASE, vr.get_lde_values(lde_w, li, step), vr.get_lde_values(lde_cs, li, step))
        for a in range(q["nc"]):
            out[a, i] = vr.reduce_with_powers(vr.BASE, t, q["alphas"][a])
    return out


def _commit(eng, q):
    from plonky2_amd.fri.oracle import PolynomialBatch
    return {name: PolynomialBatch.from_values(q[name], q["rate_bits"], False, 0, engine=eng) for name in ("wires", "cs", "zs")}


def _library_quotient(eng, q, b, gate_sums):
    from plonky2_amd.plonk.prover import compute_quotient_polys_lookup
    return compute_quotient_polys_lookup(b["wires"], b["cs"], q["sigmas_first"], b["zs"], q["k_is"], q["qdf"], q["betas"], q["gammas"],
                                         q["alphas"], q["lu_slots"], q["lut_slots"], SEL_FIRST, q["deltas"], q["evals"],
                                         gate_sums=gate_sums, want_values=True, engine=eng)


QUOTIENT_SHAPES = [(12, 4), (14, 3), (20, 3), (80, 8)]      # num_routed, quotient degree factor (lookup_degree + 1)
# ... with the number of challenges: 1 and 2 everywhere, 3 (lookup_terms_kernel<3>, quotient_perm_kernel<3, 0>; the Zs batch of
# _instance is as wide as its challenges ask) on the shape whose last LookupGate group has one slot
QUOTIENT_CASES = [(r, f, nc) for nc in (1, 2) for r, f in QUOTIENT_SHAPES] + [(14, 3, 3)]
_SHARED = {}


def _shared(num_routed, qdf, nc, satisfied):
    """the instance, the restatement's LDEs and its quotient values (with and without the gate terms): computed once per shape"""
    key = (num_routed, qdf, nc, satisfied)
    if key not in _SHARED:
        rng = np.random.default_rng(num_routed * 1000 + qdf * 10 + nc + (0 if satisfied else 5))
        q = _instance(rng, nc, qdf, num_routed, 3, 4, satisfied=satisfied)
        ldes = _ref_ldes(q)
        gs = _gate_sums(q, ldes["wires"], ldes["cs"])
        _SHARED[key] = (q, ldes, gs, {False: _ref_quotient(q, ldes, False), True: _ref_quotient(q, ldes, True)})
    return _SHARED[key]


@pytest.mark.parametrize("satisfied", [True, False])
@pytest.mark.parametrize("num_routed,qdf,nc", QUOTIENT_CASES)
def test_quotient_values_vs_restatement(eng, num_routed, qdf, nc, satisfied):
    """every point of the quotient coset (rate_bits 3, 2^4 rows), with and without gate_sums, on a satisfied and on a random instance"""
    q, ldes, gs, exp = _shared(num_routed, qdf, nc, satisfied)
    b = _commit(eng, q)
    for gates in (False, True):
        vals = _raw_values(eng, q, b, gs if gates else None)
        assert (vals == np.asarray(exp[gates], dtype=np.uint64)).all(), gates


_KEEP = []


def _u64(v):
    a = np.ascontiguousarray(np.asarray(v, dtype=np.uint64))
    _KEEP.append(a)
    return a.ctypes.data_as(C.c_void_p)


def _ptrs(rows2d):
    a = np.ascontiguousarray(np.asarray(rows2d, dtype=np.uint64))
    _KEEP.append(a)
    return (C.c_void_p * a.shape[0])(*[a[c].ctypes.data for c in range(a.shape[0])])


def _raw_values(eng, q, b, gate_sums, zs=None):
    """p2hot_quotient_polys_lookup for the VALUES on the coset alone (no chunks: nothing is trimmed, any instance has values)"""
    from plonky2_amd import _lib
    nc = q["nc"]
    vals = np.zeros((nc, q["n"] << vr.log2_ceil(q["qdf"])), dtype=np.uint64)
    rc = eng.lib.p2hot_quotient_polys_lookup(
        eng.ctx, b["wires"]._h, b["cs"]._h, q["sigmas_first"], (zs or b["zs"])._h, _u64(q["k_is"]), q["num_routed"], q["qdf"],
        _u64(q["betas"]), _u64(q["gammas"]), _u64(q["alphas"]), nc, _ptrs(gate_sums) if gate_sums is not None else None, q["lu_slots"],
        q["lut_slots"], len(q["luts"]), SEL_FIRST, _u64(q["deltas"]), _u64(q["evals"]), vals.ctypes.data_as(C.c_void_p), None)
    assert rc == _lib.OK, eng.lib.p2hot_last_error(eng.ctx)
    return vals


def _pairs(a):
    return [(int(v[0]), int(v[1])) for v in a]


def _zeta(rng):
    return (int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(1, P, dtype=np.uint64)))


def _vanishing_at(q, zeta, w_z, cs_z, zs_z, zs_gz, variant=None):
    nc, nr, base = q["nc"], q["num_routed"], q["num_zpp"]
    cons = vr.gate_constraints(vr.EXT, w_z, cs_z)
    return lr.eval_vanishing_poly(vr.EXT, q["n"], zeta, w_z, zs_z[:nc], zs_gz[:nc], zs_z[nc:base], zs_z[base:], zs_gz[base:],
                                  cs_z[q["sigmas_first"]:q["sigmas_first"] + nr], cs_z[SEL_FIRST:SEL_FIRST + 4 + len(q["luts"])],
                                  q["k_is"], q["betas"], q["gammas"], q["alphas"], q["deltas"], q["luts"], q["qdf"], cons, variant)


@pytest.mark.parametrize("num_routed,qdf", QUOTIENT_SHAPES)
def test_quotient_divisibility_and_verifier_identity(eng, num_routed, qdf):
    """a satisfied instance: chunks come back (the tail is zero), and the library's own openings of the three batches at zeta / g zeta
    satisfy vanishing(zeta) = Z_H(zeta) sum_j chunk_j(zeta) zeta^(n j) with the restated lookup terms; a restatement with the lookup
    terms behind the gate terms, or with the challenges' lookup terms interleaved, does not"""
    from plonky2_amd.fri.oracle import PolynomialBatch, eval_openings
    nc = 2
    q, ldes, gs, exp = _shared(num_routed, qdf, nc, True)
    b = _commit(eng, q)
    cols, vals = _library_quotient(eng, q, b, gs)
    chunks = cols.host()
    assert chunks.shape == (nc * qdf, q["n"])
    assert (chunks == np.asarray(vr.quotient_chunks(exp[True], q["log_n"], qdf), dtype=np.uint64)).all()
    b_q = PolynomialBatch.from_coeffs(chunks, q["rate_bits"], False, 0, engine=eng)
    rng = np.random.default_rng(num_routed)
    zeta = _zeta(rng)
    gz = vr.EXT.scalar_mul(zeta, vr.root_of_unity(q["log_n"]))
    cs_z, w_z, zs_z, q_z = [_pairs(e[0]) for e in eval_openings([b["cs"], b["wires"], b["zs"], b_q], [zeta], eng)]
    zs_gz = _pairs(eval_openings([b["zs"]], [gz], eng)[0][0])
    assert zs_z == [vr.eval_ext(c, zeta) for c in ldes["zs"].coeffs]
    van = _vanishing_at(q, zeta, w_z, cs_z, zs_z, zs_gz)
    assert vr.verifier_check(vr.EXT, zeta, q["n"], van, q_z, qdf) == [True] * nc
    for variant in lr.VARIANTS[1:]:
        bad = _vanishing_at(q, zeta, w_z, cs_z, zs_z, zs_gz, variant)
        assert vr.verifier_check(vr.EXT, zeta, q["n"], bad, q_z, qdf) == [False] * nc, variant


@pytest.mark.parametrize("what", ["multiplicity", "looking_pair"])
def test_broken_lookup_fails_the_quotient(eng, what):
    """one multiplicity changed, or one looking pair replaced by a pair that is not in the table: "Quotient has failed" """
    num_routed, qdf, nc = 14, 3, 2      # 3 n of the 4 n coefficients are kept: the trim sees a quotient that is no polynomial
    q, ldes, gs, _ = _shared(num_routed, qdf, nc, True)
    q = dict(q)
    wires = q["wires"].copy()
    last_lu, last_lut, first_lut = q["rows"][0]
    if what == "multiplicity":
        wires[2][first_lut] = (int(wires[2][first_lut]) + 1) % P
    else:
        present = {a for lut in q["luts"] for a, _ in lut}
        wires[0][last_lu] = next(v for v in range(1 << 16) if v not in present)
    # e = w0 w1 and f = w0 + w1 follow the change: the gate stays satisfied, only the lookup argument is broken
    wires[-2] = [int(a) * int(b) % P for a, b in zip(wires[0], wires[1])]
    wires[-1] = [(int(a) + int(b)) % P for a, b in zip(wires[0], wires[1])]
    q["wires"] = wires
    routed = wires[:num_routed]
    zs = list(q["zs"][:q["num_zpp"]]) + lr.compute_all_lookup_polys(routed, q["deltas"], q["rows"], num_routed, qdf)
    q["zs"] = np.asarray(zs, dtype=np.uint64)
    ldes = _ref_ldes(q)
    b = _commit(eng, q)
    with pytest.raises(ValueError, match="Quotient has failed"):
        _library_quotient(eng, q, b, _gate_sums(q, ldes["wires"], ldes["cs"]))
    assert eng.lib.p2hot_ctx_trim(eng.ctx) == 0


@pytest.mark.parametrize("num_routed,qdf", [(12, 4), (80, 8)])
def test_lookup_terms_sit_between_the_permutation_and_the_gate_terms(eng, num_routed, qdf):
    """with every lookup selector column zeroed the lookup terms are zero but still occupy Klu = nc (4 + num_luts + 2 S) places:
    p2hot_quotient_polys_lookup with gate_sums = g equals the existing p2hot_quotient_polys with gate_sums = alpha^Klu g"""
    from plonky2_amd.fri.oracle import PolynomialBatch
    nc = 2
    rng = np.random.default_rng(num_routed + 1)
    q = _instance(rng, nc, qdf, num_routed, 3, 4, satisfied=False, zero_selectors=True)
    b = _commit(eng, q)
    m = q["n"] << vr.log2_ceil(qdf)
    g = _rand(rng, nc, m)
    klu = nc * (4 + len(q["luts"]) + 2 * q["S"])
    scaled = np.asarray([[int(v) * pow(q["alphas"][a], klu, P) % P for v in g[a]] for a in range(nc)], dtype=np.uint64)
    from plonky2_amd import _lib
    vals = _raw_values(eng, q, b, g)
    b_zpp = PolynomialBatch.from_values(q["zs"][:q["num_zpp"]], q["rate_bits"], False, 0, engine=eng)
    plain = np.zeros((nc, m), dtype=np.uint64)
    rc = eng.lib.p2hot_quotient_polys(eng.ctx, b["wires"]._h, b["cs"]._h, q["sigmas_first"], b_zpp._h, _u64(q["k_is"]), num_routed, qdf,
                                      _u64(q["betas"]), _u64(q["gammas"]), _u64(q["alphas"]), nc, _ptrs(scaled),
                                      plain.ctypes.data_as(C.c_void_p), None)
    assert rc == _lib.OK
    assert vals.any() and (vals == plain).all()


# ------------------------------------------------------------------ 8. shape errors
def test_shape_errors_leave_the_context_usable(eng):
    from plonky2_amd import _lib
    from plonky2_amd.fri.oracle import DeviceColumns, PolynomialBatch
    rng = np.random.default_rng(8)
    num_routed, log_n = 12, 5
    n = 1 << log_n
    wires = DeviceColumns.upload(_rand(rng, num_routed, n), eng)
    deltas = _u64(_deltas(rng, 2))
    good = [(1, 3, 4)]

    def polys(rows=good, lu=6, lut=4, deg=3, nc=2, w=wires):
        h = C.c_void_p()
        rc = eng.lib.p2hot_lookup_polys(eng.ctx, w._h, 0, lu, lut, deg, _u64(rows), len(rows), deltas, nc, None, C.byref(h))
        if h.value:
            eng.lib.p2hot_cols_free(h)
        return rc
    assert polys() == _lib.OK
    assert polys(rows=[(1, 3, n - 1)]) == _lib.EINVAL               # first_lut_gate + 1 >= n
    assert b"first_lut_gate + 1" in eng.lib.p2hot_last_error(eng.ctx)
    assert polys(rows=[(1, 3, n)]) == _lib.EINVAL
    assert polys(rows=[(4, 3, 5)]) == _lib.EINVAL                   # last_lu > last_lut
    assert polys(rows=[(1, 6, 5)]) == _lib.EINVAL                   # last_lut > first_lut
    assert polys(lu=7) == _lib.EINVAL                               # 2 * 7 wires
    assert polys(lut=5) == _lib.EINVAL                              # 3 * 5 wires
    assert polys(deg=0) == _lib.EINVAL
    assert polys(nc=0) == _lib.EINVAL and polys(nc=5) == _lib.EINVAL
    assert polys() == _lib.OK
    # a zero alpha - combination: the reference panics in batch_multiplicative_inverse
    w = _rand(rng, num_routed, n)
    d = _deltas(rng, 1)
    w[0][2], w[1][2] = d[0][lr.ALPHA], 0                            # LU row 2, slot 0: combo = alpha
    from plonky2_amd.plonk.prover import all_lookup_polys
    with pytest.raises(ValueError, match="Tried to invert zero"):
        all_lookup_polys(w, good, d, 6, 4, 3, engine=eng)
    assert polys() == _lib.OK
    # the quotient: a Zs batch of the wrong width, slots beyond the wires, challenges outside 1..4
    q = _instance(rng, 2, 4, num_routed, 3, 4, satisfied=False)
    b = _commit(eng, q)
    m = q["n"] << 2
    vals = np.zeros((2, m), dtype=np.uint64)

    def quot(zs=None, lu=q["lu_slots"], lut=q["lut_slots"], nc=2, qdf=4):
        return eng.lib.p2hot_quotient_polys_lookup(
            eng.ctx, b["wires"]._h, b["cs"]._h, q["sigmas_first"], (zs or b["zs"])._h, _u64(q["k_is"]), num_routed, qdf, _u64(q["betas"] * 3),
            _u64(q["gammas"] * 3), _u64(q["alphas"] * 3), nc, None, lu, lut, len(q["luts"]), SEL_FIRST, _u64(q["deltas"] * 3), _u64(q["evals"] * 3),
            vals.ctypes.data_as(C.c_void_p), None)
    assert quot() == _lib.OK
    narrow = PolynomialBatch.from_values(q["zs"][:-1], 3, False, 0, engine=eng)
    wide = PolynomialBatch.from_values(np.concatenate([q["zs"], q["zs"][:1]]), 3, False, 0, engine=eng)
    assert quot(zs=narrow) == _lib.EINVAL and quot(zs=wide) == _lib.EINVAL
    assert b"Zs batch" in eng.lib.p2hot_last_error(eng.ctx)
    assert quot(lu=8) == _lib.EINVAL and quot(lut=6) == _lib.EINVAL          # 16 / 18 of 15 wires
    assert quot(nc=0) == _lib.EINVAL and quot(nc=5) == _lib.EINVAL
    assert quot() == _lib.OK and vals.any()


# ------------------------------------------------------------------ 9. p2hot_cols_concat
def test_cols_concat(eng):
    from plonky2_amd import _lib
    from plonky2_amd.fri.oracle import DeviceColumns
    from plonky2_amd.plonk.prover import concat_columns
    rng = np.random.default_rng(9)
    a, b = _rand(rng, 3, 32), _rand(rng, 5, 32)
    da, db = DeviceColumns.upload(a, eng), DeviceColumns.upload(b, eng)
    both = concat_columns(da, db, eng)
    assert both.width == 8 and both.degree_log == 5
    assert (both.host() == np.concatenate([a, b])).all()
    assert (da.host() == a).all() and (db.host() == b).all()      # the inputs are untouched and still valid
    assert (concat_columns(db, da).host() == np.concatenate([b, a])).all()
    other = DeviceColumns.upload(_rand(rng, 2, 16), eng)
    h = C.c_void_p()
    assert eng.lib.p2hot_cols_concat(eng.ctx, da._h, other._h, C.byref(h)) == _lib.EINVAL and not h.value
    assert eng.lib.p2hot_cols_concat(eng.ctx, da._h, None, C.byref(h)) == _lib.EINVAL
    assert (da.host() == a).all()
