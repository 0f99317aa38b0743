"""The composed arithmetic kernels on edge words, a different one in every lane (tests/edge_words.py): the gate kernels, the
permutation argument's quotient and partial products, the Plonk and STARK lookup kernels, the two interpreters, the M-forms and
the FRI / opening arithmetic.  Uniformly random operands leave the rare branches of the Goldilocks code alone -- the second fold
of gl::add and of gl::sub, the borrow of the multiply streams, accumulators that stay in [P, 2^64) -- and constant columns put
one path into every lane of a wave; here every column holds the whole grid, shuffled per column.

Every comparison is bit for bit on canonical output words against a Python-integer reference evaluated row by row on the same
matrix.  Matrices the kernels read as LDEs are wrapped (p2hot_batch_wrap_dev) and hold canonical words in one mode and words of
[P, 2^64) in the other (the decision and the header lines it rests on: tests/edge_words.py).  References are computed once per
case and shared by the two tiers."""
import ctypes as C

import numpy as np
import pytest

from tests import edge_words as ew
from tests import gates_ref as gr
from tests import recursion_gates_ref as rr
from tests import test_gates as tg
from tests import test_quotient_edges as tq
from tests import test_recursion_gates as trg
from tests import vanishing_ref as vr
from tests.conftest import P
from tests.pyref import G

RATE_BITS = 3
MODES = [True, False]      # canonical words only; all of the grid
_REF = {}                  # case key -> (inputs, expected): built once, shared by the emulator and the GPU tier, left unchanged


def _once(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _challenges(rng, count, canonical, from_grid=False):
    """random canonical words, or grid words (raw: [P, 2^64) too where the mode has them)"""
    if from_grid:
        g = ew.grid(canonical)
        return [g[int(k)] for k in rng.choice(len(g), size=count, replace=False)]
    return [int(v) for v in rng.integers(0, P, count, dtype=np.uint64)]


# ------------------------------------------------------------------ a. the gate kernels
ALL_ALONE = dict(tg.ALONE)
ALL_ALONE.update(trg.ALONE)
assert len(ALL_ALONE) == len(tg.ALONE) + len(trg.ALONE) == 29


def _selector_columns(cs, gates, ns, rng):
    """the first ns columns of cs become selectors: every fourth row names a gate of the set (its own selector column holds the
    gate's row index, the others UNUSED_SELECTOR), every fourth row (two rows on) names an index of the gate's group that is not
    the gate's -- or the unused marker -- and the odd rows keep their edge words"""
    N = cs.shape[1]
    named = [g for g in gates if g.kind != gr.NOOP] or gates      # (a row that names Noop alone has no term at all)
    for L in range(0, N, 2):
        g = named[(L // 4) % len(named)] if L % 4 == 0 else gates[(L // 4) % len(gates)]
        if L % 4 == 0:
            for k in range(ns):
                cs[k][L] = g.row if k == g.selector_index else gr.UNUSED_SELECTOR
        else:
            others = [i for i in range(g.group[0], g.group[1]) if i != g.row] + ([gr.UNUSED_SELECTOR] if ns > 1 else [])
            cs[g.selector_index][L] = others[int(rng.integers(0, len(others)))]


def _gate_case(key, gates, ns, log_n, qdf, nc, canonical, seed, rate_bits=RATE_BITS):
    def make():
        rng = np.random.default_rng(seed)
        N = 1 << (log_n + rate_bits)
        wires = ew.edge_matrix(rng, tg.W, N, canonical)
        cs = ew.edge_matrix(rng, ns + tg.NUM_GATE_CONSTS + 1, N, canonical)        # selectors, c0, c1, one "sigma"
        _selector_columns(cs, gates, ns, rng)
        for g in gates:
            if g.kind == gr.POSEIDON:       # in a row that names the gate: state word 8 + its first round constant = 2^64 exactly (gl::add_canon)
                from tests.pyref import RC
                rows = [L for L in range(0, N >> (rate_bits - vr.log2_ceil(qdf)), 4) if int(cs[g.selector_index][L]) == g.row]
                L = next(L for L in rows if set(ew.grid(canonical)) <= set(int(v) for k, v in enumerate(wires[8]) if k != L))
                wires[8][L] = 2**64 - RC[8]
                assert RC[8] >= 2**32 and (wires[8][1:] != wires[8][:-1]).all()
        pih = _challenges(rng, 4, canonical, from_grid=True)
        # (a grid word that is not zero: with alpha = 0 a sum is the gate's first constraint alone, which edge wires do satisfy)
        alphas = [a for a in _challenges(rng, 3, canonical, from_grid=True) if a % P][:1] + _challenges(rng, nc - 1, canonical)
        lw, lcs = ew.leaves(wires, log_n, rate_bits), ew.leaves(cs, log_n, rate_bits)
        qbits = vr.log2_ceil(qdf)
        m = (1 << log_n) << qbits
        exp = np.zeros((nc, m), dtype=np.uint64)
        filters = set()
        for i in range(m):
            L, _ = ew.point_rows(i, log_n, rate_bits, qbits)
            w, c = lw.row(L), lcs.row(L)
            exp[:, i] = rr.reduced_sums(vr.BASE, gates, ns, 0, w, c, pih, alphas)
            filters |= {(g.row, gr.compute_filter(vr.BASE, g.row, g.group, c[g.selector_index], ns > 1) != 0) for g in gates}
        # the filter selects and rejects every gate of the set somewhere
        assert filters == {(g.row, f) for g in gates for f in (False, True)}
        return dict(wires=wires, cs=cs, pih=pih, alphas=alphas), exp
    return _once(("gates",) + key + (canonical,), make)


def _run_gate_case(eng, inp, gates, ns, log_n, qdf, rate_bits=RATE_BITS):
    from plonky2_amd.plonk.prover import GateSet, gate_sums
    bw, bcs = ew.wrap(eng, inp["wires"], log_n, rate_bits), ew.wrap(eng, inp["cs"], log_n, rate_bits)
    return gate_sums(bw, bcs, ns + tg.NUM_GATE_CONSTS, GateSet([g.descriptor() for g in gates], ns, 0, inp["pih"]), qdf, inp["alphas"], engine=eng)


@pytest.mark.parametrize("name", sorted(ALL_ALONE))
def test_gate_sums_of_one_gate_on_edge_rows(eng, name):
    """every standard and every recursion kind alone in a group of three, two challenges (the stream instantiation), 2^3 rows:
    64 points = one wave of 64 different rows"""
    kind, p0, p1 = ALL_ALONE[name]
    gates = tg._alone(kind, p0, p1, row=1, group=(0, 3))
    for canonical in MODES:
        inp, exp = _gate_case((name,), gates, 1, 3, 8, 2, canonical, 7000 + 100 * kind + p0 + (p1 & 0xFF))
        got = _run_gate_case(eng, inp, gates, 1, 3, 8)
        assert got.shape == exp.shape == (2, 64) and (got == exp).all(), canonical
        assert exp.any() or kind == gr.NOOP


@pytest.mark.parametrize("nc", [2, 3])
def test_gate_sums_of_the_recursion_set_on_edge_rows(eng, nc):
    """all fourteen kinds in four selector groups at 2^4 rows (128 points); two challenges run the stream instantiation of the
    kernels, three the generic one"""
    gates, ns = trg._recursion_set()
    for canonical in MODES:
        inp, exp = _gate_case(("set", nc), gates, ns, 4, 8, nc, canonical, 7100 + nc)
        got = _run_gate_case(eng, inp, gates, ns, 4, 8)
        assert got.shape == exp.shape == (nc, 128) and (got == exp).all() and exp.all(), canonical


def test_gate_sums_on_every_second_edge_row(eng):
    """qbits = rate_bits - 1: factor 4 at rate 3, point i is committed row bitrev(2 i); the eight standard kinds in the groups of a
    factor-4 circuit"""
    gates, ns = tq._factor4_set()
    for canonical in MODES:
        inp, exp = _gate_case(("factor4",), gates, ns, 3, 4, 2, canonical, 7200)
        got = _run_gate_case(eng, inp, gates, ns, 3, 4)
        assert got.shape == exp.shape == (2, 32) and (got == exp).all() and exp.all(), canonical


# ------------------------------------------------------------------ b. the permutation argument, quotient side
def _quotient_ref_point(i, lw, lcs, lzs, sigmas_first, k_is, qdf, betas, gammas, alphas, gs):
    """vanishing_ref.quotient_value_at with the caller's gate sums behind alpha^K (one constraint term per challenge)"""
    log_n, rate_bits, qbits = lw.degree_bits, lw.rate_bits, vr.log2_ceil(qdf)
    nc, num_routed = len(betas), len(k_is)
    num_prods = vr.num_partial_products(num_routed, qdf)
    L, Ln = ew.point_rows(i, log_n, rate_bits, qbits)
    x = vr.quotient_point(i, log_n, qbits)
    w, c, z, zn = lw.row(L), lcs.row(L), lzs.row(L), lzs.row(Ln)
    zh_inv = vr.BASE.inv(vr.eval_zero_poly(vr.BASE, 1 << log_n, x))
    out = []
    for a in range(nc):
        terms = [] if gs is None else [int(gs[a][i]) % P]
        v = vr.eval_vanishing_poly(vr.BASE, 1 << log_n, x, w, z[:nc], zn[:nc], z[nc:nc + nc * num_prods], c[sigmas_first:sigmas_first + num_routed],
                                   k_is, betas, gammas, [alphas[a]], qdf, terms)
        out.append(v[0] * zh_inv % P)
    return out


# nc, qdf, num_routed, log_n, rate_bits, grid challenges, host gate sums
QUOTIENT_CASES = [(2, 8, 17, 3, 3, False, True),      # <2, 8>, the streams; a ragged last chunk
                  (2, 8, 9, 4, 3, True, False),       # <2, 8>, challenges from the grid
                  (2, 4, 9, 3, 3, False, True),       # <2, 0>: qbits = rate_bits - 1
                  (1, 8, 11, 3, 3, False, False),     # <1, 0>
                  (3, 4, 7, 5, 3, False, True),       # <3, 0>, 2^5 rows
                  (3, 8, 13, 3, 3, True, True),
                  (2, 8, 9, 3, 3, "sub", False),      # <2, 8> and <3, 0> with the operands of gl::sub's second fold placed
                  (3, 8, 9, 3, 3, "sub", True)]


def _place_sub_second_fold(wires, zs, nc, num_routed, qdf, log_n, rate_bits):
    """With beta_0 = gamma_0 = 0 a chunk's check is prev * prod(wires) - next * prod(wires).  The last chunk of 9 routed wires at
    degree 8 is ONE wire: where it is 1, the last partial product of challenge 0 is 0 and Z_0 of the next row is 2^64 - 1, the
    products leave the multiplier as the raw words 0 and 2^64 - 1 and the kernel computes gl::sub(0, 2^64 - 1) -- a minuend below
    2^32 - 1 under a subtrahend above P, the one way into the second fold of gl::sub.  The first point whose rows can take the three
    words (the columns keep their words, neighbouring rows stay different) is used; returns it."""
    num_prods = vr.num_partial_products(num_routed, qdf)
    assert num_routed % qdf == 1 and num_prods >= 1
    for i in range((1 << log_n) << vr.log2_ceil(qdf)):
        L, Ln = ew.point_rows(i, log_n, rate_bits, vr.log2_ceil(qdf))
        w, z = wires.copy(), zs.copy()
        try:
            ew.place(w, num_routed - 1, L, 1)
            ew.place(z, nc + num_prods - 1, L, 0)
            ew.place(z, 0, Ln, 2**64 - 1)
        except AssertionError:
            continue
        if int(z[nc + num_prods - 1][L]) == 0:      # (the two placements in zs are in different columns: both hold)
            wires[...], zs[...] = w, z
            return i
    raise AssertionError("no point whose rows take the three words")


def _quotient_case(case, canonical):
    nc, qdf, num_routed, log_n, rate_bits, grid_ch, host_gs = case

    def make():
        rng = np.random.default_rng(7300 + 10 * nc + qdf + num_routed)
        N = 1 << (log_n + rate_bits)
        num_prods = vr.num_partial_products(num_routed, qdf)
        assert num_routed % qdf
        wires = ew.edge_matrix(rng, num_routed + 1, N, canonical)
        cs = ew.edge_matrix(rng, 2 + num_routed, N, canonical)
        zs = ew.edge_matrix(rng, nc * (1 + num_prods), N, canonical)
        k_is = _challenges(rng, num_routed, True)
        betas, gammas, alphas = (_challenges(rng, nc, canonical, from_grid=grid_ch is True) for _ in range(3))
        m = (1 << log_n) << vr.log2_ceil(qdf)
        if grid_ch == "sub":
            betas[0] = gammas[0] = 0
            if not canonical:       # (2^64 - 1 is no canonical word: the canonical mode keeps the challenges and places nothing)
                i = _place_sub_second_fold(wires, zs, nc, num_routed, qdf, log_n, rate_bits)
                L, Ln = ew.point_rows(i, log_n, rate_bits, vr.log2_ceil(qdf))
                assert (int(wires[num_routed - 1][L]), int(zs[nc][L]), int(zs[0][Ln])) == (1, 0, 2**64 - 1)
        gs = None
        if host_gs:     # the caller's sums are raw words too: the grid (2^64 - 1 with it), in every mode
            gs = ew.edge_matrix(rng, nc, max(m, len(ew.GRID)), False)[:, :m].copy()
            gs[0][0], gs[nc - 1][m - 1] = 2**64 - 1, 2**64 - 1
        lw, lcs, lzs = (ew.leaves(a, log_n, rate_bits) for a in (wires, cs, zs))
        exp = np.asarray([_quotient_ref_point(i, lw, lcs, lzs, 2, k_is, qdf, betas, gammas, alphas, gs) for i in range(m)], dtype=np.uint64).T
        return dict(wires=wires, cs=cs, zs=zs, k_is=k_is, betas=betas, gammas=gammas, alphas=alphas, gs=gs), np.ascontiguousarray(exp)
    return _once(("quotient",) + case + (canonical,), make)


@pytest.mark.parametrize("case", QUOTIENT_CASES, ids=lambda c: "nc%d_qdf%d_r%d_n%d%s%s" % (c[0], c[1], c[2], c[3], "_sub" if c[5] == "sub" else "_grid" if c[5] else "", "_gs" if c[6] else ""))
def test_quotient_values_on_edge_rows(eng, case):
    """p2hot_quotient_polys with values_out and chunks_out = NULL (the values belong to no polynomial) on wrapped wires,
    constants / sigmas and Zs / partial products"""
    nc, qdf, num_routed, log_n, rate_bits, _, _ = case
    for canonical in MODES:
        inp, exp = _quotient_case(case, canonical)
        keep = []
        b = [ew.wrap(eng, inp[k], log_n, rate_bits) for k in ("wires", "cs", "zs")]
        got = np.zeros(exp.shape, dtype=np.uint64)
        gptrs = None
        if inp["gs"] is not None:
            gs = np.ascontiguousarray(inp["gs"])
            gptrs = (C.c_void_p * nc)(*[gs[c].ctypes.data for c in range(nc)])
        eng.check(eng.lib.p2hot_quotient_polys(eng.ctx, b[0]._h, b[1]._h, 2, b[2]._h, ew.u64p(keep, inp["k_is"]), num_routed, qdf,
                                               ew.u64p(keep, inp["betas"]), ew.u64p(keep, inp["gammas"]), ew.u64p(keep, inp["alphas"]), nc, gptrs,
                                               got.ctypes.data_as(C.c_void_p), None))
        assert (got == exp).all() and exp.all(), canonical


# ------------------------------------------------------------------ c. partial products
def _pp_case(num_routed, degree, log_n, nc, seed):
    def make():
        rng = np.random.default_rng(seed)
        n = 1 << log_n
        wires, sigmas = ew.edge_matrix(rng, num_routed, n, False), ew.edge_matrix(rng, num_routed, n, False)
        k_is = [pow(G, j, P) for j in range(num_routed)]
        betas, gammas = _challenges(rng, nc, True), _challenges(rng, nc, True)
        if nc % 2:      # the single-challenge kernel: beta sigma = (2^32 - 1)(2^32 + 1) = 2^64 - 1 comes out of gl::mul unreduced and
            betas[-1] = 2**32 - 1       # meets a wire above P in gl::add, whose second fold it takes
        defined = lambda b, g: all((int(w) + b * (int(s) % P) + g) % P for wc, sc in zip(wires, sigmas) for w, s in zip(wc, sc))
        if nc >= 2:     # the paired kernel: wire + gamma = 2^64 exactly in gl::add_canon (the first such gamma that zeroes no denominator)
            gammas[0] = next(g for g in (2**64 - int(w) for w in wires[num_routed - 1] if int(w) >= 2**32) if defined(betas[0], g))
        assert max(betas + gammas) < P
        # no zero denominator (that error has its own test): asserted on the reference, before any device call
        for b, g in zip(betas, gammas):
            assert defined(b, g)
        if nc % 2 and num_routed << log_n >= 2048:      # (enough words for the two to meet: a sigma of 2^32 + 1 under a wire above P)
            assert ((sigmas == np.uint64(2**32 + 1)) & (wires > np.uint64(P))).any()
        exp = np.asarray(vr.zs_partial_products_batch(wires, sigmas, k_is, betas, gammas, degree), dtype=np.uint64)
        return dict(wires=wires, sigmas=sigmas, k_is=k_is, betas=betas, gammas=gammas), exp
    return _once(("pp", num_routed, degree, log_n, nc, seed), make)


@pytest.mark.parametrize("num_routed,degree,log_n,nc", [(5, 7, 5, 2), (8, 7, 5, 3), (80, 7, 5, 2), (80, 7, 7, 2), (21, 8, 7, 3), (9, 4, 5, 1)])
def test_partial_products_on_edge_columns(eng, num_routed, degree, log_n, nc):
    """p2hot_partial_products (columns through p2hot_cols_upload: raw words, [P, 2^64) included) and p2hot_partial_products_dev on
    edge wires and sigmas; 2^5 rows are one scan chunk and 2^7 two; degree 7 with 5 (no partial product: the Zs alone, and only
    through the device-pointer entry point, whose checks admit it), 8 and 80 routed wires;
    two challenges run the paired kernel, one and the third of three the single one"""
    from plonky2_amd.fri.oracle import DeviceColumns
    inp, exp = _pp_case(num_routed, degree, log_n, nc, 7400 + num_routed + degree + log_n)
    n, keep = 1 << log_n, []
    assert (exp[:nc, 0] == 1).all() and (inp["wires"] >= np.uint64(P)).any() and (inp["sigmas"] >= np.uint64(P)).any()
    dw, ds = DeviceColumns.upload(inp["wires"], eng), DeviceColumns.upload(inp["sigmas"], eng)
    host = np.zeros(exp.shape, dtype=np.uint64)
    h = C.c_void_p()
    args = (ew.u64p(keep, inp["k_is"]), num_routed, degree, ew.u64p(keep, inp["betas"]), ew.u64p(keep, inp["gammas"]), nc)
    rc = eng.lib.p2hot_partial_products(eng.ctx, dw._h, 0, ds._h, 0, *args, host.ctypes.data_as(C.c_void_p), C.byref(h))
    if degree < num_routed:
        eng.check(rc)
        cols = DeviceColumns(eng, h)
        assert (host == exp).all() and (cols.host() == exp).all()
    else:       # prover.rs:215-218: the host entry point refuses what the reference asserts away; the device-pointer one takes it
        from plonky2_amd import _lib
        assert rc == _lib.EINVAL and not h.value and not host.any() and exp.shape == (nc, n)
    d_w, d_s, out = eng.dev(inp["wires"]), eng.dev(inp["sigmas"]), eng.mem.zeros(*exp.shape)
    eng.check(eng.lib.p2hot_partial_products_dev(eng.ctx, eng.ptr(d_w), n, eng.ptr(d_s), n, args[0], num_routed, log_n, degree, args[3], args[4], nc,
                                                 eng.ptr(out), n))
    assert (eng.host(out) == exp).all()


# ------------------------------------------------------------------ g. the M-forms: an edge proof between two random ones
def _rand(rng, *shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


@pytest.mark.parametrize("nc,degree", [(2, 8), (3, 4)])
def test_partial_products_many_with_an_edge_proof(eng, nc, degree):
    """M = 3: p2hot_partial_products_many reads the wires' COEFFICIENTS (and transforms them), so proof 1's wrapped coefficients are
    edge words and the shared sigma columns are too; every proof equals its p2hot_partial_products call on the same values"""
    from plonky2_amd.fri.oracle import DeviceColumns
    from plonky2_amd.plonk.prover import all_wires_permutation_partial_products, all_wires_permutation_partial_products_many
    rng = np.random.default_rng(7700 + nc)
    log_n, R, M = 5, 21, 3
    n = 1 << log_n
    coeffs = [_rand(rng, R + 2, n), ew.edge_matrix(rng, R + 2, n, False), _rand(rng, R + 2, n)]
    sig = ew.edge_matrix(rng, R, n, False)
    sigmas = DeviceColumns.upload(sig, eng)
    k_is = [pow(G, j, P) for j in range(R)]
    betas, gammas = _rand(rng, M, nc), _rand(rng, M, nc)
    bw = [ew.wrap(eng, np.zeros((R + 2, n << RATE_BITS), dtype=np.uint64), log_n, RATE_BITS, coeffs=c) for c in coeffs]
    vals = []
    for b in bw:
        h = C.c_void_p()
        eng.check(eng.lib.p2hot_batch_subgroup_values(b._h, 0, R, C.byref(h)))
        vals.append(DeviceColumns(eng, h))
    for m in range(M):      # no zero denominator, from the values the calls will read
        v = vals[m].host()
        assert all((int(w) + int(betas[m][c]) * (int(s) % P) + int(gammas[m][c])) % P for c in range(nc) for wc, sc in zip(v, sig) for w, s in zip(wc, sc))
    cols, host = all_wires_permutation_partial_products_many(bw, sigmas, k_is, degree, betas, gammas, want_host=True, engine=eng)
    rows = nc * (-(-R // degree))
    inter = cols.host().reshape(rows, M, n)
    for m in range(M):
        one = all_wires_permutation_partial_products(vals[m], sigmas, k_is, degree, betas[m], gammas[m], eng).host()
        assert one.any() and (host[m] == one).all() and (inter[:, m] == one).all(), m
    exp = np.asarray(vr.zs_partial_products_batch(vals[1].host(), sig, k_is, betas[1], gammas[1], degree), dtype=np.uint64)
    assert (host[1] == exp).all()


@pytest.mark.parametrize("nc,qdf", [(2, 8), (3, 8)])
def test_quotient_many_with_an_edge_proof(eng, nc, qdf):
    """M = 3 through p2hot_quotient_polys_gates_many with values_out (and no chunks: the values belong to no polynomial): the
    recursion gate set and the permutation terms on wrapped matrices, proof 1's wires and Zs edge words, the shared
    constants / sigmas edge words, per-proof challenges and public-input hashes; every proof equals its single call"""
    from plonky2_amd.plonk.prover import GateSet, compute_quotient_polys_gates_many
    rng = np.random.default_rng(7800 + nc)
    log_n, R, M = 3, 17, 3
    N = 1 << (log_n + RATE_BITS)
    gates, ns = trg._recursion_set(qdf)
    sf = ns + tg.NUM_GATE_CONSTS
    num_prods = vr.num_partial_products(R, qdf)
    cs = ew.edge_matrix(rng, sf + R, N, False)
    _selector_columns(cs, gates, ns, rng)
    wires = [_rand(rng, tg.W, N), ew.edge_matrix(rng, tg.W, N, False), _rand(rng, tg.W, N)]
    zs = [_rand(rng, nc * (1 + num_prods), N), ew.edge_matrix(rng, nc * (1 + num_prods), N, False), _rand(rng, nc * (1 + num_prods), N)]
    k_is = [pow(G, j, P) for j in range(R)]
    betas, gammas, alphas = _rand(rng, M, nc), _rand(rng, M, nc), _rand(rng, M, nc)
    gammas[1][0] = 2**64 - next(int(w) for w in wires[1][R - 1] if int(w) >= 2**32)      # wire + gamma = 2^64 exactly (gl::add_canon at nc 2)
    assert gammas[1][0] < P
    pihs =np.asarray([_challenges(rng, 4, True), _challenges(rng, 4, False, from_grid=True), _challenges(rng, 4, True)], dtype=np.uint64)
    bw, bz, bcs = [ew.wrap(eng, w, log_n, RATE_BITS) for w in wires], [ew.wrap(eng, z, log_n, RATE_BITS) for z in zs], ew.wrap(eng, cs, log_n, RATE_BITS)
    gs = GateSet([g.descriptor() for g in gates], ns, 0, (0, 0, 0, 0))
    many = compute_quotient_polys_gates_many(bw, bcs, sf, bz, k_is, qdf, betas, gammas, alphas, gate_set=gs, public_inputs_hashes=pihs,
                                             want_values=True, want_chunks=False, engine=eng)
    assert many.shape == (M, nc, (1 << log_n) << 3)
    keep = []
    for m in range(M):
        one = np.zeros(many.shape[1:], dtype=np.uint64)
        gm = GateSet([g.descriptor() for g in gates], ns, 0, [int(v) for v in pihs[m]])
        eng.check(eng.lib.p2hot_quotient_polys_gates(eng.ctx, bw[m]._h, bcs._h, sf, bz[m]._h, ew.u64p(keep, k_is), R, qdf, ew.u64p(keep, betas[m]),
                                                     ew.u64p(keep, gammas[m]), ew.u64p(keep, alphas[m]), nc, None, gm.ptr, one.ctypes.data_as(C.c_void_p), None))
        assert one.all() and (many[m] == one).all(), m
    # proof 1 against the restatements: the permutation terms with the gate sums behind them
    lw, lcs, lzs = (ew.leaves(a, log_n, RATE_BITS) for a in (wires[1], cs, zs[1]))
    al = [int(v) for v in alphas[1]]
    for i in range(many.shape[2]):
        L, _ = ew.point_rows(i, log_n, RATE_BITS, 3)
        sums = rr.reduced_sums(vr.BASE, gates, ns, 0, lw.row(L), lcs.row(L), [int(v) for v in pihs[1]], al)
        exp = _quotient_ref_point(i, lw, lcs, lzs, sf, k_is, qdf, [int(v) for v in betas[1]], [int(v) for v in gammas[1]], al, [{i: s} for s in sums])
        assert [int(v) for v in many[1][:, i]] == exp, i


# ------------------------------------------------------------------ d. Plonk lookups
def _edge_deltas(rng):
    """thirteen challenge vectors [A, B, Alpha, Delta]: 0, 1 and P - 1 in each of the four positions, the other three random; and
    A = B = Delta = 1, with which the running sums h Delta + (input + B output) are sums of raw words"""
    out = []
    for pos in range(4):
        for v in (0, 1, P - 1):
            d = _challenges(rng, 4, True)
            d[pos] = v
            out.append(d)
    return out + [[1, 1, _challenges(rng, 1, True)[0], 1]]


def _lookup_denominators(wires, rows, deltas, num_routed):
    """every alpha - (input + A output) the reference inverts (lookup_ref.compute_lookup_polys): the looked pairs of the
    LookupTable rows, the looking pairs of the Lookup rows"""
    from tests import lookup_ref as lr
    w = lambda row, col: int(wires[col][row]) % P
    for last_lu, last_lut, first_lut in rows:
        for row in range(last_lu, first_lut + 1):
            slots, stride = (lr.num_lut_slots(num_routed), 3) if row >= last_lut else (lr.num_lu_slots(num_routed), 2)
            for s in range(slots):
                yield (deltas[lr.ALPHA] - w(row, stride * s) - deltas[lr.A] * w(row, stride * s + 1)) % P


@pytest.mark.parametrize("num_routed,lookup_degree,seed", [(12, 3, 7500), (14, 2, 7500), (80, 7, 7500)])
def test_lookup_polys_on_edge_columns(eng, num_routed, lookup_degree, seed):
    """p2hot_lookup_polys (lookup::lookup_rows_kernel and its scans) on edge wire columns through p2hot_cols_upload -- raw words,
    [P, 2^64) included -- with 0, 1 and P - 1 in every position of the challenges; the seeds are such that no denominator of the
    reference vanishes, which is asserted on the reference before the device sees anything"""
    from plonky2_amd.plonk.prover import all_lookup_polys
    from tests import lookup_ref as lr
    from tests import test_lookup as tl
    log_n = 5

    def make():
        rng = np.random.default_rng(seed)
        wires = ew.edge_matrix(rng, num_routed, 1 << log_n, False)
        rows = tl._regions(num_routed, tl._spec_for(num_routed, log_n, adjacent=True))
        # the first LookupTable row the kernel walks (RE above it is still 0): with the vector of ones RE becomes 2^64 - 1 after slot
        # 0 and takes the second fold of gl::add at slot 1
        for col, v in ((0, 2**64 - 1), (1, 0), (3, 2**64 - 1), (4, 0)):
            ew.place(wires, col, rows[0][2], v)
        deltas = _edge_deltas(rng)
        for d in deltas:
            assert all(_lookup_denominators(wires, rows, d, num_routed)), d
        exp = [np.asarray(lr.compute_all_lookup_polys(wires, deltas[k:k + 4], rows, num_routed, lookup_degree + 1), dtype=np.uint64) for k in (0, 4, 8, 12)]
        return (wires, rows, deltas), exp
    (wires, rows, deltas), exp = _once(("lookup polys", num_routed), make)
    assert (wires >= np.uint64(P)).any()
    for k in (0, 4, 8, 12):
        cols, host = all_lookup_polys(wires, rows, deltas[k:k + 4], lr.num_lu_slots(num_routed), lr.num_lut_slots(num_routed), lookup_degree,
                                      want_host=True, engine=eng)
        assert (host == exp[k // 4]).all() and (cols.host() == exp[k // 4]).all() and exp[k // 4].any(), k


@pytest.mark.parametrize("num_routed,qdf,nc", [(12, 4, 2), (14, 3, 3), (80, 8, 2), (20, 3, 1)])
def test_lookup_quotient_terms_on_edge_rows(eng, num_routed, qdf, nc):
    """the lookup terms of p2hot_quotient_polys_lookup (lookup::lookup_terms_kernel in front of the permutation kernel), values_out
    alone, on wrapped edge matrices: wires, constants / lookup selectors / sigmas, Zs / partial products / lookup polynomials.
    Edge challenge vectors (no term divides: every vector is legal), the LUT evaluations handed over as raw words"""
    from tests import lookup_ref as lr
    from tests import test_lookup as tl
    log_n = 3
    for canonical in MODES:
        def make():
            rng = np.random.default_rng(7550 + num_routed + nc)
            N = 1 << (log_n + RATE_BITS)
            lut_slots, lu_slots = lr.num_lut_slots(num_routed), lr.num_lu_slots(num_routed)
            luts = [[(int(a), int(b)) for a, b in rng.integers(0, 1 << 16, size=(t, 2))] for t in (lut_slots + 1, lut_slots - 1)]
            sigmas_first = tl.SEL_FIRST + 4 + len(luts)
            S = lr.div_ceil(lu_slots, qdf - 1)
            num_zpp = nc * (1 + vr.num_partial_products(num_routed, qdf))
            wires = ew.edge_matrix(rng, num_routed + 3, N, canonical)
            cs = ew.edge_matrix(rng, sigmas_first + num_routed, N, canonical)
            zs = ew.edge_matrix(rng, num_zpp + nc * (S + 1), N, canonical)
            k_is = _challenges(rng, num_routed, True)
            betas, gammas, alphas = (_challenges(rng, nc, canonical) for _ in range(3))
            vectors = _edge_deltas(rng)
            first = [12] + [int(k) for k in rng.choice(12, size=nc - 1, replace=False)]      # (the vector of ones first)
            picks = [first]
            if num_routed <= 20:        # the small shapes go on through ALL thirteen vectors, nc at a time (the last call wraps round)
                rest = [k for k in range(13) if k not in first]
                picks += [[rest[(t + c) % len(rest)] for c in range(nc)] for t in range(0, len(rest), nc)]
                assert {k for p in picks for k in p} == set(range(13))
            lw, lcs, lzs = (ew.leaves(a, log_n, RATE_BITS) for a in (wires, cs, zs))
            sets = []
            for pick in picks:
                deltas = [vectors[k] for k in pick]
                evals = [[lr.lut_re_poly_eval(lut, lut_slots, d) for lut in luts] for d in deltas]
                raw_evals = [[e if canonical or e + P >= 1 << 64 else e + P for e in row] for row in evals]
                exp = np.asarray(lr.quotient_values(lw, lcs, lzs, tl.SEL_FIRST, len(luts), sigmas_first, k_is, qdf, betas, gammas, alphas, deltas, luts),
                                 dtype=np.uint64)
                sets.append((deltas, raw_evals, exp))
            return dict(wires=wires, cs=cs, zs=zs, k_is=k_is, betas=betas, gammas=gammas, alphas=alphas, sigmas_first=sigmas_first,
                        lu_slots=lu_slots, lut_slots=lut_slots, num_luts=len(luts)), sets
        q, sets = _once(("lookup terms", num_routed, qdf, nc, canonical), make)
        b, keep = [ew.wrap(eng, q[k], log_n, RATE_BITS) for k in ("wires", "cs", "zs")], []
        for deltas, evals, exp in sets:
            got = np.zeros(exp.shape, dtype=np.uint64)
            eng.check(eng.lib.p2hot_quotient_polys_lookup(
                eng.ctx, b[0]._h, b[1]._h, q["sigmas_first"], b[2]._h, ew.u64p(keep, q["k_is"]), num_routed, qdf, ew.u64p(keep, q["betas"]),
                ew.u64p(keep, q["gammas"]), ew.u64p(keep, q["alphas"]), nc, None, q["lu_slots"], q["lut_slots"], q["num_luts"], tl.SEL_FIRST,
                ew.u64p(keep, deltas), ew.u64p(keep, evals), got.ctypes.data_as(C.c_void_p), None))
            assert got.shape == (nc, (1 << log_n) << vr.log2_ceil(qdf)) and (got == exp).all() and exp.all(), (canonical, deltas)


# ------------------------------------------------------------------ e. STARK lookups and cross-table lookups
STARK_W = 10      # the trace layout of tests/test_stark_lookup.py: table, frequencies, looking columns, three filter columns


@pytest.mark.parametrize("num_looking,cd,nc", [(5, 3, 2), (3, 2, 1), (2, 3, 3)])
def test_stark_lookup_polys_on_edge_traces(eng, num_looking, cd, nc):
    """p2hot_stark_lookup_polys on an edge trace (raw words, [P, 2^64) included): columns with coefficients, constants and next-row
    terms, every kind of filter.  The restatement inverts table + challenge and every looking value + challenge with
    batch_inv, which asserts that none is zero: it runs first, so the seeds are such that the reference stays defined"""
    from plonky2_amd.starky.lookup import lookup_helper_columns
    from tests import stark_lookup_ref as sr
    from tests import test_stark_lookup as tsl

    def make():
        rng = np.random.default_rng(7650 + num_looking + cd)
        trace = ew.edge_matrix(rng, STARK_W, 32, False)
        descs = tsl._parity_lookups(num_looking, STARK_W)
        ch = _challenges(rng, nc, True)
        exp = sr.all_lookup_helper_columns([tsl._ref_lookup(d) for d in descs], [[int(v) for v in col] for col in trace], ch, cd)
        return (trace, descs, ch), np.asarray(exp, dtype=np.uint64)
    (trace, descs, ch), exp = _once(("stark lookup polys", num_looking, cd, nc), make)
    cols, host = lookup_helper_columns(trace, [tsl._lib_lookup(d) for d in descs], ch, cd, want_host=True, engine=eng)
    assert (host == exp).all() and (cols.host() == exp).all() and exp.any() and (trace >= np.uint64(P)).any()


@pytest.mark.parametrize("cd", [2, 3])
def test_stark_ctl_polys_on_edge_traces(eng, cd):
    """p2hot_stark_ctl_polys on an edge trace: Zs of one, two and three looking entries, helpers or none.  As above, the restatement
    (partial_sums: batch_inv of every combined entry) asserts its own denominators before the device sees anything"""
    from plonky2_amd.starky.cross_table_lookup import ctl_polys
    from tests import stark_lookup_ref as sr
    from tests import test_stark_lookup as tsl

    def make():
        rng = np.random.default_rng(7660 + cd)
        trace = ew.edge_matrix(rng, STARK_W, 32, False)
        descs = tsl._ctl_descs(rng, STARK_W)
        zs = sr.ctl_data_for_table([[int(v) for v in col] for col in trace], [tsl._ref_z(d) for d in descs], cd)
        return (trace, descs, [len(z.helper_columns) for z in zs]), np.asarray(sr.get_ctl_auxiliary_polys(zs), dtype=np.uint64)
    (trace, descs, nh), exp = _once(("stark ctl polys", cd), make)
    cols, firsts, host = ctl_polys(trace, [tsl._lib_z(d) for d in descs], cd, want_host=True, engine=eng)
    assert (host == exp).all() and (cols.host() == exp).all() and exp.any()
    assert [int(v) for v in firsts] == [int(exp[sum(nh) + k][0]) for k in range(3)]


@pytest.mark.parametrize("log_n,cd,nc,kind", [(3, 3, 2, "both"), (4, 2, 1, "both"), (3, 3, 1, "lookup"), (3, 2, 2, "ctl")])
def test_stark_quotient_values_on_edge_rows(eng, log_n, cd, nc, kind):
    """stark::lookup / CTL terms of p2hot_stark_quotient_polys, values_out alone, on a wrapped edge trace and a wrapped edge matrix of
    auxiliary columns, with the caller's accumulators (raw words, 2^64 - 1 among them) and without; grid challenges (the
    constraint side divides by nothing).  constraint_degree 3 / 2 at rate 3: a row step of 4 / 8"""
    from tests import stark_lookup_ref as sr
    from tests import test_stark_lookup as tsl
    for canonical in MODES:
        def make():
            rng = np.random.default_rng(7670 + 10 * log_n + cd + nc)
            N = 1 << (log_n + RATE_BITS)
            lookups = [tsl._lookup_desc(3, first=2, table=([(0, 1)], [(1, 5)], 3), freq=([(1, 2)], [(0, 1)], 0), filt_cols=(7, 8, 9))] if kind != "ctl" else []
            zd = tsl._ctl_descs(rng, STARK_W)
            zdescs = [zd[0], zd[2] if cd == 3 else zd[1]] if kind != "lookup" else []
            ref_lookups, ref_zs = [tsl._ref_lookup(d) for d in lookups], [tsl._ref_z(d) for d in zdescs]
            nh = [z.num_helpers(cd) for z in (tsl._lib_z(d) for d in zdescs)]
            width = sum(nc * sr.num_helper_columns(lk, cd) for lk in ref_lookups) + sum(nh) + len(zdescs)
            trace, aux = ew.edge_matrix(rng, STARK_W, N, canonical), ew.edge_matrix(rng, width, N, canonical)
            ch, alphas = _challenges(rng, nc, canonical, from_grid=True), _challenges(rng, nc, canonical, from_grid=True)
            m = (1 << log_n) << vr.log2_ceil(sr.quotient_degree_factor(cd))
            accs = ew.edge_matrix(rng, nc, max(m, len(ew.GRID)), False)[:, :m].copy()
            accs[0][0] = 2**64 - 1
            lt, la = ew.leaves(trace, log_n, RATE_BITS), ew.leaves(aux, log_n, RATE_BITS)
            exp = [np.asarray(sr.quotient_values(lt, la, ref_lookups, ch, ref_zs, nh, alphas, cd, r), dtype=np.uint64) for r in (None, accs)]
            return (trace, aux, lookups, zdescs, nh, ch, alphas, accs), exp
        (trace, aux, lookups, zdescs, nh, ch, alphas, accs), exp = _once(("stark quotient", log_n, cd, nc, kind, canonical), make)
        bt, ba = ew.wrap(eng, trace, log_n, RATE_BITS), ew.wrap(eng, aux, log_n, RATE_BITS)
        for r, want in zip((None, accs), exp):
            _, vals = tsl._values_only(eng, bt, ba, ch, lookups, zdescs, alphas, cd, r, num_helpers=nh if zdescs else None)
            assert vals.shape == want.shape and (vals == want).all() and want.any(), (canonical, r is None)


# ------------------------------------------------------------------ f. the two interpreters: temps that leave [0, P)
BIG_CONST = (1 << 63) + 0x1234567


def _stress(add, sub, mul, leaves, flat, sums, diffs, consume):
    """The body both programs share, over any arithmetic (a builder's traced values, Python ints mod P).  `sums` / `diffs`: operand
    pairs whose raw gl::add / gl::sub results leave [0, P) on grid words (two grid words added; a larger word subtracted); products
    of such temps; then every opcode with such a temp in the first and in the second position against every operand kind (`leaves`)
    and against another temp, all of it folded into one chain acc <- (acc z + r) z' + r' that is hundreds of instructions deep.
    z, z' are the two `flat` operands (a public input, a constant: degree 0), so no value's degree exceeds 3, which the library's
    degree check of a program admits at every factor used here; `consume` takes the chain's value every tenth step and at the end."""
    temps = [add(a, b) for a, b in sums] + [sub(a, b) for a, b in diffs]
    linear = len(temps)
    temps += [mul(temps[0], temps[len(sums)]), mul(temps[len(sums) + 1], temps[1])]
    acc = add(temps[0], temps[-1])
    k = 0
    for op in (add, sub, mul):
        for t in temps:
            for o in leaves + [temps[(k + 3) % linear]]:
                acc = add(mul(add(mul(acc, flat[0]), op(t, o)), flat[1]), op(o, t))
                k += 1
                if k % 10 == 0:
                    consume(k // 10, acc)
    consume(0, acc)
    return k


def edge_air(F, lv, nv, pi, cons):
    """a constraint function in the style of tests/stark_air_ref.py (generic over F): all four constraint opcodes, the operand
    kinds LOCAL, NEXT, PUBLIC, CONST and temp in both positions of ADD, SUB and MUL"""
    K = F.lift(BIG_CONST)
    kinds = [cons.constraint, cons.constraint_transition, cons.constraint_first_row, cons.constraint_last_row]
    steps = _stress(F.add, F.sub, F.mul, [lv[4], nv[4], pi[0], K], [pi[1], K], [(lv[0], lv[1]), (nv[0], pi[0]), (K, lv[5])],
                    [(lv[2], lv[3]), (pi[1], nv[1]), (lv[5], K)], lambda j, v: kinds[j % 4](v))
    assert steps == 3 * 8 * 5


def edge_gate(b):
    """the same body as a gate: wires, GATE_CONST, the public-inputs hash, CONST and temps; every tenth value is a constraint"""
    K = b.constant(BIG_CONST)
    w, c, h = b.wires, b.constants, b.public_inputs_hash
    _stress(lambda x, y: x + y, lambda x, y: x - y, lambda x, y: x * y, [w[4], c[0], h[0], K], [h[3], K], [(w[0], w[1]), (c[1], h[1]), (K, w[5])],
            [(w[2], w[3]), (h[2], c[0]), (w[134], K)], lambda j, v: b.constraint(v))


def _air_program():
    from plonky2_amd.starky.air import AirBuilder
    from tests.test_stark_air import TracedF
    return _once(("air program",), lambda: (lambda b: (edge_air(TracedF, b.local_values, b.next_values, b.public_inputs, b), b.build())[1])(AirBuilder(6, 2)))


def test_the_stress_programs_use_the_whole_format():
    from plonky2_amd.plonk import gate_program as gp
    from plonky2_amd.starky import air
    from tests.test_gate_program import _program
    prog = _air_program()
    assert {i[0] for i in prog.insns} == set(range(7)) and 8 < prog.num_temps <= 32 and len(prog.insns) > 480
    for pos in (2, 3):      # every arithmetic opcode sees every operand kind in either position
        assert {(i[0], i[pos] >> 29) for i in prog.insns if i[0] < air.CONSTRAINT} == {(op, k) for op in (air.ADD, air.SUB, air.MUL)
                                                                                        for k in (air.LOCAL, air.NEXT, air.PUBLIC, air.CONST, air.TEMP)}
    g = _program(edge_gate, 1, 0, (0, 3)).program
    assert {i[0] for i in g.insns} == {air.ADD, air.SUB, air.MUL, air.CONSTRAINT} and sum(i[0] == air.CONSTRAINT for i in g.insns) == 13
    for pos in (2, 3):
        assert {(i[0], i[pos] >> 29) for i in g.insns if i[0] < air.CONSTRAINT} == {(op, k) for op in (air.ADD, air.SUB, air.MUL)
                                                                                     for k in (air.LOCAL, air.PUBLIC, air.CONST, air.TEMP, gp.GATE_CONST)}


@pytest.mark.parametrize("log_n,cd,nc", [(3, 9, 2), (5, 3, 3), (4, 5, 1)])
def test_constraint_program_on_edge_traces(eng, log_n, cd, nc):
    """air::eval_kernel through p2hot_stark_constraint_accs on a wrapped edge trace, raw public inputs and challenges: against
    the independent interpreter of tests/stark_air_ref.py on the built program AND against the constraint function itself on
    Python integers.  constraint_degree 9 / 5 / 3 at rate 3: a row step of 1 / 2 / 4"""
    from tests import stark_air_ref as ar
    prog = _air_program()
    for canonical in MODES:
        def make():
            rng = np.random.default_rng(7500 + log_n + cd)
            trace = ew.edge_matrix(rng, 6, 1 << (log_n + RATE_BITS), canonical)
            # (public inputs: grid words that are not zero -- with pi[1] = 0 the chain forgets itself at every step)
            pub = [v for v in _challenges(rng, 6, canonical, from_grid=True) if v % P][:2]
            alphas = _challenges(rng, nc, canonical, from_grid=nc == 1)
            lde = ew.leaves(trace, log_n, RATE_BITS)
            plain = ar.constraint_accs(edge_air, lde, pub, alphas, cd)
            interpreted = ar.constraint_accs(lambda F, lv, nv, pi, cons: ar.interpret(F, prog.insns, prog.constants, prog.num_temps, lv, nv, pi, cons),
                                             lde, pub, alphas, cd)
            assert plain == interpreted
            return (trace, pub, alphas), np.asarray(plain, dtype=np.uint64)
        (trace, pub, alphas), exp = _once(("air", log_n, cd, nc, canonical), make)
        bt, keep = ew.wrap(eng, trace, log_n, RATE_BITS), []
        got, ps = np.zeros(exp.shape, dtype=np.uint64), prog.struct()
        eng.check(eng.lib.p2hot_stark_constraint_accs(eng.ctx, bt._h, C.byref(ps), ew.u64p(keep, pub), cd, ew.u64p(keep, alphas), nc,
                                                      got.ctypes.data_as(C.c_void_p)))
        assert (got == exp).all() and exp.all(), canonical


@pytest.mark.parametrize("nc", [2, 3])
def test_gate_program_on_edge_rows(eng, nc):
    """gateprog::interp_kernel through p2hot_gate_sums_programs on wrapped edge wires and constants, beside one hand-written gate
    of the same group: against the independent interpreter of tests/gate_program_ref.py plus the restated gate"""
    from plonky2_amd.plonk.prover import GateSet, gate_sums
    from tests import gate_program_ref as gpr
    from tests.test_gate_program import _program
    log_n, qdf = 3, 8
    gates = [gr.Gate(gr.ARITHMETIC, 0, 0, (0, 3), 20)]
    program = _program(edge_gate, 1, 0, (0, 3))
    progs = [(program.program.insns, program.program.constants, program.program.num_temps, 1, 0, (0, 3))]
    for canonical in MODES:
        def make():
            rng = np.random.default_rng(7600 + nc)
            N = 1 << (log_n + RATE_BITS)
            wires, cs = ew.edge_matrix(rng, tg.W, N, canonical), ew.edge_matrix(rng, 4, N, canonical)
            _selector_columns(cs, gates + [gr.Gate(gr.CONSTANT, 1, 0, (0, 3), 2)], 1, rng)      # (row 1 stands for the program)
            if not canonical:       # w0 + w1 = 2 (2^64 - 1) takes the second fold of gl::add, in a row whose filter keeps the program
                ew.meet(wires, [0, 1], 2**64 - 1, ok=lambda L: gr.compute_filter(vr.BASE, 1, (0, 3), int(cs[0][L]) % P, False) != 0)
            pih, alphas = _challenges(rng, 4, canonical, from_grid=True), _challenges(rng, nc, canonical)
            lw, lcs = ew.leaves(wires, log_n, RATE_BITS), ew.leaves(cs, log_n, RATE_BITS)
            exp = np.zeros((nc, N), dtype=np.uint64)
            selected = set()
            for i in range(N):
                L, _ = ew.point_rows(i, log_n, RATE_BITS, 3)
                hand = rr.reduced_sums(vr.BASE, gates, 1, 0, lw.row(L), lcs.row(L), pih, alphas)
                user = gpr.filtered_sums(progs, 1, 0, lw.row(L), lcs.row(L), pih, alphas)
                exp[:, i] = [(a + b) % P for a, b in zip(hand, user)]
                selected.add(gr.compute_filter(vr.BASE, 1, (0, 3), lcs.row(L)[0], False) != 0)
            assert selected == {False, True}
            return (wires, cs, pih, alphas), exp
        (wires, cs, pih, alphas), exp = _once(("gateprog", nc, canonical), make)
        bw, bcs = ew.wrap(eng, wires, log_n, RATE_BITS), ew.wrap(eng, cs, log_n, RATE_BITS)
        got = gate_sums(bw, bcs, 3, GateSet([g.descriptor() for g in gates], 1, 0, pih), qdf, alphas, engine=eng, programs=[program])
        assert (got == exp).all() and exp.any(), canonical


# ------------------------------------------------------------------ h. FRI and opening arithmetic on edge coefficients
RANDOM_POINT = (0x0123456789ABCDEF, 0xFEDCBA9876543210 % P)
POINTS = [(0, 0), (1, 0), (P - 1, 0), (0, 1), (P - 1, P - 1), (2**32 - 1, 2**32), RANDOM_POINT]


def _edge_coeffs(seed, widths, log_n, canonical):
    """coefficient matrices [w][2^log_n] of edge words; above 2^13 a 2^12-row edge matrix repeated (its first and last rows differ)"""
    def make():
        rng = np.random.default_rng(seed)
        rows = 1 << min(log_n, 12)
        out = []
        for w in widths:
            a = ew.edge_matrix(rng, w, rows, canonical)
            for c in range(w if rows < 1 << log_n else 0):
                while a[c][0] == a[c][-1]:
                    a[c] = np.roll(a[c], 1)
            a = np.ascontiguousarray(np.tile(a, (1 << log_n) // rows))
            assert (a[:, 1:] != a[:, :-1]).all()
            out.append(a)
        return out, [a % np.uint64(P) for a in out]
    return _once(("coeffs", seed, tuple(widths), log_n, canonical), make)


def _wrap_coeffs(eng, cols, log_n):
    """the device-pointer flow: the coefficient buffers behind wrapped handles (rate 1, the LDE words are not read; the cap is
    the leaf level, so the tree has no digests)"""
    return [ew.wrap(eng, np.zeros((c.shape[0], 2 << log_n), dtype=np.uint64), log_n, 1, cap_height=log_n + 1, coeffs=c) for c in cols]


def _final_poly_check(eng, ora, log_n, widths, canonical, combos, seed):
    from plonky2_amd.fri.oracle import FriBatchInfo, final_poly_device
    from tests.test_prove_openings import _oracle_final_poly
    cols, reduced = _edge_coeffs(seed, widths, log_n, canonical)
    oracles = _wrap_coeffs(eng, cols, log_n)
    all_polys = [(oi, pi) for oi, w in enumerate(widths) for pi in range(w)]
    for z0, z1, alpha in combos:
        ob = [(z0, all_polys)] + ([(z1, [(0, 0), (0, 1)])] if z1 is not None else [])
        key = ("final", seed, log_n, canonical, z0, z1, alpha)
        # divide_by_linear is a synthetic division and reduce_polys_base a sum: the reference divides by nothing, no point is skipped
        exp = _once(key, lambda: _oracle_final_poly(ora, ob, reduced, np.array(alpha, dtype=np.uint64)))
        got = eng.host(final_poly_device([FriBatchInfo(z, p) for z, p in ob], oracles, alpha, eng))
        assert (got.T == exp).all(), (log_n, z0, z1, alpha)


@pytest.mark.parametrize("log_n,widths", [(6, [2, 1]), (6, [9, 40]), (13, [2, 3]), (17, [2])])
def test_final_poly_on_edge_coefficients(eng, ora, log_n, widths):
    """reduce_polys_base + divide_by_linear + shift / accumulate (p2hot_fri_final_poly_dev) on edge coefficients, points and alpha
    from the edge list.  2^6 and 2^13 coefficients with 3 to 49 polynomials per batch go through reduce_polys_base_small_kernel,
    2^17 (above its switch-over at 2^16 in final_poly_core) through reduce_polys_base_kernel"""
    full = [(POINTS[k], POINTS[(k + 3) % 7], POINTS[(k + 5) % 7]) for k in range(7)]
    combos = full if log_n <= 6 else full[1:7:2] if log_n <= 13 else [(POINTS[4], None, POINTS[5])]
    assert log_n > 6 or {c[i] for c in combos for i in range(3)} == set(POINTS)
    for canonical in MODES if log_n <= 13 else [False]:
        _final_poly_check(eng, ora, log_n, widths, canonical, combos, 7900 + len(widths) + widths[0])


def test_final_poly_two_level_carries_on_edge_coefficients(eng, ora):
    """past the two-level switch of the carry scan, reached as test_final_poly_long_polynomials_two_level_carries reaches it: 2^19
    coefficients on the GPU, a context with a lowered P2HOT_HORNER_2L_MIN on the emulator"""
    import os
    from tests.test_prove_openings import is_gpu
    if is_gpu(eng):
        e, log_n = eng, 19
    else:
        from tests.emu_backend import emu_engine
        old = os.environ.get("P2HOT_HORNER_2L_MIN")
        os.environ["P2HOT_HORNER_2L_MIN"] = "16"
        try:
            e = emu_engine()
        finally:
            if old is None:
                os.environ.pop("P2HOT_HORNER_2L_MIN")
            else:
                os.environ["P2HOT_HORNER_2L_MIN"] = old
        log_n = 12
    _final_poly_check(e, ora, log_n, [2, 1], False, [(POINTS[5], None, POINTS[4])], 7950)


@pytest.mark.parametrize("log_n", [6, 13])
def test_openings_of_edge_coefficients(eng, log_n):
    """p2hot_eval_openings on wrapped handles and p2hot_eval_polys_dev on a pointer table: every polynomial at every edge point;
    2^13 coefficients are two stage-1 segments.  The reference is a Horner evaluation, which divides by nothing: no point skipped"""
    from plonky2_amd.fri.oracle import eval_openings
    from tests import pyref
    for canonical in MODES:
        cols, reduced = _edge_coeffs(7960, [3, 2], log_n, canonical)
        exp = _once(("open", log_n, canonical), lambda: [[[pyref.ext_eval([(int(c), 0) for c in poly], z) for poly in r] for z in POINTS] for r in reduced])
        oracles = _wrap_coeffs(eng, cols, log_n)
        got = eval_openings(oracles, POINTS, eng)
        for oi in range(len(cols)):
            assert [[tuple(int(v) for v in e) for e in row] for row in got[oi]] == exp[oi], (canonical, oi)
        d = oracles[0]._coeffs
        table = eng.dev(np.array([eng.mem.ptr(d) + j * (8 << log_n) for j in range(3)], dtype=np.uint64))
        pts = np.array(POINTS, dtype=np.uint64)
        out = eng.mem.zeros(len(pts) * 3, 2)
        eng.check(eng.lib.p2hot_eval_polys_dev(eng.ctx, eng.ptr(table), 3, log_n, pts.ctypes.data, len(pts), eng.ptr(out)))
        assert [[tuple(int(v) for v in e) for e in row] for row in eng.host(out).reshape(len(pts), 3, 2)] == exp[0], canonical
