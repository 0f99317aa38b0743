"""A STARK's own constraints on the device from a constraint program -- plonky2_amd.starky.air.AirBuilder, p2hot_stark_constraint_accs
and p2hot_stark_quotient_polys_air (air::eval_kernel, csrc/air.hpp) -- against tests/stark_air_ref.py: constraint functions
restated from the reference's text, evaluated point by point with the lookup restatement's ConstraintConsumer, and a plain
interpreter of the program format that shares no code with the builder or the kernel."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import stark_air_ref as ar
from tests import stark_lookup_ref as sr
from tests import vanishing_ref as vr
from tests.conftest import P
from tests.pyref import root_of_unity


def _rand(rng, *shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


def _ints(rng, count):
    return [int(v) for v in _rand(rng, count)]


class TracedF:
    """the field interface of the restated constraint functions over an AirBuilder's values: the same function is traced"""
    zero, one = 0, 1
    lift = staticmethod(lambda a: int(a))
    add = staticmethod(lambda a, b: a + b)
    sub = staticmethod(lambda a, b: a - b)
    mul = staticmethod(lambda a, b: a * b)
    scalar_mul = staticmethod(lambda a, s: a * int(s))


@functools.lru_cache(maxsize=None)
def _program(name):
    from plonky2_amd.starky.air import AirBuilder
    fn, width, npub, _ = ar.AIRS[name]
    b = AirBuilder(width, npub)
    fn(TracedF, b.local_values, b.next_values, b.public_inputs, b)
    return b.build()


def _commit(eng, cols, rate_bits):
    from plonky2_amd.fri.oracle import PolynomialBatch
    return PolynomialBatch.from_values(np.asarray(cols, dtype=np.uint64), rate_bits, False, 0, engine=eng)


def _lde(cols, log_n, rate_bits):
    return vr.Lde(vr.interpolate_columns([[int(v) for v in c] for c in cols]), log_n, rate_bits)


# ------------------------------------------------------------------ 1. the builder (no device)
def test_fibonacci_transcribes_line_for_line():
    """fibonacci_stark.rs:77-98 with the builder's operators; five consumes in the reference's order; the same program as the
    restated function traced through the field interface"""
    from plonky2_amd.starky import air
    b = air.AirBuilder(2, 3)
    local_values, next_values, public_inputs, yield_constr = b.local_values, b.next_values, b.public_inputs, b
    yield_constr.constraint_first_row(local_values[0] - public_inputs[0])
    yield_constr.constraint_first_row(local_values[1] - public_inputs[1])
    yield_constr.constraint_last_row(local_values[1] - public_inputs[2])
    yield_constr.constraint_transition(next_values[0] - local_values[1])
    yield_constr.constraint_transition(next_values[1] - local_values[0] - local_values[1])
    prog = b.build()
    assert [i[0] for i in prog.insns if i[0] >= air.CONSTRAINT] == \
        [air.CONSTRAINT_FIRST_ROW, air.CONSTRAINT_FIRST_ROW, air.CONSTRAINT_LAST_ROW, air.CONSTRAINT_TRANSITION, air.CONSTRAINT_TRANSITION]
    assert b.num_constraints == 5 and prog.num_publics == 3 and prog.constants == [] and prog.num_temps == 1
    assert prog.insns == _program("fibonacci").insns
    assert prog.insns[0] == (air.SUB, 0, air.operand(air.LOCAL, 0), air.operand(air.PUBLIC, 0))
    assert prog.insns[1] == (air.CONSTRAINT_FIRST_ROW, 0, air.operand(air.TEMP, 0), 0)


def test_builder_interns_ints_and_reuses_slots():
    from plonky2_amd.starky import air
    b = air.AirBuilder(1)
    x = b.local_values[0]
    for k in range(200):                      # a dependent chain: every value dies at the next instruction
        x = x * 3 + (k % 2) if k % 3 else 5 - x
    b.constraint(x)
    prog = b.build()
    assert prog.num_temps <= 3 and len(prog.insns) > 200
    assert sorted(prog.constants) == [0, 1, 3, 5]
    # ints on either side, negative ints, a value that nothing consumes, a long-lived value next to short-lived ones
    b = air.AirBuilder(2, 1)
    keep = b.local_values[0] * b.next_values[1]
    dead = keep * 7                          # noqa: F841
    t = -1 + b.public_inputs[0]
    for _ in range(10):
        t = t * t - 2
    b.constraint_transition(t + keep)
    prog = b.build()
    assert prog.constants == [7, P - 1, 2] and prog.num_temps == 2 and len(prog.insns) == 1 + 1 + 20 + 1 + 1
    with pytest.raises(ValueError):
        air.AirBuilder(1).constraint(b.local_values[0])
    with pytest.raises(TypeError):
        b.local_values[0] * 1.5


@pytest.mark.parametrize("name", sorted(ar.AIRS))
def test_built_program_interpreted_equals_the_function(name):
    """random frames over the base field and the extension: the restated interpreter on the built program leaves the consumer
    where the function itself does"""
    rng = np.random.default_rng(len(name))
    fn, width, npub, _ = ar.AIRS[name]
    prog = _program(name)
    assert prog.num_temps <= 4
    for F in (vr.BASE, vr.EXT):
        draw = (lambda: int(_rand(rng, 1)[0])) if F is vr.BASE else (lambda: tuple(_ints(rng, 2)))
        for _ in range(4):
            lv, nv, pi = [draw() for _ in range(width)], [draw() for _ in range(width)], [F.lift(v) for v in _ints(rng, npub)]
            sel = [draw() for _ in range(3)]
            alphas = _ints(rng, 2)
            a, b = sr.ConstraintConsumer(F, alphas, *sel), sr.ConstraintConsumer(F, alphas, *sel)
            fn(F, lv, nv, pi, a)
            ar.interpret(F, prog.insns, prog.constants, prog.num_temps, lv, nv, pi, b)
            assert a.accs == b.accs and a.terms == b.terms and len(a.terms) >= 5


def test_mixed_air_uses_the_whole_format_and_accepts_its_trace():
    from plonky2_amd.starky import air
    prog = _program("mixed")
    ops = {i[0] for i in prog.insns}
    assert ops == set(range(7))
    kinds = {o >> 29 for i in prog.insns for o in ((i[2], i[3]) if i[0] < air.CONSTRAINT else (i[2],))}
    assert kinds == {air.LOCAL, air.NEXT, air.PUBLIC, air.CONST, air.TEMP}
    assert max(prog.constants) >= 1 << 63
    n = 8
    trace, pub = ar.mixed_trace(n, 5, 77)
    for i in range(n):
        cons = sr.ConstraintConsumer(vr.BASE, [3], 0 if i == n - 1 else 1, int(i == 0), int(i == n - 1))
        ar.mixed(vr.BASE, [c[i] for c in trace], [c[(i + 1) % n] for c in trace], pub, cons)
        assert not any(cons.terms), i


# ------------------------------------------------------------------ 2. the accumulators, point by point
SHAPES = [(3, 2, 1), (4, 3, 1), (4, 3, 2), (8, 2, 1), (4, 4, 2)]  # log_n, constraint_degree, rate_bits
ACC_CASES = [(s, nc, "mixed" if s[1] >= 3 else "mixed2") for s in SHAPES for nc in (1, 2)] + \
    [((4, 3, 1), 3, "mixed"), ((4, 4, 2), 4, "mixed"), ((3, 2, 1), 2, "fibonacci"), ((8, 2, 1), 4, "fibonacci"), ((8, 3, 1), 2, "mixed")]


@functools.lru_cache(maxsize=None)
def _acc_case(shape, nc, name):
    log_n, cd, rate_bits = shape
    rng = np.random.default_rng(log_n * 1000 + cd * 100 + rate_bits * 10 + nc + len(name))
    fn, width, npub, _ = ar.AIRS[name]
    trace = _rand(rng, width, 1 << log_n)
    pub, alphas = _ints(rng, npub), _ints(rng, nc)
    want = np.asarray(ar.constraint_accs(fn, _lde(trace, log_n, rate_bits), pub, alphas, cd), dtype=np.uint64)
    return trace, pub, alphas, want


@pytest.mark.parametrize("shape,nc,name", ACC_CASES)
def test_constraint_accs_vs_restatement(eng, shape, nc, name):
    """a random trace (nothing is divided or trimmed here): qbits 0, 1 (with a step of 1 and of 2) and 2; every NC instantiation.
    2^8 rows at constraint_degree 2 are 256 points, one workgroup of 256 lanes exactly; at constraint_degree 3 they are 512, two
    workgroups, and the next row of the last points wraps to the first"""
    from plonky2_amd.starky.prover import constraint_accs
    log_n, cd, rate_bits = shape
    trace, pub, alphas, want = _acc_case(shape, nc, name)
    got = constraint_accs(_commit(eng, trace, rate_bits), _program(name), pub, alphas, cd, engine=eng)
    assert got.shape == want.shape == (nc, (1 << log_n) << vr.log2_ceil(sr.quotient_degree_factor(cd))) and want.any()
    assert (got == want).all()


def test_constants_and_public_inputs_are_reduced(eng):
    """a constant and a public input given as representatives in [P, 2^64) count as their residues"""
    from plonky2_amd.starky import air
    from plonky2_amd.starky.prover import constraint_accs
    rng = np.random.default_rng(12)
    trace = _rand(rng, 1, 8)
    bt = _commit(eng, trace, 1)

    def prog(c):
        return air.Program([(air.MUL, 0, air.operand(air.LOCAL, 0), air.operand(air.CONST, 0)), (air.ADD, 0, air.operand(air.TEMP, 0), air.operand(air.PUBLIC, 0)),
                            (air.CONSTRAINT, 0, air.operand(air.TEMP, 0), 0)], [c], 1, 1, 1)
    a = constraint_accs(bt, prog(5), [9], [3], 2, engine=eng)
    ps, pub, al, out = prog(P + 5).struct(), np.asarray([P + 9], dtype=np.uint64), np.asarray([3], dtype=np.uint64), np.zeros((1, 8), dtype=np.uint64)
    assert eng.lib.p2hot_stark_constraint_accs(eng.ctx, bt._h, C.byref(ps), pub.ctypes.data_as(C.c_void_p), 2, al.ctypes.data_as(C.c_void_p), 1,
                                               out.ctypes.data_as(C.c_void_p)) == 0
    assert (a == out).all() and a.any() and (a < P).all()


# ------------------------------------------------------------------ 3. the fused call equals the two steps
# the descriptor shapes of tests/test_stark_lookup.py, restated: a column is (lin, nxt, const), a filter None or (products, constants)
def _single(c):
    return ([(c, 1)], [], 0)


def _lookup_desc():
    fa, fb, fc = 7, 8, 9
    cols = [_single(2), ([(3, 3)], [], 5), ([], [(4, 1)], 0)]
    filters = [None, ([], [_single(fa)]), ([(_single(fb), ([(fc, 2)], [], 1))], [_single(fa), ([], [(fb, 1)], 0)])]
    return {"columns": cols, "filters": filters, "table": ([(0, 1)], [(1, 5)], 3), "freq": ([(1, 2)], [(0, 1)], 0)}


def _ctl_descs(rng):
    e1 = [_single(0)]
    e3 = [([(1, 3)], [], 5), ([], [(2, 1)], 0), ([(3, 7)], [(4, 2)], 1)]
    f_single = ([], [_single(9)])
    f_prod = ([(_single(8), ([(7, 2)], [], 1))], [_single(9), ([], [(8, 1)], 0)])
    b, g = _ints(rng, 2), _ints(rng, 2)
    return [{"columns": [e3], "filters": [f_prod], "beta": b[0], "gamma": g[0]},
            {"columns": [e1, e1], "filters": [None, f_single], "beta": b[1], "gamma": g[1]}]


def _objects(mod_col, mod_filter, default_filter):
    col = lambda c: mod_col(*c)  # noqa: E731
    flt = lambda f: default_filter() if f is None else mod_filter([(col(a), col(b)) for a, b in f[0]], [col(c) for c in f[1]])  # noqa: E731
    return col, flt


def _ref_objects(ldesc, zdescs):
    col, flt = _objects(sr.Column, sr.Filter, sr.default_filter)
    lookups = [sr.Lookup([col(c) for c in d["columns"]], col(d["table"]), col(d["freq"]), [flt(f) for f in d["filters"]]) for d in ldesc]
    zs = [sr.CtlZ([[col(c) for c in cols] for cols in z["columns"]], [flt(f) for f in z["filters"]], z["beta"], z["gamma"]) for z in zdescs]
    return lookups, zs


def _lib_objects(ldesc, zdescs):
    from plonky2_amd.starky.cross_table_lookup import CtlZData
    from plonky2_amd.starky.lookup import Column, Filter, GrandProductChallenge, Lookup
    col, flt = _objects(Column, Filter, Filter)
    lookups = [Lookup([col(c) for c in d["columns"]], col(d["table"]), col(d["freq"]), [flt(f) for f in d["filters"]]) for d in ldesc]
    zs = [CtlZData(GrandProductChallenge(z["beta"], z["gamma"]), [[col(c) for c in cols] for cols in z["columns"]], [flt(f) for f in z["filters"]])
          for z in zdescs]
    return lookups, zs


@functools.lru_cache(maxsize=None)
def _fused_case(with_aux):
    rng = np.random.default_rng(31 + with_aux)
    log_n, cd, rate_bits, nc, W = 4, 3, 1, 2, 10
    trace = [[int(v) for v in c] for c in _rand(rng, W, 1 << log_n)]
    ldesc, zdescs = ([_lookup_desc()], _ctl_descs(rng)) if with_aux else ([], [])
    ch, alphas, pub = _ints(rng, nc), _ints(rng, nc), _ints(rng, ar.MIXED_PUBLIC_INPUTS)
    ref_lookups, ref_zs = _ref_objects(ldesc, zdescs)
    zs = sr.ctl_data_for_table(trace, ref_zs, cd)
    nh = [len(z.helper_columns) for z in zs]
    aux = sr.all_lookup_helper_columns(ref_lookups, trace, ch, cd) + sr.get_ctl_auxiliary_polys(zs)
    t_lde = _lde(trace, log_n, rate_bits)
    accs = ar.constraint_accs(ar.mixed, t_lde, pub, alphas, cd)
    vals = sr.quotient_values(t_lde, _lde(aux, log_n, rate_bits) if aux else None, ref_lookups, ch, zs, nh, alphas, cd, accs)
    return (log_n, cd, rate_bits), trace, aux, ldesc, zdescs, ch, alphas, pub, np.asarray(accs, dtype=np.uint64), np.asarray(vals, dtype=np.uint64)


@pytest.mark.parametrize("with_aux", [False, True], ids=["alone", "lookup+ctl"])
def test_fused_equals_two_steps(eng, with_aux):
    """p2hot_stark_quotient_polys_air = p2hot_stark_constraint_accs, then p2hot_stark_quotient_polys with those accumulators: the
    values and the chunks, bit for bit; both are the restated quotient.  Alone: aux = NULL, K = 0, the 1 / Z_H is still applied"""
    from plonky2_amd.starky.prover import compute_quotient_polys, constraint_accs
    (log_n, cd, rate_bits), trace, aux, ldesc, zdescs, ch, alphas, pub, accs_want, vals_want = _fused_case(with_aux)
    lookups, zs = _lib_objects(ldesc, zdescs)
    bt, ba = _commit(eng, trace, rate_bits), _commit(eng, aux, rate_bits) if aux else None
    prog = _program("mixed")
    accs = constraint_accs(bt, prog, pub, alphas, cd, engine=eng)
    assert (accs == accs_want).all()
    c2, v2 = compute_quotient_polys(bt, ba, ch, lookups, zs, alphas, cd, constraint_accs=accs, want_values=True, engine=eng)
    c1, v1 = compute_quotient_polys(bt, ba, ch, lookups, zs, alphas, cd, air=prog, public_inputs=pub, want_values=True, engine=eng)
    assert v1.tobytes() == v2.tobytes() and c1.host().tobytes() == c2.host().tobytes()
    assert (v1 == vals_want).all() and vals_want.any()
    assert (c1.host() == np.asarray(vr.quotient_chunks([[int(v) for v in r] for r in vals_want], log_n, 2), dtype=np.uint64)).all()
    c0, v0 = compute_quotient_polys(bt, ba, ch, lookups, zs, alphas, cd, want_values=True, engine=eng)
    assert (v0 != v1).any()
    with pytest.raises(ValueError):
        compute_quotient_polys(bt, ba, ch, lookups, zs, alphas, cd, constraint_accs=accs, air=prog, public_inputs=pub, engine=eng)
    with pytest.raises(ValueError):
        compute_quotient_polys(bt, ba, ch, lookups, zs, alphas, cd, air=prog, public_inputs=pub[:1], engine=eng)


# ------------------------------------------------------------------ 4. FibonacciStark end to end
def _pairs(a):
    return [(int(v[0]), int(v[1])) for v in a]


@functools.lru_cache(maxsize=None)
def _fibonacci_case(log_n):
    rng = np.random.default_rng(40 + log_n)
    trace, pub = ar.fibonacci_trace(1 << log_n, *_ints(rng, 2))
    alphas = _ints(rng, 2)
    accs = ar.constraint_accs(ar.fibonacci, _lde(trace, log_n, 1), pub, alphas, 2)
    vals = sr.quotient_values(_lde(trace, log_n, 1), None, [], [], [], [], alphas, 2, accs)
    return trace, pub, alphas, np.asarray(vr.quotient_chunks(vals, log_n, 1), dtype=np.uint64)


@pytest.mark.parametrize("log_n", [3, 8])
def test_fibonacci_end_to_end(eng, log_n):
    """the reference's trace and public inputs [x0, x1, res], rate 1/2, constraint_degree 2, two challenges, no lookups and no
    CTLs: the chunks are the restated quotient's; committed, they satisfy vanishing(zeta) = Z_H(zeta) reduce_with_powers(chunks(zeta),
    zeta^n) (verifier.rs:167-186) at an extension point with the constraints evaluated there by the restatement -- and with
    another `res` they do not; an empty program is the call without accumulators"""
    from plonky2_amd.fri.oracle import PolynomialBatch, eval_openings
    from plonky2_amd.starky.air import Program
    from plonky2_amd.starky.prover import compute_quotient_polys
    trace, pub, alphas, want = _fibonacci_case(log_n)
    n, nc, cd, rate_bits = 1 << log_n, 2, 2, 1
    bt = _commit(eng, trace, rate_bits)
    chunks = compute_quotient_polys(bt, None, None, [], None, alphas, cd, air=_program("fibonacci"), public_inputs=pub, engine=eng)
    assert chunks.width == nc and (chunks.host() == want).all() and want.any()
    bq = PolynomialBatch.from_coeffs(chunks, rate_bits, False, 0, engine=eng)
    rng = np.random.default_rng(41)
    zeta = (int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(1, P, dtype=np.uint64)))
    gz = vr.EXT.scalar_mul(zeta, root_of_unity(log_n))
    t_z, q_z = [_pairs(e[0]) for e in eval_openings([bt, bq], [zeta], eng)]
    t_gz, = [_pairs(e[0]) for e in eval_openings([bt], [gz], eng)]
    l0, ll = sr.eval_l_0_and_l_last(vr.EXT, log_n, zeta)
    z_last = vr.EXT.sub(zeta, vr.EXT.lift(pow(root_of_unity(log_n), P - 2, P)))

    def vanishing(publics):
        cons = sr.ConstraintConsumer(vr.EXT, alphas, z_last, l0, ll)
        ar.fibonacci(vr.EXT, t_z, t_gz, [vr.EXT.lift(p) for p in publics], cons)
        return cons.accs
    assert vr.verifier_check(vr.EXT, zeta, n, vanishing(pub), q_z, 1) == [True] * nc
    assert vr.verifier_check(vr.EXT, zeta, n, vanishing(pub[:2] + [(pub[2] + 1) % P]), q_z, 1) == [False] * nc
    # UnconstrainedStark: no instructions.  (A random residual-free quotient of a STARK without constraints is zero.)
    empty = Program([], [], 0, 0, 2)
    _, v_empty = compute_quotient_polys(bt, None, None, [], None, alphas, cd, air=empty, public_inputs=[], want_values=True, engine=eng)
    _, v_null = compute_quotient_polys(bt, None, None, [], None, alphas, cd, want_values=True, engine=eng)
    assert v_empty.tobytes() == v_null.tobytes()
    from plonky2_amd.starky.prover import constraint_accs
    assert not constraint_accs(bt, empty, [], alphas, cd, engine=eng).any()


def test_empty_program_with_lookups_equals_null_accs(eng):
    from plonky2_amd.starky.air import Program
    from plonky2_amd.starky.prover import compute_quotient_polys
    (log_n, cd, rate_bits), trace, aux, ldesc, zdescs, ch, alphas, pub, _, _ = _fused_case(True)
    lookups, zs = _lib_objects(ldesc, zdescs)
    bt, ba = _commit(eng, trace, rate_bits), _commit(eng, aux, rate_bits)
    c1, v1 = compute_quotient_polys(bt, ba, ch, lookups, zs, alphas, cd, air=Program([], [], 0, 0, 10), want_values=True, engine=eng)
    c0, v0 = compute_quotient_polys(bt, ba, ch, lookups, zs, alphas, cd, want_values=True, engine=eng)
    assert v1.tobytes() == v0.tobytes() and c1.host().tobytes() == c0.host().tobytes() and v0.any()


# ------------------------------------------------------------------ 5. divisibility
@functools.lru_cache(maxsize=None)
def _divisibility_case():
    rng = np.random.default_rng(55)
    log_n, cd, rate_bits = 4, 4, 2
    trace, pub = ar.mixed_trace(1 << log_n, *_ints(rng, 2))
    alphas = _ints(rng, 2)
    t_lde = _lde(trace, log_n, rate_bits)
    vals = sr.quotient_values(t_lde, None, [], [], [], [], alphas, cd, ar.constraint_accs(ar.mixed, t_lde, pub, alphas, cd))
    return log_n, cd, rate_bits, trace, pub, alphas, np.asarray(vr.quotient_chunks(vals, log_n, 3), dtype=np.uint64)


def test_quotient_divisibility(eng):
    """constraint_degree 4 at rate 1/4: qdf 3 on the coset of 4 n, so a quarter of the coefficients is trimmed and must be zero.
    The satisfying trace returns the restated chunks; one changed cell is "Quotient has failed" """
    from plonky2_amd.starky.prover import compute_quotient_polys
    log_n, cd, rate_bits, trace, pub, alphas, want = _divisibility_case()
    prog = _program("mixed")
    chunks = compute_quotient_polys(_commit(eng, trace, rate_bits), None, None, [], None, alphas, cd, air=prog, public_inputs=pub, engine=eng).host()
    assert chunks.shape == (2 * 3, 1 << log_n) and (chunks == want).all() and want[1].any() and want[4].any()
    bad = [list(c) for c in trace]
    bad[2][5] = (bad[2][5] + 1) % P
    with pytest.raises(ValueError, match="Quotient has failed"):
        compute_quotient_polys(_commit(eng, bad, rate_bits), None, None, [], None, alphas, cd, air=prog, public_inputs=pub, engine=eng)
    assert eng.lib.p2hot_ctx_trim(eng.ctx) == 0


# ------------------------------------------------------------------ 6. the temp cap
def _wide_program(live):
    """`live` values alive at once (local + k, k < live), then their sum"""
    from plonky2_amd.starky.air import AirBuilder
    b = AirBuilder(1)
    vals = [b.local_values[0] + (k + 1) for k in range(live)]
    s = vals[0]
    for v in vals[1:]:
        s = s + v
    b.constraint(s)
    return b.build()


def test_temp_cap(eng):
    from plonky2_amd import _lib
    from plonky2_amd.starky.prover import constraint_accs
    cap = eng.lib.p2hot_air_max_temps()
    assert cap >= 32
    rng = np.random.default_rng(61)
    log_n, rate_bits = 4, 1
    trace = _rand(rng, 1, 1 << log_n)
    bt = _commit(eng, trace, rate_bits)
    alphas = _ints(rng, 2)
    prog = _wide_program(cap)
    assert prog.num_temps == cap
    got = constraint_accs(bt, prog, [], alphas, 2, engine=eng)
    lde = _lde(trace, log_n, rate_bits)

    def interpreted(F, lv, nv, pi, cons):
        ar.interpret(F, prog.insns, prog.constants, prog.num_temps, lv, nv, pi, cons)
    want = np.asarray(ar.constraint_accs(interpreted, lde, [], alphas, 2), dtype=np.uint64)
    assert (got == want).all() and want.any()
    # cap * local + cap (cap + 1) / 2, under the alpha-free single consume
    assert int(want[0][0]) == (cap * vr.get_lde_values(lde, 0, 2)[0] + cap * (cap + 1) // 2) % P
    over = _wide_program(cap + 1)
    assert over.num_temps == cap + 1
    with pytest.raises(_lib.P2HotError) as e:
        constraint_accs(bt, over, [], alphas, 2, engine=eng)
    assert e.value.code == _lib.EUNSUPPORTED


# ------------------------------------------------------------------ 7. errors
def _live_allocs(eng):
    """the emulated runtime counts live allocations; on the GPU the accounting is the trim's return code alone"""
    assert eng.lib.p2hot_ctx_trim(eng.ctx) == 0
    if not eng.lib.p2hot_is_emulated():
        return None
    eng.lib.p2hot_emu_fault.argtypes = [C.c_char_p, C.c_int]
    eng.lib.p2hot_emu_fault.restype = C.c_int
    return eng.lib.p2hot_emu_fault(b"live_allocs", 0)


def test_errors_leave_nothing_allocated(eng):
    from plonky2_amd import _lib
    from plonky2_amd.fri.oracle import PolynomialBatch
    from plonky2_amd.hash.keccak import KeccakHash
    from plonky2_amd.starky import air
    rng = np.random.default_rng(71)
    log_n, W, rate_bits, cd, nc = 4, 3, 1, 3, 2
    trace = _rand(rng, W, 1 << log_n)
    bt, bt_rate0 = _commit(eng, trace, rate_bits), _commit(eng, trace, 0)
    alphas = np.asarray(_ints(rng, 4), dtype=np.uint64)
    pub = np.asarray(_ints(rng, 2), dtype=np.uint64)
    L, N, PUB, CST, T = (lambda i, k=k: air.operand(k, i) for k in range(5))
    good = [(air.MUL, 0, L(0), N(1)), (air.ADD, 1, T(0), CST(0)), (air.SUB, 0, T(1), PUB(1)), (air.CONSTRAINT_TRANSITION, 0, T(0), 0),
            (air.CONSTRAINT_FIRST_ROW, 0, L(2), 0)]
    keep = []

    def call(which, insns=good, constants=(7,), num_temps=2, num_publics=2, publics=pub, cd=cd, nc=nc, tr=bt, null_insns=False, null_constants=False):
        prog = air.Program(insns, constants, num_temps, num_publics, W)
        ps = prog.struct()
        if null_insns:
            ps.insns = None
        if null_constants:
            ps.constants = None
        keep.extend([prog, ps])
        pp = publics.ctypes.data_as(C.c_void_p) if publics is not None else None
        m = (1 << log_n) << vr.log2_ceil(sr.quotient_degree_factor(cd))
        out = np.zeros((max(nc, 1), m), dtype=np.uint64)
        if which == "accs":
            return eng.lib.p2hot_stark_constraint_accs(eng.ctx, tr._h, C.byref(ps), pp, cd, alphas.ctypes.data_as(C.c_void_p), nc, out.ctypes.data_as(C.c_void_p))
        h = C.c_void_p()
        rc = eng.lib.p2hot_stark_quotient_polys_air(eng.ctx, tr._h, None, None, None, 0, None, None, 0, None, cd, alphas.ctypes.data_as(C.c_void_p), nc,
                                                    C.byref(ps), pp, out.ctypes.data_as(C.c_void_p), C.byref(h))
        if rc == _lib.OK:
            eng.lib.p2hot_cols_free(h)
        else:
            assert not h.value and eng.lib.p2hot_last_error(eng.ctx)
        return rc
    both = ("accs", "quotient")
    for which in both:
        assert call(which) == _lib.OK, eng.lib.p2hot_last_error(eng.ctx)
    base = _live_allocs(eng)

    def patched(k, insn):
        return good[:k] + [insn] + good[k + 1:]
    einval = {
        "operand kind": dict(insns=patched(0, (air.MUL, 0, air.operand(5, 0), N(1)))),
        "operand kind b": dict(insns=patched(0, (air.MUL, 0, L(0), air.operand(7, 0)))),
        "local column": dict(insns=patched(0, (air.MUL, 0, L(W), N(1)))),
        "next column": dict(insns=patched(0, (air.MUL, 0, L(0), N(W)))),
        "consumed column": dict(insns=patched(4, (air.CONSTRAINT_FIRST_ROW, 0, L(W), 0))),
        "public index": dict(insns=patched(2, (air.SUB, 0, T(1), PUB(2)))),
        "constant index": dict(insns=patched(1, (air.ADD, 1, T(0), CST(1)))),
        "temp index": dict(insns=patched(1, (air.ADD, 1, T(2), CST(0)))),
        "dst index": dict(insns=patched(1, (air.ADD, 2, T(0), CST(0)))),
        "temp read before written": dict(insns=patched(0, (air.MUL, 0, T(1), N(1)))),
        "null insns": dict(null_insns=True),
        "null constants": dict(null_constants=True),
        "null public inputs": dict(publics=None),
        # MUL of two degree-2 values is degree 4 > 3; a degree-3 product under the first-row filter too
        "degree": dict(insns=[(air.MUL, 0, L(0), N(1)), (air.MUL, 1, T(0), T(0)), (air.CONSTRAINT, 0, T(1), 0)]),
        "degree with a row filter": dict(insns=[(air.MUL, 0, L(0), N(1)), (air.MUL, 1, T(0), L(2)), (air.CONSTRAINT_LAST_ROW, 0, T(1), 0)]),
        "degree at constraint_degree 2": dict(cd=2, insns=[(air.MUL, 0, L(0), N(1)), (air.CONSTRAINT_FIRST_ROW, 0, T(0), 0)]),
        "constraint_degree 1": dict(cd=1),
        "no challenge": dict(nc=0),
        "five challenges": dict(nc=5),
        "rate": dict(tr=bt_rate0),
    }
    for which in both:
        for why, kw in einval.items():
            assert call(which, **kw) == _lib.EINVAL, (which, why)
    # z_last adds nothing: a degree-3 product is a transition constraint at constraint_degree 3
    assert call("accs", insns=[(air.MUL, 0, L(0), N(1)), (air.MUL, 1, T(0), L(2)), (air.CONSTRAINT_TRANSITION, 0, T(1), 0)]) == _lib.OK
    unsupported = {
        "op": dict(insns=patched(0, (7, 0, L(0), N(1)))),
        "temps": dict(num_temps=eng.lib.p2hot_air_max_temps() + 1),
    }
    bk = PolynomialBatch.from_values(trace, rate_bits, False, 0, engine=eng, hasher=KeccakHash(25))
    unsupported["keccak"] = dict(tr=bk)
    for which in both:
        for why, kw in unsupported.items():
            assert call(which, **kw) == _lib.EUNSUPPORTED, (which, why)
    del bk, unsupported
    assert _live_allocs(eng) == base
    for which in both:
        assert call(which) == _lib.OK
