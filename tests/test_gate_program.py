"""User-defined gates' constraints on the device from gate programs -- p2hot_gate_sums_programs, p2hot_quotient_polys_gate_programs,
p2hot_quotient_polys_lookup_gate_programs (gateprog::interp_kernel of csrc/gate_program.hpp between the gate kernels and the lookup
/ permutation kernels) and their Python mirror plonky2_amd/plonk/gate_program.py -- against tests/gate_program_ref.py: an
interpreter of the format over Python ints that shares no code with the builder, nine reference gates transcribed for the builder
(each must equal the hand-written kind of the library AND the restatement of tests/gates_ref.py bit for bit), and a gate the
library does not know, written once for the builder and once as a plain function.

Shapes are tests/test_gates.py's, and so are the helpers: 135 wires (80 routed), two gate constants, rate_bits 3, quotient degree
factor 8; 2^4 rows (128 points: one partly filled workgroup) and 2^6 rows (512 points: two workgroups)."""
import ctypes as C

import numpy as np
import pytest

from tests import gate_program_ref as gpr
from tests import gates_ref as gr
from tests import test_gates as tg
from tests import test_recursion_gates as trg
from tests import vanishing_ref as vr
from tests.conftest import P

W, NUM_ROUTED, RATE_BITS, QDF, NUM_GATE_CONSTS = tg.W, tg.NUM_ROUTED, tg.RATE_BITS, tg.QDF, tg.NUM_GATE_CONSTS


def _builder(fn, num_wires=W, num_constants=NUM_GATE_CONSTS):
    from plonky2_amd.plonk.gate_program import GateBuilder
    b = GateBuilder(num_wires, num_constants)
    fn(b)
    return b


def _program(fn, row, selector_index, group, num_wires=W, num_constants=NUM_GATE_CONSTS):
    from plonky2_amd.plonk.gate_program import GateProgram
    return GateProgram(_builder(fn, num_wires, num_constants), row, selector_index, group)


def _as_program(fn, g, **kw):
    """the transcription `fn` in the place of the descriptor g"""
    return _program(fn, g.row, g.selector_index, g.group, **kw)


def _wide_gate(live):
    """`live` products, all computed before the first is consumed: a program of exactly `live` temp slots, degree 2"""
    def fn(b):
        t = [b.wires[k] * b.wires[k + 1] for k in range(live)]
        s = t[0]
        for v in t[1:]:
            s = s + v
        b.constraint(s - b.constants[1])
    return fn


def _ref_program_sums(q, ldes, programs, alphas=None):
    """the independent interpreter at every point of the quotient coset: [len(alphas)][n << qbits]"""
    qbits = vr.log2_ceil(q["qdf"])
    m = q["n"] << qbits
    alphas = q["alphas"] if alphas is None else alphas
    progs = [(p.program.insns, p.program.constants, p.program.num_temps, p.row, p.selector_index, p.group) for p in programs]
    out = np.zeros((len(alphas), m), dtype=np.uint64)
    for i in range(m):
        (li, step), _ = vr.quotient_rows(i, q["log_n"], ldes["wires"].rate_bits, qbits)
        out[:, i] = gpr.filtered_sums(progs, q["ns"], q["nls"], vr.get_lde_values(ldes["wires"], li, step),
                                      vr.get_lde_values(ldes["cs"], li, step), q["pih"], alphas)
    return out


def _add(a, b):
    return ((a.astype(object) + b.astype(object)) % P).astype(np.uint64)


def _device_sums(eng, q, b, nc, gates, programs, pih=None):
    from plonky2_amd.plonk.prover import gate_sums
    return gate_sums(b["wires"], b["cs"], q["sigmas_first"], tg._gate_set(q, gates, pih), q["qdf"], q["alphas"][:nc], engine=eng, programs=programs)


# ------------------------------------------------------------------ the builder and the interpreter on their own
def test_builder_assigns_slots_by_last_use_and_drops_dead_results():
    from plonky2_amd.plonk import gate_program as gp
    from plonky2_amd.starky import air
    b = gp.GateBuilder(6, 2)
    t0 = b.wires[0] * b.wires[1]
    b.wires[3] * b.wires[4]                              # never reaches a constraint
    t1 = t0 + b.constants[1]
    t2 = t1 - b.public_inputs_hash[3]
    b.constraint(t2 * 5)
    b.constraint(b.wires[5])
    prog = b.build()
    L, PUB, CST, T, GC = (lambda i, k=k: air.operand(k, i) for k in (air.LOCAL, air.PUBLIC, air.CONST, air.TEMP, gp.GATE_CONST))
    assert prog.insns == [(air.MUL, 0, L(0), L(1)), (air.ADD, 0, T(0), GC(1)), (air.SUB, 0, T(0), PUB(3)), (air.MUL, 0, T(0), CST(0)),
                          (air.CONSTRAINT, 0, T(0), 0), (air.CONSTRAINT, 0, L(5), 0)]
    assert prog.constants == [5] and prog.num_temps == 1 and prog.num_publics == 4 and b.num_constraints == 2
    assert gp.GATE_CONST == 5 and GC(1) == (5 << 29) | 1
    other = gp.GateBuilder(6, 2)
    with pytest.raises(ValueError, match="another"):
        b.constraint(b.wires[0] * other.wires[0])
    with pytest.raises(ValueError, match="another"):
        b.constraint(other.constants[0])
    # a built Program is taken as it is
    assert gp.GateProgram(prog, 3, 1, (2, 5)).program is prog


@pytest.mark.parametrize("name", sorted(gpr.TRANSCRIPTIONS) + ["u32_add"])
def test_traced_programs_use_the_gate_format_only(name):
    from plonky2_amd.plonk import gate_program as gp
    from plonky2_amd.starky import air
    fn = gpr.u32_add_gate if name == "u32_add" else gpr.TRANSCRIPTIONS[name][0]
    prog = _builder(fn).build()
    assert {i[0] for i in prog.insns} <= {air.ADD, air.SUB, air.MUL, air.CONSTRAINT}
    kinds = {o >> 29 for i in prog.insns for o in ((i[2], i[3]) if i[0] < air.CONSTRAINT else (i[2],))}
    assert air.NEXT not in kinds and kinds <= {air.LOCAL, air.PUBLIC, air.CONST, air.TEMP, gp.GATE_CONST}
    if name == "u32_add":
        assert kinds == {air.LOCAL, air.PUBLIC, air.CONST, air.TEMP, gp.GATE_CONST}
        assert prog.num_temps > 8 and sum(i[0] == air.CONSTRAINT for i in prog.insns) == gpr.U32_CONSTRAINTS
    else:
        kind, p0, p1 = gpr.TRANSCRIPTIONS[name][1]
        g = gr.Gate(kind, 0, 0, (0, 1), p0, p1)
        assert sum(i[0] == air.CONSTRAINT for i in prog.insns) == trg.rr.num_constraints(g)
        assert gpr.TRANSCRIPTIONS[name][2:] == (trg.rr.num_wires(g), trg.rr.num_constants(g))


def test_interpreted_programs_equal_the_functions():
    """on random rows: every transcription equals the restated gate, the synthetic gate its plain function"""
    rng = np.random.default_rng(5)
    u32 = _builder(gpr.u32_add_gate).build()
    for _ in range(3):
        w, c, pih = ([int(v) for v in tg._rand(rng, k)] for k in (W, NUM_GATE_CONSTS, 4))
        assert gpr.interpret(u32.insns, u32.constants, u32.num_temps, w, c, pih) == gpr.u32_add_plain(w, c, pih)
        for name, (fn, (kind, p0, p1), _, _) in gpr.TRANSCRIPTIONS.items():
            prog = _builder(fn).build()
            exp = trg.rr.eval_unfiltered(vr.BASE, gr.Gate(kind, 0, 0, (0, 1), p0, p1), w, c, pih)
            assert gpr.interpret(prog.insns, prog.constants, prog.num_temps, w, c, pih) == [int(v) for v in exp], name


def test_u32_add_vanishes_on_a_real_addition():
    rng = np.random.default_rng(6)
    for _ in range(4):
        x, y, cin = int(rng.integers(0, 3 ** 20)), int(rng.integers(0, 3 ** 20)), int(rng.integers(0, 2))
        c, pih = [3 ** 20, 1], [0, 0, int(rng.integers(0, 1000)), 0]
        total = x + y + cin + pih[2]
        out, cout = total % 3 ** 20, total // 3 ** 20
        w = [x, y, cin, out, cout] + [out // 3 ** k % 3 for k in range(gpr.U32_LIMBS)] + [0] * (W - gpr.U32_WIRES)
        assert cout in (0, 1) and not any(gpr.u32_add_plain(w, c, pih))
        w[7] += 1
        assert any(gpr.u32_add_plain(w, c, pih))


# ------------------------------------------------------------------ each transcription as the only gate
@pytest.mark.parametrize("name", sorted(gpr.TRANSCRIPTIONS))
def test_transcription_equals_the_hand_written_kind(eng, name):
    """program == hand-written kind == restatement, bit for bit, nc = 1..4 (two more gates in the group: the filter has two factors)"""
    fn, (kind, p0, p1), _, _ = gpr.TRANSCRIPTIONS[name]
    gates = tg._alone(kind, p0, p1, row=1, group=(0, 3))
    q = tg._instance(300 + sorted(gpr.TRANSCRIPTIONS).index(name), gates, 1, 4, nc=4)
    exp = trg._ref_sums(q, tg._ldes(q))
    assert exp.all()
    b = tg._commit(eng, q)
    prog = _as_program(fn, gates[0])
    for nc in (1, 2, 3, 4):
        hand = tg._device_sums(eng, q, b, nc)
        got = _device_sums(eng, q, b, nc, [], [prog])
        assert got.shape == (nc, 16 << 3) and got.tobytes() == hand.tobytes() and (got == exp[:nc]).all(), nc


# ------------------------------------------------------------------ the gate the library does not know
@pytest.mark.parametrize("nls", [0, 5])
def test_synthetic_gate_equals_the_interpreter_and_the_function(eng, nls):
    """row 2 of a group of four, several selector polynomials, a public_inputs_hash given by representatives in [P, 2^64)"""
    pih = [3, P - 1, 0, 12345]
    placeholder = [gr.Gate(gr.NOOP, 2, 1, (0, 4))]
    q = tg._instance(70 + nls, placeholder, 2, 4, nls=nls, nc=3, pih=pih)
    prog = _as_program(gpr.u32_add_gate, placeholder[0])
    ldes = tg._ldes(q)
    exp = _ref_program_sums(q, ldes, [prog])
    # the plain function under the restated filter and reduction
    qbits, plain = 3, np.zeros_like(exp)
    for i in range(q["n"] << qbits):
        (li, step), _ = vr.quotient_rows(i, q["log_n"], RATE_BITS, qbits)
        w, cs = vr.get_lde_values(ldes["wires"], li, step), vr.get_lde_values(ldes["cs"], li, step)
        f = gr.compute_filter(vr.BASE, 2, (0, 4), cs[1], True)
        cons = gpr.u32_add_plain(w, cs[2 + nls:], pih)
        plain[:, i] = [f * sum(v * pow(a, j, P) for j, v in enumerate(cons)) % P for a in q["alphas"]]
    assert (exp == plain).all() and exp.all()
    b = tg._commit(eng, q)
    shifted = [3 + P, P - 1, P, 12345 + P]
    assert max(shifted) < 1 << 64
    assert (_device_sums(eng, q, b, 3, [], [prog]) == exp).all()
    assert (_device_sums(eng, q, b, 3, [], [prog], pih=shifted) == exp).all()


# ------------------------------------------------------------------ a mixed call
_MIXED = {}


def _mixed(max_temps):
    """the full library set of tests/test_gates.py (rows 0..7, three groups) and three program gates behind it: a gate without
    constraints and one of exactly max_temps temp slots in group (8, 10), the synthetic gate alone in group (10, 11)"""
    if max_temps not in _MIXED:
        lib_gates, ns = tg._full_set()
        places = [gr.Gate(gr.NOOP, 8, ns, (8, 10)), gr.Gate(gr.NOOP, 9, ns, (8, 10)), gr.Gate(gr.NOOP, 10, ns + 1, (10, 11))]
        q = tg._instance(17, lib_gates + places, ns + 2, 4, satisfied=True, nc=2)
        programs = [_as_program(lambda b: None, places[0]), _as_program(_wide_gate(max_temps), places[1]), _as_program(gpr.u32_add_gate, places[2])]
        assert [p.program.num_temps for p in programs][:2] == [0, max_temps] and programs[0].program.insns == []
        ldes = tg._ldes(q)
        ref_lib, ref_prog = tg._ref_sums(q, ldes, gates=lib_gates), _ref_program_sums(q, ldes, programs)
        _MIXED[max_temps] = (q, lib_gates, programs, ref_lib, ref_prog)
    return _MIXED[max_temps]


def test_mixed_call_equals_the_reference_and_the_host_residual(eng):
    from plonky2_amd.plonk.prover import compute_quotient_polys, compute_quotient_polys_gates
    nc = 2
    q, lib_gates, programs, ref_lib, ref_prog = _mixed(eng.lib.p2hot_air_max_temps())
    assert q["ns"] == 5 and ref_lib.all() and ref_prog.all()
    b = tg._commit(eng, q, ("wires", "cs", "zs"))
    total = _add(ref_lib, ref_prog)
    assert (_device_sums(eng, q, b, nc, lib_gates, programs) == total).all()
    args = (b["wires"], b["cs"], q["sigmas_first"], b["zs"], q["k_is"], q["qdf"], q["betas"][:nc], q["gammas"][:nc], q["alphas"][:nc])
    cols, vals = compute_quotient_polys(*args, gate_sums=total, want_values=True, engine=eng)
    chunks = cols.host()
    assert chunks.any()
    # everything on the device
    cols, got = compute_quotient_polys_gates(*args, tg._gate_set(q, lib_gates), want_values=True, engine=eng, programs=programs)
    assert (got == vals).all() and (cols.host() == chunks).all()
    # the same programs through the host residual instead, and one program on the device with the others as the residual
    cols, got = compute_quotient_polys_gates(*args, tg._gate_set(q, lib_gates), gate_sums=ref_prog, want_values=True, engine=eng)
    assert (got == vals).all() and (cols.host() == chunks).all()
    rest = _ref_program_sums(q, tg._ldes(q), programs[:2])
    cols, got = compute_quotient_polys_gates(*args, tg._gate_set(q, lib_gates), gate_sums=rest, want_values=True, engine=eng, programs=programs[2:])
    assert (got == vals).all() and (cols.host() == chunks).all()


def _lookup_case(seed):
    """the lookup instance of tests/test_gates.py's lookup test (15 wires, factor 4, two selector polynomials, no gate constants):
    PublicInput as a descriptor, BaseSum<2> of 10 limbs and Reducing(3) as programs in the second group"""
    from tests import test_lookup as tl
    nc, num_routed, qdf = 2, 12, 4
    q = tl._instance(np.random.default_rng(seed), nc, qdf, num_routed, 3, 4, satisfied=False)
    nls = 4 + len(q["luts"])
    lib_gates = [gr.Gate(gr.PUBLIC_INPUT, 0, 0, (0, 1))]
    gq = dict(gates=lib_gates, ns=2, nls=nls, log_n=4, n=16, qdf=qdf, pih=[5, 6, 7, 8], alphas=q["alphas"])
    programs = [_program(lambda b: gpr.base_sum_gate(b, 10, 2), 1, 1, (1, 3), 15, 0), _program(lambda b: gpr.reducing_gate(b, 3), 2, 1, (1, 3), 15, 0)]
    return tl, q, gq, lib_gates, programs


def test_lookup_variant_equals_the_host_residual(eng):
    from plonky2_amd.plonk.prover import compute_quotient_polys_lookup, compute_quotient_polys_lookup_gates
    tl, q, gq, lib_gates, programs = _lookup_case(23)
    ldes = {name: vr.Lde(vr.interpolate_columns(q[name]), 4, 3) for name in ("wires", "cs")}
    ref_lib, ref_prog = tg._ref_sums(gq, ldes), _ref_program_sums(gq, ldes, programs)
    assert ref_lib.all() and ref_prog.all()
    b = tl._commit(eng, q)
    args = (b["wires"], b["cs"], q["sigmas_first"], b["zs"], q["k_is"], gq["qdf"], q["betas"], q["gammas"], q["alphas"], q["lu_slots"], q["lut_slots"],
            tl.SEL_FIRST, q["deltas"], q["evals"])
    cols, vals = compute_quotient_polys_lookup(*args, gate_sums=_add(ref_lib, ref_prog), want_values=True, engine=eng)
    chunks = cols.host()
    assert vals.any()
    cols, got = compute_quotient_polys_lookup_gates(*args, tg._gate_set(gq), want_values=True, engine=eng, programs=programs)
    assert (got == vals).all() and (cols.host() == chunks).all()
    cols, got = compute_quotient_polys_lookup_gates(*args, tg._gate_set(gq), gate_sums=ref_prog, want_values=True, engine=eng)
    assert (got == vals).all() and (cols.host() == chunks).all()
    cols, got = compute_quotient_polys_lookup_gates(*args, tg._gate_set(gq, []), gate_sums=_add(ref_lib, _ref_program_sums(gq, ldes, programs[1:])),
                                                    want_values=True, engine=eng, programs=programs[:1])
    assert (got == vals).all() and (cols.host() == chunks).all()


# ------------------------------------------------------------------ empty inputs, a satisfied circuit, a broken wire
_CIRCUIT = {}


def _circuit(qdf, log_n):
    """six transcribed gates in two groups ((0, 3): degrees up to 2, (3, 6): degree 3 -- size + degree <= 8 for factor 7 too), every
    row satisfied.  Arithmetic has 21 operations here: the last one sits on the unrouted wires 80..83"""
    if (qdf, log_n) not in _CIRCUIT:
        kinds = [(gr.CONSTANT, 2, 0), (gr.PUBLIC_INPUT, 0, 0), (gr.BASE_SUM, 4, 2), (gr.ARITHMETIC, 21, 0), (gr.ARITHMETIC_EXT, 10, 0), (gr.MUL_EXT, 13, 0)]
        groups = [(0, 3), (3, 6)]
        gates = [gr.Gate(kind, row, row // 3, groups[row // 3], p0, p1) for row, (kind, p0, p1) in enumerate(kinds)]
        T = gpr.TRANSCRIPTIONS
        fns = [T["constant_2"][0], T["public_input"][0], T["base_sum_2_4"][0], lambda b: gpr.arithmetic_gate(b, 21), T["arithmetic_ext_10"][0],
               T["mul_ext_13"][0]]
        q = tg._instance(90 + qdf, gates, 2, log_n, satisfied=True, qdf=qdf, nc=2)
        _CIRCUIT[(qdf, log_n)] = (q, [_as_program(fn, g) for fn, g in zip(fns, gates)])
    return _CIRCUIT[(qdf, log_n)]


def _quotients(eng, q, b, nc, gates, programs):
    from plonky2_amd.plonk.prover import compute_quotient_polys_gates
    cols, vals = compute_quotient_polys_gates(b["wires"], b["cs"], q["sigmas_first"], b["zs"], q["k_is"], q["qdf"], q["betas"][:nc], q["gammas"][:nc],
                                              q["alphas"][:nc], tg._gate_set(q, gates), want_values=True, engine=eng, programs=programs)
    return cols.host(), vals


def test_empty_inputs(eng):
    """no programs: the entry points without programs; no descriptors: the all-descriptor call.  512 points, two workgroups"""
    nc = 2
    q, programs = _circuit(8, 6)
    b = tg._commit(eng, q, ("wires", "cs", "zs"))
    hand = tg._device_sums(eng, q, b, nc)
    assert hand.all()
    assert _device_sums(eng, q, b, nc, None, []).tobytes() == hand.tobytes()
    assert _device_sums(eng, q, b, nc, [], programs).tobytes() == hand.tobytes()
    assert _device_sums(eng, q, b, nc, q["gates"][:3], programs[3:]).tobytes() == hand.tobytes()
    chunks, vals = tg._quotients(eng, q, b, nc, None, None)
    for gates, progs in ((None, []), ([], programs), (q["gates"][1::2], programs[0::2])):
        got_chunks, got_vals = _quotients(eng, q, b, nc, gates, progs)
        assert (got_vals == vals).all() and (got_chunks == chunks).all()


def test_satisfied_circuit_passes_the_verifier_identity(eng):
    nc = 2
    q, programs = _circuit(8, 6)
    b = tg._commit(eng, q, ("wires", "cs", "zs"))
    chunks, _ = _quotients(eng, q, b, nc, [], programs)
    assert tg._identity_holds(eng, q, b, chunks, nc, 3) == [True] * nc


def _break_arithmetic(q):
    """the output of Arithmetic's last operation (wire 83: not routed, the permutation argument stays satisfied)"""
    q = dict(q)
    wires = q["wires"].copy()
    row = q["row_gate"].index(3)
    wires[83][row] = (int(wires[83][row]) + 1) % P
    q["wires"] = wires
    return q


def test_broken_wire_fails_the_quotient(eng):
    """factor 7 at rate 8: the trim sees a quotient that is no polynomial (tests/test_gates.py has the reasoning)"""
    nc = 2
    q, programs = _circuit(7, 4)
    b = tg._commit(eng, q, ("wires", "cs", "zs"))
    chunks, _ = _quotients(eng, q, b, nc, [], programs)
    assert chunks.shape == (nc * 7, 16) and tg._identity_holds(eng, q, b, chunks, nc, 4) == [True] * nc
    bad = _break_arithmetic(q)
    b["wires"] = tg._commit(eng, bad, ("wires",))["wires"]
    with pytest.raises(ValueError, match="Quotient has failed"):
        _quotients(eng, bad, b, nc, [], programs)
    assert eng.lib.p2hot_ctx_trim(eng.ctx) == 0


# ------------------------------------------------------------------ errors
def test_errors_come_before_any_work(eng):
    from plonky2_amd import _lib
    from plonky2_amd.plonk import gate_program as gp
    from plonky2_amd.plonk.prover import GateSet
    from plonky2_amd.starky import air
    q, good_programs = _circuit(7, 4)
    b = tg._commit(eng, q, ("wires", "cs", "zs"))
    nc, sf, ns = 2, q["sigmas_first"], 2
    L, N, PUB, CST, T, GC = (lambda i, k=k: air.operand(k, i) for k in range(6))
    good = [(air.MUL, 0, L(0), GC(1)), (air.ADD, 1, T(0), CST(0)), (air.SUB, 0, T(1), PUB(3)), (air.CONSTRAINT, 0, T(0), 0)]
    keep = []

    # the program's place: row 6 behind the circuit's six gates, in a group that holds every value of selector polynomial 1 -- (3, 7)
    # -- so its filter vanishes on every row of H and the quotient of the calls that pass is the circuit's permutation argument's
    def call(which, insns=good, constants=(7,), num_temps=2, num_publics=4, row=6, sel=1, group=(3, 7), gates=(), null=None, count=None, qdf=7, ns=ns,
             second=None):
        prog = gp.GateProgram(air.Program(insns, constants, num_temps, num_publics, W), row, sel, group)
        arr, n, k = gp.marshal([prog] + ([second] if second else []))
        if null == "insns":
            k[0][0].program.insns = None
        if null == "constants":
            k[0][0].program.constants = None
        gs = GateSet(list(gates), ns, 0, q["pih"])
        keep.extend([k, gs])
        parr = None if null == "programs" else arr
        n = n if count is None else count
        out = np.zeros((nc, 16 << 3), dtype=np.uint64)
        if which == "sums":
            rc = eng.lib.p2hot_gate_sums_programs(eng.ctx, b["wires"]._h, b["cs"]._h, sf, gs.ptr, qdf, tg._u64(q["alphas"]), nc,
                                                  out.ctypes.data_as(C.c_void_p), parr, n)
        else:
            h = C.c_void_p(1)
            rc = eng.lib.p2hot_quotient_polys_gate_programs(eng.ctx, b["wires"]._h, b["cs"]._h, sf, b["zs"]._h, tg._u64(q["k_is"]), NUM_ROUTED, qdf,
                                                            tg._u64(q["betas"]), tg._u64(q["gammas"]), tg._u64(q["alphas"]), nc, None, gs.ptr,
                                                            out.ctypes.data_as(C.c_void_p), C.byref(h), parr, n)
            assert rc == _lib.OK or not h.value           # chunks_out is null after every failure
            if rc == _lib.OK:
                eng.lib.p2hot_cols_free(h)
        assert out.any() if rc == _lib.OK else not out.any()
        return rc, eng.lib.p2hot_last_error(eng.ctx)
    both = ("sums", "quotient")
    for which in both:
        assert call(which)[0] == _lib.OK, eng.lib.p2hot_last_error(eng.ctx)

    def patched(k, insn):
        return good[:k] + [insn] + good[k + 1:]
    deg3 = [(air.MUL, 0, L(0), L(1)), (air.MUL, 0, T(0), GC(0)), (air.CONSTRAINT, 0, T(0), 0)]
    einval = {
        "null programs": dict(null="programs"),
        "null insns": dict(null="insns"),
        "null constants": dict(null="constants"),
        "row below its group": dict(row=2), "row above its group": dict(row=7),
        "group of 257": dict(group=(3, 260), insns=[]),
        "selector index": dict(sel=2),
        "wire index": dict(insns=patched(0, (air.MUL, 0, L(W), GC(1)))),
        "gate constant reaches the sigmas": dict(insns=patched(0, (air.MUL, 0, L(0), GC(2)))),
        "gate constant behind more selectors": dict(ns=3, sel=1),
        "selectors reach the sigmas": dict(ns=5, insns=[]),
        "next operand": dict(insns=patched(0, (air.MUL, 0, N(0), GC(1)))),
        "operand kind 6": dict(insns=patched(0, (air.MUL, 0, air.operand(6, 0), GC(1)))),
        "operand kind 7": dict(insns=patched(0, (air.MUL, 0, L(0), air.operand(7, 0)))),
        "five publics": dict(num_publics=5),
        "public index": dict(num_publics=3),
        "constant index": dict(insns=patched(1, (air.ADD, 1, T(0), CST(1)))),
        "temp index": dict(insns=patched(1, (air.ADD, 1, T(2), CST(0)))),
        "dst index": dict(insns=patched(1, (air.ADD, 2, T(0), CST(0)))),
        "temp read before written": dict(insns=patched(0, (air.MUL, 0, T(1), GC(1)))),
        "row twice among the programs": dict(second=gp.GateProgram(air.Program([], [], 0, 0, W), 6, 1, (3, 7))),
        "row also a descriptor": dict(gates=[(gr.NOOP, 6, 1, 3, 7, 0, 0)]),
        # degree 3 under a filter of degree 4 + 1 (a group of five, two selector polynomials) is 8 = factor + 1; a group of six makes it 9
        "degree": dict(insns=deg3, group=(3, 9)),
        # ... and with one selector polynomial a group of six is 8, one of seven 9
        "degree with one selector": dict(insns=deg3, group=(3, 10), ns=1, sel=0),
    }
    assert call("sums", insns=deg3, group=(3, 9), ns=1, sel=0)[0] == _lib.OK       # (sums only: read as ONE selector polynomial this is no circuit)
    for which in both:
        assert call(which, insns=deg3, group=(3, 8))[0] == _lib.OK
        for why, kw in einval.items():
            rc, msg = call(which, **kw)
            assert rc == _lib.EINVAL, (which, why, msg)
            assert b"program" in msg and (b"program 0" in msg or b"program 1" in msg or why == "null programs"), (why, msg)
            if "insns" in kw and kw["insns"] and why not in ("degree", "degree with one selector"):
                assert b"instruction " in msg, (why, msg)
    assert b"instruction 2" in call("sums", insns=deg3, group=(3, 9))[1]
    unsupported = {
        "op 7": dict(insns=patched(0, (7, 0, L(0), GC(1)))),
        "transition": dict(insns=patched(3, (air.CONSTRAINT_TRANSITION, 0, T(0), 0))),
        "first row": dict(insns=patched(3, (air.CONSTRAINT_FIRST_ROW, 0, T(0), 0))),
        "last row": dict(insns=patched(3, (air.CONSTRAINT_LAST_ROW, 0, T(0), 0))),
        "temps": dict(num_temps=eng.lib.p2hot_air_max_temps() + 1),
    }
    for which in both:
        for why, kw in unsupported.items():
            rc, msg = call(which, **kw)
            assert rc == _lib.EUNSUPPORTED and b"program 0" in msg, (which, why, msg)
    # num_programs == 0 does not look at the array; the gate set's own errors stay what they are
    for which in both:
        assert call(which, null="programs", count=0, gates=[g.descriptor() for g in q["gates"]])[0] == _lib.OK
        assert call(which, gates=[(8, 0, 0, 0, 1, 0, 0)])[0] == _lib.EUNSUPPORTED
    assert eng.lib.p2hot_ctx_trim(eng.ctx) == 0
    for which in both:
        assert call(which)[0] == _lib.OK


def test_gate_const_operand_stays_invalid_in_a_stark_program(eng):
    from plonky2_amd import _lib
    from plonky2_amd.fri.oracle import PolynomialBatch
    from plonky2_amd.starky import air
    rng = np.random.default_rng(72)
    trace = PolynomialBatch.from_values(tg._rand(rng, 3, 16), 1, False, 0, engine=eng)
    alphas = np.asarray([5, 6], dtype=np.uint64)
    out = np.zeros((2, 16 << 1), dtype=np.uint64)

    def accs(a):
        prog = air.Program([(air.MUL, 0, a, air.operand(air.LOCAL, 1)), (air.CONSTRAINT, 0, air.operand(air.TEMP, 0), 0)], [], 1, 0, 3)
        ps = prog.struct()
        return eng.lib.p2hot_stark_constraint_accs(eng.ctx, trace._h, C.byref(ps), None, 3, alphas.ctypes.data_as(C.c_void_p), 2, out.ctypes.data_as(C.c_void_p))
    assert accs(air.operand(air.LOCAL, 0)) == _lib.OK and out.any()
    out[:] = 0
    assert accs(air.operand(5, 0)) == _lib.EINVAL and b"unknown kind 5" in eng.lib.p2hot_last_error(eng.ctx) and not out.any()


# ------------------------------------------------------------------ hashers
def test_keccak_hashed_commitments(eng):
    """the hasher rules of the entry points without programs: the sums take commitments of any hasher, and so does the quotient
    without lookups (p2hot_quotient_polys reads LDE matrices, not trees); the lookup quotient refuses a KeccakHash commitment"""
    from plonky2_amd import _lib
    from plonky2_amd.hash.keccak import KeccakHash
    from plonky2_amd.plonk.prover import compute_quotient_polys_lookup_gates
    nc = 2
    q, programs = _circuit(8, 6)
    poseidon = tg._commit(eng, q, ("wires", "cs", "zs"))
    keccak = tg._commit(eng, q, ("wires", "cs", "zs"), hasher=KeccakHash(25))
    assert (keccak["wires"].merkle_tree.cap.entries != poseidon["wires"].merkle_tree.cap.entries).any()
    got = _device_sums(eng, q, keccak, nc, [], programs)
    assert got.tobytes() == _device_sums(eng, q, poseidon, nc, [], programs).tobytes() and got.all()
    # the quotient without lookups: what the entry point without programs does with these commitments
    chunks, vals = tg._quotients(eng, q, keccak, nc, None, None)
    got_chunks, got_vals = _quotients(eng, q, keccak, nc, [], programs)
    assert (got_vals == vals).all() and (got_chunks == chunks).all()
    tl, lq, gq, lib_gates, lprograms = _lookup_case(24)
    from plonky2_amd.fri.oracle import PolynomialBatch
    lb = {name: PolynomialBatch.from_values(lq[name], 3, False, 0, engine=eng, hasher=KeccakHash(25)) for name in ("wires", "cs", "zs")}
    with pytest.raises(_lib.P2HotError, match="Keccak") as e:
        compute_quotient_polys_lookup_gates(lb["wires"], lb["cs"], lq["sigmas_first"], lb["zs"], lq["k_is"], gq["qdf"], lq["betas"], lq["gammas"], lq["alphas"],
                                            lq["lu_slots"], lq["lut_slots"], tl.SEL_FIRST, lq["deltas"], lq["evals"], tg._gate_set(gq), engine=eng,
                                            programs=lprograms)
    assert e.value.code == _lib.EUNSUPPORTED
