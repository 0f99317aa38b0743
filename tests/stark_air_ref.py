"""A STARK's own constraints restated from the reference's text (starky/src/fibonacci_stark.rs, constraint_consumer.rs,
prover.rs::compute_quotient_polys), independent of the library: nothing here imports it.

Constraint functions are generic over a field object F (vanishing_ref.BASE / vanishing_ref.EXT, or any object with the same
interface) and take stark_lookup_ref.ConstraintConsumer, the way the lookup restatement's functions do: the same function runs on
base-field integers at the points of the quotient coset and on extension elements at zeta.  `public_inputs` are elements of F.

Also here: a plain interpreter of the constraint-program format of include/p2hot.h, written from the header's text, so that a
builder's mistake and a kernel's cannot cancel each other."""
from tests import stark_lookup_ref as sr
from tests import vanishing_ref as vr
from tests.pyref import G, P, root_of_unity

# ------------------------------------------------------------------ FibonacciStark (starky/src/fibonacci_stark.rs)
FIBONACCI_COLUMNS, FIBONACCI_PUBLIC_INPUTS = 2, 3
PI_INDEX_X0, PI_INDEX_X1, PI_INDEX_RES = 0, 1, 2


def fibonacci(F, local_values, next_values, public_inputs, yield_constr):
    """eval_packed_generic (fibonacci_stark.rs:77-98)"""
    # Check public inputs.
    yield_constr.constraint_first_row(F.sub(local_values[0], public_inputs[PI_INDEX_X0]))
    yield_constr.constraint_first_row(F.sub(local_values[1], public_inputs[PI_INDEX_X1]))
    yield_constr.constraint_last_row(F.sub(local_values[1], public_inputs[PI_INDEX_RES]))
    # x0' <- x1
    yield_constr.constraint_transition(F.sub(next_values[0], local_values[1]))
    # x1' <- x0 + x1
    yield_constr.constraint_transition(F.sub(F.sub(next_values[1], local_values[0]), local_values[1]))


def fibonacci_trace(num_rows, x0, x1):
    """generate_trace (fibonacci_stark.rs:47-57): [2][num_rows] columns, and the public inputs [x0, x1, res]"""
    rows, acc = [], [x0 % P, x1 % P]
    for _ in range(num_rows):
        rows.append(list(acc))
        acc = [acc[1], (acc[0] + acc[1]) % P]
    cols = [[r[c] for r in rows] for c in range(FIBONACCI_COLUMNS)]
    return cols, [x0 % P, x1 % P, cols[1][num_rows - 1]]


# ------------------------------------------------------------------ a synthetic AIR that uses all of the program format
MIXED_COLUMNS, MIXED_PUBLIC_INPUTS = 6, 2
MIXED_K = (1 << 63) + 0x1234567  # a constant above 2^63


def mixed(F, lv, nv, pi, cons, cubic=True):
    """six columns: c0 counts up from pi[0]; c1' = K c1 + c0; c2 = c0 c1; c3 = c0 c0 c1 (the degree-3 product, left out with
    cubic=False so the AIR fits constraint_degree 2); c4 sums c2 from 0 and ends at pi[1]; c5 = (c0 + c1)^2 - 3.  s = c0 + c1
    is used at the top and again in the last constraint: it lives across everything in between"""
    cons.constraint_first_row(F.sub(lv[0], pi[0]))
    cons.constraint_transition(F.sub(F.sub(nv[0], lv[0]), F.lift(1)))
    s = F.add(lv[0], lv[1])
    cons.constraint(F.add(F.sub(lv[5], F.mul(s, s)), F.lift(3)))
    cons.constraint_transition(F.sub(nv[1], F.add(F.mul(lv[1], F.lift(MIXED_K)), lv[0])))
    cons.constraint(F.sub(lv[2], F.mul(lv[0], lv[1])))
    if cubic:
        cons.constraint(F.sub(lv[3], F.mul(F.mul(lv[0], lv[0]), lv[1])))
    cons.constraint_first_row(lv[4])
    cons.constraint_transition(F.sub(F.sub(nv[4], lv[4]), lv[2]))
    cons.constraint_last_row(F.sub(lv[4], pi[1]))
    cons.constraint(F.sub(F.sub(F.add(lv[5], F.lift(3)), F.mul(s, lv[0])), F.mul(s, lv[1])))


def mixed2(F, lv, nv, pi, cons):
    return mixed(F, lv, nv, pi, cons, cubic=False)


def mixed_trace(num_rows, start, seed):
    """a trace `mixed` accepts, and its public inputs"""
    c = [[0] * num_rows for _ in range(MIXED_COLUMNS)]
    c1, c4 = seed % P, 0
    for i in range(num_rows):
        c0 = (start + i) % P
        c[0][i], c[1][i], c[2][i], c[3][i], c[4][i] = c0, c1, c0 * c1 % P, c0 * c0 * c1 % P, c4
        c[5][i] = ((c0 + c1) * (c0 + c1) - 3) % P
        c1, c4 = (c1 * MIXED_K + c0) % P, (c4 + c0 * c1) % P
    return c, [start % P, c[4][num_rows - 1]]


AIRS = {"fibonacci": (fibonacci, FIBONACCI_COLUMNS, FIBONACCI_PUBLIC_INPUTS, 2),   # name -> (function, width, public inputs, degree)
        "mixed": (mixed, MIXED_COLUMNS, MIXED_PUBLIC_INPUTS, 3), "mixed2": (mixed2, MIXED_COLUMNS, MIXED_PUBLIC_INPUTS, 2)}


# ------------------------------------------------------------------ the program format (include/p2hot.h), interpreted
LOCAL, NEXT, PUBLIC, CONST, TEMP = range(5)
ADD, SUB, MUL, CONSTRAINT, CONSTRAINT_TRANSITION, CONSTRAINT_FIRST_ROW, CONSTRAINT_LAST_ROW = range(7)


def interpret(F, insns, constants, num_temps, local_values, next_values, public_inputs, consumer):
    """insns: (op, dst, a, b) words; an operand's top 3 bits are its kind, the low 29 its index"""
    temps = [None] * num_temps

    def operand(o):
        kind, idx = o >> 29, o & ((1 << 29) - 1)
        if kind == LOCAL:
            return local_values[idx]
        if kind == NEXT:
            return next_values[idx]
        if kind == PUBLIC:
            return public_inputs[idx]
        if kind == CONST:
            return F.lift(constants[idx] % P)
        assert kind == TEMP and temps[idx] is not None, "a temp read before it was written, or an unknown kind"
        return temps[idx]
    for op, dst, a, b in insns:
        if op == ADD:
            temps[dst] = F.add(operand(a), operand(b))
        elif op == SUB:
            temps[dst] = F.sub(operand(a), operand(b))
        elif op == MUL:
            temps[dst] = F.mul(operand(a), operand(b))
        else:
            [consumer.constraint, consumer.constraint_transition, consumer.constraint_first_row, consumer.constraint_last_row][op - CONSTRAINT](operand(a))


# ------------------------------------------------------------------ compute_quotient_polys' loop, the STARK's constraints alone
def coset_consumers(trace_lde, alphas, constraint_degree):
    """per point i of the quotient coset (natural order): the frame and a fresh consumer, as prover.rs:531-590 sets them up"""
    degree_bits, rate_bits = trace_lde.degree_bits, trace_lde.rate_bits
    n = 1 << degree_bits
    qbits = vr.log2_ceil(sr.quotient_degree_factor(constraint_degree))
    assert qbits <= rate_bits
    step, next_step, size = 1 << (rate_bits - qbits), 1 << qbits, n << qbits
    l_first, l_last = sr.selector_lde(n, 0, qbits), sr.selector_lde(n, n - 1, qbits)
    last = pow(root_of_unity(degree_bits), P - 2, P)
    w = root_of_unity(degree_bits + qbits)
    for i in range(size):
        x = G * pow(w, i, P) % P
        consumer = sr.ConstraintConsumer(vr.BASE, alphas, (x - last) % P, l_first[i], l_last[i])
        yield i, vr.get_lde_values(trace_lde, i, step), vr.get_lde_values(trace_lde, (i + next_step) % size, step), consumer


def constraint_accs(fn, trace_lde, public_inputs, alphas, constraint_degree):
    """ConstraintConsumer::accumulators() after fn alone at every point: [nc][n << qbits], natural order"""
    pts = list(coset_consumers(trace_lde, alphas, constraint_degree))
    out = [[0] * len(pts) for _ in alphas]
    pub = [p % P for p in public_inputs]
    for i, local, nxt, consumer in pts:
        fn(vr.BASE, local, nxt, pub, consumer)
        for a, acc in enumerate(consumer.accs):
            out[a][i] = acc % P
    return out
