"""The constraints of eight reference gates, the gate filter and their reduction, restated with Python integers from the reference
alone (plonky2/src/gates/{noop,constant,public_input,arithmetic_base,arithmetic_extension,multiplication_extension,base_sum,
poseidon}.rs, gates/gate.rs:158-185, :326-333, plonk/vanishing_poly.rs:702-728, hash/poseidon.rs).  Generic over
vanishing_ref.BASE / EXT: over EXT it is eval_unfiltered at the verifier's zeta, where the two extension gates work in the
extension ALGEBRA -- pairs (a0, a1) of field elements with (a0, a1)(b0, b1) = (a0 b0 + 7 a1 b1, a0 b1 + a1 b0).  Nothing here
imports the library or the CPU oracle; the Poseidon tables are the generated constants the naive permutation of tests/pyref.py
reads.  A witness filler per gate makes satisfied rows."""
from tests.pyref import _C, CIRC, DIAG, P, RC

NOOP, CONSTANT, PUBLIC_INPUT, ARITHMETIC, ARITHMETIC_EXT, MUL_EXT, BASE_SUM, POSEIDON = range(8)
UNUSED_SELECTOR = 0xFFFFFFFF                      # gates/selectors.rs:13
FIRST_RC = _C["P2_POSEIDON_FAST_PARTIAL_FIRST_ROUND_CONSTANT"]
FAST_RC = _C["P2_POSEIDON_FAST_PARTIAL_ROUND_CONSTANTS"]
VS = _C["P2_POSEIDON_FAST_PARTIAL_ROUND_VS"]          # [22][11]
W_HATS = _C["P2_POSEIDON_FAST_PARTIAL_ROUND_W_HATS"]  # [22][11]
INIT = _C["P2_POSEIDON_FAST_PARTIAL_ROUND_INITIAL_MATRIX"]   # [11][11] row major

# PoseidonGate's wires (gates/poseidon.rs:43-101)
WIRE_SWAP, START_DELTA, START_FULL_0, START_PARTIAL, START_FULL_1, POSEIDON_END = 24, 25, 29, 65, 87, 135


class Gate:
    """one entry of common_data.gates: `row` is its index there, group = selectors_info.groups[selector_index]"""

    def __init__(self, kind, row, selector_index, group, param0=0, param1=0):
        self.kind, self.row, self.selector_index, self.group, self.param0, self.param1 = kind, row, selector_index, tuple(group), param0, param1

    def descriptor(self):
        return (self.kind, self.row, self.selector_index, self.group[0], self.group[1], self.param0, self.param1)


def num_wires(g):
    return {NOOP: 0, CONSTANT: g.param0, PUBLIC_INPUT: 4, ARITHMETIC: 4 * g.param0, ARITHMETIC_EXT: 8 * g.param0,
            MUL_EXT: 6 * g.param0, BASE_SUM: 1 + g.param0, POSEIDON: POSEIDON_END}[g.kind]


def num_constants(g):
    return {CONSTANT: g.param0, ARITHMETIC: 2, ARITHMETIC_EXT: 2, MUL_EXT: 1}.get(g.kind, 0)


def num_constraints(g):
    return {NOOP: 0, CONSTANT: g.param0, PUBLIC_INPUT: 4, ARITHMETIC: g.param0, ARITHMETIC_EXT: 2 * g.param0,
            MUL_EXT: 2 * g.param0, BASE_SUM: 1 + g.param0, POSEIDON: 123}[g.kind]


# ------------------------------------------------------------------ the extension algebra over F (D = 2, W = 7)
def _alg_mul(F, a, b):
    return (F.add(F.mul(a[0], b[0]), F.scalar_mul(F.mul(a[1], b[1]), 7)), F.add(F.mul(a[0], b[1]), F.mul(a[1], b[0])))


def _alg_scale(F, a, c):
    return (F.mul(a[0], c), F.mul(a[1], c))


# ------------------------------------------------------------------ Poseidon layers over F (hash/poseidon.rs)
def _sbox(F, x):
    x2 = F.mul(x, x)
    x4 = F.mul(x2, x2)
    return F.mul(F.mul(x, x2), x4)


def _mds_layer(F, s):
    """poseidon.rs:180-199, :271-285: row r = sum_i s[(i + r) % 12] circ[i] + s[r] diag[r]"""
    out = []
    for r in range(12):
        acc = F.scalar_mul(s[r], DIAG[r])
        for i in range(12):
            acc = F.add(acc, F.scalar_mul(s[(i + r) % 12], CIRC[i]))
        out.append(acc)
    return out


def _constant_layer(F, s, round_ctr):
    return [F.add(s[i], F.lift(RC[12 * round_ctr + i])) for i in range(12)]


def _mds_partial_layer_init(F, s):
    """poseidon.rs:415-441: result[0] = state[0]; result[c] = sum_{r >= 1} state[r] M[r - 1][c - 1]"""
    out = [s[0]] + [F.zero] * 11
    for r in range(1, 12):
        for c in range(1, 12):
            out[c] = F.add(out[c], F.scalar_mul(s[r], INIT[11 * (r - 1) + c - 1]))
    return out


def _mds_partial_layer_fast(F, s, r):
    """poseidon.rs:516-542"""
    d = F.scalar_mul(s[0], CIRC[0] + DIAG[0])
    for i in range(1, 12):
        d = F.add(d, F.scalar_mul(s[i], W_HATS[11 * r + i - 1]))
    return [d] + [F.add(s[i], F.scalar_mul(s[0], VS[11 * r + i - 1])) for i in range(1, 12)]


def _poseidon_walk(F, w, on_sbox_input, on_output):
    """PoseidonGate's walk over the permutation (poseidon.rs:221-283): on_sbox_input(wire, computed) returns the value the state
    continues from; on_output(i, computed) sees the final state"""
    state = [None] * 12
    for i in range(4):
        d = w[START_DELTA + i]
        state[i], state[i + 4] = F.add(w[i], d), F.sub(w[i + 4], d)
    for i in range(8, 12):
        state[i] = w[i]
    round_ctr = 0
    for r in range(4):
        state = _constant_layer(F, state, round_ctr)
        if r != 0:
            state = [on_sbox_input(START_FULL_0 + 12 * (r - 1) + i, state[i]) for i in range(12)]
        state = _mds_layer(F, [_sbox(F, x) for x in state])
        round_ctr += 1
    state = [F.add(state[i], F.lift(FIRST_RC[i])) for i in range(12)]
    state = _mds_partial_layer_init(F, state)
    for r in range(22):
        x = on_sbox_input(START_PARTIAL + r, state[0])
        state[0] = _sbox(F, x)
        if r != 21:
            state[0] = F.add(state[0], F.lift(FAST_RC[r]))
        state = _mds_partial_layer_fast(F, state, r)
    round_ctr += 22
    for r in range(4):
        state = _constant_layer(F, state, round_ctr)
        state = [on_sbox_input(START_FULL_1 + 12 * r + i, state[i]) for i in range(12)]
        state = _mds_layer(F, [_sbox(F, x) for x in state])
        round_ctr += 1
    for i in range(12):
        on_output(i, state[i])


# ------------------------------------------------------------------ eval_unfiltered
def eval_unfiltered(F, g, w, c, pih):
    """the gate's constraints at one point: w = local_wires, c = the gate's own local_constants (selectors removed), pih = the four
    words of the public inputs hash; all elements of F"""
    k = g.kind
    if k == NOOP:
        return []
    if k == CONSTANT:                                   # constant.rs:126-128
        return [F.sub(c[i], w[i]) for i in range(g.param0)]
    if k == PUBLIC_INPUT:                               # public_input.rs:108-112
        return [F.sub(w[i], F.lift(pih[i])) for i in range(4)]
    if k == ARITHMETIC:                                 # arithmetic_base.rs:173-184
        return [F.sub(w[4 * i + 3], F.add(F.mul(F.mul(w[4 * i], w[4 * i + 1]), c[0]), F.mul(w[4 * i + 2], c[1]))) for i in range(g.param0)]
    if k in (ARITHMETIC_EXT, MUL_EXT):                  # arithmetic_extension.rs:92-110, multiplication_extension.rs:86-101
        per = 8 if k == ARITHMETIC_EXT else 6
        out = []
        for i in range(g.param0):
            v = w[per * i:per * i + per]
            comp = _alg_scale(F, _alg_mul(F, (v[0], v[1]), (v[2], v[3])), c[0])
            if k == ARITHMETIC_EXT:
                ad = _alg_scale(F, (v[4], v[5]), c[1])
                comp = (F.add(comp[0], ad[0]), F.add(comp[1], ad[1]))
            out += [F.sub(v[per - 2], comp[0]), F.sub(v[per - 1], comp[1])]
        return out
    if k == BASE_SUM:                                   # base_sum.rs:153-170
        limbs = w[1:1 + g.param0]
        s = F.zero
        for limb in reversed(limbs):
            s = F.add(F.scalar_mul(s, g.param1), limb)
        out = [F.sub(s, w[0])]
        for limb in limbs:
            acc = F.one
            for t in range(g.param1):
                acc = F.mul(acc, F.sub(limb, F.lift(t)))
            out.append(acc)
        return out
    assert k == POSEIDON                                # poseidon.rs:204-283
    swap = w[WIRE_SWAP]
    out = [F.mul(swap, F.sub(swap, F.one))]
    for i in range(4):
        out.append(F.sub(F.mul(swap, F.sub(w[i + 4], w[i])), w[START_DELTA + i]))

    def sbox_in(wire, computed):
        out.append(F.sub(computed, w[wire]))
        return w[wire]
    _poseidon_walk(F, w, sbox_in, lambda i, computed: out.append(F.sub(computed, w[12 + i])))
    assert len(out) == 123
    return out


def compute_filter(F, row, group, s, many_selectors):
    """gate.rs:326-333"""
    assert group[0] <= row < group[1]
    f = F.one
    for i in [i for i in range(group[0], group[1]) if i != row] + ([UNUSED_SELECTOR] if many_selectors else []):
        f = F.mul(f, F.sub(F.lift(i), s))
    return f


def evaluate_gate_constraints(F, gates, num_selectors, num_lookup_selectors, w, constants, pih):
    """vanishing_poly.rs:702-728 with eval_filtered (gate.rs:158-185): every gate's filtered constraints added into one vector"""
    out = []
    for g in gates:
        f = compute_filter(F, g.row, g.group, constants[g.selector_index], num_selectors > 1)
        cons = eval_unfiltered(F, g, w, constants[num_selectors + num_lookup_selectors:], pih)
        assert len(cons) == num_constraints(g)
        out += [F.zero] * (len(cons) - len(out))
        for j, v in enumerate(cons):
            out[j] = F.add(out[j], F.mul(f, v))
    return out


def reduced_sums(F, gates, num_selectors, num_lookup_selectors, w, constants, pih, alphas):
    """reduce_with_powers of the combined vector, per alpha"""
    cons = evaluate_gate_constraints(F, gates, num_selectors, num_lookup_selectors, w, constants, pih)
    out = []
    for a in alphas:
        s = F.zero
        for t in reversed(cons):
            s = F.add(F.mul(s, F.lift(a)), t)
        out.append(s)
    return out


# ------------------------------------------------------------------ witnesses (base field)
def determined_wires(g):
    """the wires fill_witness writes; every other wire of the row is free"""
    k = g.kind
    if k in (CONSTANT, PUBLIC_INPUT, BASE_SUM):
        return list(range(num_wires(g)))
    if k == ARITHMETIC:
        return [4 * i + 3 for i in range(g.param0)]
    if k == ARITHMETIC_EXT:
        return [8 * i + t for i in range(g.param0) for t in (6, 7)]
    if k == MUL_EXT:
        return [6 * i + t for i in range(g.param0) for t in (4, 5)]
    if k == POSEIDON:
        return list(range(12, POSEIDON_END))
    return []


def fill_witness(rng, g, w, c, pih, swap=None):
    """sets the determined wires of the row w (a list of ints, modified in place) so that the gate's constraints vanish; the free
    wires, the constants c and pih are read"""
    from tests.vanishing_ref import BASE as F
    k = g.kind
    if k == CONSTANT:
        w[:g.param0] = [int(v) % P for v in c[:g.param0]]
    elif k == PUBLIC_INPUT:
        w[:4] = [int(v) % P for v in pih]
    elif k == ARITHMETIC:
        for i in range(g.param0):
            w[4 * i + 3] = (w[4 * i] * w[4 * i + 1] * c[0] + w[4 * i + 2] * c[1]) % P
    elif k in (ARITHMETIC_EXT, MUL_EXT):
        per = 8 if k == ARITHMETIC_EXT else 6
        for i in range(g.param0):
            v = w[per * i:per * i + per]
            comp = _alg_scale(F, _alg_mul(F, (v[0], v[1]), (v[2], v[3])), c[0])
            if k == ARITHMETIC_EXT:
                comp = (comp[0] + v[4] * c[1], comp[1] + v[5] * c[1])
            w[per * i + per - 2], w[per * i + per - 1] = comp[0] % P, comp[1] % P
    elif k == BASE_SUM:
        limbs = [int(v) for v in rng.integers(0, g.param1, size=g.param0)]
        w[1:1 + g.param0] = limbs
        w[0] = sum(limb * pow(g.param1, e, P) for e, limb in enumerate(limbs)) % P
    elif k == POSEIDON:
        sw = int(rng.integers(0, 2)) if swap is None else swap
        w[WIRE_SWAP] = sw
        for i in range(4):
            w[START_DELTA + i] = sw * (w[i + 4] - w[i]) % P

        def sbox_in(wire, computed):
            w[wire] = computed
            return computed

        def output(i, computed):
            w[12 + i] = computed
        _poseidon_walk(F, w, sbox_in, output)
