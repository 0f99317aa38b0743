"""Gate programs (include/p2hot.h, "gate programs") restated for the tests of tests/test_gate_program.py.

  * `interpret`, `filtered_sums`: an interpreter of the gate-program format over Python ints, written from the header's text alone.  It
    shares no code with plonky2_amd.plonk.gate_program.GateBuilder or starky.air (the operand packing, the op numbers and the frame are
    restated here), and nothing here imports the library except the transcriptions' `ExtAlgebra` helper.
  * TRANSCRIPTIONS: nine gates of the reference written against a builder `b` (b.wires, b.constants, b.public_inputs_hash,
    b.constant, b.constraint) from their eval_unfiltered_base_one / _packed, line for line, with the descriptor of the hand-written
    kind that computes the same constraints.
  * the synthetic gate the library does not know -- a u32-style add with carry and a range check -- twice: `u32_add_gate(b)` for a
    builder and `u32_add_plain(w, c, pih)` as a plain function of ints."""
from tests import gates_ref as gr
from tests import recursion_gates_ref as rr

P = 0xFFFFFFFF00000001
# include/p2hot.h: operand kinds (top 3 bits of an operand, index in the low 29) and ops
K_LOCAL, K_NEXT, K_PUBLIC, K_CONST, K_TEMP, K_GATE_CONST = 0, 1, 2, 3, 4, 5
OP_ADD, OP_SUB, OP_MUL, OP_CONSTRAINT = 0, 1, 2, 3


# ------------------------------------------------------------------ the independent interpreter
def interpret(insns, constants, num_temps, w, c, pih):
    """the constraints of one gate at one point, in program order: w = the row's wires, c = the gate's own local constants (the
    selectors and lookup selectors removed), pih = the four words of public_inputs_hash; ints"""
    temps = [None] * num_temps

    def read(o):
        kind, idx = o >> 29, o & ((1 << 29) - 1)
        if kind == K_LOCAL:
            return int(w[idx]) % P
        if kind == K_GATE_CONST:
            return int(c[idx]) % P
        if kind == K_PUBLIC:
            return int(pih[idx]) % P
        if kind == K_CONST:
            return int(constants[idx]) % P
        assert kind == K_TEMP and temps[idx] is not None, (kind, idx)
        return temps[idx]
    out = []
    for op, dst, a, b in insns:
        if op == OP_CONSTRAINT:
            out.append(read(a))
            continue
        x, y = read(a), read(b)
        assert op in (OP_ADD, OP_SUB, OP_MUL), op
        temps[dst] = (x + y) % P if op == OP_ADD else (x - y) % P if op == OP_SUB else x * y % P
    return out


def filtered_sums(programs, num_selectors, num_lookup_selectors, w, constants, pih, alphas):
    """sum_g filter_g sum_j alpha^j c_{g,j} per alpha: programs = [(insns, program constants, num_temps, row, selector_index,
    (group_first, group_end))], `constants` = the whole constants row (selectors first)"""
    out = [0] * len(alphas)
    for insns, pconsts, num_temps, row, sel, group in programs:
        s = int(constants[sel])
        f = 1
        for k in range(group[0], group[1]):
            if k != row:
                f = f * (k - s) % P
        if num_selectors > 1:
            f = f * (0xFFFFFFFF - s) % P
        cons = interpret(insns, pconsts, num_temps, w, constants[num_selectors + num_lookup_selectors:], pih)
        for t, alpha in enumerate(alphas):
            out[t] = (out[t] + f * sum(v * pow(int(alpha), j, P) for j, v in enumerate(cons))) % P
    return out


# ------------------------------------------------------------------ transcriptions of reference gates
def constant_gate(b, num_consts):
    """constant.rs:120-128"""
    for i in range(num_consts):
        b.constraint(b.constants[i] - b.wires[i])


def public_input_gate(b):
    """public_input.rs:102-112"""
    for i in range(4):
        b.constraint(b.wires[i] - b.public_inputs_hash[i])


def arithmetic_gate(b, num_ops):
    """arithmetic_base.rs:167-184"""
    const_0, const_1 = b.constants[0], b.constants[1]
    for i in range(num_ops):
        multiplicand_0, multiplicand_1, addend, output = (b.wires[4 * i + t] for t in range(4))
        computed_output = multiplicand_0 * multiplicand_1 * const_0 + addend * const_1
        b.constraint(output - computed_output)


def arithmetic_extension_gate(b, num_ops):
    """arithmetic_extension.rs:92-110"""
    from plonky2_amd.plonk.gate_program import ExtAlgebra
    const_0, const_1 = b.constants[0], b.constants[1]
    for i in range(num_ops):
        multiplicand_0 = ExtAlgebra.from_wires(b.wires, 8 * i)
        multiplicand_1 = ExtAlgebra.from_wires(b.wires, 8 * i + 2)
        addend = ExtAlgebra.from_wires(b.wires, 8 * i + 4)
        output = ExtAlgebra.from_wires(b.wires, 8 * i + 6)
        computed_output = (multiplicand_0 * multiplicand_1).scalar_mul(const_0) + addend.scalar_mul(const_1)
        for v in (output - computed_output).to_basefield_array():
            b.constraint(v)


def mul_extension_gate(b, num_ops):
    """multiplication_extension.rs:86-101"""
    from plonky2_amd.plonk.gate_program import ExtAlgebra
    const_0 = b.constants[0]
    for i in range(num_ops):
        multiplicand_0 = ExtAlgebra.from_wires(b.wires, 6 * i)
        multiplicand_1 = ExtAlgebra.from_wires(b.wires, 6 * i + 2)
        output = ExtAlgebra.from_wires(b.wires, 6 * i + 4)
        computed_output = (multiplicand_0 * multiplicand_1).scalar_mul(const_0)
        for v in (output - computed_output).to_basefield_array():
            b.constraint(v)


def base_sum_gate(b, num_limbs, base):
    """base_sum.rs:153-170; reduce_with_powers is a Horner from the last limb"""
    total = b.wires[0]
    limbs = [b.wires[1 + k] for k in range(num_limbs)]
    computed_sum = b.constant(0)
    for limb in reversed(limbs):
        computed_sum = computed_sum * base + limb
    b.constraint(computed_sum - total)
    for limb in limbs:
        product = limb - 0
        for i in range(1, base):
            product = product * (limb - i)
        b.constraint(product)


def reducing_gate(b, num_coeffs):
    """reducing.rs:107-127"""
    from plonky2_amd.plonk.gate_program import ExtAlgebra
    alpha = ExtAlgebra.from_wires(b.wires, 2)
    old_acc = ExtAlgebra.from_wires(b.wires, 4)
    coeffs = [b.wires[6 + i] for i in range(num_coeffs)]
    start_accs = 6 + num_coeffs
    accs = [ExtAlgebra.from_wires(b.wires, 0 if i == num_coeffs - 1 else start_accs + 2 * i) for i in range(num_coeffs)]
    acc = old_acc
    for i in range(num_coeffs):
        for v in (acc * alpha + ExtAlgebra(coeffs[i], b.constant(0)) - accs[i]).to_basefield_array():
            b.constraint(v)
        acc = accs[i]


def exponentiation_gate(b, num_power_bits):
    """exponentiation.rs:210-243"""
    n = num_power_bits
    base = b.wires[0]
    power_bits = [b.wires[1 + i] for i in range(n)]
    intermediate_values = [b.wires[2 + n + i] for i in range(n)]
    output = b.wires[1 + n]
    for i in range(n):
        prev_intermediate_value = b.constant(1) if i == 0 else intermediate_values[i - 1] * intermediate_values[i - 1]
        cur_bit = power_bits[n - i - 1]
        not_cur_bit = 1 - cur_bit
        computed_intermediate_value = prev_intermediate_value * (cur_bit * base + not_cur_bit)
        b.constraint(computed_intermediate_value - intermediate_values[i])
    b.constraint(output - intermediate_values[n - 1])


def random_access_gate(b, bits, num_copies, num_extra_constants=0):
    """random_access.rs:302-343; wires as random_access.rs:144-175"""
    vec_size = 1 << bits
    stride = 2 + vec_size
    for copy in range(num_copies):
        access_index = b.wires[stride * copy]
        claimed_element = b.wires[stride * copy + 1]
        list_items = [b.wires[stride * copy + 2 + i] for i in range(vec_size)]
        bit_wires = [b.wires[stride * num_copies + num_extra_constants + copy * bits + i] for i in range(bits)]
        for bit in bit_wires:
            b.constraint(bit * (bit - 1))
        reconstructed_index = b.constant(0)
        for bit in reversed(bit_wires):
            reconstructed_index = reconstructed_index + reconstructed_index + bit
        b.constraint(reconstructed_index - access_index)
        for bit in bit_wires:
            list_items = [x + bit * (y - x) for x, y in zip(list_items[0::2], list_items[1::2])]
        assert len(list_items) == 1
        b.constraint(list_items[0] - claimed_element)
    for i in range(num_extra_constants):
        b.constraint(b.constants[i] - b.wires[stride * num_copies + i])


# name -> (transcription(b), (kind, param0, param1) of the hand-written gate, wires read, constants read)
TRANSCRIPTIONS = {
    "constant_2": (lambda b: constant_gate(b, 2), (gr.CONSTANT, 2, 0), 2, 2),
    "public_input": (public_input_gate, (gr.PUBLIC_INPUT, 0, 0), 4, 0),
    "arithmetic_20": (lambda b: arithmetic_gate(b, 20), (gr.ARITHMETIC, 20, 0), 80, 2),
    "arithmetic_ext_10": (lambda b: arithmetic_extension_gate(b, 10), (gr.ARITHMETIC_EXT, 10, 0), 80, 2),
    "mul_ext_13": (lambda b: mul_extension_gate(b, 13), (gr.MUL_EXT, 13, 0), 78, 1),
    "base_sum_2_4": (lambda b: base_sum_gate(b, 4, 2), (gr.BASE_SUM, 4, 2), 5, 0),
    "reducing_3": (lambda b: reducing_gate(b, 3), (rr.REDUCING, 3, 0), 13, 0),
    "exponentiation_3": (lambda b: exponentiation_gate(b, 3), (rr.EXPONENTIATION, 3, 0), 8, 0),
    "random_access_2_2": (lambda b: random_access_gate(b, 2, 2), (rr.RANDOM_ACCESS, 2, rr.ra_param1(2, 0)), 16, 0),
}


# ------------------------------------------------------------------ a gate the library does not know
U32_LIMBS = 20          # ternary limbs of the sum: 3^20 < 2^32 < 3^21 (a range check of degree 3, where base 4 would have degree 4)
U32_WIRES = 5 + U32_LIMBS
U32_CONSTRAINTS = 3 + U32_LIMBS


def u32_add_gate(b):
    """out + carry_out * c0 = x + y + carry_in + c1 * public_inputs_hash[2] (c0: the gate's modulus constant, c1: a per-row switch for
    an offset taken from the hash), carry_out boolean, out the sum of its ternary limbs, every limb in {0, 1, 2}.  Wires: x, y,
    carry_in, out, carry_out, then the limbs.  The limbs' first two range factors are all computed before any is consumed: twenty
    results are live at once."""
    x, y, carry_in, out, carry_out = b.wires[:5]
    limbs = [b.wires[5 + k] for k in range(U32_LIMBS)]
    c0, c1 = b.constants[0], b.constants[1]
    b.constraint(x + y + carry_in + c1 * b.public_inputs_hash[2] - out - carry_out * c0)
    b.constraint(carry_out * (carry_out - 1))
    partial = [limb * (limb - 1) for limb in limbs]
    total = b.constant(0)
    for limb in reversed(limbs):
        total = total * 3 + limb
    b.constraint(total - out)
    for limb, two in zip(limbs, partial):
        b.constraint(two * (limb - 2))


def u32_add_plain(w, c, pih):
    """the same gate as a function of ints"""
    x, y, carry_in, out, carry_out = (int(v) for v in w[:5])
    limbs = [int(v) for v in w[5:5 + U32_LIMBS]]
    cons = [(x + y + carry_in + int(c[1]) * int(pih[2]) - out - carry_out * int(c[0])) % P, carry_out * (carry_out - 1) % P,
            (sum(limb * 3 ** k for k, limb in enumerate(limbs)) - out) % P]
    return cons + [limb * (limb - 1) * (limb - 2) % P for limb in limbs]
