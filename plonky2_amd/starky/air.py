"""A STARK's own constraints as a constraint program (include/p2hot.h, "constraint program"; csrc/air.hpp interprets it).

AirBuilder traces a constraint function -- the body of a Stark::eval_packed_generic, written against `local_values`, `next_values`,
`public_inputs` and the four methods of ConstraintConsumer (starky/src/constraint_consumer.rs:62-85) -- into a straight-line
program; `build()` assigns temp slots by last use and marshals it.  Tracing and marshalling only: nothing is evaluated here, and
nothing is folded or shared (a subexpression written twice is computed twice)."""
import ctypes as C

from .. import _lib

P = 0xFFFFFFFF00000001
LOCAL, NEXT, PUBLIC, CONST, TEMP = range(5)
ADD, SUB, MUL, CONSTRAINT, CONSTRAINT_TRANSITION, CONSTRAINT_FIRST_ROW, CONSTRAINT_LAST_ROW = range(7)
KIND_SHIFT = 29
INDEX_MASK = (1 << KIND_SHIFT) - 1


def operand(kind, index):
    """P2HOT_AIR_OPERAND"""
    if not 0 <= index <= INDEX_MASK:
        raise ValueError("operand index %d does not fit 29 bits" % index)
    return (kind << KIND_SHIFT) | index


class Value:
    """a symbolic field element of one builder: a frame value, a public input, a constant or the result of an instruction"""
    __slots__ = ("builder", "leaf", "node")

    def __init__(self, builder, leaf=None, node=None):
        self.builder, self.leaf, self.node = builder, leaf, node

    def __add__(self, other):
        return self.builder._arith(ADD, self, other)

    def __radd__(self, other):
        return self.builder._arith(ADD, other, self)

    def __sub__(self, other):
        return self.builder._arith(SUB, self, other)

    def __rsub__(self, other):
        return self.builder._arith(SUB, other, self)

    def __mul__(self, other):
        return self.builder._arith(MUL, self, other)

    def __rmul__(self, other):
        return self.builder._arith(MUL, other, self)

    def __neg__(self):
        return self.builder._arith(SUB, 0, self)


class Program:
    """a built program: `insns` [(op, dst, a, b)], `constants` [int], the counts, and `struct()` for the library (the arrays live
    as long as this object)"""

    def __init__(self, insns, constants, num_temps, num_publics, width):
        self.insns, self.constants = [tuple(int(v) for v in i) for i in insns], [int(c) for c in constants]
        self.num_temps, self.num_publics, self.width = num_temps, num_publics, width
        self._keep = None

    def struct(self):
        insns = (_lib.AirInsn * max(len(self.insns), 1))(*[_lib.AirInsn(*i) for i in self.insns])
        consts = (C.c_uint64 * max(len(self.constants), 1))(*self.constants)
        s = _lib.AirProgram(C.cast(insns, C.POINTER(_lib.AirInsn)), C.cast(consts, C.POINTER(C.c_uint64)), len(self.insns), len(self.constants),
                            self.num_temps, self.num_publics)
        self._keep = (insns, consts, s)
        return s


class AirBuilder:
    def __init__(self, width, num_publics=0):
        self.width, self.num_publics = int(width), int(num_publics)
        self.local_values = [Value(self, leaf=(LOCAL, c)) for c in range(self.width)]
        self.next_values = [Value(self, leaf=(NEXT, c)) for c in range(self.width)]
        self.public_inputs = [Value(self, leaf=(PUBLIC, k)) for k in range(self.num_publics)]
        self.constants, self._const_index = [], {}
        self._ops = []  # in program order: (op, a, b) with a, b Values; the consuming ops have b = None

    def constant(self, v):
        v = int(v) % P
        if v not in self._const_index:
            self._const_index[v] = len(self.constants)
            self.constants.append(v)
        return Value(self, leaf=(CONST, self._const_index[v]))

    def _value(self, v):
        if isinstance(v, Value):
            if v.builder is not self:
                raise ValueError("a value of another AirBuilder")
            return v
        if isinstance(v, bool) or not hasattr(v, "__index__"):
            raise TypeError("constraint programs combine traced values and Python ints, not %r" % type(v).__name__)
        return self.constant(v)

    def _arith(self, op, a, b):
        a, b = self._value(a), self._value(b)
        self._ops.append((op, a, b))
        return Value(self, node=len(self._ops) - 1)

    def _consume(self, op, c):
        self._ops.append((op, self._value(c), None))

    # ConstraintConsumer (constraint_consumer.rs:62-85)
    def constraint(self, c):
        self._consume(CONSTRAINT, c)

    def constraint_transition(self, c):
        self._consume(CONSTRAINT_TRANSITION, c)

    def constraint_first_row(self, c):
        self._consume(CONSTRAINT_FIRST_ROW, c)

    def constraint_last_row(self, c):
        self._consume(CONSTRAINT_LAST_ROW, c)

    @property
    def num_constraints(self):
        return sum(1 for op, _, _ in self._ops if op >= CONSTRAINT)

    def build(self):
        """The marshalled program.  Results no constraint depends on are left out; a temp slot is taken by the lowest free one
        when its instruction runs and is free again after the last instruction that reads it (that instruction's own result may
        take it: the interpreter reads both operands before it writes)."""
        ops = self._ops
        live = [op >= CONSTRAINT for op, _, _ in ops]
        last_use = [-1] * len(ops)
        for t in range(len(ops) - 1, -1, -1):
            if not live[t]:
                continue
            for v in ops[t][1:]:
                if v is not None and v.node is not None:
                    live[v.node] = True
                    last_use[v.node] = max(last_use[v.node], t)
        slot, free, num_temps, insns = {}, [], 0, []

        def enc(v):
            return operand(*v.leaf) if v.leaf is not None else operand(TEMP, slot[v.node])
        for t, (op, a, b) in enumerate(ops):
            if not live[t]:
                continue
            ea, eb = enc(a), enc(b) if b is not None else 0
            for v in {v.node for v in (a, b) if v is not None and v.node is not None}:
                if last_use[v] == t:
                    free.append(slot[v])
            dst = 0
            if op < CONSTRAINT:
                if free:
                    dst = min(free)
                    free.remove(dst)
                else:
                    dst, num_temps = num_temps, num_temps + 1
                slot[t] = dst
            insns.append((op, dst, ea, eb))
        return Program(insns, self.constants, num_temps, self.num_publics, self.width)


def trace_constraints(fn, width, num_publics=0):
    """fn(local_values, next_values, public_inputs, consumer) traced over a fresh AirBuilder (the builder is the consumer)"""
    b = AirBuilder(width, num_publics)
    fn(b.local_values, b.next_values, b.public_inputs, b)
    return b.build()
