"""A user-defined gate's constraints as a gate program (include/p2hot.h, "gate programs"; csrc/gate_program.hpp interprets it).

GateBuilder traces the body of a Gate::eval_unfiltered_base_one -- written against `wires` (vars.local_wires), `constants`
(vars.local_constants, the gate's own), `public_inputs_hash` and `constraint` -- into the straight-line program format of
starky/air.py: the same Value, the same tracing, the same slot assignment by last use.  The j-th `constraint` call is constraint j of
the gate.  ExtAlgebra writes a D = 2 extension-algebra gate over pairs of base values; GateProgram places one traced gate in
common_data.gates.  Tracing and marshalling only: nothing is evaluated here."""
import ctypes as C

from .. import _lib
from ..starky.air import AirBuilder, Program, Value

GATE_CONST = 5  # P2HOT_AIR_GATE_CONST: the operand kind a STARK's program may not use
W = 7           # F[X] / (X^2 - 7) (goldilocks_extensions.rs:19)


class GateBuilder:
    def __init__(self, num_wires, num_constants):
        self.num_wires, self.num_constants = int(num_wires), int(num_constants)
        self._air = AirBuilder(self.num_wires, 4)
        self.wires = self._air.local_values
        self.constants = [Value(self._air, leaf=(GATE_CONST, c)) for c in range(self.num_constants)]
        self.public_inputs_hash = self._air.public_inputs

    def constant(self, v):
        """a field constant of the program (not a gate constant: those are `constants[c]`)"""
        return self._air.constant(v)

    def constraint(self, expr):
        self._air.constraint(expr)

    @property
    def num_constraints(self):
        return self._air.num_constraints

    def build(self):
        return self._air.build()


class ExtAlgebra:
    """an element a0 + a1 X of the extension algebra over traced base values (ExtensionAlgebra<F, 2> in eval_unfiltered_base_one:
    two base wires), with +, -, * and scalar_mul"""
    __slots__ = ("a0", "a1")

    def __init__(self, a0, a1):
        self.a0, self.a1 = a0, a1

    @classmethod
    def from_wires(cls, wires, first):
        """vars.get_local_ext(first .. first + 2)"""
        return cls(wires[first], wires[first + 1])

    def __add__(self, other):
        return ExtAlgebra(self.a0 + other.a0, self.a1 + other.a1)

    def __sub__(self, other):
        return ExtAlgebra(self.a0 - other.a0, self.a1 - other.a1)

    def __mul__(self, other):
        return ExtAlgebra(self.a0 * other.a0 + W * (self.a1 * other.a1), self.a0 * other.a1 + self.a1 * other.a0)

    def scalar_mul(self, c):
        return ExtAlgebra(self.a0 * c, self.a1 * c)

    def to_basefield_array(self):
        return [self.a0, self.a1]


class GateProgram:
    """p2hot_gate_program: one traced gate as entry `row` of common_data.gates, group = selectors_info.groups[selector_index]"""

    def __init__(self, builder_or_program, row, selector_index, group):
        self.program = builder_or_program if isinstance(builder_or_program, Program) else builder_or_program.build()
        self.row, self.selector_index, self.group = int(row), int(selector_index), (int(group[0]), int(group[1]))

    def struct(self):
        return _lib.GateProgram(self.row, self.selector_index, self.group[0], self.group[1], self.program.struct())


def marshal(programs):
    """(array, count, keep) of a list of GateProgram for the three *_programs entry points; `keep` holds the arrays alive"""
    programs = list(programs or [])
    structs = [p.struct() for p in programs]
    array = (_lib.GateProgram * max(len(structs), 1))(*structs)
    return C.cast(array, C.c_void_p), len(structs), (array, structs, programs)
