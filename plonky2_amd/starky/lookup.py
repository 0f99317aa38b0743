"""Host-side mirror of starky/src/lookup.rs: Column, Filter, Lookup and GrandProductChallenge as the caller writes them, their
flat form for the library (the p2hot_stark_* descriptors of include/p2hot.h), and lookup_helper_columns for every lookup and
challenge as one p2hot_stark_lookup_polys call.  Marshalling only: nothing is evaluated here."""
import ctypes as C

import numpy as np

from .. import _lib
from ..engine import default_engine

P = 0xFFFFFFFF00000001


class Column:
    """lookup.rs:137-141: sum of coeff * current-row column, sum of coeff * next-row column, a constant"""

    def __init__(self, linear_combination=(), next_row_linear_combination=(), constant=0):
        self.linear_combination = [(int(c), int(f) % P) for c, f in linear_combination]
        self.next_row_linear_combination = [(int(c), int(f) % P) for c, f in next_row_linear_combination]
        self.constant_term = int(constant) % P

    @classmethod
    def single(cls, c):
        return cls([(c, 1)])

    @classmethod
    def single_next_row(cls, c):
        return cls([], [(c, 1)])

    @classmethod
    def constant(cls, constant):
        return cls([], [], constant)

    @classmethod
    def linear_combination_with_constant(cls, it, constant):
        v = list(it)
        if not v or len({c for c, _ in v}) != len(v):  # lookup.rs:201-210
            raise ValueError("a linear combination needs at least one column and no column twice")
        return cls(v, [], constant)

    @classmethod
    def linear_combination_and_next_row_with_constant(cls, it, next_row_it, constant):
        v, nv = list(it), list(next_row_it)
        if (not v and not nv) or len({c for c, _ in v}) != len(v) or len({c for c, _ in nv}) != len(nv):  # lookup.rs:228-244
            raise ValueError("a linear combination needs at least one column and no column twice per row")
        return cls(v, nv, constant)

    @classmethod
    def le_bits(cls, cs):
        return cls.linear_combination_with_constant([(c, pow(2, k, P)) for k, c in enumerate(cs)], 0)

    @classmethod
    def sum(cls, cs):
        return cls.linear_combination_with_constant([(c, 1) for c in cs], 0)


class Filter:
    """lookup.rs:37-40: sum of products of two columns plus a sum of columns; the default filter is the constant 1"""

    def __init__(self, products=(), constants=None):
        self.products = [(a, b) for a, b in products]
        self.constants = [Column.constant(1)] if constants is None and not self.products else list(constants or [])

    @classmethod
    def new_simple(cls, col):
        return cls([], [col])


class Lookup:
    """lookup.rs:415-429"""

    def __init__(self, columns, table_column, frequencies_column, filter_columns=None):
        self.columns = list(columns)
        self.table_column, self.frequencies_column = table_column, frequencies_column
        self.filter_columns = list(filter_columns) if filter_columns is not None else [Filter() for _ in self.columns]
        if len(self.filter_columns) != len(self.columns):  # lookup.rs:585
            raise ValueError("one filter per looking column")

    def num_helper_columns(self, constraint_degree):
        """lookup.rs:433-441: the helper columns and Z"""
        return -(-len(self.columns) // chunk_size(constraint_degree)) + 1


class GrandProductChallenge:
    """lookup.rs:446-451"""

    def __init__(self, beta, gamma):
        self.beta, self.gamma = int(beta) % P, int(gamma) % P


def chunk_size(constraint_degree):
    """constraint_degree.checked_sub(1).unwrap_or(1) (lookup.rs:439, :670, :755)"""
    return constraint_degree - 1 if constraint_degree >= 1 else 1


class DescriptorTables:
    """Columns, filters and looking entries collected into the flat arrays of p2hot_stark_tables; `struct()` is what the
    library takes (the arrays live as long as this object)"""

    def __init__(self):
        self.terms, self.columns, self.products, self.constants, self.filters, self.looking = [], [], [], [], [], []
        self._keep = None

    def add_column(self, col):
        first = len(self.terms)
        self.terms += [(c, 0, f) for c, f in col.linear_combination] + [(c, 1, f) for c, f in col.next_row_linear_combination]
        self.columns.append((first, len(self.terms) - first, col.constant_term))
        return len(self.columns) - 1

    def add_columns(self, cols):
        """consecutive ids; returns the first"""
        ids = [self.add_column(c) for c in cols]
        return ids[0] if ids else len(self.columns)

    def add_filter(self, flt):
        fp, fc = len(self.products), len(self.constants)
        for a, b in flt.products:
            self.products.append((self.add_column(a), self.add_column(b)))
        self.constants += [self.add_column(c) for c in flt.constants]
        self.filters.append((fp, len(self.products) - fp, fc, len(self.constants) - fc))
        return len(self.filters) - 1

    def add_lookup(self, lookup):
        first_col = self.add_columns(lookup.columns)
        flt = [self.add_filter(f) for f in lookup.filter_columns]
        assert flt == list(range(flt[0], flt[0] + len(flt))) if flt else True
        return _lib.StarkLookup(first_col, len(lookup.columns), flt[0] if flt else len(self.filters), self.add_column(lookup.table_column),
                                self.add_column(lookup.frequencies_column))

    def add_looking(self, columns, flt):
        first_col = self.add_columns(columns)
        self.looking.append((first_col, len(columns), self.add_filter(flt)))
        return len(self.looking) - 1

    def struct(self):
        def arr(ctype, rows):
            return (ctype * max(len(rows), 1))(*[ctype(*r) for r in rows])
        terms, columns = arr(_lib.StarkTerm, self.terms), arr(_lib.StarkColumn, self.columns)
        products = (C.c_uint32 * max(2 * len(self.products), 1))(*[v for p in self.products for v in p])
        constants = (C.c_uint32 * max(len(self.constants), 1))(*self.constants)
        filters, looking = arr(_lib.StarkFilter, self.filters), arr(_lib.StarkLooking, self.looking)
        t = _lib.StarkTables(C.cast(terms, C.POINTER(_lib.StarkTerm)), C.cast(columns, C.POINTER(_lib.StarkColumn)),
                             C.cast(products, C.POINTER(C.c_uint32)), C.cast(constants, C.POINTER(C.c_uint32)),
                             C.cast(filters, C.POINTER(_lib.StarkFilter)), C.cast(looking, C.POINTER(_lib.StarkLooking)), len(self.terms),
                             len(self.columns), len(self.products), len(self.constants), len(self.filters), len(self.looking))
        self._keep = (terms, columns, products, constants, filters, looking, t)
        return t


def raise_reference_panics(eng, rc):
    """the reference panics where the library returns P2HOT_EINVAL with these texts (field/src/types.rs:133, polynomial/mod.rs:164-178)"""
    if rc == _lib.EINVAL:
        text = eng.lib.p2hot_last_error(eng._ctx)
        if b"Tried to invert zero" in text or b"Quotient has failed" in text:
            raise ValueError(text.decode())
    eng.check(rc)


def marshal_lookups(tables, lookups):
    descs = [tables.add_lookup(lk) for lk in lookups]
    return (_lib.StarkLookup * max(len(descs), 1))(*descs)


def lookup_helper_columns(trace, lookups, challenges, constraint_degree, want_host=False, engine=None):
    """lookup_helper_columns (lookup.rs:579-652) for every lookup and every challenge in the order of prover.rs:177-195 -- one
    p2hot_stark_lookup_polys call.  trace: [W][n] host ndarray or DeviceColumns.  Returns DeviceColumns: per lookup, per challenge,
    the helper columns, then Z (and the same as a host array when want_host)."""
    from ..fri.oracle import DeviceColumns
    eng = engine or default_engine()
    dt = trace if isinstance(trace, DeviceColumns) else DeviceColumns.upload(eng.host(trace), eng)
    tables = DescriptorTables()
    descs = marshal_lookups(tables, lookups)
    ch = np.ascontiguousarray(np.asarray([int(c) % P for c in challenges], dtype=np.uint64))
    out = None
    if want_host:
        rows = sum(len(ch) * lk.num_helper_columns(constraint_degree) for lk in lookups) if constraint_degree != 1 else 0
        out = np.zeros((rows, 1 << dt.degree_log), dtype=np.uint64)
    h = C.c_void_p()
    t = tables.struct()
    rc = eng.lib.p2hot_stark_lookup_polys(eng.ctx, dt._h, C.byref(t), descs, len(lookups), ch.ctypes.data_as(C.c_void_p), len(ch), constraint_degree,
                                          out.ctypes.data_as(C.c_void_p) if out is not None else None, C.byref(h))
    raise_reference_panics(eng, rc)
    cols = DeviceColumns(eng, h)
    return (cols, out) if want_host else cols
