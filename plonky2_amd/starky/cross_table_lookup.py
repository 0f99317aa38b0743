"""Host-side mirror of starky/src/cross_table_lookup.rs: TableWithColumns, CrossTableLookup, CtlZData, the per-table grouping of
cross_table_lookup_data (host bookkeeping) with one p2hot_stark_ctl_polys call per table, and get_ctl_auxiliary_polys."""
import ctypes as C

import numpy as np

from .. import _lib
from ..engine import default_engine
from .lookup import DescriptorTables, GrandProductChallenge, chunk_size, raise_reference_panics


class TableWithColumns:
    """cross_table_lookup.rs:67-71"""

    def __init__(self, table, columns, flt):
        self.table, self.columns, self.filter = table, list(columns), flt


class CrossTableLookup:
    """cross_table_lookup.rs:87-108"""

    def __init__(self, looking_tables, looked_table):
        if any(len(t.columns) != len(looked_table.columns) for t in looking_tables):
            raise ValueError("all tables of a cross-table lookup have the same width")
        self.looking_tables, self.looked_table = list(looking_tables), looked_table


class CtlZData:
    """cross_table_lookup.rs:155-167.  helper_columns / z: (DeviceColumns, column index) into the table's CtlData.polys once
    cross_table_lookup_data has run; z_first: Z[0] (StarkOpeningSet::ctl_zs_first)"""

    def __init__(self, challenge, columns, filters, helper_columns=None, z=None, z_first=None):
        self.challenge, self.columns, self.filter = challenge, [list(c) for c in columns], list(filters)
        self.helper_columns, self.z, self.z_first = helper_columns or [], z, z_first

    def num_helpers(self, constraint_degree):
        """partial_sums (cross_table_lookup.rs:407-411): none for a single (columns, filter)"""
        return -(-len(self.columns) // chunk_size(constraint_degree)) if len(self.columns) > 1 else 0


class CtlData:
    """cross_table_lookup.rs:146-149 with the polynomials where the library left them: polys = DeviceColumns in
    get_ctl_auxiliary_polys' order (all helper columns, then all Zs), or None for a table without CTLs"""

    def __init__(self):
        self.zs_columns, self.polys = [], None

    def num_ctl_helper_polys(self):
        return [len(z.helper_columns) for z in self.zs_columns]


def marshal_ctl_zs(tables, zs_columns):
    """CtlZData -> p2hot_stark_ctl_z, the looking entries into `tables`"""
    descs = []
    for z in zs_columns:
        ids = [tables.add_looking(cols, flt) for cols, flt in zip(z.columns, z.filter)]
        descs.append(_lib.StarkCtlZ(ids[0] if ids else len(tables.looking), len(ids), z.challenge.beta, z.challenge.gamma))
    return (_lib.StarkCtlZ * max(len(descs), 1))(*descs)


def ctl_polys(trace, zs_columns, constraint_degree, want_host=False, engine=None):
    """partial_sums (cross_table_lookup.rs:383-414) for every Z of one table -- one p2hot_stark_ctl_polys call.  Returns
    (DeviceColumns in get_ctl_auxiliary_polys' order, zs_first[, the same columns on the host])."""
    from ..fri.oracle import DeviceColumns
    eng = engine or default_engine()
    dt = trace if isinstance(trace, DeviceColumns) else DeviceColumns.upload(eng.host(trace), eng)
    tables = DescriptorTables()
    descs = marshal_ctl_zs(tables, zs_columns)
    firsts = np.zeros(max(len(zs_columns), 1), dtype=np.uint64)
    out = None
    if want_host:
        rows = sum(z.num_helpers(constraint_degree) + 1 for z in zs_columns) if constraint_degree != 1 else 0
        out = np.zeros((rows, 1 << dt.degree_log), dtype=np.uint64)
    h = C.c_void_p()
    t = tables.struct()
    rc = eng.lib.p2hot_stark_ctl_polys(eng.ctx, dt._h, C.byref(t), descs, len(zs_columns), constraint_degree,
                                       out.ctypes.data_as(C.c_void_p) if out is not None else None, C.byref(h), firsts.ctypes.data_as(C.c_void_p))
    raise_reference_panics(eng, rc)
    cols = DeviceColumns(eng, h)
    firsts = firsts[:len(zs_columns)]
    return (cols, firsts, out) if want_host else (cols, firsts)


def cross_table_lookup_data(traces, cross_table_lookups, ctl_challenges, constraint_degree, engine=None):
    """cross_table_lookup_data (cross_table_lookup.rs:270-339): which Z belongs to which table is decided here, on the host, in
    the reference's order -- per CTL, per challenge, the looking tables grouped by consecutive equal table index (group_by,
    :349), then the looked table -- and every table's polynomials come from one library call.
    traces: per table [W][n] (host ndarray or DeviceColumns); ctl_challenges: GrandProductChallenges.  Returns [CtlData] per table."""
    data = [CtlData() for _ in traces]
    for ctl in cross_table_lookups:
        for ch in ctl_challenges:
            groups = []
            for lt in ctl.looking_tables:  # Itertools::group_by: consecutive runs
                if groups and groups[-1][0] == lt.table:
                    groups[-1][1].append(lt)
                else:
                    groups.append((lt.table, [lt]))
            for table, members in groups:
                # (the reference records the looking tables of this index from the whole list (:300-316) and sums over the run
                # (:354-364); the two agree whenever a table's entries are adjacent, the only layout it proves)
                data[table].zs_columns.append(CtlZData(ch, [m.columns for m in members], [m.filter for m in members]))
            lk = ctl.looked_table
            data[lk.table].zs_columns.append(CtlZData(ch, [lk.columns], [lk.filter]))
    for table, d in enumerate(data):
        if not d.zs_columns:
            continue
        d.polys, firsts = ctl_polys(traces[table], d.zs_columns, constraint_degree, engine=engine)
        total = sum(z.num_helpers(constraint_degree) for z in d.zs_columns)
        at = 0
        for k, z in enumerate(d.zs_columns):
            nh = z.num_helpers(constraint_degree)
            z.helper_columns = [(d.polys, at + j) for j in range(nh)]
            z.z, z.z_first = (d.polys, total + k), int(firsts[k])
            at += nh
    return data


def get_ctl_auxiliary_polys(ctl_data):
    """cross_table_lookup.rs:253-261: all helper columns, then all Zs -- the order the library wrote them in"""
    return None if ctl_data is None else ctl_data.polys


__all__ = ["TableWithColumns", "CrossTableLookup", "CtlZData", "CtlData", "GrandProductChallenge", "cross_table_lookup_data",
           "get_ctl_auxiliary_polys", "ctl_polys"]
