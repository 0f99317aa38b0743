"""The gate-program interpreter (gate_program.hpp) in the code object inside plonky2_amd/libp2hot.so (tools/codeobj.py, the pattern of
tests/test_stark_air_codeobj.py): one kernel per NC, no scratch, nothing spilled, no static LDS.  The register counts are not pinned
here (DESIGN.md records them).  Also: the Rust and ctypes mirrors of p2hot_gate_program and the new operand kind."""
import ctypes as C
import os
import re

import pytest

from tests.conftest import ROOT

SO = os.path.join(ROOT, "plonky2_amd", "libp2hot.so")


@pytest.fixture(scope="module")
def md():
    if not os.path.exists(SO):
        pytest.skip("plonky2_amd/libp2hot.so has not been built (python -c 'import __graft_entry__ as g; g.build()')")
    from tools import codeobj
    return codeobj.kernel_metadata(SO)


def test_gate_program_kernels_use_no_scratch_and_spill_nothing(md):
    mine = sorted(n for n in md if n.startswith("_ZN8gateprog"))
    assert len(mine) == 4 and all("interp_kernel" in n for n in mine), mine
    assert [re.search(r"ILi(\d)E", n).group(1) for n in mine] == ["1", "2", "3", "4"], mine
    for n in mine:
        k = md[n]
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
        assert k[".vgpr_spill_count"] == 0, n
        assert k.get(".sgpr_spill_count", 0) == 0, (n, k.get(".sgpr_spill_count"))
        assert k[".group_segment_fixed_size"] == 0, n  # the temp file is the launch's dynamic LDS: num_temps * 256 * 8 bytes


def test_gate_program_struct_has_a_repr_c_mirror():
    """p2hot_gate_program of the header against integration/p2hot.rs, field by field"""
    from tests.test_integration_files import _camel, _rust_type
    cname = "p2hot_gate_program"
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p2hot.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "integration", "p2hot.rs")).read()
    body = re.search(r"typedef struct %s \{(.*?)\}\s*%s\s*;" % (cname, cname), h, flags=re.S).group(1)
    fields = []
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        base, rest = re.match(r"((?:const\s+)?[A-Za-z_]\w*)\s*(.*)$", decl, flags=re.S).groups()
        for item in [x.strip() for x in rest.split(",")]:
            fields.append((item.replace("*", "").strip(), _rust_type(base + " *" * item.count("*"))))
    assert fields == [("row", "u32"), ("selector_index", "u32"), ("group_first", "u32"), ("group_end", "u32"), ("program", "P2hotAirProgram")]
    m = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^\)]*\)\]\s*)?pub struct %s \{(.*?)\n\}" % _camel(cname), rs, flags=re.S)
    assert m, _camel(cname)
    assert [(a, " ".join(b.split())) for a, b in re.findall(r"pub (\w+): ([^,]+),", m.group(1))] == fields
    assert "pub const P2HOT_AIR_GATE_CONST: u32 = 5;" in rs


def test_ctypes_mirror_matches_the_header():
    from plonky2_amd import _lib
    from plonky2_amd.plonk import gate_program as gp
    assert [name for name, _ in _lib.GateProgram._fields_] == ["row", "selector_index", "group_first", "group_end", "program"]
    assert all(t is C.c_uint32 for _, t in _lib.GateProgram._fields_[:4]) and _lib.GateProgram._fields_[4][1] is _lib.AirProgram
    assert C.sizeof(_lib.GateProgram) == 4 * 4 + C.sizeof(_lib.AirProgram) and _lib.GateProgram.program.offset == 16
    h = open(os.path.join(ROOT, "include", "p2hot.h")).read()
    assert "#define P2HOT_AIR_GATE_CONST 5u\n" in h and gp.GATE_CONST == 5
    for name in ("p2hot_gate_sums_programs", "p2hot_quotient_polys_gate_programs", "p2hot_quotient_polys_lookup_gate_programs"):
        base = name.replace("_programs", "").replace("polys_gate", "polys_gates").replace("lookup_gate", "lookup_gates")
        assert _lib.SIGNATURES[name] == (_lib.SIGNATURES[base][0], _lib.SIGNATURES[base][1] + [_lib.vp, _lib.u]), name
