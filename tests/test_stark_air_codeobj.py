"""The constraint-program interpreter (air.hpp) in the code object inside plonky2_amd/libp2hot.so (tools/codeobj.py, the pattern of
tests/test_stark_lookup_codeobj.py): one kernel per NC, no scratch, nothing spilled.  The register counts are not pinned here
(DESIGN.md records them).  Also: the Rust and ctypes mirrors of the p2hot_air_* structs."""
import ctypes as C
import os
import re

import pytest

from tests.conftest import ROOT

SO = os.path.join(ROOT, "plonky2_amd", "libp2hot.so")
STRUCTS = ["p2hot_air_insn", "p2hot_air_program"]


@pytest.fixture(scope="module")
def md():
    if not os.path.exists(SO):
        pytest.skip("plonky2_amd/libp2hot.so has not been built (python -c 'import __graft_entry__ as g; g.build()')")
    from tools import codeobj
    return codeobj.kernel_metadata(SO)


def test_air_kernels_use_no_scratch_and_spill_nothing(md):
    mine = sorted(n for n in md if n.startswith("_ZN3air"))
    assert len(mine) == 4 and all("eval_kernel" in n for n in mine), mine
    assert [re.search(r"ILi(\d)E", n).group(1) for n in mine] == ["1", "2", "3", "4"], mine
    for n in mine:
        k = md[n]
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
        assert k[".vgpr_spill_count"] == 0, n
        assert k.get(".sgpr_spill_count", 0) == 0, (n, k.get(".sgpr_spill_count"))
        assert k[".group_segment_fixed_size"] == 0, n  # the temp file is the launch's dynamic LDS: num_temps * 256 * 8 bytes


@pytest.mark.parametrize("cname", STRUCTS)
def test_air_structs_have_repr_c_mirrors(cname):
    """the tagged structs of the header against integration/p2hot.rs, field by field"""
    from tests.test_integration_files import _camel, _rust_type
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p2hot.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "integration", "p2hot.rs")).read()
    body = re.search(r"typedef struct %s \{(.*?)\}\s*%s\s*;" % (cname, cname), h, flags=re.S).group(1)
    fields = []
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        base, rest = re.match(r"((?:const\s+)?[A-Za-z_]\w*)\s*(.*)$", decl, flags=re.S).groups()
        for item in [x.strip() for x in rest.split(",")]:
            fields.append((item.replace("*", "").strip(), _rust_type(base + " *" * item.count("*"))))
    m = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^\)]*\)\]\s*)?pub struct %s \{(.*?)\n\}" % _camel(cname), rs, flags=re.S)
    assert m, _camel(cname)
    assert [(a, " ".join(b.split())) for a, b in re.findall(r"pub (\w+): ([^,]+),", m.group(1))] == fields


def test_ctypes_mirrors_match_the_header_sizes():
    from plonky2_amd import _lib
    from plonky2_amd.starky import air
    assert C.sizeof(_lib.AirInsn) == 16
    assert C.sizeof(_lib.AirProgram) == 2 * C.sizeof(C.c_void_p) + 4 * 4
    assert [name for name, _ in _lib.AirInsn._fields_] == ["op", "dst", "a", "b"]
    h = open(os.path.join(ROOT, "include", "p2hot.h")).read()
    for name in ("LOCAL", "NEXT", "PUBLIC", "CONST", "TEMP", "ADD", "SUB", "MUL", "CONSTRAINT", "CONSTRAINT_TRANSITION", "CONSTRAINT_FIRST_ROW",
                 "CONSTRAINT_LAST_ROW"):
        assert "#define P2HOT_AIR_%s %du\n" % (name, getattr(air, name)) in h, name
    assert air.operand(air.TEMP, 5) == (4 << 29) | 5
