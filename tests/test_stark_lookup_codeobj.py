"""The starky lookup / cross-table-lookup kernels (stark.hpp) in the code object inside plonky2_amd/libp2hot.so (tools/codeobj.py,
the pattern of tests/test_batch_fri_codeobj.py): present, no scratch, nothing spilled.  The register counts are not pinned here
(DESIGN.md records them).  Also: the Rust mirrors of the p2hot_stark_* structs, field by field."""
import os
import re

import pytest

from tests.conftest import ROOT

SO = os.path.join(ROOT, "plonky2_amd", "libp2hot.so")
KERNELS = ["helper_rows_kernel", "increments_kernel", "scan_totals_kernel", "scan_carries_kernel", "scan_emit_kernel"]
STRUCTS = ["p2hot_stark_term", "p2hot_stark_column", "p2hot_stark_filter", "p2hot_stark_lookup", "p2hot_stark_looking", "p2hot_stark_ctl_z",
           "p2hot_stark_tables"]


@pytest.fixture(scope="module")
def md():
    if not os.path.exists(SO):
        pytest.skip("plonky2_amd/libp2hot.so has not been built (python -c 'import __graft_entry__ as g; g.build()')")
    from tools import codeobj
    return codeobj.kernel_metadata(SO)


def test_stark_kernels_use_no_scratch_and_spill_nothing(md):
    mine = [n for n in md if n.startswith("_ZN5stark")]
    for k in KERNELS:
        assert len([n for n in mine if k in n]) == 1, k
    terms = sorted(n for n in mine if "aux_terms_kernel" in n)
    assert len(terms) == 4 and [re.search(r"ILi(\d)E", n).group(1) for n in terms] == ["1", "2", "3", "4"], terms
    assert len(mine) == len(KERNELS) + 4, mine
    for n in mine:
        k = md[n]
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
        assert k[".vgpr_spill_count"] == 0, n
        assert k.get(".sgpr_spill_count", 0) == 0, (n, k.get(".sgpr_spill_count"))


@pytest.mark.parametrize("cname", STRUCTS)
def test_stark_structs_have_repr_c_mirrors(cname):
    """the tagged structs of the header against integration/p2hot.rs"""
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
    """plonky2_amd/_lib.py's Structures: the sizes the C layout gives (no padding surprises between u32 runs and u64s)"""
    import ctypes as C
    from plonky2_amd import _lib
    assert [C.sizeof(t) for t in (_lib.StarkTerm, _lib.StarkColumn, _lib.StarkFilter, _lib.StarkLookup, _lib.StarkLooking, _lib.StarkCtlZ)] == \
        [16, 16, 16, 20, 12, 24]
    assert C.sizeof(_lib.StarkTables) == 6 * C.sizeof(C.c_void_p) + 6 * 4
