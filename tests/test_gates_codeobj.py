"""The gate kernels (gates.hpp) in the code object inside plonky2_amd/libp2hot.so (tools/codeobj.py, the pattern of
tests/test_keccak_codeobj.py): no scratch, nothing spilled, for every instantiation.  The register counts are not pinned here
(DESIGN.md records them).  Also: the Rust mirrors of the two gate structs of include/p2hot.h, field by field."""
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


def test_gate_kernels_use_no_scratch_and_spill_nothing(md):
    names = [n for n in md if "5gates" in n]       # namespace gates, mangled
    assert len([n for n in names if "cheap_gates_kernel" in n]) == 4 and len([n for n in names if "poseidon_gate_kernel" in n]) == 4, names
    for n in names:
        k = md[n]
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
        assert k[".vgpr_spill_count"] == 0 and k.get(".sgpr_spill_count", 0) == 0, n


def test_gate_structs_have_repr_c_mirrors():
    """p2hot_gate / p2hot_gate_set (tagged structs in the header) against integration/p2hot.rs"""
    from tests.test_integration_files import _camel, _rust_type
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p2hot.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "integration", "p2hot.rs")).read()
    for cname in ("p2hot_gate", "p2hot_gate_set"):
        body = re.search(r"typedef struct %s \{(.*?)\}\s*%s\s*;" % (cname, cname), h, flags=re.S).group(1)
        fields = []
        for decl in [d.strip() for d in body.split(";") if d.strip()]:
            base, rest = re.match(r"((?:const\s+)?[A-Za-z_]\w*)\s*(.*)$", decl, flags=re.S).groups()
            for item in [x.strip() for x in rest.split(",")]:
                nm = item.replace("*", "").strip()
                arr = re.search(r"\[(\d+)\]$", nm)
                fields.append((nm[:arr.start()], "[%s; %s]" % (_rust_type(base), arr.group(1))) if arr
                              else (nm, _rust_type(base + " *" * item.count("*"))))
        m = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^\)]*\)\]\s*)?pub struct %s \{(.*?)\n\}" % _camel(cname), rs, flags=re.S)
        assert m, cname
        assert [(a, " ".join(b.split())) for a, b in re.findall(r"pub (\w+): ([^,]+),", m.group(1))] == fields, cname
    for k, name in enumerate(("NOOP", "CONSTANT", "PUBLIC_INPUT", "ARITHMETIC", "ARITHMETIC_EXT", "MUL_EXT", "BASE_SUM", "POSEIDON")):
        assert re.search(r"pub const P2HOT_GATE_%s: u32 = %d;" % (name, k), rs), name
    order = re.search(r"enum \{(.*?)\}", h, flags=re.S).group(1)
    assert [x.strip() for x in order.split(",")] == ["P2HOT_GATE_" + n for n in ("NOOP", "CONSTANT", "PUBLIC_INPUT", "ARITHMETIC", "ARITHMETIC_EXT",
                                                                                 "MUL_EXT", "BASE_SUM", "POSEIDON")]
