"""The batch FRI kernels (fri.hpp: fold_join_kernel, batch_rows_kernel, batch_paths_kernel) and the digest-prefixed reader's
instantiations of the three leaf kernels (merkle.hpp) in the code object inside plonky2_amd/libp2hot.so (tools/codeobj.py, the
pattern of tests/test_gates_codeobj.py): no scratch, nothing spilled.  The register counts are not pinned here (DESIGN.md records
them).  Also: the Rust mirror of p2hot_fri_instance, field by field."""
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


def test_batch_fri_kernels_use_no_scratch_and_spill_nothing(md):
    new = [n for n in md if any(k in n for k in ("fold_join_kernel", "batch_rows_kernel", "batch_paths_kernel"))]
    assert len(new) == 3, new
    readers = [n for n in md if "DigestPrefixedReader" in n]
    # the word-per-lane, quad and lane-per-leaf mappings, and nothing else (no Keccak or chunked instantiation of this reader)
    assert sorted(re.search(r"\d+(hash_leaves\w*?kernel)", n).group(1) for n in readers) == ["hash_leaves_kernel", "hash_leaves_quad_kernel",
                                                                                            "hash_leaves_row_kernel"], readers
    for n in new + readers:
        k = md[n]
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
        assert k[".vgpr_spill_count"] == 0, n
        # the lane-per-leaf Poseidon stream parks round constants in VGPR lanes by design: the bound tests/test_codeobj.py sets for
        # the same stream under ColMajorReader; every other kernel here keeps its scalars in registers
        assert k.get(".sgpr_spill_count", 0) <= (96 if "18hash_leaves_kernel" in n else 0), (n, k.get(".sgpr_spill_count"))


def test_existing_readers_kept_their_kernels(md):
    """the new reader is an additional instantiation: the plain commit's leaf kernels are still there, one of each"""
    for kern in ("18hash_leaves_kernel", "23hash_leaves_quad_kernel", "22hash_leaves_row_kernel"):
        for rd in ("ColMajorReader", "RowMajorReader", "FriPlanarReader"):
            assert len([n for n in md if kern in n and rd in n]) == 1, (kern, rd)


def test_fri_instance_struct_has_a_repr_c_mirror():
    """p2hot_fri_instance (a tagged struct in the header) against integration/p2hot.rs"""
    from tests.test_integration_files import _camel, _rust_type
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p2hot.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "integration", "p2hot.rs")).read()
    body = re.search(r"typedef struct p2hot_fri_instance \{(.*?)\}\s*p2hot_fri_instance\s*;", h, flags=re.S).group(1)
    fields = []
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        base, rest = re.match(r"((?:const\s+)?[A-Za-z_]\w*)\s*(.*)$", decl, flags=re.S).groups()
        for item in [x.strip() for x in rest.split(",")]:
            fields.append((item.replace("*", "").strip(), _rust_type(base + " *" * item.count("*"))))
    m = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^\)]*\)\]\s*)?pub struct %s \{(.*?)\n\}" % _camel("p2hot_fri_instance"), rs, flags=re.S)
    assert m, "P2hotFriInstance"
    assert [(a, " ".join(b.split())) for a, b in re.findall(r"pub (\w+): ([^,]+),", m.group(1))] == fields
    assert re.search(r"pub struct P2hotBatchOracle\b", rs)
