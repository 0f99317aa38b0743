"""The M-proof kernels of the opening proof (fri.hpp) in the code object inside plonky2_amd/libp2hot.so (tools/codeobj.py, the
pattern of tests/test_many_middle_codeobj.py): every one is there once, uses no scratch and spills nothing.  The register counts
are not pinned here (DESIGN.md section 7 records them beside the single-proof kernels')."""
import os

import pytest

from tests.conftest import ROOT

SO = os.path.join(ROOT, "plonky2_amd", "libp2hot.so")

KERNELS = ["challenger_many_kernel", "challenger_copy_many_kernel", "fold_many_kernel", "interleave_many_kernel", "pow_many_kernel",
           "alpha_powers_many_kernel", "reduce_polys_base_many_kernel", "reduce_polys_base_small_many_kernel",
           "horner_chunk_totals_many_kernel", "horner_carries_many_kernel", "horner_group_walk_many_kernel", "horner_emit_many_kernel",
           "query_indices_many_kernel", "gather_rows_many_kernel", "merkle_paths_many_kernel"]


@pytest.fixture(scope="module")
def md():
    if not os.path.exists(SO):
        pytest.skip("plonky2_amd/libp2hot.so has not been built (python -c 'import __graft_entry__ as g; g.build()')")
    from tools import codeobj
    return codeobj.kernel_metadata(SO)


def test_fri_many_kernels_use_no_scratch_and_spill_nothing(md):
    for kernel in KERNELS:
        names = [n for n in md if kernel in n]
        assert len(names) == 1, (kernel, names)
        k = md[names[0]]
        assert k[".private_segment_fixed_size"] == 0, (kernel, k[".private_segment_fixed_size"])
        assert k[".vgpr_spill_count"] == 0 and k.get(".sgpr_spill_count", 0) == 0, kernel


def test_the_transcript_kernel_of_many_proofs_is_one_wave(md):
    """one transcript per 64-lane workgroup, as challenger_kernel"""
    one = next(md[n] for n in md if "challenger_kernel" in n and "k256" not in n)
    many = next(md[n] for n in md if "challenger_many_kernel" in n)
    assert many[".max_flat_workgroup_size"] == one[".max_flat_workgroup_size"] == 64
