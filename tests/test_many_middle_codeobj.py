"""The M-proof kernels of plonk.hpp, gates.hpp, gates_recursion.hpp and fri.hpp in the code object inside plonky2_amd/libp2hot.so
(tools/codeobj.py, the pattern of tests/test_gates_codeobj.py): every instantiation is there, uses no scratch and spills nothing.
The register counts are not pinned here (DESIGN.md records them)."""
import os

import pytest

from tests.conftest import ROOT

SO = os.path.join(ROOT, "plonky2_amd", "libp2hot.so")

# kernel name -> instantiations
EXPECTED = {"pp_quotients_many_kernel": 1, "pp_quotients2_many_kernel": 1, "pp_carries_many_kernel": 1, "many_gather_coeffs_kernel": 1,
            "any_nonzero_many_kernel": 1, "chunks_interleave_kernel": 1, "quotient_perm_many_kernel": 5, "cheap_gates_many_kernel": 4,
            "poseidon_gate_many_kernel": 4, "recursion_gates_many_kernel": 4, "mds_gate_many_kernel": 4, "ext_powers_many_kernel": 1,
            "eval_polys_dot_many_kernel": 1, "eval_polys_stage2_many_kernel": 1}


@pytest.fixture(scope="module")
def md():
    if not os.path.exists(SO):
        pytest.skip("plonky2_amd/libp2hot.so has not been built (python -c 'import __graft_entry__ as g; g.build()')")
    from tools import codeobj
    return codeobj.kernel_metadata(SO)


def test_many_kernels_use_no_scratch_and_spill_nothing(md):
    for kernel, count in EXPECTED.items():
        names = [n for n in md if kernel in n]
        assert len(names) == count, (kernel, names)
        for n in names:
            k = md[n]
            assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
            assert k[".vgpr_spill_count"] == 0 and k.get(".sgpr_spill_count", 0) == 0, n


def test_the_pipelined_quotient_instantiation_keeps_its_registers(md):
    """quotient_perm_many_kernel<2, 8> shares its body with quotient_perm_kernel<2, 8>, which is tuned to stream its loads: the
    per-proof values must not have moved into vector registers"""
    one = next(md[n] for n in md if "quotient_perm_kernel" in n and "Li2ELi8E" in n)
    many = next(md[n] for n in md if "quotient_perm_many_kernel" in n and "Li2ELi8E" in n)
    assert many[".vgpr_count"] <= one[".vgpr_count"], (many[".vgpr_count"], one[".vgpr_count"])
