"""The register budget of the Keccak FRI kernels (fri.hpp, suffix _k256), read from the code object inside
plonky2_amd/libp2hot.so (tools/codeobj.py, the pattern of tests/test_keccak_codeobj.py): the challenger, the round trees' leaf
kernel and the grind spill nothing and use no scratch memory; the two throughput kernels keep four waves per SIMD."""
import os

import pytest

from tests.conftest import ROOT

SO = os.path.join(ROOT, "plonky2_amd", "libp2hot.so")


@pytest.fixture(scope="module")
def md():
    if not os.path.exists(SO):
        pytest.skip("plonky2_amd/libp2hot.so has not been built (python -c 'import __graft_entry__ as g; g.build()')")
    from tools import codeobj
    return codeobj.kernel_metadata(SO)


def test_keccak_fri_kernels_use_no_scratch(md):
    from tools import codeobj
    names = [n for n in md if "_k256" in n]
    assert len(names) == 3, names
    for kernel in ("challenger_kernel_k256", "round_leaves_kernel_k256", "pow_kernel_k256"):
        assert sum(kernel in n for n in names) == 1, (kernel, names)
    for n in names:
        k = md[n]
        assert k[".vgpr_spill_count"] == 0 and k.get(".sgpr_spill_count", 0) == 0, n
        assert k[".private_segment_fixed_size"] == 0, n
        if "challenger" not in n:  # one candidate / one leaf per lane: occupancy hides the latency of the dependent rounds
            assert k[".vgpr_count"] <= 128 and codeobj.waves_per_simd(k[".vgpr_count"], 256) >= 4, n
