"""The register budget of the Keccak kernels (keccak.hpp), read from the code object inside plonky2_amd/libp2hot.so
(tools/codeobj.py, the pattern of tests/test_codeobj.py): at least four waves per SIMD, nothing spilled, no scratch."""
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


def test_keccak_kernels_fit_four_waves_without_spills(md):
    from tools import codeobj
    names = [n for n in md if "keccak" in n]
    # the leaf sponge for both readers, the tree level and the byte-message primitive; no FRI-layout instantiation
    assert len(names) == 4 and not any("FriPlanarReader" in n for n in names), names
    for n in names:
        k = md[n]
        assert k[".vgpr_count"] <= 128 and k[".vgpr_spill_count"] == 0 and k.get(".sgpr_spill_count", 0) == 0, n
        assert k[".private_segment_fixed_size"] == 0, n
        assert codeobj.waves_per_simd(k[".vgpr_count"], 256) >= 4, n
