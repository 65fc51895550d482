"""CPU: the group-photograph kernels (csrc/gcfr_fullres_group.hip) in the built library carry no private segment and no LDS.  The
composite walks a photograph's face slots from its argument block and keeps the running bytes in its output, read back by the
lane that stored them: neither a per-lane array indexed by the slot nor a staging buffer exists to become scratch or LDS.  Read
from the code objects' notes, as tests/test_fullres_anybox_resources.py reads the any-size kernels'.  The VGPR counts are printed
and recorded in DESIGN 4.17; no cap is set."""
import os

import pytest

from test_kernel_resources import LLVM, _kernel_metadata


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs the ROCm LLVM tools")
def test_the_group_kernels_have_no_scratch(tmp_path):
    k = {n: v for n, v in _kernel_metadata(tmp_path).items() if n.startswith("group_")}
    for n in sorted(k):
        print(n, k[n])
    assert sorted(k) == ["group_composites_kernel<false>", "group_composites_kernel<true>", "group_ingest_kernel"], sorted(k)
    for n, v in k.items():
        assert v["scratch"] == 0 and v["lds"] == 0, (n, v)
