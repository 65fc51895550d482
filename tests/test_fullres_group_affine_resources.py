"""CPU: the group-affine kernels (csrc/gcfr_fullres_group_affine.hip) in the built library carry no private segment and no LDS.  The
composite holds the carried x_lo of a lane's four pixels beside four affine carriers across its loop over the lights, and walks the
K x K sub-samples by run-time loops that recompute the taps from the indices: a spill, or a dynamically indexed per-lane array, would
have become scratch.  Read from the code objects' notes, as tests/test_kernel_resources.py reads the march kernels'.  The VGPR counts
are printed and recorded in DESIGN 4.19; no cap is set."""
import os

import pytest

from test_kernel_resources import LLVM, _kernel_metadata


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs the ROCm LLVM tools")
def test_the_group_affine_kernels_have_no_scratch(tmp_path):
    k = {n: v for n, v in _kernel_metadata(tmp_path).items() if n.startswith("tilted_")}
    for n in sorted(k):
        print(n, k[n])
    assert sorted(k) == ["tilted_group_composites_kernel<false>", "tilted_group_composites_kernel<true>",
                         "tilted_group_ingest_kernel"], sorted(k)
    for n, v in k.items():
        assert v["scratch"] == 0 and v["lds"] == 0, (n, v)
