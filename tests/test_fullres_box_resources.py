"""CPU: the box kernels (csrc/gcfr_fullres_box.hip) in the built library carry no private segment and no LDS.  The composite holds a
light's 48 taps, d[3][4], m[4] and the tap offsets per lane, and indexes the boxes in its argument block with the workgroup's face:
either could have become scratch.  Read from the code objects' notes, as tests/test_kernel_resources.py reads the march kernels'.
The VGPR counts are printed and recorded in DESIGN 4.14; no cap is set."""
import os

import pytest

from test_kernel_resources import LLVM, _kernel_metadata


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs the ROCm LLVM tools")
def test_the_box_kernels_have_no_scratch(tmp_path):
    k = {n: v for n, v in _kernel_metadata(tmp_path).items() if n.startswith(("fullres_composites_box_kernel<", "ingest_box_kernel"))}
    for n in sorted(k):
        print(n, k[n])
    assert sorted(k) == ["fullres_composites_box_kernel<false>", "fullres_composites_box_kernel<true>", "ingest_box_kernel"], sorted(k)
    for n, v in k.items():
        assert v["scratch"] == 0 and v["lds"] == 0, (n, v)
