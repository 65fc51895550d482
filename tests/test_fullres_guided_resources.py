"""CPU: the guided full-resolution kernels (csrc/gcfr_fullres_guided.hip) in the built library carry no private segment: a kernel
with scratch writes every resident wave's arena back to memory, and the vector path's 64 weights per lane are exactly what would
spill.  Read from the code objects' notes, as tests/test_kernel_resources.py reads the march kernels'.  The VGPR counts are printed
and recorded in DESIGN 4.13; no cap is set."""
import os

import pytest

from test_kernel_resources import LLVM, _kernel_metadata


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs the ROCm LLVM tools")
def test_the_guided_kernels_have_no_scratch(tmp_path):
    k = {n: v for n, v in _kernel_metadata(tmp_path).items() if n.startswith("fullres_composites_guided_kernel<")}
    for n in sorted(k):
        print(n, k[n])
    vector = {n: v for n, v in k.items() if n.endswith(", true>")}
    assert sorted(vector) == ["fullres_composites_guided_kernel<%d, true>" % s for s in (1, 2, 4, 8)], sorted(k)
    assert len(k) == 8
    for n, v in vector.items():
        assert v["scratch"] == 0 and v["lds"] == 0, (n, v)
