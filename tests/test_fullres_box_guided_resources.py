"""CPU: the guided box kernels (csrc/gcfr_fullres_box_guided.hip) in the built library carry no private segment.  The vector path
holds 64 normalised weights and two lights' column windows (2 x 3 x 4 x 5 or 7 values) per lane beside d[3][4] and m[4], picks
every tap out of its window by a run-time offset, and indexes the boxes in its argument block with the workgroup's face: any of
them could have become scratch (a tap chosen by ADDRESS instead of by value does put the windows there).  Read from the code objects' notes, as
tests/test_fullres_box_resources.py reads the box kernels'.  LDS is reported (the kernels stage nothing: 0 is expected, a staged
version would be allowed); the VGPR counts are printed and recorded in DESIGN 4.15; no cap is set."""
import os

import pytest

from test_kernel_resources import LLVM, _kernel_metadata


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs the ROCm LLVM tools")
def test_the_guided_box_kernels_have_no_scratch(tmp_path):
    k = {n: v for n, v in _kernel_metadata(tmp_path).items() if n.startswith("fullres_composites_box_guided_kernel<")}
    for n in sorted(k):
        print(n, k[n])
    assert sorted(k) == ["fullres_composites_box_guided_kernel<false, 0>", "fullres_composites_box_guided_kernel<true, 1>",
                         "fullres_composites_box_guided_kernel<true, 3>"], sorted(k)
    for n, v in k.items():
        assert v["scratch"] == 0, (n, v)
