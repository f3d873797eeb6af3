"""What a batch of das in double launched is what its decision said: one warm-up batch, one batch under launch_trace, and the traced
kernel list against das_f64_decide (csrc/das_f64_plan.hpp, through tests/host_emul) for the device's own CU count, with mic0_unit and
n_tr from das_f64_slots (csrc/geometry.hpp) on the same geometry.  Nothing numeric is asserted here: tests/test_das_gpu.py,
test_fused_bins_gpu.py, test_variants_gpu.py and test_node_shim_gpu.py hold the outputs."""
import pytest
import torch

from beamform_amd.capi import BF_DAS_F64, BF_INTERLEAVED, BF_PLANAR, Beamformer, launch_trace
from beamform_amd.params import make_params
from chain_plan_util import chain_kernels, params_plan
from das_f64_plan_util import das_f64_kernels, params_decide

pytestmark = pytest.mark.gpu

HOP = 512


@pytest.mark.parametrize("layout,M,F,path", [
    (BF_PLANAR, 8, 5, "frame_pair"),        # the headline's kernel; 5 frames end on a lone one
    (BF_PLANAR, 2, 1, "frame_pair"),        # the smallest shape the pair kernel accepts, a lone frame
    (BF_INTERLEAVED, 8, 5, "ring"),
    (BF_INTERLEAVED, 3, 5, "transpose"),    # interleaved_to_planar_kernel for the batch and for the carried hop
    (BF_INTERLEAVED, 1, 5, "mic_pair"),
    (BF_PLANAR, 1, 5, "chain"),
    (BF_PLANAR, 9, 5, "chain")], ids=lambda v: str(v))
def test_launched_kernels_are_the_decision(emul_lib, layout, M, F, path):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    p = make_params("das", n_mics=M, hop=HOP)
    bf = Beamformer(p, layout=layout, das_impl=BF_DAS_F64)
    x = torch.rand((1, M, F * HOP) if layout == BF_PLANAR else (1, F * HOP, M), device="cuda") - 0.5
    y = torch.empty((1, F * HOP), device="cuda")
    bf.process_device(x.data_ptr(), F, y.data_ptr(), 0)
    with launch_trace() as t:
        bf.process_device(x.data_ptr(), F, y.data_ptr(), 0)
    torch.cuda.synchronize()
    bf.close()
    d = params_decide(emul_lib, p, F, cus, layout=layout)
    assert d["path"] == path, d
    want = chain_kernels(params_plan(emul_lib, p, F, cus, layout=layout), 2 * HOP) if path == "chain" else das_f64_kernels(d)
    assert [k.replace("bf::", "") for k in t.kernels] == want, (t.kernels, d)
