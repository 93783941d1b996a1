"""GPU tier of EncoderConfig.hevc_transform_skip: k_hevc_inter with the transform-skip candidate and
k_hevc_bins with transform_skip_flag give the CPU encoder's access units, reconstruction and distortion
sums byte for byte, and the GPU stream decodes through the Python decoder to the GPU reconstruction."""
import numpy as np
import pytest

from .test_hevc_transform_skip import CASES, assert_decodes_to, cpu_streams, encode, make_cfg, stroke_frames  # noqa: F401


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_gpu_transform_skip_equals_cpu_and_decodes(gpu, cpu_streams, case):  # noqa: F811
    import torch

    from .gpu_util import pitched

    (w, h), qp, filt = case
    genc = gpu.GpuHevcEncoder(make_cfg(gpu, w, h, qp, filt, 1), torch.cuda.current_stream().cuda_stream)
    held = []  # the device copy of the frame being coded

    def put(y, uv):
        held[:] = [pitched(y, genc.pitch, genc.coded_height), pitched(uv, genc.pitch, genc.coded_height // 2, uv=True)]
        torch.cuda.synchronize()
        return held[0].data_ptr(), held[1].data_ptr()

    aus, recs, _, sse = encode(genc, stroke_frames(w, h), put)
    caus, crecs, skipped, csse = cpu_streams[case, 1]
    assert min(skipped[1:]) > 0, skipped  # the P pictures hold skipped TUs
    for t in range(3):
        assert aus[t] == caus[t], f"picture {t}: {len(aus[t])} bytes against the CPU encoder's {len(caus[t])}"
        assert np.array_equal(recs[t][0], crecs[t][0]) and np.array_equal(recs[t][1], crecs[t][1]), t
        assert sse[t] == csse[t], t
    assert_decodes_to(aus, recs)
