"""`MobileNet('shuffle5dw' / 'shuffle3dw')` on the MI355X: the pixel-shuffle kernels fd_dws_rows / fd_head_shuffle of the product library against the
fp64 restatement (whole network, and element-wise per pixel-shuffle layer: tests/shuffle_ref.py), and the models against the reference's own
outputs (tests/golden/shuffle*, tools/make_golden_shuffle.py)."""
import pytest
import torch

import shuffle_ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", shuffle_ref.SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("decoder", shuffle_ref.DECODERS)
def test_gpu_shuffle_forward_matches_restatement(decoder, shape):
    shuffle_ref.check_whole_network("hip", decoder, shape)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape", shuffle_ref.SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("decoder", shuffle_ref.DECODERS)
def test_gpu_shuffle_layers_elementwise(decoder, shape, dtype):
    shuffle_ref.check_layer_local("hip", decoder, shape, dtype)


@pytest.mark.parametrize("name", ["shuffle5dw_s10", "shuffle3dw_s11"])
def test_gpu_shuffle_matches_reference_output(name):
    """224 x 224, B = 2, through `model(x.cuda())`, in the spread norm max |y - y_ref| / (max y_ref - min y_ref).  fp32: 1e-3.  fp16 / bf16: four
    times the reference's own 16-bit storage drift in the same norm (shuffle.json: the reference module with every activation output rounded to the
    storage type) -- the engine rounds at different, and fewer, points than that hook model, hence the margin of four (as tests/test_gpu_deconv.py)."""
    m, x, y_ref, meta = shuffle_ref.golden_case(name)
    m = m.cuda()
    errs = {}
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        m.set_compute_dtype(dtype)
        with torch.no_grad():
            y = m(x.cuda()).cpu()
        assert y.shape == y_ref.shape
        errs[dtype] = shuffle_ref.spread_err(y.numpy(), y_ref.numpy())
    bounds = {torch.float32: 1e-3, torch.float16: 4 * meta["storage_drift"]["float16"]["spread_norm"],
              torch.bfloat16: 4 * meta["storage_drift"]["bfloat16"]["spread_norm"]}
    print(name, {str(k): (errs[k], bounds[k]) for k in errs})
    assert all(errs[k] < bounds[k] for k in errs), {str(k): (errs[k], bounds[k]) for k in errs}
