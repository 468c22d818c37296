"""`MobileNet('blconv5dw' / 'blconv3dw')` on the MI355X: the bilinear kernels fd_dwb_rows / fd_head_bilinear of the product library against the
fp64 restatement (whole network, and element-wise per bilinear layer: tests/bilinear_ref.py), and the models against the reference's own
outputs (tests/golden/blconv*, tools/make_golden_bilinear.py)."""
import pytest
import torch

import bilinear_ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", bilinear_ref.SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("decoder", bilinear_ref.DECODERS)
def test_gpu_bilinear_forward_matches_restatement(decoder, shape):
    bilinear_ref.check_whole_network("hip", decoder, shape)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape", bilinear_ref.SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("decoder", bilinear_ref.DECODERS)
def test_gpu_bilinear_layers_elementwise(decoder, shape, dtype):
    bilinear_ref.check_layer_local("hip", decoder, shape, dtype)


@pytest.mark.parametrize("name", ["blconv5dw_s12", "blconv3dw_s13"])
def test_gpu_bilinear_matches_reference_output(name):
    """224 x 224, B = 2, through `model(x.cuda())`, in the spread norm max |y - y_ref| / (max y_ref - min y_ref).  fp32: 1e-3.  fp16 / bf16: four
    times the reference's own 16-bit storage drift in the same norm (bilinear.json: the reference module with every activation output rounded to the
    storage type) -- the engine rounds at different, and fewer, points than that hook model, hence the margin of four (as tests/test_gpu_deconv.py)."""
    m, x, y_ref, meta = bilinear_ref.golden_case(name)
    m = m.cuda()
    errs = {}
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        m.set_compute_dtype(dtype)
        with torch.no_grad():
            y = m(x.cuda()).cpu()
        assert y.shape == y_ref.shape
        errs[dtype] = bilinear_ref.spread_err(y.numpy(), y_ref.numpy())
    bounds = {torch.float32: 1e-3, torch.float16: 4 * meta["storage_drift"]["float16"]["spread_norm"],
              torch.bfloat16: 4 * meta["storage_drift"]["bfloat16"]["spread_norm"]}
    print(name, {str(k): (errs[k], bounds[k]) for k in errs})
    assert all(errs[k] < bounds[k] for k in errs), {str(k): (errs[k], bounds[k]) for k in errs}
