"""`MobileNet('nnconv5' / 'nnconv3')` (the dense NNConv decoder) on the MI355X through the product library: the implicit-GEMM dense convolution
fd_conv_gemm (FD_OP_CONV) against the fp64 restatement, element-wise against its own stored inputs, one tap at a time, against the reference's own
outputs (tests/golden/nnconv5_s14_*, nnconv3_s15_*: made by tools/make_golden_dense.py where the reference is present; read here as data), and
bit-for-bit run to run.  Shared infrastructure: tests/dense_ref.py."""
import numpy as np
import pytest
import torch

import dense_ref
import harness
from oracle import inputs

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = ["f32", "f16", "bf16"]


@pytest.mark.parametrize("shape", dense_ref.SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("decoder", dense_ref.DECODERS)
def test_dense_forward_matches_restatement(decoder, shape):
    dense_ref.check_whole_network("gpu", decoder, shape)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", dense_ref.SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("decoder", dense_ref.DECODERS)
def test_dense_layers_elementwise(decoder, shape, dtype):
    dense_ref.check_layer_local("gpu", decoder, shape, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_narrow_plan(dtype):
    dense_ref.check_narrow("gpu", dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_tap_at_a_time(dtype):
    dense_ref.check_one_tap("gpu", dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_tap_full_width_conv1(dtype):
    dense_ref.check_one_tap_conv1("gpu", dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("decoder", dense_ref.DECODERS)
def test_big_tile_split_k_elementwise(decoder, dtype):
    """The 128 x 128 tile instance with split K, which no layer of the small shapes selects: decoder.conv3 at (2, 224, 224), layer-local."""
    dense_ref.check_big_tile("gpu", decoder, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_timed_forward_of_a_split_k_layer(dtype):
    """fd_forward_timed on the narrow plan: conv_a runs split K (fd_conv_gemm + fd_conv_reduce under the layer's one event pair): every layer reports a
    positive device time, the output is fd_forward's, and a plain forward afterwards is unchanged (the thread's event slots were put back)."""
    plan, y = dense_ref.narrow_executed("gpu", dtype)
    assert "fd_conv_reduce" in plan.info()[1]
    x = dense_ref.narrow_x().cuda()
    y2, ms = plan.forward_timed(x)
    y3 = plan.forward(x)
    print("timed narrow plan %s: ms per layer %s" % (dtype, ["%.4f" % v for v in ms]))
    assert all(0.0 < v < 50.0 for v in ms), ms
    assert torch.equal(y2.cpu(), y) and torch.equal(y3.cpu(), y)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["nnconv5_s14", "nnconv3_s15"])
def test_dense_matches_reference_outputs(name, dtype):
    """Test 4: the reference module's own fp32 output for B = 2, 224 x 224, in the spread norm: fp32 < 1e-3; fp16 / bf16 < 4 x the reference's own
    16-bit storage drift (the deconv family's thresholds: a 16-bit plan rounds every stored activation once, as the drift run does)."""
    m, x, y_ref, meta = dense_ref.golden_case(name)
    m = m.cuda()
    m.set_compute_dtype(dtype)
    with torch.no_grad():
        y = m(x.cuda()).cpu()
    err = dense_ref.spread_err(y.numpy(), y_ref.numpy())
    limit = 1e-3 if dtype == torch.float32 else 4 * meta["storage_drift"][str(dtype).replace("torch.", "")]["spread_norm"]
    print("%s %s: spread error %.3g (limit %.3g)" % (name, dtype, err, limit))
    assert err < limit, (err, limit)


def test_train_mode_forward_refuses():
    m, x, _, _ = dense_ref.case("nnconv3", dense_ref.SHAPES[0])
    import copy
    m = copy.deepcopy(m).cuda().train()
    with pytest.raises(harness.capi.FastDepthError, match=r"dense convolution units \(FD_OP_CONV\) run in inference plans only"):
        m(x.cuda())


def test_dense_forward_is_bit_reproducible():
    """Test 7: two forwards of the same fp32 plan at B = 32, 224 x 224 give identical bits (conv1 and conv2 run split K), and so do two freshly
    created plans."""
    models = inputs.product_models()
    torch.manual_seed(5)
    m = harness.randomize_bn(models.MobileNet("nnconv5", (224, 224), pretrained=False), 6).eval()
    x = torch.rand(32, 3, 224, 224, generator=torch.Generator().manual_seed(7)).cuda()
    outs = []
    for _ in range(2):
        plan = harness.CPlan("gpu", m, x, keep=False)
        info = plan.info()
        outs += [harness.bits_of(plan.forward(x)), harness.bits_of(plan.forward(x))]
        plan.close()
    assert any("fd_conv_reduce" in s for s in info[27:29]), info[27:32]
    assert all(np.array_equal(outs[0], o) for o in outs[1:])
