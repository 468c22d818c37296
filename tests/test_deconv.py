"""`MobileNet('deconv5dw' / 'deconv3dw')` (reference models.py:145-180: the DeConv decoder, depthwise form) on the CPU emulation of the
library: the polyphase transposed depthwise kernel fd_dwt_rows (FD_OP_DWT), its plan plumbing, the module surface, the deploy bundle and the
refusals.  The restatement and the layer-local bound live in tests/deconv_ref.py (shared with the GPU tier)."""
import ctypes
import os

import pytest
import torch

import deconv_ref
import harness
from oracle import inputs

REF = deconv_ref.REF


@pytest.mark.parametrize("shape", deconv_ref.SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("decoder", deconv_ref.DECODERS)
def test_emulated_deconv_forward_matches_restatement(decoder, shape):
    deconv_ref.check_whole_network("emu", decoder, shape)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape", deconv_ref.SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("decoder", deconv_ref.DECODERS)
def test_emulated_dwt_layers_elementwise(decoder, shape, dtype):
    deconv_ref.check_layer_local("emu", decoder, shape, dtype)


def test_deconv_module_surface():
    models = inputs.product_models()
    m = models.MobileNet("deconv5dw", (224, 224), pretrained=False)
    sd = m.state_dict()
    assert len(sd) == 228 and list(sd)[0] == "mobilenet.0.0.weight" and "decoder.convf.1.running_var" in sd
    assert sd["decoder.convt1.0.0.weight"].shape == (1024, 1, 5, 5) and sd["decoder.convt5.1.0.weight"].shape == (32, 64, 1, 1)
    assert isinstance(m.decoder, models.DeConv) and isinstance(m.decoder.convt3[0][0], torch.nn.ConvTranspose2d)
    assert models.MobileNet("deconv3dw", (224, 224), pretrained=False).state_dict()["decoder.convt2.0.0.weight"].shape == (512, 1, 3, 3)
    # He-normal init through weights_init (fan = k * k * in_channels for a transposed conv, reference models.py:43-47)
    assert abs(float(m.decoder.convt1[0][0].weight.detach().std()) - (2.0 / (25 * 1024)) ** 0.5) < 5e-4
    from fastdepth_hip import capi
    from fastdepth_hip.plan import layers_of
    ls = layers_of(m)
    assert [l.name for l in ls[27:]] == ["decoder.convt%d.%d" % (j, q) for j in range(1, 6) for q in (0, 1)] + ["decoder.convf.0"]
    d = [l.desc for l in ls]
    assert [(x.op, x.ksize, x.stride) for x in d[27:37:2]] == [(capi.FD_OP_DWT, 5, 2)] * 5 and [x.cin for x in d[27:37:2]] == [1024, 512, 256, 128, 64]
    assert all(x.upsample == 0 and x.skip == -1 and x.concat == 0 for x in d) and [x.src for x in d] == [-1] + list(range(37))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval()(torch.rand(1, 3, 224, 224))


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference checkout is not present")
@pytest.mark.parametrize("decoder", deconv_ref.DECODERS)
def test_seeded_constructor_and_pickle_match_reference(decoder, tmp_path):
    models = inputs.product_models()
    torch.manual_seed(17); ours = models.MobileNet(decoder, (224, 224), pretrained=False)
    with deconv_ref.reference_modules() as ref_models:
        torch.manual_seed(17); ref = ref_models.MobileNet(decoder, (224, 224), pretrained=False)
        assert type(ref) is not models.MobileNet
        path = str(tmp_path / "ckpt.pth.tar")
        torch.save({"epoch": 1, "model": ref}, path)
    a, b = ours.state_dict(), ref.state_dict()
    assert list(a) == list(b) and len(a) == 228
    assert all(a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) for k in a)
    loaded = torch.load(path, weights_only=False)["model"]      # unpickles into the product classes: models.MobileNet / models.DeConv
    assert type(loaded) is models.MobileNet and type(loaded.decoder) is models.DeConv
    assert all(torch.equal(v, b[k]) for k, v in loaded.state_dict().items())
    plan = harness.CPlan("emu", loaded.eval(), torch.rand(1, 3, 32, 32), keep=False)
    assert sum(s.startswith("dwt_rows<") for s in plan.info()) == 5
    plan.close()


def test_deconv_bundle_round_trip_is_bit_equal():
    m, x, _, _ = deconv_ref.case("deconv5dw", (2, 32, 32))
    x = x[:1].contiguous()                                      # (one image: two emulated forwards)
    plan = harness.CPlan("emu", m, x, keep=False)
    y = plan.forward(x)
    L = plan.lib
    n = L.fd_plan_export_bytes(plan.h)
    buf = (ctypes.c_ubyte * n)()
    harness.capi.check(L, L.fd_plan_export(plan.h, buf, n, None), "fd_plan_export")
    plan.close()
    h = ctypes.c_void_p()
    harness.capi.check(L, L.fd_plan_import(buf, n, 0, ctypes.byref(h)), "fd_plan_import")
    try:
        assert sum(L.fd_plan_kernel_info(h, i).decode().startswith("dwt_rows<k5") for i in range(L.fd_plan_num_kernels(h))) == 5
        nbytes = L.fd_plan_workspace_bytes(h)
        ws = torch.empty(nbytes + 256, dtype=torch.uint8)
        base = (ws.data_ptr() + 255) // 256 * 256
        harness.capi.check(L, L.fd_plan_bind_workspace(h, base, nbytes), "fd_plan_bind_workspace")
        harness.capi.check(L, L.fd_plan_import_weights(h, buf, n, None), "fd_plan_import_weights")
        y2 = torch.full_like(y, float("nan"))
        harness.capi.check(L, L.fd_forward(h, x.contiguous().data_ptr(), y2.data_ptr(), None), "fd_forward")
    finally:
        L.fd_plan_destroy(h)
    assert torch.equal(y, y2)


def test_deconv_plan_statistics():
    """k^2 / 4 multiply-adds per output, one read of the input map and one write of the (four times larger) output map."""
    m, x, _, _ = deconv_ref.case("deconv3dw", (2, 32, 32))
    plan = harness.CPlan("emu", m, x, keep=False)
    L, b, f, t = plan.lib, ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    i = 29                                                      # decoder.convt2.0: 512 channels, 2x2 -> 4x4
    harness.capi.check(L, L.fd_plan_layer_stats(plan.h, i, ctypes.byref(b), ctypes.byref(f)), "fd_plan_layer_stats")
    harness.capi.check(L, L.fd_plan_layer_traffic(plan.h, i, ctypes.byref(t)), "fd_plan_layer_traffic")
    sym = L.fd_plan_kernel_symbol(plan.h, i).decode()
    plan.close()
    assert f.value == 2.0 * 2 * 16 * 512 * 9 / 4
    assert b.value == t.value == (2 * 4 * 512 + 2 * 16 * 512) * 4 + 9 * 512 * 4 + 2 * 512 * 4
    assert sym == "fd_dwt_rows<float, 3, 1>"


def test_deconv_refusals():
    models = inputs.product_models()
    for name in ("deconv5", "deconv7dw"):
        with pytest.raises(NotImplementedError):
            models.MobileNet(name, (224, 224), pretrained=False)
    with pytest.raises(NotImplementedError):
        models.DeConv(5, False)
    from fastdepth_hip.plan import _units
    bn, act = torch.nn.BatchNorm2d(8), torch.nn.ReLU()
    _units(torch.nn.Sequential(torch.nn.ConvTranspose2d(8, 8, 5, 2, 2, 1, groups=8, bias=False), bn, act))      # the accepted form
    for bad in (torch.nn.ConvTranspose2d(8, 8, 5, 2, 2, 1, groups=8, bias=True), torch.nn.ConvTranspose2d(8, 8, 5, 2, 2, 1, groups=1, bias=False),
                torch.nn.ConvTranspose2d(8, 8, 5, 2, 2, 0, groups=8, bias=False), torch.nn.ConvTranspose2d(8, 8, 5, 2, 1, 1, groups=8, bias=False),
                torch.nn.ConvTranspose2d(8, 8, 3, 1, 1, 0, groups=8, bias=False), torch.nn.ConvTranspose2d(8, 8, 7, 2, 3, 1, groups=8, bias=False),
                torch.nn.ConvTranspose2d(8, 8, 3, 2, 2, 1, groups=8, bias=False, dilation=2)):
        with pytest.raises(harness.capi.FastDepthError, match="transposed conv"):
            _units(torch.nn.Sequential(bad, bn, act))


def test_train_plans_refuse_transposed_units():
    m, x, _, _ = deconv_ref.case("deconv5dw", (2, 32, 32))
    msg = r"layer 27: transposed depthwise units \(FD_OP_DWT\) run in inference plans only"
    with pytest.raises(harness.capi.FastDepthError, match=msg):
        harness.CTrainPlan("emu", m, x)
    from fastdepth_hip.train import TrainEngine
    import copy
    eng = TrainEngine(copy.deepcopy(m).train(), _library=harness.get_lib("emu"))
    with pytest.raises(harness.capi.FastDepthError, match=msg):
        eng.step(x, torch.rand(2, 1, 32, 32))
